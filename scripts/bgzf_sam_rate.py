"""What does -bgzf do to a files-to-SAM run?  --pairs 150 bp pairs as synth.write_fastq writes them (plain FASTQ in tmpfs), a 100 Mbp genome, batches of 1 M reads,
the SAM file in tmpfs as well.  Three legs, taken in turns (host, gpu_sam, bgzf, host, ...), --rounds rounds after a warm-up round:
  host      the host formatter (every switch off)
  gpu_sam   -gpu_sam: the text made in HBM, copied out and written as it is
  bgzf      -bgzf: the text compressed in HBM, the blocks copied out and written
Every run's seconds, the median and the range per leg, reads/s at the median, the bytes written, and — from one more run of each leg with MCX_TIMING=1 — the
front end's own lines.  --legs host,gpu_sam runs the first two alone: the form for a checkout from before the switch existed, the yardstick.
    python scripts/bgzf_sam_rate.py [--pairs 4000000] [--rounds 5] [--legs host,gpu_sam,bgzf] [--json profiles/bgzf/bgzf_sam_rate.json]"""
import argparse, json, os, shutil, statistics, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from resident_rate import timing_lines  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default="host,gpu_sam,bgzf")
    ap.add_argument("--json", default=None, help="also write the result there")
    a = ap.parse_args()
    import torch
    import bench
    from mapcaller_amd import api, synth
    kinds = {"host": {}, "gpu_sam": {"device_sam": True}, "bgzf": {"bgzf_sam": True}}
    legs = {k: kinds[k] for k in a.legs.split(",")}
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    reads = bench.make_reads(codes, lens, a.pairs, 150, seed=9, device=dev).reshape(2 * a.pairs, 150).cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_bgzf_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"pairs": a.pairs, "batch_reads": a.batch, "rounds": a.rounds, "host_cpus": int(api.lib().mcx_host_cpus())}
    try:
        p1, p2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        synth.write_fastq(p1, reads, 0, 2); synth.write_fastq(p2, reads, 1, 2)
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=a.batch)
        sam = {leg: os.path.join(tmp, "out.sam.gz" if leg == "bgzf" else "out.sam") for leg in legs}
        secs, written, reads_n = {leg: [] for leg in legs}, {}, 0
        for k in range(a.rounds + 1):  # (the first round warms up)
            for leg, kw in legs.items():
                mp.reset()
                t0 = time.perf_counter()
                st = mp.map_files(p1, p2, sam[leg], **kw)
                dt = time.perf_counter() - t0
                reads_n, written[leg] = st["reads"], os.path.getsize(sam[leg])
                if k:
                    secs[leg].append(round(dt, 3))
        for leg, kw in legs.items():
            s = secs[leg]
            res = {"seconds": s, "median": statistics.median(s), "min": min(s), "max": max(s), "reads": reads_n, "reads_per_s_at_median": round(reads_n / statistics.median(s)),
                   "bytes_written": written[leg], "route": None}

            def run():
                mp.reset()
                mp.map_files(p1, p2, sam[leg], **kw)
            res["timing"] = timing_lines(run)
            res["route"] = list(mp.last_route())
            out[leg] = res
            print(f"{leg}: median {res['median']:.3f} s ({res['min']:.3f}-{res['max']:.3f}), {res['reads_per_s_at_median'] / 1e6:.2f} M reads/s, {written[leg]} bytes written", file=sys.stderr, flush=True)
        mp.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump(out, open(a.json, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
