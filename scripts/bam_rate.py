"""What does -bam cost and save against -bgzf SAM?  Two measurements.
  * The call alone: --call-pairs 150 bp pairs mapped once from host arrays, their reads, names, qualities, records and CIGAR pool put into HBM, and
    mcx_bam_format_dev run on them: ms per kernel by HIP events on the context's stream (mcx_bam_last_ms) and GB/s of records out over the three together, median
    of --repeats after two warm-ups; mcx_sam_format_dev on the same input beside it.
  * File to file: --pairs 150 bp pairs as synth.write_fastq writes them (plain FASTQ in tmpfs), a 100 Mbp genome, batches of 1 M reads, the output in tmpfs as
    well.  Two legs taken in turns (bgzf, bam, bgzf, ...), --rounds rounds after a warm-up round: every run's seconds, the median and the range per leg, reads/s at
    the median, the bytes written, and — from one more run of each leg with MCX_TIMING=1 — the bytes that entered the deflater and left it.
    python scripts/bam_rate.py [--pairs 4000000] [--rounds 5] [--call-pairs 500000] [--json profiles/bam/bam_rate.json]"""
import argparse, ctypes as C, json, os, re, shutil, statistics, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from resident_rate import timing_lines  # noqa: E402


def call_alone(api, torch, ix, reads, n_pairs, repeats):
    """the two formatters on one mapped batch in HBM"""
    n = 2 * n_pairs
    mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=(n + 199) // 200 * 200)
    import numpy as np
    bases = np.ascontiguousarray(reads[:n].numpy()).reshape(-1)
    off = (np.arange(n + 1, dtype=np.uint64) * 150).astype(np.uint32)
    aln, cigars = mp.map_batch(bases, off, True)[:2]
    aln, pool = api._pool_of(aln, cigars)
    names = b"".join(b"read%d" % (r // 2) for r in range(n))
    name_off = np.zeros(n + 1, dtype=np.uint32)
    name_off[1:] = np.cumsum([len(b"read%d" % (r // 2)) for r in range(n)])
    qual = np.full(n * 150, 73, dtype=np.uint8)  # ('I' throughout, as synth.write_fastq writes it)
    host = {"bases": bases, "off": off, "qual": qual, "names": np.frombuffer(names + b"\0", dtype=np.uint8), "name_off": name_off, "aln": aln.view(np.uint8), "cigar": pool}
    t = {k: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda() for k, v in host.items()}
    di = api.SamIn()
    for k in host:
        setattr(di, k, t[k].data_ptr())
    di.n_reads, di.paired = n, 1
    L = api.lib()
    out = {"reads": n}
    for kind, call, last in (("bam", lambda *a: L.mcx_bam_format_dev(*a, None), L.mcx_bam_last_ms), ("sam", L.mcx_sam_format_dev, L.mcx_sam_last_ms)):
        nb = C.c_uint64()
        call(mp._h, C.byref(di), None, 0, None, C.byref(nb))
        d_out = torch.empty(nb.value + 16, dtype=torch.uint8, device="cuda")
        ms = []
        for k in range(repeats + 2):
            assert call(mp._h, C.byref(di), d_out.data_ptr(), nb.value, None, C.byref(nb)) == 0, L.mcx_last_error()
            m = (C.c_float * 3)()
            last(mp._h, m)
            if k >= 2:
                ms.append([float(v) for v in m])
        med = [statistics.median(x[i] for x in ms) for i in range(3)]
        out[kind] = {"bytes": nb.value, "bytes_per_read": round(nb.value / n, 1), "ms_len_scan_write": [round(v, 3) for v in med], "gb_per_s": round(nb.value / 1e6 / sum(med), 1)}
        print(f"{kind} alone: {nb.value} bytes ({nb.value / n:.1f} a read), len / scan / write {med[0]:.3f} / {med[1]:.3f} / {med[2]:.3f} ms, {out[kind]['gb_per_s']} GB/s", file=sys.stderr, flush=True)
    mp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--call-pairs", type=int, default=500_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None, help="also write the result there")
    a = ap.parse_args()
    import torch
    import bench
    from mapcaller_amd import api, synth
    legs = {"bgzf": {"bgzf_sam": True}, "bam": {"bam": True}}
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    reads = bench.make_reads(codes, lens, a.pairs, 150, seed=9, device=dev).reshape(2 * a.pairs, 150).cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_bam_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"pairs": a.pairs, "batch_reads": a.batch, "rounds": a.rounds, "host_cpus": int(api.lib().mcx_host_cpus())}
    try:
        if a.call_pairs:
            out["call"] = call_alone(api, torch, ix, reads, min(a.call_pairs, a.pairs), a.repeats)
        p1, p2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        synth.write_fastq(p1, reads, 0, 2); synth.write_fastq(p2, reads, 1, 2)
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=a.batch)
        path = {"bgzf": os.path.join(tmp, "out.sam.gz"), "bam": os.path.join(tmp, "out.bam")}
        secs, written, reads_n = {leg: [] for leg in legs}, {}, 0
        for k in range(a.rounds + 1):  # (the first round warms up)
            for leg, kw in legs.items():
                mp.reset()
                t0 = time.perf_counter()
                st = mp.map_files(p1, p2, path[leg], **kw)
                dt = time.perf_counter() - t0
                reads_n, written[leg] = st["reads"], os.path.getsize(path[leg])
                if k:
                    secs[leg].append(round(dt, 3))
        for leg, kw in legs.items():
            s = secs[leg]
            res = {"seconds": s, "median": statistics.median(s), "min": min(s), "max": max(s), "reads": reads_n, "reads_per_s_at_median": round(reads_n / statistics.median(s)),
                   "bytes_written": written[leg]}

            def run():
                mp.reset()
                mp.map_files(p1, p2, path[leg], **kw)
            res["timing"] = timing_lines(run)
            for l in res["timing"]:
                m = re.match(r"bgzf: (\d+) bytes of text -> (\d+) bytes of blocks", l)
                if m:
                    res["deflater_in"], res["deflater_out"] = int(m.group(1)), int(m.group(2))
                    res["compressed_over_uncompressed"] = round(int(m.group(2)) / int(m.group(1)), 4)
            res["route"] = list(mp.last_route())
            out[leg] = res
            print(f"{leg}: median {res['median']:.3f} s ({res['min']:.3f}-{res['max']:.3f}), {res['reads_per_s_at_median'] / 1e6:.2f} M reads/s, {written[leg]} bytes written, "
                  f"deflater {res.get('deflater_in')} -> {res.get('deflater_out')}", file=sys.stderr, flush=True)
        mp.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump(out, open(a.json, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
