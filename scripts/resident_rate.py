"""What does the resident route (-gpu_inflate -gpu_parse [-gpu_sam] on BGZF FASTQ: inflate, parse, pack, map and SAM text all in HBM) do to a files-in run?
The inputs of scripts/bgzf_rate.py (profiles/gpu_inflate/bgzf_rate_4m_pairs.json): 150 bp pairs as synth.write_fastq writes them, packed as bgzip packs them
(members of 0xff00 bytes of text) at levels 1 and 6, a 100 Mbp genome, batches of 1 M reads, the files in tmpfs.  Three legs, each without SAM and to SAM:
  host      the reader's pool of inflate threads, host parser, host formatter (every switch off)
  inflate   -gpu_inflate alone (one 8 MB stretch per launch, the text back over PCIe into the host's line splitter)
  resident  -gpu_inflate -gpu_parse, and -gpu_sam where a SAM file is written
reads/s of the better of two runs after a warm-up, mcx_files_route's word for each leg, and — from one more run with MCX_TIMING=1 — the front end's own stage
times.  All three legs run in the library as it is built: the first two are the code paths a run took before the route existed, in the same session — the yardstick.
The legs run one after the other, not in turns; all_seconds keeps every run, the warm-up first: look at it before trusting a difference.
--alternate N: instead, the host leg and the resident leg in turns (host, resident, host, ...), N rounds after a warm-up round, for each level without SAM
and to SAM: every run's seconds, the median and the range per leg — what says whether a difference is beyond the runs' own spread.
    python scripts/resident_rate.py [--pairs 4000000] [--alternate 7] [--json profiles/gpu_resident/resident_rate.json]"""
import argparse, json, os, shutil, statistics, subprocess, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def timing_lines(run):
    """the [mcx_map_files] lines the library writes to stderr during run() with MCX_TIMING=1"""
    os.environ["MCX_TIMING"] = "1"
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            run()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["MCX_TIMING"]
        f.seek(0)
        text = f.read().decode("utf-8", "replace")
    return [l[len("[mcx_map_files] "):] for l in text.split("\n") if l.startswith("[mcx_map_files] ") and not l.startswith("[mcx_map_files] mcx_map_batch_dev")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--alternate", type=int, default=0, help="rounds of host / resident in turns (0: the three legs one after the other)")
    ap.add_argument("--json", default=None, help="also write the result there")
    a = ap.parse_args()
    import torch
    import bench
    from mapcaller_amd import api, synth
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    reads = bench.make_reads(codes, lens, a.pairs, 150, seed=9, device=dev).reshape(2 * a.pairs, 150).cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_resident_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"pairs": a.pairs, "member_text_bytes": 0xff00, "batch_reads": a.batch, "host_cpus": int(api.lib().mcx_host_cpus()),
           "launch_bytes": int(os.environ.get("MCX_RESIDENT_LAUNCH_BYTES", 128 << 20))}
    legs = {"host": {}, "inflate": {"device_inflate": True}, "resident": {"device_inflate": True, "device_parse": True, "device_sam": True}}
    try:
        p1, p2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        synth.write_fastq(p1, reads, 0, 2); synth.write_fastq(p2, reads, 1, 2)
        out["text_bytes_per_file"] = os.path.getsize(p1)
        files = {}
        for level in (1, 6):
            files[level] = (os.path.join(tmp, f"l{level}_1.fq.gz"), os.path.join(tmp, f"l{level}_2.fq.gz"))
            for src, dst in zip((p1, p2), files[level]):
                subprocess.run([sys.executable, os.path.join(HERE, "bgzf_rate.py"), "--pack", src, dst, str(level)], check=True)
            out[f"file_bytes_level_{level}"] = os.path.getsize(files[level][0])
            print(f"packed level {level}", file=sys.stderr, flush=True)
        os.remove(p1); os.remove(p2)
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=a.batch)
        sam = os.path.join(tmp, "out.sam")
        for level in (1, 6) if a.alternate else ():
            f1, f2 = files[level]
            for to_sam in (False, True):
                secs = {"host": [], "resident": []}
                for k in range(a.alternate + 1):  # (the first round warms up)
                    for leg in secs:
                        mp.reset()
                        t0 = time.perf_counter()
                        st = mp.map_files(f1, f2, sam if to_sam else None, **legs[leg])
                        if k:
                            secs[leg].append(round(time.perf_counter() - t0, 3))
                res = {leg: {"seconds": s, "median": statistics.median(s), "min": min(s), "max": max(s), "reads_per_s_at_median": round(st["reads"] / statistics.median(s))} for leg, s in secs.items()}
                out[f"alternating_level_{level}_{'to_sam' if to_sam else 'no_sam'}"] = res
                print(f"level {level} {'to SAM' if to_sam else 'no SAM'} in turns: " + ", ".join(f"{leg} median {r['median']:.3f} s ({r['min']:.3f}-{r['max']:.3f})" for leg, r in res.items()), file=sys.stderr, flush=True)
        for level in () if a.alternate else (1, 6):
            f1, f2 = files[level]
            for to_sam in (False, True):
                for leg, kw in legs.items():
                    secs, st = [], None

                    def run():
                        nonlocal st
                        mp.reset()
                        t0 = time.perf_counter()
                        st = mp.map_files(f1, f2, sam if to_sam else None, **kw)
                        secs.append(time.perf_counter() - t0)
                    for _ in range(3):  # (a warm-up, then the better of two)
                        run()
                    dt = min(secs[1:])
                    res = {"reads": st["reads"], "seconds": round(dt, 3), "reads_per_s": round(st["reads"] / dt), "all_seconds": [round(s, 3) for s in secs], "route": list(mp.last_route())}
                    res["timing"] = timing_lines(run)
                    out[f"level_{level}_{'to_sam' if to_sam else 'no_sam'}_{leg}"] = res
                    print(f"level {level} {'to SAM' if to_sam else 'no SAM'} {leg}: {res['reads_per_s'] / 1e6:.2f} M reads/s ({dt:.3f} s) route {res['route']}", file=sys.stderr, flush=True)
        mp.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump(out, open(a.json, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
