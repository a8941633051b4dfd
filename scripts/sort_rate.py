"""What does -sort cost?  Two measurements.
  * The operation alone: --call-pairs 150 bp pairs mapped once from host arrays, their BAM records made in HBM by mcx_bam_format_dev (scripts/bam_rate.py's
    input), and mcx_bam_sort_dev run on them: ms per stage by HIP events on the context's stream (mcx_bam_sort_last_ms: index, sort, place, gather), median of
    --repeats after two warm-ups, GB/s of records over the four together and over the gather alone, k_bam_write's figure from the same process beside it.
    The gather's shape (lanes a record) is fixed when the library first sorts: run the script once per shape with MCX_SORT_LANES=16 | 32 | 64.
  * File to file: --pairs 150 bp pairs as synth.write_fastq writes them (plain FASTQ in tmpfs), a 100 Mbp genome, batches of 1 M reads, the output in tmpfs as
    well.  Two legs taken in turns (bam, sort, bam, ...), --rounds rounds after a warm-up round: every run's seconds, the median and the range per leg, and —
    from one more run of each leg with MCX_TIMING=1 — the library's own lines; of the sort: line the runs' and the merge's seconds and the bytes read back.
    (scripts/bam_rate.py of the parent commit, run before and after on the same machine, gives the -bam leg this one is held against.)
    python scripts/sort_rate.py [--pairs 4000000] [--rounds 5] [--call-pairs 500000] [--json profiles/sort/sort_rate.json]"""
import argparse, ctypes as C, json, os, re, shutil, statistics, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from resident_rate import timing_lines  # noqa: E402


def call_alone(api, torch, ix, reads, n_pairs, repeats):
    """mcx_bam_sort_dev on one mapped batch's records in HBM"""
    import numpy as np
    n = 2 * n_pairs
    mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=(n + 199) // 200 * 200)
    bases = np.ascontiguousarray(reads[:n].numpy()).reshape(-1)
    off = (np.arange(n + 1, dtype=np.uint64) * 150).astype(np.uint32)
    aln, cigars = mp.map_batch(bases, off, True)[:2]
    aln, pool = api._pool_of(aln, cigars)
    names = b"".join(b"read%d" % (r // 2) for r in range(n))
    name_off = np.zeros(n + 1, dtype=np.uint32)
    name_off[1:] = np.cumsum([len(b"read%d" % (r // 2)) for r in range(n)])
    qual = np.full(n * 150, 73, dtype=np.uint8)
    host = {"bases": bases, "off": off, "qual": qual, "names": np.frombuffer(names + b"\0", dtype=np.uint8), "name_off": name_off, "aln": aln.view(np.uint8), "cigar": pool}
    t = {k: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda() for k, v in host.items()}
    di = api.SamIn()
    for k in host:
        setattr(di, k, t[k].data_ptr())
    di.n_reads, di.paired = n, 1
    L = api.lib()
    nb = C.c_uint64()
    L.mcx_bam_format_dev(mp._h, C.byref(di), None, 0, None, C.byref(nb), None)
    d_recs = torch.empty(nb.value + 16, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    write_ms = []
    for k in range(repeats + 2):
        assert L.mcx_bam_format_dev(mp._h, C.byref(di), d_recs.data_ptr(), nb.value, d_off.data_ptr(), C.byref(nb), None) == 0, L.mcx_last_error()
        if k >= 2:
            write_ms.append(mp.bam_last_ms()[2])
    d_out = torch.empty(nb.value + 16, dtype=torch.uint8, device="cuda")
    ms, n_rec = [], C.c_uint64()
    for k in range(repeats + 2):
        assert L.mcx_bam_sort_dev(mp._h, d_recs.data_ptr(), nb.value, d_off.data_ptr(), n, d_out.data_ptr(), nb.value, None, None, C.byref(n_rec)) == 0, L.mcx_last_error()
        if k >= 2:
            ms.append(mp.bam_sort_last_ms())
    med = [statistics.median(x[i] for x in ms) for i in range(4)]
    w = statistics.median(write_ms)
    out = {"reads": n, "records": n_rec.value, "bytes": nb.value, "lanes_a_record": int(os.environ.get("MCX_SORT_LANES") or 16), "ms_index_sort_place_gather": [round(v, 3) for v in med],
           "gb_per_s": round(nb.value / 1e6 / sum(med), 1), "gather_gb_per_s": round(nb.value / 1e6 / med[3], 1), "k_bam_write_ms": round(w, 3), "k_bam_write_gb_per_s": round(nb.value / 1e6 / w, 1)}
    print(f"sort alone ({out['lanes_a_record']} lanes a record): {nb.value} bytes, {n_rec.value} records, index / sort / place / gather {med[0]:.3f} / {med[1]:.3f} / {med[2]:.3f} / {med[3]:.3f} ms, "
          f"{out['gb_per_s']} GB/s (the gather alone {out['gather_gb_per_s']}); k_bam_write {w:.3f} ms, {out['k_bam_write_gb_per_s']} GB/s", file=sys.stderr, flush=True)
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
    legs = {"bam": {"bam": True}, "sort": {"bam": True, "sort": True}}
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    n_pairs = max(a.pairs, a.call_pairs)
    reads = bench.make_reads(codes, lens, n_pairs, 150, seed=9, device=dev).reshape(2 * n_pairs, 150).cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_sort_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"pairs": a.pairs, "batch_reads": a.batch, "rounds": a.rounds, "host_cpus": int(api.lib().mcx_host_cpus())}
    try:
        if a.call_pairs:
            out["call"] = call_alone(api, torch, ix, reads, a.call_pairs, a.repeats)
        if a.pairs and a.rounds:
            reads = reads[:2 * a.pairs]
            p1, p2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
            synth.write_fastq(p1, reads, 0, 2); synth.write_fastq(p2, reads, 1, 2)
            mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=a.batch)
            path = {leg: os.path.join(tmp, f"out_{leg}.bam") for leg in legs}
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
                    m = re.match(r"sort: (\d+) runs \(([\d.]+) s of the mapper's time\), (\d+) chunks of (\d+) slices \((\d+) start inside a block\); the merge ([\d.]+) s: read ([\d.]+), copy in ([\d.]+), "
                                 r"inflate ([\d.]+), sort ([\d.]+), deflate \+ copy out ([\d.]+); (\d+) bytes read back, (\d+) of them twice", l)
                    if m:
                        g = m.groups()
                        res["sort"] = {"runs": int(g[0]), "run_making_s": float(g[1]), "chunks": int(g[2]), "slices": int(g[3]), "slices_inside_a_block": int(g[4]), "merge_s": float(g[5]),
                                       "merge_read_s": float(g[6]), "merge_copy_in_s": float(g[7]), "merge_inflate_s": float(g[8]), "merge_sort_s": float(g[9]), "merge_deflate_out_s": float(g[10]),
                                       "bytes_read_back": int(g[11]), "bytes_read_twice": int(g[12])}
                res["route"] = list(mp.last_route())
                out[leg] = res
                print(f"{leg}: median {res['median']:.3f} s ({res['min']:.3f}-{res['max']:.3f}), {res['reads_per_s_at_median'] / 1e6:.2f} M reads/s, {written[leg]} bytes written; {res.get('sort', '')}",
                      file=sys.stderr, flush=True)
            mp.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump(out, open(a.json, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
