"""What does -index cost?  Two measurements, scripts/sort_rate.py's input for both.
  * The operation alone: --call-pairs 150 bp pairs mapped once from host arrays, their BAM records made in HBM (mcx_bam_format_dev) and sorted there
    (mcx_bam_sort_dev), then mcx_bam_index_dev on the sorted records against an invented block table (blocks of 65280 bytes of text, 20 000 bytes each in the
    file) and a fresh table of windows: ms per stage by HIP events on the context's stream (mcx_bam_index_last_ms: records, stretches, windows), median of
    --repeats after two warm-ups, and the stretches the records make.
  * File to file: --pairs 150 bp pairs as synth.write_fastq writes them (plain FASTQ in tmpfs), a 100 Mbp genome, batches of 1 M reads, the output in tmpfs.
    Two legs taken in turns (sort, index, sort, ...), --rounds rounds after a warm-up round: every run's seconds, the median and the range per leg, and — from one
    more run of each leg with MCX_TIMING=1 — the library's own lines; of the index: line the stretches, bins, entries, bytes and seconds.
    (scripts/sort_rate.py of the parent commit, run before and after on the same machine, gives the -bam -sort leg the one here is held against.)
    python scripts/index_rate.py [--pairs 4000000] [--rounds 5] [--call-pairs 500000] [--json profiles/index/index_rate.json]"""
import argparse, ctypes as C, json, os, re, shutil, statistics, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from resident_rate import timing_lines  # noqa: E402


def call_alone(api, torch, ix, lens_of_contigs, reads, n_pairs, repeats):
    """mcx_bam_index_dev on one mapped batch's sorted records in HBM"""
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
    nb, n_rec = C.c_uint64(), C.c_uint64()
    L.mcx_bam_format_dev(mp._h, C.byref(di), None, 0, None, C.byref(nb), None)
    d_recs = torch.empty(nb.value + 16, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    assert L.mcx_bam_format_dev(mp._h, C.byref(di), d_recs.data_ptr(), nb.value, d_off.data_ptr(), C.byref(nb), None) == 0, L.mcx_last_error()
    d_sorted = torch.empty(nb.value + 16, dtype=torch.uint8, device="cuda")
    d_lens = torch.zeros(nb.value // 36 + 1, dtype=torch.int32, device="cuda")
    assert L.mcx_bam_sort_dev(mp._h, d_recs.data_ptr(), nb.value, d_off.data_ptr(), n, d_sorted.data_ptr(), nb.value, None, d_lens.data_ptr(), C.byref(n_rec)) == 0, L.mcx_last_error()
    rec_off = torch.zeros(n_rec.value + 1, dtype=torch.int64, device="cuda")
    rec_off[1:] = torch.cumsum(d_lens[:n_rec.value].to(torch.int64), 0)
    block = 65280
    n_blocks = (nb.value + block - 1) // block
    coff = (torch.arange(n_blocks + 1, dtype=torch.int64, device="cuda") * 20000).contiguous()
    lin_base = np.cumsum([0] + [(int(v) >> 14) + 2 for v in lens_of_contigs]).astype(np.int64)
    d_base = torch.from_numpy(lin_base).cuda()
    d_runs = torch.zeros(24 * n_rec.value, dtype=torch.uint8, device="cuda")
    ms, n_runs = [], C.c_uint64()
    for k in range(repeats + 2):
        d_lin = torch.full((int(lin_base[-1]),), -1, dtype=torch.int64, device="cuda")  # (all-ones: a fresh table every time, as a file's first chunk finds it)
        torch.cuda.synchronize()
        assert L.mcx_bam_index_dev(mp._h, d_sorted.data_ptr(), nb.value, rec_off.data_ptr(), n_rec.value, block, coff.data_ptr(), n_blocks, d_lin.data_ptr(), d_base.data_ptr(), len(lens_of_contigs),
                                   d_runs.data_ptr(), n_rec.value, C.byref(n_runs)) == 0, L.mcx_last_error()
        if k >= 2:
            ms.append(mp.bam_index_last_ms())
    med = [statistics.median(x[i] for x in ms) for i in range(3)]
    touched = int((d_lin != -1).sum().item())
    out = {"reads": n, "records": n_rec.value, "bytes": nb.value, "stretches": n_runs.value, "stretches_per_record": round(n_runs.value / max(1, n_rec.value), 4), "windows_touched": touched,
           "ms_records_stretches_windows": [round(v, 3) for v in med], "gb_per_s": round(nb.value / 1e6 / sum(med), 1)}
    print(f"index alone: {nb.value} bytes, {n_rec.value} records in {n_runs.value} stretches, {touched} windows; records / stretches / windows {med[0]:.3f} / {med[1]:.3f} / {med[2]:.3f} ms, "
          f"{out['gb_per_s']} GB/s of records", file=sys.stderr, flush=True)
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
    legs = {"sort": {"bam": True, "sort": True}, "index": {"bam": True, "sort": True, "index": True}}
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    n_pairs = max(a.pairs, a.call_pairs)
    reads = bench.make_reads(codes, lens, n_pairs, 150, seed=9, device=dev).reshape(2 * n_pairs, 150).cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_index_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"pairs": a.pairs, "batch_reads": a.batch, "rounds": a.rounds, "host_cpus": int(api.lib().mcx_host_cpus())}
    try:
        if a.call_pairs:
            out["call"] = call_alone(api, torch, ix, lens, reads, a.call_pairs, a.repeats)
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
            out["same_bam_bytes"] = open(path["sort"], "rb").read() == open(path["index"], "rb").read()
            for leg, kw in legs.items():
                s = secs[leg]
                res = {"seconds": s, "median": statistics.median(s), "min": min(s), "max": max(s), "reads": reads_n, "reads_per_s_at_median": round(reads_n / statistics.median(s)),
                       "bytes_written": written[leg]}

                def run():
                    mp.reset()
                    mp.map_files(p1, p2, path[leg], **kw)
                res["timing"] = [l for l in timing_lines(run) if l.startswith(("sort:", "index:", "bgzf:", "wall seconds:"))]
                for l in res["timing"]:
                    m = re.match(r"index: (\d+) records in (\d+) stretches, (\d+) bins and (\d+) linear entries written, (\d+) bytes; ([\d.]+) s of the merge \(on the device: records ([\d.]+), "
                                 r"stretches ([\d.]+), windows ([\d.]+) ms\)", l)
                    if m:
                        g = m.groups()
                        res["index"] = {"records": int(g[0]), "stretches": int(g[1]), "stretches_per_record": round(int(g[1]) / max(1, int(g[0])), 4), "bins": int(g[2]), "intervals": int(g[3]),
                                        "bai_bytes": int(g[4]), "seconds": float(g[5]), "device_ms_records_stretches_windows": [float(g[6]), float(g[7]), float(g[8])]}
                    m = re.match(r"sort: .*the merge ([\d.]+) s: read ([\d.]+), copy in ([\d.]+), inflate ([\d.]+), sort ([\d.]+), deflate \+ copy out ([\d.]+)", l)
                    if m:
                        res["merge"] = dict(zip(("merge_s", "read_s", "copy_in_s", "inflate_s", "sort_s", "deflate_out_s"), map(float, m.groups())))
                res["route"] = list(mp.last_route())
                out[leg] = res
                print(f"{leg}: median {res['median']:.3f} s ({res['min']:.3f}-{res['max']:.3f}), {res['reads_per_s_at_median'] / 1e6:.2f} M reads/s, {written[leg]} bytes written; "
                      f"{res.get('merge', '')} {res.get('index', '')}", file=sys.stderr, flush=True)
            mp.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump(out, open(a.json, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
