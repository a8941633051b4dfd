"""What does -md cost?  Three measurements, in the manner of scripts/bam_rate.py.
  * The call alone: --call-pairs 150 bp pairs mapped once from host arrays and put into HBM with their records and CIGAR pool, and mcx_md_dev run on them: ms per
    kernel by HIP events on the context's stream (mcx_md_last_ms) and GB/s over the bytes it must touch — SEQ, a quarter byte of genome a base, the records, the
    CIGAR words, the pool it writes —, median of --repeats after two warm-ups; mcx_sam_format_dev and mcx_bam_format_dev on the same input beside it, without
    the pool and with it.
  * File to file: --pairs 150 bp pairs as synth.write_fastq writes them (plain FASTQ in tmpfs), a 100 Mbp genome, batches of 1 M reads, the output in tmpfs as
    well.  Four legs taken in turns (bam, bam + md, sorted, sorted + md; sorted is -sort -markdup -index), --rounds rounds after a warm-up round: every run's
    seconds, the median and the range per leg, reads/s at the median, the bytes written.
  * --default-only: the legs without -md alone (bam, gpu_sam) with the md5 of what they write — run at this commit and at the one before it, the two lines say
    whether the default path moved (the script then uses nothing the commit before lacks).
    python scripts/md_rate.py [--pairs 4000000] [--rounds 5] [--call-pairs 500000] [--default-only] [--json profiles/md/md_rate.json]"""
import argparse, ctypes as C, hashlib, json, os, shutil, statistics, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def call_alone(api, torch, ix, reads, n_pairs, repeats):
    """mcx_md_dev and the two formatters on one mapped batch in HBM"""
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
    out = {"reads": n, "mapped": int((aln["chr"] >= 0).sum())}
    # the strings
    nb = C.c_uint64()
    d_off = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    L.mcx_md_dev(mp._h, C.byref(di), None, 0, d_off.data_ptr(), C.byref(nb))
    d_md = torch.empty(nb.value + 16, dtype=torch.uint8, device="cuda")
    ms = []
    for k in range(repeats + 2):
        assert L.mcx_md_dev(mp._h, C.byref(di), d_md.data_ptr(), nb.value, d_off.data_ptr(), C.byref(nb)) == 0, L.mcx_last_error()
        if k >= 2:
            ms.append(list(mp.md_last_ms()))
    med = [statistics.median(x[i] for x in ms) for i in range(3)]
    words = int(aln["n_cigar"].clip(0).sum())
    # (both passes read SEQ, the genome's bits, the records and the words; the write pass adds the pool; the scan's lengths and offsets are 20 bytes a line)
    touched = 2 * (n * 150 + n * 150 // 4 + n * 64 + words * 4) + nb.value + 20 * n
    out["md"] = {"bytes": nb.value, "bytes_per_read": round(nb.value / n, 2), "ms_len_scan_write": [round(v, 3) for v in med], "bytes_touched": touched, "gb_per_s": round(touched / 1e6 / sum(med), 1)}
    print(f"md alone: {nb.value} bytes ({nb.value / n:.2f} a read), len / scan / write {med[0]:.3f} / {med[1]:.3f} / {med[2]:.3f} ms, {out['md']['gb_per_s']} GB/s of {touched} bytes touched", file=sys.stderr, flush=True)
    # the formatters without the pool and with it
    for with_md in (False, True):
        di.md, di.md_off = (d_md.data_ptr(), d_off.data_ptr()) if with_md else (None, None)
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
            key = kind + ("_md" if with_md else "")
            out[key] = {"bytes": nb.value, "bytes_per_read": round(nb.value / n, 1), "ms_len_scan_write": [round(v, 3) for v in med], "gb_per_s": round(nb.value / 1e6 / sum(med), 1)}
            print(f"{key} alone: {nb.value} bytes ({nb.value / n:.1f} a read), len / scan / write {med[0]:.3f} / {med[1]:.3f} / {med[2]:.3f} ms, {out[key]['gb_per_s']} GB/s", file=sys.stderr, flush=True)
    mp.close()
    return out


def md5_of(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--call-pairs", type=int, default=500_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--default-only", action="store_true", help="the legs without -md alone, with the md5 of their files")
    ap.add_argument("--json", default=None, help="also write the result there")
    a = ap.parse_args()
    import torch
    import bench
    from mapcaller_amd import api, synth
    sorted_kw = {"bam": True, "sort": True, "markdup": True, "index": True}
    if a.default_only:
        legs = {"bam": {"bam": True}, "gpu_sam": {"device_sam": True}}
    else:
        legs = {"bam": {"bam": True}, "bam_md": {"bam": True, "md": True}, "sorted": sorted_kw, "sorted_md": dict(sorted_kw, md=True)}
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    reads = bench.make_reads(codes, lens, a.pairs, 150, seed=9, device=dev).reshape(2 * a.pairs, 150).cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_md_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"pairs": a.pairs, "batch_reads": a.batch, "rounds": a.rounds, "host_cpus": int(api.lib().mcx_host_cpus())}
    try:
        if a.call_pairs and not a.default_only:
            out["call"] = call_alone(api, torch, ix, reads, min(a.call_pairs, a.pairs), a.repeats)
        p1, p2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        synth.write_fastq(p1, reads, 0, 2); synth.write_fastq(p2, reads, 1, 2)
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=a.batch)
        path = {leg: os.path.join(tmp, leg + (".sam" if leg == "gpu_sam" else ".bam")) for leg in legs}
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
        for leg in legs:
            s = secs[leg]
            res = {"seconds": s, "median": statistics.median(s), "min": min(s), "max": max(s), "reads": reads_n, "reads_per_s_at_median": round(reads_n / statistics.median(s)),
                   "bytes_written": written[leg]}
            if a.default_only:
                res["md5"] = md5_of(path[leg])
            out[leg] = res
            print(f"{leg}: median {res['median']:.3f} s ({res['min']:.3f}-{res['max']:.3f}), {res['reads_per_s_at_median'] / 1e6:.2f} M reads/s, {written[leg]} bytes written {res.get('md5', '')}", file=sys.stderr, flush=True)
        mp.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump(out, open(a.json, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
