"""What do -rg and -mc cost, and did the formatters' default path move?  Two measurements, in the manner of scripts/md_rate.py.
  * The calls alone: --reads records of 150 bp pairs made here (no mapper: the formatters read arrays; 3 % of the reads unmapped, a fifth of the CIGARs with a
    clip or an indel), put into HBM once, and mcx_sam_format_dev / mcx_bam_format_dev run on them: ms per kernel by HIP events on the context's stream
    (mcx_sam_last_ms / mcx_bam_last_ms), median of --repeats after two warm-ups, with the spread.  Legs: the tags off, -rg, -mc, both.
    --default-only runs the tags-off leg alone through the entry points the commit before this one has as well: run in turns from this tree and from a
    checkout of that commit (--tree), the two rows say whether the default path moved.
  * File to file (--pairs > 0): 150 bp pairs as synth.write_fastq writes them (plain FASTQ in tmpfs), a 100 Mbp genome, batches of 1 M reads, the output in tmpfs
    as well.  Four legs taken in turns (bam, bam + tags, sorted, sorted + tags; sorted is -sort -markdup -index), --rounds rounds after a warm-up round.
    python scripts/tags_rate.py [--reads 1000000] [--repeats 5] [--default-only] [--tree DIR] [--pairs 0] [--rounds 5] [--json FILE]"""
import argparse, ctypes as C, json, os, shutil, statistics, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
RG = r"@RG\tID:lane1\tSM:na12878\tLB:lib1\tPL:ILLUMINA"


def make_batch(api, np, n):
    """host arrays of n reads (pairs) as mcx_sam_in takes them"""
    rng = np.random.default_rng(20261021)
    aln = np.zeros(n, dtype=api.ALN_DTYPE)
    kinds = [[(150 << 4) | 0], [(20 << 4) | 4, (130 << 4) | 0], [(70 << 4) | 0, (2 << 4) | 2, (80 << 4) | 0], [(60 << 4) | 0, (3 << 4) | 1, (87 << 4) | 0]]
    kind = rng.choice(4, n, p=[0.8, 0.1, 0.05, 0.05])
    mapped = rng.random(n) >= 0.03
    n_cigar = np.where(mapped, np.array([len(k) for k in kinds])[kind], 0)
    cigar_off = np.concatenate([[0], np.cumsum(n_cigar)[:-1]])
    pool = np.zeros(int(n_cigar.sum()) + 1, dtype=np.uint32)
    for k, words in enumerate(kinds):
        rows = np.nonzero(mapped & (kind == k))[0]
        for j, w in enumerate(words):
            pool[cigar_off[rows] + j] = w
    mate_mapped = mapped.reshape(-1, 2)[:, ::-1].reshape(-1)
    aln["chr"] = np.where(mapped, rng.integers(0, 3, n), -1)
    aln["pos"] = np.where(mapped, rng.integers(1, 80000, n), 0)
    aln["mapq"] = np.where(mapped, rng.integers(0, 61, n), 0)
    second = np.arange(n) & 1
    aln["fwd"] = rng.integers(0, 2, n)
    aln["flag"] = 1 | np.where(second == 1, 0x80, 0x40) | np.where(mapped, 0, 4) | np.where(mate_mapped, 0, 8) | np.where(mapped & mate_mapped, 2, 0)
    aln["has_mate"] = mapped & mate_mapped
    aln["mate_pos"] = np.where(aln["has_mate"] == 1, aln["pos"] + 200, 0)
    aln["tlen"] = np.where(aln["has_mate"] == 1, np.where(second == 1, -350, 350), 0)
    aln["nm"], aln["as"], aln["xs"] = rng.integers(0, 5, n), rng.integers(100, 151, n), rng.integers(0, 100, n)
    aln["n_cigar"], aln["cigar_off"] = n_cigar, cigar_off
    names = [b"read%d" % (r // 2) for r in range(n)]
    name_off = np.zeros(n + 1, dtype=np.uint32)
    name_off[1:] = np.cumsum([len(x) for x in names])
    return {"bases": np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n * 150)], "off": (np.arange(n + 1, dtype=np.uint64) * 150).astype(np.uint32),
            "qual": rng.integers(35, 74, n * 150).astype(np.uint8), "names": np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8), "name_off": name_off,
            "aln": aln.view(np.uint8), "cigar": pool}


def calls_alone(api, torch, np, n, repeats, default_only):
    ix = api.Index(os.path.join(HERE, "..", "tests", "golden", "mc", "idx"), device=0)  # (three contigs: the formatters take the names alone)
    mp = api.Mapper(ix, alg="nw", max_read_len=256, max_batch_reads=2000)
    host = make_batch(api, np, n)
    t = {k: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda() for k, v in host.items()}
    di = api.SamIn()
    for k in host:
        setattr(di, k, t[k].data_ptr())
    di.n_reads, di.paired = n, 1
    L = api.lib()
    out = {"reads": n}
    legs = {"off": None} if default_only else {"off": None, "rg": (True, 0), "mc": (False, 1), "both": (True, 1)}
    d_id = torch.from_numpy(np.frombuffer(b"lane1", dtype=np.uint8).copy()).cuda()
    for leg, what in legs.items():
        tg = None
        if what is not None:
            tg = api.SamTags()
            tg.rg, tg.rg_len, tg.mate_tags = (d_id.data_ptr() if what[0] else None), (5 if what[0] else 0), what[1]
        for kind, last in (("sam", L.mcx_sam_last_ms), ("bam", L.mcx_bam_last_ms)):
            if tg is None:  # the entry points of before
                call = (lambda *a: L.mcx_bam_format_dev(*a, None)) if kind == "bam" else L.mcx_sam_format_dev
            else:
                f = L.mcx_bam_format_tags_dev if kind == "bam" else L.mcx_sam_format_tags_dev
                call = (lambda h, d, *a, f=f, tg=tg, kind=kind: f(h, d, C.byref(tg), *a, *((None,) if kind == "bam" else ())))
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
            total = [sum(x) for x in ms]
            med = [statistics.median(x[i] for x in ms) for i in range(3)]
            key = f"{kind}_{leg}"
            out[key] = {"bytes": nb.value, "ms_len_scan_write": [round(v, 3) for v in med], "ms_total_median": round(statistics.median(total), 3),
                        "ms_total_min": round(min(total), 3), "ms_total_max": round(max(total), 3)}
            print(f"{key}: {nb.value} bytes, len / scan / write {med[0]:.3f} / {med[1]:.3f} / {med[2]:.3f} ms, total {out[key]['ms_total_median']:.3f} ({min(total):.3f}-{max(total):.3f})", file=sys.stderr, flush=True)
    mp.close(); ix.close()
    return out


def file_to_file(api, torch, pairs, batch, rounds):
    import bench
    from mapcaller_amd import synth
    sorted_kw = {"bam": True, "sort": True, "markdup": True, "index": True}
    tags = {"read_group": RG, "mate_tags": True}
    legs = {"bam": {"bam": True}, "bam_tags": dict(tags, bam=True), "sorted": sorted_kw, "sorted_tags": dict(sorted_kw, **tags)}
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    reads = bench.make_reads(codes, lens, pairs, 150, seed=9, device=dev).reshape(2 * pairs, 150).cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_tags_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"pairs": pairs, "batch_reads": batch, "rounds": rounds}
    try:
        p1, p2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        synth.write_fastq(p1, reads, 0, 2); synth.write_fastq(p2, reads, 1, 2)
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=batch)
        secs, written, reads_n = {leg: [] for leg in legs}, {}, 0
        for k in range(rounds + 1):  # (the first round warms up)
            for leg, kw in legs.items():
                mp.reset()
                path = os.path.join(tmp, leg + ".bam")
                t0 = time.perf_counter()
                st = mp.map_files(p1, p2, path, **kw)
                dt = time.perf_counter() - t0
                reads_n, written[leg] = st["reads"], os.path.getsize(path)
                if k:
                    secs[leg].append(round(dt, 3))
        for leg in legs:
            s = secs[leg]
            out[leg] = {"seconds": s, "median": statistics.median(s), "min": min(s), "max": max(s), "reads": reads_n, "reads_per_s_at_median": round(reads_n / statistics.median(s)), "bytes_written": written[leg]}
            print(f"{leg}: median {out[leg]['median']:.3f} s ({min(s):.3f}-{max(s):.3f}), {out[leg]['reads_per_s_at_median'] / 1e6:.2f} M reads/s, {written[leg]} bytes written", file=sys.stderr, flush=True)
        mp.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000, help="records of the calls-alone measurement (0: skip it)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--default-only", action="store_true", help="the tags-off leg alone, through the entry points of the commit before")
    ap.add_argument("--tree", default=os.path.join(HERE, ".."), help="the checkout whose mapcaller_amd is measured (default: this one)")
    ap.add_argument("--pairs", type=int, default=0, help="pairs of the file-to-file measurement (0: skip it; the figures of DESIGN.md: 4000000)")
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the result there")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import torch
    from mapcaller_amd import api
    out = {"tree": os.path.abspath(a.tree)}
    if a.reads:
        out["calls"] = calls_alone(api, torch, np, a.reads // 2 * 2, a.repeats, a.default_only)
    if a.pairs and not a.default_only:
        out["files"] = file_to_file(api, torch, a.pairs, a.batch, a.rounds)
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
