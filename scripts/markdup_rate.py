"""What does -markdup cost?  Two measurements, scripts/sort_rate.py's input for both.
  * The calls alone: --call-pairs 150 bp pairs mapped once from host arrays, their BAM records made in HBM (mcx_bam_format_dev), then mcx_bam_dup_units_dev on the
    records in read order, mcx_dup_resolve_dev on its units and mcx_bam_dup_mark_dev on the same records with the units' verdicts: ms per call by HIP events on the
    context's stream (mcx_markdup_last_ms), median of --repeats after two warm-ups.  The units kernel's lanes per unit are read once per process from
    MCX_DUP_LANES (16, 32, 64): run the script once per width with --pairs 0 (--json names the record).
  * File to file: --pairs 150 bp pairs as synth.write_fastq writes them (plain FASTQ in tmpfs), a 100 Mbp genome, batches of 1 M reads, the output in tmpfs.
    Two legs taken in turns (sort, markdup, sort, ...), --rounds rounds after a warm-up round: every run's seconds, the median and the range per leg, and — from
    one more run of each leg with MCX_TIMING=1 — the library's own lines; of the markdup: line the counts and where the time went.
    (scripts/sort_rate.py of the parent commit, run before and after on the same machine, gives the -bam -sort leg the one here is held against.)
    python scripts/markdup_rate.py [--pairs 4000000] [--rounds 5] [--call-pairs 500000] [--json profiles/markdup/markdup_rate.json]"""
import argparse, ctypes as C, json, os, re, shutil, statistics, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from resident_rate import timing_lines  # noqa: E402


def calls_alone(api, torch, ix, reads, n_pairs, repeats):
    """the three calls on one mapped batch's records in HBM, in read order"""
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
    assert L.mcx_bam_format_dev(mp._h, C.byref(di), d_recs.data_ptr(), nb.value, d_off.data_ptr(), C.byref(nb), None) == 0, L.mcx_last_error()
    d_units = torch.zeros(24 * n_pairs, dtype=torch.uint8, device="cuda")
    d_dup = torch.zeros(n_pairs, dtype=torch.uint8, device="cuda")
    ms, n_units = [], C.c_uint64()
    for k in range(repeats + 2):
        torch.cuda.synchronize()
        assert L.mcx_bam_dup_units_dev(mp._h, d_recs.data_ptr(), nb.value, d_off.data_ptr(), n, 1, d_units.data_ptr(), C.byref(n_units)) == 0, L.mcx_last_error()
        assert L.mcx_dup_resolve_dev(mp._h, d_units.data_ptr(), n_units.value, d_dup.data_ptr()) == 0, L.mcx_last_error()
        d_rec_dup = d_dup.repeat_interleave(2).contiguous()  # (one record a read: both mates take the unit's byte; a fragment's unplaced mate is not told apart here)
        torch.cuda.synchronize()
        assert L.mcx_bam_dup_mark_dev(mp._h, d_recs.data_ptr(), nb.value, d_off.data_ptr(), n, d_rec_dup.data_ptr()) == 0, L.mcx_last_error()
        if k >= 2:
            ms.append(mp.markdup_last_ms())
    med = [statistics.median(x[i] for x in ms) for i in range(3)]
    units = d_units.cpu().numpy().view(api.DUP_UNIT_DTYPE)
    out = {"reads": n, "bytes": nb.value, "units": int(n_units.value), "pair_units": int((units["kind"] & 3 == 2).sum()), "fragment_units": int((units["kind"] & 3 == 1).sum()),
           "duplicates": int(d_dup.sum().item()), "lanes": int(os.environ.get("MCX_DUP_LANES", "16")), "ms_units_resolve_mark": [round(v, 3) for v in med],
           "units_gb_per_s": round(nb.value / 1e6 / max(med[0], 1e-6), 1), "resolve_bytes_per_unit_per_ms": None}
    print(f"markdup alone ({out['lanes']} lanes a unit): {nb.value} bytes, {n} reads in {out['units']} units ({out['pair_units']} pairs, {out['duplicates']} duplicates); units / resolve / mark "
          f"{med[0]:.3f} / {med[1]:.3f} / {med[2]:.3f} ms, units {out['units_gb_per_s']} GB/s of records", file=sys.stderr, flush=True)
    out.pop("resolve_bytes_per_unit_per_ms")
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
    legs = {"sort": {"bam": True, "sort": True}, "markdup": {"bam": True, "sort": True, "markdup": True}}
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    n_pairs = max(a.pairs, a.call_pairs)
    reads = bench.make_reads(codes, lens, n_pairs, 150, seed=9, device=dev).reshape(2 * n_pairs, 150).cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_markdup_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"pairs": a.pairs, "batch_reads": a.batch, "rounds": a.rounds, "host_cpus": int(api.lib().mcx_host_cpus())}
    try:
        if a.call_pairs:
            out["call"] = calls_alone(api, torch, ix, reads, a.call_pairs, a.repeats)
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
            out["markdup_stats"] = mp.markdup_stats()
            for leg, kw in legs.items():
                s = secs[leg]
                res = {"seconds": s, "median": statistics.median(s), "min": min(s), "max": max(s), "reads": reads_n, "reads_per_s_at_median": round(reads_n / statistics.median(s)),
                       "bytes_written": written[leg]}

                def run():
                    mp.reset()
                    mp.map_files(p1, p2, path[leg], **kw)
                res["timing"] = [l for l in timing_lines(run) if l.startswith(("sort:", "markdup:", "bgzf:", "wall seconds:"))]
                for l in res["timing"]:
                    m = re.match(r"sort: .*the merge ([\d.]+) s: read ([\d.]+), copy in ([\d.]+), inflate ([\d.]+), sort ([\d.]+), deflate \+ copy out ([\d.]+)", l)
                    if m:
                        res["merge"] = dict(zip(("merge_s", "read_s", "copy_in_s", "inflate_s", "sort_s", "deflate_out_s"), map(float, m.groups())))
                res["route"] = list(mp.last_route())
                out[leg] = res
                print(f"{leg}: median {res['median']:.3f} s ({res['min']:.3f}-{res['max']:.3f}), {res['reads_per_s_at_median'] / 1e6:.2f} M reads/s, {written[leg]} bytes written; "
                      f"{res.get('merge', '')} {[l for l in res['timing'] if l.startswith('markdup:')]}", file=sys.stderr, flush=True)
            mp.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump(out, open(a.json, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
