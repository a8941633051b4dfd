"""How fast is FASTA text parsed on the device, and what does -gpu_parse do to a files-in run on plain FASTA?  150 bp single reads, about 1 GB of text, in two
layouts: single-line records, and the bases folded to 60 columns.
  (a) the call alone — mcx_fastq_parse_dev under MCX_READS_FASTA on the file's text already in HBM, every group of outputs asked for (records, bases + NUL
      qualities, names, 2-bit rows + odd bytes), by HIP events on the parser's stream (mcx_fastq_last_ms: first kernel to last, the waits in the middle
      included), median of --repeats after two warm-ups: ms and GB/s of text — the plain rule on both layouts, the GZ rule on the single-line one;
  (b) the file in tmpfs -> records only (no SAM), and -> SAM, with and without device_parse, batches of --batch reads: the two legs taken in turns (host,
      device, host, ...), --rounds rounds after a warm-up round, every run's seconds, the median and the range per leg, reads/s at the median.  The leg
      without the switch is the yardstick: the sequential host reader (one Parser thread per file) on the same file.
    python scripts/fasta_rate.py [--reads 6000000] [--rounds 5] [--json profiles/gpu_parse/fasta_rate.json]"""
import argparse, json, os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def write_folded(path, bases, width, prefix="sim"):
    """synth.write_fasta_reads with the bases folded to `width` columns"""
    import numpy as np
    arr = bases.cpu().numpy()
    n, rlen = arr.shape
    digits = max(1, len(str(max(n - 1, 0))))
    head = b">" + prefix.encode() + b"_"
    n_lines = (rlen + width - 1) // width
    out = np.empty((n, len(head) + digits + 1 + rlen + n_lines), dtype=np.uint8)
    c = 0
    out[:, c:c + len(head)] = np.frombuffer(head, dtype=np.uint8); c += len(head)
    idx = np.arange(n, dtype=np.int64)
    for d in range(digits):
        out[:, c + digits - 1 - d] = 48 + (idx // (10 ** d)) % 10
    c += digits
    out[:, c] = 10; c += 1
    for at in range(0, rlen, width):
        w = min(width, rlen - at)
        out[:, c:c + w] = arr[:, at:at + w]; c += w
        out[:, c] = 10; c += 1
    out.tofile(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=6_000_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of host / device in turns after the warm-up round (at least 5)")
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--json", default=None, help="also write the result there")
    a = ap.parse_args()
    a.rounds = max(a.rounds, 5)
    import numpy as np
    import torch
    import bench
    from mapcaller_amd import api, synth
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    reads = bench.make_reads(codes, lens, (a.reads + 1) // 2, 150, seed=9, device=dev).reshape(-1, 150)[:a.reads].cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_fasta_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"reads": a.reads, "batch_reads": a.batch, "host_cpus": int(api.lib().mcx_host_cpus())}
    try:
        paths = {"single_line": os.path.join(tmp, "one.fa"), "60_columns": os.path.join(tmp, "folded.fa")}
        synth.write_fasta_reads(paths["single_line"], reads, 0, 1)
        write_folded(paths["60_columns"], reads, 60)
        # ---- (a) the call alone
        for layout, path in paths.items():
            text = open(path, "rb").read()
            total, n = len(text), a.reads
            assert total < (1 << 32), "the text must stay under 4 GiB: fewer --reads"
            d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
            o = {"recs": [torch.empty(n * 24, dtype=torch.uint8, device=dev)],
                 "bases": torch.empty(total + 32, dtype=torch.uint8, device=dev), "qual": torch.empty(total + 32, dtype=torch.uint8, device=dev),
                 "off": torch.empty(n + 1, dtype=torch.int32, device=dev), "names": torch.empty(total, dtype=torch.uint8, device=dev),
                 "name_off": torch.empty(n + 1, dtype=torch.int32, device=dev), "rows": torch.empty((n, 16), dtype=torch.int32, device=dev),
                 "len": torch.empty(n, dtype=torch.int32, device=dev), "odd": torch.empty(1 << 20, dtype=torch.int64, device=dev)}
            for rule in (api.FASTQ_RULE_PLAIN, api.FASTQ_RULE_GZ) if layout == "single_line" else (api.FASTQ_RULE_PLAIN,):
                with api.FastqParser(0, max_text_bytes=total, max_records=n) as p:
                    p.set_format(api.READS_FASTA)
                    p.set_rule(rule)
                    ms = []
                    for k in range(a.repeats + 2):
                        rc, info = p.parse_dev([d_text], n, 256, final=True, **o)
                        assert rc == 0 and info["n_reads"] == n and info["n_bases"] == 150 * n, info
                        if k >= 2:
                            ms.append(p.last_ms())
                assert o["bases"][:150].cpu().numpy().tobytes() == reads[0].numpy().tobytes(), "the first read's bases"
                med = statistics.median(ms)
                out[f"parse_dev_{layout}_{'gz' if rule else 'plain'}_rule"] = {"text_bytes": total, "reads": n, "ms_median": round(med, 3), "ms_min": round(min(ms), 3),
                                                                               "text_gb_per_s": round(total / med / 1e6, 3), "reads_per_s": round(n / med * 1e3)}
                print(layout, "rule", rule, out[f"parse_dev_{layout}_{'gz' if rule else 'plain'}_rule"], file=sys.stderr, flush=True)
            del d_text, o, text
        # ---- (b) the file in, with and without device_parse, in turns
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=a.batch)
        sam = os.path.join(tmp, "out.sam")
        for layout, path in paths.items():
            for to_sam in (False, True):
                secs, routes = {"host": [], "device": []}, {}
                for k in range(a.rounds + 1):  # (the first round warms up)
                    for leg in secs:
                        mp.reset()
                        t0 = time.perf_counter()
                        st = mp.map_files(path, None, sam if to_sam else None, device_parse=leg == "device")
                        if k:
                            secs[leg].append(round(time.perf_counter() - t0, 3))
                        routes[leg] = list(mp.last_route())
                        assert st["reads"] == a.reads, st
                res = {leg: {"seconds": s, "median": statistics.median(s), "min": min(s), "max": max(s), "reads_per_s_at_median": round(a.reads / statistics.median(s)), "route": routes[leg]}
                       for leg, s in secs.items()}
                out[f"files_{layout}_{'to_sam' if to_sam else 'no_sam'}"] = res
                print(f"{layout} {'to SAM' if to_sam else 'no SAM'} in turns: " + ", ".join(f"{leg} median {r['median']:.3f} s ({r['min']:.3f}-{r['max']:.3f}) route {r['route']}" for leg, r in res.items()),
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
