"""How fast is FASTQ text parsed on the device, and what does -gpu_parse do to a files-in run?  150 bp pairs as synth.write_fastq writes them:
  (a) the call alone — mcx_fastq_parse_dev on the two files' text already in HBM, every group of outputs asked for (records, bases + qualities, names,
      2-bit rows + odd bytes), by HIP events on the parser's stream (mcx_fastq_last_ms: first kernel to last, the one wait in the middle included),
      median of --repeats after two warm-ups, for --pairs and a quarter of them: ms and GB/s of text;
  (b) the two files in tmpfs -> records only (no SAM), and -> SAM, with and without device_parse, batches of 2 M reads, the better of two runs after a
      warm-up: reads/s.  The run without the switch is the yardstick: the host reader on the same files (MCX_TIMING=1 in the environment makes every
      run print its parse + pack busy seconds to stderr).
    python scripts/fastq_rate.py [--pairs 4000000] [--json profiles/gpu_parse/fastq_rate_4m.json]"""
import argparse, json, os, shutil, statistics, sys, tempfile, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--batch", type=int, default=2_000_000)
    ap.add_argument("--json", default=None, help="also write the result there")
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from mapcaller_amd import api, synth
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    reads = bench.make_reads(codes, lens, a.pairs, 150, seed=9, device=dev).reshape(2 * a.pairs, 150).cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_fastq_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"pairs": a.pairs, "batch_reads": a.batch}
    try:
        p1, p2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        synth.write_fastq(p1, reads, 0, 2); synth.write_fastq(p2, reads, 1, 2)
        # ---- (a) the call alone
        raw = [open(p, "rb").read() for p in (p1, p2)]
        for pairs in (a.pairs // 4, a.pairs):
            texts = []
            for r in raw:  # the first `pairs` records of each file
                end = len(r) if pairs >= a.pairs else _nth_newline(np.frombuffer(r, dtype=np.uint8), 4 * pairs)
                texts.append(r[:end])
            total = sum(map(len, texts))
            assert total < (1 << 32), "the two texts together must stay under 4 GiB: fewer --pairs"
            d_text = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).to(dev) for t in texts]
            n = 2 * pairs
            o = {"recs": [torch.empty(pairs * 24, dtype=torch.uint8, device=dev) for _ in range(2)],
                 "bases": torch.empty(total + 32, dtype=torch.uint8, device=dev), "qual": torch.empty(total + 32, dtype=torch.uint8, device=dev),
                 "off": torch.empty(n + 1, dtype=torch.int32, device=dev), "names": torch.empty(total, dtype=torch.uint8, device=dev),
                 "name_off": torch.empty(n + 1, dtype=torch.int32, device=dev), "rows": torch.empty((n, 16), dtype=torch.int32, device=dev),
                 "len": torch.empty(n, dtype=torch.int32, device=dev), "odd": torch.empty(1 << 20, dtype=torch.int64, device=dev)}
            with api.FastqParser(0, max_text_bytes=len(texts[0]), max_records=pairs) as p:
                ms = []
                for k in range(a.repeats + 2):
                    rc, info = p.parse_dev(d_text, pairs, 256, final=True, **o)
                    assert rc == 0 and info["n_reads"] == n and info["stop"] == [0, 0], info
                    if k >= 2:
                        ms.append(p.last_ms())
            first = o["bases"][:150].cpu().numpy().tobytes()
            assert first == texts[0].split(b"\n", 2)[1], "the first read's bases"
            med = statistics.median(ms)
            out[f"parse_dev_{pairs}_pairs"] = {"text_bytes": total, "reads": n, "n_bases": info["n_bases"], "ms_median": round(med, 3), "ms_min": round(min(ms), 3),
                                              "text_gb_per_s": round(total / med / 1e6, 3), "reads_per_s": round(n / med * 1e3)}
            del d_text, o
        del raw
        # ---- (b) files in, with and without device_parse
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=a.batch)
        sam = os.path.join(tmp, "out.sam")
        for to_sam in (False, True):
            for dev_parse in (False, True):
                secs, st = [], None
                for k in range(3):  # (a warm-up, then the better of two)
                    mp.reset()
                    t0 = time.perf_counter()
                    st = mp.map_files(p1, p2, sam if to_sam else None, device_parse=dev_parse)
                    secs.append(time.perf_counter() - t0)
                dt = min(secs[1:])
                out[f"files_{'to_sam' if to_sam else 'no_sam'}_{'device' if dev_parse else 'host'}_parse"] = {
                    "reads": st["reads"], "seconds": round(dt, 3), "reads_per_s": round(st["reads"] / dt)}
        mp.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump(out, open(a.json, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _nth_newline(arr, n):
    """offset just behind the n-th newline of a byte array"""
    import numpy as np
    pos = np.flatnonzero(arr == 10)
    return int(pos[n - 1]) + 1


if __name__ == "__main__":
    main()
