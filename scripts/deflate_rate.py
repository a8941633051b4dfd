"""How fast does the device compress SAM text to BGZF blocks, and how small?  About 1 GB of SAM text — 150 bp synth pairs on a 100 Mbp genome, mapped once to a
plain SAM file with -gpu_sam — goes to HBM, and mcx_bgzf_deflate_dev runs on it alone:
  * GB/s of text by HIP events on the deflater's stream round the call's kernels (mcx_bgzf_deflate_last_ms), median of --repeats after two warm-ups;
  * compressed / text of the whole text, and — on --zlib_cuts cuts of 65 280 bytes spread evenly over it — of the device's blocks beside zlib level 1 and level 6
    on the same cuts (raw deflate streams, as a block holds one).
    python scripts/deflate_rate.py [--pairs 1400000] [--json profiles/bgzf/deflate_rate.json]"""
import argparse, json, os, shutil, statistics, struct, sys, tempfile, zlib
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
BLOCK = 65280


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_400_000)
    ap.add_argument("--text_bytes", type=int, default=1_000_000_000, help="how much of the SAM text is taken")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--zlib_cuts", type=int, default=400)
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
    tmp = tempfile.mkdtemp(prefix="mcx_deflate_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        p1, p2, sam = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq"), os.path.join(tmp, "out.sam")
        synth.write_fastq(p1, reads, 0, 2); synth.write_fastq(p2, reads, 1, 2)
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=1 << 20)
        st = mp.map_files(p1, p2, sam, device_sam=True)
        mp.close()
        text = np.fromfile(sam, dtype=np.uint8, count=a.text_bytes)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {"pairs": a.pairs, "reads_mapped_to_text": st["reads"], "text_bytes": int(text.size), "block_text_bytes": BLOCK}
    d_text = torch.from_numpy(text).to(dev)
    with api.Deflater(0) as d:
        bound = d.bound(text.size)
        d_out = torch.empty(bound, dtype=torch.uint8, device=dev)
        ms = []
        for k in range(a.repeats + 2):
            rc, n = d.deflate_dev(d_text, text.size, d_out)
            assert rc == 0
            if k >= 2:
                ms.append(d.last_ms())
    blob = d_out[:n].cpu().numpy().tobytes()
    med = statistics.median(ms)
    out.update({"blocks_bytes": n, "compressed_over_text": round(n / text.size, 4), "ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                "text_gb_per_s": round(text.size / med / 1e6, 3)})
    # the blocks' sizes, by BSIZE; the first and the last block checked against the text
    sizes, at = [], 0
    while at < len(blob):
        sizes.append(struct.unpack_from("<H", blob, at + 16)[0] + 1)
        at += sizes[-1]
    n_blocks = -(-text.size // BLOCK)
    assert len(sizes) == n_blocks and at == len(blob)
    assert zlib.decompress(blob[18:sizes[0] - 8], -15) == text[:BLOCK].tobytes()
    assert zlib.decompress(blob[at - sizes[-1] + 18:at - 8], -15) == text[(n_blocks - 1) * BLOCK:].tobytes()
    picks = sorted(set(int(i) for i in np.linspace(0, n_blocks - 1, min(a.zlib_cuts, n_blocks))))
    ours = sum(sizes[i] - 26 for i in picks)
    cut_bytes, z = 0, {1: 0, 6: 0}
    for i in picks:
        cut = text[i * BLOCK:(i + 1) * BLOCK].tobytes()
        cut_bytes += len(cut)
        for level in z:
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            z[level] += len(c.compress(cut) + c.flush())
    out["on_sampled_cuts"] = {"cuts": len(picks), "text_bytes": cut_bytes, "device_over_text": round(ours / cut_bytes, 4), "zlib1_over_text": round(z[1] / cut_bytes, 4),
                              "zlib6_over_text": round(z[6] / cut_bytes, 4), "device_over_zlib1": round(ours / z[1], 4)}
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
