"""How fast are BAM records found and unpacked on the device, and what does BAM input cost a files-in run against its BGZF FASTQ twin?  150 bp pairs as synth
makes them, written as uBAM (flags 0x4D / 0x8D, quality 40) and as FASTQ:
  (a) the parse call alone — mcx_fastq_parse_dev under MCX_READS_BAM with set_mates(1) on --reads records' bytes already in HBM, every group of outputs asked
      for, against mcx_fastq_parse_dev under the GZ rule on the FASTQ twin of the same reads (the two files' text): ms by HIP events on the parser's stream
      (mcx_fastq_last_ms) and GB/s of input bytes, and the BAM call's search, walk, join and unpack (mcx_bam_reads_last_ms); medians of five, the two legs
      taken in turns after a warm-up each;
  (b) --pairs pairs file to file on the resident route, without SAM and with -bam: the uBAM file against the BGZF FASTQ twin (-gpu_inflate -gpu_parse), medians
      of five, the legs in turns after a warm-up each: seconds and reads/s.
The inflater bounds this route at 20-28 GB/s of text (README): the record finder is in order when the parse call is a minor share of a launch's inflate time —
"parse_share_of_inflate" says which, for the slower and the faster bound.
    python scripts/bam_in_rate.py [--reads 1000000] [--pairs 4000000] [--json profiles/bam_in/bam_in_rate.json]"""
import argparse, json, os, shutil, statistics, struct, sys, tempfile, time, zlib
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

NAME_DIGITS = 9


def ubam_records(arr, flags):
    """the reads of arr (n x rlen ASCII letters) as unaligned BAM records, one matrix: read k is named sim_<k // len(flags)> and carries flags[k % len(flags)]"""
    import numpy as np
    n, rlen = arr.shape
    l_name = 4 + NAME_DIGITS + 1
    size = 36 + l_name + (rlen + 1) // 2 + rlen
    out = np.zeros((n, size), dtype=np.uint8)
    fixed = struct.pack("<iiiBBHHHiiii", size - 4, -1, -1, l_name, 0, 4680, 0, 0, rlen, -1, -1, 0)
    out[:, :36] = np.frombuffer(fixed, dtype=np.uint8)
    idx = np.arange(n, dtype=np.int64)
    out[:, 18] = np.asarray(flags, dtype=np.uint8)[idx % len(flags)]
    out[:, 36:40] = np.frombuffer(b"sim_", dtype=np.uint8)
    for d in range(NAME_DIGITS):
        out[:, 40 + NAME_DIGITS - 1 - d] = 48 + ((idx // len(flags)) // (10 ** d)) % 10
    nib = np.full(256, 15, dtype=np.uint8)
    for c, v in zip(b"ACGT", (1, 2, 4, 8)):
        nib[c] = v
    codes = nib[arr]
    if rlen % 2:
        codes = np.concatenate([codes, np.zeros((n, 1), dtype=np.uint8)], axis=1)
    at = 36 + l_name
    out[:, at:at + (rlen + 1) // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    out[:, at + (rlen + 1) // 2:] = 40
    return out


def write_bgzf(path, data, block=0xff00, level=1):
    eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    view = memoryview(data)
    with open(path, "wb") as f:
        for i in range(0, len(view), block):
            chunk = view[i:i + block]
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            comp = c.compress(chunk) + c.flush()
            f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
        f.write(eof)


def in_turns(legs, repeats=5):
    """legs: name -> callable returning a dict of numbers; a warm-up each, then `repeats` rounds with the legs in turns: name -> dict of medians"""
    for f in legs.values():
        f()
    got = {k: [] for k in legs}
    for _ in range(repeats):
        for k, f in legs.items():
            got[k].append(f())
    return {k: {m: round(statistics.median(r[m] for r in v), 4) for m in v[0]} for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000, help="records of the parse call alone (an even number)")
    ap.add_argument("--pairs", type=int, default=4_000_000, help="pairs of the file-to-file runs (0: leave them out)")
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
    n_pairs = max(a.pairs, a.reads // 2)
    reads = bench.make_reads(codes, lens, n_pairs, 150, seed=9, device=dev).reshape(2 * n_pairs, 150).cpu()
    out = {"reads": a.reads, "pairs": a.pairs, "batch_reads": a.batch}
    tmp = tempfile.mkdtemp(prefix="mcx_bam_in_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        # ---- (a) the call alone
        n = a.reads // 2 * 2
        recs = ubam_records(reads[:n].numpy(), (0x4D, 0x8D))
        d_bam = torch.from_numpy(recs.reshape(-1)).to(dev)
        twin = [torch.from_numpy(synth._records(reads[:n], k, 2, "sim", True).reshape(-1)).to(dev) for k in (0, 1)]
        bam_bytes, twin_bytes = d_bam.numel(), sum(t.numel() for t in twin)
        o = {"bases": torch.empty(n * 150 + 32, dtype=torch.uint8, device=dev), "qual": torch.empty(n * 150 + 32, dtype=torch.uint8, device=dev),
             "off": torch.empty(n + 1, dtype=torch.int32, device=dev), "names": torch.empty(n * 16, dtype=torch.uint8, device=dev),
             "name_off": torch.empty(n + 1, dtype=torch.int32, device=dev), "rows": torch.empty((n, 16), dtype=torch.int32, device=dev),
             "len": torch.empty(n, dtype=torch.int32, device=dev), "odd": torch.empty(1 << 20, dtype=torch.int64, device=dev)}
        recs_out = [torch.empty(n * 24, dtype=torch.uint8, device=dev), torch.empty(n // 2 * 24, dtype=torch.uint8, device=dev)]
        with api.FastqParser(0) as pb, api.FastqParser(0) as pf:
            pb.set_reads(api.READS_BAM); pb.set_mates(True)
            pf.set_rule(api.FASTQ_RULE_GZ)

            def bam_leg():
                rc, info = pb.parse_dev([d_bam], n, 256, final=True, recs=recs_out[:1], **o)
                assert rc == 0 and info["n_reads"] == n and info["stop"][0] == api.FASTQ_MORE, info
                s, w, j, u = pb.bam_last_ms()
                return {"ms": pb.last_ms(), "search_ms": s, "walk_ms": w, "join_ms": j, "unpack_ms": u}

            def twin_leg():
                rc, info = pf.parse_dev(twin, n // 2, 256, final=True, recs=[recs_out[1], recs_out[0]], **o)
                assert rc == 0 and info["n_reads"] == n, info
                return {"ms": pf.last_ms()}
            med = in_turns({"bam": bam_leg, "fastq_twin_gz_rule": twin_leg})
            last = pb.bam_last()
        pb_ms = med["bam"]["ms"]
        med["bam"].update(input_bytes=bam_bytes, gb_per_s=round(bam_bytes / pb_ms / 1e6, 3), chunks=last["chunks"], chunks_off_chain=last["off_chain"])
        med["fastq_twin_gz_rule"].update(input_bytes=twin_bytes, gb_per_s=round(twin_bytes / med["fastq_twin_gz_rule"]["ms"] / 1e6, 3))
        # a launch's inflate time for these bytes at the README's 20 and 28 GB/s of text
        med["parse_share_of_inflate"] = {"at_20_gb_per_s": round(pb_ms / (bam_bytes / 20e6), 3), "at_28_gb_per_s": round(pb_ms / (bam_bytes / 28e6), 3)}
        out["parse_call"] = med
        del d_bam, twin, o, recs_out, recs
        # ---- (b) file to file
        if a.pairs:
            m = 2 * a.pairs
            bam_path, f1, f2 = os.path.join(tmp, "reads.bam"), os.path.join(tmp, "r1.fq.gz"), os.path.join(tmp, "r2.fq.gz")
            header = b"BAM\1" + struct.pack("<ii", 0, 0)
            write_bgzf(bam_path, header + ubam_records(reads[:m].numpy(), (0x4D, 0x8D)).tobytes())
            for k, p in ((0, f1), (1, f2)):
                write_bgzf(p, synth._records(reads[:m], k, 2, "sim", True).tobytes())
            out["file_bytes"] = {"bam": os.path.getsize(bam_path), "fastq_twin": os.path.getsize(f1) + os.path.getsize(f2)}
            ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
            mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=a.batch)
            for tag, kw in (("no_sam", {}), ("to_bam", {"bam": True})):
                dst = os.path.join(tmp, "out.bam") if kw else None

                def leg(files, more):
                    def run():
                        mp.reset()
                        t0 = time.perf_counter()
                        st = mp.map_files(files[0], files[1], dst, **more, **kw)
                        dt = time.perf_counter() - t0
                        assert st["reads"] == m, st
                        return {"seconds": dt, "reads_per_s": m / dt}
                    return run
                out["files_" + tag] = in_turns({"ubam": leg((bam_path, None), {}), "bgzf_fastq_twin": leg((f1, f2), dict(device_inflate=True, device_parse=True, device_sam=True))})
                route = mp.last_route()
                assert route[0] & api.ROUTE_ROWS, route  # (the twin ran last: the resident route)
            mp.close(); ix.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump(out, open(a.json, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
