"""How fast are BGZF members inflated on the device, and what does -gpu_inflate do to a files-in run?  150 bp pairs as synth.write_fastq writes them, packed
as bgzip packs them (members of 0xff00 bytes of text):
  (a) the kernel alone — mcx_inflate_dev on members already in HBM, by HIP events on the inflater's stream (mcx_inflate_last_ms), median of --repeats after
      warm-ups: one 8 MB stretch (128 members) at a time, and 1 GB at once (the file's members, repeated until they make 1 GB), levels 1 and 6; beside it
      the host yardstick on the same members: zlib's inflate + crc32 per member on 8 threads, the calls the reader's pool makes for a stretch
      (Parser::feed_bgzf), here from Python threads (both calls release the interpreter's lock); and the reader by itself, mcx_bgzf_inflate: file to text
      in host memory, copies included;
  (b) two files in tmpfs -> no SAM, and -> SAM, with and without device_inflate: reads/s.
    python scripts/bgzf_rate.py [--pairs 4000000] [--json profiles/gpu_inflate/bgzf_rate.json]
(--pack IN OUT LEVEL: packs a file, in a process of its own that never opens the GPU, with a pool of worker processes.)"""
import argparse, json, os, shutil, statistics, struct, subprocess, sys, tempfile, threading, time, zlib
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

BLOCK = 0xff00
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _pack_some(job):
    data, level = job
    out = []
    for i in range(0, len(data), BLOCK):
        chunk = data[i:i + BLOCK]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = c.compress(chunk) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return b"".join(out)


def pack(src, dst, level, workers=16):
    import multiprocessing
    data = open(src, "rb").read()
    step = BLOCK * 64
    with multiprocessing.Pool(workers) as pool, open(dst, "wb") as f:
        for part in pool.imap(_pack_some, ((data[i:i + step], level) for i in range(0, len(data), step)), chunksize=4):
            f.write(part)
        f.write(EOF_MEMBER)


def members_of(raw):
    """(src_off, src_len, isize, crc) of every member of a BGZF file with text"""
    out, o = [], 0
    while o + 28 <= len(raw):
        xlen = raw[o + 10] | raw[o + 11] << 8
        size = (raw[o + 16] | raw[o + 17] << 8) + 1  # (the 'BC' subfield first, as written above)
        crc, isize = struct.unpack_from("<II", raw, o + size - 8)
        if isize:
            out.append((o + 12 + xlen, size - 12 - xlen - 8, isize, crc))
        o += size
    return out


def host_pool_rate(raw, mem, threads=8, repeats=3):
    """GB/s of text: zlib inflate + crc32 per member, `threads` threads, a share of the members each"""
    text = sum(m[2] for m in mem)

    def work(k):
        for off, clen, isize, crc in mem[k::threads]:
            t = zlib.decompressobj(-15).decompress(raw[off:off + clen])
            assert len(t) == isize and zlib.crc32(t) == crc
    best = []
    for _ in range(repeats):
        ts = [threading.Thread(target=work, args=(k,)) for k in range(threads)]
        t0 = time.perf_counter()
        for t in ts: t.start()
        for t in ts: t.join()
        best.append(text / (time.perf_counter() - t0) / 1e9)
    return round(statistics.median(best), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pack", nargs=3, default=None)
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None, help="also write the result there")
    a = ap.parse_args()
    if a.pack:
        pack(a.pack[0], a.pack[1], int(a.pack[2]))
        return
    import numpy as np
    import torch
    import bench
    from mapcaller_amd import api, synth
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    reads = bench.make_reads(codes, lens, a.pairs, 150, seed=9, device=dev).reshape(2 * a.pairs, 150).cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_bgzf_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"pairs": a.pairs, "member_text_bytes": BLOCK}
    try:
        p1, p2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        synth.write_fastq(p1, reads, 0, 2); synth.write_fastq(p2, reads, 1, 2)
        files = {}
        for level in (1, 6):
            files[level] = (os.path.join(tmp, f"l{level}_1.fq.gz"), os.path.join(tmp, f"l{level}_2.fq.gz"))
            for src, dst in zip((p1, p2), files[level]):
                subprocess.run([sys.executable, os.path.abspath(__file__), "--pack", src, dst, str(level)], check=True)
        # ---- (a) the kernel alone
        for level in (1, 6):
            raw = open(files[level][0], "rb").read()
            mem = members_of(raw)
            res = {"file_bytes": len(raw), "text_bytes": sum(m[2] for m in mem), "members": len(mem)}
            res["host_pool_8_threads_gb_per_s"] = host_pool_rate(raw, mem[:4096])
            d_src = torch.from_numpy(np.frombuffer(raw + bytes(8), dtype=np.uint8).copy()).to(dev)
            for tag, count in (("stretch_8mb", 128), ("at_once_1gb", (1 << 30) // BLOCK)):
                recs = np.zeros(count, dtype=api.MEMBER_DTYPE)
                at = 0
                for i in range(count):
                    off, clen, isize, crc = mem[i % (len(mem) - 1)]  # (the file's full members, again and again)
                    recs[i] = (off, at, clen, isize, crc, 0)
                    at += isize
                d_mem = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
                d_dst = torch.empty(at, dtype=torch.uint8, device=dev)
                d_st = torch.zeros(count, dtype=torch.int32, device=dev)
                with api.Inflater(device=0, max_members=count) as inf:
                    ms = []
                    for k in range(a.repeats + 2):
                        assert inf.inflate_dev(d_src, d_mem, count, d_dst, d_st) == 0
                        if k >= 2:
                            ms.append(inf.last_ms())
                first = mem[0]
                assert zlib.crc32(d_dst[:first[2]].cpu().numpy().tobytes()) == first[3]
                res[tag] = {"members": count, "text_bytes": at, "kernel_ms_median": round(statistics.median(ms), 3), "kernel_ms_min": round(min(ms), 3),
                            "text_gb_per_s": round(at / statistics.median(ms) / 1e6, 3)}
                del d_mem, d_dst, d_st
            del d_src
            host = np.empty(res["text_bytes"] + 64, dtype=np.uint8)
            L = api.lib()
            secs = []
            for k in range(3):
                t0 = time.perf_counter()
                n = L.mcx_bgzf_inflate(files[level][0].encode(), 0, host.ctypes.data, host.size, None)
                secs.append(time.perf_counter() - t0)
                assert n == res["text_bytes"], n
            res["reader_alone_file_to_host_text_gb_per_s"] = round(res["text_bytes"] / min(secs[1:]) / 1e9, 3)
            out[f"level_{level}"] = res
        # ---- (b) files in, with and without device_inflate
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=1 << 20)
        sam = os.path.join(tmp, "out.sam")
        for level in (1, 6):
            for to_sam in (False, True):
                for dev_inf in (False, True):
                    f1, f2 = files[level]
                    secs, st = [], None
                    for k in range(3):  # (a warm-up, then the better of two)
                        mp.reset()
                        t0 = time.perf_counter()
                        st = mp.map_files(f1, f2, sam if to_sam else None, device_inflate=dev_inf)
                        secs.append(time.perf_counter() - t0)
                    dt = min(secs[1:])
                    out[f"files_level_{level}_{'to_sam' if to_sam else 'no_sam'}_{'device' if dev_inf else 'host'}_inflate"] = {
                        "reads": st["reads"], "seconds": round(dt, 3), "reads_per_s": round(st["reads"] / dt)}
        mp.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump(out, open(a.json, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
