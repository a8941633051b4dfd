"""How fast is an ORDINARY gzip stream inflated on the device (mcx_gunzipper: block-start search, symbolic inflate, window chain, text + CRC-32), and what does
-gpu_gz -gpu_parse [-gpu_sam] do to a files-in run?  The inputs of scripts/resident_rate.py — 150 bp pairs as synth.write_fastq writes them (1.27 GB of text a
file at 4 M pairs), a 100 Mbp genome, batches of 1 M reads, the files in tmpfs — as ordinary .gz at level 6: ONE member, one deflate stream, compressed in
pieces of 4 MB by a pool of processes that each end their piece on a byte boundary (a sync flush: what pigz writes, with larger pieces).
  (a) the two calls alone on file 1's stream in HBM: mcx_gunzip_round_dev + mcx_gunzip_text_dev round by round over the whole stream, for stretches of 32, 64 and
      128 KB and rounds of 512 to 4096 stretches; --repeats passes per setting, the settings in turns; GB/s of text by the wall clock of the calling thread (host
      work between the kernels included) and the sums of ms[0..3] (search, inflate, windows, text + CRC: events on the object's stream); the whole text's CRC-32
      is held against zlib's.  Beside it, on the same text: mcx_gz_inflate with the box's host threads (file to text in host memory), mcx_gz_inflate_dev (file to
      text in host memory: staging and the copy back included), and mcx_inflate_dev on the text packed as BGZF, all members at once.
  (b) two files -> no SAM, and -> SAM: the host readers (every switch off) and the new route in turns, --alternate rounds after a warm-up round: every run's
      seconds, median and range per leg, and mcx_files_route's word.
    python scripts/gz_dev_rate.py [--pairs 4000000] [--repeats 5] [--alternate 5] [--json profiles/gpu_gz/gz_dev_rate.json]
(--pack IN OUT LEVEL: packs a file, in a process of its own that never opens the GPU.)"""
import argparse, json, os, shutil, statistics, struct, subprocess, sys, tempfile, time, zlib
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

PIECE = 4 << 20
HEADER = b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03"


def _pack_piece(job):
    data, level, last = job
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH)


def pack(src, dst, level, workers=16):
    import multiprocessing
    data = open(src, "rb").read()
    n = (len(data) + PIECE - 1) // PIECE
    with multiprocessing.Pool(workers) as pool, open(dst, "wb") as f:
        f.write(HEADER)
        for comp in pool.imap(_pack_piece, ((data[i * PIECE:(i + 1) * PIECE], level, i == n - 1) for i in range(n)), chunksize=1):
            f.write(comp)
        f.write(struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF))


def one_pass(api, torch, z, d_src, n_src, d_dst):
    """the whole stream round by round: (seconds, [sum of ms[k]], rounds, mean chain share, text bytes)"""
    z.reset()
    bit, at, ms, rounds, share = 0, 0, [0.0] * 4, 0, []
    t0 = time.perf_counter()
    while True:
        info = z.round_dev(d_src, bit >> 3, n_src - (bit >> 3), bit & 7, True)
        assert info.status == api.GZ_OK, info.status
        z.text_dev(d_dst[at:at + max(info.text_bytes, 1)], info)
        for k in range(4):
            ms[k] += info.ms[k]
        rounds += 1; at += info.text_bytes; share.append(info.chain / info.stretches)
        if info.final:
            break
        bit = (bit >> 3) * 8 + info.end_bit
    return time.perf_counter() - t0, ms, rounds, sum(share) / len(share), at


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pack", nargs=3, default=None)
    ap.add_argument("--pairs", type=int, default=4_000_000)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--alternate", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write the result there")
    a = ap.parse_args()
    if a.pack:
        pack(a.pack[0], a.pack[1], int(a.pack[2]))
        return
    import numpy as np
    import torch
    import bench
    import bgzf_rate
    from mapcaller_amd import api, synth
    args = argparse.Namespace(genome_mbp=100.0, contigs=4, repeats=200, genome="uniform")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    reads = bench.make_reads(codes, lens, a.pairs, 150, seed=9, device=dev).reshape(2 * a.pairs, 150).cpu()
    tmp = tempfile.mkdtemp(prefix="mcx_gz_dev_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"pairs": a.pairs, "level": 6, "piece_bytes": PIECE, "batch_reads": a.batch, "host_cpus": int(api.lib().mcx_host_cpus())}
    L = api.lib()
    try:
        p1, p2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        synth.write_fastq(p1, reads, 0, 2); synth.write_fastq(p2, reads, 1, 2)
        f1, f2, b1 = os.path.join(tmp, "o1.fq.gz"), os.path.join(tmp, "o2.fq.gz"), os.path.join(tmp, "b1.fq.gz")
        for src, dst in ((p1, f1), (p2, f2)):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--pack", src, dst, "6"], check=True)
        subprocess.run([sys.executable, os.path.join(HERE, "bgzf_rate.py"), "--pack", p1, b1, "6"], check=True)
        text_bytes = os.path.getsize(p1)
        want_crc = zlib.crc32(open(p1, "rb").read())
        os.remove(p1); os.remove(p2)
        out["text_bytes_per_file"], out["file_bytes"] = text_bytes, os.path.getsize(f1)
        print(f"packed: {text_bytes} bytes of text, {out['file_bytes']} compressed", file=sys.stderr, flush=True)
        # ---- (a) the calls alone
        raw = open(f1, "rb").read()[len(HEADER):-8]
        d_src = torch.from_numpy(np.frombuffer(raw + bytes(8), dtype=np.uint8).copy()).to(dev)
        d_dst = torch.empty(text_bytes + 64, dtype=torch.uint8, device=dev)
        settings = [(s << 10, n) for s in (32, 64, 128) for n in (512, 1024, 2048, 4096)]
        runs = {k: [] for k in settings}
        for rep in range(a.repeats + 1):  # (the first pass warms up; the settings in turns)
            for s, n in settings:
                with api.Gunzipper(0, s, n) as z:
                    secs, ms, rounds, share, got = one_pass(api, torch, z, d_src, len(raw), d_dst)
                assert got == text_bytes
                if rep == 0 and (s, n) == settings[0]:
                    assert zlib.crc32(d_dst[:text_bytes].cpu().numpy().tobytes()) == want_crc
                if rep:
                    runs[(s, n)].append((secs, ms, rounds, share))
        out["calls"] = {}
        for (s, n), rs in runs.items():
            wall = [text_bytes / r[0] / 1e9 for r in rs]
            dev_ms = [sum(r[1]) for r in rs]
            med = sorted(rs, key=lambda r: r[0])[len(rs) // 2]
            out["calls"][f"{s >> 10}KB_x_{n}"] = {"rounds": med[2], "chain_share": round(med[3], 3), "wall_gb_per_s_median": round(statistics.median(wall), 2), "wall_gb_per_s_range": [round(min(wall), 2), round(max(wall), 2)],
                                                  "kernels_gb_per_s_median": round(text_bytes / statistics.median(dev_ms) / 1e6, 2), "ms_search_inflate_windows_text": [round(x, 2) for x in med[1]]}
            print(f"{s >> 10} KB x {n}: {out['calls'][f'{s >> 10}KB_x_{n}']}", file=sys.stderr, flush=True)
        del d_src, d_dst
        host = np.empty(text_bytes + 64, dtype=np.uint8)
        for tag, call in (("mcx_gz_inflate_host_threads", lambda: L.mcx_gz_inflate(f1.encode(), out["host_cpus"], 2 << 20, host.ctypes.data, host.size, None)),
                          ("mcx_gz_inflate_dev_file_to_host", lambda: L.mcx_gz_inflate_dev(f1.encode(), 0, 0, 0, host.ctypes.data, host.size, None))):
            secs = []
            for k in range(a.repeats + 1):
                t0 = time.perf_counter()
                assert call() == text_bytes
                if k:
                    secs.append(time.perf_counter() - t0)
            out[tag] = {"gb_per_s_median": round(text_bytes / statistics.median(secs) / 1e9, 2), "gb_per_s_range": [round(text_bytes / max(secs) / 1e9, 2), round(text_bytes / min(secs) / 1e9, 2)]}
            print(tag, out[tag], file=sys.stderr, flush=True)
        del host
        braw = open(b1, "rb").read()
        mem = bgzf_rate.members_of(braw)
        recs = np.zeros(len(mem), dtype=api.MEMBER_DTYPE)
        at = 0
        for i, (off, clen, isize, crc) in enumerate(mem):
            recs[i] = (off, at, clen, isize, crc, 0)
            at += isize
        d_b = torch.from_numpy(np.frombuffer(braw + bytes(8), dtype=np.uint8).copy()).to(dev)
        d_mem = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
        d_t = torch.empty(at, dtype=torch.uint8, device=dev)
        d_st = torch.zeros(len(mem), dtype=torch.int32, device=dev)
        with api.Inflater(device=0, max_members=len(mem)) as inf:
            ms = []
            for k in range(a.repeats + 1):
                assert inf.inflate_dev(d_b, d_mem, len(mem), d_t, d_st) == 0
                if k:
                    ms.append(inf.last_ms())
        out["mcx_inflate_dev_bgzf_at_once"] = {"members": len(mem), "gb_per_s_median": round(at / statistics.median(ms) / 1e6, 2), "gb_per_s_range": [round(at / max(ms) / 1e6, 2), round(at / min(ms) / 1e6, 2)]}
        print("bgzf", out["mcx_inflate_dev_bgzf_at_once"], file=sys.stderr, flush=True)
        del d_b, d_mem, d_t, d_st
        # ---- (b) files in: the host readers and the route in turns
        legs = {"host": {}, "gz": {"device_gz": True, "device_parse": True, "device_sam": True}}
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=a.batch)
        sam = os.path.join(tmp, "out.sam")
        for to_sam in (False, True):
            secs, routes, st = {leg: [] for leg in legs}, {}, None
            for k in range(a.alternate + 1):
                for leg, kw in legs.items():
                    mp.reset()
                    t0 = time.perf_counter()
                    st = mp.map_files(f1, f2, sam if to_sam else None, **kw)
                    if k:
                        secs[leg].append(round(time.perf_counter() - t0, 3))
                    routes[leg] = list(mp.last_route())
            res = {leg: {"seconds": s, "median": statistics.median(s), "min": min(s), "max": max(s), "reads_per_s_at_median": round(st["reads"] / statistics.median(s)),
                         "reads_per_s_range": [round(st["reads"] / max(s)), round(st["reads"] / min(s))], "route": routes[leg]} for leg, s in secs.items()}
            out["files_to_sam" if to_sam else "files_no_sam"] = res
            print(("to SAM" if to_sam else "no SAM") + " in turns: " + ", ".join(f"{leg} {r['reads_per_s_at_median'] / 1e6:.2f} M reads/s ({r['min']:.3f}-{r['max']:.3f} s) route {r['route']}" for leg, r in res.items()), file=sys.stderr, flush=True)
        mp.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            json.dump(out, open(a.json, "w"), indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
