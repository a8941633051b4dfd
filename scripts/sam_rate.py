"""How fast is the SAM text made on the device, and what does -gpu_sam do to a files-to-SAM run?  One bench-shaped batch (bench.make_genome /
make_reads, 150 bp pairs, names and qualities as synth.write_fastq writes them):
  * mcx_sam_format_dev on the mapped batch in HBM: the kernels' times by HIP events on the context's stream (length, scan, write) and the whole call's
    wall time, median of --repeats after a warm-up; bytes in and out, GB/s;
  * files in tmpfs -> SAM with and without device_sam, plain FASTQ and .gz pairs: reads/s and the MCX_TIMING lines.
    python scripts/sam_rate.py [--genome-mbp 3100 --pairs 4000000] [--json profiles/sam_rate.json]"""
import argparse, ctypes as C, json, os, shutil, statistics, subprocess, sys, tempfile, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import bench
from mapcaller_amd import api, synth


class Stderr:
    """the library's MCX_TIMING lines (written to fd 2) of the calls inside"""
    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("latin-1")
        self.tmp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=float, default=3100.0)
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--pairs", type=int, default=4_000_000, help="read pairs of the batch (bench.py's --batch-pairs)")
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--file-batch-reads", type=int, default=1 << 21)
    ap.add_argument("--json", default=None, help="also write the result there")
    a = ap.parse_args()
    args = argparse.Namespace(genome_mbp=a.genome_mbp, contigs=a.contigs, repeats=2000, genome="human")
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(args, dev, seed=5)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=True)
    n = 2 * a.pairs
    reads = bench.make_reads(codes, lens, a.pairs, 150, seed=9, device=dev).reshape(n, 150)
    tmp = tempfile.mkdtemp(prefix="mcx_sam_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"reads": n, "genome_mbp": a.genome_mbp}
    L = api.lib()
    try:
        f1, f2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        host = reads.cpu()
        synth.write_fastq(f1, host, 0, 2); synth.write_fastq(f2, host, 1, 2)
        # ---- the batch in HBM: names as the files hold them, qualities 'I'
        names = [l[1:] for l in open(f1, "rb").read().split(b"\n")[0::4] if l]
        names = [x for x in names for _ in (0, 1)]
        name_off = np.zeros(n + 1, dtype=np.uint32)
        name_off[1:] = np.cumsum([len(x) for x in names])
        t_names = torch.from_numpy(np.frombuffer(b"".join(names) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        t_name_off = torch.from_numpy(name_off).to(dev)
        t_bases = torch.cat([reads.reshape(-1), torch.zeros(64, dtype=torch.uint8, device=dev)])
        t_off = (torch.arange(n + 1, device=dev, dtype=torch.int64) * 150).to(torch.int32)
        t_qual = torch.full((n * 150 + 16,), ord("I"), dtype=torch.uint8, device=dev)
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=n)
        d_aln = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
        d_cig = torch.zeros(api.cigar_pool_words(n), dtype=torch.int32, device=dev)
        mp.map_batch_dev(t_bases.data_ptr(), t_off.data_ptr(), n, True, d_aln.data_ptr(), d_cig.data_ptr())
        t = time.perf_counter()
        mp.map_batch_dev(t_bases.data_ptr(), t_off.data_ptr(), n, True, d_aln.data_ptr(), d_cig.data_ptr())
        out["map_batch_dev_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        words = C.c_uint32()
        L.mcx_cigar_words(mp._h, C.byref(words))
        si = api.SamIn()
        si.bases, si.off, si.qual, si.names, si.name_off = t_bases.data_ptr(), t_off.data_ptr(), t_qual.data_ptr(), t_names.data_ptr(), t_name_off.data_ptr()
        si.aln, si.cigar, si.n_reads, si.paired = d_aln.data_ptr(), d_cig.data_ptr(), n, 1
        nb = C.c_uint64()
        L.mcx_sam_format_dev(mp._h, C.byref(si), None, 0, None, C.byref(nb))
        d_text = torch.empty(nb.value + 64, dtype=torch.uint8, device=dev)
        ms = (C.c_float * 3)()
        L.mcx_sam_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        runs = []
        for k in range(a.repeats + 2):
            t = time.perf_counter()
            rc = L.mcx_sam_format_dev(mp._h, C.byref(si), d_text.data_ptr(), nb.value, None, C.byref(nb))
            wall = (time.perf_counter() - t) * 1e3
            assert rc == 0, L.mcx_last_error()
            L.mcx_sam_last_ms(mp._h, ms)
            if k >= 2:
                runs.append((ms[0], ms[1], ms[2], wall))
        med = [statistics.median(r[i] for r in runs) for i in range(4)]
        bytes_in = int(name_off[-1]) + 2 * n * 150 + n * 64 + words.value * 4 + (n + 1) * 16
        out["format_dev"] = {"len_kernel_ms": round(med[0], 3), "scan_ms": round(med[1], 3), "write_kernel_ms": round(med[2], 3), "call_ms": round(med[3], 3),
                             "min_call_ms": round(min(r[3] for r in runs), 3), "max_call_ms": round(max(r[3] for r in runs), 3), "repeats": len(runs),
                             "bytes_in": bytes_in, "bytes_out": nb.value, "write_kernel_gb_per_s": round((bytes_in + nb.value) / med[2] / 1e6, 1),
                             "call_gb_per_s": round((bytes_in + nb.value) / med[3] / 1e6, 1)}
        mp.close()
        del d_text, d_aln, d_cig, t_qual
        # ---- files -> SAM
        procs = [subprocess.Popen(["gzip", "-6", "-k", f]) for f in (f1, f2)]
        assert all(q.wait() == 0 for q in procs)
        os.environ["MCX_TIMING"] = "1"
        mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=a.file_batch_reads)
        sam = os.path.join(tmp, "o.sam")
        for tag, (p1, p2) in (("plain", (f1, f2)), ("gz", (f1 + ".gz", f2 + ".gz"))):
            for dev_sam in (False, True):
                best = None
                for rep in range(3):  # (the first warms the page cache and the batch objects)
                    mp.reset()
                    with Stderr() as err:
                        t = time.perf_counter()
                        st = mp.map_files(p1, p2, sam, device_sam=dev_sam)
                        dt = time.perf_counter() - t
                    if rep and (best is None or dt < best[0]):
                        best = (dt, [l for l in err.text.split("\n") if l.startswith("[mcx_map_files] busy") or "device_sam" in l or "wall seconds" in l])
                out[f"files_{tag}_{'gpu_sam' if dev_sam else 'host_sam'}"] = {"reads_per_s": round(st["reads"] / best[0]), "seconds": round(best[0], 3), "sam_bytes": os.path.getsize(sam),
                                                                                "timing": best[1]}
        mp.close()
        print(json.dumps(out))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
