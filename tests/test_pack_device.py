"""k_pack_reads with rows as long as the batch's longest read needs, and the batch's tail (k_reduce_stats, k_chunk_sums, k_avg_walk, k_check_est),
through the public API on the GPU: batches of mixed read lengths against the oracle, the stride of one batch not kept for the next, a batch that
goes through an avgDist replay and the large tier, and the tail at pair counts around the chunk size and the walk's workgroup size."""
import gzip
import os

import numpy as np
import pytest

from conftest import GOLD, ROOT, sam_diff

pytestmark = pytest.mark.gpu

LENS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 149, 150, 151, 255, 256, 1000)
DIFFERS = "device's walk of the batch's chunks differs"


@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()  # raises if the HIP extension is missing: there is no fallback
    assert a.device_count() >= 1, "no GPU visible"
    return a


def _oracle_sam(prefix, f1, f2, alg, out):
    import ctypes
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libmcx_oracle.so"))
    L.mcxo_index_load.restype = ctypes.c_void_p
    L.mcxo_index_load.argtypes = [ctypes.c_char_p]
    L.mcxo_map_files.restype = ctypes.c_int64
    L.mcxo_map_files.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]
    ix = L.mcxo_index_load(prefix.encode())
    assert ix
    assert L.mcxo_map_files(ix, f1.encode(), (f2 or "").encode(), 0 if alg == "nw" else 1, out.encode(), 1, None) > 0


def _rc(s):
    return s[::-1].translate(bytes.maketrans(b"ACGTN", b"TGCAN"))


@pytest.fixture(scope="module")
def mc_genome():
    return b"".join(l for l in gzip.open(os.path.join(GOLD, "mc", "genome.fa.gz"), "rb").read().split(b"\n") if not l.startswith(b">"))


def _mixed_pairs(genome, n_pairs, longest, seed):
    """pairs whose mates take the lengths of LENS up to `longest` in turn (mate 1 and mate 2 different ones), cut from the genome 300 apart,
    every third read with an N at its first, its last or a boundary base"""
    rng = np.random.default_rng(seed)
    lens = [n for n in LENS if n <= longest]
    pairs = []
    for i in range(n_pairs):
        a, b = lens[i % len(lens)], lens[(i * 5 + 3) % len(lens)]
        p = int(rng.integers(2000, len(genome) - 3000))
        r1, r2 = bytearray(genome[p:p + a]), bytearray(_rc(genome[p + 300:p + 300 + b]))
        for r in (r1, r2):
            if rng.integers(3) == 0:
                at = [0, len(r) - 1, 15, 16, 31, 32, len(r) - 16, len(r) - 17][int(rng.integers(8))]
                if 0 <= at < len(r):
                    r[at] = ord("N")
        pairs.append((bytes(r1), bytes(r2)))
    return pairs


def _write_fastq(path, reads):
    with open(path, "wb") as f:
        for i, s in enumerate(reads):
            f.write(b"@p%05d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))


def _batch_arrays(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in reads])
    return np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), off


def _sam_of_batch(api, ix, mp, reads, paired, path):
    """the batch through mcx_map_batch (the step packs it itself, rows as long as its longest read needs) and the records as SAM text"""
    bases, off = _batch_arrays(reads)
    aln, cig = mp.map_batch(bases, off, paired)
    names = [b"p%05d" % (i // 2 if paired else i) for i in range(len(reads))]
    text = mp.sam_text(bases, off, names, [b"I" * len(s) for s in reads], paired, aln, cig)
    with open(path, "wb") as f:
        f.write(api.sam_header(ix) + text)


@pytest.mark.parametrize("max_read_len,longest", [(256, 151), (256, 256), (1000, 256), (1000, 1000)])
def test_mixed_read_lengths_equal_oracle(api, golden, mc_genome, tmp_path, max_read_len, longest):
    """Mates of 1 to `longest` bases mixed in one batch, paired and single-end, on contexts made for reads of 256 and of 1000 bases — rows as long as the
    context's would be longer than the batch's, or just as long: the file front end's way in (rows packed on the way in keep the context's stride) and
    mcx_map_batch (the step packs, the batch's own stride) — SAM equal to the oracle's both ways."""
    g = golden["mc"]
    pairs = _mixed_pairs(mc_genome, 127, longest, seed=11)
    ix = api.Index(g["prefix"], device=0)
    for paired in (True, False):
        m1, m2 = [p[0] for p in pairs], [p[1] for p in pairs]
        f1, f2 = str(tmp_path / f"r1.{paired}.fq"), str(tmp_path / f"r2.{paired}.fq")
        for path, mates in ((f1, m1), (f2, m2)):
            with open(path, "wb") as f:
                for i, s in enumerate(mates):
                    f.write(b"@p%05d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
        ora = str(tmp_path / f"ora.{paired}.sam")
        _oracle_sam(g["prefix"], f1, f2 if paired else None, "ksw2", ora)
        for ctx_len in (max_read_len,):
            mp = api.Mapper(ix, alg="ksw2", max_read_len=ctx_len, max_batch_reads=400)
            out = str(tmp_path / f"files.{paired}.{ctx_len}.sam")
            mp.map_files(f1, f2 if paired else None, out)
            nd, ex = sam_diff(ora, out, mask_se_reverse_qual=True)
            assert nd == 0, ("map_files", paired, ctx_len, ex)
            reads = [x for p in pairs for x in p] if paired else m1
            out = str(tmp_path / f"batch.{paired}.{ctx_len}.sam")
            mp.reset()
            _sam_of_batch(api, ix, mp, reads, paired, out)
            nd, ex = sam_diff(ora, out, mask_se_reverse_qual=True)
            assert nd == 0, ("map_batch", paired, ctx_len, ex)
            mp.close()
    ix.close()


def test_a_batch_does_not_keep_the_stride_of_the_batch_before(api, golden, mc_genome, tmp_path):
    """Two batches on one context, the longest read 150 bases in the first and 40 in the second (rows of 20 words, then of 8): each equals the oracle's
    SAM of the same reads, the second one after the first and on a fresh context alike."""
    g = golden["mc"]
    rng = np.random.default_rng(5)
    ix = api.Index(g["prefix"], device=0)
    batches = []
    for n in (150, 40):
        reads = []
        for i in range(200):
            p = int(rng.integers(2000, len(mc_genome) - 3000))
            reads += [mc_genome[p:p + n - (i % 3)], _rc(mc_genome[p + 250:p + 250 + n])]
        batches.append(reads)
    mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=400)
    for k, reads in enumerate(batches):
        f1, f2, ora, out = (str(tmp_path / f"{x}.{k}") for x in ("r1.fq", "r2.fq", "ora.sam", "gpu.sam"))
        _write_fastq(f1, reads[0::2]); _write_fastq(f2, reads[1::2])
        _oracle_sam(g["prefix"], f1, f2, "ksw2", ora)
        mp.reset()  # (the insert-size state: each batch is a run of its own to the oracle)
        _sam_of_batch(api, ix, mp, reads, True, out)
        nd, ex = sam_diff(ora, out)
        assert nd == 0, (k, ex)
    mp.close(); ix.close()


def test_replay_and_large_tier_on_the_batch_stride(api, golden, tmp_path, monkeypatch, capfd):
    """The `var` pairs in batches of 200 pairs with what only a large batch switches on (MCX_ORDER_MIN=1) on a context made for reads of 1000 bases:
    pairs are replayed for the insert-size estimate (asserted) and, on `mc`, pairs go through the large tier (asserted) — every pass of a batch strides
    over rows of the batch's own length.  SAM equal to the reference's, and the device's walk of the chunks never differs from the host's."""
    monkeypatch.setenv("MCX_ORDER_MIN", "1")
    monkeypatch.setenv("MCX_TIMING", "1")
    seen = {}
    for name in ("var", "mc"):
        g = golden[name]
        reads1 = [l for i, l in enumerate(open(g["r1"], "rb").read().split(b"\n")) if i % 4 == 1]
        reads2 = [l for i, l in enumerate(open(g["r2"], "rb").read().split(b"\n")) if i % 4 == 1]
        names = [l[1:].split()[0] for i, l in enumerate(open(g["r1"], "rb").read().split(b"\n")) if i % 4 == 0 and l]
        quals1 = [l for i, l in enumerate(open(g["r1"], "rb").read().split(b"\n")) if i % 4 == 3]
        quals2 = [l for i, l in enumerate(open(g["r2"], "rb").read().split(b"\n")) if i % 4 == 3]
        ix = api.Index(g["prefix"], device=0, full_sa=True)
        mp = api.Mapper(ix, alg="ksw2", max_read_len=1000, max_batch_reads=400)
        capfd.readouterr()
        text = api.sam_header(ix)
        for lo in range(0, len(names), 200):
            hi = min(len(names), lo + 200)
            reads = [x for p in range(lo, hi) for x in (reads1[p], reads2[p])]
            quals = [x for p in range(lo, hi) for x in (quals1[p], quals2[p])]
            bases, off = _batch_arrays(reads)
            aln, cig = mp.map_batch(bases, off, True)
            text += mp.sam_text(bases, off, [n for p in range(lo, hi) for n in (names[p], names[p])], quals, True, aln, cig)
        err = capfd.readouterr().err
        assert DIFFERS not in err, err[-2000:]
        out = str(tmp_path / f"{name}.sam")
        open(out, "wb").write(text)
        nd, ex = sam_diff(g["sam"]["ksw2"], out)
        assert nd == 0, (name, ex)
        seen[name] = mp.stats.as_dict()
        mp.close(); ix.close()
    print("[pack stride]", {k: (v["replayed_pairs"], v["tier1_pairs"]) for k, v in seen.items()})
    assert seen["var"]["replayed_pairs"] > 0, seen["var"]
    assert seen["var"]["tier1_pairs"] + seen["mc"]["tier1_pairs"] > 0, seen


# ---- the tail's shapes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tail_setup(api, golden):
    """300 pairs of `var`, each through the step API as a batch of its own: what k_chunk_sums makes of a batch of ONE pair is that pair's record
    (proper or not, its distance, its mates' lengths) — the per-pair records the sums of the larger batches are computed from in numpy.  A pair's
    record depends on its reads and the estimate it is mapped under and on nothing else, so the same est0 is handed to every batch below."""
    import torch
    g = golden["var"]
    reads1 = [l for i, l in enumerate(open(g["r1"], "rb").read().split(b"\n")) if i % 4 == 1][:300]
    reads2 = [l for i, l in enumerate(open(g["r2"], "rb").read().split(b"\n")) if i % 4 == 1][:300]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    n_max = 2 * (100 * 1024 + 1)
    with pytest.MonkeyPatch.context() as env:
        env.setenv("MCX_TIMING", "1")  # (read when the context is made: the call then says when its two walks differ)
        mp = api.Mapper(ix, alg="ksw2", max_batch_reads=n_max)
    d_aln = torch.empty(n_max * 64, dtype=torch.uint8, device="cuda")
    d_cig = torch.empty(api.cigar_pool_words(n_max), dtype=torch.int32, device="cuda")
    est0 = 1500
    rec = np.zeros((300, 3), dtype=np.int64)
    for p in range(300):
        bases, off = _batch_arrays([reads1[p], reads2[p]])
        tb, to = torch.from_numpy(np.concatenate([bases, np.zeros(64, np.uint8)])).cuda(), torch.from_numpy(off.astype(np.int64)).to(torch.int32).cuda()
        mp.batch_begin(tb.data_ptr(), to.data_ptr(), 2, True, est0, 0, d_aln.data_ptr(), d_cig.data_ptr())
        ok, ds, ls = mp.batch_sums()
        rec[p] = (int(ok[0]), int(ds[0]), int(ls[0]))
        mp.batch_end()
    assert rec[:, 0].sum() > 100, rec[:, 0].sum()  # (most pairs of the set are proper ones)
    yield dict(api=api, ix=ix, mp=mp, reads1=reads1, reads2=reads2, rec=rec, est0=est0, d_aln=d_aln, d_cig=d_cig)
    mp.close(); ix.close()


@pytest.mark.parametrize("n_pairs", [1, 99, 100, 101, 199, 200, 100 * 1024 + 1])
def test_tail_sums_and_estimates(tail_setup, capfd, n_pairs):
    """A batch of n_pairs pairs (the 300 in turn): the chunk sums of the step API (k_chunk_sums) equal the per-pair records summed in numpy chunk
    by chunk; and the same batch through mcx_map_batch_dev, whose tail walks the chunks on the device (k_avg_walk) — it compares the device's
    estimates with mcx_avg_walk's and says so under MCX_TIMING when they differ: it must not."""
    import torch
    t = tail_setup
    api, mp = t["api"], t["mp"]
    idx = np.arange(n_pairs) % 300
    one = [_batch_arrays([t["reads1"][p], t["reads2"][p]]) for p in range(300)]
    lens = np.array([[len(t["reads1"][p]), len(t["reads2"][p])] for p in range(300)])
    off = np.zeros(2 * n_pairs + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens[idx].reshape(-1))
    bases = np.concatenate([one[p][0] for p in idx] + [np.zeros(64, np.uint8)])
    tb, to = torch.from_numpy(bases).cuda(), torch.from_numpy(off).to(torch.int32).cuda()
    # the step API: the sums as the first pass leaves them
    mp.batch_begin(tb.data_ptr(), to.data_ptr(), 2 * n_pairs, True, t["est0"], 0, t["d_aln"].data_ptr(), t["d_cig"].data_ptr())
    ok, ds, ls = (np.array(x, dtype=np.int64) for x in mp.batch_sums())
    mp.batch_end()
    n_chunks = (n_pairs + 99) // 100
    want = np.zeros((n_chunks * 100, 3), dtype=np.int64)
    want[:n_pairs] = t["rec"][idx]
    want = want.reshape(n_chunks, 100, 3).sum(axis=1)
    assert len(ok) == n_chunks
    assert np.array_equal(ok, want[:, 0]) and np.array_equal(ds, want[:, 1]) and np.array_equal(ls, want[:, 2])
    # the whole call, from a state in the middle of a run (more than 1000 proper pairs behind it, so that every chunk's estimate is a mean of what lies
    # before it): the tail behind the batch's kernels, its walk against the host's
    mp.reset()
    mp.avg[0], mp.avg[1], mp.avg[2], mp.avg[3] = 400, 5000, 5000 * 400, 0
    capfd.readouterr()
    mp.map_batch_dev(tb.data_ptr(), to.data_ptr(), 2 * n_pairs, True, t["d_aln"].data_ptr(), t["d_cig"].data_ptr())
    err = capfd.readouterr().err
    assert DIFFERS not in err, err[-2000:]
    assert mp.avg[3] == 2 * n_pairs and mp.avg[1] >= 5000
