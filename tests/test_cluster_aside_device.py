"""The heavy pairs aside (run_pairs, mapcaller_amd/csrc/mcx_pipeline.hip): with the order made, the pairs of the heavy weight classes are listed and
clustered on a side stream behind k_seed, beside the straight-line path, the light ones on the pass's stream behind it; MCX_CLUSTER_IN_LINE=1 is the
one launch over all classes.  Everything here runs with MCX_ORDER_MIN=1, so that the small batches of the golden sets take the path.

The golden sets `var` and `mc`, both algorithms, go through Mapper.map_batch in batches of 1 pair (the first 300 pairs: a batch whose only pair is heavy
leaves the light launch empty, and the reverse), of 63 pairs (a class boundary inside a wavefront) and of 200 pairs; each pair's records come from the batch
that holds it.  Records and CIGAR words per read must be equal between the default and MCX_CLUSTER_IN_LINE=1.  The golden SAM itself is compared through
map_files (sam_diff) in batches of 200 pairs (max_batch_reads = 400): map_batch on a batch that is no multiple of the reference's 200-read chunks moves the
insert-size estimate at other places than the reference does, so only whole chunks can be held against its SAM.

mcx_pass_last_shape says what the last tier-0 pass did; the combinations (aside taken; heavy > 0 and light = 0; heavy = 0 and light > 0; both > 0) are
counted over the batches, per set, and each must be seen (at most one may be missing per set, none over both)."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, sam_diff

gpu = pytest.mark.gpu
FIELDS = ("pos", "mate_pos", "chr", "flag", "mapq", "tlen", "nm", "as", "xs", "n_cigar", "fwd", "has_mate")  # (not cigar_off: the pool's order is the atomics')


@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()  # raises if the HIP extension is missing: there is no fallback
    assert a.device_count() >= 1, "no GPU visible"
    return a


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def read_seqs(path):
    lines = open(path, "rb").read().split(b"\n")
    if lines[0].startswith(b">"):  # FASTA, one line a read
        return [l for i, l in enumerate(lines) if i % 2 == 1 and l]
    return [l for i, l in enumerate(lines) if i % 4 == 1]


def make_batch(g, lo, hi):
    """reads of pairs (single-end: reads) lo..hi-1 as map_batch takes them"""
    r1 = g["_r1"][lo:hi]
    seqs = [x for p in zip(r1, g["_r2"][lo:hi]) for x in p] if g["paired"] else r1
    off = np.zeros(len(seqs) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), off, any(b"N" in s for s in seqs)


def spans(n_total):
    """the batches of a set: 1 pair each over the first 300, then 63 pairs, then 200 pairs"""
    out = [(i, i + 1) for i in range(min(300, n_total))]
    out += [(lo, lo + 63) for lo in range(0, min(1008, n_total - 62), 63)]
    out += [(lo, lo + 200) for lo in range(0, min(2000, n_total - 199), 200)]
    return out


def run_batches(api, ix, alg, paired, batches, in_line):
    """every batch through one fresh context: per batch (record fields, CIGAR words per read, shape of the pass, large-tier pairs of the batch)"""
    kv = {"MCX_ORDER_MIN": "1"}
    if in_line:
        kv["MCX_CLUSTER_IN_LINE"] = "1"
    out = []
    with env(**kv):
        mp = api.Mapper(ix, alg=alg, max_batch_reads=400)  # (the switches are read when the context is made)
    try:
        for bases, off, _ in batches:
            t1 = mp.stats.tier1_pairs
            if mp.avg[3] % 200:  # a batch starts a new 200-read chunk of the insert-size estimate (as a further library does in map_files)
                mp.avg[3] += 200 - mp.avg[3] % 200
            aln, cig = mp.map_batch(bases, off, paired)
            out.append((np.stack([aln[f] for f in FIELDS]), [c.tolist() for c in cig], mp.pass_last_shape(), mp.stats.tier1_pairs - t1))
    finally:
        mp.close()
    return out


_sets, _runs = {}, {}


def the_set(api, golden, name):
    if name not in _sets:
        g = dict(golden[name])
        g["_r1"] = read_seqs(g["r1"])
        g["_r2"] = read_seqs(g["r2"]) if g["paired"] else None
        g["ix"] = api.Index(g["prefix"], device=0, full_sa=True)  # (k_simple takes text positions: every suffix-array entry in HBM, the product's default)
        _sets[name] = g
    return _sets[name]


def the_runs(api, golden, name, alg, lo=0):
    """(batches, default, in line) of a set under an algorithm: computed once, shared by the tests below and left as they are"""
    key = (name, alg, lo)
    if key not in _runs:
        g = the_set(api, golden, name)
        n = len(g["_r1"])
        sp = spans(n) if name in ("var", "mc") else [(a, min(a + 200, n)) for a in range(lo, n, 200)]
        batches = [make_batch(g, a, b) for a, b in sp]
        _runs[key] = (sp, batches, run_batches(api, g["ix"], alg, g["paired"], batches, False), run_batches(api, g["ix"], alg, g["paired"], batches, True))
    return _runs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for g in _sets.values():
        g["ix"].close()
    _sets.clear(); _runs.clear()


def assert_equal_runs(sp, a, b):
    assert len(a) == len(b) == len(sp)
    for (lo, hi), (fa, ca, sa, ta), (fb, cb, sb, tb) in zip(sp, a, b):
        assert np.array_equal(fa, fb), ("records differ", lo, hi, np.argwhere(fa != fb)[:4].tolist())
        assert ca == cb, ("CIGAR words differ", lo, hi)
        assert sa["classes"] == sb["classes"] and sa["early"] == sb["early"] and ta == tb, (lo, hi, sa, sb, ta, tb)
        assert sb["aside"] == 0, (lo, hi, sb)


@gpu
@pytest.mark.parametrize("alg", ["nw", "ksw2"])
@pytest.mark.parametrize("name", ["var", "mc"])
def test_records_equal_the_in_line_launch(api, golden, name, alg):
    """batches of 1, 63 and 200 pairs: records and CIGAR words per read, the class counts and the early list equal between the default and the one launch in line"""
    sp, _, dflt, inl = the_runs(api, golden, name, alg)
    assert {hi - lo for lo, hi in sp} == {1, 63, 200}
    assert_equal_runs(sp, dflt, inl)
    for (lo, hi), (_, _, s, _) in zip(sp, dflt):
        assert sum(s["classes"]) <= hi - lo and s["heavy"] == sum(s["classes"][:4]) and s["light"] == sum(s["classes"][4:]), (lo, hi, s)


@gpu
@pytest.mark.parametrize("alg", ["nw", "ksw2"])
@pytest.mark.parametrize("name", ["var", "mc"])
def test_sam_equals_reference_with_the_heavy_pairs_aside(api, golden, tmp_path, name, alg):
    """the default against the golden SAM, in batches of 200 pairs; the last pass took the aside path"""
    g = the_set(api, golden, name)
    with env(MCX_ORDER_MIN="1"):
        mp = api.Mapper(g["ix"], alg=alg, max_batch_reads=400)
    out = str(tmp_path / "gpu.sam")
    st = mp.map_files(g["r1"], g["r2"], out)
    shape = mp.pass_last_shape()
    mp.close()
    nd, ex = sam_diff(g["sam"][alg], out)
    assert nd == 0, ex
    assert st["simple_pairs"] > 0 and shape["aside"] == 1, (st, shape)


def combos(runs):
    seen = {"aside": 0, "heavy only": 0, "light only": 0, "both": 0}
    for _, _, s, _ in runs:
        seen["aside"] += s["aside"]
        seen["heavy only"] += s["heavy"] > 0 and s["light"] == 0
        seen["light only"] += s["heavy"] == 0 and s["light"] > 0
        seen["both"] += s["heavy"] > 0 and s["light"] > 0
    return seen


@gpu
def test_every_combination_of_the_two_launches_is_seen(api, golden):
    """counted over the batches of each set (the shape does not depend on the algorithm): the aside path taken, a heavy launch beside an empty light one,
    the reverse, and both with pairs.  At most one of the four may be missing in a set, none over both sets.  (Seen: all four in both sets — of the 326 batches
    of `var` 9 with a heavy launch alone, 58 with a light one alone, 24 with both; of `mc`'s 11, 57 and 23; the others hold straight-line pairs only.)"""
    seen = {name: combos(the_runs(api, golden, name, "ksw2")[2]) for name in ("var", "mc")}
    print(seen)
    for name, s in seen.items():
        assert sum(1 for v in s.values() if v == 0) <= 1, (name, s)
    for k in seen["var"]:
        assert seen["var"][k] + seen["mc"][k] > 0, (k, seen)
    for name in seen:  # every batch of the default took the aside path
        runs = the_runs(api, golden, name, "ksw2")[2]
        assert seen[name]["aside"] == len(runs), (name, seen[name], len(runs))


@gpu
def test_single_end_reads(api, golden):
    """the single-end set (a read is a "pair" of one; many of its reads hold an N): 200-read batches, default against in line"""
    sp, batches, dflt, inl = the_runs(api, golden, "se", "ksw2")
    assert_equal_runs(sp, dflt, inl)
    assert all(s["aside"] for _, _, s, _ in dflt) and any(s["heavy"] or s["light"] for _, _, s, _ in dflt)


@gpu
def test_single_end_sam_equals_reference(api, golden, tmp_path):
    g = the_set(api, golden, "se")
    with env(MCX_ORDER_MIN="1"):
        mp = api.Mapper(g["ix"], alg="ksw2", max_batch_reads=400)
    out = str(tmp_path / "gpu.sam")
    mp.map_files(g["r1"], None, out)
    shape = mp.pass_last_shape()
    mp.close()
    nd, ex = sam_diff(g["sam"]["ksw2"], out)
    assert nd == 0, ex
    assert shape["aside"] == 1, shape


@gpu
def test_a_batch_with_a_read_that_holds_n(api, golden):
    """mc's reads with an N (k_simple leaves such a pair to the per-pair kernels, whichever its weight): the batches that hold one, default against in line"""
    sp, batches, dflt, inl = the_runs(api, golden, "mc", "ksw2")
    with_n = [i for i, b in enumerate(batches) if b[2]]
    assert {sp[i][1] - sp[i][0] for i in with_n} >= {63, 200}, [sp[i] for i in with_n]
    assert_equal_runs([sp[i] for i in with_n], [dflt[i] for i in with_n], [inl[i] for i in with_n])
    assert all(dflt[i][2]["aside"] == 1 for i in with_n)


@gpu
def test_the_early_list_comes_from_the_heavy_launch(api, golden):
    """pairs that run over tier 0's capacities while clustering are listed by the heavy launch on the side stream, and the large tier starts from there:
    over the 200-pair batches of `long` (its repeat-rich end included) and the batches of `var` and `mc`, with the aside path taken, the early list is never
    longer than the batch's large-tier pairs (which count the pairs that ran over later as well) nor than its heavy pairs, at least one batch has large-tier
    pairs, and in at least one of those the early list is all of them.  (Seen: pairs 200-400 of `long` and four batches of `var` send one pair each through the
    early list; pairs 0-200 of `long` have one large-tier pair that ran over after clustering, a late pair, and an empty early list.)"""
    rows = []
    for name in ("long", "var", "mc"):
        sp, _, dflt, inl = the_runs(api, golden, name, "ksw2")
        if name == "long":
            assert_equal_runs(sp, dflt, inl)
        rows += [(name, lo, hi, s["aside"], s["early"], t1, s["heavy"]) for (lo, hi), (_, _, s, t1) in zip(sp, dflt)]
    big = [r for r in rows if r[5] > 0]
    print("batches with large-tier pairs (set, lo, hi, aside, early, tier1_pairs, heavy):", big[:40])
    assert all(r[3] == 1 for r in rows)
    assert all(r[4] <= r[5] and r[4] <= r[6] for r in rows), [r for r in rows if r[4] > r[5] or r[4] > r[6]]
    assert big, "no batch reached the large tier"
    assert any(r[4] == r[5] for r in big), big


@gpu
def test_twenty_runs_of_one_batch_give_the_same_records(api, golden):
    """one 200-pair batch twenty times on one context (the insert-size state set back each time): identical every time.  A cheap look for an ordering
    between the two streams that only sometimes holds; it does not replace reading the event edges."""
    best = None  # the 200-pair batch with the most pairs on its smaller side, of the three paired sets
    for name in ("var", "mc", "long"):
        sp, batches, dflt, _ = the_runs(api, golden, name, "ksw2")
        for (lo, hi), b, (_, _, s, _) in zip(sp, batches, dflt):
            if hi - lo == 200 and (best is None or min(s["heavy"], s["light"]) > best[0]):
                best = (min(s["heavy"], s["light"]), name, b)
    g = the_set(api, golden, best[1])
    bases, off, _ = best[2]
    with env(MCX_ORDER_MIN="1"):
        mp = api.Mapper(g["ix"], alg="ksw2", max_batch_reads=400)
    try:
        first = None
        for k in range(20):
            mp.reset()
            aln, cig = mp.map_batch(bases, off, True)
            got = (np.stack([aln[f] for f in FIELDS]), [c.tolist() for c in cig])
            s = mp.pass_last_shape()
            assert s["aside"] == 1 and s["heavy"] > 0 and s["light"] > 0, s
            if first is None:
                first = got
            assert np.array_equal(first[0], got[0]) and first[1] == got[1], k
    finally:
        mp.close()


def test_the_guard_refuses_capacities_below_the_light_bound(tmp_path):
    """light_pairs_fit (mcx_types.h), which the context asks once where tier 0's capacities are made, on capacities around kLightHits: tests/hostemu/aside_guard_check.cpp"""
    exe = str(tmp_path / "aside_guard_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", os.path.join(ROOT, "tests", "hostemu", "aside_guard_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "all cases agree" in r.stdout
