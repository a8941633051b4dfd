"""k_cluster's register path (mapcaller_amd/csrc/mcx_glue.h cluster_read<CAP>, stage_cluster_pair_regs<CAP>; k_cluster in mcx_pipeline.hip): on tier 0 a
read's seeds are fetched once into packed words, sorted and clustered in registers, with the capacity (4, 8, 16, 32) picked per workgroup from the weight
class of its first slot; MCX_CLUSTER_MEM=1 is the memory path (prep_seeds + cluster_seeds in the pair record) everywhere.  Everything here runs with
MCX_ORDER_MIN=1, so that the small batches of the golden sets are listed by weight.

The golden sets `var`, `mc`, `long` and `se`, both algorithms, go through Mapper.map_batch in batches of 1 pair (the first 300 pairs), of 63 pairs (a class
boundary, hence a CAP boundary, inside a workgroup) and of 200 pairs.  Records and CIGAR words per read, pass_last_shape's class counts and early list and
the large-tier pairs per batch must be equal between the default and MCX_CLUSTER_MEM=1 — with the heavy pairs aside (the default: two launches) and with
MCX_CLUSTER_IN_LINE=1 (one launch over all classes).  The default is also held against the golden SAM through map_files (batches of 200 pairs: whole chunks
of the reference's insert-size estimate).  Over the batches of the sets taken together every class from 2 to 5 (CAP 32, 16, 8, 4) and one of the classes
0-1 (the memory path inside the register build) must have held a pair."""
import numpy as np
import pytest

from conftest import sam_diff
from test_cluster_aside_device import FIELDS, env, make_batch, read_seqs, spans

gpu = pytest.mark.gpu
PAIRED_SETS = ("var", "mc", "long")


@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()  # raises if the HIP extension is missing: there is no fallback
    assert a.device_count() >= 1, "no GPU visible"
    return a


_sets, _runs = {}, {}


def the_set(api, golden, name):
    if name not in _sets:
        g = dict(golden[name])
        g["_r1"] = read_seqs(g["r1"])
        g["_r2"] = read_seqs(g["r2"]) if g["paired"] else None
        g["ix"] = api.Index(g["prefix"], device=0, full_sa=True)
        _sets[name] = g
    return _sets[name]


def run_batches(api, ix, alg, paired, batches, mem, in_line):
    """every batch through one fresh context: per batch (record fields, CIGAR words per read, shape of the pass, large-tier pairs of the batch)"""
    kv = {"MCX_ORDER_MIN": "1"}
    if mem:
        kv["MCX_CLUSTER_MEM"] = "1"
    if in_line:
        kv["MCX_CLUSTER_IN_LINE"] = "1"
    out = []
    with env(**kv):
        mp = api.Mapper(ix, alg=alg, max_batch_reads=400)  # (the switches are read when the context is made)
    try:
        for bases, off, _ in batches:
            t1 = mp.stats.tier1_pairs
            if mp.avg[3] % 200:  # a batch starts a new 200-read chunk of the insert-size estimate
                mp.avg[3] += 200 - mp.avg[3] % 200
            aln, cig = mp.map_batch(bases, off, paired)
            out.append((np.stack([aln[f] for f in FIELDS]), [c.tolist() for c in cig], mp.pass_last_shape(), mp.stats.tier1_pairs - t1))
    finally:
        mp.close()
    return out


def the_runs(api, golden, name, alg):
    """(spans, {(mem, in_line): run}) of a set under an algorithm: computed once, shared by the tests below and left as they are"""
    key = (name, alg)
    if key not in _runs:
        g = the_set(api, golden, name)
        sp = spans(len(g["_r1"]))
        batches = [make_batch(g, a, b) for a, b in sp]
        _runs[key] = (sp, {(mem, inl): run_batches(api, g["ix"], alg, g["paired"], batches, mem, inl) for mem in (False, True) for inl in (False, True)})
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
        assert sa["aside"] == sb["aside"], (lo, hi, sa, sb)


@gpu
@pytest.mark.parametrize("in_line", [False, True], ids=["aside", "in_line"])
@pytest.mark.parametrize("alg", ["nw", "ksw2"])
@pytest.mark.parametrize("name", ["var", "mc", "long", "se"])
def test_records_equal_the_memory_path(api, golden, name, alg, in_line):
    """batches of 1, 63 and 200 pairs: the default against MCX_CLUSTER_MEM=1, in two launches and in one"""
    sp, runs = the_runs(api, golden, name, alg)
    assert {hi - lo for lo, hi in sp} == {1, 63, 200}
    assert_equal_runs(sp, runs[(False, in_line)], runs[(True, in_line)])
    assert all(s["aside"] == (0 if in_line else 1) for _, _, s, _ in runs[(False, in_line)])


@gpu
@pytest.mark.parametrize("alg", ["nw", "ksw2"])
@pytest.mark.parametrize("name", ["var", "mc", "se"])
def test_sam_equals_reference(api, golden, tmp_path, name, alg):
    """the default against the golden SAM, in batches of 200 pairs"""
    g = the_set(api, golden, name)
    with env(MCX_ORDER_MIN="1"):
        mp = api.Mapper(g["ix"], alg=alg, max_batch_reads=400)
    out = str(tmp_path / "gpu.sam")
    mp.map_files(g["r1"], g["r2"], out)
    shape = mp.pass_last_shape()
    mp.close()
    nd, ex = sam_diff(g["sam"][alg], out)
    assert nd == 0, ex
    assert shape["aside"] == 1, shape


@gpu
def test_every_capacity_and_the_memory_path_are_seen(api, golden):
    """from pass_last_shape's class counts over the batches (they do not depend on the algorithm): classes 5, 4, 3 and 2 — CAP 4, 8, 16 and 32 — and one of
    the classes 0-1, which keep the memory path, are non-empty in some batch of the sets taken together; and a CAP boundary falls inside a workgroup: a
    batch of 63 pairs that holds pairs of two classes with different capacities.  (Seen, batches with a pair of class 0..5: `var` 0, 17, 15, 28, 57, 50;
    `mc` 0, 12, 11, 31, 59, 45; `long` 7, 3, 25, 221, 83, 0; `se` 0, 1, 11, 10, 16, 83 — class 0 comes from `long` alone.)"""
    seen = [0] * 6
    mixed = 0
    for name in PAIRED_SETS + ("se",):
        sp, runs = the_runs(api, golden, name, "ksw2")
        per_set = [0] * 6
        for (lo, hi), (_, _, s, _) in zip(sp, runs[(False, False)]):
            for k in range(6):
                per_set[k] += s["classes"][k] > 0
            mixed += hi - lo == 63 and len({(0, 0, 32, 16, 8, 4)[k] for k in range(6) if s["classes"][k] > 0}) >= 2
        print(name, "batches with a pair of class 0..5:", per_set)
        seen = [a + b for a, b in zip(seen, per_set)]
    assert all(seen[k] > 0 for k in (2, 3, 4, 5)), seen
    assert seen[0] + seen[1] > 0, seen
    assert mixed > 0
