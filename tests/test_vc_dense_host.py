"""The CPU stand-in for the variant caller's dense half (tests/hostemu/hostemu_variants.cpp: hostemu_vc_dense over HostProfile)
against numpy restatements that do not go through eval_site, on the synthetic planes of vc_planes.py — and the premises of those
inputs: that the large case puts more than a staging buffer's records into one workgroup's tiles, and more records than the first
sizing of the record list holds.  The GPU kernels are held against this stand-in in test_vc_dense_device.py."""
import numpy as np
import pytest

import vc_planes as vp


def _tiny_cases():
    return {f"tiny{G}-{what}": (lambda G=G, what=what: vp.tiny(G, what)) for G in vp.TINY_SIZES for what in ("gap", "covered", "feature")}


MAKERS = {**_tiny_cases(), "small": vp.small, "large": vp.large, "large-twice": lambda: vp.large(overflow=1_100_000)}
_cases = {}


def case_of(name):
    if name not in _cases:
        if name.startswith("large"):  # (170 MB each: one at a time)
            for k in [k for k in _cases if k.startswith("large")]:
                del _cases[k]
        _cases[name] = MAKERS[name]()
    return _cases[name]


def coverage(case):
    return case.rows[0:4].sum(axis=0, dtype=np.int64)


def boundaries(case):
    """(position, type) of the run-boundary records in (position, type) order: the class of every position from coverage and
    multi_hit alone (0 covered, 1 nothing mapped, 2 multi-mapped reads only), a boundary wherever the class changes."""
    cov = coverage(case)
    cls = np.where(cov > 0, 0, np.where(case.rows[vp.MULTI] == 0, 1, 2))
    prev = np.concatenate([[0], cls[:-1]])
    ends = np.flatnonzero((prev != 0) & (cls != prev))
    starts = np.flatnonzero((cls != 0) & (cls != prev))
    pos = np.concatenate([ends, starts])
    typ = np.concatenate([np.where(prev[ends] == 1, vp.GAP_END, vp.DUP_END), np.where(cls[starts] == 1, vp.GAP_START, vp.DUP_START)])
    order = np.lexsort((typ, pos))
    return pos[order], typ[order]


# (the boundaries do not depend on the switches: the tiny and the large cases once)
@pytest.mark.parametrize("name,switch", [(n, "default") for n in list(_tiny_cases()) + ["large"]] + [("small", s) for s in vp.SWITCHES])
def test_run_boundaries_equal_numpy(hostemu_variants_lib, name, switch):
    case = case_of(name)
    sites, _, _ = vp.host_dense(hostemu_variants_lib, case, switch)
    got = sites[(sites["type"] >= vp.GAP_START) & (sites["type"] <= vp.DUP_END)]
    pos, typ = boundaries(case)
    assert len(got) == len(pos)
    assert np.array_equal(got["pos"], pos) and np.array_equal(got["type"], typ)
    for f in ("geno", "qscore", "DP", "AD_ref", "AD_alt", "pad"):
        assert not got[f].any(), f
    assert (got["alt"] == 0xFF).all()
    assert np.all(np.diff(sites["pos"].astype(np.int64) * 256 + sites["type"]) > 0)  # (position, type) order, nothing twice


@pytest.mark.parametrize("name", ["tiny1-covered", "tiny65-feature", "tiny257-covered", "small", "large"])
def test_block_depths_equal_numpy(hostemu_variants_lib, name):
    case = case_of(name)
    nb = -(-case.G // vp.BLOCK)
    cov = np.concatenate([coverage(case), np.zeros(nb * vp.BLOCK - case.G, dtype=np.int64)])
    want = cov.reshape(nb, vp.BLOCK).sum(axis=1) // vp.BLOCK  # (the partial last block divides by 100 as well)
    first = np.arange(nb, dtype=np.int64) * vp.BLOCK
    last = np.minimum(first + vp.BLOCK - 1, case.G - 1)
    for pos in (first, last):
        _, cols, _ = vp.host_dense(hostemu_variants_lib, case, "default", pos)
        assert np.array_equal(cols["depth"], want)
        assert np.array_equal(cols["v"].astype(np.int64), case.rows[:, pos].T) and np.array_equal(cols["ref"], case.codes[pos])


@pytest.mark.parametrize("name", ["tiny1-covered", "tiny64-feature", "tiny257-gap", "small", "large"])
def test_columns_and_ranges_equal_numpy(hostemu_variants_lib, name):
    case = case_of(name)
    G = case.G
    pos, rq = vp.positions_for(case), vp.ranges_for(case)
    _, cols, vals = vp.host_dense(hostemu_variants_lib, case, "default", pos, rq)
    inside = (pos >= 0) & (pos < G)
    assert np.array_equal(cols["v"][inside].astype(np.int64), case.rows[:, pos[inside]].T) and np.array_equal(cols["ref"][inside], case.codes[pos[inside]])
    assert not cols["v"][~inside].any() and not cols["depth"][~inside].any() and not cols["ref"][~inside].any()
    cov = coverage(case)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    n_none = 0
    for (beg, end, mode), got in zip(rq.tolist(), vals):
        part = cov[max(beg, 0):max(min(end, G - 1) + 1, 0)]
        if mode == 0:
            want = np.uint64(part.sum())
        else:
            want = np.uint64(part[part > 0].min()) if (part > 0).any() else none
            n_none += want == none
        assert got == want, (beg, end, mode)
    assert n_none >= 3  # outside the genome, and (but for the all-covered tiny cases) an uncovered run


def test_alt_columns_are_called_where_they_should_be(hostemu_variants_lib):
    """with default switches: the columns made to sit just over a threshold give a record, the ones just under it (and the ones in a
    block whose depth puts the block's threshold over them) give none"""
    for name in ("small", "large"):
        case = case_of(name)
        sites, _, _ = vp.host_dense(hostemu_variants_lib, case)
        called = set(sites["pos"][sites["type"] == vp.SUB].tolist())
        kinds = vp.snv_kinds()
        assert {k for _, k in case.snvs} >= set(kinds) | {"deep"}
        for p, kind in case.snvs:
            assert (p in called) == (kind != "deep" and kinds[kind][1]), (p, kind)
        assert len(called) == sum(1 for _, k in case.snvs if k != "deep" and kinds[k][1])


def test_premises_of_the_large_case(hostemu_variants_lib):
    """Conditions on the input, read off the stand-in's output: if one fails the INPUT is wrong."""
    G = vp.LARGE_G
    assert vp.per_group(G) >= 3 and vp.n_tiles(G) == 16386 and vp.n_groups(G) == 5462 and G - (vp.n_tiles(G) - 1) * vp.TILE == 44
    assert vp.per_group(vp.SMALL_G) == 1 and vp.n_tiles(vp.SMALL_G) == 40 and vp.SMALL_G % 64 and vp.SMALL_G % 100
    case = case_of("large")
    span = case.span
    counts = {}
    for switch in ("default", "gvcf", "mono"):
        sites, _, _ = vp.host_dense(hostemu_variants_lib, case, switch)
        counts[switch] = len(sites)
        per = np.bincount(sites["pos"] // span, minlength=vp.n_groups(G))
        if switch != "default":  # the mid-loop flush: more than the staging buffer holds within one workgroup's tiles
            for a, b in case.windows:
                assert a % span == 0 and b - a == span and per[a // span] > vp.STAGE, (switch, a, int(per[a // span]))
            print("large", switch, ": records in the windows' groups", [int(per[a // span]) for a, _ in case.windows], "against", vp.STAGE)
        assert len(sites) > vp.cap0(G), switch  # the repeat after overflow
    assert counts["default"] < 1.25 * vp.cap0(G)  # "a little over"
    print("large: records", counts, "against cap0", vp.cap0(G))


def test_premises_of_the_twice_case(hostemu_variants_lib):
    case = case_of("large-twice")
    sites, _, _ = vp.host_dense(hostemu_variants_lib, case)
    assert 2 * vp.cap0(case.G) < len(sites) < 2.5 * vp.cap0(case.G)
    pos, typ = boundaries(case)
    got = sites[(sites["type"] >= vp.GAP_START) & (sites["type"] <= vp.DUP_END)]
    assert np.array_equal(got["pos"], pos) and np.array_equal(got["type"], typ)
