"""The lane forms of the gapped extension (csrc/mcx_dp_lane.h: one problem per lane; csrc/mcx_dp_lane2.h: two per lane in 16-bit halves) on
the GPU, through mcx_extend_lanes, on problems of the test's choosing: tests/dp_problems.py's seeded set, who shares a lane and a
wavefront with whom, how many groups a wavefront takes in one stretch of scratch.  The reference side is the oracle alone (mcxo_nw /
mcxo_ksw2 / mcxo_ksw2_extz) — never the host build of the same headers, never another device form.  Bar: equality, byte for byte.

Problems compared per parametrisation (either algorithm; none left out but targets over 64 bases with strips of 8):
strips of 16: 1149 in the natural order, 2298 + 384 with unlike neighbours, 579 in ragged lists, 4 x 1149 with reused stretches;
strips of 8: 509, 1018 + 384, 579, 4 x 509; the wavefront form 1149 + 8."""
import os
import random
import subprocess

import pytest

import dp_problems as dp
from conftest import ROOT

pytestmark = pytest.mark.gpu

ALGS = ["nw", "ksw2"]
FORMS = [(1, 8), (1, 16), (2, 8), (2, 16)]  # (problems per lane, columns per strip)


@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    if not os.path.exists(a.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "mapcaller_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    a.lib()  # raises if the HIP extension is missing: there is no fallback
    assert a.device_count() >= 1, "no GPU visible"
    return a


@pytest.fixture(scope="module")
def mapper(api, golden):
    ix = api.Index(golden["toy"]["prefix"], device=0)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=4096)
    yield mp
    mp.close(); ix.close()


def _want(L, alg, probs):
    """[(column string, doubled nw score or 0)] from the oracle."""
    return [(dp.oracle_columns(L, alg, q, t), dp.nw_score2(*dp.oracle_gapped(L, "nw", q, t)) if alg == "nw" else 0) for q, t in probs]


def _lanes(mapper, alg, form, strip, probs, blocks=0, summaries=False):
    return mapper.extend_lanes(alg, form, strip, [q.encode() for q, _ in probs], [t.encode() for _, t in probs], blocks=blocks, summaries=summaries)


def _compare(got, want, probs, what):
    ops, ops_len, score, _ = got
    assert len(ops) == len(want) == len(probs)
    for i, (w, s) in enumerate(want):
        assert ops[i] == w, (what, i, probs[i])
        assert int(ops_len[i]) == len(w), (what, i, probs[i], int(ops_len[i]))
        assert int(score[i]) == s, (what, i, probs[i], int(score[i]), s)
    print(f"{what}: {len(want)} problems compared")


_NATURAL = {}


def _natural(mapper, oracle_lib, alg, form, strip):
    """The whole set in its natural order (with summaries), run once per parametrisation."""
    key = (alg, form, strip)
    if key not in _NATURAL:
        probs = dp.for_strip(dp.problem_set(), strip)
        _NATURAL[key] = (probs, _want(oracle_lib, alg, probs), _lanes(mapper, alg, form, strip, probs, summaries=True))
    return _NATURAL[key]


@pytest.mark.parametrize("form,strip", FORMS)
@pytest.mark.parametrize("alg", ALGS)
def test_lane_forms_equal_the_oracle(mapper, oracle_lib, alg, form, strip):
    """The whole set in its natural order: every column string is the oracle's, ops_len its length, and nw's score twice the score of the
    oracle's alignment, counted in Python from its gapped strings with nw_alignment's parameters (match 1, mismatch -1, a gap's first column
    -1.5, further ones -0.5).  (The kernels report the sweep's s[m][n]; the traceback compares s with r and t for equality without
    following the gap states, so an alignment it walks could in principle score below s[m][n] — on every problem of this set the two
    are equal, which tests/test_hostemu_golden.py shows on the host first.)"""
    probs, want, got = _natural(mapper, oracle_lib, alg, form, strip)
    assert len(probs) == (1149 if strip == 16 else 509)
    _compare(got, want, probs, f"natural order {alg} form {form} strip {strip}")


@pytest.mark.parametrize("form,strip", FORMS)
@pytest.mark.parametrize("alg", ALGS)
def test_unlike_neighbours(mapper, oracle_lib, alg, form, strip):
    """Every problem once in the low half and once in the high half of a lane beside a problem a third of the list away (the one-per-lane form:
    beside other neighbours in the wavefront), and one 300- or 1000-row problem of full width among 127 of 1 x 1 ... 9 x 9: a half, a lane
    whose problem is far smaller than what the group's layout was made for computes cells nobody reads.  The same strings as in the natural
    order, and as the oracle's."""
    probs, want, got = _natural(mapper, oracle_lib, alg, form, strip)
    pairs, idx = dp.unlike_order(probs)
    res = _lanes(mapper, alg, form, strip, pairs)
    _compare(res, [want[i] for i in idx], pairs, "unlike neighbours")
    for k, i in enumerate(idx):
        assert res[0][k] == got[0][i] and int(res[2][k]) == int(got[2][i]), (k, i)
    mixed = dp.mixed_groups(strip)
    assert len(mixed) == 384
    _compare(_lanes(mapper, alg, form, strip, mixed), _want(oracle_lib, alg, mixed), mixed, "one large problem among 127 tiny ones")


@pytest.mark.parametrize("form,strip", FORMS)
@pytest.mark.parametrize("alg", ALGS)
def test_ragged_ends(mapper, oracle_lib, alg, form, strip):
    """Lists that end inside a group: a last group that is partly empty, an odd count (the last lane's high half holds no problem)."""
    probs = dp.for_strip(dp.problem_set(), strip)
    random.Random(dp.SEED + 3).shuffle(probs)
    for n in dp.RAGGED_N:
        part = probs[:n]
        _compare(_lanes(mapper, alg, form, strip, part), _want(oracle_lib, alg, part), part, f"n = {n}")
        probs = probs[n:] + part  # (other problems for the next length)


@pytest.mark.parametrize("form,strip", FORMS)
@pytest.mark.parametrize("alg", ALGS)
def test_stretch_reuse(mapper, oracle_lib, alg, form, strip):
    """One and three wavefronts over the whole set, so that a wavefront takes group after group in the same stretch of scratch — over the
    words the group before left there, laid out for another shape — the large groups ahead of the small ones and the other way round:
    the same results as with a stretch per group."""
    probs, want, got = _natural(mapper, oracle_lib, alg, form, strip)
    for down in (True, False):
        order = sorted(range(len(probs)), key=lambda i: len(probs[i][0]) * len(probs[i][1]), reverse=down)
        part = [probs[i] for i in order]
        for blocks in (1, 3):
            res = _lanes(mapper, alg, form, strip, part, blocks=blocks)
            _compare(res, [want[i] for i in order], part, f"{blocks} wavefront(s), {'large' if down else 'small'} groups first")
            for k, i in enumerate(order):
                assert res[0][k] == got[0][i] and int(res[2][k]) == int(got[2][i]), (k, i)


@pytest.mark.parametrize("form,strip", FORMS)
@pytest.mark.parametrize("alg", ALGS)
def test_summaries(mapper, oracle_lib, alg, form, strip):
    """The DpSummary the walking lane leaves for the finish stage (which builds CIGAR and NM from it): every field against a restatement in
    Python (dp_problems.summary_of) from the oracle's column string and the two input strings alone."""
    probs, want, got = _natural(mapper, oracle_lib, alg, form, strip)
    sums = got[3]
    assert sums is not None and len(sums) == len(probs)
    for i, ((q, t), (cols, _)) in enumerate(zip(probs, want)):
        w = dp.summary_of(cols, q, t)
        g = sums[i]
        for f in ("cols_off", "cols_len", "n", "mis", "switches", "lead_d", "lead_i", "lead_runs", "tail_d", "tail_i", "tail_runs", "n_rle"):
            assert int(g[f]) == w[f], (f, i, q, t, int(g[f]), w[f])
        if w["rle"] is not None:
            assert [int(x) for x in g["rle"][8 - len(w["rle"]):]] == w["rle"], (i, q, t)
    print(f"summaries: {len(probs)} problems compared")


def test_refusals_leave_the_context_usable(api, mapper, oracle_lib):
    """What the lane forms do not take is refused with a message, and the context goes on working."""
    ok = dp.problem_set()[200:330]
    cases = [
        ("outside ACGT", dict(form=1, strip=16), [("ACGT", "ACNT")]),
        ("longer than 256", dict(form=2, strip=16), [("ACGT", "A" * 257)]),
        ("longer than 64", dict(form=1, strip=8), [("ACGT", "A" * 65)]),
        ("longer than 2048", dict(form=2, strip=16), [("A" * 2049, "ACGT")]),
        ("empty", dict(form=1, strip=16), [("", "ACGT")]),
        ("empty", dict(form=2, strip=8), [("ACGT", "")]),
        ("strip must be", dict(form=1, strip=4), [("ACGT", "ACGT")]),
        ("form must be", dict(form=3, strip=16), [("ACGT", "ACGT")]),
    ]
    for alg in ALGS:
        for msg, kw, bad in cases:
            with pytest.raises(api.McxError, match=msg) as e:
                _lanes(mapper, alg, kw["form"], kw["strip"], ok[:5] + bad + ok[5:9])
            assert "(-5)" in str(e.value)  # MCX_ERR_UNSUPPORTED
            _compare(_lanes(mapper, alg, 2, 16, ok), _want(oracle_lib, alg, ok), ok, f"after '{msg}'")


@pytest.mark.parametrize("alg", ALGS)
def test_wavefront_form_equals_the_oracle_on_the_seeded_shapes(api, mapper, oracle_lib, alg):
    """The same set through mcx_extend_batch — k_extend<1|4|16>, one wavefront per problem; the grid straddles 64 / 65 and 256 / 257, where the
    call changes kernels — with what only this form takes: targets of 257, 1023 and 1024 bases, a 2048 x 1024 problem, targets that hold
    an N.  The gapped strings are the oracle's, ksw2's score is mcxo_ksw2_extz's."""
    probs = dp.problem_set() + dp.wavefront_extras()
    assert len(probs) == 1157
    ops, score = mapper.extend(alg, [q.encode() for q, _ in probs], [t.encode() for _, t in probs])
    for i, (q, t) in enumerate(probs):
        assert api.apply_ops(q, t, ops[i]) == dp.oracle_gapped(oracle_lib, alg, q, t), (i, q, t, ops[i])
        if alg == "ksw2":
            assert int(score[i]) == dp.oracle_ksw2_score(oracle_lib, q, t), (i, q, t)
    print(f"wavefront form {alg}: {len(probs)} problems compared")
