"""-markdup on the device: mcx_bam_dup_units_dev, mcx_dup_resolve_dev and mcx_bam_dup_mark_dev on synthetic records and units, and the file front end on the golden
set mc with duplicates planted in it — all against the rule restated in Python (tests/test_markdup_host.py), which is the specification."""
import ctypes as C
import hashlib
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import test_bgzf_resident as tb
from conftest import ROOT
from test_bai_device import SETTINGS, WrittenBam, environment, query
from test_bai_host import parse_bai
from test_bam_device import bam_stream
from test_bam_host import decode_header
from test_bam_sort_device import no_temporary_file, rec_key, split_records
from test_markdup_host import ONES, end_of, in_range, pack_record, packed_of, read_verdicts, resolve, units_of

EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
GUARD = 64


@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


@pytest.fixture(scope="module")
def mapper(api, golden):
    ix = api.Index(golden["toy"]["prefix"], device=0)
    mp = api.Mapper(ix, alg="nw", max_batch_reads=2000)
    yield mp
    mp.close(); ix.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- units ---------------------------------------------------------------------------------------------------------------------------------
L_SEQS = (0, 1, 15, 16, 17, 255, 256, 5000)


def random_cigar(rng):
    ops = [(rng.randrange(1, 30), op) for op in rng.sample("MIDNP=X", rng.randrange(1, 8))]
    lead = [(rng.randrange(1, 9), op) for op in rng.choice(("", "S", "H", "HS"))]
    trail = [(rng.randrange(1, 9), op) for op in rng.choice(("", "S", "H", "SH"))]
    return lead + ops + trail


def random_dup_record(rng, k):
    """records of 38 bytes (a one-byte name, nothing else) to beyond 5000; few positions, so that ends meet; every l_seq of L_SEQS; every CIGAR operation"""
    kind = k % 10
    if kind == 0:
        return pack_record(rng.choice((0, 1)), rng.randrange(100, 104), rng.choice((0, 0x10)))
    flag = rng.choice((0, 0x10, 0x63, 0x93, 0x53)) | (4 if kind == 1 else 0)
    ref_id = -1 if kind == 1 and rng.random() < 0.5 else rng.choice((0, 0, 1, 7))
    l_seq = L_SEQS[k % len(L_SEQS)] if kind != 2 else rng.randrange(0, 300)
    qual = bytes(rng.choice((0, 14, 15, 16, 40, 41, 93, 0xff)) for _ in range(l_seq))
    return pack_record(ref_id, rng.randrange(100, 104), flag, random_cigar(rng), qual, name=b"q%d" % k, extra=b"NMC\1" * rng.randrange(0, 3))


def make_groups(rng, n):
    """n groups of 0, 1 and 3 records"""
    groups = []
    for g in range(n):
        take = 1 if n < 3 else rng.choice((0, 1, 1, 1, 1, 3))
        groups.append([random_dup_record(rng, 10 * g + j if j else g) for j in range(take)])
    return groups


def want_units(api, groups, paired):
    out = np.zeros(len(groups) // 2 if paired else len(groups), dtype=api.DUP_UNIT_DTYPE)
    for u, (kind, key, score, reads) in enumerate(units_of(groups, paired)):
        if kind == "pair":
            out[u] = (packed_of(key[0]), packed_of(key[1]), score, api.DUP_PAIR)
        elif kind == "fragment":
            out[u] = (packed_of(key), ONES, score, api.DUP_FRAGMENT | (api.DUP_SECOND_MATE if paired and reads[0] & 1 else 0))
        else:
            out[u] = (ONES, ONES, 0, api.DUP_NONE)
    return out


def run_units(api, mp, groups, paired, shift=0, want_rc=0, data=None, grp_off=None):
    """the call between guard bytes: (rc, units as a numpy array, n_units, the absolute address of the records)"""
    import torch
    if data is None:
        data = b"".join(r for g in groups for r in g)
        grp_off = np.cumsum([0] + [sum(len(r) for r in g) for g in groups]).astype(np.uint64)
    n_bytes, n_groups = len(data), len(grp_off) - 1
    src = torch.full((GUARD + 16 + n_bytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    s0 = GUARD + shift
    if n_bytes:
        src[s0:s0 + n_bytes] = dev(np.frombuffer(data, dtype=np.uint8).copy())
    off = dev(np.asarray(grp_off, dtype=np.uint64).view(np.int64).copy())
    most = max(1, n_groups)
    out = torch.full((GUARD + 24 * most + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = C.c_uint64(99)
    rc = api.lib().mcx_bam_dup_units_dev(mp._h, src.data_ptr() + s0, n_bytes, off.data_ptr(), n_groups, int(paired), out.data_ptr() + GUARD, C.byref(n))
    assert rc == want_rc, api.lib().mcx_last_error()
    got = out.cpu().numpy()
    used = 24 * n.value
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + used:] == 0xA5).all()  # not a byte outside the units
    assert src.cpu().numpy()[s0:s0 + n_bytes].tobytes() == data and (src.cpu().numpy()[:s0] == 0x5A).all()
    return rc, got[GUARD:GUARD + used].copy().view(api.DUP_UNIT_DTYPE), n.value, src.data_ptr() + s0


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_the_units_are_the_rule(api, mapper, n, paired):
    rng = random.Random(500 + n)
    groups = make_groups(rng, n)
    if paired and n % 2:  # pairs come two by two
        rc, got, n_units, _ = run_units(api, mapper, groups, True, want_rc=api.ERR_ARG)
        assert n_units == 0
        groups.append([])
    records = [r for g in groups for r in g]
    assert all(in_range(end_of(g[0])) for g in groups if g and not struct.unpack_from("<H", g[0], 18)[0] & 4)
    if n >= 1000:  # the stream is what the issue asks for
        assert {len(g) for g in groups} == {0, 1, 3} and min(map(len, records)) == 38 and max(map(len, records)) > 5000
        assert {struct.unpack_from("<I", r, 20)[0] for r in records} >= set(L_SEQS)
        assert {w & 15 for r in records for w in struct.unpack_from("<%dI" % struct.unpack_from("<H", r, 16)[0], r, 36 + r[12])} == set(range(9))
        kinds = [u[0] for u in units_of(groups, paired)]
        assert kinds.count("fragment") > 50 and kinds.count(None) > 5 and (not paired or kinds.count("pair") > 100)
        if paired:  # a mate without a record, on either side
            assert any(not groups[2 * u] and groups[2 * u + 1] for u in range(len(groups) // 2)) and any(groups[2 * u] and not groups[2 * u + 1] for u in range(len(groups) // 2))
    want = want_units(api, groups, paired)
    classes = set()
    for shift in range(16) if n in (65, 1000) else (0, 5):
        rc, got, n_units, at = run_units(api, mapper, groups, paired, shift=shift)
        assert n_units == len(want)
        assert got.tobytes() == want.tobytes(), [k for k in range(len(want)) if got[k] != want[k]][:5]
        for r in records:
            classes.add(at % 16)
            at += len(r)
    if n >= 65:
        assert len(classes) == 16  # every offset class mod 16
    assert mapper.markdup_last_ms()[0] >= 0


@pytest.mark.gpu
def test_the_python_wrappers(api, mapper):
    groups = make_groups(random.Random(9), 64)
    data = b"".join(r for g in groups for r in g)
    recs = dev(np.frombuffer(data, dtype=np.uint8).copy())
    off = dev(np.cumsum([0] + [sum(len(r) for r in g) for g in groups]).astype(np.int64))
    units = mapper.bam_dup_units(recs, off, True)
    assert units.cpu().numpy().tobytes() == want_units(api, groups, True).tobytes()
    dup = mapper.dup_resolve(units).cpu().numpy()
    assert [bool(v) for v in dup] == resolve(units_of(groups, True))[0]
    rec_off = dev(np.cumsum([0] + [len(r) for g in groups for r in g]).astype(np.int64))
    marks = np.array([k % 3 == 0 for g in groups for k, _ in enumerate(g)], dtype=np.uint8)
    mapper.bam_dup_mark(recs, rec_off, dev(marks))
    assert recs.cpu().numpy().tobytes() == b"".join(marked(r, m) for r, m in zip([r for g in groups for r in g], marks))
    assert len(mapper.markdup_last_ms()) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["chain leaves its group", "block_size 8", "offsets do not reach n_bytes", "offsets descend", "QUAL leaves its record", "CIGAR leaves its record",
                                 "a later record of a group is cut short", "refID beyond the packing", "u5 beyond the packing"])
def test_broken_input_is_an_argument_error_and_writes_nothing(api, mapper, how):
    rng = random.Random(3)
    records = [random_dup_record(rng, k + 2 if k % 10 < 2 else k) for k in range(40)]
    ends = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
    words = b"chain"
    if how == "chain leaves its group":
        ends[20] += 5
    elif how == "block_size 8":
        records[7] = struct.pack("<I", 8) + records[7][4:]
    elif how == "offsets do not reach n_bytes":
        ends = ends[:-1]
    elif how == "offsets descend":
        ends[10], ends[11] = ends[11], ends[10]
    elif how == "QUAL leaves its record":
        r = pack_record(0, 5, 0, [(10, "M")], bytes(40))
        records[12] = r[:20] + struct.pack("<I", 41) + r[24:]  # l_seq says one base more than the record holds
        ends = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
    elif how == "CIGAR leaves its record":
        r = pack_record(0, 5, 0, [(10, "M")], b"")
        records[12] = r[:16] + struct.pack("<H", 3) + r[18:]
        ends = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
    elif how == "a later record of a group is cut short":
        r = pack_record(0, 5, 0, [(10, "M")], bytes(40))
        records[13] = r[:20] + struct.pack("<I", 4000) + r[24:]
        ends = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
        ends = np.delete(ends, 13)  # records 12 and 13 are one group: the second record is the broken one
    else:
        records[12] = pack_record((1 << 24) - 1, 5, 0, [(10, "M")], bytes(4)) if how.startswith("refID") else pack_record(0, 5, 0, [((1 << 28) - 1, "S")] * 1025 + [(1, "M")], bytes(4))
        ends = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
        words = b"packed end"
    data = b"".join(records)
    for paired in (False, True):
        if paired and (len(ends) - 1) % 2:
            continue
        rc, got, n_units, _ = run_units(api, mapper, None, paired, shift=3, want_rc=api.ERR_ARG, data=data, grp_off=ends)
        assert n_units == 0 and words in api.lib().mcx_last_error()


@pytest.mark.gpu
def test_null_arguments_and_the_empty_call(api, mapper):
    import torch
    L = api.lib()
    d = torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    n = C.c_uint64(5)
    assert L.mcx_bam_dup_units_dev(mapper._h, d.data_ptr(), 100, d.data_ptr(), 0, 1, d.data_ptr() + 128, C.byref(n)) == 0 and n.value == 0
    assert L.mcx_bam_dup_units_dev(None, d.data_ptr(), 100, d.data_ptr(), 2, 1, d.data_ptr(), C.byref(n)) == api.ERR_ARG
    assert L.mcx_bam_dup_units_dev(mapper._h, None, 100, d.data_ptr(), 2, 1, d.data_ptr(), C.byref(n)) == api.ERR_ARG
    assert L.mcx_bam_dup_units_dev(mapper._h, d.data_ptr(), 100, None, 2, 1, d.data_ptr(), C.byref(n)) == api.ERR_ARG
    assert L.mcx_bam_dup_units_dev(mapper._h, d.data_ptr(), 100, d.data_ptr(), 2, 1, None, C.byref(n)) == api.ERR_ARG
    assert L.mcx_bam_dup_units_dev(mapper._h, d.data_ptr(), 100, d.data_ptr(), 2, 1, d.data_ptr(), None) == api.ERR_ARG
    assert L.mcx_dup_resolve_dev(mapper._h, d.data_ptr(), 0, d.data_ptr()) == 0 and L.mcx_dup_resolve_dev(None, d.data_ptr(), 1, d.data_ptr()) == api.ERR_ARG
    assert L.mcx_dup_resolve_dev(mapper._h, None, 1, d.data_ptr()) == api.ERR_ARG and L.mcx_dup_resolve_dev(mapper._h, d.data_ptr(), 1, None) == api.ERR_ARG
    assert L.mcx_dup_resolve_dev(mapper._h, d.data_ptr(), 1 << 30, d.data_ptr()) == api.ERR_CAPACITY and b"bytes" in L.mcx_last_error()
    assert L.mcx_bam_dup_mark_dev(mapper._h, d.data_ptr(), 100, d.data_ptr(), 0, d.data_ptr()) == 0 and L.mcx_bam_dup_mark_dev(None, d.data_ptr(), 100, d.data_ptr(), 1, d.data_ptr()) == api.ERR_ARG
    assert L.mcx_bam_dup_mark_dev(mapper._h, None, 100, d.data_ptr(), 1, d.data_ptr()) == api.ERR_ARG and L.mcx_bam_dup_mark_dev(mapper._h, d.data_ptr(), 100, d.data_ptr(), 1, None) == api.ERR_ARG
    ms = (C.c_float * 3)()
    assert L.mcx_markdup_last_ms(mapper._h, None) == api.ERR_ARG and L.mcx_markdup_last_ms(None, ms) == api.ERR_ARG
    assert bool((d == 0xA5).all())


# ---- resolve --------------------------------------------------------------------------------------------------------------------------------
def unit_array(api, units):
    """units: (kind, end0, end1, score) with kind 'pair' / 'fragment' / None"""
    out = np.zeros(len(units), dtype=api.DUP_UNIT_DTYPE)
    for u, (kind, e0, e1, score) in enumerate(units):
        out[u] = (min(e0, e1), max(e0, e1), score, api.DUP_PAIR) if kind == "pair" else (e0, ONES, score, api.DUP_FRAGMENT | (4 if u % 3 == 0 else 0)) if kind == "fragment" else (ONES, ONES, 0, 0)
    return out


def restated(units):
    return resolve([(kind, (min(e0, e1), max(e0, e1)) if kind == "pair" else e0, score, []) for kind, e0, e1, score in units])


def run_resolve(api, mp, arr, want_rc=0):
    import torch
    n = len(arr)
    d_units = dev(arr.view(np.uint8).copy()) if n else torch.zeros(24, dtype=torch.uint8, device="cuda")
    out = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = api.lib().mcx_dup_resolve_dev(mp._h, d_units.data_ptr(), n, out.data_ptr() + GUARD)
    assert rc == want_rc, api.lib().mcx_last_error()
    got = out.cpu().numpy()
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + n:] == 0xA5).all()
    assert d_units.cpu().numpy().tobytes()[:24 * n] == arr.tobytes()
    return got[GUARD:GUARD + n]


def end(ref_id, u5, reverse):
    return packed_of((ref_id, u5, reverse))


def random_units(rng, n, n_ends, scores, kinds=("pair", "pair", "fragment", None)):
    pool = [end(rng.choice((0, 1)), rng.randrange(-5, 1000), rng.randrange(2)) for _ in range(n_ends)]
    return [(rng.choice(kinds), rng.choice(pool), rng.choice(pool), rng.choice(scores)) for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1000, 100000])
def test_the_resolve_is_the_rule(api, mapper, n):
    rng = random.Random(n)
    for n_ends, scores in ((max(2, n // 20), (0, 7, 7, 300, 0xFFFFFFFF)), (4 * n + 8, (5,))):  # ends that meet often, scores that tie; then hardly any meeting
        units = random_units(rng, n, n_ends, scores)
        got = run_resolve(api, mapper, unit_array(api, units))
        want, groups = restated(units)
        assert [bool(v) for v in got] == want
        assert set(got.tolist()) <= {0, 1}
    assert mapper.markdup_last_ms()[1] >= 0


@pytest.mark.gpu
def test_the_resolve_on_the_cases_that_matter(api, mapper):
    rng = random.Random(12)
    a, b, c = end(0, 100, 0), end(0, 300, 1), end(0, 500, 1)
    check = lambda units: np.testing.assert_array_equal(run_resolve(api, mapper, unit_array(api, units)).astype(bool), restated(units)[0])  # noqa: E731
    # all keys distinct: no duplicate
    units = [("pair", end(0, k, 0), end(0, k + 200, 1), 5) for k in range(300)] + [("fragment", end(1, k, 0), ONES, 5) for k in range(300)]
    assert not any(restated(units)[0])
    check(units)
    # one key holds half of all units
    units = [("pair", a, b, rng.choice((1, 2, 3))) if k % 2 else ("pair", end(0, k, 0), end(0, k + 1, 1), 1) for k in range(2000)]
    assert sum(restated(units)[0]) == 999
    check(units)
    # ties decided by number (the first of the best stays), and by score (the best is not the first)
    units = [("pair", a, b, 10), ("pair", b, a, 10), ("pair", a, b, 10), ("pair", a, c, 7), ("pair", a, c, 9), ("pair", a, c, 8), ("pair", a, c, 9)]
    assert restated(units)[0] == [False, True, True, True, False, True, True]
    check(units)
    # keys that agree in the first end only, or in the second end only
    units = [("pair", a, b, 1), ("pair", a, c, 1), ("pair", end(0, 101, 0), b, 1)]
    assert not any(restated(units)[0])
    check(units)
    # ends that differ only in strand, only in refID, only in the top bit of u5 (the bias sets bit 38 for u5 >= 0)
    for x, y in ((end(0, 100, 0), end(0, 100, 1)), (end(0, 100, 0), end(1, 100, 0)), (end(0, 7, 0), end(0, 7 - (1 << 38), 0)), (end(0, 0, 0), end((1 << 24) - 2, 0, 0))):
        assert x != y
        units = [("pair", x, b, 1), ("pair", y, b, 2), ("fragment", x, ONES, 1), ("fragment", y, ONES, 1), ("fragment", x, ONES, 3)]
        check(units)
        units = [("fragment", x, ONES, 1), ("fragment", y, ONES, 1), ("fragment", x, ONES, 3), ("fragment", y, ONES, 1)]
        assert restated(units)[0] == [True, False, False, True]
        check(units)
    # a fragment on a pair's first end, on its second end, and on neither; a better fragment does not save it
    units = [("pair", a, b, 1), ("fragment", a, ONES, 99), ("fragment", b, ONES, 99), ("fragment", c, ONES, 1), ("fragment", c, ONES, 2), (None, ONES, ONES, 0), ("pair", a, b, 0)]
    assert restated(units) == ([False, True, True, True, False, False, True], 4)
    check(units)
    # fragment groups without any pair
    units = [("fragment", rng.choice((a, b, c)), ONES, rng.choice((1, 2))) for _ in range(500)]
    assert sum(restated(units)[0]) == 497
    check(units)


@pytest.mark.gpu
def test_a_unit_of_no_kind_is_an_argument_error(api, mapper):
    arr = unit_array(api, [("pair", 5, 9, 1), ("fragment", 5, ONES, 1), (None, ONES, ONES, 0)] * 30)
    for bad in (3, 8, 2 | 4, 4):
        arr2 = arr.copy()
        arr2["kind"][40] = bad
        got = run_resolve(api, mapper, arr2, want_rc=api.ERR_ARG)
        assert (got == 0xA5).all()


# ---- mark -----------------------------------------------------------------------------------------------------------------------------------
def marked(rec, yes):
    return rec[:19] + bytes([rec[19] | 4]) + rec[20:] if yes else rec


def run_mark(api, mp, records, marks, shift, want_rc=0, rec_off=None, times=1):
    import torch
    data = b"".join(records)
    n_bytes = len(data)
    buf = torch.full((GUARD + 16 + n_bytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    s0 = GUARD + shift
    buf[s0:s0 + n_bytes] = dev(np.frombuffer(data, dtype=np.uint8).copy())
    if rec_off is None:
        rec_off = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
    off, d_marks = dev(np.asarray(rec_off, dtype=np.uint64).view(np.int64).copy()), dev(np.asarray(marks, dtype=np.uint8))
    torch.cuda.synchronize()
    for _ in range(times):
        rc = api.lib().mcx_bam_dup_mark_dev(mp._h, buf.data_ptr() + s0, n_bytes, off.data_ptr(), len(rec_off) - 1, d_marks.data_ptr())
        assert rc == want_rc, api.lib().mcx_last_error()
    got = buf.cpu().numpy()
    assert (got[:s0] == 0x5A).all() and (got[s0 + n_bytes:] == 0x5A).all()
    return got[s0:s0 + n_bytes].tobytes(), buf.data_ptr() + s0


@pytest.mark.gpu
def test_the_marks_set_one_bit_and_nothing_else(api, mapper):
    rng = random.Random(21)
    records = [random_dup_record(rng, k) for k in range(300)]
    records = [r[:18] + struct.pack("<H", rng.choice((0, 0x10, 0x400, 0x463, 0xFBFF, 0xFFFF, 0x93))) + r[20:] if k % 4 == 0 else r for k, r in enumerate(records)]
    marks = [rng.choice((0, 0, 1, 255)) for _ in records]
    want = b"".join(marked(r, m) for r, m in zip(records, marks))
    assert want != b"".join(records)
    classes = set()
    for shift in range(16):
        got, at = run_mark(api, mapper, records, marks, shift, times=1 + shift % 2)  # (marking twice is harmless)
        assert got == want
        for r in records:
            classes.add(at % 16)
            at += len(r)
    assert len(classes) == 16
    changed = [(a, b) for a, b in zip(b"".join(records), want) if a != b]
    assert changed and all(a | 4 == b for a, b in changed)
    assert run_mark(api, mapper, records, [0] * len(records), 3)[0] == b"".join(records)
    assert mapper.markdup_last_ms()[2] >= 0
    # offsets that descend, leave n_bytes, or leave less than the 20 bytes that end with the flag: nothing is written
    off = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
    for k, v in ((10, off[12]), (300, off[300] + 1), (50, off[49] + 19)):
        bad = off.copy()
        bad[k] = v
        assert run_mark(api, mapper, records, [1] * len(records), 5, want_rc=api.ERR_ARG, rec_off=bad)[0] == b"".join(records)


# ---- the front end on the golden set mc, duplicates planted -------------------------------------------------------------------------------
def fastq_records(path):
    lines = open(path, "rb").read().split(b"\n")
    return [lines[k:k + 4] for k in range(0, len(lines) - 1, 4)]


def planted(g, tmp, single=False):
    """the golden reads with copies of 70 pairs under new names spread through the file: copies with the original's qualities (ties, settled by number), with lower
    and with higher ones (settled by score), and copies whose second read is replaced by bases that lie nowhere (a fragment beside the pair it came from)"""
    rng = random.Random(4242)
    r1, r2 = fastq_records(g["r1"]), fastq_records(g["r2"])
    assert len(r1) == len(r2) == 2000
    pairs = [(a, b) for a, b in zip(r1, r2)]
    out = list(pairs)
    for k, src in enumerate(rng.sample(range(len(pairs)), 70)):
        for j in range(rng.choice((1, 2, 3))):
            a, b = [list(x) for x in pairs[src]]
            how = (k + j) % 4
            for m, x in enumerate((a, b)):
                x[0] = b"@copy%d_%d_of_%d/%d" % (k, j, src, m + 1)
                if how == 1:
                    x[3] = bytes(max(33 + 2, q - 9) for q in x[3])
                elif how == 2:
                    x[3] = bytes(min(126, q + 3) for q in x[3])
            if how == 3:
                b[1] = bytes(rng.choice(b"ACGT") for _ in b[1])
            out.insert(rng.randrange(len(out) + 1), (a, b))
    files = [str(tmp / "dup_1.fq"), str(tmp / "dup_2.fq")]
    for k, f in enumerate(files):
        open(f, "wb").write(b"".join(b"\n".join(p[k]) + b"\n" for p in out))
    return (files[0], None) if single else tuple(files)


def run_front(api, g, files, out, batch, markdup=True, sort=True, index=False, **kw):
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=batch)
    header = api.bam_header(ix, sorted=sort)
    try:
        st = mp.map_files(files[0], files[1], out, bam=True, sort=sort, markdup=markdup, index=index, **kw)
        return st, mp.last_route(), mp.sort_stats(), mp.markdup_stats(), header
    finally:
        mp.close(); ix.close()


_MC = {}


def mc_runs(api, golden, tmp_path_factory, single=False):
    """once per module: the planted files, the plain -bam run's records in read order, the restatement's verdicts, the -bam -sort stream, and the -markdup stream it must be"""
    if single not in _MC:
        g = golden["mc"]
        tmp = tmp_path_factory.mktemp("markdup_mc")
        files = planted(g, tmp, single)
        with environment(MCX_BGZF_BLOCK="4096", MCX_SORT_CHUNK="200000"):
            plain, sorted_ = str(tmp / "plain.bam"), str(tmp / "sorted.bam")
            st, route, _, _, header = run_front(api, g, files, plain, 1000, markdup=False, sort=False)
            stream = bam_stream(plain)[0]
            records = split_records(stream, len(header))
            assert len(records) == st["reads"] and not route[0] & api.ROUTE_MARKDUP  # a record a read, in read order
            st, route, sort_stats, _, sorted_header = run_front(api, g, files, sorted_, 1000, markdup=False)
            sorted_stream = bam_stream(sorted_)[0]
        verdict, units, dup, n_groups = read_verdicts([[r] for r in records], not single)
        order = sorted(range(len(records)), key=lambda k: rec_key(records[k]))  # (stable)
        assert sorted_stream == sorted_header + b"".join(records[k] for k in order)
        want = sorted_header + b"".join(marked(records[k], verdict[k]) for k in order)
        _MC[single] = dict(files=files, records=records, verdict=verdict, units=units, dup=dup, groups=n_groups, sorted=sorted_stream, want=want, header=sorted_header, tmp=tmp,
                           runs=sort_stats["runs"])
    return _MC[single]


def counts(m):
    kinds = [u[0] for u in m["units"]]
    return dict(pairs=kinds.count("pair"), duplicate_pairs=sum(d for d, k in zip(m["dup"], kinds) if k == "pair"), fragments=kinds.count("fragment"),
                duplicate_fragments=sum(d for d, k in zip(m["dup"], kinds) if k == "fragment"), groups=m["groups"])


@pytest.mark.gpu
def test_the_planted_input_has_what_the_check_needs(api, golden, tmp_path_factory):
    m = mc_runs(api, golden, tmp_path_factory)
    units, dup = m["units"], m["dup"]
    by_key = {}
    for u, (kind, key, score, _) in enumerate(units):
        if kind == "pair":
            by_key.setdefault(key, []).append(u)
    shared = [v for v in by_key.values() if len(v) > 1]
    assert sum(dup[u] for v in shared for u in v) >= 50  # duplicate pair units
    assert m["runs"] >= 3 and any(len({2 * u // 1000 for u in v}) > 1 for v in shared)  # a group whose members lie in different runs (a run is a part of 1000 reads)
    pair_ends = {e for key in by_key for e in key}
    assert any(kind == "fragment" and key in pair_ends and dup[u] for u, (kind, key, _, _) in enumerate(units))  # a fragment beaten by a pair
    best = lambda v: max(units[u][2] for u in v)  # noqa: E731
    assert any(sum(units[u][2] == best(v) for u in v) > 1 for v in shared)  # a tie settled by number
    assert any(units[v[0]][2] < best(v) for v in shared)  # a tie settled by score: the first is not the best
    assert all(sum(not dup[u] for u in v) == 1 for v in by_key.values())  # exactly one unflagged unit in every group
    assert m["want"] != m["sorted"] and len(m["want"]) == len(m["sorted"])
    assert not any(v and struct.unpack_from("<H", r, 18)[0] & 4 for r, v in zip(m["records"], m["verdict"]))  # unplaced records are never flagged


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2])
def test_the_marked_file_is_the_sorted_file_with_exactly_those_bits(api, golden, tmp_path_factory, tmp_path, k):
    m = mc_runs(api, golden, tmp_path_factory)
    batch, chunk = SETTINGS[k]
    out = str(tmp_path / "o.bam")
    with environment(MCX_BGZF_BLOCK="4096", MCX_SORT_CHUNK=chunk):
        st, route, sort_stats, stats, header = run_front(api, golden["mc"], m["files"], out, batch, index=k == 2)
    assert route[0] & api.ROUTE_MARKDUP and route[0] & api.ROUTE_SORT and (k != 1) == (sort_stats["runs"] >= 3 and sort_stats["chunks"] >= 3)
    stream = bam_stream(out)[0]
    assert stream == m["want"]
    diff = [(a, b) for a, b in zip(stream, m["sorted"]) if a != b]
    assert len(diff) == sum(m["verdict"]) and all(a == b | 4 for a, b in diff)  # the unmarked file, but for that one bit
    seconds = stats.pop("seconds")
    assert stats == counts(m) and seconds > 0
    assert no_temporary_file(tmp_path)
    if k == 2:  # -index reads marked records: 50 regions, each against a scan
        bam = WrittenBam(out, header)
        index = parse_bai(open(out + ".bai", "rb").read())
        assert index == bam.restated()
        lens = [n for _, n in decode_header(header)[1]]
        offsets, at = [], len(header)
        for r in split_records(bam.stream, at):
            offsets.append(at)
            at += len(r)
        rng = random.Random(8)
        for _ in range(50):
            tid = rng.randrange(len(lens))
            beg = rng.randrange(lens[tid])
            stop = min(lens[tid], beg + rng.choice((1, 100, 1000, 20000, lens[tid])))
            assert sorted(set(query(bam, index, tid, beg, stop))) == [o for o, r in zip(offsets, bam.records) if r[0] == tid and r[1] < stop and r[2] > beg]


@pytest.mark.gpu
def test_single_end(api, golden, tmp_path_factory, tmp_path):
    m = mc_runs(api, golden, tmp_path_factory, single=True)
    assert {u[0] for u in m["units"]} <= {"fragment", None} and sum(m["dup"]) >= 50
    out = str(tmp_path / "se.bam")
    with environment(MCX_BGZF_BLOCK="4096", MCX_SORT_CHUNK="100000"):
        st, route, sort_stats, stats, _ = run_front(api, golden["mc"], m["files"], out, 400)
    assert sort_stats["runs"] >= 3 and bam_stream(out)[0] == m["want"]
    stats.pop("seconds")
    assert stats == counts(m) and stats["pairs"] == 0


@pytest.mark.gpu
def test_the_resident_route(api, golden, tmp_path_factory, tmp_path):
    m = mc_runs(api, golden, tmp_path_factory)
    files = []
    for k, f in enumerate(m["files"]):
        files.append(str(tmp_path / f"dup_{k + 1}.fq.gz"))
        tb.write_bgzf(files[-1], open(f, "rb").read(), 3000)
    out = str(tmp_path / "res.bam")
    with environment(MCX_BGZF_BLOCK="4096", MCX_SORT_CHUNK="100000", MCX_RESIDENT_LAUNCH_BYTES="65536"):
        st, route, sort_stats, stats, _ = run_front(api, golden["mc"], files, out, 800, device_inflate=True, device_parse=True)
    everything = tb.ALL_FOUR | api.ROUTE_BGZF | api.ROUTE_BAM | api.ROUTE_SORT | api.ROUTE_MARKDUP
    assert route == (everything, everything)
    assert bam_stream(out)[0] == m["want"] and no_temporary_file(tmp_path)


@pytest.mark.gpu
def test_two_runs_give_the_same_file(api, golden, tmp_path_factory, tmp_path):
    m = mc_runs(api, golden, tmp_path_factory)
    digests = []
    with environment(MCX_SORT_CHUNK="300000"):
        for k in range(2):
            out = str(tmp_path / f"run{k}.bam")
            run_front(api, golden["mc"], m["files"], out, 1000)
            digests.append(hashlib.md5(open(out, "rb").read()).hexdigest())
    assert digests[0] == digests[1]


@pytest.mark.gpu
def test_the_temporary_file_is_gone_after_a_run_that_fails(api, golden, tmp_path_factory, tmp_path):
    m = mc_runs(api, golden, tmp_path_factory)
    text = open(m["files"][1], "rb").read()
    cut = str(tmp_path / "r2_cut.fq")
    open(cut, "wb").write(text[:len(text) // 2 + 7])  # file 2 ends inside a record, after the temporary file was made
    out = str(tmp_path / "cut.bam")
    open(out + ".bai", "wb").write(b"an index an earlier run left here")
    ix = api.Index(golden["mc"]["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=400)
    with pytest.raises(Exception):
        mp.map_files(m["files"][0], cut, out, bam=True, sort=True, markdup=True, index=True)
    assert no_temporary_file(tmp_path) and not os.path.exists(out + ".bai")
    assert set(mp.markdup_stats().values()) == {0}
    mp.close(); ix.close()


@pytest.mark.gpu
def test_the_refusals(api, golden, tmp_path):
    g = golden["toy"]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    L = api.lib()
    out = str(tmp_path / "refused.bam")

    def call(mp, device_sam):
        fo = api.FileOpts()
        L.mcx_file_opts_default(C.byref(fo))
        fo.device_sam = device_sam
        st = api.Stats()
        rc = L.mcx_map_files_ex(mp._h, g["r1"].encode(), g["r2"].encode(), C.byref(fo), out.encode(), C.byref(st))
        err = L.mcx_last_error()
        assert not os.path.exists(out) and no_temporary_file(tmp_path)
        return rc, err

    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1000)
    rc, err = call(mp, api.SAM_MARKDUP | api.SAM_BAM)
    assert rc == api.ERR_UNSUPPORTED and b"needs -sort" in err
    mp.close()
    mp = api.Mapper(ix, alg="ksw2", multi=True, max_batch_reads=1000)
    rc, err = call(mp, api.SAM_MARKDUP | api.SAM_SORT | api.SAM_BAM)
    assert rc == api.ERR_UNSUPPORTED and b"-m" in err
    mp.close(); ix.close()
    assert api.SAM_MARKDUP == 32 and api.ROUTE_MARKDUP == 256


@pytest.mark.gpu
def test_cli_markdup(api, golden, tmp_path_factory, tmp_path):
    m = mc_runs(api, golden, tmp_path_factory)
    g = golden["mc"]
    out = str(tmp_path / "cli.bam")
    args = [EXE, "-i", g["prefix"], "-f", m["files"][0], "-f2", m["files"][1], "-alg", "ksw2", "-no_vcf", "-batch", "1000"]
    env = dict(os.environ, MCX_TIMING="1", MCX_BGZF_BLOCK="4096", MCX_SORT_CHUNK="200000", TMPDIR=str(tmp_path))
    r = subprocess.run(args + ["-bam", out, "-sort", "-markdup"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    c = counts(m)
    assert b"[mcx_map_files] markdup:" in r.stderr and b"markdup: %d of %d pairs and %d of %d single reads are duplicates, in %d groups\n" % (
        c["duplicate_pairs"], c["pairs"], c["duplicate_fragments"], c["fragments"], c["groups"]) in r.stderr
    assert bam_stream(out)[0] == m["want"]
    r = subprocess.run(args + ["-bam", out, "-sort"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)  # without the switch: the unmarked file, no word of it
    assert r.returncode == 0 and bam_stream(out)[0] == m["sorted"] and b"markdup" not in r.stderr
    bad = str(tmp_path / "bad.bam")
    for extra, words in ((["-bam", bad, "-markdup"], b"needs -bam -sort"), (["-sam", bad, "-markdup"], b"needs -bam -sort"), (["-bam", bad, "-sort", "-markdup", "-m"], b"-m")):
        r = subprocess.run(args + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode != 0 and b"-markdup" in r.stderr and words in r.stderr, r.stderr[-500:]
        assert not os.path.exists(bad)
    assert no_temporary_file(tmp_path)
    usage = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"-markdup" in usage.stdout + usage.stderr
