"""-sort on the host: the order (mapcaller_amd/csrc/mcx_bam_sort.h) and the plan of the merge (mcx_sort_plan.h), compiled for the host by
tests/hostemu/sort_check.cpp.

The key is held against the formula written out here, on hand-packed records; the plan against brute force: random sorted runs with many equal keys, one key
that holds half of all records, block tables with blocks of 1 to 4096 bytes — the slices partition every run, no key lies in two chunks, the chunks
stable-sorted one by one give the global stable sort, and the covering blocks are exactly those that hold a slice's bytes.  The stand-alone form of the tool
(the one a sanitizer build takes) must say the same as the library form."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "hostemu", "sort_check.cpp")


def key_of(ref_id, pos, flag):
    """the issue's formula: (uint32_t)refID << 32 | (uint32_t)(pos + 1) << 1 | reverse"""
    return ((ref_id & 0xFFFFFFFF) << 32) | ((((pos + 1) & 0xFFFFFFFF) << 1) & 0xFFFFFFFF) | (1 if flag & 0x10 else 0)


def pack_record(ref_id, pos, flag, name=b"r", seq_len=0, extra=b""):
    """a BAM record by hand: block_size, the 32 bytes of the core, QNAME NUL, no CIGAR, SEQ, QUAL, `extra` for tags"""
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) + 1, 0, 4680, 0, flag, seq_len, -1, -1, 0) + name + b"\0" + bytes((seq_len + 1) // 2) + b"\xff" * seq_len + extra
    return struct.pack("<I", len(body)) + body


@pytest.fixture(scope="module")
def sort_check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sort_check") / "libsort_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", SRC, "-o", out], check=True, stderr=subprocess.PIPE, timeout=600)
    L = C.CDLL(out)
    L.sort_check_key.restype = C.c_uint64
    L.sort_check_key.argtypes = [C.c_char_p]
    L.sort_check_plan.restype = C.c_int64
    L.sort_check_plan.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
    return L


KEY_CASES = [(ref_id, pos, flag) for ref_id in (-1, 0, 24) for pos in (-1, 0, (1 << 31) - 2) for flag in (0, 0x10, 0x63, 0x93, 4, 0x14)]


def test_the_key_is_the_formula(sort_check):
    for ref_id, pos, flag in KEY_CASES:
        rec = pack_record(ref_id, pos, flag, name=b"read/1", seq_len=7, extra=b"ASC\0")
        assert struct.unpack_from("<i", rec, 4)[0] == ref_id and struct.unpack_from("<i", rec, 8)[0] == pos and struct.unpack_from("<H", rec, 18)[0] == flag
        assert sort_check.sort_check_key(rec) == key_of(ref_id, pos, flag), (ref_id, pos, flag)


def test_the_key_orders_like_samtools_sort(sort_check):
    k = lambda *a: sort_check.sort_check_key(pack_record(*a))  # noqa: E731
    assert k(0, 5, 0) < k(0, 5, 0x10) < k(0, 6, 0) < k(1, 0, 0) < k(24, (1 << 31) - 2, 0x10) < k(-1, -1, 4)  # forward before reverse on one position; unmapped last
    assert k(0, -1, 0) < k(0, 0, 0) and k(-1, -1, 0x14) == (0xFFFFFFFF << 32) | 1
    assert k(2, 100, 0x63) == k(2, 100, 0x83)  # (only the strand bit of the flag counts)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def make_case(rng, n_runs, heavy=False):
    """random sorted runs: few distinct keys (many ties); heavy: one key holds half of all records"""
    n_keys = rng.choice((1, 3, 20, 200))
    pool = sorted(rng.sample(range(1 << 40), n_keys))
    runs = []
    for _ in range(n_runs):
        n = rng.choice((0, 1, 2, rng.randrange(0, 301)))
        keys = [rng.choice(pool) for _ in range(n)]
        if heavy:
            keys = [pool[len(pool) // 2] if rng.random() < 0.5 else k for k in keys]
        keys.sort()
        lens = [rng.choice((36, 38, 290, rng.randrange(36, 3000))) for _ in range(n)]
        total, blocks = sum(lens), []
        while sum(blocks) < total:
            blocks.append(min(rng.choice((1, 2, 17, 4096, rng.randrange(1, 4097))), total - sum(blocks)))
        runs.append((keys, lens, blocks))
    total = sum(sum(r[1]) for r in runs)
    chunk_bytes = rng.choice((1, 500, 5000, max(1, total // 3), total + 1, 1 << 28))
    return runs, chunk_bytes


def all_cases():
    rng = random.Random(20240607)
    cases = [make_case(rng, n_runs, heavy) for n_runs in range(1, 8) for heavy in (False, True) for _ in range(6)]
    cases.append(([([], [], [])], 100))  # nothing at all
    return cases


def flat(case):
    runs, chunk_bytes = case
    a = lambda v, t: np.array(v, dtype=t)  # noqa: E731
    return (a([len(r[0]) for r in runs], np.uint64), a([k for r in runs for k in r[0]], np.uint64), a([v for r in runs for v in r[1]], np.uint32),
            a([len(r[2]) for r in runs], np.uint64), a([v for r in runs for v in r[2]], np.uint32), chunk_bytes)


def plan_of(L, case):
    run_n, keys, lens, run_nb, usize, chunk_bytes = flat(case)
    n = len(keys)
    out, splitters, n_chunks = np.zeros(8 * (n + 1), dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64), C.c_uint64()
    got = L.sort_check_plan(len(run_n), run_n.ctypes.data, keys.ctypes.data, lens.ctypes.data, run_nb.ctypes.data, usize.ctypes.data, chunk_bytes, out.ctypes.data, n + 1,
                            C.byref(n_chunks), splitters.ctypes.data)
    assert got >= 0
    return [tuple(int(v) for v in out[8 * i:8 * i + 8]) for i in range(got)], int(n_chunks.value), [int(v) for v in splitters[:max(0, n_chunks.value - 1)]]


def check_plan(case, slices, n_chunks, splitters):
    runs, chunk_bytes = case
    assert n_chunks == len(splitters) + 1 and splitters == sorted(set(splitters))
    # the slices partition every run, in chunk order
    for r, (keys, lens, blocks) in enumerate(runs):
        mine = [s for s in slices if s[1] == r]
        assert [s[0] for s in mine] == sorted(s[0] for s in mine) and len(set(s[0] for s in mine)) == len(mine)
        at = 0
        for s in mine:
            assert s[2] == at and s[3] > s[2]
            at = s[3]
        assert at == len(keys)
    # no key in two chunks; a chunk's keys lie between its splitters
    where = {}
    for c, r, r0, r1, b0, b1, k0, k1 in slices:
        keys, lens, blocks = runs[r]
        for k in keys[r0:r1]:
            assert where.setdefault(k, c) == c
            assert (c == 0 or splitters[c - 1] <= k) and (c == n_chunks - 1 or k < splitters[c])
        # bytes and covering blocks
        assert b0 == sum(lens[:r0]) and b1 == sum(lens[:r1]) and b1 > b0
        u = [0]
        for v in blocks:
            u.append(u[-1] + v)
        assert 0 <= k0 < k1 <= len(blocks)
        assert u[k0] <= b0 and u[k1] >= b1             # the covering blocks contain the slice's bytes
        assert u[k0 + 1] > b0 and u[k1 - 1] < b1       # ... and no block is beyond them
    # the chunks in (run, index) order, each stable-sorted, are the global stable sort
    everything = [(k, r, i) for r, (keys, _, _) in enumerate(runs) for i, k in enumerate(keys)]
    want = sorted(everything, key=lambda t: t[0])      # (stable: ties stay in (run, index) order)
    got = []
    for c in range(n_chunks):
        part = [(runs[r][0][i], r, i) for cc, r, r0, r1, *_ in sorted(slices, key=lambda s: (s[0], s[1])) if cc == c for i in range(r0, r1)]
        got += sorted(part, key=lambda t: t[0])
    assert got == want
    # (the slices come in chunk order, and within a chunk in run order)
    assert [(s[0], s[1]) for s in slices] == sorted((s[0], s[1]) for s in slices)


def test_the_plan_against_brute_force(sort_check):
    several = 0
    for case in all_cases():
        slices, n_chunks, splitters = plan_of(sort_check, case)
        check_plan(case, slices, n_chunks, splitters)
        several += n_chunks > 2
    assert several >= 10  # (a check of the cases, not of the plan: enough of them are cut into three chunks or more)


def test_a_pile_up_on_one_key_stays_in_one_chunk(sort_check):
    runs = [([7] * 150 + [9] * 3, [100] * 153, [4096] * 3 + [3012]), ([5] + [7] * 200, [50] * 201, [1] * 10050)]
    slices, n_chunks, splitters = plan_of(sort_check, (runs, 1000))
    check_plan((runs, 1000), slices, n_chunks, splitters)
    assert len(set(s[0] for s in slices if 7 in runs[s[1]][0][s[2]:s[3]])) == 1


def test_the_result_does_not_depend_on_the_chunk_size(sort_check):
    rng = random.Random(5)
    runs, _ = make_case(rng, 5)
    orders = []
    for chunk_bytes in (1, 777, 40000, 1 << 30):
        slices, n_chunks, _ = plan_of(sort_check, (runs, chunk_bytes))
        order = []
        for c in range(n_chunks):
            part = [(runs[r][0][i], r, i) for cc, r, r0, r1, *_ in slices if cc == c for i in range(r0, r1)]
            order += sorted(part, key=lambda t: t[0])
        orders.append(order)
    assert all(o == orders[0] for o in orders)


# ---- the stand-alone form ------------------------------------------------------------------------------------------------------------
def dump_cases(path, records, cases):
    """what tests/hostemu/sort_check.cpp's main reads: the records for the key (each at exactly the 20 bytes the key reads), then the plan cases"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(records)))
        for rec in records:
            f.write(struct.pack("<Q", 20) + rec[:20])
        f.write(struct.pack("<Q", len(cases)))
        for case in cases:
            run_n, keys, lens, run_nb, usize, chunk_bytes = flat(case)
            f.write(struct.pack("<QQQQ", len(run_n), chunk_bytes, len(keys), len(usize)))
            for part in (run_n, run_nb, keys, lens, usize):
                f.write(part.tobytes())


def test_the_standalone_program_says_the_same(tmp_path, sort_check):
    """tests/hostemu/sort_check.cpp with its own main (the form a sanitizer build takes), built plainly here"""
    exe = str(tmp_path / "sort_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DSORT_CHECK_MAIN", "-Wall", "-Wno-unused-function", SRC, "-o", exe], check=True, stderr=subprocess.PIPE, timeout=600)
    records = [pack_record(*k) for k in KEY_CASES]
    cases = all_cases()
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    dump_cases(src, records, cases)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(dst, dtype=np.uint64)
    assert [int(v) for v in got[:len(records)]] == [key_of(*k) for k in KEY_CASES]
    at = len(records)
    for case in cases:
        slices, n_chunks, _ = plan_of(sort_check, case)
        n = int(got[at])
        assert (n, int(got[at + 1])) == (len(slices), n_chunks)
        assert [tuple(int(v) for v in got[at + 2 + 8 * i:at + 10 + 8 * i]) for i in range(n)] == slices
        at += 2 + 8 * n
    assert at == len(got)
