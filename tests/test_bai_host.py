"""-index on the host: the accumulator, the finish and the writer of mapcaller_amd/csrc/mcx_bai.h, compiled for the host by tests/hostemu/bai_check.cpp, and
the surface of -index (header, bindings, exports, switches).

The stand-in is `Restated`: htslib's hts_idx_push / hts_idx_finish said again in Python from the rules, record by record with the same state (last and saved
bin, contig and offset; the meta pairs at a change of contig; insert_to_l's first-writer windows; update_loff; compress_binning level by level over every
bin from that level down; the join of neighbours).  It never sees a stretch: the code under test gets stretches and a window table (`stretches_of`, the
device's part of the work done plainly here), the stand-in gets the records.  The written bytes come back through `parse_bai`, a reader written here from the
SAM specification's section on BAI; bins compare as a mapping, since the file lists them ascending and htslib in hash order.  The stand-in itself is held
against htslib once: tests/golden/bai/ keeps the index the reference's vendored htslib 1.5 made of the golden set's sorted BAM file, and that file's member
table.  tests/test_bai_device.py takes the same stand-in to the kernels."""
import ctypes as C
import inspect
import json
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_bam_host import bam_check  # noqa: F401 (fixture)

SRC = os.path.join(ROOT, "tests", "hostemu", "bai_check.cpp")
NEW = ("mcx_bam_index_dev", "mcx_bam_index_last_ms", "mcx_bgzf_deflate_blocks", "mcx_files_index_stats")
META, N_BINS, NO_COOR_BIN = 37450, 37449, 4680
RUN = np.dtype([("ref_id", "<i4"), ("bin", "<u4"), ("u", "<u8"), ("n_mapped", "<u4"), ("n_unmapped", "<u4")])
assert RUN.itemsize == 24


# ---- CPU: the surface ---------------------------------------------------------------------------------------
def test_the_index_calls_are_declared_bound_and_exported():
    from mapcaller_amd import api, run
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for s in NEW:
        assert s in api.SYMBOLS and re.search(r"\b%s\s*\(" % s, header), s
    for name, value in (("MCX_SAM_INDEX", 16), ("MCX_ROUTE_INDEX", 128)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
    assert api.SAM_INDEX == 16 and api.ROUTE_INDEX == 128
    assert re.search(r"typedef struct mcx_bai_run\s*\{\s*int32_t ref_id;\s*uint32_t bin;\s*uint64_t u;\s*uint32_t n_mapped, n_unmapped;\s*\}", header)
    assert C.sizeof(api.BaiRun) == 24 and api.BaiRun.u.offset == 8
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in NEW:
            assert f" {s}\n" in nm, s
        L = api.lib()
        assert L.mcx_bam_index_dev.restype is C.c_int and len(L.mcx_bam_index_dev.argtypes) == 14
        assert len(L.mcx_files_index_stats.argtypes) == 2 and len(L.mcx_bgzf_deflate_blocks.argtypes) == 3
    assert C.sizeof(api.FileOpts) == 48 and api.FileOpts.device_sam.offset == 12
    assert inspect.signature(api.Mapper.map_files).parameters["index"].default is False
    assert "bam_index" in dir(api.Mapper) and "index_stats" in dir(api.Mapper)
    a = run.parse(["-i", "x", "-f", "a.fq", "-bam", "o.bam", "-sort", "-index"])
    assert a.bai and a.sort and a.bam and a.index == "x" and not run.parse(["-i", "x", "-f", "a.fq", "-bam", "o.bam", "-sort"]).bai  # (dest "index" is -i's)
    main = open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_main.cpp")).read()
    assert '"-index"' in main and re.search(r'"\s+-index\s', main)  # the switch and its line in usage()
    sort_help = re.search(r'" {9}-sort .*?(?=" {9}-)', main, re.S).group(0)
    assert "no index" not in sort_help and "-index" in sort_help  # -sort's help points to it
    mk = open(os.path.join(ROOT, "mapcaller_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_bai.h")) and "mcx_bai.o" in mk


# ---- the rules, said again -----------------------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    """hts_reg2bin at min_shift 14, 5 levels (Python's >> of a negative number rounds down, as C's does on these machines)"""
    end -= 1
    s, t = 14, ((1 << 15) - 1) // 7
    for l in range(5, 0, -1):
        if beg >> s == end >> s:
            return t + (beg >> s)
        s += 3
        t -= 1 << (3 * (l - 1))
    return 0


def bin_first(level):
    return ((1 << (3 * level)) - 1) // 7


class Restated:
    """hts_idx_init / hts_idx_push / hts_idx_finish for BAI.  A record is pushed as (tid, beg, end, the offset BEHIND it, mapped), as bam_index does with
    bgzf_tell after the read; offset0 is the offset of the first record."""

    def __init__(self, n_ref, offset0):
        self.n = n_ref
        self.bidx = [None] * n_ref               # per contig: None or {bin: [[u, v], ...]} in insertion order
        self.lidx = [[] for _ in range(n_ref)]   # per contig: the windows, None where untouched
        self.n_no_coor = 0
        self.save_bin = self.last_bin = None     # (0xffffffff)
        self.save_tid = self.last_tid = -1
        self.save_off = self.last_off = self.off_beg = self.off_end = offset0
        self.n_mapped = self.n_unmapped = 0
        self.last_coor = -1

    def insert_to_b(self, tid, b, u, v):
        self.bidx[tid].setdefault(b, []).append([u, v])

    def push(self, tid, beg, end, offset, mapped):
        if tid < 0:
            beg, end = -1, 0
        assert tid < 0 or (beg <= 1 << 29 and end <= 1 << 29)
        if self.last_tid != tid or (self.last_tid >= 0 and tid < 0):  # change of chromosome
            assert not (tid >= 0 and self.n_no_coor), "NO_COOR reads not in a single block at the end"
            assert not (tid >= 0 and self.bidx[tid] is not None), "Chromosome blocks not continuous"
            self.last_tid, self.last_bin = tid, None
        else:
            assert not (tid >= 0 and self.last_coor > beg), "Unsorted positions"
        if tid >= 0:
            if self.bidx[tid] is None:
                self.bidx[tid] = {}
            if mapped:
                if beg < 0:
                    beg = 0
                if end <= 0:
                    end = 1
                w = self.lidx[tid]
                hi = (end - 1) >> 14
                while len(w) < hi + 1:
                    w.append(None)
                for i in range(beg >> 14, hi + 1):
                    if w[i] is None:
                        w[i] = self.last_off  # (the start of this record)
        else:
            self.n_no_coor += 1
        b = reg2bin(beg, end)
        if self.last_bin != b:
            if self.save_bin is not None:
                self.insert_to_b(self.save_tid, self.save_bin, self.save_off, self.last_off)
            if self.last_bin is None and self.save_bin is not None:  # change of chr; keep meta information
                self.off_end = self.last_off
                self.insert_to_b(self.save_tid, META, self.off_beg, self.off_end)
                self.insert_to_b(self.save_tid, META, self.n_mapped, self.n_unmapped)
                self.n_mapped = self.n_unmapped = 0
                self.off_beg = self.off_end
            self.save_off = self.last_off
            self.save_bin = self.last_bin = b
            self.save_tid = tid
        if mapped:
            self.n_mapped += 1
        else:
            self.n_unmapped += 1
        self.last_off = offset
        self.last_coor = beg

    def finish(self, final_offset):
        if self.save_tid >= 0:
            self.insert_to_b(self.save_tid, self.save_bin, self.save_off, final_offset)
            self.insert_to_b(self.save_tid, META, self.off_beg, final_offset)
            self.insert_to_b(self.save_tid, META, self.n_mapped, self.n_unmapped)
        for i in range(self.n):
            self.update_loff(i)
            self.compress_binning(i)
        return {"refs": [({} if b is None else {k: [tuple(c) for c in v] for k, v in b.items()}, list(w)) for b, w in zip(self.bidx, self.lidx)], "n_no_coor": self.n_no_coor}

    def update_loff(self, i):
        b, w = self.bidx[i], self.lidx[i]
        l = 1
        if b is not None:
            offset0 = b[META][0][0] if META in b else 0
            l = 0
            while l < len(w) and w[l] is None:
                w[l] = offset0
                l += 1
        for k in range(l, len(w)):
            if w[k] is None:
                w[k] = w[k - 1]

    def compress_binning(self, i):
        b = self.bidx[i]
        if b is None:
            return
        for l in range(5, 0, -1):
            start = bin_first(l)
            for k in list(b.keys()):  # (htslib walks its hash table; a bin's fate does not depend on the order — only its parent's list grows, and that is a level above)
                if k not in b or k >= N_BINS or k < start:
                    continue
                p = b[k]
                if l < 5 and len(p) > 1:
                    p.sort(key=lambda c: c[0])
                if (p[-1][1] >> 16) - (p[0][0] >> 16) < 0x10000:
                    parent = (k - 1) >> 3
                    if parent not in b:
                        continue
                    b[parent].extend(p)
                    del b[k]
        if 0 in b:
            b[0].sort(key=lambda c: c[0])
        for k, p in b.items():
            if k >= N_BINS:
                continue
            m = 0
            for l in range(1, len(p)):
                if p[m][1] >> 16 >= p[l][0] >> 16:
                    if p[m][1] < p[l][1]:
                        p[m][1] = p[l][1]
                else:
                    m += 1
                    p[m] = p[l]
            del p[m + 1:]


REF_OPS = (0, 2, 3, 7, 8)  # M, D, N, = and X take reference


def decoded(rec):
    """(tid, beg, end, mapped) by the rule: pos + the reference length of the CIGAR (M, D, N, = and X), pos + 1 when flag bit 4 is set or that length is 0"""
    tid, pos, l_name, _, _, n_cigar, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    ref_len = 0
    for k in range(n_cigar):
        w, = struct.unpack_from("<I", rec, 36 + l_name + 4 * k)
        if w & 15 in REF_OPS:
            ref_len += w >> 4
    mapped = not flag & 4
    return tid, pos, pos + (ref_len if mapped and ref_len else 1), mapped


def restated_index(n_ref, records, final_offset):
    """records: (tid, beg, end, mapped, u) in file order; a record ends where the next one begins, the last at final_offset"""
    r = Restated(n_ref, records[0][4] if records else final_offset)
    for k, (tid, beg, end, mapped, u) in enumerate(records):
        r.push(tid, beg, end, records[k + 1][4] if k + 1 < len(records) else final_offset, mapped)
    return r.finish(final_offset)


# ---- a reader of the file, from the specification -------------------------------------------------------------------------------------
def parse_bai(data, ascending=True):
    """ascending: the file lists every contig's bins by number, as ours does (htslib's own files come in the order of its hash table)"""
    assert data[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", data, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", data, at)
        at += 4
        bins, order = {}, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, at)
            at += 8
            assert b not in bins and n_chunk >= 1
            bins[b] = [struct.unpack_from("<QQ", data, at + 16 * k) for k in range(n_chunk)]
            order.append(b)
            at += 16 * n_chunk
        assert not ascending or order == sorted(order)
        n_intv, = struct.unpack_from("<i", data, at)
        at += 4
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, data, at))))
        at += 8 * n_intv
    n_no_coor, = struct.unpack_from("<Q", data, at)
    assert at + 8 == len(data)
    return {"refs": refs, "n_no_coor": n_no_coor}


# ---- the input of the code under test: stretches and windows -------------------------------------------------------------------------
def shoehorned(tid, beg, end, mapped):
    if tid < 0:
        return -1, 0
    if mapped:
        beg = max(beg, 0)
        end = 1 if end <= 0 else end
    return beg, end


def stretches_of(records):
    """the run list one device call makes of these records: [ref_id, bin, u, n_mapped, n_unmapped] per maximal stretch of equal (ref_id, bin)"""
    runs = []
    for tid, beg, end, mapped, u in records:
        b = reg2bin(*shoehorned(tid, beg, end, mapped))
        key = (-1, NO_COOR_BIN) if tid < 0 else (tid, b)
        if not runs or (runs[-1][0], runs[-1][1]) != key:
            runs.append([key[0], key[1], u, 0, 0])
        runs[-1][3 if mapped else 4] += 1
    return runs


def windows_of(records, lin_base):
    lin = np.full(int(lin_base[-1]), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    for tid, beg, end, mapped, u in records:
        if 0 <= tid < len(lin_base) - 1 and mapped:  # (a contig the file does not have: for the code under test to refuse)
            beg, end = shoehorned(tid, beg, end, mapped)
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                k = int(lin_base[tid]) + w
                assert k < lin_base[tid + 1]
                lin[k] = min(int(lin[k]), u)
    return lin


def flat(case):
    n_ref, records, final_offset, cuts = case
    lens = [1 << 29] * n_ref
    lin_base = np.cumsum([0] + [(n >> 14) + 2 for n in lens]).astype(np.uint64)
    calls = [stretches_of(records[a:b]) for a, b in zip([0] + cuts, cuts + [len(records)])]
    runs = np.array([tuple(r) for c in calls for r in c], dtype=RUN)
    return n_ref, np.array([len(c) for c in calls], dtype=np.uint64), runs, final_offset, windows_of(records, lin_base), lin_base


@pytest.fixture(scope="module")
def bai_check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bai_check") / "libbai_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", SRC, "-o", out], check=True, stderr=subprocess.PIPE, timeout=600)
    L = C.CDLL(out)
    L.bai_check_reg2bin.restype = C.c_uint32
    L.bai_check_reg2bin.argtypes = [C.c_int64, C.c_int64]
    L.bai_check_build.restype = C.c_int64
    L.bai_check_build.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def build(L, case):
    """(the file's bytes, stats) of the code under test; the result code when it refuses"""
    n_ref, call_n, runs, final_offset, lin, lin_base = flat(case)
    stats = np.zeros(4, dtype=np.uint64)
    args = (n_ref, len(call_n), call_n.ctypes.data, runs.ctypes.data if len(runs) else None, final_offset, lin.ctypes.data, lin_base.ctypes.data)
    need = L.bai_check_build(*args, None, 0, stats.ctypes.data)
    if need < 0:
        return need, None
    out = np.full(need + 16, 0xA5, dtype=np.uint8)
    assert L.bai_check_build(*args, out.ctypes.data, need, stats.ctypes.data) == need and (out[need:] == 0xA5).all()
    return out[:need].tobytes(), [int(v) for v in stats]


def check(L, case):
    n_ref, records, final_offset, cuts = case
    data, stats = build(L, case)
    got, want = parse_bai(data), restated_index(n_ref, records, final_offset)
    assert got == want
    assert stats[1] == sum(len(b) for b, _ in got["refs"]) and stats[2] == sum(len(w) for _, w in got["refs"]) and stats[3] == len(data)
    return got


def V(coffset, uoffset=0):
    return coffset << 16 | uoffset


# ---- hand-made cases, on both sides of every rule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("span,merged", [(0xFFFF, True), (0x10000, False)])
def test_a_small_bin_goes_to_its_parent_and_a_large_one_stays(bai_check, span, merged):
    A = 1000
    records = [(0, 0, 20000, True, V(A - 1, 7)),        # bin 585: the parent
               (0, 100, 200, True, V(A, 9)),             # bin 4681, its chunk from block A ...
               (0, 16384 + 5, 16384 + 99, True, V(A + span, 5))]  # ... to block A + span (bin 4682)
    got = check(bai_check, (1, records, V(A + span + 0x20000), []))
    bins = got["refs"][0][0]
    assert (4681 not in bins) == merged and 4682 in bins  # (4682's own chunk spans 0x20000 blocks)
    if merged:
        assert bins[585] == [(V(A - 1, 7), V(A + span, 5))]  # (the child's chunk begins in the block the parent's ends in: joined)
    else:
        assert bins[585] == [(V(A - 1, 7), V(A, 9))] and bins[4681] == [(V(A, 9), V(A + span, 5))]


def test_a_small_bin_without_its_parent_stays(bai_check):
    records = [(0, 100, 200, True, V(50, 1)), (0, 150, 300, True, V(50, 400))]
    got = check(bai_check, (1, records, V(51), []))
    assert sorted(got["refs"][0][0]) == [4681, META]


def test_a_chain_of_merges_over_three_levels(bai_check):
    records = [(0, 0, (1 << 20) + 1, True, V(9, 0)),    # bin 9 (level 2)
               (0, 0, (1 << 17) + 1, True, V(9, 300)),  # bin 73 (level 3)
               (0, 0, 16385, True, V(9, 600)),          # bin 585 (level 4)
               (0, 0, 100, True, V(9, 900))]            # bin 4681 (level 5)
    assert [reg2bin(r[1], r[2]) for r in records] == [9, 73, 585, 4681]
    got = check(bai_check, (1, records, V(10), []))
    assert got["refs"][0][0] == {9: [(V(9, 0), V(10))], META: [(V(9, 0), V(10)), (4, 0)]}  # (bin 1, bin 9's parent, does not exist: 9 stays)


@pytest.mark.parametrize("apart,joined", [(0, True), (1, False)])
def test_neighbours_are_joined_when_they_touch_one_block(bai_check, apart, joined):
    records = [(0, 100, 200, True, V(20, 5)),                    # bin 4681
               (0, 100, (1 << 17) + 5, True, V(30, 77)),         # bin 73 (not 4681's parent): ends 4681's first chunk in block 30
               (0, 300, 400, True, V(30 + apart, 500))]          # bin 4681 again: begins in block 30, or one behind it
    final = V(0x20000)
    got = check(bai_check, (1, records, final, []))
    want = [(V(20, 5), final)] if joined else [(V(20, 5), V(30, 77)), (V(30 + apart, 500), final)]
    assert got["refs"][0][0][4681] == want


def test_a_contig_without_records_between_two_with_records(bai_check):
    records = [(0, 5, 50, True, V(1, 0)), (2, 70000, 70100, True, V(1, 300)), (2, 70001, 70002, False, V(1, 600))]
    got = check(bai_check, (4, records, V(2), []))
    assert got["refs"][1] == ({}, []) and got["refs"][3] == ({}, [])
    assert got["refs"][0][0][META] == [(V(1, 0), V(1, 300)), (1, 0)] and got["refs"][2][0][META] == [(V(1, 300), V(2)), (1, 1)]


def test_only_records_without_a_contig_and_no_records_at_all(bai_check):
    records = [(-1, -1, 0, False, V(3, 100 * k)) for k in range(5)]
    got = check(bai_check, (2, records, V(4), [2]))
    assert got == {"refs": [({}, []), ({}, [])], "n_no_coor": 5}
    got = check(bai_check, (2, [], V(3), []))
    assert got == {"refs": [({}, []), ({}, [])], "n_no_coor": 0}
    data, _ = build(bai_check, (0, [], V(3), []))
    assert data == b"BAI\1" + bytes(4) + bytes(8)


def test_leading_and_inner_untouched_windows(bai_check):
    records = [(0, 3 * 16384 + 10, 3 * 16384 + 20, True, V(7, 0)), (0, 3 * 16384 + 15, 3 * 16384 + 16, False, V(7, 50)),  # (an unmapped mate: no window of its own)
               (0, 7 * 16384, 8 * 16384 + 1, True, V(7, 100)), (-1, -1, 0, False, V(7, 200))]
    got = check(bai_check, (1, records, V(8), []))
    assert got["refs"][0][1] == [V(7, 0)] * 7 + [V(7, 100)] * 2 and got["n_no_coor"] == 1
    assert got["refs"][0][0][META] == [(V(7, 0), V(7, 200)), (2, 1)]


@pytest.mark.parametrize("cuts", [[], [3], [2, 5], [1, 2], [0, 0], [7, 7]])
def test_a_stretch_split_over_calls(bai_check, cuts):
    records = [(0, 100 + k, 200 + k, k % 3 != 1, V(40, 30 * k)) for k in range(6)] + [(1, 5, 6, True, V(40, 300))]
    got = check(bai_check, (2, records, V(41), cuts))
    assert got["refs"][0][0] == {4681: [(V(40, 0), V(40, 300))], META: [(V(40, 0), V(40, 300)), (4, 2)]}
    _, stats = build(bai_check, (2, records, V(41), cuts))
    assert stats[0] == 2  # two stretches, however many calls brought them


def test_offsets_above_2_to_the_32(bai_check):
    big = (5 << 32) + 123
    records = [(0, 0, 20000, True, V(big, 1)), (0, 10, 20, True, V(big + 0xFFFF, 2)), (0, 20000, 20010, True, V(big + 0x1FFFF, 65535))]
    got = check(bai_check, (1, records, V(big + 0x40000), []))
    assert got["refs"][0][0][4681] == [(V(big + 0xFFFF, 2), V(big + 0x1FFFF, 65535))] and got["refs"][0][1][0] == V(big, 1)


def test_a_run_list_that_does_not_continue_the_order_is_refused(bai_check):
    a, b = [(1, 5, 6, True, V(1, 0))], [(0, 5, 6, True, V(1, 100))]
    assert build(bai_check, (2, a + b, V(2), [1]))[0] == -1
    assert build(bai_check, (2, [(-1, -1, 0, False, V(1, 0))] + b, V(2), [1]))[0] == -1
    assert build(bai_check, (1, a, V(2), []))[0] == -2  # contig 1 of a file with one


# ---- random cases ----------------------------------------------------------------------------------------------------------------------
def random_case(rng):
    n_ref = rng.randrange(1, 5)
    n = rng.choice((1, 2, 5, 40, rng.randrange(1, 200)))
    tids = sorted(rng.randrange(n_ref) for _ in range(n))
    spread = rng.choice((2000, 1 << 15, 1 << 18, 1 << 24, (1 << 29) - (1 << 21)))
    recs = []
    for tid in tids:
        beg = rng.randrange(spread)
        length = rng.choice((1, 100, 150, 150, 150, 20000, 200000, (1 << 20) + 7))
        recs.append((tid, beg, beg + length, rng.random() < 0.9))
    recs.sort(key=lambda r: (r[0], r[1]))
    recs += [(-1, -1, 0, rng.random() < 0.1) for _ in range(rng.choice((0, 0, 1, 7)))]
    coffset, uoffset, out = rng.choice((0, 1 << 20, 3 << 32)), 0, []
    step = rng.choice((1, 300, 0x3000, 0x10000))  # how fast the file grows: which bins are small
    for tid, beg, end, mapped in recs:
        out.append((tid, beg, end if mapped or tid < 0 else beg + 1, mapped, V(coffset, uoffset)))
        if rng.random() < 0.3:
            coffset, uoffset = coffset + rng.choice((1, step, rng.randrange(1, 2 * step + 1))), 0
        else:
            uoffset += rng.randrange(36, 400)
            if uoffset >= 65280:
                coffset, uoffset = coffset + rng.randrange(1, step + 1), 0
    final = V(coffset + rng.choice((1, step, 0xFFFF, 0x10000)))
    cuts = sorted(rng.randrange(len(out) + 1) for _ in range(rng.choice((0, 0, 1, 2))))
    return n_ref, out, final, cuts


def random_cases(n=400):
    rng = random.Random(20240915)
    return [random_case(rng) for _ in range(n)]


def test_random_cases_against_the_restatement(bai_check):
    merged = kept = joined = 0
    for case in random_cases():
        got = check(bai_check, case)
        n_ref, records, final, cuts = case
        before = {(r[0], r[1]) for r in stretches_of(records) if r[0] >= 0}
        after = {(t, b) for t, (bins, _) in enumerate(got["refs"]) for b in bins if b != META}
        merged += len(before - after)
        kept += len(after)
        joined += sum(1 for r in stretches_of(records) if r[0] >= 0) - sum(len(c) for bins, _ in got["refs"] for b, c in bins.items() if b != META)
    assert merged > 500 and kept > 500 and joined > 500  # (a check of the cases: the rules were at work)


def test_reg2bin_is_the_specification_s(bai_check):
    rng = random.Random(3)
    edges = [0, 1, 16383, 16384, 16385, (1 << 17) - 1, 1 << 17, (1 << 20) - 1, 1 << 20, 1 << 23, 1 << 26, (1 << 29) - 1]
    pairs = [(a, b) for a in edges for b in edges if b > a] + [(-1, 0)] + [tuple(sorted(rng.sample(range(1 << 29), 2))) for _ in range(500)]
    for beg, end in pairs:
        assert bai_check.bai_check_reg2bin(beg, end) == reg2bin(beg, end), (beg, end)
    assert reg2bin(-1, 0) == NO_COOR_BIN and {reg2bin(0, 1 << s) for s in (14, 17, 20, 23, 26)} == {4681, 585, 73, 9, 1} and reg2bin(0, (1 << 26) + 1) == 0


# ---- the stand-alone form ------------------------------------------------------------------------------------------------------------
def dump_cases(path, cases):
    """what tests/hostemu/bai_check.cpp's main reads"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cases)))
        for case in cases:
            n_ref, call_n, runs, final_offset, lin, lin_base = flat(case)
            f.write(struct.pack("<QQQQQ", n_ref, len(call_n), final_offset, len(runs), len(lin)))
            for part in (call_n, runs, lin_base, lin):
                f.write(part.tobytes())


def standalone_cases():
    """every hand-made shape once more, and some of the random ones (with 2^29-long contigs a case's table is 0.25 MB a contig)"""
    hand = [(1, [(0, 0, 20000, True, V(999, 7)), (0, 100, 200, True, V(1000, 9)), (0, 16389, 16483, True, V(1000 + s, 5))], V(1000 + s + 0x20000), []) for s in (0xFFFF, 0x10000)]
    hand += [(2, [(-1, -1, 0, False, V(3, 100 * k)) for k in range(5)], V(4), [2]), (2, [], V(3), []), (0, [], V(3), [])]
    hand += [(2, [(0, 100 + k, 200 + k, k % 3 != 1, V(40, 30 * k)) for k in range(6)] + [(1, 5, 6, True, V(40, 300))], V(41), cuts) for cuts in ([], [2, 5], [0, 0], [7, 7])]
    hand += [(2, [(1, 5, 6, True, V(1, 0)), (0, 5, 6, True, V(1, 100))], V(2), [1]), (1, [(1, 5, 6, True, V(1, 0))], V(2), [])]  # the refusals
    return hand + random_cases(60)


def test_the_standalone_program_says_the_same(tmp_path, bai_check):
    """tests/hostemu/bai_check.cpp with its own main (the form a sanitizer build takes), built plainly here"""
    exe = str(tmp_path / "bai_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DBAI_CHECK_MAIN", "-Wall", "-Wno-unused-function", SRC, "-o", exe], check=True, stderr=subprocess.PIPE, timeout=600)
    cases = standalone_cases()
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    dump_cases(src, cases)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    blob, at = open(dst, "rb").read(), 0
    for case in cases:
        n, = struct.unpack_from("<q", blob, at)
        at += 8
        want, _ = build(bai_check, case)
        if n < 0:
            assert want == n
        else:
            assert blob[at:at + n] == want
            at += n
    assert at == len(blob)


# ---- htslib itself ---------------------------------------------------------------------------------------------------------------------
def test_the_restatement_against_htslib_on_the_golden_set(bam_check, golden):
    """tests/golden/bai/: the index that sam_index_build of the reference's vendored htslib 1.5 (a scratch build with an empty config.h) made of the coordinate-sorted
    BAM file of golden mc (ksw2, 4096-byte blocks, chunks of 200 000 bytes), and that file's member table.  The records are the stable sort of the host
    encoder's (tests/test_bam_sort_device.py: want_sorted), the file's stream is the sorted header and those records, the member table says where each byte of the
    stream lies in the file: the restatement over them must be htslib's index, parsed, bins as a mapping."""
    import bisect
    from test_bam_sort_device import split_records, want_sorted
    gold = os.path.join(ROOT, "tests", "golden", "bai")
    table = json.load(open(os.path.join(gold, "mc_sorted.members.json")))
    want = parse_bai(open(os.path.join(gold, "mc_sorted.htslib.bai"), "rb").read(), ascending=False)
    records = split_records(want_sorted(bam_check, golden, "mc", "ksw2")[0])
    assert len(records) == 4000
    # where the stream's bytes lie in the file
    csize, isize = [m[0] for m in table["members"]], [m[1] for m in table["members"]]
    assert isize[-1] == 0 and sum(isize) == table["header_bytes"] + sum(map(len, records))
    coff = np.cumsum([0] + csize).tolist()
    text = [(c, u) for c, u, n in zip(coff, np.cumsum([0] + isize).tolist(), isize) if n]
    starts = [u for _, u in text]
    tuples, at = [], table["header_bytes"]
    for r in records:
        k = bisect.bisect_right(starts, at) - 1
        tuples.append(decoded(r) + (V(text[k][0], at - starts[k]),))
        at += len(r)
    assert restated_index(3, tuples, V(coff[len(csize) - 1])) == want
