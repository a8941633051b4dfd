"""-index on the device: mcx_bam_index_dev on synthetic sorted records, and the file front end's .bai on the golden sets.

The operation's stretches and windows are held against tests/test_bai_host.py's `stretches_of` / `windows_of` over records decoded here (the end from the CIGAR
by the rule, the virtual offset from the invented block table), and — through the host half compiled by tests/hostemu/bai_check.cpp — the finished index
against `Restated`, htslib's push and finish said again in Python.  The front end's parsed .bai equals the restatement run over the records and the block
table of the BAM file it wrote; and the index does its job: for a few hundred regions, the records found through bins, chunks and linear entries are exactly
those a scan of the whole file finds."""
import bisect
import ctypes as C
import hashlib
import os
import pathlib
import random
import shutil
import struct
import subprocess
from contextlib import contextmanager

import numpy as np
import pytest

import test_bgzf_resident as tb
from conftest import ROOT
from test_bai_host import META, RUN, V, bai_check, decoded, parse_bai, reg2bin, restated_index, stretches_of, windows_of  # noqa: F401 (fixtures)
from test_bam_device import bam_stream
from test_bam_host import decode_header
from test_bam_sort_device import no_temporary_file, split_records

EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
GUARD = 64
ONES = 0xFFFFFFFFFFFFFFFF
M, I, D, N, S, H, P, EQ, X = range(9)


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


# ---- records, packed and read again in Python ------------------------------------------------------------------------------------------
def pack(ref_id, pos, flag, cigar=(), size=None, name=b"r"):
    """a BAM record by hand: block_size, the core, QNAME NUL, the CIGAR words, no bases; `size`: padded with tag bytes to that many bytes in all"""
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) + 1, 0, 4680, len(cigar), flag, 0, -1, -1, 0) + name + b"\0" + b"".join(struct.pack("<I", n << 4 | op) for op, n in cigar)
    if size is not None:
        assert size >= 4 + len(body)
        body += b"\x5a" * (size - 4 - len(body))
    return struct.pack("<I", len(body)) + body


def tuples_of(records, block, coffs):
    """the records as the restatement takes them: (tid, beg, end, mapped, u), u from the record's offset and the block table"""
    out, at = [], 0
    for r in records:
        out.append(decoded(r) + (V(coffs[at // block], at % block),))
        at += len(r)
    return out


def invented_blocks(rng, n_bytes, block, base):
    n_blocks = (n_bytes + block - 1) // block
    return [base + v for v in np.cumsum([0] + [rng.randrange(26, 70000) for _ in range(n_blocks)]).tolist()]


LENS = [1 << 29, 1 << 29, 70000]  # the contigs of the synthetic files
LIN_BASE = np.cumsum([0] + [(n >> 14) + 2 for n in LENS]).astype(np.uint64)


def fresh_table():
    return np.full(int(LIN_BASE[-1]), ONES, dtype=np.uint64)


def run_index(api, mp, records, block, coffs, table, shift=0, runs_cap=None, want_rc=0, data=None, rec_off=None, n_ref=3):
    """one call between guard bytes round every output: (the stretches as rows, the table afterwards, n_runs, the records' absolute address)"""
    import torch
    if data is None:
        data = b"".join(records)
        rec_off = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
    n, n_bytes = len(rec_off) - 1, len(data)
    cap = n if runs_cap is None else runs_cap
    src = torch.full((GUARD + 16 + n_bytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    s0 = GUARD + shift
    if n_bytes:
        src[s0:s0 + n_bytes] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    off = torch.from_numpy(np.asarray(rec_off, dtype=np.uint64).view(np.int64).copy()).cuda()
    coff = torch.from_numpy(np.asarray(coffs, dtype=np.uint64).view(np.int64).copy()).cuda()
    lin = torch.from_numpy(np.concatenate([np.full(8, 0xA5A5, np.uint64), table, np.full(8, 0xA5A5, np.uint64)]).view(np.int64).copy()).cuda()
    base = torch.from_numpy(LIN_BASE[:n_ref + 1].view(np.int64).copy()).cuda()
    runs = torch.full((GUARD + 24 * cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n_runs = C.c_uint64(99)
    rc = api.lib().mcx_bam_index_dev(mp._h, src.data_ptr() + s0, n_bytes, off.data_ptr(), n, block, coff.data_ptr(), len(coffs) - 1, lin.data_ptr() + 64, base.data_ptr(), n_ref,
                                     runs.data_ptr() + GUARD, cap, C.byref(n_runs))
    assert rc == want_rc, api.lib().mcx_last_error()
    got_runs, got_lin = runs.cpu().numpy(), lin.cpu().numpy().view(np.uint64)
    used = 24 * n_runs.value if rc == 0 else 0
    assert (got_runs[:GUARD] == 0xA5).all() and (got_runs[GUARD + used:] == 0xA5).all()  # not a byte outside the stretches written
    assert (got_lin[:8] == 0xA5A5).all() and (got_lin[-8:] == 0xA5A5).all()
    assert src.cpu().numpy()[s0:s0 + n_bytes].tobytes() == data
    rows = [[int(v) for v in r] for r in got_runs[GUARD:GUARD + used].view(RUN).tolist()]
    return rows, got_lin[8:-8].copy(), n_runs.value, src.data_ptr() + s0


def check_call(api, mp, records, block, coffs, shift=0):
    """one call over a fresh table against the Python of the rules; returns the records as tuples"""
    tuples = tuples_of(records, block, coffs)
    rows, table, n_runs, at = run_index(api, mp, records, block, coffs, fresh_table(), shift=shift)
    assert rows == stretches_of(tuples) and n_runs == len(rows)
    assert (table == windows_of(tuples, LIN_BASE)).all()
    return tuples, rows, table, at


def finished(bai_check, calls, table, final_offset, n_ref=3):
    """the host half over the device's output: the parsed index of the run lists of consecutive calls and the table"""
    call_n = np.array([len(c) for c in calls], dtype=np.uint64)
    runs = np.array([tuple(r) for c in calls for r in c], dtype=RUN)
    need = bai_check.bai_check_build(n_ref, len(calls), call_n.ctypes.data, runs.ctypes.data if len(runs) else None, final_offset, table.ctypes.data, LIN_BASE.ctypes.data, None, 0, None)
    assert need > 0
    out = np.zeros(need, dtype=np.uint8)
    assert bai_check.bai_check_build(n_ref, len(calls), call_n.ctypes.data, runs.ctypes.data if len(runs) else None, final_offset, table.ctypes.data, LIN_BASE.ctypes.data, out.ctypes.data, need, None) == need
    return parse_bai(out.tobytes())


def random_sorted_records(rng, n):
    """n sorted records over three contigs with a tail without contig: every length class, CIGARs of all kinds, unmapped mates placed at their mate's position"""
    keys = []
    for k in range(n):
        tid = rng.choice((0, 0, 1, 2, -1)) if n > 3 else rng.choice((0, -1))
        pos = -1 if tid < 0 else rng.randrange(0, 69000) if tid == 2 else rng.choice((rng.randrange(0, 40000), rng.randrange(0, 1 << 28)))
        keys.append((tid & 0xFFFFFFFF, pos))
    keys.sort()
    out = []
    for k, (tid, pos) in enumerate(keys):
        tid = tid - (1 << 32) if tid >= 1 << 31 else tid
        kind = rng.randrange(6)
        cigar = ((), ((M, 150),), ((S, 5), (M, 100), (I, 3), (M, 42)), ((M, 50), (D, 2), (M, 98), (H, 4)), ((M, 60), (N, rng.choice((500, 20000))), (M, 90)), ((EQ, 70), (X, 1), (EQ, 79)))[kind]
        if tid == 2:
            cigar = cigar if kind != 4 else ((M, 100),)
        flag = rng.choice((0, 0x10, 0x63, 0x93)) | (4 if tid < 0 or rng.random() < 0.08 else 0)
        out.append(pack(tid, pos, flag, cigar if tid >= 0 else (), name=b"q%d" % k if kind else b"r", size=None if kind < 4 else rng.choice((64, 290, 1000))))
    return out


# ---- the operation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_stretches_and_windows_are_the_rules(api, mapper, bai_check, n):
    rng = random.Random(500 + n)
    records = random_sorted_records(rng, n)
    if n == 0:
        rows, table, n_runs, _ = run_index(api, mapper, [], 4096, [0], fresh_table())
        assert rows == [] and n_runs == 0 and (table == ONES).all()  # no stretches, nothing touched
        return
    n_bytes, classes = sum(map(len, records)), set()
    for block, base in ((100, 0), (4096, 1 << 20), (65280, 5 << 32)):
        coffs = invented_blocks(rng, n_bytes, block, base)
        for shift in range(16) if (n >= 65 and block == 4096) else (0, 5):
            tuples, rows, table, at = check_call(api, mapper, records, block, coffs, shift=shift)
            classes |= {(at + o) % 16 for o in np.cumsum([0] + [len(r) for r in records[:-1]]).tolist()}
        final = V(coffs[-1])
        assert finished(bai_check, [rows], table, final) == restated_index(3, tuples, final)
    if n >= 65:
        assert len(classes) == 16  # records at every residue mod 16
    if n == 1000:  # (the stream is what it is here for)
        t = [decoded(r) for r in records]
        assert {x[0] for x in t} == {-1, 0, 1, 2} and any(not x[3] and x[0] >= 0 for x in t) and len(stretches_of(tuples)) > 100
    assert all(v >= 0 for v in mapper.bam_index_last_ms())


SPECIAL = sorted([
    (0, 16383, ((M, 1),)),                 # ends exactly on a window edge: window 0 only
    (0, 16383, ((M, 2),)),                 # one past it: windows 0 and 1, bin 585
    (0, 16384, ((M, 1),)),                 # the first base of window 1
    (0, 16000, ((M, 50), (N, 40000), (M, 50))),  # spans windows 0 .. 3
    (0, (1 << 17) - 5, ((M, 10),)),        # crosses 2^17: a level-3 bin
    (0, (1 << 20) - 5, ((M, 10),)),        # 2^20: level 2
    (0, (1 << 23) - 5, ((M, 10),)),        # 2^23: level 1
    (0, (1 << 26) - 5, ((M, 10),)),        # 2^26: bin 0
    (0, 500, ()),                          # mapped without a CIGAR: end = pos + 1
] + [(1, 1000 + 10 * op, ((M, 5), (op, 7), (M, 5))) for op in range(9)] + [(1, 2000 + 10 * op, ((op, 7),)) for op in range(9)], key=lambda r: (r[0], r[1]))


@pytest.mark.gpu
def test_positions_cigars_and_bins_of_every_level(api, mapper, bai_check):
    records = [pack(tid, pos, 0x10 if k % 2 else 0, cigar, name=b"s%d" % k) for k, (tid, pos, cigar) in enumerate(SPECIAL)]
    records.insert(3, pack(0, 16383, 0x4 | 0x1, ((M, 100),)))  # flag 4 on a contig: its CIGAR does not count, it touches no window
    records += [pack(-1, -1, 0x4 | 0x1), pack(-1, -1, 0x4 | 0x41), pack(-1, -1, 0x41)]  # the tail without a contig (one of them not flagged unmapped)
    rng = random.Random(9)
    coffs = invented_blocks(rng, sum(map(len, records)), 100, 7 << 32)
    tuples, rows, table, _ = check_call(api, mapper, records, 100, coffs)
    ends = {(t[0], t[1]): t[2] for t in tuples}
    assert ends[(0, 500)] == 501 and ends[(0, 16000)] == 16000 + 40100 and [ends[(1, 1000 + 10 * op)] - (1000 + 10 * op) for op in range(9)] == [17, 10, 17, 17, 10, 10, 10, 17, 17]
    assert [ends[(1, 2000 + 10 * op)] - (2000 + 10 * op) for op in range(9)] == [7, 1, 7, 7, 1, 1, 1, 7, 7]
    bins = {r[1] for r in rows if r[0] == 0}
    assert bins >= {4681, 4682, 585, 73, 9, 1, 0} and rows[-1][:2] == [-1, 4680] and rows[-1][3:] == [1, 2]
    w = table[:8]
    assert w[0] == tuples[0][4] and w[1] == w[2] == w[3] == next(t[4] for t in tuples if t[1] == 16000)  # the long record is the first to reach windows 1 .. 3
    final = V(coffs[-1])
    assert finished(bai_check, [rows], table, final) == restated_index(3, tuples, final)


@pytest.mark.gpu
def test_stretches_at_wavefront_edges_a_long_one_and_alternating_bins(api, mapper):
    short, long_ = ((M, 1),), ((M, 10),)
    records = [pack(0, 100, 0, short) for _ in range(63)] + [pack(0, 16380, 0, long_)]     # a stretch that begins on lane 63 ...
    records += [pack(0, 16384 + 5, 0, short) for _ in range(200)]                             # ... one on lane 0 of the next wavefront, 200 records long
    records += [pack(0, 3 * 16384 - 4, 0, short if k % 2 else long_) for k in range(100)]    # alternating bins: every record a stretch
    coffs = invented_blocks(random.Random(2), sum(map(len, records)), 4096, 0)
    tuples, rows, table, _ = check_call(api, mapper, records, 4096, coffs)
    assert [r[3] for r in rows[:3]] == [63, 1, 200] and [r[1] for r in rows[:3]] == [4681, 585, 4682] and len(rows) == 103
    assert [r[1] for r in rows[3:]] == [585 + 0, 4681 + 2] * 50


@pytest.mark.gpu
def test_a_record_that_ends_at_a_block_s_end(api, mapper, bai_check):
    records = [pack(0, 10 * k, 0, ((M, 30),), size=50) for k in range(40)]  # two records a block of 100 bytes
    coffs = invented_blocks(random.Random(4), 2000, 100, 3 << 32)
    tuples, rows, table, _ = check_call(api, mapper, records, 100, coffs)
    assert [t[4] for t in tuples[:4]] == [V(coffs[0], 0), V(coffs[0], 50), V(coffs[1], 0), V(coffs[1], 50)]
    final = V(coffs[-1])
    want = restated_index(3, tuples, final)
    assert finished(bai_check, [rows], table, final) == want and want["refs"][0][0][4681][-1][1] == final


@pytest.mark.gpu
@pytest.mark.parametrize("cuts", [(14,), (2, 30), (20, 20)])
def test_consecutive_calls_over_one_table_equal_one_call(api, mapper, bai_check, cuts):
    rng = random.Random(31)
    pos = sorted(rng.randrange(0, 60000) for _ in range(36))
    records = [pack(0 if k < 24 else 2, pos[k] if k < 24 else pos[k - 24], 4 if k % 7 == 3 else 0, ((M, rng.choice((1, 30, 20000))),), size=50) for k in range(36)]
    records += [pack(-1, -1, 4, size=50) for _ in range(4)]
    coffs = invented_blocks(rng, 2000, 100, 1 << 33)
    tuples, rows_one, table_one, _ = check_call(api, mapper, records, 100, coffs)
    calls, table = [], fresh_table()
    for a, b in zip((0,) + cuts, cuts + (40,)):  # (a call's first record begins a block: the cuts are even)
        part = b"".join(records[a:b])
        off = np.arange(b - a + 1, dtype=np.uint64) * 50
        rows, table, _, _ = run_index(api, mapper, None, 100, coffs[a // 2:b // 2 + 1] if b > a else [0], table, data=part, rec_off=off)
        calls.append(rows)
    assert (table == table_one).all()
    final = V(coffs[-1])
    assert finished(bai_check, calls, table, final) == finished(bai_check, [rows_one], table_one, final) == restated_index(3, tuples, final)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["chain leaves its record", "block_size 8", "offsets do not reach n_bytes", "offsets descend", "cigar leaves its record",
                                 "positions descend", "contigs descend", "a contig behind none", "refID beyond n_ref", "beyond the windows"])
def test_broken_input_is_an_argument_error_and_writes_nothing(api, mapper, how):
    rng = random.Random(3)
    records = random_sorted_records(rng, 40)
    data = b"".join(records)
    ends = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)

    def put(k, rec):
        nonlocal data
        assert len(rec) == len(records[k])
        data = data[:int(ends[k])] + rec + data[int(ends[k + 1]):]

    if how == "chain leaves its record":
        ends[20] += 5
    elif how == "block_size 8":
        data = data[:int(ends[7])] + struct.pack("<I", 8) + data[int(ends[7]) + 4:]
    elif how == "offsets do not reach n_bytes":
        ends = ends[:-1]
    elif how == "offsets descend":
        ends[10], ends[11] = ends[11], ends[10]
    elif how == "cigar leaves its record":
        put(5, records[5][:16] + struct.pack("<H", 60000) + records[5][18:])
    elif how == "positions descend":
        k = next(k for k in range(1, 40) if decoded(records[k])[0] == decoded(records[k - 1])[0] >= 0 and decoded(records[k - 1])[1] > 0)
        put(k, records[k][:8] + struct.pack("<i", decoded(records[k - 1])[1] - 1) + records[k][12:])
    elif how == "contigs descend":
        k = next(k for k in range(1, 40) if decoded(records[k])[0] > 0)
        put(k + 1, records[k + 1][:4] + struct.pack("<i", 0) + records[k + 1][8:])
    elif how == "a contig behind none":
        put(39, records[39][:4] + struct.pack("<ii", 2, 5) + records[39][12:])
        assert decoded(records[38])[0] < 0
    elif how == "refID beyond n_ref":
        k = next(k for k in range(40) if decoded(records[k])[0] == 2)
        put(k, records[k][:4] + struct.pack("<i", 3) + records[k][8:])
    else:
        k = max(k for k in range(40) if decoded(records[k])[0] == 2)
        put(k, records[k][:8] + struct.pack("<i", 70000 + 3 * 16384) + records[k][12:])  # contig 2 has 70000 bases: its table ends two windows behind them
    n_bytes = len(data)
    coffs = invented_blocks(rng, n_bytes, 4096, 0)
    rows, table, n_runs, _ = run_index(api, mapper, None, 4096, coffs, fresh_table(), shift=3, want_rc=api.ERR_ARG, data=data, rec_off=ends)
    assert rows == [] and n_runs == 0 and (table == ONES).all()


@pytest.mark.gpu
def test_capacity_the_empty_call_and_the_python_wrapper(api, mapper):
    import torch
    records = random_sorted_records(random.Random(12), 64)
    coffs = invented_blocks(random.Random(13), sum(map(len, records)), 4096, 0)
    tuples = tuples_of(records, 4096, coffs)
    want = stretches_of(tuples)
    rows, table, n_runs, _ = run_index(api, mapper, records, 4096, coffs, fresh_table(), runs_cap=len(want) - 1, want_rc=api.ERR_CAPACITY)
    assert rows == [] and n_runs == len(want) and (table == ONES).all()  # what is needed, and nothing written
    rows, table, n_runs, _ = run_index(api, mapper, records, 4096, coffs, fresh_table(), runs_cap=len(want))
    assert rows == want
    L, n, d = api.lib(), C.c_uint64(5), torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    assert L.mcx_bam_index_dev(mapper._h, p, 100, p, 0, 4096, p, 1, p, p, 3, p, 10, C.byref(n)) == 0 and n.value == 0 and bool((d == 0xA5).all())  # no record: nothing to do
    assert L.mcx_bam_index_dev(None, p, 100, p, 1, 4096, p, 1, p, p, 3, p, 10, C.byref(n)) == api.ERR_ARG
    assert L.mcx_bam_index_dev(mapper._h, None, 100, p, 1, 4096, p, 1, p, p, 3, p, 10, C.byref(n)) == api.ERR_ARG
    assert L.mcx_bam_index_dev(mapper._h, p, 100, p, 1, 4096, p, 2, p, p, 3, p, 10, C.byref(n)) == api.ERR_ARG  # 100 bytes are one block of 4096
    assert L.mcx_bam_index_dev(mapper._h, p, 100, p, 1, 0, p, 1, p, p, 3, p, 10, C.byref(n)) == api.ERR_ARG
    assert L.mcx_bam_index_dev(mapper._h, p, 100, p, 3, 4096, p, 1, p, p, 3, p, 10, C.byref(n)) == api.ERR_ARG  # three records do not fit 100 bytes
    ms = (C.c_float * 3)()
    assert L.mcx_bam_index_last_ms(mapper._h, None) == api.ERR_ARG and L.mcx_bam_index_last_ms(None, ms) == api.ERR_ARG
    # the wrapper
    cu = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()  # noqa: E731
    lin = cu(fresh_table())
    got = mapper.bam_index(torch.from_numpy(np.frombuffer(b"".join(records), dtype=np.uint8).copy()).cuda(), cu(np.cumsum([0] + [len(r) for r in records])), 4096, cu(coffs), lin, cu(LIN_BASE))
    assert [[int(v) for v in r] for r in got.tolist()] == want and (lin.cpu().numpy().view(np.uint64) == windows_of(tuples, LIN_BASE)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("block", [100, 1])  # (a launch of the deflater takes 65536 blocks at most: 70000 blocks of one byte are two launches)
def test_the_deflater_says_where_its_blocks_are(api, mapper, block):
    """the records are deflated, and the operation takes the deflater's own array for the blocks' places: every record a stretch, so every offset shows"""
    import torch
    records = [pack(0, 16380, 0, ((M, 10 if k % 2 else 1),), size=50) for k in range(1400)]
    data = b"".join(records)
    d = api.Deflater(0)
    assert d.set_block(block) == 0
    cu = lambda a: torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()  # noqa: E731
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    out = torch.zeros(d.bound(len(data)), dtype=torch.uint8, device="cuda")
    rc, made = d.deflate_dev(src, len(data), out)
    assert rc == 0
    ptr, n_blocks = d.blocks()
    assert n_blocks == (len(data) + block - 1) // block and ptr
    blob, places, o = out[:made].cpu().numpy().tobytes(), [], 0
    while o < len(blob):  # where the blocks lie, read off the blocks
        places.append(o)
        o += struct.unpack_from("<H", blob, o + 16)[0] + 1
    assert len(places) == n_blocks and o == made
    lin, runs, n_runs = cu(fresh_table()), torch.zeros(24 * 1400, dtype=torch.uint8, device="cuda"), C.c_uint64()
    off, base = cu(np.arange(1401) * 50), cu(LIN_BASE)  # (held until the call is over)
    torch.cuda.synchronize()
    rc = api.lib().mcx_bam_index_dev(mapper._h, src.data_ptr(), len(data), off.data_ptr(), 1400, block, ptr, n_blocks, lin.data_ptr(), base.data_ptr(), 3,
                                     runs.data_ptr(), 1400, C.byref(n_runs))
    assert rc == 0 and n_runs.value == 1400, api.lib().mcx_last_error()
    got = runs.cpu().numpy().view(RUN)
    assert [int(v) for v in got["u"]] == [V(places[50 * k // block], 50 * k % block) for k in range(1400)]
    rc, made = d.deflate_dev(src, 0, out)
    assert d.blocks() == (0, 0)  # a call without text leaves none
    d.close()


# ---- the front end ---------------------------------------------------------------------------------------------------------------------
@contextmanager
def environment(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def map_indexed(api, g, alg, out, batch, multi=False, files=None, index=True, **kw):
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg=alg, multi=multi, max_batch_reads=batch)
    header = api.bam_header(ix, sorted=True)
    r1, r2 = files or (g["r1"], g["r2"])
    try:
        st = mp.map_files(r1, r2, out, bam=True, sort=True, index=index, **kw)
        return st, mp.last_route(), mp.index_stats(), header
    finally:
        mp.close(); ix.close()


class WrittenBam:
    """a BAM file as it lies on disk: the inflated stream, where every member begins in the file and in the stream, and the records with their virtual offsets"""

    def __init__(self, path, header):
        self.blob = open(path, "rb").read()
        self.stream, members = bam_stream(path)
        assert self.stream[:len(header)] == header
        self.coff, self.uoff, c, u = [], [], 0, 0
        for payload, _, isize in members:
            self.coff.append(c); self.uoff.append(u)
            c += len(payload) + 26; u += isize
        self.eof = self.coff[-1]
        self.first = {c: u for c, u, m in zip(self.coff, self.uoff, members) if m[2]}  # coffset -> the stream offset of the member's text
        self.starts = [u for u, m in zip(self.uoff, members) if m[2]]
        self.cstarts = [c for c, m in zip(self.coff, members) if m[2]]
        self.n_ref, = struct.unpack_from("<i", header, 8 + struct.unpack_from("<i", header, 4)[0])
        self.records, at = [], len(header)
        for r in split_records(self.stream, at):
            self.records.append(decoded(r) + (self.virtual(at),))
            at += len(r)

    def virtual(self, at):
        """the virtual offset of stream offset `at`: the member whose text holds that byte (the EOF block's for the stream's end)"""
        if at >= len(self.stream):
            return V(self.eof)
        k = bisect.bisect_right(self.starts, at) - 1
        return V(self.cstarts[k], at - self.starts[k])

    def at(self, v):
        return len(self.stream) if v >> 16 == self.eof else self.first[v >> 16] + (v & 0xFFFF)

    def restated(self):
        return restated_index(self.n_ref, self.records, V(self.eof))


SETTINGS = ((1000, "200000"), (1 << 14, None), (400, "50000"))  # test_the_file_does_not_depend_on_batch_or_chunk_size's batch and chunk sizes
_RUNS = {}


def indexed_mc(api, golden, tmp_path_factory, k):
    """golden mc, ksw2, 4096-byte blocks, setting k: mapped once per module"""
    if k not in _RUNS:
        batch, chunk = SETTINGS[k]
        out = str(tmp_path_factory.mktemp("bai_mc") / f"o{k}.bam")
        with environment(MCX_BGZF_BLOCK="4096", MCX_SORT_CHUNK=chunk):
            st, route, stats, header = map_indexed(api, golden["mc"], "ksw2", out, batch)
        assert st["reads"] == 4000 and route[0] & api.ROUTE_INDEX and route[0] & api.ROUTE_SORT
        _RUNS[k] = (out, header, stats)
    return _RUNS[k]


@pytest.mark.gpu
def test_the_index_of_golden_mc_is_the_restatement_whatever_the_batch_and_chunk_size(api, golden, tmp_path_factory):
    parsed = []
    for k in range(3):
        out, header, stats = indexed_mc(api, golden, tmp_path_factory, k)
        data = open(out + ".bai", "rb").read()
        bam = WrittenBam(out, header)
        got = parse_bai(data)
        assert len(got["refs"]) == 3 and all(bins for bins, _ in got["refs"]) and got["n_no_coor"] == 46  # (three contigs with records, the unmapped lines of the set)
        assert got == bam.restated()
        assert stats["bytes"] == len(data) and stats["bins"] == sum(len(b) for b, _ in got["refs"]) and stats["intervals"] == sum(len(w) for _, w in got["refs"])
        assert stats["stretches"] == len(stretches_of(bam.records))
        # what of an index says nothing of offsets: the counts per contig, the records without one, the windows, the stretches
        parsed.append(([bins[META][1] for bins, _ in got["refs"]], got["n_no_coor"], [len(w) for _, w in got["refs"]], stats["stretches"], bam.stream))
        assert no_temporary_file(pathlib.Path(out).parent)
    # the chunks of the merge begin blocks of their own, so the three files differ in their blocks and the indexes in their offsets — each is its own file's (above);
    # the records are the same, and so is everything in the index that counts records
    assert parsed[0] == parsed[1] == parsed[2]


@pytest.mark.gpu
def test_the_bam_file_is_that_of_a_run_without_the_switch(api, golden, tmp_path_factory, tmp_path):
    out, header, _ = indexed_mc(api, golden, tmp_path_factory, 0)
    plain = str(tmp_path / "plain.bam")
    with environment(MCX_BGZF_BLOCK="4096", MCX_SORT_CHUNK=SETTINGS[0][1]):
        st, route, stats, _ = map_indexed(api, golden["mc"], "ksw2", plain, SETTINGS[0][0], index=False)
    assert open(plain, "rb").read() == open(out, "rb").read()
    assert not os.path.exists(plain + ".bai") and not route[0] & api.ROUTE_INDEX and not route[1] & api.ROUTE_INDEX


def reg2bins(beg, end):
    """the bins that may hold records overlapping [beg, end) (the SAM specification)"""
    end -= 1
    out = [0]
    for first, shift in ((1, 26), (9, 23), (73, 20), (585, 17), (4681, 14)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def query(bam, index, tid, beg, end):
    """what a reader does with the index: the region's bins, their chunks that end behind the linear entry of the region's first window, the records in them"""
    bins, linear = index["refs"][tid]
    min_off = linear[beg >> 14] if (beg >> 14) < len(linear) else (linear[-1] if linear else 0)
    chunks = sorted(c for b in reg2bins(beg, end) if b in bins for c in bins[b] if c[1] > min_off)
    found = []
    for u, v in chunks:
        at, stop = bam.at(u), bam.at(v)
        while at < stop:
            n = 4 + struct.unpack_from("<I", bam.stream, at)[0]
            t, b, e, mapped = decoded(bam.stream[at:at + n])
            if t == tid and b < end and e > beg:
                found.append(at)
            at += n
        assert at == stop  # a chunk ends where a record ends
    return found


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 2])
def test_every_region_finds_exactly_the_records_a_scan_finds(api, golden, tmp_path_factory, k):
    out, header, _ = indexed_mc(api, golden, tmp_path_factory, k)
    bam = WrittenBam(out, header)
    index = parse_bai(open(out + ".bai", "rb").read())
    lens = [n for _, n in decode_header(header)[1]]
    assert len(lens) == 3
    offsets, at = [], len(header)
    for r in split_records(bam.stream, at):
        offsets.append(at)
        at += len(r)
    rng = random.Random(77 + k)
    regions = []
    for _ in range(200):
        tid = rng.randrange(3)
        beg = rng.randrange(lens[tid])
        regions.append((tid, beg, min(lens[tid], beg + rng.choice((1, 100, 1000, 20000, 200000, lens[tid])))))
    for tid in range(3):
        last = max(r[2] for r in bam.records if r[0] == tid)
        regions += [(tid, 0, lens[tid]), (tid, last + 1, last + 5000)]  # the whole contig, and a region behind its last record
    found_any = 0
    for tid, beg, end in regions:
        want = [o for o, r in zip(offsets, bam.records) if r[0] == tid and r[1] < end and r[2] > beg]
        assert sorted(set(query(bam, index, tid, beg, end))) == want, (tid, beg, end)
        found_any += bool(want)
    assert found_any > 100


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["multi", "single-end", "resident"])
def test_the_index_on_the_other_routes(api, golden, tmp_path, what):
    with environment(MCX_BGZF_BLOCK="4096", MCX_SORT_CHUNK="100000", MCX_RESIDENT_LAUNCH_BYTES="65536" if what == "resident" else None):
        out = str(tmp_path / "o.bam")
        if what == "multi":
            st, route, stats, header = map_indexed(api, golden["mc"], "ksw2", out, 1000, multi=True)
        elif what == "single-end":
            st, route, stats, header = map_indexed(api, golden["se"], "ksw2", out, 400)
        else:
            g, files = golden["toy"], []
            for k, t in enumerate(tb.read_texts(g, "toy")):
                files.append(str(tmp_path / f"toy_{k + 1}.fq.gz"))
                tb.write_bgzf(files[-1], t, 3000)
            st, route, stats, header = map_indexed(api, g, "ksw2", out, 800, files=files, device_inflate=True, device_parse=True)
            everything = tb.ALL_FOUR | api.ROUTE_BGZF | api.ROUTE_BAM | api.ROUTE_SORT | api.ROUTE_INDEX
            assert route == (everything, everything)
    bam = WrittenBam(out, header)
    assert parse_bai(open(out + ".bai", "rb").read()) == bam.restated() and stats["stretches"] == len(stretches_of(bam.records)) > 10
    assert no_temporary_file(tmp_path)


@pytest.mark.gpu
def test_two_runs_give_the_same_index(api, golden, tmp_path):
    digests = []
    with environment(MCX_SORT_CHUNK="300000"):
        for k in range(2):
            out = str(tmp_path / f"run{k}.bam")
            map_indexed(api, golden["mc"], "nw", out, 1000)
            digests.append(hashlib.md5(open(out + ".bai", "rb").read()).hexdigest())
    assert digests[0] == digests[1]


@pytest.mark.gpu
def test_no_index_after_a_run_that_fails(api, golden, tmp_path):
    g = golden["toy"]
    with pytest.raises(Exception):
        map_indexed(api, g, "ksw2", str(tmp_path / "no_such_dir" / "o.bam"), 1000)
    assert not os.path.exists(str(tmp_path / "no_such_dir"))
    text = open(g["r2"], "rb").read()
    cut = str(tmp_path / "r2_cut.fq")
    open(cut, "wb").write(text[:len(text) // 2 + 7])  # file 2 ends inside a record, after the temporary file was made
    out = str(tmp_path / "cut.bam")
    open(out + ".bai", "wb").write(b"an index an earlier run left here")
    failed = False
    try:
        map_indexed(api, g, "ksw2", out, 400, files=(g["r1"], cut))
    except Exception:
        failed = True
    assert failed and not os.path.exists(out + ".bai") and no_temporary_file(tmp_path)


@pytest.mark.gpu
def test_the_refusals(api, golden, tmp_path):
    g = golden["toy"]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1000)
    L = api.lib()
    out = str(tmp_path / "refused.bam")

    def call(device_sam, path):
        fo = api.FileOpts()
        L.mcx_file_opts_default(C.byref(fo))
        fo.device_sam = device_sam
        st = api.Stats()
        rc = L.mcx_map_files_ex(mp._h, g["r1"].encode(), g["r2"].encode(), C.byref(fo), path.encode(), C.byref(st))
        err = L.mcx_last_error()
        assert not os.path.exists(out) and not os.path.exists(out + ".bai") and no_temporary_file(tmp_path)
        return rc, err

    rc, err = call(api.SAM_INDEX | api.SAM_BAM, out)
    assert rc == api.ERR_UNSUPPORTED and b"needs -sort" in err
    rc, err = call(api.SAM_INDEX | api.SAM_SORT | api.SAM_BAM, "-")
    assert rc == api.ERR_UNSUPPORTED and b"stdout" in err
    mp.close(); ix.close()


@pytest.mark.gpu
def test_a_contig_beyond_bai_s_reach_is_refused(api, golden, tmp_path):
    """the toy index under another name, its .ann saying that the first contig has 2^29 + 1 bases: refused in words before a file is opened (nothing is mapped)"""
    g = golden["toy"]
    prefix = str(tmp_path / "long")
    for ext in (".ann", ".amb", ".pac", ".bwt", ".sa"):
        shutil.copy(g["prefix"] + ext, prefix + ext)
    lines = open(prefix + ".ann").read().split("\n")
    off, n, n_ambs = lines[2].split()
    lines[2] = " ".join((off, str((1 << 29) + 1), n_ambs))
    open(prefix + ".ann", "w").write("\n".join(lines))
    ix = api.Index(prefix, device=0)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1000)
    out = str(tmp_path / "long.bam")
    with pytest.raises(Exception, match="2\\^29"):
        mp.map_files(g["r1"], g["r2"], out, bam=True, sort=True, index=True)
    assert not os.path.exists(out) and not os.path.exists(out + ".bai") and no_temporary_file(tmp_path)
    mp.close(); ix.close()


@pytest.mark.gpu
def test_cli_index(api, golden, tmp_path):
    g = golden["toy"]
    out = str(tmp_path / "cli.bam")
    args = [EXE, "-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-alg", "ksw2", "-no_vcf", "-batch", "1000"]
    env = dict(os.environ, MCX_TIMING="1", MCX_SORT_CHUNK="100000", TMPDIR=str(tmp_path))
    r = subprocess.run(args + ["-bam", out, "-sort", "-index"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert b"[mcx_map_files] index:" in r.stderr and b" stretches" in r.stderr and b"linear entries" in r.stderr
    ix = api.Index(g["prefix"], device=0)
    header = api.bam_header(ix, sorted=True)
    ix.close()
    bam = WrittenBam(out, header)
    assert parse_bai(open(out + ".bai", "rb").read()) == bam.restated()
    # without the switch: the same file, no index
    plain = str(tmp_path / "plain.bam")
    r = subprocess.run(args + ["-bam", plain, "-sort"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    assert r.returncode == 0 and open(plain, "rb").read() == bam.blob and not os.path.exists(plain + ".bai") and b"index:" not in r.stderr
    # the refusals, in words, before anything is opened
    bad = str(tmp_path / "bad.bam")
    for extra, words in ((["-bam", bad, "-index"], b"needs -bam -sort"), (["-sam", bad, "-index"], b"needs -bam -sort"), (["-bam", "-", "-sort", "-index"], b"stdout")):
        r = subprocess.run(args + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode != 0 and b"-index" in r.stderr and words in r.stderr and not r.stdout, r.stderr[-500:]
        assert not os.path.exists(bad) and not os.path.exists(bad + ".bai")
    assert no_temporary_file(tmp_path)
