"""-markdup on the host: the rule restated in Python — it is the specification — and the arithmetic of mapcaller_amd/csrc/mcx_markdup.h (a record's end, score and
packed end), compiled for the host by tests/hostemu/markdup_check.cpp, held against it on hand-packed records.

The restatement is written from the rule's words, not from the header: a record is unpacked with struct, its CIGAR made a list of (length, operation) pairs, and
the end read off that list.  tests/test_markdup_device.py takes the same functions for the kernels and the front end."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "hostemu", "markdup_check.cpp")
OPS = "MIDNSHP=X"
ONES = (1 << 64) - 1


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def pack_record(ref_id, pos, flag, cigar=(), qual=b"", name=b"r", extra=b""):
    """a BAM record by hand: ``cigar`` a list of (length, letter), ``qual`` the QUAL bytes (their number is l_seq), ``extra`` for tags"""
    words = b"".join(struct.pack("<I", n << 4 | OPS.index(op)) for n, op in cigar)
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) + 1, 0, 4680, len(cigar), flag, len(qual), -1, -1, 0) + name + b"\0" + words + bytes((len(qual) + 1) // 2) + bytes(qual) + extra
    return struct.pack("<I", len(body)) + body


def fields(rec):
    size, ref_id, pos, l_name, _, _, n_cigar, flag, l_seq = struct.unpack_from("<IiiBBHHHI", rec, 0)
    at = 36 + l_name
    if at + 4 * n_cigar > len(rec):
        return dict(ref_id=ref_id, pos=pos, flag=flag, cigar=[], qual=b"", fits=False)
    cigar = [(w >> 4, OPS[w & 15]) for w in struct.unpack_from("<%dI" % n_cigar, rec, at)]
    at += 4 * n_cigar + (l_seq + 1) // 2
    return dict(ref_id=ref_id, pos=pos, flag=flag, cigar=cigar, qual=rec[at:at + l_seq], fits=at + l_seq <= len(rec) and 4 + size == len(rec))


def placed(rec):
    return not struct.unpack_from("<H", rec, 18)[0] & 4


def end_of(rec):
    """(refID, u5, reverse): the unclipped 5' end"""
    f = fields(rec)
    clips = lambda ops: sum(n for n, _ in ops[:next((k for k, (_, op) in enumerate(ops) if op not in "SH"), len(ops))])  # noqa: E731
    if not f["flag"] & 0x10:
        return f["ref_id"], f["pos"] - clips(f["cigar"]), 0
    reflen = sum(n for n, op in f["cigar"] if op in "MDN=X")
    return f["ref_id"], f["pos"] + reflen - 1 + clips(f["cigar"][::-1]), 1


def score_of(rec):
    return sum(q for q in fields(rec)["qual"] if 15 <= q != 0xff)


def in_range(end, rec=None):
    """what a packed end must hold apart: n_ref < 2^24, |u5| < 2^38 (and, the implementation's own bound, fewer than 2^23 bases)"""
    return 0 <= end[0] < (1 << 24) - 1 and abs(end[1]) < 1 << 38 and (rec is None or len(fields(rec)["qual"]) < 1 << 23)


def units_of(groups, paired):
    """groups: per read the list of its records.  A unit: (kind, key, score, the reads that carry its verdict); kind 'pair', 'fragment' or None"""
    first = [g[0] if g and placed(g[0]) else None for g in groups]
    units = []
    for k in range(0, len(groups), 2 if paired else 1):
        reads = [r for r in range(k, k + (2 if paired else 1)) if first[r] is not None]
        if len(reads) == 2:
            units.append(("pair", tuple(sorted(end_of(first[r]) for r in reads)), sum(score_of(first[r]) for r in reads), reads))
        elif len(reads) == 1:
            units.append(("fragment", end_of(first[reads[0]]), score_of(first[reads[0]]), reads))
        else:
            units.append((None, None, 0, []))
    return units


def resolve(units):
    """per unit: is it a duplicate; and the groups — keys two or more pairs share, plus ends on which a fragment is a duplicate"""
    dup = [False] * len(units)
    best_first = lambda members: sorted(members, key=lambda u: (-units[u][2], u))  # noqa: E731
    pairs, frags, pair_ends = {}, {}, set()
    for u, (kind, key, _, _) in enumerate(units):
        if kind == "pair":
            pairs.setdefault(key, []).append(u)
            pair_ends.update(key)
        elif kind == "fragment":
            frags.setdefault(key, []).append(u)
    groups = 0
    for members in pairs.values():
        for u in best_first(members)[1:]:
            dup[u] = True
        groups += len(members) > 1
    for end, members in frags.items():
        losers = members if end in pair_ends else best_first(members)[1:]
        for u in losers:
            dup[u] = True
        groups += len(losers) > 0
    return dup, groups


def read_verdicts(groups, paired):
    """per read: does its record get flag bit 0x400"""
    units = units_of(groups, paired)
    dup, n_groups = resolve(units)
    out = [False] * len(groups)
    for u, (_, _, _, reads) in enumerate(units):
        for r in reads:
            out[r] = dup[u]
    return out, units, dup, n_groups


def packed_of(end):
    return end[0] << 40 | (end[1] + (1 << 38)) << 1 | end[2]


# ---- the header, compiled for the host -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def markdup_check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("markdup_check") / "libmarkdup_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", SRC, "-o", out], check=True, stderr=subprocess.PIPE, timeout=600)
    L = C.CDLL(out)
    L.markdup_check_record.restype = C.c_int
    L.markdup_check_record.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_int64)]
    return L


def host_says(L, rec):
    out = (C.c_int64 * 6)()
    rc = L.markdup_check_record(bytes(rec), len(rec), out)
    return rc, [int(v) for v in out]


Q = bytes([14, 15, 0xff, 40, 0, 93, 15, 14])  # scores 15 + 40 + 93 + 15
BIG = (1 << 28) - 1  # the longest operation a CIGAR word holds


def cases():
    """(name, record): what the issue lists, and the corners of the CIGAR walk"""
    c = []
    add = lambda title, *a, **k: c.append((title, pack_record(*a, **k)))  # noqa: E731
    for flag in (0, 0x10):
        s = "reverse " if flag else "forward "
        add(s + "plain", 3, 1000, flag, [(50, "M")], Q)
        add(s + "leading S", 3, 1000, flag, [(7, "S"), (43, "M")], Q)
        add(s + "trailing S", 3, 1000, flag, [(43, "M"), (7, "S")], Q)
        add(s + "leading H", 3, 1000, flag, [(9, "H"), (50, "M")], Q)
        add(s + "trailing H", 3, 1000, flag, [(50, "M"), (9, "H")], Q)
        add(s + "both on both sides", 3, 1000, flag, [(2, "H"), (5, "S"), (30, "M"), (6, "S"), (3, "H")], Q)
        add(s + "D and N", 3, 1000, flag, [(10, "M"), (4, "D"), (10, "M"), (500, "N"), (10, "M"), (2, "I"), (5, "="), (3, "X"), (1, "P"), (4, "S")], Q)
        add(s + "no reference taken", 3, 1000, flag, [(5, "S"), (20, "I"), (5, "S")], Q)
        add(s + "only clips", 3, 1000, flag, [(5, "S"), (5, "H")], Q)
        add(s + "no CIGAR", 3, 1000, flag, [], Q)
        add(s + "an S in the middle ends the leading ones", 3, 1000, flag, [(3, "S"), (10, "M"), (4, "S"), (10, "M"), (2, "S")], Q)
        add(s + "negative u5", 0, 2, flag, [(40, "S"), (10, "M")] if not flag else [(1, "M")], Q, name=b"neg")
        add(s + "pos -1", 0, -1, flag, [(10, "M")], Q)
        add(s + "refID -1 without flag 4", -1, 5, flag, [(10, "M")], Q)
        add(s + "flag 4", 2, 77, flag | 4, [(10, "M")], Q)
        add(s + "refID -1 with flag 4", -1, -1, flag | 4, [], Q)
        add(s + "l_seq 0", 1, 10, flag, [(10, "M")], b"")
        add(s + "refID at the limit", (1 << 24) - 2, 10, flag, [(10, "M")], Q)
        add(s + "refID one past", (1 << 24) - 1, 10, flag, [(10, "M")], Q)
    for k, q in enumerate((b"", bytes([14]), bytes([15]), bytes([0xff]), bytes([0xff] * 20), bytes(range(256)), bytes([14, 15] * 100), bytes([41]) * 5000)):
        add("quality %d, of %d bytes" % (k, len(q)), 0, 0, 0, [(1, "M")], q, name=b"a-name-of-some-length")
    # u5 at the packing's limits and one past them: 2^38 is 1024 operations of 2^28
    far = (1 << 31) - 1
    more = lambda total: [(BIG, "S")] * (total // BIG) + ([(total % BIG, "S")] if total % BIG else [])  # noqa: E731
    add("u5 = 2^38 - 1", 0, far, 0x10, [(1, "M")] + more((1 << 38) - 1 - far))
    add("u5 = 2^38", 0, far, 0x10, [(1, "M")] + more((1 << 38) - far))
    add("u5 = -(2^38 - 1)", 0, 0, 0, more((1 << 38) - 1) + [(1, "M")])
    add("u5 = -2^38", 0, 0, 0, more(1 << 38) + [(1, "M")])
    return c


def test_the_cases_are_what_the_issue_lists():
    names = [n for n, _ in cases()]
    assert len(names) == len(set(names)) == 50
    ends = {n: end_of(r) for n, r in cases()}
    assert ends["forward leading S"] == (3, 993, 0) and ends["forward trailing S"] == (3, 1000, 0) and ends["reverse trailing S"] == (3, 1049, 1) and ends["reverse leading S"] == (3, 1042, 1)
    assert ends["forward both on both sides"] == (3, 993, 0) and ends["reverse both on both sides"] == (3, 1038, 1)
    assert ends["reverse D and N"] == (3, 1000 + 542 - 1 + 4, 1) and ends["reverse no reference taken"] == (3, 1004, 1) and ends["reverse only clips"] == (3, 1009, 1)
    assert ends["forward negative u5"][1] == -38 and ends["reverse pos -1"][1] == 8 and ends["forward pos -1"][1] == -1
    assert ends["forward an S in the middle ends the leading ones"][1] == 997 and ends["reverse an S in the middle ends the leading ones"][1] == 1000 + 20 - 1 + 2
    assert ends["u5 = 2^38"][1] == 1 << 38 and ends["u5 = -2^38"][1] == -(1 << 38) and ends["u5 = 2^38 - 1"][1] == (1 << 38) - 1
    assert score_of(pack_record(0, 0, 0, [], Q)) == 163 and score_of(pack_record(0, 0, 0, [], bytes(range(256)))) == sum(range(15, 255))


def test_end_score_and_packed_end_are_the_rule(markdup_check):
    seen = set()
    for name, rec in cases():
        rc, (ref_id, u5, reverse, score, is_placed, packed) = host_says(markdup_check, rec)
        end = end_of(rec)
        assert (ref_id, u5, reverse) == end, name
        assert score == score_of(rec) and bool(is_placed) == placed(rec), name
        assert rc == (1 if in_range(end, rec) else 0), name
        assert packed & ONES == (packed_of(end) if rc else ONES), name
        if rc:
            assert packed & ONES != ONES
            seen.add((end, packed & ONES))
    # injective, and ordered like the ends
    assert len({e for e, _ in seen}) == len({p for _, p in seen})
    assert [e for e, _ in sorted(seen)] == [e for e, _ in sorted(seen, key=lambda s: s[1])]
    out_of_range = [n for n, r in cases() if not in_range(end_of(r))]
    assert sorted(out_of_range) == sorted(["u5 = 2^38", "u5 = -2^38", "forward refID one past", "reverse refID one past", "forward refID -1 without flag 4", "reverse refID -1 without flag 4",
                                           "forward refID -1 with flag 4", "reverse refID -1 with flag 4"])


def test_a_record_shorter_than_its_fields_is_refused(markdup_check):
    rec = pack_record(1, 5, 0, [(10, "M")], Q, extra=b"NMC\1")
    assert host_says(markdup_check, rec)[0] == 1
    bare = pack_record(1, 5, 0, [(10, "M")], Q)
    for cut in range(1, len(bare) - 35):  # the record ends inside its QUAL, SEQ, CIGAR or name
        short = struct.pack("<I", len(bare) - 4 - cut) + bare[4:len(bare) - cut]
        assert not fields(short)["fits"] and host_says(markdup_check, short)[0] == -1, cut
    assert host_says(markdup_check, rec[:-1])[0] == -1 and host_says(markdup_check, rec[:20])[0] == -1  # block_size says another length


def test_the_standalone_program_says_the_same(tmp_path, markdup_check):
    """tests/hostemu/markdup_check.cpp with its own main (the form a sanitizer build takes), built plainly here"""
    exe = str(tmp_path / "markdup_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DMARKDUP_CHECK_MAIN", "-Wall", "-Wno-unused-function", SRC, "-o", exe], check=True, stderr=subprocess.PIPE, timeout=600)
    records = dump_records()
    src, dst = str(tmp_path / "records.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<Q", len(records)))
        for r in records:
            f.write(struct.pack("<Q", len(r)) + r)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and r.stdout == b"%d records\n" % len(records), r.stderr
    got = np.fromfile(dst, dtype=np.int64).reshape(-1, 7)
    for k, rec in enumerate(records):
        rc, vals = host_says(markdup_check, rec)
        assert int(got[k][6]) == rc and (rc < 0 or [int(v) for v in got[k][:6]] == vals), k


def dump_records():
    """the cases, and the same records cut short at every length of one of them"""
    records = [r for _, r in cases()]
    bare = pack_record(1, 5, 0x10, [(3, "S"), (10, "M"), (2, "H")], Q)
    records += [struct.pack("<I", len(bare) - 4 - cut) + bare[4:len(bare) - cut] for cut in range(1, len(bare) - 35)]
    records += [bare[:k] for k in (0, 3, 20, 35)]
    return records


# ---- the restatement against itself: small cases whose answer is plain ------------------------------------------------------------------
def test_the_restated_rule_on_cases_read_off_the_words():
    fwd = lambda pos, q, flag=0: pack_record(0, pos, flag, [(10, "M")], bytes([q] * 10))  # noqa: E731
    # three pairs on one key: the best score stays, a tie goes to the first; a fourth pair shares the first end only
    groups = [[fwd(100, 20)], [fwd(300, 20, 0x10)], [fwd(100, 30)], [fwd(300, 30, 0x10)], [fwd(100, 30)], [fwd(300, 30, 0x10)], [fwd(100, 40)], [fwd(301, 40, 0x10)]]
    verdict, units, dup, n_groups = read_verdicts(groups, True)
    assert dup == [True, False, True, False] and n_groups == 1 and verdict == [True, True, False, False, True, True, False, False]
    # a fragment on a pair's end loses whatever it scores; on no pair's end the best fragment stays; an unplaced mate is never flagged; a read without a record is none
    groups = [[fwd(100, 20)], [fwd(300, 20, 0x10)], [fwd(100, 41)], [pack_record(0, 100, 4 | 0x20, [], b"")], [fwd(300, 41, 0x10)], [], [fwd(500, 20)], [pack_record(-1, -1, 4)],
              [pack_record(-1, -1, 4)], [fwd(500, 21)], [], []]
    verdict, units, dup, n_groups = read_verdicts(groups, True)
    assert [u[0] for u in units] == ["pair", "fragment", "fragment", "fragment", "fragment", None]
    assert dup == [False, True, True, True, False, False] and n_groups == 3
    assert verdict == [False, False, True, False, True, False, True, False, False, False, False, False]
    # single-end: every placed read is a fragment
    verdict, units, dup, n_groups = read_verdicts([[fwd(7, 20)], [fwd(7, 20)], [fwd(7, 20, 0x10)], [], [fwd(7, 25)]], False)
    assert verdict == [True, True, False, False, False] and n_groups == 1


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
NEW = ("mcx_bam_dup_units_dev", "mcx_dup_resolve_dev", "mcx_bam_dup_mark_dev", "mcx_markdup_last_ms", "mcx_files_markdup_stats")


def test_the_calls_are_declared_bound_and_exported():
    import inspect
    import re
    from mapcaller_amd import api, run
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for s in NEW:
        assert s in api.SYMBOLS and re.search(r"\b%s\s*\(" % s, header), s
    for name, value in (("MCX_SAM_MARKDUP", 32), ("MCX_ROUTE_MARKDUP", 256)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
    assert api.SAM_MARKDUP == 32 and api.ROUTE_MARKDUP == 256
    assert re.search(r"typedef struct mcx_dup_unit\s*\{\s*uint64_t end0, end1;\s*uint32_t score, kind;\s*\}", header) and api.DUP_UNIT_DTYPE.itemsize == 24
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in NEW:
            assert f" {s}\n" in nm, s
        L = api.lib()
        assert [len(getattr(L, s).argtypes) for s in NEW] == [8, 4, 6, 2, 2] and all(getattr(L, s).restype is C.c_int for s in NEW)
    assert inspect.signature(api.Mapper.map_files).parameters["markdup"].default is False
    assert all(m in dir(api.Mapper) for m in ("bam_dup_units", "dup_resolve", "bam_dup_mark", "markdup_stats", "markdup_last_ms"))
    a = run.parse(["-i", "x", "-f", "a.fq", "-bam", "o.bam", "-sort", "-markdup"])
    assert a.markdup and a.sort and not run.parse(["-i", "x", "-f", "a.fq", "-bam", "o.bam", "-sort"]).markdup
    main = open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_main.cpp")).read()
    assert '"-markdup"' in main and "MCX_SAM_MARKDUP" in main and "-markdup      with -bam -sort" in main
