"""The plain FM-index reference (tests/fm_ref.py) against the reference-made fixtures, and the product's seeding walk as it
runs on the host (tests/hostemu: mcx_fm.h compiled for the CPU, K = 7 jump table, with and without the host-made pair
records) against the plain walk, on the texts of tests/fm_cases.py.  No GPU."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

import fm_cases
import fm_ref
from conftest import GOLD

EDGES = os.path.join(GOLD, "fm_edges")
EXTS = ("pac", "ann", "amb", "bwt", "sa")
CASES = fm_cases.cases()
WALK_CASES = [n for n, c in CASES.items() if c.has_reads]
SEARCH_TEXTS = ("threshold", "at600", "palindrome")


def fixture_files(case):
    """ext -> bytes of the reference-made files kept for the case (none below 15 bases; .pac/.ann/.amb only for the long line)"""
    d = os.path.join(EDGES, case.note or case.name)
    return {e: open(os.path.join(d, f"idx.{e}"), "rb").read() for e in EXTS if os.path.exists(os.path.join(d, f"idx.{e}"))}


def golden_contigs(name):
    text = gzip.open(os.path.join(GOLD, name, "genome.fa.gz"), "rt").read()
    out = []
    for rec in text.split(">")[1:]:
        lines = rec.split("\n")
        head = lines[0].split(None, 1)
        out.append((head[0], head[1] if len(head) > 1 else None, "".join(lines[1:])))
    return out


# ---- the reference against itself and against the fixtures ---------------------------------------
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.G * 2 <= 2000])
def test_suffix_array_equals_the_sorted_suffixes(name):
    T = CASES[name].text().bytes
    assert list(fm_ref.suffix_array(np.frombuffer(T, dtype=np.uint8))) == sorted(range(len(T)), key=lambda i: T[i:])


def test_rand48_is_the_c_library_generator():
    g = fm_ref.Rand48(11)
    libc = ctypes.CDLL(None)
    libc.lrand48.restype = ctypes.c_long
    libc.srand48(ctypes.c_long(11))
    assert [g.lrand48() for _ in range(1000)] == [libc.lrand48() for _ in range(1000)]


@pytest.mark.parametrize("name", ["toy", "mc", "long"])
def test_index_files_equal_the_golden_sets(name):
    files = fm_ref.index_files(golden_contigs(name))
    for e in EXTS:
        assert files[e] == open(os.path.join(GOLD, name, f"idx.{e}"), "rb").read(), e


def test_every_text_of_15_bases_or_more_has_reference_files():
    for name, case in CASES.items():
        have = fixture_files(case) if case.has_fixture else {}
        if case.G < fm_cases.MIN_FIXTURE_G:
            assert not have and f"| {name} |" in open(os.path.join(EDGES, "README.md")).read()
        elif case.G > fm_cases.MAX_WALK_G:
            assert sorted(have) == ["amb", "ann", "pac"], name
        else:
            assert sorted(have) == sorted(EXTS), name
    total = sum(os.path.getsize(os.path.join(r, f)) for r, _d, fs in os.walk(EDGES) for f in fs)
    assert total < 400 * 1024


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.has_fixture])
def test_index_files_equal_the_fm_edges_fixtures(name):
    case = CASES[name]
    files, want = case.files(), fixture_files(case)
    assert want
    for e, data in want.items():
        assert files[e] == data, e


def test_search_equals_the_toy_vectors():
    text = fm_ref.Text(fm_ref.forward_codes(golden_contigs("toy"))[0])
    q = json.load(open(os.path.join(GOLD, "func", "bwt_search.json")))
    assert len(q) >= 1500
    for rec in q:
        codes = bytes("ACGTN".index(c) for c in rec["seq"])
        ln, fr, loc, _n = fm_ref.search(text, codes, rec["start"])
        assert (ln, fr, loc) == (rec["len"], rec["freq"], rec["loc"]), rec


def stored_searches(name):
    return json.load(gzip.open(os.path.join(EDGES, name, "searches.json.gz"), "rt"))


@pytest.mark.parametrize("name", SEARCH_TEXTS)
def test_search_and_walk_equal_the_stored_results(name):
    case = CASES[name]
    text, reads, stored = case.text(), fm_cases.reads_for(case), stored_searches(name)
    assert len(stored) == len(reads)
    for (_tag, codes), rec in zip(reads, stored):
        assert rec["seq"] == "".join("ACGTN"[c] for c in codes)
        triples = []
        for start, ln, fr, loc in rec["searches"]:
            got = fm_ref.search(text, codes, start)
            assert got[:3] == (ln, fr, loc), (rec["seq"], start)
            if start < len(codes) - 16:
                triples += [(g, start, ln) for g in loc]
        assert fm_ref.walk(text, codes) == triples, rec["seq"]


# ---- the premises of the read sets, on the reference's output ------------------------------------
def walk_searches(text, codes):
    """(start, len, freq, occurrences capped at 51, locations) of every search of the walk"""
    out, pos = [], 0
    while pos < len(codes) - 16:
        if codes[pos] > 3:
            pos += 1
            continue
        ln, fr, loc, n = fm_ref.search(text, codes, pos)
        out.append((pos, ln, fr, n, loc))
        pos += ln + 1
    return out


_SEARCHES = {}


def searches_of(name):
    if name not in _SEARCHES:
        case = CASES[name]
        _SEARCHES[name] = [(tag, codes, walk_searches(case.text(), codes)) for tag, codes in fm_cases.reads_for(case)]
    return _SEARCHES[name]


def test_the_planted_counts_are_what_was_planned():
    case = CASES["threshold"]
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    for name, (kmer, count) in case.planted.items():
        for k in (kmer, fm_ref.revcomp(kmer)):
            assert len(fm_ref.occurrences(case.text().bytes, bytes(code[c] for c in k))) == count, name
    assert case.planted["k50"][1] == 50 and case.planted["k52"][1] == 52


@pytest.mark.parametrize("name", WALK_CASES)
def test_read_sets_hold_their_premises(name):
    """What the reads are for, stated on the plain reference's results: every text has a search that stops at the text's
    end, one that crosses the strand junction at G, and searches of exactly 15, 16 and 17 bases; the threshold text has
    a search that keeps exactly 50 rows and one that drops more than 50, kept intervals of 2, 3, 7, 8 and 9 rows, and
    kept intervals that begin on even and on odd rows; the periodic deep texts drop an interval of more than 50 rows, the
    two-copy ones keep one of a piece of 150 bases or more."""
    case, text = CASES[name], CASES[name].text()
    all_s = [(codes, s) for _tag, codes, ss in searches_of(name) for s in ss]
    assert 250 <= len(fm_cases.reads_for(case)) <= 400
    lens = {s[1] for _c, s in all_s}
    assert {15, 16, 17} <= lens, sorted(lens)
    # (the last pattern is a suffix of the text and the read goes on with a base: nothing but the text's end stopped that occurrence)
    assert any(text.bytes.endswith(codes[start:start + ln]) and start + ln < len(codes) and codes[start + ln] <= 3 for codes, (start, ln, _fr, _n, _loc) in all_s), "no search stops at the text's end"
    # (an occurrence of the last pattern lies over the junction — kept or not: in the periodic texts everything occurs often)
    assert any(ln >= 16 and any(text.bytes.startswith(codes[start:start + ln], text.G - k) for k in range(1, ln)) for codes, (start, ln, _fr, _n, _loc) in all_s), "no search crosses G"
    if case.kind == "threshold":
        assert any(fr == 50 for _c, (_s, _l, fr, _n, _loc) in all_s)
        assert any(ln >= 16 and n > 50 for _c, (_s, ln, _fr, n, _loc) in all_s)
        assert {2, 3, 7, 8, 9, 50} <= {fr for _c, (_s, _l, fr, _n, _loc) in all_s}
        first_rows = {(int(text.rank[loc[0]]) + 1) & 1 for _c, (_s, _l, fr, _n, loc) in all_s if fr > 1}
        assert first_rows == {0, 1}
    if case.kind == "deep" and name in ("palindrome", "dup1500"):  # every long piece of these occurs twice, or four times
        assert any(ln >= 150 and fr >= 2 for _c, (_s, ln, fr, _n, _loc) in all_s)
    elif case.kind == "deep":
        assert any(ln >= 16 and n > 50 for _c, (_s, ln, _fr, n, _loc) in all_s)


# ---- the product's walk on the host against the plain walk -----------------------------------------
HIT = np.dtype([("gPos", np.int64), ("rPos", np.int32), ("len", np.int32)])
CAP = 1024


@pytest.fixture(scope="module")
def host_walk(hostemu_lib):
    f = hostemu_lib.hostemu_seed_walk
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]

    def run(prefix, pairs, reads, fm_budget, cap=CAP):
        seqs = [fm_cases.ascii_of(codes) for _tag, codes in reads]
        off = np.zeros(len(seqs) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(s) for s in seqs])
        buf = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy()
        n_hits = np.zeros(len(seqs), dtype=np.int32)
        hits = np.zeros((len(seqs), cap), dtype=HIT)
        assert f(prefix.encode(), pairs, buf.ctypes.data, off.ctypes.data, len(seqs), fm_budget, cap, n_hits.ctypes.data, hits.ctypes.data) == 0
        return n_hits, hits
    return run


@pytest.mark.parametrize("pairs", [0, 1], ids=["single_steps", "pair_records"])
@pytest.mark.parametrize("name", WALK_CASES)
def test_host_walk_equals_the_plain_walk(host_walk, tmp_path, name, pairs):
    case = CASES[name]
    prefix = fm_cases.write_index(case, str(tmp_path / "idx"))
    for fm_budget in (1 << 30, 3):
        n_hits, hits = host_walk(prefix, pairs, fm_cases.reads_for(case), fm_budget)
        assert max(n_hits) <= CAP
        bad = fm_cases.compare_walks(case, n_hits, hits, CAP)
        assert not bad, (fm_budget, len(bad), bad[:2])
