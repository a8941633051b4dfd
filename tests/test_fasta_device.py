"""FASTA reads parsed on the device: mcx_fastq_parser_set_format (MCX_READS_FASTA) under the plain rule and the GZ rule, the file front end's device_parse
(-gpu_parse) on plain FASTA files and the resident route (-gpu_inflate -gpu_parse) on BGZF FASTA.

Expectations come from a restatement, in Python, of the reference's FASTA readers (GetNextEntry, GetData.cpp:56-77: a header line, then every line up to the
next line that begins with '>', each less its last byte; gzGetNextEntry, :101-128: gzgets pieces of at most 1023 bytes, a header piece and ONE sequence
piece) as mcx_reader.h's Parser::entry holds them.  Nothing is expected from the code under test; the header rule, the output layout and the drivers are
tests/test_fastq_device.py's, the pieces tests/test_bgzf_resident.py's.
CPU: the surface; the restatement on a record worked by hand; the rules compiled for the host (mcx_fastq.h through tests/hostemu/fasta_check.cpp) against
it on every vector and on a text cut at every byte; the restatement against the product's own sequential reader; the host build as a stand-alone program
under -fsanitize=address,undefined.  GPU: the kernels on every vector under both rules, at every alignment, a text fed in pieces, the host-buffer form,
the refusals; the front end on the golden FASTA sets with the switches on, its fallbacks, its ends of input against the host route, the command line."""
import ctypes as C
import gzip
import os
import random
import re
import struct
import subprocess
import threading

import numpy as np
import pytest

import test_bgzf_resident as tb
import test_fastq_device as tf
from conftest import ROOT, VCF_RUNS, VcfOpts, sam_diff, vcf_alg, vcf_body

CHECK_SRC = os.path.join(ROOT, "tests", "hostemu", "fasta_check.cpp")
EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
MORE, END, EMPTY, TOO_LONG = 0, 1, 2, 3
PLAIN, GZ = 0, 1
ALL_FOUR = 1 | 2 | 4 | 8


# ---- CPU: the surface ---------------------------------------------------------------------------------------
def test_set_format_is_declared_bound_and_exported():
    from mapcaller_amd import api
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    s = "mcx_fastq_parser_set_format"
    assert s in api.SYMBOLS and re.search(r"\bint\s+%s\s*\(\s*mcx_fastq_parser\s*\*\s*,\s*int\s+format\s*\)" % s, header)
    m = re.search(r"enum\s+mcx_reads_format\s*\{([^}]*)\}", header)
    assert m and [x.strip() for x in m.group(1).split(",")] == ["MCX_READS_FASTQ = 0", "MCX_READS_FASTA = 1"]
    assert (api.READS_FASTQ, api.READS_FASTA) == (0, 1)
    assert callable(api.FastqParser.set_format)
    assert (C.sizeof(api.FastqIn), C.sizeof(api.FastqOut), C.sizeof(api.FastqInfo)) == (48, 112, 64)  # (the structs keep their layout)
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        assert f" {s}\n" in nm
        L = api.lib()
        assert L.mcx_fastq_parser_set_format.restype is C.c_int and L.mcx_fastq_parser_set_format.argtypes == [C.c_void_p, C.c_int]
    main = open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_main.cpp")).read()
    assert "FASTA" in main[main.index("-gpu_parse    "):][:400]


# ---- the rules, restated ------------------------------------------------------------------------------------
def getlines(text):
    """[(start, end)]: what getline gives, up to and including the newline; the last line may lack it"""
    out, at = [], 0
    while at < len(text):
        e = text.find(b"\n", at)
        e = len(text) if e < 0 else e + 1
        out.append((at, e))
        at = e
    return out


def restate_plain_text(text, max_records, max_read_len, final):
    """(records as tuples of REC_DTYPE's fields, their sequences, stop, consumed) of one text under plain FASTA: the first line is a header (GetNextEntry reads
    it as one whatever it holds), then lines are appended less their last byte until one begins with '>', which is the next header"""
    lines = getlines(text)
    heads = [i for i, (s, _) in enumerate(lines) if i == 0 or text[s] == 0x3E]
    recs, seqs, stop = [], [], MORE
    while len(recs) < max_records:
        k = len(recs)
        if k >= len(heads):
            stop = END if final else MORE
            break
        h = heads[k]
        nxt = heads[k + 1] if k + 1 < len(heads) else len(lines)
        s, e = lines[h]
        p1, name_len = tf.header_span(text[s:e])
        seq = b"".join(text[a:b - 1] for a, b in lines[h + 1:nxt])
        if not final and k + 1 >= len(heads):  # no later header yet: more of this record may follow
            stop = TOO_LONG if len(seq) > max_read_len else MORE
            break
        if len(seq) == 0:
            stop = EMPTY
            break
        if len(seq) > max_read_len:
            stop = TOO_LONG
            break
        recs.append((s + p1, name_len, e, len(seq), 0, 0))
        seqs.append(seq)
    k = len(recs)
    return recs, seqs, stop, lines[heads[k]][0] if k < len(heads) else len(text)


def restate_gz_text(text, max_records, max_read_len, final):
    """the same under the GZ rule: record k is pieces 2k (header) and 2k + 1 (the sequence), C lengths"""
    P = tb.gz_pieces(text)

    def complete(q):
        return q < len(P) and (text[P[q][1] - 1:P[q][1]] == b"\n" or P[q][1] - P[q][0] == tb.PIECE)
    recs, seqs, stop = [], [], MORE
    while len(recs) < max_records:
        k = len(recs)
        if not final and not (complete(2 * k) and complete(2 * k + 1)):
            break
        if 2 * k >= len(P):
            stop = END
            break
        hs, he = P[2 * k]
        cl = tb.c_len(text[hs:he])
        if cl == 0 or text[hs] not in b"@>":
            stop = EMPTY
            break
        p1, name_len = tf.header_span(text[hs:hs + cl])
        if 2 * k + 1 >= len(P):
            stop = EMPTY
            break
        ss, se = P[2 * k + 1]
        cl = tb.c_len(text[ss:se])
        rlen = cl - 1 if cl else 0
        if rlen == 0:
            stop = EMPTY
            break
        if rlen > max_read_len:
            stop = TOO_LONG
            break
        recs.append((hs + p1, name_len, ss, rlen, 0, 0))
        seqs.append(text[ss:ss + rlen])
    k = len(recs)
    return recs, seqs, stop, P[2 * k][0] if 2 * k < len(P) else len(text)


RESTATE = {PLAIN: restate_plain_text, GZ: restate_gz_text}


def restate(lib, rule, texts, max_records, max_read_len, final, row_words=None):
    """Every output of the call as a dict of numpy arrays (and "info"), in tf.restate's form; rows and odd bytes through mcx_pack_row."""
    per = [RESTATE[rule](t, max_records, max_read_len, final) for t in texts]
    n_rec = [len(p[0]) for p in per]
    n = n_rec[0] if len(texts) == 1 else 2 * min(n_rec)
    where = [(0, r) if len(texts) == 1 else (r & 1, r >> 1) for r in range(n)]
    reads = [(t, per[t][0][i], per[t][1][i]) for t, i in where]
    bases = b"".join(s for _, _, s in reads)
    names = b"".join(texts[t][c[0]:c[0] + c[1]] for t, c, _ in reads)
    lens = np.array([c[3] for _, c, _ in reads], dtype=np.uint32)
    if row_words is None:
        row_words = (max(max_read_len, 0) + 15) // 16
    rows = np.zeros((n, row_words), dtype=np.uint32)
    odd_cap = len(bases) + 1
    odd = np.zeros(odd_cap, dtype=np.uint64)
    n_odd = C.c_uint32(0)
    for r, (_, c, s) in enumerate(reads):
        seq = np.frombuffer(s, dtype=np.uint8)
        lib.mcx_pack_row(seq.ctypes.data, c[3], r, rows[r].ctypes.data, row_words, odd.ctypes.data, odd_cap, C.byref(n_odd))
    out = {"recs": [np.array(p[0], dtype=np.uint32).reshape(-1, 6) for p in per],
           "bases": np.frombuffer(bases, dtype=np.uint8), "qual": np.zeros(len(bases), dtype=np.uint8), "names": np.frombuffer(names, dtype=np.uint8),
           "off": np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)]).astype(np.uint32),
           "name_off": np.concatenate([[0], np.cumsum([c[1] for _, c, _ in reads], dtype=np.uint64)]).astype(np.uint32),
           "rows": rows, "len": lens, "odd": odd[:n_odd.value].copy(), "row_words": row_words}
    out["info"] = {"n_records": n_rec + [0] * (2 - len(texts)), "stop": [p[2] for p in per] + [0] * (2 - len(texts)),
                   "consumed": [p[3] for p in per] + [0] * (2 - len(texts)), "n_reads": n, "longest": int(lens.max()) if n else 0, "n_odd": int(n_odd.value),
                   "n_bases": len(bases), "n_name_bytes": len(names)}
    return out


packer = tf.packer


def test_the_restatement_on_a_record_worked_by_hand(packer):
    t = b">>r1/1 x\nACN\nT>\n\n>r2\nGGA"  # lines at 0, 9, 13, 16, 17, 21; 24 bytes
    recs, seqs, stop, consumed = restate_plain_text(t, 10, 8, True)
    assert recs == [(2, 2, 9, 5, 0, 0), (18, 2, 21, 2, 0, 0)] and seqs == [b"ACNT>", b"GG"] and stop == END and consumed == 24
    e = restate(packer, PLAIN, [t], 10, 8, True)
    assert e["bases"].tobytes() == b"ACNT>GG" and e["qual"].tobytes() == bytes(7) and e["names"].tobytes() == b"r1r2" and e["off"].tolist() == [0, 5, 7]
    assert e["rows"][:, 0].tolist() == [0b0001001100 << 22, 0b1010 << 28] and e["odd"].tolist() == [(2 << 8) | ord("N"), (4 << 8) | ord(">")]
    assert restate_plain_text(t, 10, 8, False)[2:] == (MORE, 17)      # (the last record may go on)
    assert restate_plain_text(t, 10, 4, True)[2:] == (TOO_LONG, 0)
    assert restate_plain_text(t[:21], 10, 8, True)[2:] == (EMPTY, 17)  # (a header last)
    # the GZ rule: a header piece and ONE sequence piece; the piece behind them is no header, and the input ends
    recs, seqs, stop, consumed = restate_gz_text(t, 10, 8, True)
    assert recs == [(2, 2, 9, 3, 0, 0)] and seqs == [b"ACN"] and stop == EMPTY and consumed == 13


# ---- the vectors --------------------------------------------------------------------------------------------
def fa(name, seq, width=0, nl=b"\n"):
    """a record: single-line (width 0), or folded to `width` columns"""
    body = seq + nl if not width else b"".join(seq[i:i + width] + nl for i in range(0, len(seq), width))
    return b">" + name + nl + body


def seeded_text(seed=5, size=200 * 1024, widths=(0, 0, 60, 60, 17, 1)):
    rng = random.Random(seed)
    out, k = [], 0
    while sum(map(len, out)) < size:
        n = rng.randint(1, 300)
        seq = bytes(rng.choice(b"ACGT") if rng.random() > 0.01 else rng.choice(b"NacgtRY") for _ in range(n))
        out.append(fa(b"r%d%s" % (k, rng.choice([b"", b" x", b"/1", b"\tq"])), seq, rng.choice(widths)))
        k += 1
    return b"".join(out)


def make_vectors():
    """[(name, text, max_read_len)], each under 64 KB but the seeded one"""
    acgt = b"ACGTTGCA" * 700
    four = b"".join(fa(b"read%d/1" % i, s) for i, s in enumerate([b"ACGTACGTAC", b"TTTTGGGGCCCCAAAA", b"GATTACA", b"ACGTACGTACGTACGTACGTACGTACGTACGTA"]))
    folded = b"".join(fa(b"ml%d" % i, acgt[i:i + n], 60) for i, n in enumerate((59, 60, 61, 120, 121, 250)))
    v = [("four", four, 300), ("folded_60", folded, 300), ("no_final_newline", four[:-1], 300), ("folded_no_final_newline", folded[:-1], 300),
         ("empty", b"", 300), ("newline", b"\n", 300),
         ("many_lines", fa(b"a", b"ACGT") + fa(b"many", acgt[:300], 3) + fa(b"b", b"GG"), 300),  # 100 lines in a record
         ("long_line", fa(b"a", b"ACGT") + fa(b"long", acgt[:1500]) + fa(b"b", b"GG"), 2000),
         ("empty_lines_inside", b">a\nACGT\n\n\nGGTT\n\n>b\n\nCC\n", 300),
         ("header_header", fa(b"a", b"ACGT") + b">b\n>c\nGG\n", 300), ("header_last", fa(b"a", b"ACGT") + b">b\n", 300), ("header_last_unterminated", fa(b"a", b"ACGT") + b">b", 300),
         ("first_line_no_gt", b"name here\nACGT\nGG\n" + fa(b"b", b"TT"), 300), ("gt_inside", b">a\nAC>GT\nG>\n" + fa(b"b", b"TT"), 300),
         ("crlf", four.replace(b"\n", b"\r\n"), 300), ("folded_crlf", folded.replace(b"\n", b"\r\n"), 300),
         ("odd_bytes", fa(b"lc", b"acgtACGTnNacgt") + fa(b"iupac", b"RYKMSWBDHVN-.ACGT*", 5) + fa(b"allN", b"N" * 40) + fa(b"mix", b"ACGTNACGTNACGTNACGTNACGTNACGTNACG", 7), 300),
         ("long_header", fa(b"h" * 150, b"ACGT") + fa(b"x" * 98 + b" tail", b"GGCC") + fa(b"y" * 99, b"TT"), 300),
         ("name_ends", b"".join(fa(b"nm" + e + b"more", b"ACGTAC") for e in (b" ", b"\t", b"/", b"\x7f", b"\x80", b"\x00", b"\x1f")), 300),
         ("nul_in_seq", fa(b"a", b"ACGT") + b">n\nAC\0GT\nGG\n" + fa(b"b", b"TT"), 300), ("nul_first_in_line", fa(b"a", b"ACGT") + b">n\n\0CGT\n" + fa(b"b", b"TT"), 300),
         ("other_header", fa(b"a", b"ACGT") + b"Xbad\nACGT\n" + fa(b"b", b"TT"), 300),
         ("lengths", b"".join(fa(b"len%d" % n, acgt[:n], w) for n, w in ((1, 0), (15, 0), (16, 60), (17, 0), (31, 60), (32, 0), (33, 16), (5000, 60))), 5000),
         ("too_long", fa(b"a", b"ACGT") + fa(b"big", b"ACGT" * 13, 20) + fa(b"c", b"GG"), 50), ("just_fits", fa(b"fit", b"ACGT" * 12 + b"AC", 20), 50),
         ("too_long_one_line", fa(b"a", b"ACGT") + fa(b"big", b"ACGT" * 13) + fa(b"c", b"GG"), 50), ("just_fits_one_line", fa(b"fit", b"ACGT" * 12 + b"AC"), 50)]
    for n in (1022, 1023, 1024, 2047):  # lines round the .gz readers' 1023-byte cut, header and sequence
        v.append(("seq_line_%d" % n, fa(b"a", b"ACGT") + b">s\n" + acgt[:n - 1] + b"\n" + fa(b"b", b"TT"), 2100))
        v.append(("header_line_%d" % n, fa(b"a", b"ACGT") + b">" + b"h" * (n - 2) + b"\nACGT\n" + fa(b"b", b"TT"), 2100))
    assert all(len(t) < 65536 for _, t, _ in v)
    return v + [("seeded", seeded_text(), 300)]


@pytest.fixture(scope="module")
def vectors():
    return make_vectors()


@pytest.fixture(scope="module")
def fasta_check(tmp_path_factory):
    from mapcaller_amd import api
    out = str(tmp_path_factory.mktemp("fasta_check") / "libfasta_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", CHECK_SRC, "-o", out], check=True, stderr=subprocess.PIPE, timeout=600)
    L = C.CDLL(out)
    L.fasta_check_parse.restype = C.c_int
    L.fasta_check_parse.argtypes = [C.POINTER(api.FastqIn), C.POINTER(api.FastqOut), C.POINTER(api.FastqInfo), C.c_int]
    return {rule: tb._AsCheck(lambda a, b, c, rule=rule: L.fasta_check_parse(a, b, c, rule)) for rule in (PLAIN, GZ)}


# ---- CPU: the rules compiled for the host -------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [PLAIN, GZ])
def test_host_build_equals_the_restatement_on_every_vector(fasta_check, packer, vectors, rule):
    for tag, texts, max_len in tf.cases_of(vectors):
        big = max(len(t) for t in texts) // 3 + 1
        for final, max_records in ((True, big), (False, big), (True, 2), (False, 1), (True, 0)):
            exp = restate(packer, rule, texts, max_records, max_len, final)
            tf.assert_result((rule, tag, final, max_records), *tf.run_call("check", fasta_check[rule], texts, max_records, max_len, final, exp), exp)
    stops = {RESTATE[rule](t, 1 << 20, m, True)[2] for _, t, m in vectors}
    assert stops == {END, EMPTY, TOO_LONG}  # (the vectors reach every way a text can end)


def text_3k():
    """3 KB of records folded to several widths, with empty lines and a '>' inside a line"""
    rng = random.Random(3)
    t, k = b"", 0
    while len(t) < 3000:
        seq = bytes(rng.choice(b"ACGTN") for _ in range(rng.randint(1, 150)))
        t += fa(b"c%d x" % k, seq, rng.choice([0, 60, 60, 7])) + (b"\n" if k % 5 == 4 else b"") + (b"A>C\n" if k % 7 == 6 else b"")
        k += 1
    return t[:3072]


def test_host_build_on_a_text_cut_at_every_byte(fasta_check, packer):
    """final = 0 on text_3k[:cut] for every cut: records, stop and consumed — the cut or a header line's start, from which the text's remaining records follow"""
    text = text_3k()
    whole, _, _, _ = restate_plain_text(text, 1 << 10, 300, True)
    head_starts = {s for s, _ in getlines(text) if s == 0 or text[s] == 0x3E}
    for cut in range(len(text) + 1):
        part = text[:cut]
        exp = restate(packer, PLAIN, [part], 1 << 10, 300, False)
        tf.assert_result(("cut", cut), *tf.run_call("check", fasta_check[PLAIN], [part], 1 << 10, 300, False, exp, groups=("recs", "bases")), exp)
        consumed, n = exp["info"]["consumed"][0], exp["info"]["n_records"][0]
        assert consumed == cut or consumed in head_starts, cut
        if cut % 16 == 0 or cut > len(text) - 64:  # the rest from there on: the whole text's remaining records
            rest, _, _, _ = restate_plain_text(text[consumed:], 1 << 10, 300, True)
            assert [(a + consumed, b, c + consumed, d, 0, 0) for a, b, c, d, _, _ in rest] == whole[n:], cut


def test_the_restatement_equals_the_products_own_reader(packer, vectors, tmp_path, monkeypatch):
    """The vectors as plain files (multi-line FASTA) and as ordinary .gz files (the GZ rule) through mcx_reader.h's Parser (tests/hostemu/parser_check.cpp):
    names and bases.  The reader takes a file whose first byte is not '@' for FASTA; under the GZ rule a header must begin with '>' or '@'."""
    d = os.path.join(ROOT, "tests", "hostemu")
    subprocess.run(["make", "-C", d, "libparser_check.so"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(d, "libparser_check.so"))
    L.parser_dump.restype = C.c_longlong
    L.parser_dump.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    monkeypatch.setenv("MCX_SERIAL_PARSER", "1")
    compared = {PLAIN: 0, GZ: 0}
    for name, text, _ in vectors:
        if name in ("too_long", "empty") or text.startswith(b"@"):
            continue
        for rule in (PLAIN, GZ):
            recs, seqs, _, _ = RESTATE[rule](text, 1 << 20, 100000, True)
            want = b"".join(text[c[0]:c[0] + c[1]] + b"\t" + s + b"\t\n" for c, s in zip(recs, seqs))
            path, out = str(tmp_path / (name + (".fa.gz" if rule == GZ else ".fa"))), str(tmp_path / (name + ".txt"))
            if rule == GZ:
                tb.write_ordinary_gz(path, text)
            else:
                open(path, "wb").write(text)
            err = C.create_string_buffer(512)
            n = L.parser_dump(path.encode(), 100000, 3, out.encode(), err, 512)
            assert n == len(recs), (rule, name, n, len(recs), err.value)
            assert open(out, "rb").read() == want, (rule, name)
            compared[rule] += 1
    assert min(compared.values()) >= 30


def seeded_small_texts(n=1000, seed=13):
    rng = random.Random(seed)
    alphabet = b"\n" * 14 + b">" * 8 + b"ACGT" * 6 + b"N" * 3 + b" /\x00" * 2 + bytes(range(0x80, 0x100, 9)) + b"acgt\r\t@"
    return [bytes(rng.choice(alphabet) for _ in range(rng.randint(0, rng.choice([8, 64, 512, 4096])))) for _ in range(n)]


def test_host_build_under_the_sanitizers(tmp_path, vectors):
    """The stand-alone program (its own main; nothing of it is loaded into Python) built with -fsanitize=address,undefined: the vectors alone and in pairs, and
    1 000 seeded texts of at most 4 KB over an alphabet weighted towards newline, '>', bases, N, blank, '/', NUL and bytes >= 0x80 — each under both rules with
    final 0 and 1 and max_records 0 .. 3 and unbounded, into heap buffers of exactly the contract's sizes.  It must exit 0 and report nothing."""
    exe = str(tmp_path / "fasta_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-DFASTA_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    CHECK_SRC, "-o", exe], check=True, stderr=subprocess.PIPE, timeout=600)
    small = seeded_small_texts()
    assert len(small) == 1000 and max(map(len, small)) <= 4096
    cases = [(texts, max_len) for _, texts, max_len in tf.cases_of(vectors)] + [([t], 64) for t in small] + [([a, b], 64) for a, b in zip(small[::50], small[1::50])]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for texts, max_len in cases:
            b = [len(t) for t in texts] + [0] * (2 - len(texts))
            f.write(struct.pack("<IIQQ", len(texts), max_len, b[0], b[1]) + b"".join(texts))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout == "" and r.stderr == "", (r.stdout[-1500:], r.stderr[-3000:])


# ---- GPU: the kernels -------------------------------------------------------------------------------------------------
api = tf.api


def fasta_parser(api, rule, **kw):
    p = api.FastqParser(0, **kw)
    p.set_format(api.READS_FASTA)
    p.set_rule(rule)
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [PLAIN, GZ])
def test_parse_dev_equals_the_restatement_on_every_vector(api, packer, vectors, rule):
    with fasta_parser(api, rule) as p:
        for tag, texts, max_len in tf.cases_of(vectors):
            big = max(len(t) for t in texts) // 3 + 1
            for final, max_records in ((True, big), (False, big)) + (((True, 2), (False, 1), (True, 0)) if len(texts) == 1 else ()):
                exp = restate(packer, rule, texts, max_records, max_len, final)
                tf.assert_result((rule, tag, final, max_records), *tf.run_call("dev", p, texts, max_records, max_len, final, exp), exp)
        assert p.last_ms() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [PLAIN, GZ])
def test_parse_dev_at_every_alignment_of_the_text(api, packer, vectors, rule):
    head = (vectors[-1][1] if rule == PLAIN else seeded_text(6, 8192, (0,)))[:8192]  # (the GZ rule takes one sequence line: single-line records for it)
    exp = restate(packer, rule, [head], 4096, 300, True)
    assert exp["info"]["n_reads"] > 20
    with fasta_parser(api, rule) as p:
        for shift in range(16):
            tf.assert_result(("shift", shift), *tf.run_call("dev", p, [head], 4096, 300, True, exp, shift=shift), exp)


@pytest.mark.gpu
def test_a_text_fed_in_pieces(api, packer, vectors):
    """final = 0, 97 records a call, every piece from the last `consumed` on, the ends of the pieces at three arbitrary offsets; the last piece with final = 1"""
    import torch
    text = vectors[-1][1]
    whole = restate(packer, PLAIN, [text], 1 << 20, 300, True)
    d = torch.device("cuda", 0)
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(d)
    ends = [61003, 61007 + 70001, 150000 + 17, len(text)]
    pos, recs, bases, calls = 0, [], [], 0
    with fasta_parser(api, PLAIN) as p:
        for i, end in enumerate(ends):
            last = i == len(ends) - 1
            while True:
                d_recs = torch.zeros(97 * 24, dtype=torch.uint8, device=d)
                d_bases = torch.zeros(end - pos + 32, dtype=torch.uint8, device=d)
                d_off = torch.zeros(98, dtype=torch.int32, device=d)
                rc, info = p.parse_dev([d_text[pos:end]], 97, 300, final=last, recs=[d_recs], bases=d_bases, off=d_off)
                calls += 1
                assert rc == 0 and calls < 200
                n = info["n_records"][0]
                piece = restate(packer, PLAIN, [text[pos:end]], 97, 300, last)
                assert info == piece["info"]
                r = d_recs.cpu().numpy().view(np.uint32).reshape(-1, 6)[:n].astype(np.int64)
                r[:, [0, 2]] += pos
                recs.append(r)
                bases.append(d_bases.cpu().numpy()[:info["n_bases"]].tobytes())
                pos += info["consumed"][0]
                if n < 97:
                    assert info["stop"][0] == (END if last else MORE)
                    break
    assert pos == len(text)
    assert np.array_equal(np.concatenate(recs), whole["recs"][0].astype(np.int64)) and b"".join(bases) == whole["bases"].tobytes()


@pytest.mark.gpu
def test_refusals_leave_the_outputs_alone(api, packer, vectors):
    by = dict((n, t) for n, t, _ in vectors)
    texts = [by["odd_bytes"], by["folded_60"]]
    exp = restate(packer, PLAIN, texts, 100, 300, True)
    assert exp["info"]["n_odd"] > 0 and exp["info"]["n_name_bytes"] > 0
    with fasta_parser(api, PLAIN) as p:
        for short, group in (("bases_cap", "bases"), ("names_cap", "names"), ("odd_cap", "rows")):
            rc, info, out, written = tf.run_call("dev", p, texts, 100, 300, True, exp, short=short)
            assert rc == api.ERR_CAPACITY and "cap" in api.lib().mcx_last_error().decode()
            tf.assert_result(short, rc, info, out, written, exp, untouched=tf.GROUPS[group])
        tf.assert_result("afterwards", *tf.run_call("dev", p, texts, 100, 300, True, exp), exp)
        for bad in (2, -1, 7):
            with pytest.raises(api.McxError):
                p.set_format(bad)
            assert api.lib().mcx_fastq_parser_set_format(p._h, bad) == api.ERR_ARG
        tf.assert_result("after a refused format", *tf.run_call("dev", p, texts, 100, 300, True, exp), exp)  # (the format stays)
        # back to FASTQ: the FASTQ results on a FASTQ vector
        p.set_format(api.READS_FASTQ)
        fq = tf.make_vectors()[0][1]
        want = tf.restate(packer, [fq], 100, 300, True)
        tf.assert_result("fastq again", *tf.run_call("dev", p, [fq], 100, 300, True, want), want)


@pytest.mark.gpu
def test_the_host_buffer_form_and_a_parser_that_grows(api, packer, vectors):
    text = vectors[-1][1]
    exp = restate(packer, PLAIN, [text, text[:100000]], 1 << 20, 300, True)
    with fasta_parser(api, PLAIN, max_text_bytes=4096, max_records=16) as p:
        assert p.grown() == 0
        tf.assert_result("host", *tf.run_call("host", p, [text, text[:100000]], 1 << 20, 300, True, exp), exp)
        g = p.grown()
        assert g >= 1
        tf.assert_result("host again", *tf.run_call("host", p, [text, text[:100000]], 1 << 20, 300, True, exp), exp)
        assert p.grown() == g  # (once: the second call finds room)
        p.set_rule(GZ)
        gz = restate(packer, GZ, [text[:50000]], 1 << 20, 300, True)
        tf.assert_result("host, GZ rule", *tf.run_call("host", p, [text[:50000]], 1 << 20, 300, True, gz), gz)


# ---- GPU: the file front end ------------------------------------------------------------------------------------------------
def _mapper(api, prefix, alg="ksw2", full_sa=True, **kw):
    ix = api.Index(prefix, device=0, full_sa=full_sa)
    return ix, api.Mapper(ix, alg=alg, max_batch_reads=1000, **kw)


@pytest.mark.gpu
def test_front_end_multi_line_fasta_with_device_parse(api, io_golden, tmp_path):
    g = io_golden
    ix, mp = _mapper(api, g["prefix"], alg="nw", full_sa=False)
    out = str(tmp_path / "ml.sam")
    st = mp.map_files(g["ml.fa"], None, out, device_parse=True)
    assert mp.last_route() == (api.ROUTE_PARSE, 0)
    assert st["reads"] == 400
    nd, ex = sam_diff(g["ref.ml.sam"], out, mask_se_reverse_qual=True)
    assert nd == 0, ex
    mp.close(); ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ["ksw2", "nw"])
def test_front_end_single_end_fasta_with_device_parse(api, golden, tmp_path, alg):
    """`se` (several batches of 1 000): the golden SAM with the host formatter and with device_sam, and -m against the golden extras"""
    import test_multi as tm
    g = golden["se"]
    n = open(g["r1"], "rb").read().count(b">")
    for sam_on_device in (False, True):
        ix, mp = _mapper(api, g["prefix"], alg=alg)
        out = str(tmp_path / f"se_{alg}_{int(sam_on_device)}.sam")
        st = mp.map_files(g["r1"], None, out, device_parse=True, device_sam=sam_on_device)
        assert mp.last_route() == (api.ROUTE_PARSE | (api.ROUTE_SAM if sam_on_device else 0), 0)
        assert st["reads"] == n
        nd, ex = sam_diff(g["sam"][alg], out)
        assert nd == 0, (sam_on_device, ex)
        mp.close(); ix.close()
    ix, mp = _mapper(api, g["prefix"], alg=alg, multi=True)
    out = str(tmp_path / f"se_{alg}_m.sam")
    mp.map_files(g["r1"], None, out, device_parse=True)
    assert mp.last_route() == (api.ROUTE_PARSE, 0)
    tm.compare("se", alg, out)
    mp.close(); ix.close()


def as_fasta(fq_text, width=0):
    l = fq_text.split(b"\n")
    return b"".join(fa(h[1:], s, width) for h, s in zip(l[0::4], l[1::4]) if h)


@pytest.mark.gpu
def test_front_end_paired_fasta_with_device_parse(api, golden, tmp_path):
    """The toy pairs as two FASTA files (file 2 folded to 60 columns): read count and SAM bytes of the host route, and the toy golden SAM but for QUAL"""
    g = golden["toy"]
    f1, f2 = str(tmp_path / "t1.fa"), str(tmp_path / "t2.fa")
    open(f1, "wb").write(as_fasta(open(g["r1"], "rb").read())); open(f2, "wb").write(as_fasta(open(g["r2"], "rb").read(), 60))
    res = []
    for switch in (False, True):
        ix, mp = _mapper(api, g["prefix"])
        out = str(tmp_path / f"pair_{int(switch)}.sam")
        st = mp.map_files(f1, f2, out, device_parse=switch)
        assert mp.last_route() == ((api.ROUTE_PARSE, api.ROUTE_PARSE) if switch else (0, 0))
        res.append((st["reads"], open(out, "rb").read()))
        mp.close(); ix.close()
    assert res[0] == res[1] and res[0][0] == 3000
    assert tb.drop_qual(res[1][1]) == tb.drop_qual(open(g["sam"]["ksw2"], "rb").read())


@pytest.mark.gpu
def test_fallbacks_take_the_old_routes(api, golden, io_golden, tmp_path):
    """device_parse on where the new route does not apply: -p, a sharded run, ordinary .gz FASTA, a FASTA and a FASTQ file — today's routes and bytes"""
    g = golden["se"]
    text = open(g["r1"], "rb").read()
    ix, mp = _mapper(api, g["prefix"])

    def run(f1, f2, out, **kw):
        mp.reset()
        try:
            st = mp.map_files(f1, f2, out, **kw)
            return st["reads"], "", open(out, "rb").read(), mp.last_route()
        except api.McxError as e:
            return None, str(e), None, mp.last_route()
    # -p
    host = run(g["r1"], None, str(tmp_path / "p0.sam"), interleaved=True)
    got = run(g["r1"], None, str(tmp_path / "p1.sam"), interleaved=True, device_parse=True)
    assert got == host and got[3] == (0, 0) and got[0] == text.count(b">")
    # ordinary .gz
    gz = str(tmp_path / "se.fa.gz")
    tb.write_ordinary_gz(gz, text)
    host = run(gz, None, str(tmp_path / "g0.sam"))
    got = run(gz, None, str(tmp_path / "g1.sam"), device_parse=True, device_inflate=True)
    assert got == host and got[3] == (0, 0) and got[0] == text.count(b">")
    # a FASTA and a FASTQ file
    fq = str(tmp_path / "se.fq")
    open(fq, "wb").write(tb.se_as_fastq(g["r1"]))
    host = run(g["r1"], fq, str(tmp_path / "d0.sam"))
    got = run(g["r1"], fq, str(tmp_path / "d1.sam"), device_parse=True)
    assert got[:3] == host[:3] and "with different format" in got[1]
    mp.close(); ix.close()
    # a sharded run: two shards on one device, each a mapper of its own on a thread, one output file
    want = open(g["sam"]["ksw2"], "rb").read()
    for switch in (False, True):
        links = (api.Exchange * 2)()
        assert api.lib().mcx_exchange_local(2, links) == 0
        out = str(tmp_path / f"sh_{int(switch)}.sam")
        res = [None, None]

        def shard(r):
            ix, mp = _mapper(api, g["prefix"])
            try:
                st = mp.map_files(g["r1"], None, out, shard=(r, 2), exchange=links[r], device_parse=switch)
                res[r] = (st["reads"], mp.last_route())
            except api.McxError as e:
                res[r] = (str(e), None)
            mp.close(); ix.close()
        ts = [threading.Thread(target=shard, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        api.lib().mcx_exchange_local_free(links)
        assert all(r is not None and r[1] == (0, 0) for r in res), res
        assert open(out, "rb").read() == want, switch


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["se", "ml"])
def test_front_end_resident_route_on_bgzf_fasta(api, golden, io_golden, tmp_path, monkeypatch, name):
    """Members of 3 000 bytes and launches of 64 KB of text: launch and carry boundaries inside records.  All four route bits; `se` gives its golden SAM;
    ml.fa as .gz is read under the GZ rule — the first sequence line only, and the line behind it is no header, so the input ends: the host route's SAM on the
    same file (not ref.ml.sam)."""
    monkeypatch.setenv("MCX_RESIDENT_LAUNCH_BYTES", "65536")
    g = golden["se"] if name == "se" else io_golden
    src = g["r1"] if name == "se" else g["ml.fa"]
    path = str(tmp_path / (name + ".fa.gz"))
    tb.write_bgzf(path, open(src, "rb").read(), 3000)
    fr = tb.Front(api, g, max_batch_reads=1000)
    got = fr.run([path], str(tmp_path / "res.sam"), True)
    host = fr.run([path], str(tmp_path / "host.sam"), False)
    fr.close()
    assert got[3] == (ALL_FOUR, 0) and host[3] == (0, 0), (got[3], host[3])
    assert got[1] == "" and got[:3] == host[:3] and got[0] > 0
    if name == "se":
        assert got[0] == open(src, "rb").read().count(b">")
        nd, ex = sam_diff(g["sam"]["ksw2"], str(tmp_path / "res.sam"))
        assert nd == 0, ex


@pytest.mark.gpu
def test_front_end_resident_route_on_fasta_without_sam_gives_the_reference_vcf(api, golden, tmp_path, monkeypatch):
    monkeypatch.setenv("MCX_RESIDENT_LAUNCH_BYTES", "65536")
    g = golden["se"]
    tag = "default"
    o = VcfOpts(VCF_RUNS[tag][1]).struct
    path = str(tmp_path / "se.fa.gz")
    tb.write_bgzf(path, open(g["r1"], "rb").read(), 3000)
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg=vcf_alg("se", tag), max_batch_reads=1000)
    planes = api.planes_alloc(ix.genome_size, "cuda")
    mp.profile_attach(planes.data_ptr(), max_dup=o.max_dup, max_clip=o.max_clip)
    st = mp.map_files(path, None, None, device_inflate=True, device_parse=True, device_sam=True)
    assert mp.last_route() == (7, 0)
    mp.profile_finalize(planes.data_ptr())
    out = str(tmp_path / "o.vcf")
    switches = {k: getattr(o, k) for k in ("ploidy", "min_allele_depth", "min_cnv", "min_gap", "fragment_size", "filter", "gvcf", "monomorphic", "somatic")}
    ix.call_variants(planes.data_ptr(), mp.profile_sparse(), st["pairs"], st["pair_dist_sum"], st["pair_len_sum"], out, sample_id=o.sample_id.decode(), ref_name="ref", cmdline="test", **switches)
    got, want = vcf_body(out), vcf_body(g["vcf"][tag])
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:3]
    mp.close(); ix.close()


@pytest.mark.gpu
def test_ends_of_input_equal_the_host_route(api, golden, tmp_path, monkeypatch):
    """Each case through the host route and through each new route on the same files — plain FASTA with device_parse, BGZF FASTA on the resident route:
    return code, error text, read count; SAM bytes where the run succeeds, and where it fails what each left in its file is whole batches from the start, so
    the shorter is the beginning of the longer."""
    monkeypatch.setenv("MCX_RESIDENT_LAUNCH_BYTES", "65536")
    g = golden["toy"]
    a1, a2 = as_fasta(open(g["r1"], "rb").read()), as_fasta(open(g["r2"], "rb").read())
    l1, l2 = a1.split(b"\n"), a2.split(b"\n")

    def swap(lines, i, new):
        return b"\n".join(lines[:i] + [new] + lines[i + 1:])
    cases = {"empty_record": (swap(l1, 2 * 500 + 1, b""), a2), "too_long": (swap(l1, 2 * 700 + 1, b"ACGT" * 64 + b"A"), a2), "too_long_2": (a1, swap(l2, 2 * 700 + 1, b"ACGT" * 64 + b"A")),
             "file_2_shorter": (a1, b"\n".join(l2[:-21]) + b"\n"), "file_2_longer": (b"\n".join(l1[:-21]) + b"\n", a2),
             "header_x": (swap(l1, 2 * 500, b"X" + l1[2 * 500][1:]), a2), "no_final_newline": (a1[:-1], a2[:-1])}
    fr = tb.Front(api, g, max_batch_reads=1000)
    seen = {}
    for tag, (a, b) in cases.items():
        for kind in ("plain", "bgzf"):
            files = [str(tmp_path / f"{tag}_{k}.fa{'.gz' if kind == 'bgzf' else ''}") for k in (1, 2)]
            for f, t in zip(files, (a, b)):
                if kind == "bgzf":
                    tb.write_bgzf(f, t, 3000)
                else:
                    open(f, "wb").write(t)
            res, written = [], []
            for switch in (False, True):
                out = str(tmp_path / f"{tag}_{kind}_{int(switch)}.sam")
                fr.mp.reset()
                try:
                    st = fr.mp.map_files(files[0], files[1], out, device_parse=switch, device_inflate=switch and kind == "bgzf", device_sam=kind == "bgzf")
                    res.append((st["reads"], "", open(out, "rb").read()))
                except api.McxError as e:
                    res.append((None, str(e), None))
                sam_bit = api.ROUTE_SAM if kind == "bgzf" else 0
                want_route = ((ALL_FOUR, ALL_FOUR) if kind == "bgzf" else (api.ROUTE_PARSE, api.ROUTE_PARSE)) if switch else (sam_bit, sam_bit)
                assert fr.mp.last_route() == want_route, (tag, kind, switch, fr.mp.last_route())
                written.append(open(out, "rb").read() if os.path.exists(out) else b"")
            assert res[0] == res[1], (tag, kind, res[0][:2], res[1][:2])
            if res[0][1]:
                short, long_ = sorted(written, key=len)
                assert long_.startswith(short), (tag, kind)
            seen[tag, kind] = res[0]
    fr.close()
    for kind in ("plain", "bgzf"):
        assert seen["empty_record", kind][:2] == (1000, "") and seen["file_2_longer", kind][:2] == (2 * (1500 - 10), "") and seen["no_final_newline", kind][:2] == (3000, "")
        assert "holds fewer reads than" in seen["file_2_shorter", kind][1]
        for tag in ("too_long", "too_long_2"):
            assert "is longer than max_read_len" in seen[tag, kind][1] and "read " in seen[tag, kind][1]
    # a header that begins with 'X': under the GZ rule it ends the input; under the plain rule it is sequence — read 499 grows to 150 + 9 + 150 bases, more
    # than the context's max_read_len of 256
    assert seen["header_x", "bgzf"][:2] == (1000, "") and "read sim_0499 is longer than max_read_len" in seen["header_x", "plain"][1]


@pytest.mark.gpu
def test_cli_gpu_parse_on_fasta(golden, io_golden, tmp_path):
    env = dict(os.environ, MCX_TIMING="1")
    out = str(tmp_path / "ml.sam")
    r = subprocess.run([EXE, "-i", io_golden["prefix"], "-f", io_golden["ml.fa"], "-alg", "nw", "-sam", out, "-no_vcf", "-gpu_parse"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "file 1 2, file 2 0" in r.stderr and "parse + pack" in r.stderr, r.stderr[-2000:]
    nd, ex = sam_diff(io_golden["ref.ml.sam"], out, mask_se_reverse_qual=True)
    assert nd == 0, ex
    g = golden["se"]
    path, out = str(tmp_path / "se.fa.gz"), str(tmp_path / "se.sam")
    tb.write_bgzf(path, open(g["r1"], "rb").read(), 3000)
    r = subprocess.run([EXE, "-i", g["prefix"], "-f", path, "-alg", "ksw2", "-sam", out, "-no_vcf", "-gpu_inflate", "-gpu_parse", "-gpu_sam"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "file 1 15, file 2 0" in r.stderr and "the resident route" in r.stderr, r.stderr[-2000:]
    nd, ex = sam_diff(g["sam"]["ksw2"], out)
    assert nd == 0, ex
