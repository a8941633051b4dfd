"""bgzip reads kept in HBM from inflate to SAM: the .gz readers' line rule in the device parser (mcx_fastq_parser_set_rule, MCX_FASTQ_RULE_GZ), a batch that
enters its slot from HBM (mcx_stream_submit_dev), the file front end's resident route (-gpu_inflate -gpu_parse on BGZF FASTQ) and mcx_files_route.

Expectations for the GZ rule come from a restatement in Python of the rule as include/mcx.h words it (pieces of at most 1023 bytes, C lengths, records of
four pieces), with nothing taken from the code under test; the header rule, the vectors' driver and the output layout are tests/test_fastq_device.py's.
CPU: the surface; the rule compiled for the host (mapcaller_amd/csrc/mcx_fastq.h through tests/hostemu/fastq_gz_check.cpp) against the restatement; the
restatement against the product's own sequential reader (tests/hostemu/parser_check.cpp, which golden set `io` pins to the compiled reference); the host
build as a stand-alone program under -fsanitize=address,undefined.  GPU: the kernels under the GZ rule on every vector, alignment and block boundary; a text
fed in two parts at every byte; mcx_stream_submit_dev against mcx_stream_submit_packed; the device chain inflate -> parse -> submit -> map -> SAM text on
tensors; the front end on the golden sets, its fallbacks, its ends of input against the host route, and the command line.

The golden single-end set `se` is FASTA, which neither rule of the parser covers: where a case asks for `se` on the resident route its reads go as FASTQ
(qualities 'I'), and the SAM is held against the host route's on the same file and against the golden SAM with the QUAL column set aside."""
import ctypes as C
import gzip
import inspect
import os
import random
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import test_fastq_device as tf
from conftest import ROOT, VCF_RUNS, VcfOpts, sam_diff, vcf_alg, vcf_body

NEW = ("mcx_fastq_parser_set_rule", "mcx_stream_submit_dev", "mcx_files_route")
CHECK_SRC = os.path.join(ROOT, "tests", "hostemu", "fastq_gz_check.cpp")
EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
MORE, END, EMPTY, TOO_LONG = 0, 1, 2, 3
PIECE = 1023
ALL_FOUR = 1 | 2 | 4 | 8


# ---- CPU: the surface ---------------------------------------------------------------------------------------
def test_the_new_calls_are_declared_bound_and_exported():
    from mapcaller_amd import api, run
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for s in NEW:
        assert s in api.SYMBOLS and re.search(r"\b%s\s*\(" % s, header), s
    for name, value in (("MCX_FASTQ_RULE_PLAIN", 0), ("MCX_FASTQ_RULE_GZ", 1), ("MCX_ROUTE_INFLATE", 1), ("MCX_ROUTE_PARSE", 2), ("MCX_ROUTE_ROWS", 4), ("MCX_ROUTE_SAM", 8)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
    assert (api.FASTQ_RULE_PLAIN, api.FASTQ_RULE_GZ) == (0, 1) and (api.ROUTE_INFLATE, api.ROUTE_PARSE, api.ROUTE_ROWS, api.ROUTE_SAM) == (1, 2, 4, 8)
    m = re.search(r"enum\s+mcx_fastq_stop\s*\{([^}]*)\}", header)
    assert m and len(m.group(1).split(",")) == 4
    assert "MCX_RESIDENT_LAUNCH_BYTES" in header
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in NEW:
            assert f" {s}\n" in nm, s
        L = api.lib()
        assert L.mcx_stream_submit_dev.argtypes == L.mcx_stream_submit_packed.argtypes and L.mcx_files_route.restype is C.c_int
        assert L.mcx_gz_inflate.restype is C.c_int64 and L.mcx_gz_inflate.argtypes[2] is C.c_uint64
    assert (C.sizeof(api.FileOpts), C.sizeof(api.FastqIn), C.sizeof(api.FastqOut), C.sizeof(api.FastqInfo)) == (48, 48, 112, 64)
    for name in ("last_route", "submit_dev"):
        assert callable(getattr(api.Mapper, name))
    assert callable(api.FastqParser.set_rule)
    assert "device_parse" in inspect.signature(api.Mapper.map_files).parameters
    a = run.parse(["-i", "x", "-f", "a.fq.gz", "-gpu_inflate", "-gpu_parse", "-gpu_sam"])
    assert a.gpu_inflate and a.gpu_parse and a.gpu_sam


# ---- the GZ rule, restated from its wording ------------------------------------------------------------------------
def gz_pieces(text):
    """[(start, end)]: the piece at s is the bytes up to and including the first newline within text[s, s + 1023); without one, those 1023 bytes when
    there are as many, else the rest of the text"""
    out, s = [], 0
    while s < len(text):
        w = text[s:s + PIECE]
        i = w.find(b"\n")
        e = s + i + 1 if i >= 0 else (s + PIECE if len(w) == PIECE else len(text))
        out.append((s, e))
        s = e
    return out


def c_len(piece):
    i = piece.find(b"\0")
    return len(piece) if i < 0 else i


def restate_gz_text(text, max_records, max_read_len, final):
    """(records as tuples of REC_DTYPE's fields, stop, consumed) of one text under the GZ rule"""
    P = gz_pieces(text)

    def complete(q):
        return q < len(P) and (text[P[q][1] - 1:P[q][1]] == b"\n" or P[q][1] - P[q][0] == PIECE)
    recs, stop = [], MORE
    while len(recs) < max_records:
        k = len(recs)
        if not final and not all(complete(4 * k + j) for j in range(4)):
            break
        if 4 * k >= len(P):
            stop = END
            break
        hs, he = P[4 * k]
        cl = c_len(text[hs:he])
        if cl == 0 or text[hs] not in b"@>":
            stop = EMPTY
            break
        p1, name_len = tf.header_span(text[hs:hs + cl])
        if 4 * k + 1 >= len(P):
            stop = EMPTY
            break
        ss, se = P[4 * k + 1]
        cl = c_len(text[ss:se])
        rlen = cl - 1 if cl else 0
        if rlen == 0:
            stop = EMPTY
            break
        if rlen > max_read_len:
            stop = TOO_LONG
            break
        has_q = 4 * k + 3 < len(P)
        ql = c_len(text[P[4 * k + 3][0]:P[4 * k + 3][1]]) if has_q else 0
        recs.append((hs + p1, name_len, ss, rlen, P[4 * k + 3][0] if has_q else 0, min(ql, rlen)))
    k = len(recs)
    return recs, stop, P[4 * k][0] if 4 * k < len(P) else len(text)


def restate_gz(lib, texts, max_records, max_read_len, final, row_words=None):
    """tf.restate with the GZ rule's records: every output of the call as a dict of numpy arrays (and "info")"""
    saved = tf.restate_text
    tf.restate_text = restate_gz_text
    try:
        return tf.restate(lib, texts, max_records, max_read_len, final, row_words)
    finally:
        tf.restate_text = saved


def test_the_restatement_on_pieces_worked_by_hand():
    assert gz_pieces(b"ab\ncd") == [(0, 3), (3, 5)]
    for n, want in ((1022, 1), (1023, 1), (1024, 2), (2046, 2), (2047, 3), (3070, 4)):  # a line of L bytes with its newline: ceil(L / 1023) pieces
        assert len(gz_pieces(b"x" * (n - 1) + b"\n")) == want == -(-n // PIECE), n
    assert gz_pieces(b"x" * 1024) == [(0, 1023), (1023, 1024)] and gz_pieces(b"x" * 1023) == [(0, 1023)]
    t = b"@r1 x\nAC\0T\n+\nIIIIII\n@r2\nGG"
    recs, stop, consumed = restate_gz_text(t, 10, 8, True)
    assert recs == [(1, 2, 6, 1, 13, 1), (21, 2, 24, 1, 0, 0)] and stop == END and consumed == len(t)  # (the NUL cuts the sequence piece: C length 2, rlen 1)
    assert restate_gz_text(t, 10, 8, False)[1:] == (MORE, 20)
    long_seq = b"@a\n" + b"A" * 1500 + b"\n+\n" + b"I" * 1500 + b"\n"  # the 1023-byte cut makes other records of it
    recs, stop, _ = restate_gz_text(long_seq, 10, 5000, True)
    assert recs == [(1, 1, 3, 1022, 1504, 2)] and stop == EMPTY  # (the line's second piece is skipped as the third, "+" is the fourth; then a header piece that is none)


# ---- the vectors --------------------------------------------------------------------------------------------
def long_line_record(pos, n):
    """a record whose line `pos` (0 header, 1 sequence, 2 '+', 3 quality) is n bytes long with its newline"""
    lines = [b"@name", b"ACGTACGT", b"+", b"IIIIIIII"]
    fill = {0: b"h", 1: b"A", 2: b"p", 3: b"I"}[pos]
    lines[pos] = (lines[pos][:1] + fill * n)[:n - 1]
    return b"".join(l + b"\n" for l in lines)


def text_3k():
    """3 KB with a 1024-byte line in it: the sequence line of the second record — two pieces, the sequence and the one that is skipped, so that the record has no
    '+' line of its own and the records behind it stay in step"""
    t = tf.rec(b"first/1", b"ACGTACGTAC") + b"@long x\n" + b"ACGT" * 255 + b"ACG\n" + b"I" * 30 + b"\n"
    k = 0
    while len(t) < 3000:
        t += tf.rec(b"r%d" % k, b"ACGTTGCA" * 9 + b"N")
        k += 1
    return t[:3072]


def make_gz_vectors():
    """[(name, text, max_read_len)], each at most 8 KB"""
    ok = tf.rec(b"ok/1", b"ACGTACGTAC")
    v = []
    for n in (1022, 1023, 1024, 2046, 2047, 3070):
        for pos in range(4):
            v.append(("line%d_%d" % (pos, n), ok + long_line_record(pos, n) + tf.rec(b"after", b"GGCC") + ok, 1100))
    for n in (1022, 1023, 1024):
        v.append(("last_seq_%d" % n, ok + b"@b\n" + b"C" * n, 1100))
        v.append(("last_qual_%d" % n, ok + b"@b\nACGT\n+\n" + b"I" * n, 1100))
    v += [("nul_header_first", ok + b"\0bad\nACGT\n+\nIIII\n" + ok, 300), ("nul_header_middle", ok + b"@na\0me rest\nACGT\n+\nIIII\n" + ok, 300),
          ("nul_seq_first", ok + b"@a\n\0CGT\n+\nIIII\n" + ok, 300), ("nul_seq_middle", ok + b"@a\nACG\0TTT\n+\nIIIIIII\n" + ok, 300),
          ("nul_qual_first", ok + b"@a\nACGT\n+\n\0III\n" + ok, 300), ("nul_qual_middle", ok + b"@a\nACGT\n+\nII\0I\n" + ok, 300),
          ("nul_text_first", b"\0" + ok, 300), ("other_header", ok + b"Xbad\nACGT\n+\nIIII\n" + ok, 300), ("fasta_header", ok + b">fa\nACGT\n+\nIIII\n" + ok, 300),
          ("crlf", (ok * 3).replace(b"\n", b"\r\n"), 300), ("empty", b"", 300), ("newline", b"\n", 300), ("at_only", b"@", 300),
          ("empty_seq", ok + b"@b\n\n+\n\n" + ok, 300), ("too_long", ok + tf.rec(b"big", b"ACGT" * 13) + ok, 50), ("no_newline_at_all", b"@" + b"A" * 5000, 1100),
          ("odd_bytes", tf.rec(b"lc", b"acgtACGTnNacgt") + tf.rec(b"iupac", b"RYKMSWBDHVN-.ACGT*"), 300), ("text_3k", text_3k(), 1100)]
    assert all(len(t) <= 8192 for _, t, _ in v)
    return v


@pytest.fixture(scope="module")
def vectors():
    return make_gz_vectors()


@pytest.fixture(scope="module")
def packer():
    from mapcaller_amd import api
    if not os.path.exists(api.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "mapcaller_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    L = api.lib()
    L.mcx_pack_row.restype = C.c_uint32
    L.mcx_pack_row.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    return L


class _AsCheck:
    """tf.run_call's "check" form calls handle.fastq_check_parse"""

    def __init__(self, fn):
        self.fastq_check_parse = fn


@pytest.fixture(scope="module")
def gz_check(tmp_path_factory):
    from mapcaller_amd import api
    out = str(tmp_path_factory.mktemp("fastq_gz_check") / "libfastq_gz_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", CHECK_SRC, "-o", out], check=True, stderr=subprocess.PIPE, timeout=600)
    L = C.CDLL(out)
    L.fastq_gz_check_parse.restype = C.c_int
    L.fastq_gz_check_parse.argtypes = [C.POINTER(api.FastqIn), C.POINTER(api.FastqOut), C.POINTER(api.FastqInfo)]
    return _AsCheck(L.fastq_gz_check_parse)


# ---- CPU: the rule compiled for the host ---------------------------------------------------------------------------
def test_host_build_equals_the_restatement_on_every_vector(gz_check, packer, vectors):
    for tag, texts, max_len in tf.cases_of(vectors):
        big = max(len(t) for t in texts) // 3 + 1
        for final, max_records in ((True, big), (False, big), (True, 2), (False, 1), (True, 0)):
            exp = restate_gz(packer, texts, max_records, max_len, final)
            tf.assert_result((tag, final, max_records), *tf.run_call("check", gz_check, texts, max_records, max_len, final, exp), exp)
    stops = {restate_gz_text(t, 1 << 20, m, True)[1] for _, t, m in vectors}
    assert stops == {END, EMPTY, TOO_LONG}


def test_host_build_on_a_record_cut_at_every_byte(gz_check, packer):
    """final = 0 on text_3k[:cut] for every cut: records, stop and consumed — a piece start, from which the same pieces follow"""
    text = text_3k()
    whole = gz_pieces(text)
    for cut in range(len(text) + 1):
        part = text[:cut]
        exp = restate_gz(packer, [part], 1 << 10, 1100, False)
        tf.assert_result(("cut", cut), *tf.run_call("check", gz_check, [part], 1 << 10, 1100, False, exp, groups=("recs", "bases")), exp)
        consumed = exp["info"]["consumed"][0]
        assert consumed == cut or consumed in {s for s, _ in whole}, cut


def write_ordinary_gz(path, data):
    with open(path, "wb") as f:
        f.write(gzip.compress(data, 6))


def test_the_restatement_equals_the_products_own_reader(packer, vectors, tmp_path):
    """The vectors as ordinary .gz files through mcx_reader.h's Parser (tests/hostemu/parser_check.cpp): names, bases and qualities.  The reader decides FASTQ
    or FASTA by the text's first byte, so the vectors that do not begin with '@' are left to the other tests."""
    d = os.path.join(ROOT, "tests", "hostemu")
    subprocess.run(["make", "-C", d, "libparser_check.so"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(d, "libparser_check.so"))
    L.parser_dump.restype = C.c_longlong
    L.parser_dump.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    compared = 0
    for name, text, max_len in vectors:
        if not text.startswith(b"@") or name == "too_long":
            continue
        recs, _, _ = restate_gz_text(text, 1 << 20, 100000, True)
        want = b"".join(text[c[0]:c[0] + c[1]] + b"\t" + text[c[2]:c[2] + c[3]] + b"\t" + text[c[4]:c[4] + c[5]] + b"\n" for c in recs)
        path, out = str(tmp_path / (name + ".fq.gz")), str(tmp_path / (name + ".txt"))
        write_ordinary_gz(path, text)
        err = C.create_string_buffer(512)
        n = L.parser_dump(path.encode(), 100000, 3, out.encode(), err, 512)
        assert n == len(recs), (name, n, len(recs), err.value)
        assert open(out, "rb").read() == want, name
        compared += 1
    assert compared >= 40


def seeded_gz_texts(n=1000, seed=23):
    """texts of at most 4 KB that mix the vectors' cases: lines around the 1023-byte cut in any position, NULs, headers that are none, CR, a missing last newline"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        t = b""
        for _ in range(rng.randint(0, 5)):
            lines = [b"@" + bytes(rng.choice(b"nm /\t@>\x7f") for _ in range(rng.randint(0, 12))), bytes(rng.choice(b"ACGTNacgt") for _ in range(rng.randint(0, 40))), b"+",
                     bytes(rng.randint(33, 73) for _ in range(rng.randint(0, 40)))]
            if rng.random() < 0.3:
                k = rng.randrange(4)
                lines[k] = lines[k][:1] + bytes([lines[k][0] if lines[k] else 65]) * rng.choice([1020, 1021, 1022, 1023, 1024, 2045, 2046])
            if rng.random() < 0.2:
                k = rng.randrange(4)
                at = rng.randint(0, len(lines[k]))
                lines[k] = lines[k][:at] + b"\0" + lines[k][at:]
            if rng.random() < 0.1:
                lines[0] = b"X" + lines[0][1:]
            nl = b"\r\n" if rng.random() < 0.1 else b"\n"
            t += nl.join(lines) + nl
        if t and rng.random() < 0.3:
            t = t[:rng.randint(0, len(t))]
        out.append(t[:4096])
    return out


def test_host_build_under_the_sanitizers(tmp_path, vectors):
    """The stand-alone program (its own main; nothing of it is loaded into Python) built with -fsanitize=address,undefined: the vectors alone and in pairs and 1 000
    seeded texts that mix their cases, each with final 0 and 1 and max_records 0 .. 3 and unbounded, into heap buffers of exactly the contract's sizes — the piece
    table among them.  It must exit 0 and report nothing."""
    exe = str(tmp_path / "fastq_gz_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-DFASTQ_GZ_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    CHECK_SRC, "-o", exe], check=True, stderr=subprocess.PIPE, timeout=600)
    small = seeded_gz_texts()
    assert len(small) == 1000 and max(map(len, small)) <= 4096 and sum(b"\0" in t for t in small) > 50 and sum(len(t) > 1023 for t in small) > 100
    cases = [(texts, max_len) for _, texts, max_len in tf.cases_of(vectors)] + [([t], 1100) for t in small] + [([a, b], 64) for a, b in zip(small[::50], small[1::50])]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for texts, max_len in cases:
            b = [len(t) for t in texts] + [0] * (2 - len(texts))
            f.write(struct.pack("<IIQQ", len(texts), max_len, b[0], b[1]) + b"".join(texts))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout == "" and r.stderr == "", (r.stdout[-1500:], r.stderr[-3000:])


def test_host_build_equals_the_restatement_on_the_seeded_texts(gz_check, packer):
    for i, t in enumerate(seeded_gz_texts(300)):
        for final in (True, False):
            exp = restate_gz(packer, [t], 1 << 10, 1100, final)
            tf.assert_result(("seeded", i, final), *tf.run_call("check", gz_check, [t], 1 << 10, 1100, final, exp), exp)


# ---- GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


@pytest.mark.gpu
def test_parse_dev_under_the_gz_rule_equals_the_restatement_on_every_vector(api, packer, vectors):
    with api.FastqParser(0) as p:
        p.set_rule(api.FASTQ_RULE_GZ)
        for tag, texts, max_len in tf.cases_of(vectors):
            big = max(len(t) for t in texts) // 3 + 1
            for final, max_records in ((True, big), (False, big)) + (((True, 2), (False, 1), (True, 0)) if len(texts) == 1 else ()):
                exp = restate_gz(packer, texts, max_records, max_len, final)
                tf.assert_result((tag, final, max_records), *tf.run_call("dev", p, texts, max_records, max_len, final, exp), exp)
        # back to the plain rule: the plain results again
        p.set_rule(api.FASTQ_RULE_PLAIN)
        for name, text, max_len in vectors[::5]:
            exp = tf.restate(packer, [text], len(text) // 3 + 1, max_len, True)
            tf.assert_result((name, "plain"), *tf.run_call("dev", p, [text], len(text) // 3 + 1, max_len, True, exp), exp)
        assert api.lib().mcx_fastq_parser_set_rule(p._h, 2) == api.ERR_ARG


def boundary_text(target):
    """a text whose long sequence line has a piece boundary (the start of its second piece) at byte `target`"""
    prefix = b"".join(tf.rec(b"p%d" % i, b"ACGTTGCAAC" * 9) for i in range(14))
    k = target - PIECE - len(prefix) - 2
    assert 0 < k < 900
    t = prefix + b"@" + b"n" * k + b"\n" + b"ACGT" * 500 + b"\n+\n" + b"I" * 2000 + b"\n" + tf.rec(b"tail", b"GGCCA")
    assert (target - PIECE, target) in gz_pieces(t) and len(t) <= 8192
    return t


@pytest.mark.gpu
def test_parse_dev_under_the_gz_rule_at_every_alignment_and_block_boundary(api, packer, vectors):
    # records the 1023-byte cut leaves in step: a sequence line of 1024 bytes gives the sequence piece and, of its newline, the piece that is skipped — such a
    # record has no '+' line of its own
    text = b"".join(tf.rec(b"r%d/1" % i, b"ACGTNACGTT" * (i + 1)) + b"@long%d x\n" % i + b"ACGT" * 255 + b"ACG\n" + b"I" * (40 + i) + b"\n" for i in range(12))
    exp = restate_gz(packer, [text], 4096, 1100, True)
    assert exp["info"]["n_reads"] == 24 and exp["info"]["longest"] == 1022 and exp["info"]["stop"][0] == END and len(text) > 3 * 4096
    with api.FastqParser(0) as p:
        p.set_rule(api.FASTQ_RULE_GZ)
        for shift in range(16):
            tf.assert_result(("shift", shift), *tf.run_call("dev", p, [text], 4096, 1100, True, exp, shift=shift), exp)
        # a piece boundary on each side of a 4 KB counting block's edge and of a 16-byte load's (the blocks start at the text's first byte when shift is 0)
        for target in (4095, 4096, 4097, 4111, 4112, 4113, 4079, 4080, 4081):
            t = boundary_text(target)
            for final in (True, False):
                e = restate_gz(packer, [t], 4096, 1100, final)
                tf.assert_result(("boundary", target, final), *tf.run_call("dev", p, [t], 4096, 1100, final, e), e)


@pytest.mark.gpu
def test_a_text_fed_in_two_parts_at_every_byte_under_the_gz_rule(api, packer):
    """text_3k[:cut] with final = 0, then the remainder from `consumed` with final = 1: the records put together are the whole text's"""
    import torch
    text = text_3k()
    whole = np.array(restate_gz_text(text, 1 << 10, 1100, True)[0], dtype=np.int64)
    d = torch.device("cuda", 0)
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(d)
    cap = len(text) // 3 + 1
    d_recs = torch.zeros(cap * 24, dtype=torch.uint8, device=d)

    def parse(p, lo, hi, final):
        rc, info = p.parse_dev([d_text[lo:hi]], cap, 1100, final=final, recs=[d_recs], text_bytes=[hi - lo])
        assert rc == 0
        r = d_recs.cpu().numpy().view(np.uint32).reshape(-1, 6)[:info["n_records"][0]].astype(np.int64)
        r[:, [0, 2]] += lo
        r[:, 4] += np.where(r[:, 4] > 0, lo, 0)
        return r, info
    with api.FastqParser(0) as p:
        p.set_rule(api.FASTQ_RULE_GZ)
        for cut in range(1, len(text) + 1):
            first, info = parse(p, 0, cut, False)
            want = restate_gz_text(text[:cut], cap, 1100, False)
            assert (info["n_records"][0], info["stop"][0], info["consumed"][0]) == (len(want[0]), want[1], want[2]), cut
            rest, info2 = parse(p, info["consumed"][0], len(text), True)
            assert np.array_equal(np.concatenate([first, rest]), whole), cut


def _reads_with_odd_bytes(path, n, fasta):
    """the first n reads of a golden read file as (lines of bytes), some bytes turned to N and to lower case"""
    lines = open(path, "rb").read().split(b"\n")
    seqs = [bytearray(s) for s in (lines[1::2] if fasta else lines[1::4])[:n]]
    rng = random.Random(5)
    for s in seqs[::7]:
        s[rng.randrange(len(s))] = ord("N")
    for s in seqs[3::11]:
        i = rng.randrange(len(s))
        s[i] = ord(chr(s[i]).lower())
    return [bytes(s) for s in seqs]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy", "se"])
def test_submit_dev_equals_submit_packed(api, golden, name):
    """The same rows, lengths and odd bytes from page-locked host memory and from a tensor: records and CIGAR words of mcx_stream_map32; a length longer than
    its row is refused after the fact both ways, with every read unmapped; a batch without odd bytes; bytes_in counts the host batches only."""
    import torch
    g = golden[name]
    paired = g["r2"] is not None
    if paired:
        a, b = _reads_with_odd_bytes(g["r1"], 500, False), _reads_with_odd_bytes(g["r2"], 500, False)
        seqs = [s for pair in zip(a, b) for s in pair]
    else:
        seqs = _reads_with_odd_bytes(g["r1"], 1000, True)
    n = len(seqs)
    assert n == 1000
    width = max(map(len, seqs))
    mat = np.zeros((n, width), dtype=np.uint8)
    for r, s in enumerate(seqs):
        mat[r, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    lens = torch.tensor([len(s) for s in seqs], dtype=torch.int32)
    words, tl, odd, n_odd, rw = api.pack_reads(torch.from_numpy(mat), lens)
    assert n_odd > 100
    clean = np.where(np.isin(mat, np.frombuffer(b"ACGT", dtype=np.uint8)) | (mat == 0), mat, ord("A")).astype(np.uint8)
    words0, tl0, odd0, n_odd0, _ = api.pack_reads(torch.from_numpy(clean), lens)
    assert n_odd0 == 0
    L = api.lib()
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=n)
    outs = [(torch.zeros(n * 32, dtype=torch.uint8).pin_memory(), torch.zeros(api.cigar_pool_words(n), dtype=torch.int32).pin_memory()) for _ in range(2)]
    h2d = C.c_uint64()

    def run(w, l, o, k, dev, out):
        mp.reset()
        if dev:
            keep = (w.cuda(), l.cuda(), o.cuda())  # (alive until the batch has been handed out: the call below returns after that)
            torch.cuda.synchronize()
            rc = L.mcx_stream_submit_dev(mp._h, keep[0].data_ptr(), rw, keep[1].data_ptr(), n, keep[2].data_ptr() if k else None, k)
        else:
            rc = L.mcx_stream_submit_packed(mp._h, w.data_ptr(), rw, l.data_ptr(), n, o.data_ptr() if k else None, k)
        assert rc == 0, L.mcx_last_error()
        rc = L.mcx_stream_map32(mp._h, int(paired), mp.avg, out[0].data_ptr(), out[1].data_ptr(), C.byref(mp.stats))
        msg = L.mcx_last_error() if rc else b""
        if rc == 0:
            assert L.mcx_stream_collect(mp._h, C.byref(h2d), None) == 0, L.mcx_last_error()
        return rc, msg, out[0].numpy().copy(), out[1].numpy().copy()

    def same(x, y, tag):
        assert x[0] == y[0] == 0, (tag, x[0], y[0], x[1], y[1])
        ra, rb = np.frombuffer(x[2].tobytes(), dtype=api.ALN32_DTYPE), np.frombuffer(y[2].tobytes(), dtype=api.ALN32_DTYPE)
        for f in api.ALN32_DTYPE.names:  # (where a read's operations lie in the pool is the run's own: its cursor is an atomic one)
            assert f == "cigar_off" or np.array_equal(ra[f], rb[f]), (tag, f)
        assert (ra["flag"] & 4 == 0).sum() > n // 2, tag  # (most reads map: the comparison is not of two empty results)
        for r in range(n):
            la, lb = int(ra["cigar_off"][r]), int(rb["cigar_off"][r])
            assert np.array_equal(x[3][la:la + int(ra["n_cigar"][r])], y[3][lb:lb + int(rb["n_cigar"][r])]), (tag, r)
    before = h2d.value
    host = run(words, tl, odd, n_odd, False, outs[0])
    counted = h2d.value - before
    assert counted == n * rw * 4 + n * 4 + n_odd * 8
    dev = run(words, tl, odd, n_odd, True, outs[1])
    assert h2d.value - before == counted  # (a batch that entered from HBM crossed no boundary)
    same(host, dev, "odd bytes")
    same(run(words0, tl0, odd0, 0, False, outs[0]), run(words0, tl0, odd0, 0, True, outs[1]), "n_odd = 0")
    bad = tl.clone()
    bad[7] = rw * 16 + 1
    bad = bad.pin_memory()
    for dev_side in (False, True):
        for o in outs[0]:
            o.fill_(0x5A)
        rc, msg, _, _ = run(words, bad, odd, n_odd, dev_side, outs[0])
        assert rc == api.ERR_ARG and b"longer than its row" in msg, (dev_side, rc, msg)
    # ... and mapped as empty reads both ways: the two-half form hands the records over with the refusal
    L.mcx_stream_next.restype = C.c_int
    L.mcx_stream_next.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    got = []
    for dev_side in (False, True):
        mp.reset()
        keep = (words.cuda(), bad.cuda(), odd.cuda())
        torch.cuda.synchronize()
        if dev_side:
            assert L.mcx_stream_submit_dev(mp._h, keep[0].data_ptr(), rw, keep[1].data_ptr(), n, keep[2].data_ptr(), n_odd) == 0, L.mcx_last_error()
        else:
            assert L.mcx_stream_submit_packed(mp._h, words.data_ptr(), rw, bad.data_ptr(), n, odd.data_ptr(), n_odd) == 0, L.mcx_last_error()
        db, do, da, dc, nr = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
        assert L.mcx_stream_next(mp._h, C.byref(db), C.byref(do), C.byref(nr), C.byref(da), C.byref(dc)) == 0, L.mcx_last_error()
        mp.map_batch_dev(db.value, do.value, nr.value, paired, da.value, dc.value)
        assert L.mcx_stream_mapped32(mp._h, outs[0][0].data_ptr(), outs[0][1].data_ptr()) == 0, L.mcx_last_error()
        assert L.mcx_stream_collect(mp._h, None, None) == api.ERR_ARG and b"empty reads" in L.mcx_last_error()
        recs = np.frombuffer(outs[0][0].numpy().tobytes(), dtype=api.ALN32_DTYPE)
        assert (recs["flag"] & 4 != 0).all(), dev_side  # every read unmapped
        got.append(recs["flag"].copy())
    assert np.array_equal(got[0], got[1])
    mp.close(); ix.close()


def write_bgzf(path, data, block=0xff00, level=6, empty_after=None):
    """bgzip's container: independent gzip members, each with its own size in a 'BC' extra field (tests/test_inflate_device.py's); empty_after: (member index,
    how many) empty members put behind that member"""
    empty = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    with open(path, "wb") as f:
        for k, i in enumerate(range(0, len(data), block)):
            chunk = data[i:i + block]
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            comp = c.compress(chunk) + c.flush()
            f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
            if empty_after and k == empty_after[0]:
                f.write(empty * empty_after[1])
        f.write(empty)


def bgzf_members(raw):
    """MEMBER records of a BGZF file's bytes (src_off into raw, texts back to back) and the text's length"""
    from mapcaller_amd import api
    out, o, at = [], 0, 0
    while o < len(raw):
        xlen = raw[10 + o] | (raw[11 + o] << 8)
        size = (raw[o + 16] | (raw[o + 17] << 8)) + 1
        isize = int.from_bytes(raw[o + size - 4:o + size], "little")
        if isize:
            out.append((o + 12 + xlen, at, size - 12 - xlen - 8, isize, int.from_bytes(raw[o + size - 8:o + size - 4], "little"), 0))
        at += isize
        o += size
    return np.array(out, dtype=api.MEMBER_DTYPE), at


@pytest.mark.gpu
def test_device_chain_inflate_parse_submit_map_format(api, golden, tmp_path):
    """The `var` pairs as BGZF with members of 3 000 bytes, copied to HBM once as compressed bytes: mcx_inflate_dev -> mcx_fastq_parse_dev under the GZ rule, each
    file's text in three parts with text[consumed ..) carried in front of the next -> mcx_stream_submit_dev -> mcx_stream_map32 -> mcx_sam_format_dev, all on
    tensors.  The text equals the golden SAM."""
    import torch
    g = golden["var"]
    d = torch.device("cuda", 0)
    L = api.lib()
    L.mcx_stream_next.restype = C.c_int
    L.mcx_stream_next.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    texts = []
    with api.Inflater(0, max_members=1 << 16) as inf:
        for k in ("r1", "r2"):
            path = str(tmp_path / (k + ".fq.gz"))
            write_bgzf(path, open(g[k], "rb").read(), 3000)
            raw = open(path, "rb").read()
            members, total = bgzf_members(raw)
            d_src = torch.from_numpy(np.frombuffer(raw + bytes(8), dtype=np.uint8).copy()).to(d)
            d_mem = torch.from_numpy(members.view(np.uint8).copy()).to(d)
            d_dst = torch.zeros(total, dtype=torch.uint8, device=d)
            d_status = torch.zeros(len(members), dtype=torch.int32, device=d)
            assert inf.inflate_dev(d_src, d_mem, len(members), d_dst, d_status) == 0
            texts.append(d_dst)
    n_pairs = open(g["r1"], "rb").read().count(b"\n") // 4
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=2 * n_pairs)
    rw = 16
    sam = api.sam_header(ix)
    cuts = [[0, len(t) // 3 + 11, 2 * len(t) // 3 + 5, len(t)] for t in texts]
    carry = [texts[0][:0], texts[1][:0]]
    total_reads = 0
    with api.FastqParser(0) as p:
        p.set_rule(api.FASTQ_RULE_GZ)
        for part in range(3):
            last = part == 2
            cur = [torch.cat([carry[f], texts[f][cuts[f][part]:cuts[f][part + 1]]]) for f in range(2)]  # (the carry in front of the next text: device to device)
            rc, info = p.parse_dev(cur, 1 << 20, 256, final=last)
            assert rc == 0
            take = min(info["n_records"]) if last else min(info["n_records"]) // 100 * 100  # (paired batches go to the mapper in whole 200-read chunks)
            cap = sum(t.numel() for t in cur) + 32
            o = {"bases": torch.zeros(cap, dtype=torch.uint8, device=d), "qual": torch.zeros(cap, dtype=torch.uint8, device=d), "off": torch.zeros(2 * take + 1, dtype=torch.int32, device=d),
                 "names": torch.zeros(cap, dtype=torch.uint8, device=d), "name_off": torch.zeros(2 * take + 1, dtype=torch.int32, device=d),
                 "rows": torch.zeros((2 * take, rw), dtype=torch.int32, device=d), "len": torch.zeros(2 * take, dtype=torch.int32, device=d), "odd": torch.zeros(cap, dtype=torch.int64, device=d)}
            rc, info = p.parse_dev(cur, take, 256, final=last, **o)  # (once more with max_records set to what the batch takes: the file that is ahead keeps its surplus)
            assert rc == 0 and info["n_reads"] == 2 * take
            carry = [cur[f][info["consumed"][f]:].clone() for f in range(2)]
            if take == 0:
                continue
            m = 2 * take
            mp.submit_dev(o["rows"].data_ptr(), rw, o["len"].data_ptr(), m, o["odd"].data_ptr(), info["n_odd"])
            db, do, da, dc, nr = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
            assert L.mcx_stream_next(mp._h, C.byref(db), C.byref(do), C.byref(nr), C.byref(da), C.byref(dc)) == 0, L.mcx_last_error()
            assert nr.value == m
            mp.map_batch_dev(db.value, do.value, m, True, da.value, dc.value)
            di = api.SamIn()
            di.bases, di.off, di.qual, di.names, di.name_off = db.value, do.value, o["qual"].data_ptr(), o["names"].data_ptr(), o["name_off"].data_ptr()
            di.aln, di.cigar, di.n_reads, di.paired = da.value, dc.value, m, 1
            size = C.c_uint64()
            assert L.mcx_sam_format_dev(mp._h, C.byref(di), None, 0, None, C.byref(size)) == api.ERR_CAPACITY
            d_sam = torch.zeros(size.value, dtype=torch.uint8, device=d)
            assert L.mcx_sam_format_dev(mp._h, C.byref(di), d_sam.data_ptr(), size.value, None, C.byref(size)) == 0, L.mcx_last_error()
            sam += d_sam.cpu().numpy().tobytes()
            out32 = torch.zeros(m * 32, dtype=torch.uint8).pin_memory()
            pool = torch.zeros(api.cigar_pool_words(m), dtype=torch.int32).pin_memory()
            assert L.mcx_stream_mapped32(mp._h, out32.data_ptr(), pool.data_ptr()) == 0, L.mcx_last_error()
            assert L.mcx_stream_collect(mp._h, None, None) == 0, L.mcx_last_error()
            total_reads += m
    mp.close(); ix.close()
    assert total_reads == 2 * n_pairs and carry[0].numel() == 0 and carry[1].numel() == 0
    out = tmp_path / "chain.sam"
    out.write_bytes(sam)
    nd, ex = sam_diff(g["sam"]["ksw2"], str(out))
    assert nd == 0, ex


# ---- the file front end ------------------------------------------------------------------------------------------------
def se_as_fastq(path):
    fa = open(path, "rb").read().split(b"\n")
    return b"".join(b"@" + h[1:] + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for h, s in zip(fa[0::2], fa[1::2]) if h)


def read_texts(g, name):
    if name == "se":
        return [se_as_fastq(g["r1"])]
    return [open(g["r1"], "rb").read(), open(g["r2"], "rb").read()]


class Front:
    """an index and a mapper of small batches for a golden set, for several runs"""

    def __init__(self, api, g, max_batch_reads=1 << 13, **kw):
        self.api = api
        self.ix = api.Index(g["prefix"], device=0, full_sa=True)
        self.mp = api.Mapper(self.ix, alg="ksw2", max_batch_reads=max_batch_reads, **kw)

    def run(self, files, out, resident, device_sam=None, **kw):
        """(reads or None, error text, SAM bytes or None, route)"""
        self.mp.reset()
        files = list(files) + [None] * (2 - len(files))
        try:
            st = self.mp.map_files(files[0], files[1], out, device_inflate=resident, device_parse=resident, device_sam=resident if device_sam is None else device_sam, **kw)
            return st["reads"], "", open(out, "rb").read() if out else None, self.mp.last_route()
        except self.api.McxError as e:
            return None, str(e), None, self.mp.last_route()

    def close(self):
        self.mp.close(); self.ix.close()


def drop_qual(sam_bytes):
    lines = sam_bytes.decode("latin-1").split("\n")
    return "\n".join("\t".join(f[:10] + ["*"] + f[11:]) if len(f := l.split("\t")) > 10 and not l.startswith("@") else l for l in lines)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy", "var", "se"])
def test_front_end_resident_route_equals_reference(api, golden, tmp_path, monkeypatch, name):
    """Members of 0xff00 and of 3 000 bytes, launches of 64 KB of text, batches of 8 192 reads: many launches, carries and batches in each file.  The SAM is the
    golden SAM (se: see the module's note), and every file's route has all four bits."""
    monkeypatch.setenv("MCX_RESIDENT_LAUNCH_BYTES", "65536")
    g = golden[name]
    texts = read_texts(g, name)
    fr = Front(api, g)
    n_reads = sum(t.count(b"\n") // 4 for t in texts)
    for block in (0xff00, 3000):
        files = []
        for k, t in enumerate(texts):
            files.append(str(tmp_path / f"{name}_{block}_{k + 1}.fq.gz"))
            write_bgzf(files[-1], t, block)
        out = str(tmp_path / f"{name}_{block}.sam")
        reads, err, sam, route = fr.run(files, out, True)
        assert err == "" and reads == n_reads, (block, err, reads)
        assert route == (ALL_FOUR, ALL_FOUR if len(texts) == 2 else 0), (block, route)
        if name == "se":
            host = fr.run(files, str(tmp_path / "host.sam"), False)
            assert host[3] == (0, 0) and sam == host[2], block
            assert drop_qual(sam) == drop_qual(open(g["sam"]["ksw2"], "rb").read()), block
        else:
            nd, ex = sam_diff(g["sam"]["ksw2"], out)
            assert nd == 0, (block, ex)
    fr.close()


@pytest.mark.gpu
def test_front_end_resident_route_without_sam_gives_the_reference_vcf(api, golden, tmp_path, monkeypatch):
    """No SAM file and -vcf on `var`: rows from HBM, the profile on the device — the golden VCF, and a route of inflate | parse | rows"""
    monkeypatch.setenv("MCX_RESIDENT_LAUNCH_BYTES", "65536")
    g = golden["var"]
    tag = "default"
    o = VcfOpts(VCF_RUNS[tag][1]).struct
    files = [str(tmp_path / "v1.fq.gz"), str(tmp_path / "v2.fq.gz")]
    write_bgzf(files[0], open(g["r1"], "rb").read(), 3000); write_bgzf(files[1], open(g["r2"], "rb").read(), 0xff00)
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg=vcf_alg("var", tag), max_batch_reads=1 << 13)
    planes = api.planes_alloc(ix.genome_size, "cuda")
    mp.profile_attach(planes.data_ptr(), max_dup=o.max_dup, max_clip=o.max_clip)
    st = mp.map_files(files[0], files[1], None, device_inflate=True, device_parse=True, device_sam=True)
    assert mp.last_route() == (7, 7)
    mp.profile_finalize(planes.data_ptr())
    out = str(tmp_path / "o.vcf")
    switches = {k: getattr(o, k) for k in ("ploidy", "min_allele_depth", "min_cnv", "min_gap", "fragment_size", "filter", "gvcf", "monomorphic", "somatic")}
    ix.call_variants(planes.data_ptr(), mp.profile_sparse(), st["pairs"], st["pair_dist_sum"], st["pair_len_sum"], out, sample_id=o.sample_id.decode(), ref_name="ref", cmdline="test", **switches)
    got, want = vcf_body(out), vcf_body(g["vcf"][tag])
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:3]
    mp.close(); ix.close()


@pytest.mark.gpu
def test_fallbacks_take_the_old_routes(api, golden, io_golden, tmp_path):
    """Both switches on where the resident route does not apply: the host formatter, an interleaved file, an ordinary .gz — no MCX_ROUTE_PARSE, today's SAM"""
    g = golden["toy"]
    texts = read_texts(g, "toy")
    files = [str(tmp_path / "t1.fq.gz"), str(tmp_path / "t2.fq.gz")]
    for f, t in zip(files, texts):
        write_bgzf(f, t, 3000)
    fr = Front(api, g)
    want = fr.run(files, str(tmp_path / "host.sam"), False)
    assert want[3] == (0, 0) and sam_diff(g["sam"]["ksw2"], str(tmp_path / "host.sam"))[0] == 0
    # the host formatter
    got = fr.run(files, str(tmp_path / "a.sam"), True, device_sam=False)
    assert got[3] == (api.ROUTE_INFLATE, api.ROUTE_INFLATE) and got[:3] == want[:3]
    # ordinary .gz
    plain = [str(tmp_path / "p1.fq.gz"), str(tmp_path / "p2.fq.gz")]
    for f, t in zip(plain, texts):
        write_ordinary_gz(f, t)
    got = fr.run(plain, str(tmp_path / "b.sam"), True)
    assert got[3] == (api.ROUTE_SAM, api.ROUTE_SAM) and got[:3] == want[:3]
    # one BGZF and one ordinary file
    got = fr.run([files[0], plain[1]], str(tmp_path / "c.sam"), True)
    assert got[3] == (api.ROUTE_INFLATE | api.ROUTE_SAM, api.ROUTE_SAM) and got[:3] == want[:3]
    # an interleaved file
    il = str(tmp_path / "il.fq.gz")
    write_bgzf(il, open(io_golden["il.fq"], "rb").read(), 3000)
    host = fr.run([il], str(tmp_path / "il_host.sam"), False, interleaved=True)
    got = fr.run([il], str(tmp_path / "il.sam"), True, interleaved=True)
    assert got[3] == (api.ROUTE_INFLATE | api.ROUTE_SAM, 0) and got[:3] == host[:3] and host[0] > 0
    fr.close()


@pytest.mark.gpu
def test_ends_of_input_equal_the_host_routes(api, golden, tmp_path, monkeypatch):
    """Each case through the host route (all switches off) and through the resident route on the same files: read count, SAM bytes and error text.  Where the
    run fails the file is not compared: how many batches were written before the failure reached the mapper depends on the threads' timing, with either route."""
    monkeypatch.setenv("MCX_RESIDENT_LAUNCH_BYTES", "65536")
    g = golden["toy"]
    r1, r2 = read_texts(g, "toy")
    l1, l2 = r1.split(b"\n"), r2.split(b"\n")

    def swap(lines, i, new):
        return b"\n".join(lines[:i] + [new] + lines[i + 1:])
    cases = {"file_2_shorter": (r1, b"\n".join(l2[:-41]) + b"\n"), "file_2_longer": (b"\n".join(l1[:-41]) + b"\n", r2),
             "header_x": (swap(l1, 4 * 500, b"X" + l1[4 * 500][1:]), r2), "empty_sequence": (swap(l1, 4 * 500 + 1, b""), r2),
             "too_long": (swap(l1, 4 * 700 + 1, b"ACGT" * 64 + b"A"), r2),
             "too_long_2": (r1, swap(l2, 4 * 700 + 1, b"ACGT" * 64 + b"A"))}
    fr = Front(api, g, max_batch_reads=1000)
    seen = {}

    golden_sam = open(g["sam"]["ksw2"], "rb").read()
    default_fr = fr

    def both(tag, files, fr=fr, resident_route=(ALL_FOUR, ALL_FOUR)):
        res, written = [], []
        for resident in (False, True):
            out = str(tmp_path / f"{tag}_{int(resident)}.sam")
            reads, err, sam, route = fr.run(files, out, resident)
            assert route == (resident_route if resident else (0, 0)), (tag, route)
            res.append((reads, err, sam))
            written.append(open(out, "rb").read() if os.path.exists(out) else b"")
        assert res[0] == res[1], (tag, res[0][:2], res[1][:2])
        if res[0][1]:
            # a run that failed: the batches before the stop were mapped and written by both routes — what each left in its file is whole batches from
            # the file's start, so the shorter is the beginning of the longer, and (where the context is the golden run's) both begin the golden SAM
            short, long_ = sorted(written, key=len)
            assert long_.startswith(short), tag
            if fr is default_fr:
                assert all(golden_sam.startswith(w) for w in written), tag
        seen[tag] = res[0] + (written,)
    for tag, (a, b) in cases.items():
        files = [str(tmp_path / f"{tag}_1.fq.gz"), str(tmp_path / f"{tag}_2.fq.gz")]
        write_bgzf(files[0], a, 3000); write_bgzf(files[1], b, 3000)
        both(tag, files)
    # damage to the container, in file 1
    whole_path = str(tmp_path / "whole_1.fq.gz")
    write_bgzf(whole_path, r1, 3000)
    whole = open(whole_path, "rb").read()
    cut = whole.find(b"\x1f\x8b\x08\x04", len(whole) // 2)
    f2 = str(tmp_path / "whole_2.fq.gz")
    write_bgzf(f2, r2, 3000)
    garbage, crc, empties = str(tmp_path / "garbage_1.fq.gz"), str(tmp_path / "crc_1.fq.gz"), str(tmp_path / "empties_1.fq.gz")
    open(garbage, "wb").write(whole[:cut] + b"not a member at all, forty bytes of it.." + whole[cut:])
    flipped = bytearray(whole); flipped[cut - 8] ^= 1
    open(crc, "wb").write(bytes(flipped))
    write_bgzf(empties, r1, 3000, empty_after=(40, 300))
    both("garbage", [garbage, f2]); both("empty_members", [empties, f2])
    # a wrong CRC takes its stretch of 8 MB of text with it.  In a file of one stretch nothing is left, the file has no first byte to be FASTQ by, and the
    # route leaves the run to the host reader (which finds the two files "with different format"); in a file of two stretches the first one counts
    both("flipped_crc", [crc, f2], resident_route=(0, 0))
    fr.close()
    big = Front(api, g)
    files = [str(tmp_path / "big_1.fq.gz"), str(tmp_path / "big_2.fq.gz")]
    write_bgzf(files[0], r1 * 20, 0xff00, 1); write_bgzf(files[1], r2 * 20, 0xff00, 1)
    assert len(r1) * 20 > (8 << 20) + 65536
    whole = bytearray(open(files[0], "rb").read())
    whole[len(whole) - 28 - 8] ^= 1  # (the CRC-32 of the last member with text, in the file's second stretch)
    open(files[0], "wb").write(bytes(whole))
    both("flipped_crc_late", files, fr=big)
    big.close()
    # Lines of 1 500 bytes, which the 1023-byte cut changes into other records.  A sequence line: its first piece is a read of 1 022 bases, longer than any
    # context takes (max_read_len <= 1000), so the run ends with that read's name.  A header line: its second piece is taken for a sequence of 476 bytes, the
    # sequence line is skipped, "+" is the quality piece, and the quality line is a header that is none — the input ends behind 601 records of file 1.
    long_fr = Front(api, g, max_batch_reads=1000, max_read_len=1000)
    for tag, a in (("line_1500", swap(swap(l1, 4 * 600 + 1, b"ACGT" * 375).split(b"\n"), 4 * 600 + 3, b"I" * 1500)), ("header_1500", swap(l1, 4 * 600, b"@" + b"h" * 1499))):
        files = [str(tmp_path / f"{tag}_1.fq.gz"), str(tmp_path / f"{tag}_2.fq.gz")]
        write_bgzf(files[0], a, 3000); write_bgzf(files[1], r2, 3000)
        both(tag, files, fr=long_fr)
    long_fr.close()
    n = r1.count(b"\n") // 4
    assert "holds fewer reads than" in seen["file_2_shorter"][1] and "with different format" in seen["flipped_crc"][1]
    assert seen["garbage"][1] == "" and 0 < seen["garbage"][0] < 2 * n
    assert seen["flipped_crc_late"][1] == "" and 2 * 8 * n < seen["flipped_crc_late"][0] < 2 * 20 * n
    assert seen["file_2_longer"][:2] == (2 * (n - 10), "") and seen["header_x"][:2] == (1000, "") and seen["empty_sequence"][:2] == (1000, "")
    assert seen["empty_members"][:2] == (2 * n, "") and seen["header_1500"][:2] == (1202, "") and "is longer than max_read_len" in seen["line_1500"][1]
    for tag in ("too_long", "too_long_2"):
        assert "is longer than max_read_len" in seen[tag][1] and "read " in seen[tag][1], seen[tag][1]
        assert all(w.startswith(b"@") for w in seen[tag][3]), tag  # (the header at least: the files were opened before the stop)


@pytest.mark.gpu
def test_cli_resident_route(golden, tmp_path):
    g = golden["toy"]
    f1, f2 = str(tmp_path / "t1.fq.gz"), str(tmp_path / "t2.fq.gz")
    write_bgzf(f1, open(g["r1"], "rb").read()); write_bgzf(f2, open(g["r2"], "rb").read(), 3000, 1)
    out = str(tmp_path / "cli.sam")
    env = dict(os.environ, MCX_TIMING="1")
    r = subprocess.run([EXE, "-i", g["prefix"], "-f", f1, "-f2", f2, "-alg", "ksw2", "-sam", out, "-no_vcf", "-gpu_inflate", "-gpu_parse", "-gpu_sam"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "file 1 15, file 2 15" in r.stderr, r.stderr[-2000:]
    nd, ex = sam_diff(g["sam"]["ksw2"], out)
    assert nd == 0, ex
