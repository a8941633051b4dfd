"""Plain FASTQ text parsed on the device: mcx_fastq_parser_create / _free, mcx_fastq_parse_dev / mcx_fastq_parse and the file front end's device_parse
(-gpu_parse).

Expectations come from a restatement, in Python, of the reader's rules for plain FASTQ (GetData.cpp:3-20, :32-55 as MappedFastq::parse and header_of of
mcx_reader.h hold them): a line is what getline gives, record k is lines 4k .. 4k+3, the last byte of the sequence line goes, min(quality line, read)
bytes of quality count; rows and odd bytes come from the library's host packer mcx_pack_row.  Nothing is expected from the code under test.
CPU: the ABI surface; the rules compiled for the host (mapcaller_amd/csrc/mcx_fastq.h through tests/hostemu/fastq_check.cpp) on every vector and on
the toy and var read files, with guard bytes round each output; the same file as a stand-alone program under -fsanitize=address,undefined on the
vectors and 1 000 seeded texts.  GPU: the vectors through the kernels alone and in pairs and at every alignment, a text fed in pieces, the refusals,
the host-buffer form, the device chain parse -> map -> SAM text on tensors, the file front end and the command line with the switch on."""
import ctypes as C
import inspect
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, sam_diff

NEW = ("mcx_fastq_parser_create", "mcx_fastq_parser_free", "mcx_fastq_parse_dev", "mcx_fastq_parse")
NEW_TYPES = ("mcx_fastq_rec", "mcx_fastq_in", "mcx_fastq_out")
CHECK_SRC = os.path.join(ROOT, "tests", "hostemu", "fastq_check.cpp")
EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
MORE, END, EMPTY, TOO_LONG = 0, 1, 2, 3
G = 64  # guard bytes on either side of every output


# ---- CPU: the surface ---------------------------------------------------------------------------------------
def test_the_fastq_calls_are_declared_bound_and_exported():
    from mapcaller_amd import api, run
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for s in NEW:
        assert s in api.SYMBOLS and re.search(r"\b%s\s*\(" % s, header), s
    for s in NEW_TYPES + ("mcx_fastq_info", "mcx_fastq_parser"):
        assert re.search(r"\}\s*%s\s*;|struct\s+%s\s+%s\s*;" % (s, s, s), header), s
    m = re.search(r"enum\s+mcx_fastq_stop\s*\{([^}]*)\}", header)
    assert m and [x.strip() for x in m.group(1).split(",")] == ["MCX_FASTQ_MORE = 0", "MCX_FASTQ_END = 1", "MCX_FASTQ_EMPTY = 2", "MCX_FASTQ_TOO_LONG = 3"]
    assert (api.FASTQ_MORE, api.FASTQ_END, api.FASTQ_EMPTY, api.FASTQ_TOO_LONG) == (MORE, END, EMPTY, TOO_LONG)
    assert "device_parse" in header and "reserved2" not in header
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in NEW:
            assert f" {s}\n" in nm, s
    F = api.FileOpts
    assert F.device_parse.offset == 36 and C.sizeof(F) == 48
    assert [(n, getattr(F, n).offset) for n, _ in F._fields_] == [("interleaved_pairs", 0), ("host_threads", 4), ("append_sam", 8), ("device_sam", 12), ("avg_state", 16),
                                                                  ("shard_rank", 24), ("shard_count", 28), ("device_inflate", 32), ("device_parse", 36), ("exchange", 40)]
    assert api.REC_DTYPE.itemsize == 24 and api.REC_DTYPE.names == ("name", "name_len", "seq", "rlen", "qual", "q_take")
    assert (C.sizeof(api.FastqIn), C.sizeof(api.FastqOut), C.sizeof(api.FastqInfo)) == (48, 112, 64)
    assert inspect.signature(api.Mapper.map_files).parameters["device_parse"].default is False
    for name in ("parse_dev", "parse", "last_ms", "close", "__enter__", "__exit__"):
        assert callable(getattr(api.FastqParser, name))
    assert run.parse(["-i", "x", "-f", "a.fq", "-gpu_parse"]).gpu_parse and not run.parse(["-i", "x", "-f", "a.fq"]).gpu_parse
    main = open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_main.cpp")).read()
    assert main.count("-gpu_parse") >= 2  # the switch and its line in usage


# ---- the rules, restated ------------------------------------------------------------------------------------
def header_span(line):
    """IdentifyHeaderBegPos / IdentifyHeaderEndPos (GetData.cpp:3-20) on a header line with its newline: (p1, name length)"""
    n = len(line)
    lim = min(n, 100)
    p1 = next((i for i in range(1, n) if line[i] not in b">@"), n - 1)
    p2 = next((i for i in range(1, lim) if line[i] <= 0x20 or line[i] == 0x2F or line[i] >= 0x7F), lim - 1)
    return p1, max(p2 - p1, 0)


def restate_text(text, max_records, max_read_len, final):
    """(records as tuples of REC_DTYPE's fields, stop, consumed) of one text"""
    starts, at = [], 0
    while at < len(text):
        starts.append(at)
        e = text.find(b"\n", at)
        at = len(text) if e < 0 else e + 1
    ends = starts[1:] + [len(text)]
    n_lines, n_nl = len(starts), text.count(b"\n")
    recs, stop = [], MORE
    while len(recs) < max_records:
        k = len(recs)
        if not final and n_nl < 4 * k + 4:
            break
        if 4 * k >= n_lines:
            stop = END
            break
        p1, name_len = header_span(text[starts[4 * k]:ends[4 * k]])
        if 4 * k + 1 >= n_lines:
            stop = EMPTY
            break
        rlen = ends[4 * k + 1] - starts[4 * k + 1] - 1
        if rlen == 0:
            stop = EMPTY
            break
        if rlen > max_read_len:
            stop = TOO_LONG
            break
        has_q = 4 * k + 3 < n_lines
        ql = ends[4 * k + 3] - starts[4 * k + 3] if has_q else 0
        recs.append((starts[4 * k] + p1, name_len, starts[4 * k + 1], rlen, starts[4 * k + 3] if has_q else 0, min(ql, rlen)))
    k = len(recs)
    return recs, stop, starts[4 * k] if 4 * k < n_lines else len(text)


def restate(lib, texts, max_records, max_read_len, final, row_words=None):
    """Every output of the call as a dict of numpy arrays (and "info"); rows and odd bytes through mcx_pack_row."""
    per = [restate_text(t, max_records, max_read_len, final) for t in texts]
    n_rec = [len(p[0]) for p in per]
    n = n_rec[0] if len(texts) == 1 else 2 * min(n_rec)
    reads = [(0, per[0][0][r]) if len(texts) == 1 else (r & 1, per[r & 1][0][r >> 1]) for r in range(n)]
    bases = b"".join(texts[t][c[2]:c[2] + c[3]] for t, c in reads)
    qual = b"".join(texts[t][c[4]:c[4] + c[5]] + bytes(c[3] - c[5]) for t, c in reads)
    names = b"".join(texts[t][c[0]:c[0] + c[1]] for t, c in reads)
    lens = np.array([c[3] for _, c in reads], dtype=np.uint32)
    longest = int(lens.max()) if n else 0
    if row_words is None:
        row_words = (max(max_read_len, 0) + 15) // 16
    rows = np.zeros((n, row_words), dtype=np.uint32)
    odd_cap = len(bases) + 1
    odd = np.zeros(odd_cap, dtype=np.uint64)
    n_odd = C.c_uint32(0)
    for r, (t, c) in enumerate(reads):
        seq = np.frombuffer(texts[t], dtype=np.uint8, count=c[3], offset=c[2])
        lib.mcx_pack_row(seq.ctypes.data, c[3], r, rows[r].ctypes.data, row_words, odd.ctypes.data, odd_cap, C.byref(n_odd))
    out = {"recs": [np.array(p[0], dtype=np.uint32).reshape(-1, 6) for p in per],
           "bases": np.frombuffer(bases, dtype=np.uint8), "qual": np.frombuffer(qual, dtype=np.uint8), "names": np.frombuffer(names, dtype=np.uint8),
           "off": np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)]).astype(np.uint32),
           "name_off": np.concatenate([[0], np.cumsum([c[1] for _, c in reads], dtype=np.uint64)]).astype(np.uint32),
           "rows": rows, "len": lens, "odd": odd[:n_odd.value].copy(), "row_words": row_words}
    out["info"] = {"n_records": n_rec + [0] * (2 - len(texts)), "stop": [p[1] for p in per] + [0] * (2 - len(texts)),
                   "consumed": [p[2] for p in per] + [0] * (2 - len(texts)), "n_reads": n, "longest": longest, "n_odd": int(n_odd.value),
                   "n_bases": len(bases), "n_name_bytes": len(names)}
    return out


# ---- the vectors --------------------------------------------------------------------------------------------
def rec(name, seq, qual=None, plus=b"+"):
    return b"@" + name + b"\n" + seq + b"\n" + plus + b"\n" + (b"I" * len(seq) if qual is None else qual) + b"\n"


def seeded_text(seed=7, size=200 * 1024):
    rng = random.Random(seed)
    out, k = [], 0
    while sum(map(len, out)) < size:
        n = rng.randint(1, 300)
        seq = bytes(rng.choice(b"ACGT") if rng.random() > 0.01 else rng.choice(b"NacgtRY") for _ in range(n))
        qual = bytes(rng.randint(33, 73) for _ in range(n))
        out.append(rec(b"r%d%s" % (k, rng.choice([b"", b" x", b"/1", b"\tq"])), seq, qual))
        k += 1
    return b"".join(out)


def make_vectors():
    """[(name, text, max_read_len)], each under 64 KB but the seeded one"""
    four = b"".join(rec(b"read%d/1" % i, s) for i, s in enumerate([b"ACGTACGTAC", b"TTTTGGGGCCCCAAAA", b"GATTACA", b"ACGTACGTACGTACGTACGTACGTACGTACGTA"]))
    v = [("four", four, 300), ("no_final_newline", four[:-1], 300), ("empty", b"", 300), ("newline", b"\n", 300),
         ("long_header", rec(b"h" * 150, b"ACGT") + rec(b"x" * 98 + b" tail", b"GGCC") + rec(b"y" * 99, b"TT"), 300),
         ("at_only", b"@\nACGT\n+\nIIII\n" + b"@@>name rest\nGGTT\n+\nIIII\n" + b"@@@@\nAC\n+\nII\n", 300),
         ("name_ends", b"".join(rec(b"nm" + e + b"more", b"ACGTAC") for e in (b" ", b"\t", b"/", b"\x7f", b"\x80", b"\x00", b"\x1f")), 300),
         ("crlf", four.replace(b"\n", b"\r\n"), 300),
         ("odd_bytes", rec(b"lc", b"acgtACGTnNacgt") + rec(b"iupac", b"RYKMSWBDHVN-.ACGT*") + rec(b"allN", b"N" * 40) + rec(b"mix", b"ACGTNACGTNACGTNACGTNACGTNACGTNACG"), 300),
         ("lengths", b"".join(rec(b"len%d" % n, (b"ACGTTGCA" * 700)[:n]) for n in (1, 15, 16, 17, 31, 32, 33, 5000)), 5000),
         ("qual_short_long", rec(b"short", b"ACGTACGTAC", b"III") + rec(b"long", b"ACGT", b"IIIIIIIIII") + rec(b"none", b"ACGT", b""), 300),
         ("qual_missing", rec(b"a", b"ACGT") + b"@b\nACGTAC\n+\n", 300), ("plus_missing", rec(b"a", b"ACGT") + b"@b\nACGTAC\n", 300),
         ("seq_unterminated", rec(b"a", b"ACGT") + b"@b\nACGTAC", 300), ("qual_unterminated_short", b"@b\nACGTAC\n+\nII", 300),
         ("empty_seq_middle", rec(b"a", b"ACGT") + b"@b\n\n+\n\n" + rec(b"c", b"GG"), 300),
         ("header_last", rec(b"a", b"ACGT") + rec(b"b", b"CC") + b"@c\n", 300), ("header_last_unterminated", rec(b"a", b"ACGT") + b"@c", 300),
         ("too_long", rec(b"a", b"ACGT") + rec(b"big", b"ACGT" * 13) + rec(b"c", b"GG"), 50), ("just_fits", rec(b"fit", b"ACGT" * 12 + b"AC"), 50),
         ("not_fastq", b"no header\n\nat all\n" * 5 + b"x", 300)]
    assert all(len(t) < 65536 for _, t, _ in v)
    return v + [("seeded", seeded_text(), 300)]


@pytest.fixture(scope="module")
def vectors():
    return make_vectors()


@pytest.fixture(scope="module")
def packer():
    """libmcx.so for its host packer mcx_pack_row (no device involved)"""
    from mapcaller_amd import api
    if not os.path.exists(api.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "mapcaller_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    L = api.lib()
    L.mcx_pack_row.restype = C.c_uint32
    L.mcx_pack_row.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    return L


def test_the_restatement_on_a_record_worked_by_hand(packer):
    e = restate(packer, [b"@@r1/1 x\nACNT\n+\nIIIIII\n@r2\nGG"], 10, 8, True)
    assert e["recs"][0].tolist() == [[2, 2, 9, 4, 16, 4], [24, 2, 27, 1, 0, 0]] and e["info"]["stop"][0] == END and e["info"]["consumed"][0] == 29
    assert e["bases"].tobytes() == b"ACNTG" and e["qual"].tobytes() == b"IIII\0" and e["names"].tobytes() == b"r1r2" and e["off"].tolist() == [0, 4, 5]
    assert e["rows"][:, 0].tolist() == [0b00010011 << 24, 0b10 << 30] and e["odd"].tolist() == [(0 << 32) | (2 << 8) | ord("N")]
    assert restate_text(b"@a\nAC\n+\nII\n@b\nAC\n+\nII", 10, 8, False)[1:] == (MORE, 11)


# ---- one driver for the three forms of the call: the host build, device tensors, host buffers ------------------------------------------
GROUPS = {"recs": ("recs",), "bases": ("bases", "off", "qual"), "names": ("names", "name_off"), "rows": ("rows", "len", "odd")}


def payload_sizes(exp, n_texts):
    """bytes written (and, for bases and qual, the 32 more the contract asks room for) per output of an expected result"""
    n, info = exp["info"]["n_reads"], exp["info"]
    w = {"bases": info["n_bases"], "qual": info["n_bases"], "off": (n + 1) * 4, "names": info["n_name_bytes"], "name_off": (n + 1) * 4,
         "rows": n * exp["row_words"] * 4, "len": n * 4, "odd": info["n_odd"] * 8}
    for t in range(n_texts):
        w["recs%d" % t] = info["n_records"][t] * 24
    room = dict(w)
    room["bases"] += 32
    room["qual"] += 32
    return w, room


def run_call(form, handle, texts, max_records, max_read_len, final, exp, groups=("recs", "bases", "names", "rows"), short=None, shift=0):
    """One call with outputs of exactly the sizes the contract asks for, 0xA5 all round.  form: "check" (handle: the host build), "dev" or "host"
    (handle: an api.FastqParser).  short: a capacity to give one too small.  shift: bytes the text lies off 16-byte alignment (dev).
    Returns (rc, info, outputs as numpy byte arrays with their guards, written sizes)."""
    from mapcaller_amd import api
    written, room = payload_sizes(exp, len(texts))
    keys = [k for g in groups for k in GROUPS[g] if k != "recs"] + (["recs%d" % t for t in range(len(texts))] if "recs" in groups else [])
    dev = form == "dev"
    if dev:
        import torch
        d = torch.device("cuda", 0)
        bufs = {k: torch.full((room[k] + 2 * G,), 0xA5, dtype=torch.uint8, device=d) for k in keys}
        tx = []
        for t in texts:
            b = torch.zeros(len(t) + 48, dtype=torch.uint8, device=d)
            b[16 + shift:16 + shift + len(t)] = torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).to(d)
            b[:16 + shift] = 10; b[16 + shift + len(t):] = 10  # (newlines outside the text: counted by a kernel that looks there)
            tx.append(b[16 + shift:])
    else:
        bufs = {k: np.full(room[k] + 2 * G, 0xA5, dtype=np.uint8) for k in keys}
        tx = [np.frombuffer(t + b"\n", dtype=np.uint8) for t in texts]
    kw = {k: bufs[k][G:] for k in keys if not k.startswith("recs")}
    if "recs" in groups:
        kw["recs"] = [bufs["recs%d" % t][G:] for t in range(len(texts))]
    kw.update(text_bytes=[len(t) for t in texts], bases_cap=room["bases"], names_cap=room["names"], odd_cap=exp["info"]["n_odd"], row_words=exp["row_words"])
    if short:
        kw[short] -= 1
    if form == "check":
        fi, fo = api.FastqParser._structs(lambda x: x.ctypes.data, lambda x: x.size, tx, max_records, max_read_len, final, kw)
        info = api.FastqInfo()
        rc = handle.fastq_check_parse(C.byref(fi), C.byref(fo), C.byref(info))
        info = info.as_dict()
    else:
        rc, info = (handle.parse_dev if dev else handle.parse)(tx, max_records, max_read_len, final, **kw)
    out = {k: (v.cpu().numpy() if dev else v) for k, v in bufs.items()}
    return rc, info, out, written


def assert_result(tag, rc, info, out, written, exp, untouched=()):
    assert rc == (0 if not untouched else -4), (tag, rc)
    assert info == exp["info"], (tag, info, exp["info"])
    want = {"bases": exp["bases"], "qual": exp["qual"], "names": exp["names"], "off": exp["off"], "name_off": exp["name_off"], "rows": exp["rows"],
            "len": exp["len"], "odd": exp["odd"], "recs0": exp["recs"][0], "recs1": exp["recs"][-1]}
    for k, buf in out.items():
        if k in untouched:
            assert (buf == 0xA5).all(), (tag, k, "a refused group was written to")
            continue
        w = written[k]
        assert (buf[:G] == 0xA5).all() and (buf[G + w:] == 0xA5).all(), (tag, k, "bytes written outside the output")
        assert buf[G:G + w].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (tag, k)


def cases_of(vectors):
    """(tag, texts, max_read_len): every vector alone, with itself and with the next one"""
    for i, (name, text, max_len) in enumerate(vectors):
        yield name, [text], max_len
        yield name + "+itself", [text, text], max_len
        other = vectors[(i + 1) % len(vectors)]
        yield name + "+" + other[0], [text, other[1]], max(max_len, other[2])


# ---- CPU: the rules compiled for the host -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fastq_check(tmp_path_factory):
    from mapcaller_amd import api
    out = str(tmp_path_factory.mktemp("fastq_check") / "libfastq_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", CHECK_SRC, "-o", out], check=True, stderr=subprocess.PIPE, timeout=600)
    L = C.CDLL(out)
    L.fastq_check_parse.restype = C.c_int
    L.fastq_check_parse.argtypes = [C.POINTER(api.FastqIn), C.POINTER(api.FastqOut), C.POINTER(api.FastqInfo)]
    return L


def test_host_build_equals_the_restatement_on_every_vector(fastq_check, packer, vectors):
    for tag, texts, max_len in cases_of(vectors):
        big = max(len(t) for t in texts) // 3 + 1
        for final, max_records in ((True, big), (False, big), (True, 2), (False, 1), (True, 0)):
            exp = restate(packer, texts, max_records, max_len, final)
            assert_result((tag, final, max_records), *run_call("check", fastq_check, texts, max_records, max_len, final, exp), exp)
    stops = {restate_text(t, 1 << 20, m, True)[1] for _, t, m in vectors}
    assert stops == {END, EMPTY, TOO_LONG}  # (the vectors reach every way a text can end)


@pytest.mark.parametrize("name", ["toy", "var"])
def test_host_build_equals_the_restatement_on_the_read_files(fastq_check, packer, golden, name):
    texts = [open(golden[name]["r1"], "rb").read(), open(golden[name]["r2"], "rb").read()]
    exp = restate(packer, texts, 1 << 20, 256, True)
    assert exp["info"]["n_reads"] == 2 * (texts[0].count(b"\n") // 4) and exp["info"]["stop"] == [END, END]
    assert_result(name, *run_call("check", fastq_check, texts, 1 << 20, 256, True, exp), exp)


def seeded_small_texts(n=1000, seed=11):
    rng = random.Random(seed)
    alphabet = b"\n" * 14 + b"@" * 5 + b"+" * 5 + b"ACGT" * 6 + b"N" * 3 + b" /\x00" * 2 + bytes(range(0x80, 0x100, 9)) + b"acgt\r\t>"
    return [bytes(rng.choice(alphabet) for _ in range(rng.randint(0, rng.choice([8, 64, 512, 4096])))) for _ in range(n)]


def test_host_build_under_the_sanitizers(tmp_path, vectors):
    """The stand-alone program (its own main; nothing of it is loaded into Python) built with -fsanitize=address,undefined: the vectors alone and in pairs, and 1 000
    seeded texts of at most 4 KB over an alphabet weighted towards newlines, '@', '+', bases, N, blank, '/', NUL and bytes >= 0x80 — each with final 0 and 1 and
    max_records 0 .. 3 and unbounded, into heap buffers of exactly the contract's sizes.  It must exit 0 and report nothing."""
    exe = str(tmp_path / "fastq_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-DFASTQ_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    CHECK_SRC, "-o", exe], check=True, stderr=subprocess.PIPE, timeout=600)
    small = seeded_small_texts()
    assert len(small) == 1000 and max(map(len, small)) <= 4096
    cases = [(texts, max_len) for _, texts, max_len in cases_of(vectors)] + [([t], 64) for t in small] + [([a, b], 64) for a, b in zip(small[::50], small[1::50])]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        for texts, max_len in cases:
            b = [len(t) for t in texts] + [0] * (2 - len(texts))
            f.write(struct.pack("<IIQQ", len(texts), max_len, b[0], b[1]) + b"".join(texts))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout == "" and r.stderr == "", (r.stdout[-1500:], r.stderr[-3000:])


# ---- GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


@pytest.mark.gpu
def test_parse_dev_equals_the_restatement_on_every_vector(api, packer, vectors):
    with api.FastqParser(0) as p:
        for tag, texts, max_len in cases_of(vectors):
            big = max(len(t) for t in texts) // 3 + 1
            for final, max_records in ((True, big), (False, big)) + (((True, 2), (False, 1), (True, 0)) if len(texts) == 1 else ()):
                exp = restate(packer, texts, max_records, max_len, final)
                assert_result((tag, final, max_records), *run_call("dev", p, texts, max_records, max_len, final, exp), exp)
        assert p.last_ms() > 0


@pytest.mark.gpu
def test_parse_dev_at_every_alignment_of_the_text(api, packer, vectors):
    head = vectors[-1][1][:8192]
    exp = restate(packer, [head], 4096, 300, True)
    assert exp["info"]["n_reads"] > 20
    with api.FastqParser(0) as p:
        for shift in range(16):
            assert_result(("shift", shift), *run_call("dev", p, [head], 4096, 300, True, exp, shift=shift), exp)


@pytest.mark.gpu
def test_a_text_fed_in_pieces(api, packer, vectors):
    """final = 0, 97 records a call, every piece from the last `consumed` on, the ends of the pieces at three arbitrary offsets; the last piece with final = 1"""
    import torch
    text = vectors[-1][1]
    whole = restate(packer, [text], 1 << 20, 300, True)
    d = torch.device("cuda", 0)
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(d)
    ends = [61003, 61007 + 70001, 150000 + 17, len(text)]
    pos, recs, bases, calls = 0, [], [], 0
    with api.FastqParser(0) as p:
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
                piece = restate(packer, [text[pos:end]], 97, 300, last)
                assert info == piece["info"]
                r = d_recs.cpu().numpy().view(np.uint32).reshape(-1, 6)[:n].astype(np.int64)
                r[:, [0, 2]] += pos
                r[:, 4] += np.where(r[:, 4] > 0, pos, 0)
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
    texts = [dict((n, t) for n, t, _ in vectors)["odd_bytes"], dict((n, t) for n, t, _ in vectors)["four"]]
    exp = restate(packer, texts, 100, 300, True)
    assert exp["info"]["n_odd"] > 0 and exp["info"]["n_name_bytes"] > 0
    with api.FastqParser(0) as p:
        for short, group in (("bases_cap", "bases"), ("names_cap", "names"), ("odd_cap", "rows")):
            rc, info, out, written = run_call("dev", p, texts, 100, 300, True, exp, short=short)
            assert rc == api.ERR_CAPACITY and "cap" in api.lib().mcx_last_error().decode()
            assert_result(short, rc, info, out, written, exp, untouched=GROUPS[group])  # (info holds the needs; the group is still 0xA5; the others are there)
        narrow = restate(packer, texts, 100, 300, True, row_words=18)  # ceil(300 / 16) = 19
        rc, info, out, written = run_call("dev", p, texts, 100, 300, True, narrow)
        assert rc == api.ERR_ARG and "row_words" in api.lib().mcx_last_error().decode()
        assert all((b == 0xA5).all() for b in out.values()) and info["n_reads"] == 0
        assert_result("afterwards", *run_call("dev", p, texts, 100, 300, True, exp), exp)


@pytest.mark.gpu
def test_the_host_buffer_form_and_a_parser_that_grows(api, packer, vectors):
    text = vectors[-1][1]
    exp = restate(packer, [text, text[:100000]], 1 << 20, 300, True)
    with api.FastqParser(0, max_text_bytes=4096, max_records=16) as p:
        assert p.grown() == 0
        assert_result("host", *run_call("host", p, [text, text[:100000]], 1 << 20, 300, True, exp), exp)
        g = p.grown()
        assert g >= 1
        assert_result("host again", *run_call("host", p, [text, text[:100000]], 1 << 20, 300, True, exp), exp)
        assert p.grown() == g  # (once: the second call finds room)
        for short, group in (("bases_cap", "bases"), ("names_cap", "names"), ("odd_cap", "rows")):
            rc, info, out, written = run_call("host", p, [text, text[:100000]], 1 << 20, 300, True, exp, short=short)
            assert_result(short, rc, info, out, written, exp, untouched=GROUPS[group])
        four = vectors[0][1]
        small = restate(packer, [four], 10, 300, True)
        assert_result("small", *run_call("host", p, [four], 10, 300, True, small), small)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy", "var"])
def test_device_chain_parse_map_format(api, golden, tmp_path, name):
    """Read files copied to HBM once, then per batch mcx_fastq_parse_dev (4 096 pairs, `consumed` carried) -> mcx_map_batch_dev -> mcx_sam_format_dev, all on
    tensors: no read text comes back to the host in between.  mcx_map_batch_dev takes paired batches on 200-read boundaries only, so what a parse
    gives beyond the last whole 200 reads waits, on the device, for the next one."""
    import torch
    g = golden[name]
    d = torch.device("cuda", 0)
    files = [open(g["r1"], "rb").read(), open(g["r2"], "rb").read()]
    d_text = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).to(d) for t in files]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="ksw2", max_read_len=256, max_batch_reads=8400)
    L = api.lib()
    text = api.sam_header(ix)
    pos, per, total_reads = [0, 0], 4096, 0
    held = None  # reads parsed and not mapped yet: (lens, name_lens, bases, qual, names)
    with api.FastqParser(0) as p:
        done = False
        while not done:
            cap = sum(len(t) - q for t, q in zip(files, pos)) + 32
            o = {"bases": torch.zeros(cap, dtype=torch.uint8, device=d), "qual": torch.zeros(cap, dtype=torch.uint8, device=d), "off": torch.zeros(2 * per + 1, dtype=torch.int32, device=d),
                 "names": torch.zeros(cap, dtype=torch.uint8, device=d), "name_off": torch.zeros(2 * per + 1, dtype=torch.int32, device=d)}
            rc, info = p.parse_dev([d_text[0][pos[0]:], d_text[1][pos[1]:]], per, 256, final=True, text_bytes=[len(files[0]) - pos[0], len(files[1]) - pos[1]], **o)
            assert rc == 0 and info["n_records"][0] == info["n_records"][1]
            n = info["n_reads"]
            pos = [a + b for a, b in zip(pos, info["consumed"])]
            done = info["stop"][0] != MORE or n == 0
            new = (o["off"][1:n + 1] - o["off"][:n], o["name_off"][1:n + 1] - o["name_off"][:n], o["bases"][:info["n_bases"]], o["qual"][:info["n_bases"]], o["names"][:info["n_name_bytes"]])
            held = new if held is None else tuple(torch.cat([a, b]) for a, b in zip(held, new))
            m = held[0].numel() if done else held[0].numel() // 200 * 200
            if m == 0:
                continue
            zero = torch.zeros(1, dtype=torch.int64, device=d)
            off = torch.cat([zero, torch.cumsum(held[0].long(), 0)])
            noff = torch.cat([zero, torch.cumsum(held[1].long(), 0)])
            nb, nn = int(off[m]), int(noff[m])  # (two sizes, no text)
            bases = torch.cat([held[2][:nb], torch.zeros(32, dtype=torch.uint8, device=d)])
            qual, names = held[3][:nb].clone(), held[4][:nn].clone()
            d_off, d_noff = off[:m + 1].to(torch.int32), noff[:m + 1].to(torch.int32)
            held = (held[0][m:], held[1][m:], held[2][nb:], held[3][nb:], held[4][nn:])
            d_aln = torch.zeros(m * 64, dtype=torch.uint8, device=d)
            d_cig = torch.zeros(api.cigar_pool_words(m), dtype=torch.int32, device=d)
            mp.map_batch_dev(bases.data_ptr(), d_off.data_ptr(), m, True, d_aln.data_ptr(), d_cig.data_ptr())  # (mp.avg: the insert-size state carried from batch to batch)
            di = api.SamIn()
            di.bases, di.off, di.qual, di.names, di.name_off = bases.data_ptr(), d_off.data_ptr(), qual.data_ptr(), names.data_ptr(), d_noff.data_ptr()
            di.aln, di.cigar, di.n_reads, di.paired = d_aln.data_ptr(), d_cig.data_ptr(), m, 1
            size = C.c_uint64()
            assert L.mcx_sam_format_dev(mp._h, C.byref(di), None, 0, None, C.byref(size)) == api.ERR_CAPACITY
            d_sam = torch.zeros(size.value, dtype=torch.uint8, device=d)
            assert L.mcx_sam_format_dev(mp._h, C.byref(di), d_sam.data_ptr(), size.value, None, C.byref(size)) == 0, L.mcx_last_error()
            text += d_sam.cpu().numpy().tobytes()
            total_reads += m
    mp.close(); ix.close()
    assert pos == [len(files[0]), len(files[1])] and total_reads == 2 * (files[0].count(b"\n") // 4)
    out = tmp_path / "chain.sam"
    out.write_bytes(text)
    nd, ex = sam_diff(g["sam"]["ksw2"], str(out))
    assert nd == 0, ex


def _map(api, prefix, fq1, fq2, out, alg="ksw2", full_sa=True, **kw):
    ix = api.Index(prefix, device=0, full_sa=full_sa)
    mp = api.Mapper(ix, alg=alg, max_batch_reads=1000)
    try:
        return mp.map_files(fq1, fq2, out, **kw)
    finally:
        mp.close(); ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [("toy", {}), ("var", {}), ("se", {}), ("var", {"device_sam": True})])
def test_front_end_with_device_parse_equals_reference(api, golden, tmp_path, name, kw):
    g = golden[name]
    out = str(tmp_path / "dev.sam")
    st = _map(api, g["prefix"], g["r1"], g["r2"], out, device_parse=True, **kw)
    n_lines = open(g["r1"], "rb").read().count(b"\n")
    assert st["reads"] == (2 * (n_lines // 4) if g["r2"] else n_lines // 2)  # (several batches of 1 000 and a partial last one; se: FASTA, read as before)
    nd, ex = sam_diff(g["sam"]["ksw2"], out)
    assert nd == 0, ex


@pytest.mark.gpu
def test_front_end_with_device_parse_on_one_fastq_file(api, golden, tmp_path):
    """The golden single-end set is FASTA, which the switch leaves alone: its reads as a FASTQ file, host reader against device parser."""
    g = golden["se"]
    fa = open(g["r1"], "rb").read().split(b"\n")
    fq = tmp_path / "se.fq"
    fq.write_bytes(b"".join(b"@" + h[1:] + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for h, s in zip(fa[0::2], fa[1::2]) if h))
    out, plain = str(tmp_path / "dev.sam"), str(tmp_path / "host.sam")
    st = _map(api, g["prefix"], str(fq), None, out, device_parse=True)
    st0 = _map(api, g["prefix"], str(fq), None, plain)
    assert st["reads"] == st0["reads"] == len(fa) // 2
    assert open(out, "rb").read() == open(plain, "rb").read()


@pytest.mark.gpu
def test_front_end_with_device_parse_on_an_interleaved_file_with_an_odd_tail(api, io_golden, tmp_path):
    g = io_golden
    out = str(tmp_path / "il.sam")
    st = _map(api, g["prefix"], g["il.fq"], None, out, full_sa=False, interleaved=True, device_parse=True)
    assert st["reads"] == open(g["il.fq"], "rb").read().count(b"\n") // 4 and st["reads"] % 2 == 1
    nd, ex = sam_diff(g["ref.il.sam"], out, mask_se_reverse_qual=True)
    assert nd == 0, ex


@pytest.mark.gpu
def test_files_that_stop_early_end_the_same_way_with_and_without_device_parse(api, golden, tmp_path):
    """Return code, error text, read count and SAM bytes with the switch off and on.  Where the run fails the file is not compared: how many batches
    were written before the failure reached the mapper depends on the threads' timing, with either reader."""
    g = golden["toy"]
    r1, r2 = open(g["r1"], "rb").read(), open(g["r2"], "rb").read()
    l1, l2 = r1.split(b"\n"), r2.split(b"\n")

    def swap(lines, i, new):
        return b"\n".join(lines[:i] + [new] + lines[i + 1:])
    cases = {"short_file_2": (r1, b"\n".join(l2[:-5]) + b"\n"), "empty_sequence": (swap(l1, 4 * 500 + 1, b""), r2), "too_long": (swap(l1, 4 * 700 + 1, b"ACGT" * 64 + b"A"), r2),
             "no_final_newline": (r1[:-1], r2[:-1]), "crlf": (r1.replace(b"\n", b"\r\n"), r2.replace(b"\n", b"\r\n"))}
    for tag, (a, b) in cases.items():
        fa, fb = tmp_path / (tag + "_1.fq"), tmp_path / (tag + "_2.fq")
        fa.write_bytes(a); fb.write_bytes(b)
        got = []
        for switch in (False, True):
            out = tmp_path / f"{tag}_{int(switch)}.sam"
            try:
                st = _map(api, g["prefix"], str(fa), str(fb), str(out), device_parse=switch)
                got.append((0, "", st["reads"], out.read_bytes()))
            except api.McxError as e:
                got.append((1, str(e), None, None))
        assert got[0] == got[1], (tag, got[0][:3], got[1][:3])
        if tag in ("short_file_2", "too_long"):
            assert got[0][0] == 1 and ("holds fewer reads than" if tag == "short_file_2" else "is longer than max_read_len") in got[0][1], (tag, got[0][1])
        else:
            assert got[0][0] == 0 and got[0][2] == {"empty_sequence": 1000, "no_final_newline": 3000, "crlf": 3000}[tag], (tag, got[0][:3])


@pytest.mark.gpu
def test_cli_gpu_parse(golden, tmp_path):
    g = golden["toy"]
    out = str(tmp_path / "cli.sam")
    r = subprocess.run([EXE, "-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-alg", "ksw2", "-sam", out, "-no_vcf", "-gpu_parse"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    nd, ex = sam_diff(g["sam"]["ksw2"], out)
    assert nd == 0, ex
