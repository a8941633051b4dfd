"""SAM text made on the device: mcx_sam_format_dev / mcx_sam_format / mcx_sam_header and the file front end's device_sam (-gpu_sam).

CPU: the ABI surface, and the formatter itself (mapcaller_amd/csrc/mcx_sam.h compiled for the host, tests/hostemu/sam_check.cpp) against every
golden SAM: the records are parsed back out of the reference's files, the reads taken from the read files by the reference's rules, and the
text made from them must be the file again.  GPU: the same bytes through the kernels — the file front end with device_sam on every golden set,
the ABI on device and host buffers, a synthetic input against the host formatter, the command lines."""
import ctypes as C
import gzip
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, SETS, sam_diff, vcf_alg, vcf_body
from test_multi import MULTI_SETS, compare, mask_se_extra_flags, read_extras, rebuild_multi

NEW = ("mcx_sam_format_dev", "mcx_sam_format", "mcx_sam_header")
ALGS = ("nw", "ksw2")
EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")


# ---- CPU: the surface ---------------------------------------------------------------------------------------
def test_the_sam_calls_are_declared_bound_and_exported():
    from mapcaller_amd import api, run
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for s in NEW:
        assert s in api.SYMBOLS and re.search(r"\b%s\s*\(" % s, header), s
    assert "device_sam" in header and "reserved0" not in header
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in NEW:
            assert f" {s}\n" in nm, s
        L = api.lib()
        for s in ("mcx_sam_format_dev", "mcx_sam_format"):
            assert getattr(L, s).argtypes[3] is C.c_uint64 and getattr(L, s).argtypes[2] is C.c_void_p
        assert L.mcx_sam_header.argtypes[2] is C.c_uint64
        assert L.mcx_gz_inflate.restype is C.c_int64 and L.mcx_gz_inflate.argtypes[4] is C.c_uint64
    names = [f[0] for f in api.FileOpts._fields_]
    assert names[:4] == ["interleaved_pairs", "host_threads", "append_sam", "device_sam"] and api.FileOpts.device_sam.offset == 12
    assert inspect.signature(api.Mapper.map_files).parameters["device_sam"].default is False
    assert "sam_text" in dir(api.Mapper) and callable(api.sam_header)
    assert run.parse(["-i", "x", "-f", "a.fq", "-sam", "o.sam", "-gpu_sam"]).gpu_sam and not run.parse(["-i", "x", "-f", "a.fq"]).gpu_sam
    assert "-gpu_sam" in open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_main.cpp")).read()


# ---- reads and records as the reference holds them ----------------------------------------------------------------
def header_name(line):
    """IdentifyHeaderBegPos / IdentifyHeaderEndPos (GetData.cpp:3-20) on a header line with its newline."""
    n = len(line)
    lim = min(n, 100)
    p1, p2 = n - 1, lim - 1
    for i in range(1, n):
        if line[i] not in b">@":
            p1 = i
            break
    for i in range(1, lim):
        if line[i] <= 32 or line[i] == 47 or line[i] >= 127:
            p2 = i
            break
    return line[p1:p2] if p2 > p1 else b""


def lines_of(data, gz):
    """getline's lines with their newline; the .gz reader's gzgets(buffer, 1024) cuts at 1023 bytes."""
    parts = data.split(b"\n")
    lines = [p + b"\n" for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])
    if not gz:
        return lines
    out = []
    for l in lines:
        out.extend(l[i:i + 1023] for i in range(0, len(l), 1023))
    return out


def parse_reads(path, gz=False):
    """[(name, bases, quality bytes that count or None)] by GetNextEntry / gzGetNextEntry (GetData.cpp:33-128): the last byte of a sequence
    line dropped, min(quality line, read length) bytes of quality taken, multi-line FASTA for plain files."""
    data = gzip.open(path, "rb").read() if gz else open(path, "rb").read()
    lines = lines_of(data, gz)
    out = []
    if data[:1] == b"@":
        for i in range(0, len(lines), 4):
            if i + 1 >= len(lines) or len(lines[i + 1]) < 2:
                break
            seq = lines[i + 1][:-1]
            q = lines[i + 3] if i + 3 < len(lines) else b""
            out.append((header_name(lines[i]), seq, q[:min(len(q), len(seq))]))
        return out
    i = 0
    while i < len(lines):
        name, seq = header_name(lines[i]), b""
        i += 1
        if gz:
            seq = lines[i][:-1] if i < len(lines) else b""
            i += 1
        else:
            while i < len(lines) and lines[i][:1] != b">":
                seq += lines[i][:-1]
                i += 1
        if not seq:
            break
        out.append((name, seq, None))
    return out


OPS = {c: i for i, c in enumerate("MIDNSHP=")}


def parse_line(line, contigs):
    """(QNAME, record fields, CIGAR words) of a SAM line"""
    f = line.split("\t")
    flag = int(f[1])
    rec = dict(flag=flag, chr=-1 if f[2] == "*" else contigs.index(f[2]), pos=int(f[3]), mapq=int(f[4]), has_mate=int(f[6] == "="), mate_pos=int(f[7]),
               tlen=int(f[8]), fwd=int(not flag & 0x10), nm=0, xs=0)
    rec["as"] = 0
    for t in f[11:]:
        if t[:5] in ("NM:i:", "AS:i:", "XS:i:"):
            rec[t[:2].lower()] = int(t[5:])
    words = [] if f[5] == "*" else [(int(n) << 4) | OPS[c] for n, c in re.findall(r"(\d+)([MIDNSHP=])", f[5])]
    if f[5] != "*":
        assert "".join(f"{w >> 4}{'MIDNSHP='[w & 7]}" for w in words) == f[5], f[5]
    return f[0], rec, words


COMP = bytes([{65: 84, 67: 71, 71: 67, 84: 65, 97: 84, 99: 71, 103: 67, 116: 65}.get(c, 78) for c in range(256)])  # GetComplementaryBase


def records_of(lines, contigs, mate2, bases, flag_unset=False):
    """ALN_DTYPE records + one CIGAR pool for SAM lines.  mate2[i]: the line is of the second read of a pair — the reference maps the reverse complement of
    that read (ReadMapping.cpp:451), so the strand its record speaks of (fwd) is the other one than FLAG 0x10 says of the read as it came.  A mapped read
    of a pair whose mate is not (FLAG 0x8) carries 0x10 AND 0x20 whatever its strand (SetPairedAlignmentFlag, SamReport.cpp:26-84): FLAG does not hold the
    record's strand there, so it is read off the line's SEQ — the reverse complement of the read's bases (bases[i]) or not.  flag_unset: the -m lines
    of single-end reads, whose FLAG the reference leaves unset (test_multi.mask_se_extra_flags reads their strand off SEQ too)."""
    from mapcaller_amd import api
    aln = np.zeros(len(lines), dtype=api.ALN_DTYPE)
    pool, names = [], []
    for i, l in enumerate(lines):
        name, rec, words = parse_line(l, contigs)
        names.append(name)
        if mate2[i]:
            rec["fwd"] = 1 - rec["fwd"]
        if flag_unset or (rec["flag"] & 0x1 and rec["flag"] & 0x8 and rec["flag"] & 0x30 == 0x30):
            turned = l.split("\t")[9].encode("latin-1") == bases[i].translate(COMP)[::-1]
            rec["fwd"] = int(turned == bool(mate2[i]))
        for k, v in rec.items():
            aln[i][k] = v
        aln[i]["n_cigar"], aln[i]["cigar_off"] = len(words), len(pool)
        pool.extend(words)
    return aln, np.array(pool + [0], dtype=np.uint32), names


def sam_in(api, reads, paired, aln, pool, extras=None, keep=None):
    """api.SamIn over host arrays for `reads` (kept alive in `keep`)"""
    n = len(reads)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(r[1]) for r in reads])
    name_off = np.zeros(n + 1, dtype=np.uint32)
    name_off[1:] = np.cumsum([len(r[0]) for r in reads])
    bases = np.frombuffer(b"".join(r[1] for r in reads) + b"\0" * 64, dtype=np.uint8).copy()
    names = np.frombuffer(b"".join(r[0] for r in reads) + b"\0", dtype=np.uint8).copy()
    si = api.SamIn()
    si.bases, si.off, si.names, si.name_off = bases.ctypes.data, off.ctypes.data, names.ctypes.data, name_off.ctypes.data
    si.aln, si.cigar, si.n_reads, si.paired = aln.ctypes.data, pool.ctypes.data, n, int(paired)
    keep += [off, name_off, bases, names, aln, pool]
    if n and reads[0][2] is not None:
        q = np.zeros(int(off[-1]) + 1, dtype=np.uint8)  # NUL behind what the reference took of the quality line
        for r, (_, seq, qual) in enumerate(reads):
            q[int(off[r]):int(off[r]) + len(qual)] = np.frombuffer(qual, dtype=np.uint8)
        si.qual = q.ctypes.data
        keep.append(q)
    if extras is not None:
        index, x_aln, x_pool = extras
        si.x_index, si.x_recs, si.x_cigar = index.ctypes.data, x_aln.ctypes.data, x_pool.ctypes.data
        keep += [index, x_aln, x_pool]
    return si, off


@pytest.fixture(scope="session")
def sam_check(tmp_path_factory):
    """mcx_sam.h for the host (tests/hostemu/sam_check.cpp)"""
    out = str(tmp_path_factory.mktemp("sam_check") / "libsam_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", os.path.join(ROOT, "tests", "hostemu", "sam_check.cpp"), "-o", out],
                   check=True, stderr=subprocess.PIPE, timeout=600)
    from mapcaller_amd import api
    L = C.CDLL(out)
    L.sam_check_format.restype = C.c_int64
    L.sam_check_format.argtypes = [C.POINTER(api.SamIn), C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def host_format(L, reads, n_pair_reads, lines, contigs, extras=None):
    """The text of `reads` whose first lines are `lines` (and whose further lines are `extras`: [(read, line)]), through the host build of the
    device's formatter: the pairs' part and the single reads' part, as the file front end maps them.  Returns (text, per-read lengths)."""
    from mapcaller_amd import api
    cn_text = "".join(contigs).encode()
    cn_off = np.zeros(len(contigs) + 1, dtype=np.uint32)
    cn_off[1:] = np.cumsum([len(c) for c in contigs])
    text, lens = b"", []
    for lo, hi, paired in ((0, n_pair_reads, True), (n_pair_reads, len(reads), False)):
        if hi == lo:
            continue
        keep = []
        aln, pool, names = records_of(lines[lo:hi], contigs, [paired and i % 2 == 1 for i in range(hi - lo)], [r[1] for r in reads[lo:hi]])
        assert names == [r[0].decode("latin-1") for r in reads[lo:hi]], "the read files and the SAM do not line up"
        x = None
        if extras is not None:
            mine = [(i - lo, l) for i, l in extras if lo <= i < hi]
            index = np.zeros(hi - lo + 1, dtype=np.uint32)
            for i, _ in mine:
                index[i + 1] += 1
            index = np.cumsum(index).astype(np.uint32)
            x_aln, x_pool, x_names = records_of([l for _, l in mine], contigs, [paired and i % 2 == 1 for i, _ in mine], [reads[lo + i][1] for i, _ in mine], flag_unset=not paired)
            assert x_names == [names[i] for i, _ in mine]
            x = (index, x_aln, x_pool)
        si, off = sam_in(api, reads[lo:hi], paired, aln, pool, x, keep)
        line_off = np.zeros(hi - lo + 1, dtype=np.uint64)
        assert L.sam_check_format(C.byref(si), cn_text, cn_off.ctypes.data, None, 0, line_off.ctypes.data) == -1  # (the size alone)
        total = int(line_off[-1])
        out = np.full(total + 64, 0xA5, dtype=np.uint8)
        assert L.sam_check_format(C.byref(si), cn_text, cn_off.ctypes.data, out.ctypes.data, total, line_off.ctypes.data) == total
        assert (out[total:] == 0xA5).all()
        text += out[:total].tobytes()
        lens += np.diff(line_off).astype(np.int64).tolist()
    return text, lens


def split_golden(path):
    text = open(path, "rb").read().decode("latin-1")
    lines = text.split("\n")
    head = [l for l in lines if l.startswith("@")]
    body = [l for l in lines if l and not l.startswith("@")]
    return head, body, [l.split("\t")[1][3:] for l in head if l.startswith("@SQ")]


def interleave(a, b):
    out = []
    for x, y in zip(a, b):
        out += [x, y]
    return out


def n_pairs_part(n, paired):
    """reads of a stream mapped as pairs: all of them, or — an odd number of interleaved reads — the whole 200-read chunks (ReadMapping.cpp:442)"""
    if not paired:
        return 0
    return n if n % 2 == 0 else n // 200 * 200


def check_text(tmp_path, got, want_lines, masked):
    a, b = tmp_path / "want.sam", tmp_path / "got.sam"
    a.write_bytes(("\n".join(want_lines) + "\n").encode("latin-1"))
    b.write_bytes(got)
    nd, ex = sam_diff(str(a), str(b), mask_se_reverse_qual=masked)
    assert nd == 0, ex


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("name", list(SETS))
def test_host_build_of_the_formatter_rewrites_the_golden_sam(sam_check, golden, tmp_path, name, alg):
    g = golden[name]
    paired = SETS[name]
    reads = parse_reads(g["r1"])
    if g["r2"]:
        reads = interleave(reads, parse_reads(g["r2"]))
    _, body, contigs = split_golden(g["sam"][alg])
    assert len(body) == len(reads)
    got, lens = host_format(sam_check, reads, n_pairs_part(len(reads), paired), body, contigs)
    # (the reference prints an uninitialised first quality byte for reverse-strand single-end FASTQ reads: conftest.sam_diff's mask, on single-end sets only)
    check_text(tmp_path, got, body, masked=not paired)
    if paired or reads[0][2] is None:
        assert lens == [len(l.encode("latin-1")) + 1 for l in body]
    if name in MULTI_SETS:  # -m: every read's further lines behind its first
        extras = read_extras(name, alg)
        got, lens = host_format(sam_check, reads, n_pairs_part(len(reads), paired), body, contigs, extras)
        want, _ = mask_se_extra_flags(rebuild_multi("\n".join(body) + "\n", extras), paired)
        mine, _ = mask_se_extra_flags(got.decode("latin-1"), paired)
        check_text(tmp_path, mine.encode("latin-1"), [l for l in want.split("\n") if l], masked=not paired)
        by = {}
        for i, l in extras:
            by[i] = by.get(i, 0) + len(l.encode("latin-1")) + 1
        assert lens == [len(l.encode("latin-1")) + 1 + by.get(i, 0) for i, l in enumerate(body)]


@pytest.mark.parametrize("case", ["il", "ml", "gz", "lib"])
def test_host_build_of_the_formatter_rewrites_the_input_side_cases(sam_check, io_golden, tmp_path, case):
    g = io_golden
    if case == "il":
        reads, paired = parse_reads(g["il.fq"]), True
    elif case == "ml":
        reads, paired = parse_reads(g["ml.fa"]), False
    elif case == "gz":
        reads, paired = interleave(parse_reads(g["gz1"], gz=True), parse_reads(g["gz2"], gz=True)), True
    else:
        reads, paired = interleave(parse_reads(g["a1"]) + parse_reads(g["b1"]), parse_reads(g["a2"]) + parse_reads(g["b2"])), True
    _, body, contigs = split_golden(g[f"ref.{case}.sam"])
    assert len(body) == len(reads)
    got, _ = host_format(sam_check, reads, n_pairs_part(len(reads), paired), body, contigs)
    check_text(tmp_path, got, body, masked=True)  # (as tests/test_gpu_parity.py::test_input_side_cases compares them)


# ---- GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


def _map_files(api, g, alg, out, multi=False, **kw):
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg=alg, multi=multi, **kw)
    st = mp.map_files(g["r1"], g["r2"], out, device_sam=True)
    mp.close(); ix.close()
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("name", list(SETS))
def test_device_sam_equals_reference(api, golden, tmp_path, name, alg):
    g = golden[name]
    for batch in (1 << 14, 400):  # (400: batch seams, replays, and both parts of a batch)
        out = str(tmp_path / f"gpu{batch}.sam")
        st = _map_files(api, g, alg, out, max_batch_reads=batch)
        assert st["reads"] > 0
        nd, ex = sam_diff(g["sam"][alg], out)  # (no mask: tests/test_gpu_parity.py::test_sam_equals_reference uses none)
        assert nd == 0, (batch, ex)


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("name", MULTI_SETS)
def test_device_sam_with_multi_equals_reference(api, golden, tmp_path, name, alg):
    for batch in (1 << 14, 400):
        out = str(tmp_path / f"m{batch}.sam")
        _map_files(api, golden[name], alg, out, multi=True, max_batch_reads=batch)
        compare(name, alg, out)


@pytest.mark.gpu
def test_device_sam_input_side_cases(api, io_golden, tmp_path):
    """tests/test_gpu_parity.py::test_input_side_cases through device_sam, and the two libraries (append_sam)"""
    g = io_golden
    ix = api.Index(g["prefix"], device=0)
    for alg, args, kw, ref in (("ksw2", (g["il.fq"], None), {"interleaved": True}, "ref.il.sam"),
                               ("nw", (g["ml.fa"], None), {}, "ref.ml.sam"),
                               ("ksw2", (g["gz1"], g["gz2"]), {"threads": 3}, "ref.gz.sam")):
        mp = api.Mapper(ix, alg=alg, max_batch_reads=1000)
        out = str(tmp_path / (ref + ".out"))
        mp.map_files(args[0], args[1], out, device_sam=True, **kw)
        nd, ex = sam_diff(g[ref], out, mask_se_reverse_qual=True)
        assert nd == 0, (ref, ex)
        mp.close()
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1000)
    out = str(tmp_path / "lib.out")
    mp.map_files(g["a1"], g["a2"], out, device_sam=True)
    mp.map_files(g["b1"], g["b2"], out, device_sam=True, append_sam=True)
    nd, ex = sam_diff(g["ref.lib.sam"], out)
    assert nd == 0, ex
    mp.close(); ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,alg,multi", [("mc", "nw", False), ("se", "ksw2", False), ("var", "ksw2", True), ("toy", "ksw2", False)])
def test_format_dev_on_tensors(api, golden, tmp_path, name, alg, multi):
    import torch
    g = golden[name]
    paired = SETS[name]
    reads = parse_reads(g["r1"])
    if g["r2"]:
        reads = interleave(reads, parse_reads(g["r2"]))
    n = len(reads)
    head, body, _ = split_golden(g["sam"][alg])
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    assert api.sam_header(ix) == ("\n".join(head) + "\n").encode("latin-1")
    mp = api.Mapper(ix, alg=alg, max_read_len=256, max_batch_reads=(n + 199) // 200 * 200, multi=multi)
    keep = []
    dummy = np.zeros(1, dtype=api.ALN_DTYPE)
    si, off = sam_in(api, reads, paired, dummy, np.zeros(1, dtype=np.uint32), None, keep)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in zip(("off", "name_off", "bases", "names"), keep[:4])}
    d_aln = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_cig = torch.zeros(api.cigar_pool_words(n), dtype=torch.int32, device=dev)
    mp.map_batch_dev(t["bases"].data_ptr(), t["off"].data_ptr(), n, paired, d_aln.data_ptr(), d_cig.data_ptr())
    di = api.SamIn()
    di.bases, di.off, di.names, di.name_off = t["bases"].data_ptr(), t["off"].data_ptr(), t["names"].data_ptr(), t["name_off"].data_ptr()
    di.aln, di.cigar, di.n_reads, di.paired = d_aln.data_ptr(), d_cig.data_ptr(), n, int(paired)
    if si.qual:
        t["qual"] = torch.from_numpy(keep[6]).to(dev)
        di.qual = t["qual"].data_ptr()
    extras = None
    if multi:
        p = [C.c_void_p() for _ in range(3)]
        nl, nw = C.c_uint32(), C.c_uint32()
        assert api.lib().mcx_multi_lines(mp._h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(nl), C.byref(nw)) == 0
        di.x_index, di.x_recs, di.x_cigar = p[0].value, p[1].value, p[2].value
        extras = mp.multi_lines(n)
    L = api.lib()
    nb = C.c_uint64()
    assert L.mcx_sam_format_dev(mp._h, C.byref(di), None, 0, None, C.byref(nb)) == api.ERR_CAPACITY
    total = nb.value
    d_text = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device=dev)
    d_line = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    nb2 = C.c_uint64()
    assert L.mcx_sam_format_dev(mp._h, C.byref(di), d_text.data_ptr(), total - 1, d_line.data_ptr(), C.byref(nb2)) == api.ERR_CAPACITY
    assert nb2.value == total and bool((d_text == 0x5A).all())  # too small: the size again, and not a byte written
    assert L.mcx_sam_format_dev(mp._h, C.byref(di), d_text.data_ptr(), total, d_line.data_ptr(), C.byref(nb2)) == 0, L.mcx_last_error()
    assert nb2.value == total and bool((d_text[total:] == 0x5A).all())
    text = d_text[:total].cpu().numpy().tobytes()
    line_off = d_line.cpu().numpy()
    assert line_off[0] == 0 and line_off[-1] == total and (np.diff(line_off) > 0).all()
    assert all(text[int(e) - 1] == 10 for e in line_off[1:])
    if multi:
        out = tmp_path / "m.sam"
        out.write_bytes(("\n".join(head) + "\n").encode("latin-1") + text)
        compare(name, alg, str(out))
    else:
        check_text(tmp_path, text, body, masked=False)
    # the same from host arrays
    aln = np.frombuffer(d_aln.cpu().numpy().tobytes(), dtype=api.ALN_DTYPE).copy()
    pool = d_cig.cpu().numpy().view(np.uint32).copy()
    host = mp.sam_text(keep[2][:int(off[-1])], off, [r[0] for r in reads], None if reads[0][2] is None else [r[2] for r in reads], paired, aln, pool, extras)
    assert host == text
    mp.close(); ix.close()


def synthetic_reads(path1, path2, genome, seed, n_pairs, max_len):
    """Pairs of ragged lengths 1..max_len off `genome` with what the formatter must carry through: lower case, N and IUPAC bytes, indels (long CIGARs),
    quality lines shorter and longer than the read, long and decorated names."""
    rng = np.random.default_rng(seed)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    with open(path1, "wb") as f1, open(path2, "wb") as f2:
        for i in range(n_pairs):
            frag = int(rng.integers(max_len, 2 * max_len))
            at = int(rng.integers(0, len(genome) - frag))
            piece = genome[at:at + frag]
            for f, mate in ((f1, 0), (f2, 1)):
                rlen = int(rng.choice([1, 2, 17, 63, 64, 65, 150, 151, 255, max_len, int(rng.integers(1, max_len + 1))]))
                seq = bytearray(piece[:rlen] if mate == 0 else piece[::-1].translate(comp)[:rlen])
                if rng.random() < 0.3 and rlen > 120:  # indels every few dozen bases: CIGARs of tens of operations
                    k = 40
                    while k < len(seq) - 40:
                        if rng.random() < 0.5:
                            del seq[k]
                        else:
                            seq.insert(k, b"ACGT"[int(rng.integers(0, 4))])
                        k += int(rng.integers(25, 60))
                    seq = seq[:max_len]
                for _ in range(int(rng.integers(0, 4))):
                    k = int(rng.integers(0, len(seq)))
                    seq[k] = b"acgtNnRYKM"[int(rng.integers(0, 10))]
                qual = bytes(rng.integers(33, 74, len(seq)).astype(np.uint8))
                cut = rng.random()
                if cut < 0.1:
                    qual = qual[:int(rng.integers(0, len(seq) + 1))]
                elif cut < 0.2:
                    qual += b"I" * int(rng.integers(1, 30))
                name = b"r%d" % i + (b"_" + b"x" * int(rng.integers(60, 120)) if rng.random() < 0.1 else b"") + (b" desc/1" if rng.random() < 0.3 else b"/%d" % (mate + 1))
                f.write(b"@" + name + b"\n" + bytes(seq) + b"\n+\n" + qual + b"\n")


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [True, False])
def test_device_sam_equals_the_host_formatter_on_synthetic_reads(api, golden, tmp_path, paired):
    genome = b"".join(l for l in gzip.open(os.path.join(GOLD, "mc", "genome.fa.gz")).read().split(b"\n") if not l.startswith(b">"))
    f1, f2 = str(tmp_path / "s1.fq"), str(tmp_path / "s2.fq")
    synthetic_reads(f1, f2, genome, 20260117, 3000, 1000)
    ix = api.Index(golden["mc"]["prefix"], device=0, full_sa=True)
    outs = []
    for dev_sam in (False, True):
        for multi in (False, True):
            mp = api.Mapper(ix, alg="ksw2", max_read_len=1000, max_batch_reads=2000, multi=multi)
            out = str(tmp_path / f"o{int(dev_sam)}{int(multi)}.sam")
            st = mp.map_files(f1, f2 if paired else None, out, device_sam=dev_sam)
            assert st["reads"] == (6000 if paired else 3000) and st["mapped"] > 1000
            mp.close()
            outs.append(open(out, "rb").read())
    ix.close()
    assert outs[0] == outs[2] and outs[1] == outs[3]
    # (a quality line shorter than its read is taken with its newline — GetData.cpp:51-52 — which then stands inside QUAL: only whole lines are looked at here)
    body = [l for l in outs[2].split(b"\n") if l and not l.startswith(b"@") and l.count(b"\t") >= 11]
    assert max(l.split(b"\t")[5].count(b"I") + l.split(b"\t")[5].count(b"D") for l in body) >= 10  # long CIGARs were among them
    assert max(len(l) for l in body) > 2048  # ... and lines longer than the kernel's staging


def _cli(args, timeout=900):
    subprocess.run([EXE] + args, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout)


@pytest.mark.gpu
def test_cli_gpu_sam(golden, tmp_path):
    g = golden["mc"]
    alg = vcf_alg("mc", "default")
    sam, vcf = str(tmp_path / "o.sam"), str(tmp_path / "o.vcf")
    _cli(["-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-alg", alg, "-sam", sam, "-vcf", vcf, "-gpu_sam", "-t", "2"])
    nd, ex = sam_diff(g["sam"][alg], sam)
    assert nd == 0, ex
    assert vcf_body(vcf) == vcf_body(g["vcf"]["default"])
    _cli(["-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-alg", alg, "-no_vcf", "-gpu_sam"])  # nothing to do without -sam


@pytest.mark.gpu
@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("name", ["mc", "se"])
def test_cli_gpu_sam_on_two_shards(golden, tmp_path, name, multi):
    g = golden[name]
    sam = str(tmp_path / "o.sam")
    _cli(["-i", g["prefix"], "-f", g["r1"]] + (["-f2", g["r2"]] if g["r2"] else []) + ["-alg", "nw", "-sam", sam, "-no_vcf", "-t", "2", "-devices", "0,0",
         "-batch", "400", "-gpu_sam"] + (["-m"] if multi else []), timeout=1200)
    if multi:
        compare(name, "nw", sam)
    else:
        nd, ex = sam_diff(g["sam"]["nw"], sam, mask_se_reverse_qual=not g["r2"])
        assert nd == 0, ex


@pytest.mark.gpu
def test_run_module_gpu_sam(golden, tmp_path):
    g = golden["var"]
    sam = str(tmp_path / "o.sam")
    cmd = [sys.executable, "-m", "mapcaller_amd.run", "-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-alg", "ksw2", "-sam", sam, "-no_vcf", "-gpu_sam"]
    subprocess.run(cmd, check=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    nd, ex = sam_diff(g["sam"]["ksw2"], sam)
    assert nd == 0, ex
