"""BAM records on the host: mapcaller_amd/csrc/mcx_bam.h compiled for the host (tests/hostemu/bam_check.cpp) against the golden SAM files and against
records assembled here from the rules, plus the surface of -bam (header, bindings, exports, switches).

The reference's -bam hands every SAM line to htslib's sam_parse1 and writes the result with sam_write1, and its vendored htslib is recorded as unbuildable (oracle/Makefile): so the
check is a decoder of the uncompressed BAM stream written in this file from the SAM/BAM specification, held field by field against the golden SAM lines —
refID / pos / mapq / bin (recomputed here) / flag / CIGAR words / mate fields / SEQ through the 4-bit rule / QUAL - 33 or 0xff / NM AS XS with the smallest
integer type.  On the golden sets no line is dropped (no name of 252 bytes, no QUAL of another length than SEQ): records == lines is a condition.  What the
golden sets never reach — odd lengths, long and empty names, cut quality lines, '*' qualities, every tag width, every base code, a CIGAR beyond the kernel's
LDS staging, the mate and bin edge cases, -m extras — is covered by synthetic batches whose expected bytes are packed here with struct, never by the code
under test.  tests/test_bam_device.py takes the same batches through the kernels."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SETS
from test_multi import MULTI_SETS, read_extras
from test_sam_device import COMP, interleave, n_pairs_part, parse_reads, records_of, sam_in, split_golden

NEW = ("mcx_bam_format_dev", "mcx_bam_format", "mcx_bam_header")
ALGS = ("nw", "ksw2")
SEQ_CODES = "=ACMGRSVTWYHKDBN"
KERNEL_STAGE = 2048  # bytes of LDS a wavefront of k_bam_write stages a record in (mcx_bam.hip: kBamStage)


# ---- CPU: the surface ---------------------------------------------------------------------------------------
def test_the_bam_calls_are_declared_bound_and_exported():
    from mapcaller_amd import api, run
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for s in NEW:
        assert s in api.SYMBOLS and re.search(r"\b%s\s*\(" % s, header), s
    for name, value in (("MCX_SAM_BAM", 4), ("MCX_ROUTE_BAM", 32)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
    assert api.SAM_BAM == 4 and api.ROUTE_BAM == 32
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in NEW:
            assert f" {s}\n" in nm, s
        L = api.lib()
        for s in ("mcx_bam_format_dev", "mcx_bam_format"):
            f = getattr(L, s)
            assert f.restype is C.c_int and len(f.argtypes) == 7 and f.argtypes[3] is C.c_uint64 and f.argtypes[2] is C.c_void_p
        assert L.mcx_bam_header.argtypes[2] is C.c_uint64
    assert C.sizeof(api.FileOpts) == 48 and api.FileOpts.device_sam.offset == 12
    assert inspect.signature(api.Mapper.map_files).parameters["bam"].default is False
    assert "bam_records" in dir(api.Mapper) and callable(api.bam_header)
    a = run.parse(["-i", "x", "-f", "a.fq", "-bam", "o.bam"])
    assert a.bam and a.sam == "o.bam" and not run.parse(["-i", "x", "-f", "a.fq", "-sam", "o.sam"]).bam
    a = run.parse(["-i", "x", "-f", "a.fq", "-bam", "o.bam", "-sam", "o.sam"])  # the later of the two decides (reference src/main.cpp:274-285)
    assert not a.bam and a.sam == "o.sam"
    main = open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_main.cpp")).read()
    assert '"-bam"' in main and re.search(r'"\s+-bam\s', main) and "is not supported" not in main  # the switch, its line in usage(), the refusal gone
    assert os.path.exists(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_bam.h")) and "mcx_bam.o" in open(os.path.join(ROOT, "mapcaller_amd", "csrc", "Makefile")).read()


# ---- a BAM decoder, from the specification ---------------------------------------------------------------------------------
def decode_header(data):
    """(header text, [(contig, length)], offset of the first record) of an uncompressed BAM stream"""
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    text = data[8:8 + l_text]
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, at)
    at += 4
    contigs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, at)
        name = data[at + 4:at + 4 + l_name]
        assert name[-1:] == b"\0" and b"\0" not in name[:-1]
        l_ref, = struct.unpack_from("<i", data, at + 4 + l_name)
        contigs.append((name[:-1].decode("latin-1"), l_ref))
        at += 8 + l_name
    return text, contigs, at


TAG_TYPES = {"C": "<B", "c": "<b", "S": "<H", "s": "<h", "I": "<I", "i": "<i"}


def decode_records(data, at=0):
    """every record from `at` to the end of the stream: a dict per record, SEQ as 4-bit codes, QUAL as bytes, tags as (name, type letter, value)"""
    out = []
    while at < len(data):
        block_size, = struct.unpack_from("<i", data, at)
        body = data[at + 4:at + 4 + block_size]
        assert len(body) == block_size >= 32, (at, block_size)
        ref, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, next_ref, next_pos, tlen = struct.unpack_from("<iiBBHHHiiii", body, 0)
        p = 32
        name = body[p:p + l_name]
        assert l_name >= 1 and name[-1:] == b"\0"
        p += l_name
        cigar = list(struct.unpack_from("<%dI" % n_cigar, body, p))
        p += 4 * n_cigar
        packed = body[p:p + (l_seq + 1) // 2]
        seq = [(packed[k >> 1] >> (0 if k & 1 else 4)) & 15 for k in range(l_seq)]
        assert l_seq % 2 == 0 or packed[-1] & 15 == 0  # the unused low nibble
        p += (l_seq + 1) // 2
        qual = body[p:p + l_seq]
        assert len(qual) == l_seq
        p += l_seq
        tags = []
        while p < len(body):
            fmt = TAG_TYPES[chr(body[p + 2])]
            tags.append((body[p:p + 2].decode(), chr(body[p + 2]), struct.unpack_from(fmt, body, p + 3)[0]))
            p += 3 + struct.calcsize(fmt)
        assert p == len(body)
        out.append(dict(ref=ref, pos=pos, mapq=mapq, bin=bin_, flag=flag, l_seq=l_seq, next_ref=next_ref, next_pos=next_pos, tlen=tlen, name=name[:-1], cigar=cigar,
                        seq=seq, qual=qual, tags=tags, size=4 + block_size))
        at += 4 + block_size
    assert at == len(data)
    return out


# ---- the rules, restated (SAM/BAM specification; what htslib 1.5's sam_parse1 does with a line) -----------------------------------------
def seq_code(c):
    """the 4-bit code of a SEQ byte"""
    ch = chr(c).upper() if c < 128 else ""
    if ch and ch in SEQ_CODES:
        return SEQ_CODES.index(ch)
    return {48: 1, 49: 2, 50: 4, 51: 8}.get(c, 15)


def reg2bin(beg, end):
    """the UCSC bin of [beg, end): 14-bit windows at the finest of 5 levels below the root — as the record's 16 bits hold it (beyond 2^29 the scheme has no
    bins: htslib stores what is left of the number, and so does the field)"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return (first + (beg >> shift)) & 0xffff
    return 0


def ref_len(words):
    return sum(w >> 4 for w in words if w & 15 in (0, 2, 3, 7, 8))


def tag_type(v):
    if v >= 0:
        return "C" if v <= 255 else "S" if v <= 65535 else "I"
    return "c" if v >= -128 else "s" if v >= -32768 else "i"


def fields_of_line(line, contigs):
    """what the record of a SAM line must hold, by the rules; None: the line makes no record"""
    f = line.split("\t")
    name, seq, qual = f[0].encode("latin-1"), f[9].encode("latin-1"), f[10].encode("latin-1")
    if len(name) >= 252 or (qual != b"*" and len(qual) != len(seq)):
        return None
    flag, mapped = int(f[1]), f[2] != "*"
    words = [] if f[5] == "*" else [(int(n) << 4) | "MIDNSHP=X".index(c) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", f[5])]
    pos = int(f[3]) - 1
    ref = contigs.index(f[2]) if mapped else -1
    next_pos = int(f[7]) - 1
    next_ref = ref if f[6] == "=" and next_pos >= 0 else -1
    tags = []
    for t in f[11:]:
        v = int(t[5:])
        assert t[2:5] == ":i:"
        tags.append((t[:2], tag_type(v), v))
    return dict(ref=ref, pos=pos, mapq=int(f[4]), bin=reg2bin(pos, pos + (ref_len(words) if mapped and words else 1)), flag=(flag if mapped else flag | 4) & 0xffff,
                l_seq=len(seq), next_ref=next_ref, next_pos=next_pos, tlen=int(f[8]), name=name, cigar=words, seq=[seq_code(c) for c in seq],
                qual=b"\xff" * len(seq) if qual == b"*" else bytes((c - 33) & 255 for c in qual), tags=tags)


def assert_records_are_lines(records, lines, contigs, qual_of=None):
    """record k holds what line k says.  qual_of(k): the QUAL bytes to expect instead of the line's (None: the line's) — the golden files' QUAL of a
    reverse-strand single-end FASTQ read is not the reference's intent (conftest.sam_diff's mask), the read file's quality line reversed is"""
    assert len(records) == len(lines)
    for k, (rec, line) in enumerate(zip(records, lines)):
        want = fields_of_line(line, contigs)
        assert want is not None, line
        if qual_of is not None and qual_of(k) is not None:
            want["qual"] = bytes((c - 33) & 255 for c in qual_of(k))
        for key, v in want.items():
            assert rec[key] == v, (k, key, rec[key], v, line)
        if want["ref"] >= 0 and want["cigar"]:  # the pipeline's invariant: the CIGAR takes the read's bases
            assert sum(w >> 4 for w in want["cigar"] if w & 15 in (0, 1, 4, 7, 8)) == want["l_seq"], line


# ---- the host build ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def bam_check(tmp_path_factory):
    """mcx_bam.h for the host (tests/hostemu/bam_check.cpp)"""
    out = str(tmp_path_factory.mktemp("bam_check") / "libbam_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", os.path.join(ROOT, "tests", "hostemu", "bam_check.cpp"), "-o", out],
                   check=True, stderr=subprocess.PIPE, timeout=600)
    from mapcaller_amd import api
    L = C.CDLL(out)
    L.bam_check_format.restype = C.c_int64
    L.bam_check_format.argtypes = [C.POINTER(api.SamIn), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
    L.bam_check_bin.restype = C.c_uint32
    L.bam_check_bin.argtypes = [C.c_int64, C.c_int64]
    L.bam_check_nibble.restype = C.c_uint32
    L.bam_check_nibble.argtypes = [C.c_uint32]
    return L


def host_encode_in(L, si, n):
    """(bytes, rec_off, dropped) of one mcx_sam_in through the host build: the size alone first, then into a buffer with guard bytes behind exactly that size"""
    rec_off = np.zeros(n + 1, dtype=np.uint64)
    nd = C.c_uint64()
    rc = L.bam_check_format(C.byref(si), None, 0, rec_off.ctypes.data, C.byref(nd))
    total = int(rec_off[-1])
    assert rc == (-1 if total else 0)
    out = np.full(total + 64, 0xA5, dtype=np.uint8)
    nd2 = C.c_uint64()
    assert L.bam_check_format(C.byref(si), out.ctypes.data, total, rec_off.ctypes.data, C.byref(nd2)) == total
    assert (out[total:] == 0xA5).all() and nd2.value == nd.value
    return out[:total].tobytes(), rec_off, int(nd.value)


def golden_parts(reads, n_pair_reads, lines, contigs, extras=None):
    """mcx_sam_in for the pairs' part and the single reads' part of a golden set, rebuilt from the reference's SAM and read files as tests/test_sam_device.py's
    host_format rebuilds them: yields (SamIn, reads of the part, what keeps the arrays alive)"""
    from mapcaller_amd import api
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
        si, _ = sam_in(api, reads[lo:hi], paired, aln, pool, x, keep)
        yield si, hi - lo, keep


def host_encode(L, reads, n_pair_reads, lines, contigs, extras=None):
    """the records of a golden set through the host build: (bytes, dropped)"""
    data, dropped = b"", 0
    for si, n, keep in golden_parts(reads, n_pair_reads, lines, contigs, extras):
        part, _, nd = host_encode_in(L, si, n)
        data += part
        dropped += nd
    return data, dropped


def lines_with_extras(body, extras):
    """(the lines in the file's order, the read each belongs to, whether it is the read's first)"""
    by = {}
    for i, l in extras:
        by.setdefault(i, []).append(l)
    lines, owner, first = [], [], []
    for i, l in enumerate(body):
        for k, x in enumerate([l] + by.get(i, [])):
            lines.append(x)
            owner.append(i)
            first.append(k == 0)
    return lines, owner, first


def check_golden(L, reads, paired, body, contigs, extras=None):
    data, dropped = host_encode(L, reads, n_pairs_part(len(reads), paired), body, contigs, extras)
    lines, owner, first = lines_with_extras(body, extras or [])
    records = decode_records(data)
    assert dropped == 0 and len(records) == len(lines)  # no golden line has a name of 252 bytes or a QUAL of another length than SEQ

    def qual_of(k):
        # the golden files' QUAL of a reverse-strand read mapped single-end from FASTQ is masked by conftest.sam_diff (its first byte is not the reference's
        # intent): there the read file's quality line reversed is what the record must hold.  (The -m lines behind a read's first are compared as they are.)
        flag = lines[k].split("\t")[1]
        q = reads[owner[k]][2]
        return q[::-1] if first[k] and q is not None and (int(flag) & 0x11) == 0x10 else None
    assert_records_are_lines(records, lines, contigs, qual_of)
    assert all(t[1] == "C" for r in records for t in r["tags"])  # every tag value of the golden sets lies in 0..255
    return data


def golden_reads(g):
    reads = parse_reads(g["r1"])
    return interleave(reads, parse_reads(g["r2"])) if g["r2"] else reads


@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("name", list(SETS))
def test_host_build_encodes_the_golden_sam(bam_check, golden, name, alg):
    g = golden[name]
    reads = golden_reads(g)
    _, body, contigs = split_golden(g["sam"][alg])
    assert len(body) == len(reads)
    check_golden(bam_check, reads, SETS[name], body, contigs)
    if name in MULTI_SETS:  # -m: every read's further records behind its first
        check_golden(bam_check, reads, SETS[name], body, contigs, read_extras(name, alg))


def io_case(g, case):
    if case == "il":
        return parse_reads(g["il.fq"]), True
    if case == "ml":
        return parse_reads(g["ml.fa"]), False
    if case == "gz":
        return interleave(parse_reads(g["gz1"], gz=True), parse_reads(g["gz2"], gz=True)), True
    return interleave(parse_reads(g["a1"]) + parse_reads(g["b1"]), parse_reads(g["a2"]) + parse_reads(g["b2"])), True


@pytest.mark.parametrize("case", ["il", "ml", "gz", "lib"])
def test_host_build_encodes_the_input_side_cases(bam_check, io_golden, case):
    reads, paired = io_case(io_golden, case)
    _, body, contigs = split_golden(io_golden[f"ref.{case}.sam"])
    assert len(body) == len(reads)
    check_golden(bam_check, reads, paired, body, contigs)


def expected_header(head_lines, contig_lengths):
    text = ("\n".join(head_lines) + "\n").encode("latin-1")
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(contig_lengths))
    for name, length in contig_lengths:
        out += struct.pack("<i", len(name) + 1) + name.encode("latin-1") + b"\0" + struct.pack("<i", length)
    return out


def sq_lines(head):
    return [(l.split("\t")[1][3:], int(l.split("\t")[2][3:])) for l in head if l.startswith("@SQ")]


def test_the_header_bytes_decode_to_the_golden_header(golden):
    """the stream's header as the rules give it for a golden set's @PG / @SQ lines decodes to them again (the library's own bytes: tests/test_bam_device.py)"""
    head, _, contigs = split_golden(golden["mc"]["sam"]["nw"])
    blob = expected_header(head, sq_lines(head))
    text, got, at = decode_header(blob)
    assert text.decode("latin-1").split("\n")[:-1] == head and [c for c, _ in got] == contigs and at == len(blob)


# ---- synthetic batches: what the golden sets never reach ---------------------------------------------------------------------------
def turned(seq, qual_buf, paired, r, rec):
    """(SEQ, QUAL) of the SAM line of read r, by mcx_sam.h's rules restated: mate 2 is held reverse-complemented; a reverse-strand hit turns again"""
    flipped = paired and r % 2 == 1
    again = rec["chr"] >= 0 and rec["fwd"] == 0
    if flipped != again:
        s = seq.translate(COMP)[::-1]
    else:
        s = seq.translate(COMP).translate(COMP) if flipped and again else seq
    if qual_buf is None:
        return s, b"*"
    q = qual_buf if flipped == again else qual_buf[::-1]
    return s, q.split(b"\0")[0]


def pack_tag(name, v):
    t = tag_type(v)
    return name + t.encode() + struct.pack(TAG_TYPES[t], v)


def pack_record(name, seq_line, qual_line, rec, words):
    """the record of one line, by the rules of the issue; b"" when the line makes none"""
    if len(name) >= 252 or (qual_line != b"*" and len(qual_line) != len(seq_line)):
        return b""
    mapped = rec["chr"] >= 0
    words = words if mapped else []
    pos0 = rec["pos"] - 1 if mapped else -1
    mate = mapped and rec["has_mate"] and rec["mate_pos"] >= 1
    body = struct.pack("<iiBBHHHiiii", rec["chr"] if mapped else -1, pos0, len(name) + 1, rec["mapq"] if mapped else 0,
                       reg2bin(pos0, pos0 + (ref_len(words) if mapped and words else 1)), len(words), (rec["flag"] if mapped else rec["flag"] | 4) & 0xffff, len(seq_line),
                       rec["chr"] if mate else -1, rec["mate_pos"] - 1 if mate else -1, rec["tlen"] if mate else 0)
    body += name + b"\0" + struct.pack("<%dI" % len(words), *words)
    codes = [seq_code(c) for c in seq_line] + [0]
    body += bytes(codes[k] << 4 | codes[k + 1] for k in range(0, len(seq_line), 2))
    body += b"\xff" * len(seq_line) if qual_line == b"*" else bytes((c - 33) & 255 for c in qual_line)
    if mapped:
        body += pack_tag(b"NM", rec["nm"]) + pack_tag(b"AS", rec["as"]) + pack_tag(b"XS", rec["xs"])
    else:
        body += pack_tag(b"AS", 0) + pack_tag(b"XS", 0)
    return struct.pack("<i", len(body)) + body


PALETTE = b"ACGTacgtNnRYKMSWBDHVrykmswbdhv=0123\x80\xffXx.*-"


def synthetic_batches():
    """[dict(name, reads, paired, aln, pool, extras, want: the expected bytes per read, dropped)] — the first with qualities and pairs, the second
    without qualities (qual == NULL) and single-end"""
    from mapcaller_amd import api
    rng = np.random.default_rng(20260119)
    batches = []
    for paired, with_qual in ((True, True), (False, False)):
        reads, recs, cigars, extras = [], [], [], {}  # extras: read -> [(rec, words)]

        def rec_of(**kw):
            r = dict(pos=1000, mate_pos=1200, chr=0, flag=99, mapq=60, tlen=350, nm=1, xs=0, n_cigar=0, fwd=1, has_mate=1)
            r["as"] = 140
            r.update(kw)
            return r

        def add(name, seq, qual, rec, words=None):
            if rec["chr"] >= 0 and words is None:
                words = [len(seq) << 4]
            reads.append((name, seq, qual if with_qual else None))
            recs.append(rec)
            cigars.append(words or [])

        def bases(n):
            return bytes(rng.choice(np.frombuffer(PALETTE, dtype=np.uint8), n))

        def quals(n):
            return bytes(rng.integers(33, 127, n).astype(np.uint8))

        # every length round the wavefront's strides, in each of the four turn cases (mate 1 / mate 2 x forward / reverse), bases of every kind
        for rlen in (1, 2, 63, 64, 65, 127, 128, 129):
            for fwd in (1, 1, 0, 0):  # (two reads a pair: both strands for both mates)
                add(b"len%d_%d" % (rlen, len(reads)), bases(rlen), quals(rlen), rec_of(fwd=fwd, flag=83 if not fwd else 99, pos=int(rng.integers(1, 1 << 28))))
        seq = PALETTE + PALETTE[::-1]
        for fwd in (1, 1, 0, 0):
            add(b"palette%d" % len(reads), seq, quals(len(seq)), rec_of(fwd=fwd))
        # names: empty, one byte, the longest kept, the shortest dropped
        for n in (0, 1, 251, 252):
            add(b"n" * n, bases(30), quals(30), rec_of())
        # QUAL shorter than SEQ in both printing directions (dropped), empty (dropped), exactly '*' (kept, 0xff), '*' in front of NULs printed backwards (dropped)
        for fwd in (1, 1, 0, 0):
            add(b"shortq%d" % len(reads), bases(40), quals(17), rec_of(fwd=fwd))
        for fwd in (1, 1, 0, 0):
            add(b"noq%d" % len(reads), bases(12), b"", rec_of(fwd=fwd))
        for fwd in (1, 1, 0, 0):
            add(b"star%d" % len(reads), bases(5), b"*", rec_of(fwd=fwd))
        add(b"star_one_a", bases(1), b"*", rec_of())
        add(b"star_one_b", bases(1), b"*", rec_of(fwd=0))
        # every tag width on both sides of its edge
        edge = (255, 256, 65535, 65536, -1, -128, -129, -32768, -32769, 0, 2147483647, -2147483648)
        for k in range(len(edge)):
            add(b"tag%d" % k, bases(20), quals(20), rec_of(nm=edge[k], xs=edge[(k + 1) % len(edge)], **{"as": edge[(k + 5) % len(edge)]}))
        # 300 CIGAR operations: beyond the kernel's staging
        words = []
        for _ in range(150):
            words += [3 << 4, 1 << 4 | 1]
        add(b"long_cigar_a", bases(600), quals(600), rec_of(), words)
        add(b"long_cigar_b", bases(600), quals(600), rec_of(fwd=0, flag=147), words)
        # mate fields: a mate at position 0, a negative TLEN, no mate
        add(b"mate0", bases(25), quals(25), rec_of(mate_pos=0, tlen=77))
        add(b"mate_neg", bases(25), quals(25), rec_of(tlen=-412, fwd=0, flag=147))
        add(b"no_mate", bases(25), quals(25), rec_of(has_mate=0, tlen=0, mate_pos=0, flag=73))
        add(b"unmapped", bases(25), quals(25), rec_of(chr=-1, pos=0, flag=77, mapq=0, has_mate=0))
        # bins: both sides of a 16 Kbp and a 128 Kbp boundary, alignments across them (with D, N, I, S in the sum), a second contig
        for pos0, w in ((16383, [10 << 4]), (16384, [10 << 4]), (16380, [10 << 4]), (131071, [10 << 4]), (131072, [10 << 4]), (131070, [10 << 4]),
                        (16370, [2 << 4 | 4, 4 << 4, 9 << 4 | 2, 4 << 4]), (16370, [4 << 4, 1 << 4 | 1, 5 << 4]), (1 << 20, [5 << 4, (1 << 20) << 4 | 3, 5 << 4]),
                        ((1 << 23) - 3, [10 << 4]), ((1 << 26) - 3, [10 << 4]), ((1 << 29) - 5, [10 << 4]), (0, [10 << 4 | 7])):
            add(b"bin%d" % len(reads), bases(10), quals(10), rec_of(pos=pos0 + 1, chr=len(reads) % 2), w)
        if len(reads) % 2:
            add(b"even", bases(10), quals(10), rec_of())
        # -m: a read with three further lines, one of them flagged unmapped; a read with one; most with none
        multi_at = 4
        extras[multi_at] = [(rec_of(pos=5000, fwd=0, flag=83, nm=300), [reads[multi_at][1].__len__() << 4]), (rec_of(chr=-1, pos=0, flag=77), []),
                            (rec_of(pos=70000, chr=1, xs=-5), [1 << 4 | 4, (len(reads[multi_at][1]) - 1) << 4])]
        extras[9] = [(rec_of(pos=123456, fwd=1), [len(reads[9][1]) << 4])]
        n = len(reads)
        aln = np.zeros(n, dtype=api.ALN_DTYPE)
        pool = []
        for r in range(n):
            for k, v in recs[r].items():
                aln[r][k] = v
            aln[r]["n_cigar"], aln[r]["cigar_off"] = len(cigars[r]), len(pool)
            pool += cigars[r]
        n_x = sum(len(v) for v in extras.values())
        index, x_aln, x_pool = np.zeros(n + 1, dtype=np.uint32), np.zeros(n_x, dtype=api.ALN_DTYPE), []
        i = 0
        for r in range(n):
            index[r] = i
            for rec, w in extras.get(r, []):
                for k, v in rec.items():
                    x_aln[i][k] = v
                x_aln[i]["n_cigar"], x_aln[i]["cigar_off"] = len(w), len(x_pool)
                x_pool += w
                i += 1
        index[n] = i
        want, dropped = [], 0
        for r, (name, seq, qual) in enumerate(reads):
            qbuf = None if qual is None else qual[:len(seq)] + b"\0" * (len(seq) - len(qual))
            mine = b""
            for rec, w in [(recs[r], cigars[r])] + extras.get(r, []):
                one = pack_record(name, *turned(seq, qbuf, paired, r, rec), rec, w)
                dropped += not one
                mine += one
            want.append(mine)
        batches.append(dict(name="pairs+qual" if paired else "single,no-qual", reads=reads, paired=paired, aln=aln, pool=np.array(pool + [0], dtype=np.uint32),
                            extras=(index, x_aln, np.array(x_pool + [0], dtype=np.uint32)), want=want, dropped=dropped))
    return batches


@pytest.fixture(scope="session")
def synthetic():
    return synthetic_batches()


def test_the_synthetic_batches_reach_what_they_are_for(synthetic):
    a = synthetic[0]
    sizes = [len(w) for w in a["want"]]
    assert max(sizes) > KERNEL_STAGE and a["dropped"] >= 10 and synthetic[1]["dropped"] == 1  # (without qualities only the 252-byte name is dropped)
    letters = {t[1] for w in a["want"] for r in decode_records(w) for t in r["tags"]}
    assert letters == set("CcSsIi")
    assert {r["bin"] for w in a["want"] for r in decode_records(w)} >= {4680, 4681, 4682, 585, 4681 + 7, 4681 + 8, 73, 9, 1, 0}
    assert len(decode_records(a["want"][4])) == 4 and sum(1 for w in a["want"] if not w) >= 8


def test_host_build_equals_the_hand_packed_records(bam_check, synthetic):
    from mapcaller_amd import api
    for b in synthetic:
        for extras in (None, b["extras"]):
            keep = []
            si, _ = sam_in(api, b["reads"], b["paired"], b["aln"], b["pool"], extras, keep)
            data, rec_off, dropped = host_encode_in(bam_check, si, len(b["reads"]))
            want = b["want"] if extras is not None else [w[:decode_records(w)[0]["size"]] if w else w for w in b["want"]]
            for r, w in enumerate(want):
                got = data[int(rec_off[r]):int(rec_off[r + 1])]
                assert got == w, (b["name"], r, b["reads"][r][0][:20], got[:48].hex(), w[:48].hex())
            assert data == b"".join(want)
            if extras is not None:
                assert dropped == b["dropped"]


def test_bins_and_base_codes_one_by_one(bam_check):
    for c in range(256):
        assert bam_check.bam_check_nibble(c) == seq_code(c), c
    assert [seq_code(c) for c in b"=ACMGRSVTWYHKDBN"] == list(range(16)) and seq_code(ord("u")) == 15 and seq_code(ord("3")) == 8
    rng = np.random.default_rng(7)
    edges = [s * k + d for s in (1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26, 1 << 29) for k in (0, 1, 2, 3, 7) for d in (-2, -1, 0, 1)]
    for beg in edges + [int(v) for v in rng.integers(0, 1 << 31, 200)]:
        for length in (0, 1, 2, 150, 1 << 14, (1 << 17) + 1, 1 << 27):
            if beg >= -1 and beg + length < 1 << 32:
                assert bam_check.bam_check_bin(beg, beg + length) == reg2bin(beg, beg + length), (beg, length)
    assert reg2bin(-1, 0) == 4680 and reg2bin(0, 1) == 4681 and reg2bin(16383, 16385) == 585


def dump_batch(path, b, with_extras=True):
    """one synthetic batch as tests/hostemu/bam_check.cpp's stand-alone program reads it (every array at exactly its size)"""
    n = len(b["reads"])
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(r[1]) for r in b["reads"]])
    name_off = np.zeros(n + 1, dtype=np.uint32)
    name_off[1:] = np.cumsum([len(r[0]) for r in b["reads"]])
    has_qual = b["reads"][0][2] is not None
    qual = b"".join(r[2][:len(r[1])] + b"\0" * (len(r[1]) - len(r[2])) for r in b["reads"]) if has_qual else b""
    index, x_aln, x_pool = b["extras"]
    pool = b["pool"][:-1]
    x_pool = x_pool[:-1]
    head = np.array([n, int(b["paired"]), int(has_qual), int(off[-1]), int(name_off[-1]), len(pool), len(x_aln) if with_extras else 0xFFFFFFFFFFFFFFFF, len(x_pool)], dtype=np.uint64)
    with open(path, "wb") as f:
        for part in (head, off, name_off, b"".join(r[1] for r in b["reads"]), qual, b"".join(r[0] for r in b["reads"]), b["aln"], pool):
            f.write(part if isinstance(part, bytes) else part.tobytes())
        if with_extras:
            for part in (index, x_aln, x_pool):
                f.write(part.tobytes())


def test_the_standalone_program_gives_the_same_bytes(tmp_path, synthetic):
    """tests/hostemu/bam_check.cpp with its own main (the form a sanitizer build takes), built plainly here"""
    exe = str(tmp_path / "bam_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DBAM_CHECK_MAIN", "-Wall", "-Wno-unused-function", os.path.join(ROOT, "tests", "hostemu", "bam_check.cpp"), "-o", exe],
                   check=True, stderr=subprocess.PIPE, timeout=600)
    for k, b in enumerate(synthetic):
        src, dst = str(tmp_path / f"b{k}.bin"), str(tmp_path / f"o{k}.bin")
        dump_batch(src, b)
        r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 0, r.stderr
        assert open(dst, "rb").read() == b"".join(b["want"])
        assert r.stdout.split()[-3] == b"%d" % b["dropped"]
