"""MD:Z strings (include/mcx.h at mcx_md_dev): the definition restated in plain Python, and mapcaller_amd/csrc/mcx_md.h compiled for the host held against it.

The yardstick, py_md, works from a SAM line's POS, CIGAR and SEQ and the genome's FASTA — nothing of the code under test — and has an inverse: the reference
span rebuilt from SEQ, CIGAR and MD is the FASTA's slice.  CPU only: every mapped line of every golden SAM (both algorithms, the -m lines), the SAM text with
the tags appended, and hand-made records at the edges of the kernel's 64-column rounds, of the contigs, of the .pac bytes and of the ambiguity holes.
tests/test_md_device.py runs the same inputs through the kernels."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT, SETS
from test_bam_host import golden_parts, golden_reads
from test_multi import MULTI_SETS, read_extras
from test_sam_device import ALGS, COMP, check_text, interleave, n_pairs_part, parse_reads, split_golden

NEW = ("mcx_md_dev", "mcx_md", "mcx_md_last_ms")
MD_TAG = re.compile(r"\tMD:Z:[^\t\n]*")


# ---- the definition, restated -----------------------------------------------------------------------------------------------
def nibble(c):
    """BAM's 4-bit code of a base letter, case ignored; 15 for anything else"""
    k = "=ACMGRSVTWYHKDBN".find(c.upper())
    return k if k >= 0 else 15


def cigar_ops(text):
    return [(int(n), c) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def py_md(pos, ops, seq, contig):
    """the MD string of a line: pos 1-based, ops [(length, letter)], seq the printed SEQ, contig the contig's FASTA letters in upper case"""
    out, u, x, y = [], 0, pos - 1, 0
    for n, op in ops:
        if op in "M=X":
            for j in range(n):
                ref = contig[x + j] if 0 <= x + j < len(contig) else "N"
                a = nibble(seq[y + j]) if y + j < len(seq) else 15
                if a != 15 and a == nibble(ref):
                    u += 1
                else:
                    out.append(f"{u}{ref}")
                    u = 0
            x += n
            y += n
        elif op == "D":
            out.append(f"{u}^" + "".join(contig[x + j] if 0 <= x + j < len(contig) else "N" for j in range(n)))
            u = 0
            x += n
        elif op in "IS":
            y += n
        elif op == "N":
            x += n
    return "".join(out) + str(u)


def py_ref_from_md(ops, seq, md):
    """the inverse: the reference letters under the line's M, =, X and D columns, from SEQ, CIGAR and MD alone"""
    tokens = re.findall(r"(\d+)|(\^[A-Z]+)|([A-Z])", md)
    assert "".join(a or b or c for a, b, c in tokens) == md, md
    stream = []  # per column of MD: None (a match: the read's letter) or the reference letter
    for num, dele, mis in tokens:
        if num:
            stream += [None] * int(num)
        elif dele:
            stream += [("D", c) for c in dele[1:]]
        else:
            stream.append(("X", mis))
    out, y, k = [], 0, 0
    for n, op in ops:
        if op in "M=X":
            for j in range(n):
                t = stream[k]
                k += 1
                assert t is None or t[0] == "X", (md, k)
                out.append(seq[y + j].upper() if t is None else t[1])
            y += n
        elif op == "D":
            for j in range(n):
                t = stream[k]
                k += 1
                assert t is not None and t[0] == "D", (md, k)
                out.append(t[1])
        elif op in "IS":
            y += n
    assert k == len(stream), md
    return "".join(out)


def ref_span(pos, ops, contig):
    """the FASTA's letters under the same columns"""
    out, x = [], pos - 1
    for n, op in ops:
        if op in "M=XD":
            out.append(contig[x:x + n])
        if op in "M=XDN":
            x += n
    return "".join(out)


def load_fasta(path):
    """[(name, letters in upper case)] of a (gzipped) FASTA file"""
    data = (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")).read().decode("latin-1")
    out = []
    for block in data.split(">")[1:]:
        lines = block.split("\n")
        out.append((lines[0].split()[0], "".join(lines[1:]).replace("\r", "").upper()))
    return out


def md_of_line(line, genome):
    """py_md of a SAM line (None: unmapped or no CIGAR), with the inverse checked on the way"""
    f = line.split("\t")
    if f[2] == "*" or f[5] == "*":
        return None
    contig = genome[f[2]]
    ops = cigar_ops(f[5])
    md = py_md(int(f[3]), ops, f[9], contig)
    assert py_ref_from_md(ops, f[9], md) == ref_span(int(f[3]), ops, contig), line
    return md.encode()


# ---- the genome as the code under test takes it ------------------------------------------------------------------------------------
def ref_arrays(pac, G, lens, holes):
    """what md_check_strings takes: holes [(offset, length, letter)] sorted by offset"""
    chr_fwd = np.zeros(len(lens) + 1, dtype=np.int64)
    chr_fwd[1:] = np.cumsum(lens)
    return dict(pac=np.frombuffer(bytes(pac) + b"\0" * 32, dtype=np.uint8).copy(), G=G, chr_fwd=chr_fwd,
                hole_off=np.array([h[0] for h in holes] + [0], dtype=np.int64), hole_len=np.array([h[1] for h in holes] + [0], dtype=np.int32),
                hole_letter=np.frombuffer(b"".join(h[2].encode() for h in holes) + b"\0", dtype=np.uint8).copy(), n_holes=len(holes))


def index_ref(prefix):
    """... of index files: .ann (sizes), .pac (two bits a base), .amb (lines of offset, length, letter)"""
    ann = open(prefix + ".ann").read().split("\n")
    G, n_seqs = int(ann[0].split()[0]), int(ann[0].split()[1])
    lens = [int(ann[2 + 2 * i].split()[1]) for i in range(n_seqs)]
    amb = [l.split() for l in open(prefix + ".amb").read().split("\n")[1:] if l.strip()]
    holes = sorted((int(a), int(b), c) for a, b, c in amb)
    return ref_arrays(open(prefix + ".pac", "rb").read(), G, lens, holes)


def pack_ref(seqs):
    """... of contig strings, packed here: a base that is not ACGT gets some base in the .pac (the packer's are random) and joins the hole of the same letter before it"""
    codes, holes, lens = [], [], []
    for s in seqs:
        last = ""
        for i, ch in enumerate(s):
            k = "ACGT".find(ch.upper())
            if k < 0:
                if last == ch:
                    holes[-1][1] += 1
                else:
                    holes.append([len(codes), 1, ch])
                k = (len(codes) * 7 + 1) & 3
            last = ch
            codes.append(k)
        lens.append(len(s))
    pac = bytearray(len(codes) // 4 + 2)
    for i, k in enumerate(codes):
        pac[i >> 2] |= k << ((~i & 3) << 1)
    return ref_arrays(pac, len(codes), lens, [tuple(h) for h in holes])


@pytest.fixture(scope="session")
def md_check(tmp_path_factory):
    """mcx_md.h, mcx_sam.h and mcx_bam.h for the host (tests/hostemu/md_check.cpp)"""
    out = str(tmp_path_factory.mktemp("md_check") / "libmd_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", os.path.join(ROOT, "tests", "hostemu", "md_check.cpp"), "-o", out],
                   check=True, stderr=subprocess.PIPE, timeout=600)
    from mapcaller_amd import api
    L = C.CDLL(out)
    L.md_check_strings.restype = C.c_int64
    L.md_check_strings.argtypes = [C.POINTER(api.SamIn), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.md_check_sam.restype = C.c_int64
    L.md_check_sam.argtypes = [C.POINTER(api.SamIn), C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.md_check_bam.restype = C.c_int64
    L.md_check_bam.argtypes = [C.POINTER(api.SamIn), C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def n_lines_of(si):
    n_x = int(np.ctypeslib.as_array(C.cast(si.x_index, C.POINTER(C.c_uint32)), shape=(si.n_reads + 1,))[-1]) if si.x_index and si.n_reads else 0
    return si.n_reads + n_x


def host_md(L, si, ref, keep):
    """(the strings' pool, md_off) of one mcx_sam_in through the host build: the size alone first, then into a buffer with guard bytes behind exactly that size"""
    n = n_lines_of(si)
    md_off = np.zeros(n + 1, dtype=np.uint32)
    args = (ref["pac"].ctypes.data, ref["G"], ref["chr_fwd"].ctypes.data, ref["hole_off"].ctypes.data, ref["hole_len"].ctypes.data, ref["hole_letter"].ctypes.data, ref["n_holes"])
    rc = L.md_check_strings(C.byref(si), *args, None, 0, md_off.ctypes.data)
    total = int(md_off[-1])
    assert rc == (-1 if total else 0)
    out = np.full(total + 64, 0xA5, dtype=np.uint8)
    assert L.md_check_strings(C.byref(si), *args, out.ctypes.data, total, md_off.ctypes.data) == total
    assert (out[total:] == 0xA5).all() and md_off[0] == 0 and (np.diff(md_off.astype(np.int64)) >= 0).all()
    keep += [out, md_off]
    return out, md_off


def strings_of(pool, md_off):
    buf = pool.tobytes()
    return [buf[int(a):int(b)] if b > a else None for a, b in zip(md_off[:-1], md_off[1:])]


def part_lines(n_reads, n_pair_reads, body, extras):
    """the lines behind the entries of each part's pool, as golden_parts cuts a set: the part's own lines, then its extras in their order"""
    for lo, hi in ((0, n_pair_reads), (n_pair_reads, n_reads)):
        if hi > lo:
            yield body[lo:hi] + [l for i, l in (extras or []) if lo <= i < hi]


def host_sam_with_md(L, si, contigs, keep):
    cn_text = "".join(contigs).encode()
    cn_off = np.zeros(len(contigs) + 1, dtype=np.uint32)
    cn_off[1:] = np.cumsum([len(c) for c in contigs])
    line_off = np.zeros(si.n_reads + 1, dtype=np.uint64)
    assert L.md_check_sam(C.byref(si), cn_text, cn_off.ctypes.data, None, 0, line_off.ctypes.data) == -1
    total = int(line_off[-1])
    out = np.full(total + 64, 0xA5, dtype=np.uint8)
    assert L.md_check_sam(C.byref(si), cn_text, cn_off.ctypes.data, out.ctypes.data, total, line_off.ctypes.data) == total
    assert (out[total:] == 0xA5).all()
    return out[:total].tobytes()


def golden_cases():
    """(id, directory, read files, SAM file, paired, extras or None) of every golden set with a genome: both algorithms, the -m sets twice"""
    out = []
    for name, paired in SETS.items():
        d = os.path.join(GOLD, name)
        r1 = [f for f in sorted(os.listdir(d)) if f.startswith("r1.")][0]
        r2 = r1.replace("r1.", "r2.") if paired else None
        for alg in ALGS:
            out.append((f"{name}-{alg}", d, r1, r2, f"ref.{alg}.sam.gz", paired, None))
            if name in MULTI_SETS:
                out.append((f"{name}-{alg}-m", d, r1, r2, f"ref.{alg}.sam.gz", paired, (name, alg)))
    d = os.path.join(GOLD, "opt")
    for lib, r1, r2 in (("pe150", "pe150.r1.fq.gz", "pe150.r2.fq.gz"), ("pe250", "pe250.r1.fq.gz", "pe250.r2.fq.gz"), ("se", "se.r1.fa.gz", None)):
        for alg in ALGS:
            out.append((f"opt-{lib}-{alg}", d, r1, r2, f"{lib}.{alg}.default.sam.gz", r2 is not None, None))
    return out


GOLDEN_CASES = golden_cases()


def load_case(case, tmp_path):
    """(reads, body lines, contig names, extras, paired, index prefix, genome) of a golden case, its files unpacked into tmp_path"""
    _, d, r1, r2, sam, paired, multi = case
    paths = []
    for fn in (r1, r2, sam):
        if fn:
            p = tmp_path / fn[:-3]
            p.write_bytes(gzip.open(os.path.join(d, fn), "rb").read())
            paths.append(str(p))
        else:
            paths.append(None)
    reads = parse_reads(paths[0])
    if paths[1]:
        reads = interleave(reads, parse_reads(paths[1]))
    _, body, contigs = split_golden(paths[2])
    assert len(body) == len(reads)
    extras = read_extras(*multi) if multi else None
    return reads, body, contigs, extras, paired, os.path.join(d, "idx"), dict(load_fasta(os.path.join(d, "genome.fa.gz")))


# ---- CPU: the surface ---------------------------------------------------------------------------------------------------------------
def test_the_md_calls_are_declared_and_bound():
    import inspect
    from mapcaller_amd import api, run
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for s in NEW:
        assert s in api.SYMBOLS and re.search(r"\b%s\s*\(" % s, header), s
    assert re.search(r"MCX_SAM_MD\s*=\s*64\b", header) and api.SAM_MD == 64
    names = [f[0] for f in api.SamIn._fields_]
    assert names[-4:] == ["n_reads", "paired", "md", "md_off"] and api.SamIn.md.offset == 88 and C.sizeof(api.SamIn) == 104
    for f in ("sam_text", "bam_records"):
        assert inspect.signature(getattr(api.Mapper, f)).parameters["md"].default is False
    assert inspect.signature(api.Mapper.map_files).parameters["md"].default is False and callable(api.Mapper.md_strings)
    assert run.parse(["-i", "x", "-f", "a.fq", "-sam", "o.sam", "-md"]).md and not run.parse(["-i", "x", "-f", "a.fq"]).md
    assert '"-md"' in open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_main.cpp")).read()
    if os.path.exists(api.LIB_PATH):
        L = api.lib()
        for s in ("mcx_md_dev", "mcx_md"):
            f = getattr(L, s)
            assert f.restype is C.c_int and f.argtypes[3] is C.c_uint64 and f.argtypes[2] is C.c_void_p and len(f.argtypes) == 6


def test_the_restatement_on_strings_written_out():
    ref = "ACGTACGTACGT"
    assert py_md(1, [(12, "M")], "ACGTACGTACGT", ref) == "12"
    assert py_md(1, [(4, "M")], "TCGA", ref) == "0A2T0"             # a mismatch in the first column and in the last
    assert py_md(1, [(4, "M")], "CATG", ref) == "0A0C0G0T0"         # adjacent mismatches
    assert py_md(1, [(2, "M"), (2, "D"), (2, "M")], "ACTC", ref) == "2^GT0A1"  # a mismatch directly behind a deletion
    assert py_md(2, [(2, "S"), (3, "M"), (2, "I"), (3, "M"), (1, "S")], "NNCGTTTACGN", ref) == "6"  # I and S do not end a run
    assert py_md(1, [(2, "M"), (4, "N"), (2, "M"), (3, "H"), (1, "P")], "ACGA", ref) == "3T0"  # N skips reference without text; H and P do nothing
    assert py_md(1, [(3, "M")], "aNg", "ANG") == "1N1"              # case is ignored; a read N never matches, not even a reference N


# ---- CPU: the host build on the golden sets ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_host_build_gives_the_python_md_on_the_golden_sam(md_check, tmp_path, case):
    reads, body, contigs, extras, paired, prefix, genome = load_case(case, tmp_path)
    ref = index_ref(prefix)
    n_pr = n_pairs_part(len(reads), paired)
    text, n_tags = b"", 0
    for (si, n, keep), lines in zip(golden_parts(reads, n_pr, body, contigs, extras), part_lines(len(reads), n_pr, body, extras)):
        pool, md_off = host_md(md_check, si, ref, keep)
        got = strings_of(pool, md_off)
        want = [md_of_line(l, genome) for l in lines]
        assert len(got) == len(lines)
        bad = [(l, g, w) for l, g, w in zip(lines, got, want) if g != w]
        assert not bad, bad[:3]
        n_tags += sum(w is not None for w in want)
        si.md, si.md_off = pool.ctypes.data, md_off.ctypes.data
        text += host_sam_with_md(md_check, si, contigs, keep)
    assert n_tags == sum(l.split("\t")[5] != "*" for ls in part_lines(len(reads), n_pr, body, extras) for l in ls) > 0  # a tag on every mapped line, on no other
    assert len(MD_TAG.findall(text.decode("latin-1"))) == n_tags
    # the text with the tags taken out again is the golden SAM (the -m lines: each read's extras right behind its first line)
    by = {}
    for i, l in extras or []:
        by.setdefault(i, []).append(l)
    want_lines = [x for i, l in enumerate(body) for x in [l] + by.get(i, [])]
    stripped = MD_TAG.sub("", text.decode("latin-1")).encode("latin-1")
    if extras:  # (the reference leaves FLAG of a single-end read's -m lines unset: tests/test_multi.py masks it on both sides)
        from test_multi import mask_se_extra_flags
        stripped = mask_se_extra_flags(stripped.decode("latin-1"), paired)[0].encode("latin-1")
        want_lines = [l for l in mask_se_extra_flags("\n".join(want_lines) + "\n", paired)[0].split("\n") if l]
    check_text(tmp_path, stripped, want_lines, masked=not paired)


# ---- hand-made records -----------------------------------------------------------------------------------------------------------------
def hand_genome():
    """two contigs with ambiguity holes: a run of N, a run of R (a letter other than N), a lone lower-case n; contig 0 is 1203 long, so contig 1 starts at g & 3 = 3"""
    rng = np.random.default_rng(20261021)
    a = "".join("ACGT"[k] for k in rng.integers(0, 4, 1203))
    b = "".join("ACGT"[k] for k in rng.integers(0, 4, 2100))
    a = a[:300] + "N" * 30 + a[330:500] + "RRR" + a[503:700] + "n" + a[701:]
    return [("hA", a), ("hB", b)]


def turn(raw, mate2, fwd):
    """the printed SEQ of a mapped read (mcx_sam.h): mate 2 was reverse-complemented before mapping, a reverse-strand hit is turned once more"""
    again = not fwd
    if mate2 != again:
        return raw.translate(COMP)[::-1]
    return raw.translate(COMP).translate(COMP) if mate2 and again else raw


def hand_cases(genome):
    """[(contig index, pos, ops, raw read bytes, mate2, fwd)]; contig index -1: unmapped"""
    rng = np.random.default_rng(7)
    up = [s.upper() for _, s in genome]
    cases = []

    def add(chrom, pos, cigar, mism=(), mate2=False, fwd=True, patch=None):
        ops = cigar_ops(cigar)
        seq, x = [], pos - 1
        for n, op in ops:
            if op in "M=X":
                seq += [c if c in "ACGT" else "A" for c in up[chrom][x:x + n]]
            elif op in "IS":
                seq += ["ACGT"[k] for k in rng.integers(0, 4, n)]
            if op in "M=XDN":
                x += n
        assert x <= len(up[chrom]), (cigar, pos)
        for k in (range(len(seq)) if mism == "all" else mism):
            seq[k] = "ACGT"[("ACGT".index(seq[k]) + 1 + k % 3) % 4]
        printed = "".join(seq)
        if patch:
            printed = patch(printed)
        raw = printed.encode()
        if mate2 != (not fwd):  # stored so that the printed SEQ is the one made here
            raw = raw.translate(COMP)[::-1]
        assert turn(raw, mate2, fwd) == printed.upper().encode() or not (mate2 or not fwd)
        cases.append((chrom, pos, ops, raw, mate2, fwd))

    for n in (1, 63, 64, 65, 128, 129, 1000):  # the lengths around the 64-column rounds: all match, all mismatch
        add(1, 11, f"{n}M")
        add(1, 12, f"{n}M", mism="all")
    add(1, 100, "150M", mism=(0,))
    add(1, 100, "150M", mism=(149,))
    add(1, 100, "150M", mism=(0, 1, 63, 64, 65, 149))
    add(1, 200, "60M4D50M")      # a deletion that ends at column 63
    add(1, 200, "64M3D40M")      # ... starts at column 64
    add(1, 200, "62M4D40M")      # ... straddles 63 / 64
    add(1, 300, "30M100D30M")    # a 100-base deletion: two rounds of deleted columns
    add(1, 300, "20M3I2D20M")    # I next to D, both ways
    add(1, 300, "20M2D3I20M")
    add(1, 300, "10M2D2D10M")    # two deletions side by side: "^xx0^yy"
    add(1, 400, "5S40M7S", mism=(5, 44))
    add(1, 400, "10M2D10M", mism=(10,))  # "^AC0T"
    add(1, 500, "50M", patch=lambda s: s[:3] + "N" + s[4:10] + s[10:20].lower() + s[20:30] + "ACGT"[("ACGT".index(s[30]) + 1) % 4].lower() + s[31:])
    for mate2 in (False, True):  # the four turns of SEQ
        for fwd in (True, False):
            add(1, 600, "40M2I30M1D28M", mism=(3, 50, 99), mate2=mate2, fwd=fwd)
    for chrom in (0, 1):  # POS 1 and the contig's last base; g0 & 3 = 0 .. 3 on both contigs
        add(chrom, 1, "70M", mism=(0,))
        add(chrom, len(up[chrom]) - 69, "70M", mism=(69,))
        for pos in (1, 2, 3, 4, 5):
            add(chrom, pos, "67M", mism=(1, 66))
    cases.append((-1, 0, [], b"ACGTNACGT", False, True))  # unmapped lines get no tag
    cases.append((1, 50, [], b"ACGT", False, True))       # ... nor does a line without a CIGAR
    add(1, 700, "3H10M50N10=2P5X5M4H", mism=(2, 12, 22))  # the operations the pipeline does not make
    add(1, 700, "20M300N70M", mism=(19, 20, 89))          # a jump: the columns behind it lie in other .pac bytes
    add(1, 800, "4S3I")                                    # no reference column at all: "0"
    # the holes of contig 0: N at [300, 330), R at [500, 503), n at [700, 701) (0-based)
    add(0, 311, "50M")             # starts in a hole
    add(0, 281, "30M")             # ends in one
    add(0, 291, "60M")             # spans one
    add(0, 271, "30M")             # only touches one: its last base lies before the hole's first
    add(0, 331, "30M")             # ... its first base behind the hole's last
    add(0, 290, "20M15D20M")       # deletes across one
    add(0, 480, "60M", patch=lambda s: s[:21] + "R" + s[22:])  # a hole letter other than N: read R matches it, read A does not
    add(0, 600, "130M", mism=(5,))  # the lone lower-case n, in the second round
    return cases


def hand_batches(genome, api):
    """the cases as mcx_sam_in: [(SamIn, keep, [(contig, pos, ops, printed SEQ) or None per line])] — a paired batch (every case in a slot of the parity its turn needs,
    unmapped reads in the gaps) and the same cases with mate2 = False as single reads"""
    cases = hand_cases(genome)
    out = []
    for paired in (True, False):
        slots = []
        for c in cases:
            if paired:
                while len(slots) % 2 != int(c[4]):
                    slots.append((-1, 0, [], b"GATTACA", len(slots) % 2 == 1, True))
                slots.append(c)
            elif not c[4]:
                slots.append(c)
        if paired and len(slots) % 2:
            slots.append((-1, 0, [], b"GATTACA", True, True))
        aln = np.zeros(len(slots), dtype=api.ALN_DTYPE)
        pool, lines = [], []
        for i, (chrom, pos, ops, raw, mate2, fwd) in enumerate(slots):
            aln[i]["chr"], aln[i]["pos"], aln[i]["fwd"], aln[i]["flag"] = chrom, pos, int(fwd), 0 if chrom >= 0 else 4
            aln[i]["n_cigar"], aln[i]["cigar_off"] = len(ops), len(pool)
            pool += [(n << 4) | "MIDNSHP=X".index(op) for n, op in ops]
            lines.append((chrom, pos, ops, turn(raw, mate2, fwd).decode()) if chrom >= 0 and ops else None)
        reads = [(b"h%d" % i, s[3], None) for i, s in enumerate(slots)]
        keep = []
        from test_sam_device import sam_in
        si, _ = sam_in(api, reads, paired, aln, np.array(pool + [0], dtype=np.uint32), None, keep)
        out.append((si, keep, lines))
    return out


def hand_want(lines, genome):
    up = [s.upper() for _, s in genome]
    want = []
    for l in lines:
        if l is None:
            want.append(None)
            continue
        chrom, pos, ops, seq = l
        md = py_md(pos, ops, seq, up[chrom])
        assert py_ref_from_md(ops, seq, md) == ref_span(pos, ops, up[chrom])
        want.append(md.encode())
    return want


def test_host_build_on_hand_made_records(md_check):
    from mapcaller_amd import api
    genome = hand_genome()
    ref = pack_ref([s for _, s in genome])
    assert ref["n_holes"] == 3 and int(ref["chr_fwd"][1]) & 3 == 3
    seen = set()
    for si, keep, lines in hand_batches(genome, api):
        pool, md_off = host_md(md_check, si, ref, keep)
        got, want = strings_of(pool, md_off), hand_want(lines, genome)
        bad = [(l, g, w) for l, g, w in zip(lines, got, want) if g != w]
        assert len(got) == len(want) and not bad, bad[:3]
        seen |= {w for w in want if w}
    # what the cases are for did come out
    assert {b"1", b"63", b"64", b"65", b"128", b"129", b"1000", b"0"} <= seen
    assert any(re.fullmatch(rb"(0[ACGT]){1000}0", w) for w in seen) and any(re.fullmatch(rb"(0[ACGT]){65}0", w) for w in seen)
    assert any(re.fullmatch(rb"10\^[ACGT]{2}0[ACGT]9", w) for w in seen)                 # ^AC0T
    assert any(re.fullmatch(rb"10\^[ACGT]{2}0\^[ACGT]{2}10", w) for w in seen)
    assert any(re.fullmatch(rb"30\^[ACGT]{100}30", w) for w in seen) and any(re.fullmatch(rb"60\^[ACGT]{4}50", w) for w in seen)
    assert any(w.startswith(b"0N0N0N") for w in seen) and any(w.endswith(b"0N0N0") for w in seen)  # a line that starts in the N hole, one that ends in it
    assert any(b"R0R" in w for w in seen) and any(re.search(rb"\^[ACGT]*N{15}", w) or b"N" * 10 in w for w in seen)
    assert b"30" in seen  # the lines that only touch the hole


def test_host_bam_records_carry_the_tag(md_check):
    """mcx_bam.h with a pool: block_size grows by the tag and nothing else of the record changes"""
    import struct
    from mapcaller_amd import api
    genome = hand_genome()
    ref = pack_ref([s for _, s in genome])
    si, keep, lines = hand_batches(genome, api)[0]

    def records(si):
        rec_off = np.zeros(si.n_reads + 1, dtype=np.uint64)
        md_check.md_check_bam(C.byref(si), None, 0, rec_off.ctypes.data)
        out = np.zeros(int(rec_off[-1]) + 1, dtype=np.uint8)
        assert md_check.md_check_bam(C.byref(si), out.ctypes.data, int(rec_off[-1]), rec_off.ctypes.data) == int(rec_off[-1])
        return [out[int(a):int(b)].tobytes() for a, b in zip(rec_off[:-1], rec_off[1:])]
    plain = records(si)
    pool, md_off = host_md(md_check, si, ref, keep)
    si.md, si.md_off = pool.ctypes.data, md_off.ctypes.data
    for a, b, md in zip(plain, records(si), strings_of(pool, md_off)):
        tag = b"MDZ" + md + b"\0" if md else b""
        assert b == struct.pack("<i", len(a) - 4 + len(tag)) + a[4:] + tag
