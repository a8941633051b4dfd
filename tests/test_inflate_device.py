"""BGZF input inflated on the device: mcx_inflater_create / _free, mcx_inflate_dev, mcx_inflate, mcx_bgzf_inflate and the file front end's
device_inflate (-gpu_inflate).

The vectors are made here with Python's zlib and a small LSB-first bit writer, and each is first held against zlib.decompress(s, -15) itself.
CPU: the ABI surface; the decoder (mapcaller_amd/csrc/mcx_inflate.h compiled for the host, tests/hostemu/inflate_check.cpp) on every vector and every
damaged member, with guard bytes round each output; and the same file as a stand-alone program under -fsanitize=address,undefined on the vectors, the
damaged list and 2 000 seeded corruptions (single-bit flips and truncations) — the only place random corruption runs.  GPU: the same vectors and the
same fixed damaged list through the kernel (device buffers, host buffers cut into several launches), the BGZF reader on re-packed golden read files,
and the front end with device_inflate against the golden SAM and against the host path on damaged files.

Not reached by any vector: distance codes longer than the 11 bits zlib produced on these inputs.  They run through the same table builder and the
same canonical walk as the 15-bit literal code of the Fibonacci vector."""
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

from conftest import GOLD, ROOT, sam_diff

NEW = ("mcx_inflater_create", "mcx_inflater_free", "mcx_inflate_dev", "mcx_inflate", "mcx_bgzf_inflate")
EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
OK, DAMAGED, INPUT, LENGTH, CRC = 0, 1, 2, 3, 4  # mcx_inflate_status
ANY_BAD = 255
GUARD = 64
CHECK_SRC = os.path.join(ROOT, "tests", "hostemu", "inflate_check.cpp")


# ---- CPU: the surface -----------------------------------------------------------------------------------------------
def test_the_inflate_calls_are_declared_bound_and_exported():
    from mapcaller_amd import api, run
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for s in NEW:
        assert s in api.SYMBOLS and re.search(r"\b%s\s*\(" % s, header), s
    for name, value in (("MCX_INFLATE_OK", OK), ("MCX_INFLATE_DAMAGED", DAMAGED), ("MCX_INFLATE_INPUT", INPUT), ("MCX_INFLATE_LENGTH", LENGTH), ("MCX_INFLATE_CRC", CRC)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
    assert "device_inflate" in header and "reserved1" not in header
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in NEW:
            assert f" {s}\n" in nm, s
        L = api.lib()
        assert L.mcx_inflater_create.argtypes[1] is C.c_uint64 and L.mcx_inflater_create.argtypes[3] is C.c_uint32
        assert L.mcx_inflater_free.restype is None
        for s in ("mcx_inflate_dev", "mcx_inflate"):
            f = getattr(L, s)
            assert f.restype is C.c_int and f.argtypes[2] is C.c_uint64 and f.argtypes[4] is C.c_uint32 and f.argtypes[6] is C.c_uint64
        assert L.mcx_bgzf_inflate.restype is C.c_int64 and L.mcx_bgzf_inflate.argtypes[3] is C.c_uint64
    assert api.FileOpts.device_inflate.offset == 32 and C.sizeof(api.FileOpts) == 48
    assert api.FileOpts.exchange.offset == 40 and api.FileOpts.avg_state.offset == 16 and api.FileOpts.device_sam.offset == 12
    assert api.MEMBER_DTYPE.itemsize == 32
    assert inspect.signature(api.Mapper.map_files).parameters["device_inflate"].default is False
    assert callable(api.Inflater) and callable(api.bgzf_inflate)
    assert run.parse(["-i", "x", "-f", "a.fq.gz", "-gpu_inflate"]).gpu_inflate and not run.parse(["-i", "x", "-f", "a.fq.gz"]).gpu_inflate
    assert "-gpu_inflate" in open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_main.cpp")).read()


# ---- the vectors ----------------------------------------------------------------------------------------------------
class BitWriter:
    """LSB-first bits, as RFC 1951 packs them; Huffman codes go in most significant bit first."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, n):
        self.bits(int(format(value, "0%db" % n)[::-1], 2), n)

    def fixed(self, sym):
        if sym < 144: self.code(0x30 + sym, 8)
        elif sym < 256: self.code(0x190 + sym - 144, 9)
        elif sym < 280: self.code(sym - 256, 7)
        else: self.code(0xC0 + sym - 280, 8)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def fastq_text():
    return gzip.open(os.path.join(GOLD, "toy", "r1.fq.gz"), "rb").read()[:65280]


def fibonacci_text():
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    data = bytearray()
    for k, c in enumerate(fib):
        data += bytes([65 + k]) * c
    assert len(data) == 46367
    random.Random(7).shuffle(data)
    return bytes(data)


def far_match_stream():
    """a fixed-Huffman block by hand: 32 768 literals, a match of 258 at distance 32 768, one of 258 at distance 1"""
    lit = random.Random(3).randbytes(32768)
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2)
    for b in lit:
        w.fixed(b)
    w.fixed(285); w.code(29, 5); w.bits(32768 - 24577, 13)
    w.fixed(285); w.code(0, 5)
    w.fixed(256)
    text = lit + lit[:258] + lit[257:258] * 258
    return w.done(), text


def make_vectors():
    """[(name, deflate stream, text)]"""
    fq = fastq_text()
    v = [("fastq level %d" % l, raw(fq, l), fq) for l in (1, 6, 9)]
    v.append(("fastq fixed", raw(fq, 6, zlib.Z_FIXED), fq))
    v.append(("fastq stored", raw(fq, 0), fq))
    rnd = random.Random(1).randbytes(65280)
    v.append(("random bytes", raw(rnd, 6), rnd))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    three = c.compress(fq[:20000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(fq[20000:40000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(fq[40000:]) + c.flush()
    v.append(("three blocks", three, fq))
    fib = fibonacci_text()
    v.append(("fibonacci huffman-only", raw(fib, 6, zlib.Z_HUFFMAN_ONLY), fib))
    v.append(("far match",) + far_match_stream())
    v.append(("empty", bytes.fromhex("0300"), b""))
    v.append(("one byte", raw(b"A"), b"A"))
    v.append(("zeros 65536", raw(bytes(65536)), bytes(65536)))
    for name, s, text in v:
        assert zlib.decompress(s, -15) == text, name
    assert v[3][1][0] & 7 == 3 or v[3][1][0] & 6 == 2, "Z_FIXED: the first block is of type 1"
    assert len(v[5][1]) + 26 == 65326
    return v


def member_of(s, text):
    return dict(src=s, isize=len(text), crc=zlib.crc32(text), text=text)


def zlib_raises(s):
    try:
        zlib.decompress(s, -15)
    except zlib.error:
        return True
    return False


def make_damaged(vectors):
    """[(name, member, set of statuses that fit)]: the fixed list, from the level-6 FASTQ vector and the Fibonacci vector (and two streams by hand)"""
    out = []
    for name, s, text in (vectors[1], vectors[7]):
        m = member_of(s, text)
        out.append((name + ": wrong CRC", dict(m, crc=m["crc"] ^ 1), {CRC}))
        out.append((name + ": ISIZE one less", dict(m, isize=m["isize"] - 1), {LENGTH}))
        out.append((name + ": ISIZE one more", dict(m, isize=m["isize"] + 1), {LENGTH}))
        out.append((name + ": cut in half", dict(m, src=s[:len(s) // 2]), {INPUT}))
        assert s[0] & 6 == 4, "a dynamic block first"
        bit = next(b for b in range(3, 3 + 14 + 19 * 3) if zlib_raises(bytes([*s[:b >> 3], s[b >> 3] ^ (1 << (b & 7)), *s[(b >> 3) + 1:]])))
        flipped = bytes([*s[:bit >> 3], s[bit >> 3] ^ (1 << (bit & 7)), *s[(bit >> 3) + 1:]])
        # (zlib decodes without a limit on the output: what it calls invalid may show here as text running past isize, or as the input running out, first)
        out.append((name + ": bit %d of the dynamic header flipped" % bit, dict(m, src=flipped), {DAMAGED, INPUT, LENGTH}))
        out.append((name + ": block type 3", dict(m, src=bytes([s[0] | 6]) + s[1:]), {DAMAGED}))
    text = vectors[1][2][:3000]
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2); w.fixed(257); w.code(0, 5)
    for b in text[3:]:
        w.fixed(b)
    w.fixed(256)
    out.append(("a first symbol that is a match", dict(member_of(w.done(), text)), {DAMAGED}))
    stored = bytes([1]) + struct.pack("<HH", len(text), (~len(text) & 0xFFFF) ^ 0x10) + text
    out.append(("stored block with LEN != ~NLEN", member_of(stored, text), {DAMAGED}))
    for name, m, kinds in out:
        assert OK not in kinds, name
    return out


def zlib_verdict(m):
    """What zlib makes of the member's stream.  A stream zlib inflates to its end — a flipped bit often leaves a valid stream of another text — becomes a
    member of the text zlib gave, which the decoder must give too; anything else keeps the original's isize and CRC and must fail."""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(m["src"], 65537)
    except zlib.error:
        return m, None
    if not d.eof or len(text) > 65536:
        return m, None
    return member_of(m["src"], text), text


def make_corruptions(vectors, count=2000):
    rng = random.Random(2024)
    out = []
    for k in range(count):
        name, s, text = vectors[(1, 6, 7)[k % 3]]
        if rng.random() < 0.8:
            # (half of the flips in the first 200 bytes: the headers, where a bit changes the most)
            bit = rng.randrange(8 * min(len(s), 200)) if rng.random() < 0.5 else rng.randrange(8 * len(s))
            s2 = bytearray(s); s2[bit >> 3] ^= 1 << (bit & 7); s2 = bytes(s2)
        else:
            s2 = s[:rng.randrange(len(s))]
        out.append(member_of(s2, text))
    return out


@pytest.fixture(scope="module")
def vectors():
    return make_vectors()


@pytest.fixture(scope="module")
def damaged(vectors):
    return make_damaged(vectors)


# ---- CPU: the decoder compiled for the host ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inflate_check(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("inflate_check") / "libinflate_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", CHECK_SRC, "-o", out], check=True, stderr=subprocess.PIPE, timeout=600)
    L = C.CDLL(out)
    L.inflate_check_member.restype = C.c_uint32
    L.inflate_check_member.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    return L


def host_member(L, m, slack=True):
    """(status, text, longest codes) of one member through the host build, 64 guard bytes of 0xA5 on either side of its output checked"""
    src = np.frombuffer(m["src"] + (b"\xff" * 8 if slack else b""), dtype=np.uint8).copy()
    if src.size == 0:
        src = np.zeros(1, dtype=np.uint8)
    room = min(m["isize"], 65536)
    out = np.full(room + 2 * GUARD, 0xA5, dtype=np.uint8)
    longest = np.zeros(3, dtype=np.uint32)
    st = L.inflate_check_member(src.ctypes.data, len(m["src"]), len(m["src"]) + (8 if slack else 0), out.ctypes.data + GUARD, m["isize"], m["crc"], longest.ctypes.data)
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + room:] == 0xA5).all(), "the guards"
    return st, out[GUARD:GUARD + room].tobytes(), longest.tolist()


def test_host_build_inflates_every_vector(inflate_check, vectors):
    for name, s, text in vectors:
        for slack in (True, False):
            st, got, longest = host_member(inflate_check, member_of(s, text), slack)
            assert st == OK and got == text, (name, slack, st)
        if name.startswith("fibonacci"):
            assert longest[0] == 15 and longest[1] == 1, longest  # zlib's limit for the literal code; the single one-bit distance code
        if name == "three blocks":
            assert longest[2] >= 4, longest  # (the empty stored blocks of the two flushes among them)


def test_host_build_gives_every_damaged_member_its_status(inflate_check, damaged):
    for name, m, kinds in damaged:
        for slack in (True, False):
            st, _, _ = host_member(inflate_check, m, slack)
            assert st in kinds, (name, slack, st)


def write_vector_file(path, records):
    """tests/hostemu/inflate_check.cpp's input: (member, expected status or ANY_BAD)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(records)))
        for m, expect in records:
            text = m["text"] if expect == OK else b""
            f.write(struct.pack("<5I", len(m["src"]), m["isize"], m["crc"], expect, len(text)) + m["src"] + text)


def test_sanitizer_build_takes_vectors_damaged_and_seeded_corruptions(tmp_path, vectors, damaged):
    """A stand-alone program (its own main) under AddressSanitizer and UndefinedBehaviorSanitizer: every member in buffers of exactly the contract's
    sizes, with and without slack behind the input.  Every corruption must return — with zlib's verdict where zlib accepts the stream — and nothing
    may be reported."""
    exe = str(tmp_path / "inflate_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-DINFLATE_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    CHECK_SRC, "-o", exe], check=True, stderr=subprocess.PIPE, timeout=600)
    records = [(member_of(s, text), OK) for _, s, text in vectors]
    records += [(m, next(iter(kinds)) if len(kinds) == 1 else ANY_BAD) for _, m, kinds in damaged]
    accepted = 0
    for m in make_corruptions(vectors):
        m, text = zlib_verdict(m)
        accepted += text is not None
        records.append((m, OK if text is not None else ANY_BAD))
    assert accepted >= 100  # (a flipped bit in a literal's code or in extra bits leaves a valid stream)
    vec = str(tmp_path / "members.bin")
    write_vector_file(vec, records)
    r = subprocess.run([exe, vec], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = [l for l in r.stdout.split("\n") if l and not l.startswith("#")]
    assert len(lines) == len(records)


# ---- GPU ------------------------------------------------------------------------------------------------------------
def layout(members, odd=True):
    """the members' bytes and texts at deliberately odd offsets, 64 guard bytes between them and behind the last: (src, records, dst size)"""
    src = bytearray(b"\xee" * 3)
    recs = np.zeros(len(members), dtype=[("src_off", "<u8"), ("dst_off", "<u8"), ("src_len", "<u4"), ("isize", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")])
    at = GUARD + 1
    for i, m in enumerate(members):
        if odd and len(src) % 2 == 0:
            src += b"\xee"
        recs[i] = (len(src), at, len(m["src"]), m["isize"], m["crc"], 0)
        src += m["src"] + b"\xee" * 9
        at += min(m["isize"], 65536) + GUARD + (1 if (at + m["isize"]) % 2 == 0 else 0)
    return bytes(src) + bytes(8), recs, at


def check_texts(dst, recs, members, statuses, want_kinds):
    covered = np.zeros(dst.size, dtype=bool)
    for i, m in enumerate(members):
        lo, n = int(recs["dst_off"][i]), min(m["isize"], 65536)
        covered[lo:lo + n] = True
        if want_kinds[i] == {OK}:
            assert statuses[i] == OK and dst[lo:lo + n].tobytes() == m["text"], i
        else:
            assert statuses[i] in want_kinds[i], (i, statuses[i], want_kinds[i])
    assert (dst[~covered] == 0xA5).all(), "the guards"


@pytest.mark.gpu
def test_inflate_dev_all_vectors_in_one_launch(vectors):
    import torch
    from mapcaller_amd import api
    members = [member_of(s, text) for _, s, text in vectors]
    src, recs, dst_bytes = layout(members)
    dev = torch.device("cuda:0")
    d_src = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).to(dev)
    d_mem = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
    d_dst = torch.full((dst_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    d_st = torch.full((len(members),), 77, dtype=torch.int32, device=dev)
    with api.Inflater(device=0) as inf:
        rc = inf.inflate_dev(d_src, d_mem, len(members), d_dst, d_st)
        assert rc == 0, api.lib().mcx_last_error()
        assert inf.last_ms() > 0
        # what breaks the contract is refused before any launch
        for field, value in (("isize", 65537), ("src_off", len(src)), ("dst_off", dst_bytes)):
            bad = recs.copy(); bad[field][3] = value
            assert inf.inflate_dev(d_src, torch.from_numpy(bad.view(np.uint8).copy()).to(dev), len(members), d_dst, d_st) == api.ERR_ARG
    small = api.Inflater(device=0, max_members=4)
    assert small.inflate_dev(d_src, d_mem, len(members), d_dst, d_st) == api.ERR_ARG
    small.close()
    check_texts(d_dst.cpu().numpy(), recs, members, d_st.cpu().numpy().tolist(), [{OK}] * len(members))


@pytest.mark.gpu
def test_inflate_host_buffers_in_several_launches(vectors):
    from mapcaller_amd import api
    members = [member_of(s, text) for _, s, text in vectors] * 2
    src, recs, dst_bytes = layout(members)
    with api.Inflater(device=0, max_src_bytes=256 << 10, max_dst_bytes=256 << 10, max_members=16) as inf:
        dst = np.full(dst_bytes, 0xA5, dtype=np.uint8)
        rc, st = inf.inflate(src[:-8], recs, dst)  # (no slack behind the host's bytes: the object stages them)
        assert rc == 0, api.lib().mcx_last_error()
        assert sum(m["isize"] for m in members) > 4 * (256 << 10)  # more text than four launches hold
        check_texts(dst, recs, members, st.tolist(), [{OK}] * len(members))
        bad = recs.copy(); bad["dst_off"][5] = dst_bytes - 10
        assert inf.inflate(src, bad, dst)[0] == api.ERR_ARG


@pytest.mark.gpu
def test_damaged_members_among_good_ones(vectors, damaged):
    from mapcaller_amd import api
    good = [member_of(s, text) for _, s, text in vectors]
    members, kinds = [], []
    for k, (name, m, want) in enumerate(damaged):
        members += [good[k % len(good)], m]
        kinds += [{OK}, want]
    members.append(good[0]); kinds.append({OK})
    src, recs, dst_bytes = layout(members)
    with api.Inflater(device=0) as inf:
        dst = np.full(dst_bytes, 0xA5, dtype=np.uint8)
        rc, st = inf.inflate(src, recs, dst)
        assert rc == api.ERR_IO
        check_texts(dst, recs, members, st.tolist(), kinds)
        # the object is as good as new
        src2, recs2, n2 = layout(good)
        dst2 = np.full(n2, 0xA5, dtype=np.uint8)
        rc, st = inf.inflate(src2, recs2, dst2)
        assert rc == 0 and not st.any()
        check_texts(dst2, recs2, good, st.tolist(), [{OK}] * len(good))


def write_bgzf(path, data, block=0xff00, level=6):
    """bgzip's container (tests/test_gpu_parity.py's _write_bgzf restated): independent gzip members, each carrying its own size in a 'BC' extra field"""
    with open(path, "wb") as f:
        for i in range(0, len(data), block):
            chunk = data[i:i + block]
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            comp = c.compress(chunk) + c.flush()
            f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
        f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


@pytest.mark.gpu
def test_bgzf_reader_by_itself(tmp_path):
    from mapcaller_amd import api
    for name in ("toy", "var"):
        text = gzip.open(os.path.join(GOLD, name, "r1.fq.gz"), "rb").read()
        for block, level in ((0xff00, 1), (3000, 9)):
            path = str(tmp_path / f"{name}_{block}.fq.gz")
            write_bgzf(path, text, block, level)
            total, got = api.bgzf_inflate(path, device=0, cap=len(text) + 100)
            assert total == len(text) and got == text, (name, block)
    # a tail that is no member: the text up to there
    whole = open(str(tmp_path / "var_3000.fq.gz"), "rb").read()
    cut = whole.find(b"\x1f\x8b\x08\x04", len(whole) // 2)
    half = str(tmp_path / "half.fq.gz")
    open(half, "wb").write(whole[:cut] + b"not a member at all, forty bytes of it..")
    want = b""
    rest = whole[:cut]
    while rest:
        d = zlib.decompressobj(31)
        want += d.decompress(rest)
        rest = d.unused_data
    total, got = api.bgzf_inflate(half, device=0, cap=len(text))
    assert 0 < total == len(want) and got == want
    # a member whose CRC is wrong: -2, and the text before its stretch
    bad = bytearray(whole)
    third = whole.find(b"\x1f\x8b\x08\x04", len(whole) // 2)
    bad[third - 8] ^= 1  # (the CRC-32 of the member before)
    open(half, "wb").write(bytes(bad))
    total, got = api.bgzf_inflate(half, device=0, cap=len(text))
    assert total == -2 and text.startswith(got)
    # an ordinary gzip file is no BGZF
    plain = str(tmp_path / "plain.fq.gz")
    open(plain, "wb").write(gzip.compress(text[:100000]))
    assert api.bgzf_inflate(plain, device=0, cap=10)[0] == -1
    assert api.bgzf_inflate(str(tmp_path / "nope.gz"), device=0, cap=10)[0] == -1


@pytest.mark.gpu
def test_front_end_with_device_inflate(golden, tmp_path):
    """tests/test_gpu_parity.py's test_bgzf_input_equals_plain with device_inflate: the `var` pairs as BGZF, members of 64 KB and of 3 KB, give the
    golden SAM; with device_sam as well; a garbage tail and a falsified CRC give what the host path gives on the same file."""
    from mapcaller_amd import api
    g = golden["var"]
    raw_text = [open(g[k], "rb").read() for k in ("r1", "r2")]
    ix = api.Index(g["prefix"], device=0)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1 << 15)
    for block, dev_sam in ((0xff00, False), (3000, False), (3000, True)):
        f1, f2 = str(tmp_path / f"b{block}_1.fq.gz"), str(tmp_path / f"b{block}_2.fq.gz")
        write_bgzf(f1, raw_text[0], block); write_bgzf(f2, raw_text[1], block)
        out = str(tmp_path / f"b{block}.sam")
        mp.reset()
        st = mp.map_files(f1, f2, out, device_inflate=True, device_sam=dev_sam)
        nd, ex = sam_diff(g["sam"]["ksw2"], out)
        assert nd == 0, (block, dev_sam, ex)
        assert st["reads"] == 2 * raw_text[0].count(b"\n") // 4
    whole = open(str(tmp_path / "b3000_1.fq.gz"), "rb").read()
    cut = whole.find(b"\x1f\x8b\x08\x04", len(whole) // 2)
    half = str(tmp_path / "half_1.fq.gz")
    open(half, "wb").write(whole[:cut] + b"not a member at all, forty bytes of it..")
    crc = bytearray(whole); crc[cut - 8] ^= 1
    bad_crc = str(tmp_path / "crc_1.fq.gz")
    open(bad_crc, "wb").write(bytes(crc))
    for path in (half, bad_crc):
        res = []
        for dev in (False, True):
            out = str(tmp_path / f"cmp{int(dev)}.sam")
            mp.reset()
            st = mp.map_files(path, None, out, device_inflate=dev)
            res.append((st["reads"], open(out, "rb").read()))
        assert res[0] == res[1], path
        assert 0 <= res[0][0] < raw_text[0].count(b"\n") // 4
    mp.close(); ix.close()


@pytest.mark.gpu
def test_cli_accepts_gpu_inflate(golden, tmp_path):
    g = golden["toy"]
    f1, f2 = str(tmp_path / "t1.fq.gz"), str(tmp_path / "t2.fq.gz")
    write_bgzf(f1, open(g["r1"], "rb").read()); write_bgzf(f2, open(g["r2"], "rb").read(), 3000, 1)
    out = str(tmp_path / "cli.sam")
    r = subprocess.run([EXE, "-i", g["prefix"], "-f", f1, "-f2", f2, "-alg", "ksw2", "-sam", out, "-gpu_inflate"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    nd, ex = sam_diff(g["sam"]["ksw2"], out)
    assert nd == 0, ex
