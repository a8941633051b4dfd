"""Vectors and the host build for the tests of the device gunzipper (tests/test_gz_dev_host.py, tests/test_gz_device.py): ordinary gzip files made here
with Python's zlib / gzip, each first held against zlib.decompress itself; and tests/hostemu/gz_dev_check.cpp — mapcaller_amd/csrc/mcx_gz_dev.h compiled for
the host with one lane — behind ctypes.  Everything is made once per session and shared."""
import ctypes as C
import functools
import gzip
import os
import subprocess
import tempfile
import zlib

from test_gz_inflate import fastq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CHECK_SRC = os.path.join(ROOT, "tests", "hostemu", "gz_dev_check.cpp")

OK, DAMAGED, INPUT, CAPACITY, MORE = 0, 1, 2, 3, 4


class Round(C.Structure):
    """mcx_gz_round"""
    _fields_ = [("end_bit", C.c_uint64), ("text_bytes", C.c_uint64), ("crc32", C.c_uint32), ("final", C.c_uint32), ("status", C.c_uint32),
                ("stretches", C.c_uint32), ("starts", C.c_uint32), ("chain", C.c_uint32), ("overflowed", C.c_uint32), ("ms", C.c_float * 4)]

    def figures(self):
        return (self.end_bit, self.text_bytes, self.crc32, self.final, self.status, self.stretches, self.starts, self.chain, self.overflowed)


def gz_wrap(raw, text, header=b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03"):
    return header + raw + (zlib.crc32(text) & 0xFFFFFFFF).to_bytes(4, "little") + (len(text) & 0xFFFFFFFF).to_bytes(4, "little")


def gz_level(text, level, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 31, mem_level, strategy)
    return co.compress(text) + co.flush()


def header_len(blob):
    """the length of the RFC 1952 header of a member made here"""
    o, flg = 10, blob[3]
    if flg & 8:
        o = blob.index(b"\0", o) + 1
    if flg & 16:
        o = blob.index(b"\0", o) + 1
    return o


def golden_text(name, fn="r1.fq.gz"):
    return gzip.open(os.path.join(GOLD, name, fn), "rb").read()


@functools.lru_cache(maxsize=None)
def v1():
    """the golden `var` r1 text at level 6, memLevel 3: blocks of 0.5 - 1 KB; stretch 4096, 32 stretches a round, so several rounds"""
    text = golden_text("var")
    return gz_level(text, 6, 3), text


@functools.lru_cache(maxsize=None)
def v2(level):
    text = fastq(40_000, 7 + level)
    return gz_level(text, level), text


@functools.lru_cache(maxsize=None)
def v3():
    """false starts: deflate up to a full flush; stored blocks whose payload is a deflate stream of its own; a fresh deflate stream.  Returns the file, its text
    and the bit range of the stored blocks in the member's deflate stream."""
    a, p, b = fastq(6000, 1), fastq(6000, 3), fastq(6000, 2)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    first = co.compress(a) + co.flush(zlib.Z_FULL_FLUSH)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = co.compress(p) + co.flush()
    stored = b""
    for o in range(0, len(payload), 65535):
        piece = payload[o:o + 65535]
        stored += b"\x00" + len(piece).to_bytes(2, "little") + (len(piece) ^ 0xFFFF).to_bytes(2, "little") + piece
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    last = co.compress(b) + co.flush()
    text = a + payload + b
    return gz_wrap(first + stored + last, text), text, (len(first) * 8, (len(first) + len(stored)) * 8)


@functools.lru_cache(maxsize=None)
def v4():
    """room: 8 MB of one repeated record between two ordinary halves"""
    half = fastq(6000, 5)
    rec = half[:half.index(b"\n@") + 1]
    text = half[:len(half) // 2] + rec * ((8 << 20) // len(rec)) + half[len(half) // 2:]
    return gz_level(text, 6), text


@functools.lru_cache(maxsize=None)
def v5():
    """[(name, file, text, stretch, stretches a round)]"""
    data = fastq(4000, 3)
    tiny = b"@r\nACGT\n+\nFFFF\n"
    named = gz_wrap(zlib.compress(data[:500_000], 6)[2:-4], data[:500_000], b"\x1f\x8b\x08\x18" + b"\0\0\0\0" + b"\x00\x03" + b"reads.fq\0" + b"a comment\0")
    members = b"".join(gz_level(data[k * 300_000:(k + 1) * 300_000], 6) + (gz_level(b"", 6) if k == 1 else b"") for k in range(4))
    noise = os.urandom(1 << 18) * 2 + bytes(range(256)) * 500
    return [("stored", gz_level(data[:600_000], 0), data[:600_000], 65536, 8), ("fixed", gz_level(data[:300_000], 6, 8, zlib.Z_FIXED), data[:300_000], 16384, 8),
            ("tiny", gz_level(tiny, 9), tiny, 4096, 4), ("named", named, data[:500_000], 16384, 8), ("members", members, data[:1_200_000], 16384, 8),
            ("urandom", gz_level(noise, 6), noise, 65536, 8)]


@functools.lru_cache(maxsize=None)
def damaged():
    """[(name, file, the return value, the whole text)]: -2 damaged, -1 no gzip file"""
    text = fastq(4000, 11)
    good = gz_level(text, 6)
    flipped = bytearray(good); flipped[len(good) // 2] ^= 0x55
    crc = bytearray(good); crc[-6] ^= 1
    return [("flipped", bytes(flipped), -2, text), ("trailer", bytes(crc), -2, text), ("cut", good[:len(good) * 2 // 3], -2, text), ("no gzip", text[:1000], -1, text)]


@functools.lru_cache(maxsize=None)
def all_files():
    """[(name, file, text, stretch, stretches a round)]: every vector as a file"""
    out = [("v1", *v1(), 4096, 32)]
    out += [("v2 level %d" % l, *v2(l), 65536, 64) for l in (1, 6, 9)]
    f, t, _ = v3()
    out += [("v3", f, t, 65536, 32), ("v4", *v4(), 65536, 32)]
    out += v5()
    for name, f, t, _, _ in out:
        assert gzip.decompress(f) == t, name
    return out


@functools.lru_cache(maxsize=None)
def host_build():
    """tests/hostemu/gz_dev_check.cpp as a shared library"""
    out = os.path.join(tempfile.mkdtemp(prefix="gz_dev_check"), "libgz_dev_check.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", CHECK_SRC, "-o", out, "-lz"], check=True, stderr=subprocess.PIPE, timeout=600)
    L = C.CDLL(out)
    L.gzc_create.restype = C.c_void_p
    L.gzc_create.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64]
    L.gzc_free.restype = None
    L.gzc_free.argtypes = [C.c_void_p]
    L.gzc_reset.restype = None
    L.gzc_reset.argtypes = [C.c_void_p]
    L.gzc_guard_faults.restype = C.c_uint32
    L.gzc_guard_faults.argtypes = [C.c_void_p]
    L.gzc_round.restype = C.c_int
    L.gzc_round.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(Round)]
    L.gzc_text.restype = C.c_int
    L.gzc_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Round)]
    L.gzc_chain.restype = C.c_uint32
    L.gzc_chain.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_uint32]
    L.gzc_records.restype = C.c_uint32
    L.gzc_records.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]
    L.gzc_file.restype = C.c_int64
    L.gzc_file.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                           C.POINTER(C.c_uint32)]
    L.gzc_file_staging.restype = None
    L.gzc_file_staging.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


def host_file(blob, stretch, stretches, room, arena=0):
    """gzc_file: (return value, text delivered, status, rounds, rounds with an overflow, guard faults)"""
    L = host_build()
    buf = C.create_string_buffer(room + 16)
    n, st, rounds, over, faults = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    r = L.gzc_file(blob, len(blob), stretch, stretches, arena, buf, room, C.byref(n), C.byref(st), C.byref(rounds), C.byref(over), C.byref(faults))
    return r, buf.raw[:min(n.value, room)], st.value, rounds.value, over.value, faults.value


def rounds_of(round_fn, text_fn, raw, stretch):
    """A member's raw deflate stream `raw` (the whole of it, so src_is_end = 1) round by round through round_fn(src bytes, start_bit, is_end, Round) and
    text_fn(Round) -> bytes: ([figures of every round], the text).  Ends at the final block, at a status that is not OK, or after 4096 rounds."""
    figs, text, bit = [], [], 0
    for _ in range(4096):
        info = Round()
        src = raw[bit >> 3:]
        round_fn(src, bit & 7, 1, info)
        t = text_fn(info) if info.status == OK else b""
        figs.append(info.figures())
        text.append(t)
        if info.status != OK or info.final:
            break
        bit = (bit >> 3) * 8 + info.end_bit
    return figs, b"".join(text)


def host_rounds(raw, stretch, stretches, arena=0, want_chain=False):
    """rounds_of through the host build; want_chain: also [(stretch, start bit in raw)] of every round's chain"""
    L = host_build()
    z = L.gzc_create(stretch, stretches, arena)
    chains, at = [], [0]
    try:
        def rnd(src, bit, end, info):
            assert L.gzc_round(z, src, len(src), bit, end, C.byref(info)) == 0
            idx, sb = (C.c_uint32 * stretches)(), (C.c_uint64 * stretches)()
            k = L.gzc_chain(z, idx, sb, stretches)
            chains.append([(idx[i], at[0] * 8 + sb[i]) for i in range(k)])
            at[0] += info.end_bit >> 3

        def txt(info):
            buf = C.create_string_buffer(info.text_bytes + 1)
            assert L.gzc_text(z, buf, info.text_bytes, C.byref(info)) == 0
            return buf.raw[:info.text_bytes]
        figs, text = rounds_of(rnd, txt, raw, stretch)
        assert L.gzc_guard_faults(z) == 0
    finally:
        L.gzc_free(z)
    return (figs, text, chains) if want_chain else (figs, text)


def host_staging(blob, stretch, stretches):
    """gzc_file_staging: (rounds begun, rounds whose bytes lay inside what the walker staged the round before)"""
    rounds, hits = C.c_uint64(), C.c_uint64()
    host_build().gzc_file_staging(blob, len(blob), stretch, stretches, C.byref(rounds), C.byref(hits))
    return rounds.value, hits.value


def members_of(blob):
    """[(raw deflate stream, text)] of the members of a file made here of members without names (10-byte headers)"""
    out, o = [], 0
    while o < len(blob):
        d = zlib.decompressobj(-15)
        text = d.decompress(blob[o + 10:])
        raw_len = len(blob) - o - 10 - len(d.unused_data)
        out.append((blob[o + 10:o + 10 + raw_len], text))
        o += 10 + raw_len + 8
    return out
