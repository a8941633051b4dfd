"""The BGZF encoder on the host: mapcaller_amd/csrc/mcx_deflate.h compiled for the CPU (tests/hostemu/deflate_check.cpp, a stand-alone program).

Every vector — one text with a block size — goes through the program; zlib must read every block back (raw inflate of the payload, gzip of the whole file
with the EOF block), header, BSIZE, CRC-32 and ISIZE must be exact, no block may pass 65 536 bytes or its text + 5 + 26, and the program itself checks the
guard bytes round every slot and member.  The same program under -fsanitize=address,undefined runs all vectors once.  The size conditions: see SIZE_CAPS and
test_golden_sam_text_against_zlib.  tests/test_deflate_device.py takes the vectors and this build's bytes from here: the kernel must give the same bytes."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import pytest

from conftest import GOLD, ROOT
from test_inflate_device import fibonacci_text

CHECK_SRC = os.path.join(ROOT, "tests", "hostemu", "deflate_check.cpp")
BLOCK = 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# compressed / text that the host build reaches on the golden SAM cuts, relative to zlib level 1 on the same cuts (measured with this build, which is
# deterministic): the encoder may not get worse than that by more than 2 % (the margin is for another zlib version's level 1)
RATIO_TO_ZLIB1 = 0.9575


def golden_sam_text():
    return gzip.open(os.path.join(GOLD, "mc", "ref.nw.sam.gz"), "rb").read()[:200000]


def make_vectors():
    rnd = random.Random(20260)
    v = [("byte*%d" % n, b"\x07" * n, BLOCK) for n in (0, 1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 260)]
    v.append(("AB*40", b"AB" * 40, BLOCK))
    v.append(("zeros", bytes(BLOCK), BLOCK))
    v.append(("random", rnd.randbytes(BLOCK), BLOCK))
    v.append(("acgt", bytes(rnd.choice(b"ACGT") for _ in range(BLOCK)), BLOCK))
    piece = rnd.randbytes(1000)
    v.append(("piece", (piece * 66)[:BLOCK], BLOCK))
    far = rnd.randbytes(32768)
    v.append(("dist32768", far + far[:32768 - 256], BLOCK))
    far = rnd.randbytes(32769)
    v.append(("dist32769", far + far[:300], BLOCK))
    # (the encoder keeps one earlier position per hash, so in random bytes a copy 32 768 back is long forgotten; behind a gap of zeros it is not: these two
    #  make the encoder use the longest distance, and show that it does not use a longer one)
    head = rnd.randbytes(300)
    v.append(("gap32768", head + bytes(32768 - 300) + head, BLOCK))
    v.append(("gap32769", head + bytes(32769 - 300) + head, BLOCK))
    v.append(("fibonacci", fibonacci_text(), BLOCK))
    v.append(("all256", bytes(range(256)), BLOCK))
    sam = golden_sam_text()
    assert len(sam) == 200000
    for b in (65280, 65279, 4096, 1000, 77):
        v.append(("sam@%d" % b, sam, b))
    return v


# cap on compressed / text (payload bytes), from the issue: zlib level 1 stays within each
SIZE_CAPS = {"zeros": 0.01, "piece": 0.05, "acgt": 0.35}


@pytest.fixture(scope="session")
def vectors():
    return make_vectors()


def build_check(directory, name, *flags):
    exe = os.path.join(str(directory), name)
    subprocess.run(["g++", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", *flags, CHECK_SRC, "-o", exe], check=True)
    return exe


def run_check(exe, vectors, directory):
    src, dst = os.path.join(str(directory), "vectors.bin"), os.path.join(str(directory), "members.bin")
    with open(src, "wb") as f:
        for _, text, block in vectors:
            f.write(struct.pack("<II", block, len(text)) + text)
    r = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    blob, out, at = open(dst, "rb").read(), [], 0
    for _ in vectors:
        (n,) = struct.unpack_from("<I", blob, at)
        out.append(blob[at + 4:at + 4 + n])
        at += 4 + n
    assert at == len(blob)
    return out


@pytest.fixture(scope="session")
def host_members(vectors, tmp_path_factory):
    """name -> the BGZF blocks the host build makes of the vector (no EOF block)"""
    d = tmp_path_factory.mktemp("deflate_check")
    return dict(zip([v[0] for v in vectors], run_check(build_check(d, "deflate_check", "-O2"), vectors, d)))


def walk(blob):
    """the members of a BGZF byte string: (payload, crc, isize) each; every header byte checked"""
    out, at = [], 0
    while at < len(blob):
        assert blob[at:at + 16] == bytes.fromhex("1f8b08040000000000ff060042430200"), at
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        assert 26 <= size <= 65536 and at + size <= len(blob)
        crc, isize = struct.unpack_from("<II", blob, at + size - 8)
        out.append((blob[at + 18:at + size - 8], crc, isize))
        at += size
    return out


def check_blocks(blob, text, block):
    """every condition a vector's blocks must satisfy; returns the payload bytes in all"""
    members = walk(blob)
    cuts = [text[i:i + block] for i in range(0, len(text), block)]
    assert len(members) == len(cuts)
    for (payload, crc, isize), cut in zip(members, cuts):
        assert isize == len(cut) and crc == zlib.crc32(cut)
        d = zlib.decompressobj(-15)
        assert d.decompress(payload) == cut and d.eof and not d.unused_data
        assert len(payload) <= isize + 5
    assert gzip.decompress(blob + EOF) == text
    return sum(len(m[0]) for m in members)


def test_host_build_every_vector(vectors, host_members):
    for name, text, block in vectors:
        payload = check_blocks(host_members[name], text, block)
        if name in SIZE_CAPS:
            assert payload <= SIZE_CAPS[name] * len(text), (name, payload / len(text))
    assert host_members["byte*0"] == b""
    # random bytes do not compress: the block is stored
    (payload, _, _), = walk(host_members["random"])
    assert len(payload) == BLOCK + 5 and payload[:5] == b"\x01" + struct.pack("<HH", BLOCK, BLOCK ^ 0xFFFF)
    # a distance of 32 769 is not used: what lies 32 769 back is the only earlier copy of those 300 bytes, so nothing of the tail may shrink
    (payload, _, _), = walk(host_members["dist32769"])
    assert len(payload) >= 32769 + 300
    # the same 300 random bytes 32 768 back are found and used, 32 769 back they are out of reach and cost their literals
    (near, _, _), = walk(host_members["gap32768"])
    (far, _, _), = walk(host_members["gap32769"])
    assert len(near) + 200 < len(far) and len(far) > 2 * 300


def raw(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def test_golden_sam_text_against_zlib(vectors, host_members):
    """Matching has to pay for itself: strictly less than Z_HUFFMAN_ONLY's total on the same cuts; and no worse than the recorded ratio to zlib level 1"""
    text = golden_sam_text()
    ours = sum(len(m[0]) for m in walk(host_members["sam@65280"]))
    cuts = [text[i:i + BLOCK] for i in range(0, len(text), BLOCK)]
    huffman_only = sum(len(raw(c, 6, zlib.Z_HUFFMAN_ONLY)) for c in cuts)
    level1 = sum(len(raw(c, 1)) for c in cuts)
    print("golden SAM text, 65 280-byte cuts: ours %.4f  zlib level 1 %.4f  Z_HUFFMAN_ONLY %.4f  ours / level 1 %.4f" %
          (ours / len(text), level1 / len(text), huffman_only / len(text), ours / level1))
    assert ours < huffman_only
    assert ours / level1 <= RATIO_TO_ZLIB1 * 1.02


def test_host_build_is_deterministic(vectors, host_members, tmp_path):
    some = [v for v in vectors if v[0] in ("sam@4096", "acgt", "fibonacci", "piece")]
    again = run_check(build_check(tmp_path, "deflate_check_o0", "-O0"), some, tmp_path)
    for (name, _, _), blob in zip(some, again):
        assert blob == host_members[name], name


def test_sanitized_program_on_all_vectors(vectors, host_members, tmp_path):
    """The stand-alone program (its own main; nothing of it is loaded into Python) built with -fsanitize=address,undefined: all vectors once, the same bytes"""
    exe = build_check(tmp_path, "deflate_check_san", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    for (name, _, _), blob in zip(vectors, run_check(exe, vectors, tmp_path)):
        assert blob == host_members[name], name
