"""The arithmetic of the read packer (mapcaller_amd/csrc/mcx_pack.h) piece by piece, on the host, through tests/hostemu/pack4_check.cpp: pack4 on
every byte value 0-255 at each of the four byte positions of a word (the other bytes from ACGTacgtNn and from random bytes), both strands, with and
without the odd flags, against nt4_code() and "bit 5 set" byte by byte; and pack16_span on every span of reads of 1 to 83 bytes that start at every
byte offset 0-15, both strands, each read seen through a buffer of exactly the 16-byte words that hold its bytes, against pack_read().  (What
pack_check covers — batches walked the way the kernel walks them, rows, the any-N word, reads that do not fit the stride — stays in test_pack_host.py.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "pack4_check.cpp")


def build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pack4"), "pack4_check", "-O2")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pack4_san"), "pack4_check_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def test_pack4_and_spans_equal_nt4_code(plain):
    r = subprocess.run([plain], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "all cases agree" in r.stdout


def test_no_access_outside_the_read_under_sanitizers(sanitized):
    r = subprocess.run([sanitized], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "all cases agree" in r.stdout
