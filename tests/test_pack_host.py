"""The read packer's body (mapcaller_amd/csrc/mcx_pack.h: what k_pack_reads runs per 32 bases of a read) by itself, on the host, through
tests/hostemu/pack_check.cpp: batches of 2, 254 and 4098 reads of 1 to 1000 bases (every length next to a 16- or 32-base boundary, offsets at
every residue mod 16), single-end and paired with mate 2 reversed, N / lower-case / IUPAC bytes at the first and last byte and around every
boundary, rows as long as the batch's longest read needs and as long as a larger context's — part by part the way the kernel walks a batch, each
read seen through a buffer of exactly the 16-byte words that hold its bytes.  Every row's words [0, packed_words(rlen)) must equal pack_read()'s,
the any-N word and the odd flags theirs; the AddressSanitizer build stops at a load or store outside a read's words or the batch's rows."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "pack_check.cpp")


def build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, SRC, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pack"), "pack_check", "-O2")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pack_san"), "pack_check_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def test_rows_equal_pack_read(plain):
    r = subprocess.run([plain], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "all cases agree" in r.stdout


def test_no_access_outside_the_batch_under_sanitizers(sanitized):
    r = subprocess.run([sanitized], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "all cases agree" in r.stdout
