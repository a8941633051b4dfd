"""The file front end's thread pool (mapcaller_amd/csrc/mcx_pool.h) by itself, on the host, through tests/hostemu/pool_check.cpp: rounds of run() with part
counts that change from round to round (2 to 41, a fixed seed), jobs that only count their index, and after every round the check that each index below the
count ran exactly once and none above it.  A pool whose workers read the next run's counters runs a job twice and then waits for ever; the plain build sees
either, the ThreadSanitizer build the unguarded access behind it.  The time limits are caps against a hang, not measurements: a sound pool needs seconds."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "pool_check.cpp")


def build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, SRC, "-o", exe, "-pthread"], check=True)
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pool"), "pool_check", "-O2")


@pytest.fixture(scope="module")
def tsan(tmp_path_factory):
    return build(tmp_path_factory.mktemp("pool_tsan"), "pool_check_tsan", "-O1", "-g", "-fsanitize=thread")


@pytest.mark.parametrize("threads", [12, 4])
def test_every_index_runs_once(plain, threads):
    r = subprocess.run([plain, str(threads), "100000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_no_data_race_under_threadsanitizer(tsan):
    r = subprocess.run([tsan, "8", "20000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-2000:]
