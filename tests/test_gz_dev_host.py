"""The device gunzipper on the CPU (none of this needs a GPU): its surface — the calls, enums and struct declared, bound and exported, mcx_file_opts unchanged,
-gpu_gz known to the CLI and to run.py —; mapcaller_amd/csrc/mcx_gz_dev.h compiled for the host with one lane (tests/hostemu/gz_dev_check.cpp) on every vector
of tests/gz_dev_vectors.py at several stretch and round sizes, with guard symbols round every stretch's region and guard bytes round the text; and the same file
as a stand-alone program under -fsanitize=address,undefined on the vectors, the damaged list and 2 000 seeded corruptions (single-bit flips and truncations) —
the only place random corruption runs.  Nothing sanitised is loaded into Python."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import pytest

import gz_dev_vectors as V

ROOT = V.ROOT
sys.path.insert(0, ROOT)
NEW = ["mcx_gz_inflate_dev_last", "mcx_gunzipper_create", "mcx_gunzipper_free", "mcx_gunzipper_reset", "mcx_gunzip_round_dev", "mcx_gunzip_text_dev", "mcx_gz_inflate_dev"]


def test_the_new_calls_are_declared_bound_and_exported():
    from mapcaller_amd import api
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in api.SYMBOLS, s
    for name, value in (("MCX_GZ_OK", 0), ("MCX_GZ_DAMAGED", 1), ("MCX_GZ_INPUT", 2), ("MCX_GZ_CAPACITY", 3), ("MCX_GZ_MORE", 4), ("MCX_INFLATE_BGZF", 1), ("MCX_INFLATE_GZ", 2), ("MCX_ROUTE_GZ", 512)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
    assert (api.GZ_OK, api.GZ_DAMAGED, api.GZ_INPUT, api.GZ_CAPACITY, api.GZ_MORE, api.ROUTE_GZ, api.INFLATE_BGZF, api.INFLATE_GZ) == (0, 1, 2, 3, 4, 512, 1, 2)
    # mcx_gz_round as the header has it: 2 x u64, 7 x u32, 4 floats
    body = re.search(r"typedef struct mcx_gz_round \{(.*?)\} mcx_gz_round;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(uint64_t|uint32_t|float)\s", "", decl.strip()).split(",") if decl.strip()]
    assert fields == ["end_bit", "text_bytes", "crc32", "final", "status", "stretches", "starts", "chain", "overflowed", "ms[4]"], fields
    assert [f[0] for f in api.GzRound._fields_] == [f.split("[")[0] for f in fields] and C.sizeof(api.GzRound) == 64
    assert [f[0] for f in V.Round._fields_] == [f[0] for f in api.GzRound._fields_] and C.sizeof(V.Round) == 64
    # mcx_file_opts keeps its layout: device_inflate is the same 32-bit field, now a bit set
    assert C.sizeof(api.FileOpts) == 48
    want = {"interleaved_pairs": 0, "host_threads": 4, "append_sam": 8, "device_sam": 12, "avg_state": 16, "shard_rank": 24, "shard_count": 28, "device_inflate": 32, "device_parse": 36, "exchange": 40}
    assert {n: getattr(api.FileOpts, n).offset for n, _ in api.FileOpts._fields_} == want
    opts = re.search(r"typedef struct mcx_file_opts \{(.*?)\} mcx_file_opts;", header, re.S).group(1)
    names = re.findall(r"\b(interleaved_pairs|host_threads|append_sam|device_sam|avg_state|shard_rank|shard_count|device_inflate|device_parse|exchange)\b\s*[,;]", re.sub(r"/\*.*?\*/", "", opts, flags=re.S))
    assert names == list(want), names
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in NEW:
            assert f" {s}\n" in nm, s
        L = api.lib()
        P = C.POINTER
        assert (L.mcx_gunzipper_create.restype, L.mcx_gunzipper_create.argtypes) == (C.c_int, [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, P(C.c_void_p)])
        assert (L.mcx_gunzipper_free.restype, L.mcx_gunzipper_free.argtypes) == (None, [C.c_void_p])
        assert (L.mcx_gunzipper_reset.restype, L.mcx_gunzipper_reset.argtypes) == (None, [C.c_void_p])
        assert (L.mcx_gunzip_round_dev.restype, L.mcx_gunzip_round_dev.argtypes) == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, P(api.GzRound)])
        assert (L.mcx_gunzip_text_dev.restype, L.mcx_gunzip_text_dev.argtypes) == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, P(api.GzRound)])
        assert (L.mcx_gz_inflate_dev.restype, L.mcx_gz_inflate_dev.argtypes) == (C.c_int64, [C.c_char_p, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, P(C.c_uint64)])


def test_the_switch_is_known_to_the_cli_and_to_run_py():
    import inspect
    from mapcaller_amd import api, run
    main = open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_main.cpp")).read()
    assert '"-gpu_gz"' in main and "MCX_INFLATE_GZ" in main and "         -gpu_gz " in main
    assert re.search(r'"-gpu_inflate"\)\s*fo\.device_inflate\s*\|=\s*MCX_INFLATE_BGZF', main)
    a = run.parse(["-i", "idx", "-f", "r1.fq.gz", "-gpu_gz", "-gpu_parse"])
    assert a.gpu_gz and a.gpu_parse and not a.gpu_inflate
    assert not run.parse(["-i", "idx", "-f", "r1.fq.gz"]).gpu_gz
    assert inspect.signature(api.Mapper.map_files).parameters["device_gz"].default is False
    assert list(inspect.signature(api.gz_inflate_dev).parameters) == ["path", "device", "stretch_bytes", "round_stretches", "cap"]
    # the front end tests bits, not truth: BGZF readers take bit 1, the route's ordinary files bit 2, a sharded or -p call neither
    files = open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_files.cpp")).read()
    assert "(opt.device_inflate & MCX_INFLATE_BGZF) ? idx->device : -1" in files
    assert "(opt.device_inflate & (MCX_INFLATE_BGZF | MCX_INFLATE_GZ)) && opt.device_parse && !sharded && !opt.interleaved_pairs" in files


SIZES = [(s, n) for s in (4096, 16384, 65536) for n in (1, 3, 32)]


@pytest.mark.parametrize("stretch,stretches", SIZES)
def test_host_build_gives_zlibs_bytes_and_crc_whatever_the_stretch(stretch, stretches):
    """Every vector as a file through the walker of members: the text is zlib's, and it is accepted only because every member's combined CRC-32 and ISIZE equal its
    trailer's (zlib's own); no guard symbol round a stretch's region and no guard byte round the text changes.  The arena is 16 M symbols at every size: a round of
    ONE stretch must hold a whole deflate block's text, a 16-bit symbol a byte (up to 16 K codes of up to 258 bytes: V4's are 4 MB), which the default — 8 symbols
    per compressed byte of a full round, 32 K symbols for one stretch of 4096 bytes — is not made for; there CAPACITY is the documented answer, which the last lines hold V4 to."""
    for name, blob, text, s0, n0 in V.all_files():
        r, got, status, rounds, over, faults = V.host_file(blob, stretch, stretches, len(text), arena=1 << 24)
        assert r == len(text) and got == text and status == V.OK and faults == 0, (name, r, status, faults)
    if (stretch, stretches) == (4096, 1):
        blob, text = V.v4()
        r, got, status, rounds, over, faults = V.host_file(blob, stretch, stretches, len(text))
        assert r == -2 and status == V.CAPACITY and faults == 0 and text.startswith(got) and len(got) < len(text)


def test_host_build_at_the_sizes_the_vectors_are_made_for():
    """each vector at its own stretch and round size: the rounds it is meant to take, V4's overflow"""
    seen = {}
    for name, blob, text, stretch, stretches in V.all_files():
        r, got, status, rounds, over, faults = V.host_file(blob, stretch, stretches, len(text))
        assert r == len(text) and got == text and faults == 0, name
        seen[name] = (rounds, over)
    assert seen["v1"][0] >= 4 and seen["v2 level 6"][0] == 1 and seen["v4"][1] >= 1, seen


def test_the_walker_stages_the_bytes_the_next_round_asks_for():
    """The next round's bytes are staged while this one runs: a round ends on the first block end at or beyond its last stretch, so the next begins a little
    further on than the staged range does, and asks for as many bytes again — the staged range carries four stretches of slack for that.  Over files of
    several rounds every round but the first of a member lies inside what was staged before it, except where a round ended short (an overflow: V4)."""
    seen = {}
    for name, blob, text, stretch, stretches in V.all_files():
        seen[name] = V.host_staging(blob, stretch, stretches)
    rounds, hits = seen["v1"]
    assert rounds >= 5 and hits == rounds - 1, seen
    for level in (1, 6, 9):  # several rounds of 8 stretches of 64 KB
        blob, _ = V.v2(level)
        rounds, hits = V.host_staging(blob, 65536, 8)
        assert rounds >= 5 and hits == rounds - 1, (level, rounds, hits)
    rounds, hits = seen["members"]  # four members and an empty one: a member's first round begins behind a header nobody staged for
    assert hits >= rounds - 5 - 1 and hits >= 1, seen


def test_host_build_on_the_damaged_files():
    want = {"flipped": (-2, (V.DAMAGED, V.INPUT)), "trailer": (-2, (V.DAMAGED,)), "cut": (-2, (V.INPUT,)), "no gzip": (-1, (0,))}
    for name, blob, ret, text in V.damaged():
        for stretch, stretches in ((4096, 32), (16384, 8), (65536, 3)):
            r, got, status, rounds, over, faults = V.host_file(blob, stretch, stretches, len(text))
            assert r == ret == want[name][0] and status in want[name][1] and faults == 0, (name, r, status)
            if name in ("trailer", "cut"):
                assert text.startswith(got) and len(got) < len(text), name


def test_v3_no_false_start_is_in_the_chain():
    """20 starts are found, 7 of them inside the stored blocks' payload (a deflate stream of its own: true block headers that the member's decoder never visits);
    the chain holds none of them, runs through the stored blocks to the fresh stream behind them, and the text is right"""
    blob, text, (lo, hi) = V.v3()
    raw = blob[V.header_len(blob):-8]
    L = V.host_build()
    figs, got, chains = V.host_rounds(raw, 65536, 32, want_chain=True)
    assert got == text and len(text) == 4_668_016
    assert len(figs) == 1 and figs[0][5] == 22 and figs[0][6] == 20 and figs[0][7] >= 12, figs
    assert not [c for c in chains[0] if lo < c[1] < hi], chains[0]
    # the records themselves: the stretches that begin inside the payload found starts there, and none was met
    z = L.gzc_create(65536, 32, 0)
    info = V.Round()
    assert L.gzc_round(z, raw, len(raw), 0, 1, C.byref(info)) == 0
    sb, eb, how, ns = (C.c_uint64 * 32)(), (C.c_uint64 * 32)(), (C.c_uint32 * 32)(), (C.c_uint32 * 32)()
    n = L.gzc_records(z, sb, eb, how, ns, 32)
    L.gzc_free(z)
    inside = [i for i in range(1, n) if lo < sb[i] < hi]
    assert len(inside) == 7 and not set(inside) & {c[0] for c in chains[0]}, inside


def write_vector_file(path, records):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(records)))
        for blob, expect, text, stretch, stretches, corrupt in records:
            f.write(struct.pack("<6I", len(blob), expect, len(text), stretch, stretches, corrupt))
            f.write(blob); f.write(text)


def test_host_build_under_the_sanitizers(tmp_path):
    """gz_dev_check.cpp as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer, every input and output in a buffer of exactly its size:
    the vectors, the damaged files, and 2 000 seeded corruptions of the small vectors.  Every run must return; nothing may be reported."""
    exe = str(tmp_path / "gz_dev_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-DGZ_DEV_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    V.CHECK_SRC, "-o", exe, "-lz"], check=True, stderr=subprocess.PIPE, timeout=600)
    small = {"tiny": (4096, 4), "fixed": (4096, 8), "named": (4096, 8), "members": (16384, 3)}
    records = [(blob, 0, text, stretch, stretches, 0) for name, blob, text, stretch, stretches in V.all_files()]
    records += [(blob, 0, text, *small[name], 1) for name, blob, text, _, _ in V.v5() if name in small]
    records += [(blob, 3 if name == "flipped" else 1 if ret == -2 else 2, text, 16384, 8, 0) for name, blob, ret, text in V.damaged()]
    vec = str(tmp_path / "vectors.bin")
    write_vector_file(vec, records)
    r = subprocess.run([exe, vec, "2000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = [l for l in r.stdout.split("\n") if l and not l.startswith("#")]
    assert len(lines) == len(records) + 1
    m = re.match(r"corruptions: (\d+) accepted, (\d+) refused", lines[-1])
    assert m and int(m.group(1)) + int(m.group(2)) == 2000 and int(m.group(2)) >= 1000, lines[-1]
