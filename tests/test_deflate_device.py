"""BGZF output deflated on the device: mcx_deflater_* / mcx_bgzf_deflate_dev / mcx_bgzf_deflate / mcx_bgzf_eof and the file front end's -bgzf.

CPU: the surface (header, binding, exports, switches).  GPU: every vector of tests/test_deflate_host.py through the kernel — the bytes must EQUAL the host
build's, pass the same zlib checks, and come back through mcx_inflate_dev; capacity and block-size errors; the front end with bgzf_sam on the golden sets (many
parts, 4 096-byte blocks), -m, the io cases (append: one EOF block), the resident route, the CLI (also to stdout), two runs' md5, and the sharded refusal."""
import ctypes as C
import gzip
import hashlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import test_bgzf_resident as tb
from conftest import ROOT, sam_diff
from test_deflate_host import EOF, check_blocks, host_members, vectors, walk  # noqa: F401 (host_members, vectors: fixtures)
from test_multi import MULTI_SETS, compare

NEW = ("mcx_deflater_create", "mcx_deflater_free", "mcx_deflater_set_block", "mcx_bgzf_bound", "mcx_bgzf_deflate_dev", "mcx_bgzf_deflate", "mcx_bgzf_eof")
EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
GUARD = 64


# ---- CPU: the surface -----------------------------------------------------------------------------------------------
def test_the_deflate_calls_are_declared_bound_and_exported():
    from mapcaller_amd import api, run
    header = open(os.path.join(ROOT, "include", "mcx.h")).read()
    for s in NEW:
        assert s in api.SYMBOLS and re.search(r"\b%s\s*\(" % s, header), s
    for name, value in (("MCX_SAM_BGZF", 2), ("MCX_ROUTE_BGZF", 16)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
    assert "MCX_BGZF_BLOCK" in header
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in NEW:
            assert f" {s}\n" in nm, s
        L = api.lib()
        assert L.mcx_deflater_create.argtypes[1] is C.c_uint64 and L.mcx_deflater_free.restype is None
        assert L.mcx_deflater_set_block.argtypes[1] is C.c_uint32 and L.mcx_bgzf_bound.restype is C.c_uint64
        for s in ("mcx_bgzf_deflate_dev", "mcx_bgzf_deflate"):
            f = getattr(L, s)
            assert f.restype is C.c_int and f.argtypes[2] is C.c_uint64 and f.argtypes[4] is C.c_uint64
        assert L.mcx_bgzf_bound(0, 65280) == 0 and L.mcx_bgzf_bound(1, 65280) == 32 and L.mcx_bgzf_bound(65281, 65280) == 65281 + 62 and L.mcx_bgzf_bound(154, 77) == 154 + 62
        assert api.bgzf_eof() == EOF
    assert C.sizeof(api.FileOpts) == 48 and api.FileOpts.device_sam.offset == 12
    assert api.SAM_BGZF == 2 and api.ROUTE_BGZF == 16
    assert inspect.signature(api.Mapper.map_files).parameters["bgzf_sam"].default is False
    assert callable(api.Deflater) and inspect.signature(api.bgzf_deflate).parameters["block"].default == 65280
    assert run.parse(["-i", "x", "-f", "a.fq", "-sam", "o.sam.gz", "-bgzf"]).bgzf and not run.parse(["-i", "x", "-f", "a.fq"]).bgzf
    main = open(os.path.join(ROOT, "mapcaller_amd", "csrc", "mcx_main.cpp")).read()
    assert '"-bgzf"' in main and re.search(r'"\s+-bgzf\s', main) and '"-bam"' in main  # (the switch, its line in usage(), and the -bam refusal still there)


# ---- GPU: the encoder -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


@pytest.fixture(scope="module")
def device_members(api, vectors):
    """name -> the blocks mcx_bgzf_deflate_dev makes of the vector: text and output in torch tensors, the output with guard bytes round exactly the bound"""
    import torch
    out = {}
    with api.Deflater(0) as d:
        for name, text, block in vectors:
            assert d.set_block(block) == 0
            bound = d.bound(len(text))
            d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda() if text else torch.zeros(1, dtype=torch.uint8, device="cuda")
            d_out = torch.full((GUARD + bound + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            rc, n = d.deflate_dev(d_text, len(text), d_out[GUARD:], bound)
            assert rc == 0 and n <= bound, name
            got = d_out.cpu().numpy()
            assert (got[:GUARD] == 0xA5).all() and (got[GUARD + bound:] == 0xA5).all(), name
            out[name] = got[GUARD:GUARD + n].tobytes()
    return out


@pytest.mark.gpu
def test_device_bytes_equal_the_host_builds(vectors, host_members, device_members):
    for name, text, block in vectors:
        assert device_members[name] == host_members[name], name
        check_blocks(device_members[name], text, block)


@pytest.mark.gpu
def test_host_buffer_form_in_several_launches(api, vectors, host_members):
    """max_text_bytes = 10 000: the 200 000-byte text takes many launches at the small block sizes, one block a launch at the large ones — the same bytes"""
    with api.Deflater(0, max_text_bytes=10000) as d:
        for name, text, block in vectors:
            assert d.set_block(block) == 0
            assert d.deflate(text) == host_members[name], name
    assert api.bgzf_deflate(vectors[-1][1], block=1000) == host_members["sam@1000"]
    assert gzip.decompress(api.bgzf_deflate(b"ACGT" * 50000) + api.bgzf_eof()) == b"ACGT" * 50000


@pytest.mark.gpu
def test_blocks_come_back_through_the_device_inflater(api, vectors, device_members):
    import torch
    with api.Inflater(0, max_members=4096) as inf:
        for name, text, block in vectors:
            blob = device_members[name]
            if not blob:
                continue
            members, total = tb.bgzf_members(blob)
            assert total == len(text) and len(members) == -(-len(text) // block) <= 4096, name
            d_src = torch.frombuffer(bytearray(blob + bytes(8)), dtype=torch.uint8).cuda()
            d_mem = torch.frombuffer(bytearray(members.tobytes()), dtype=torch.uint8).cuda()
            d_dst = torch.zeros(total, dtype=torch.uint8, device="cuda")
            d_status = torch.full((len(members),), 77, dtype=torch.int32, device="cuda")
            assert inf.inflate_dev(d_src, d_mem, len(members), d_dst, d_status) == 0, name
            assert (d_status == 0).all() and d_dst.cpu().numpy().tobytes() == text, name


@pytest.mark.gpu
def test_capacity_and_block_size_errors(api):
    import torch
    text = bytes(range(256)) * 300
    with api.Deflater(0) as d:
        assert d.set_block(0) == api.ERR_ARG and d.set_block(65281) == api.ERR_ARG and d.block == 65280
        assert d.set_block(1000) == 0
        bound = d.bound(len(text))
        assert bound == len(text) + 31 * 77
        d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        d_out = torch.full((bound,), 0xA5, dtype=torch.uint8, device="cuda")
        rc, n = d.deflate_dev(d_text, len(text), d_out, bound - 1)
        assert rc == api.ERR_CAPACITY and n == 0 and (d_out == 0xA5).all()
        rc, n = d.deflate_dev(d_text, 0, d_out, 0)  # no text: nothing written
        assert rc == 0 and n == 0 and (d_out == 0xA5).all()
        rc, n = d.deflate_dev(d_text, len(text), d_out)
        assert rc == 0 and gzip.decompress(d_out[:n].cpu().numpy().tobytes() + EOF) == text
        L = api.lib()
        buf, got = np.full(bound, 0xA5, dtype=np.uint8), C.c_uint64(5)
        src = np.frombuffer(text, dtype=np.uint8)
        assert L.mcx_bgzf_deflate(d._h, src.ctypes.data, src.size, buf.ctypes.data, bound - 1, C.byref(got)) == api.ERR_CAPACITY and got.value == 0 and (buf == 0xA5).all()


# ---- GPU: the front end -----------------------------------------------------------------------------------------------
def bgzf_file_text(path):
    """the file walks as BGZF from byte 0 to its end, no block above 65 536 bytes, exactly one EOF block and that one last; returns gzip's text of it"""
    blob = open(path, "rb").read()
    members = walk(blob)  # (asserts every header and size)
    assert members and members[-1] == (b"\x03\x00", 0, 0) and blob.endswith(EOF)
    assert sum(1 for m in members if m[2] == 0) == 1
    return gzip.decompress(blob)


def unpacked(path, tmp_path, name):
    out = str(tmp_path / name)
    open(out, "wb").write(bgzf_file_text(path))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ("nw", "ksw2"))
@pytest.mark.parametrize("name", ("toy", "mc", "se"))
def test_bgzf_sam_equals_reference(api, golden, tmp_path, monkeypatch, name, alg):
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    g = golden[name]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg=alg, max_batch_reads=400)
    out = str(tmp_path / "o.sam.gz")
    st = mp.map_files(g["r1"], g["r2"], out, bgzf_sam=True)
    route = mp.last_route()
    mp.close(); ix.close()
    assert st["reads"] > 0 and route[0] & api.ROUTE_BGZF and route[0] & api.ROUTE_SAM
    assert len(walk(open(out, "rb").read())) > 20  # (many parts, many blocks)
    nd, ex = sam_diff(g["sam"][alg], unpacked(out, tmp_path, "o.sam"))
    assert nd == 0, ex


@pytest.mark.gpu
def test_bgzf_sam_with_multi(api, golden, tmp_path, monkeypatch):
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    name, alg = MULTI_SETS[0], "ksw2"
    g = golden[name]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg=alg, multi=True, max_batch_reads=400)
    out = str(tmp_path / "m.sam.gz")
    mp.map_files(g["r1"], g["r2"], out, bgzf_sam=True)
    mp.close(); ix.close()
    compare(name, alg, unpacked(out, tmp_path, "m.sam"))


@pytest.mark.gpu
def test_bgzf_sam_libraries_and_gz_input(api, io_golden, tmp_path, monkeypatch):
    """two libraries into one file (the second starts over the first's EOF block: one EOF block, at the end), and .gz read files"""
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    g = io_golden
    ix = api.Index(g["prefix"], device=0)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1000)
    out = str(tmp_path / "lib.sam.gz")
    mp.map_files(g["a1"], g["a2"], out, bgzf_sam=True)
    first = open(out, "rb").read()
    bgzf_file_text(out)
    mp.map_files(g["b1"], g["b2"], out, bgzf_sam=True, append_sam=True)
    assert open(out, "rb").read()[:len(first) - 28] == first[:-28]
    nd, ex = sam_diff(g["ref.lib.sam"], unpacked(out, tmp_path, "lib.sam"))
    assert nd == 0, ex
    mp.close()
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1000)
    out = str(tmp_path / "gz.sam.gz")
    mp.map_files(g["gz1"], g["gz2"], out, bgzf_sam=True, threads=3)
    nd, ex = sam_diff(g["ref.gz.sam"], unpacked(out, tmp_path, "gz.sam"), mask_se_reverse_qual=True)
    assert nd == 0, ex
    mp.close(); ix.close()


@pytest.mark.gpu
def test_bgzf_sam_on_the_resident_route(api, golden, tmp_path, monkeypatch):
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    monkeypatch.setenv("MCX_RESIDENT_LAUNCH_BYTES", "65536")
    g = golden["toy"]
    files = []
    for k, t in enumerate(tb.read_texts(g, "toy")):
        files.append(str(tmp_path / f"toy_{k + 1}.fq.gz"))
        tb.write_bgzf(files[-1], t, 3000)
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=800)
    out = str(tmp_path / "res.sam.gz")
    mp.map_files(files[0], files[1], out, device_inflate=True, device_parse=True, bgzf_sam=True)
    all_five = tb.ALL_FOUR | api.ROUTE_BGZF
    assert mp.last_route() == (all_five, all_five)
    mp.close(); ix.close()
    nd, ex = sam_diff(g["sam"]["ksw2"], unpacked(out, tmp_path, "res.sam"))
    assert nd == 0, ex


@pytest.mark.gpu
def test_two_runs_give_the_same_file(api, golden, tmp_path):
    g = golden["mc"]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    digests = []
    for k in range(2):
        mp = api.Mapper(ix, alg="nw", max_batch_reads=1 << 14)
        out = str(tmp_path / f"run{k}.sam.gz")
        mp.map_files(g["r1"], g["r2"], out, bgzf_sam=True)
        mp.close()
        digests.append(hashlib.md5(open(out, "rb").read()).hexdigest())
    ix.close()
    assert digests[0] == digests[1]
    nd, ex = sam_diff(g["sam"]["nw"], unpacked(out, tmp_path, "run.sam"))
    assert nd == 0, ex


@pytest.mark.gpu
def test_cli_bgzf(golden, tmp_path):
    g = golden["toy"]
    out = str(tmp_path / "cli.sam.gz")
    args = [EXE, "-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-alg", "ksw2", "-no_vcf", "-bgzf"]
    r = subprocess.run(args + ["-sam", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, MCX_TIMING="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert re.search(rb"\[mcx_map_files\] bgzf: \d+ bytes of text -> \d+ bytes of blocks", r.stderr)
    nd, ex = sam_diff(g["sam"]["ksw2"], unpacked(out, tmp_path, "cli.sam"))
    assert nd == 0, ex
    # to stdout: the same stream
    r = subprocess.run(args + ["-sam", "-"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(out, "rb").read()
    # -gpus 2 is refused before anything is opened
    bad = str(tmp_path / "bad.sam.gz")
    r = subprocess.run(args + ["-sam", bad, "-gpus", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode != 0 and b"-bgzf" in r.stderr and not os.path.exists(bad)


@pytest.mark.gpu
def test_sharded_bgzf_is_refused(api, golden, tmp_path):
    g = golden["toy"]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1000)
    out = str(tmp_path / "sharded.sam.gz")
    L = api.lib()
    links = (api.Exchange * 2)()
    assert L.mcx_exchange_local(2, links) == 0
    fo = api.FileOpts()
    L.mcx_file_opts_default(C.byref(fo))
    fo.device_sam = api.SAM_BGZF
    fo.shard_rank, fo.shard_count = 0, 2
    fo.exchange = C.pointer(links[0])
    st = api.Stats()
    rc = L.mcx_map_files_ex(mp._h, g["r1"].encode(), g["r2"].encode(), C.byref(fo), out.encode(), C.byref(st))
    assert rc == api.ERR_UNSUPPORTED and b"BGZF" in L.mcx_last_error() and not os.path.exists(out)
    L.mcx_exchange_local_free(links)
    mp.close(); ix.close()
