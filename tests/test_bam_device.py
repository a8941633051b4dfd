"""BAM records made on the device: mcx_bam_format_dev / mcx_bam_format / mcx_bam_header and the file front end's -bam.

Every byte is held against the host build of the same header (tests/hostemu/bam_check.cpp, which tests/test_bam_host.py holds against the golden SAM files and
against hand-packed records): the synthetic batches and a golden set through the kernels on torch tensors with guard bytes round exactly n_bytes, the
capacity contract, the host-buffer twin; then the front end with bam=True — many parts and many 4 096-byte blocks on the golden sets, -m, two libraries in
one file (one header, one EOF block and that one last), the resident route — whose file must walk as BGZF and inflate to the header plus the host build's
records, byte for byte, and decode to the golden SAM's fields; two runs' md5; the command line (file and stdout, -sam x -bam y, the refusals)."""
import ctypes as C
import gzip
import hashlib
import os
import subprocess

import numpy as np
import pytest

import test_bgzf_resident as tb
from conftest import ROOT, SETS
from test_bam_host import (assert_records_are_lines, bam_check, decode_header, decode_records, expected_header, golden_parts, golden_reads, host_encode,  # noqa: F401 (fixtures)
                           host_encode_in, io_case, lines_with_extras, sq_lines, synthetic)
from test_deflate_host import EOF, walk
from test_multi import read_extras
from test_sam_device import n_pairs_part, sam_in, split_golden

EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
GUARD = 64


@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


@pytest.fixture(scope="module")
def mapper(api, golden):
    """a context to format with (the encoder looks nothing up in the index: any will do)"""
    ix = api.Index(golden["toy"]["prefix"], device=0)
    mp = api.Mapper(ix, alg="nw", max_batch_reads=2000)
    yield mp
    mp.close(); ix.close()


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def on_device(api, si, keep):
    """the SamIn of test_sam_device.sam_in (host arrays in `keep`) with every array in a torch tensor: (SamIn, the tensors)"""
    import torch
    names = ["off", "name_off", "bases", "names", "aln", "cigar"] + (["qual"] if si.qual else []) + (["x_index", "x_recs", "x_cigar"] if si.x_index else [])
    assert len(names) == len(keep)
    t = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).copy()).cuda() for k, v in zip(names, keep)}
    di = api.SamIn()
    for k in names:
        setattr(di, k, t[k].data_ptr())
    di.n_reads, di.paired = si.n_reads, si.paired
    return di, t


def format_dev_checked(api, mp, di, n, want, want_off, want_dropped):
    """mcx_bam_format_dev's whole contract on one input: the size with cap = 0, nothing written one byte short, then the bytes between untouched guards"""
    import torch
    L = api.lib()
    nb, nd = C.c_uint64(), C.c_uint64()
    rc = L.mcx_bam_format_dev(mp._h, C.byref(di), None, 0, None, C.byref(nb), C.byref(nd))
    total = nb.value
    assert total == len(want) and nd.value == want_dropped and rc == (api.ERR_CAPACITY if total else 0)
    d_out = torch.full((GUARD + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    out_ptr = d_out.data_ptr() + GUARD
    if total:
        nb2 = C.c_uint64()
        assert L.mcx_bam_format_dev(mp._h, C.byref(di), out_ptr, total - 1, d_off.data_ptr(), C.byref(nb2), C.byref(nd)) == api.ERR_CAPACITY
        assert nb2.value == total and bool((d_out == 0xA5).all())  # too small: the size again, and not a byte written
    assert L.mcx_bam_format_dev(mp._h, C.byref(di), out_ptr, total, d_off.data_ptr(), C.byref(nb), C.byref(nd)) == 0, L.mcx_last_error()
    got = d_out.cpu().numpy()
    assert nb.value == total and nd.value == want_dropped
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + total:] == 0xA5).all()
    assert (d_off.cpu().numpy().astype(np.uint64) == want_off).all()
    data = got[GUARD:GUARD + total].tobytes()
    if data != want:
        bad = next(i for i in range(total) if data[i] != want[i])
        r = int(np.searchsorted(want_off, bad, side="right")) - 1
        raise AssertionError(("first differing byte", bad, "read", r, "at", bad - int(want_off[r]), data[bad - 8:bad + 8].hex(), want[bad - 8:bad + 8].hex()))
    return data


@pytest.mark.gpu
@pytest.mark.parametrize("with_extras", [False, True])
@pytest.mark.parametrize("k", [0, 1])
def test_format_dev_on_the_synthetic_batches(api, mapper, bam_check, synthetic, k, with_extras):
    b = synthetic[k]
    keep = []
    si, _ = sam_in(api, b["reads"], b["paired"], b["aln"], b["pool"], b["extras"] if with_extras else None, keep)
    n = len(b["reads"])
    want, want_off, want_dropped = host_encode_in(bam_check, si, n)
    if with_extras:
        assert want == b"".join(b["want"]) and want_dropped == b["dropped"]  # (tests/test_bam_host.py's check, once more: these are the hand-packed bytes)
    di, t = on_device(api, si, keep)
    format_dev_checked(api, mapper, di, n, want, want_off, want_dropped)
    # the host-buffer twin
    L = api.lib()
    nb, nd = C.c_uint64(), C.c_uint64()
    out = np.full(len(want) + GUARD, 0xA5, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    assert L.mcx_bam_format(mapper._h, C.byref(si), out.ctypes.data, len(want) - 1, off.ctypes.data, C.byref(nb), C.byref(nd)) == api.ERR_CAPACITY
    assert nb.value == len(want) and (out == 0xA5).all() and (off == want_off).all()
    assert L.mcx_bam_format(mapper._h, C.byref(si), out.ctypes.data, len(want), off.ctypes.data, C.byref(nb), C.byref(nd)) == 0, L.mcx_last_error()
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0xA5).all() and (off == want_off).all() and nd.value == want_dropped


@pytest.mark.gpu
def test_format_dev_on_a_golden_set_and_the_python_wrapper(api, mapper, bam_check, golden):
    g = golden["mc"]
    reads = golden_reads(g)
    _, body, contigs = split_golden(g["sam"]["ksw2"])
    extras = read_extras("mc", "ksw2")
    for si, n, keep in golden_parts(reads, n_pairs_part(len(reads), True), body, contigs, extras):
        want, want_off, dropped = host_encode_in(bam_check, si, n)
        assert dropped == 0
        di, t = on_device(api, si, keep)
        data = format_dev_checked(api, mapper, di, n, want, want_off, 0)
        lines, _, _ = lines_with_extras(body, extras)
        assert_records_are_lines(decode_records(data), lines, contigs)
    b = {k: v for k, v in zip(("off", "name_off", "bases", "names", "aln", "cigar", "qual", "x_index", "x_recs", "x_cigar"), keep)}
    got, nd = mapper.bam_records(b["bases"][:int(b["off"][-1])], b["off"], [r[0] for r in reads], [r[2] for r in reads], True, b["aln"], b["cigar"],
                                 (b["x_index"], b["x_recs"], b["x_cigar"]))
    assert got == want and nd == 0
    assert all(v >= 0 for v in mapper.bam_last_ms())


@pytest.mark.gpu
def test_format_dev_with_nothing_to_do(api, mapper):
    si = api.SamIn()
    nb, nd = C.c_uint64(7), C.c_uint64(7)
    assert api.lib().mcx_bam_format_dev(mapper._h, C.byref(si), None, 0, None, C.byref(nb), C.byref(nd)) == 0 and nb.value == 0 and nd.value == 0
    assert api.lib().mcx_bam_format_dev(None, C.byref(si), None, 0, None, C.byref(nb), C.byref(nd)) == api.ERR_ARG


@pytest.mark.gpu
def test_the_header_call(api, golden):
    for name in ("toy", "mc"):
        head, _, _ = split_golden(golden[name]["sam"]["nw"])
        ix = api.Index(golden[name]["prefix"], device=0)
        want = expected_header(head, sq_lines(head))
        assert api.bam_header(ix) == want
        text, contigs, at = decode_header(want)
        assert text == api.sam_header(ix) and at == len(want) and contigs == sq_lines(head)
        L = api.lib()
        buf, nb = np.full(len(want), 0xA5, dtype=np.uint8), C.c_uint64()
        assert L.mcx_bam_header(ix._h, buf.ctypes.data, len(want) - 1, C.byref(nb)) == api.ERR_CAPACITY and nb.value == len(want) and (buf == 0xA5).all()
        ix.close()


# ---- the front end ---------------------------------------------------------------------------------------------------------------
def bam_stream(path_or_bytes):
    """the file walks as BGZF from byte 0 to its end with exactly one EOF block, and that one last; returns what gzip makes of it"""
    blob = path_or_bytes if isinstance(path_or_bytes, bytes) else open(path_or_bytes, "rb").read()
    members = walk(blob)  # (asserts every header and size)
    assert members and members[-1] == (b"\x03\x00", 0, 0) and blob.endswith(EOF)
    assert sum(1 for m in members if m[2] == 0) == 1
    return gzip.decompress(blob), members


def check_stream(stream, head, contigs, lines, want_records, qual_of=None):
    """an inflated file: the golden header, records that say what the golden lines say, and — byte for byte — the host build's records behind the header"""
    text, got_contigs, at = decode_header(stream)
    assert text.decode("latin-1").split("\n")[:-1] == head and got_contigs == sq_lines(head)
    assert stream[:at] == expected_header(head, sq_lines(head))
    assert_records_are_lines(decode_records(stream, at), lines, contigs, qual_of)
    assert stream[at:] == want_records


def se_qual_of(reads, lines, owner, first):
    def qual_of(k):  # (tests/test_bam_host.py check_golden: the golden QUAL of a reverse-strand single-end FASTQ read is masked)
        q = reads[owner[k]][2]
        return q[::-1] if first[k] and q is not None and (int(lines[k].split("\t")[1]) & 0x11) == 0x10 else None
    return qual_of


def map_to_bam(api, g, alg, out, multi=False, batch=400, **kw):
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg=alg, multi=multi, max_batch_reads=batch)
    st = mp.map_files(g["r1"], g["r2"], out, bam=True, **kw)
    route = mp.last_route()
    mp.close(); ix.close()
    return st, route


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ("nw", "ksw2"))
@pytest.mark.parametrize("name", ("toy", "mc", "se"))
def test_bam_file_equals_reference(api, bam_check, golden, tmp_path, monkeypatch, name, alg):
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    g = golden[name]
    out = str(tmp_path / "o.bam")
    st, route = map_to_bam(api, g, alg, out)
    assert st["reads"] > 0 and route[0] & api.ROUTE_BAM and route[0] & api.ROUTE_BGZF and route[0] & api.ROUTE_SAM
    stream, members = bam_stream(out)
    assert len(members) > 20  # (many parts, many blocks)
    reads = golden_reads(g)
    head, body, contigs = split_golden(g["sam"][alg])
    want, dropped = host_encode(bam_check, reads, n_pairs_part(len(reads), SETS[name]), body, contigs)
    assert dropped == 0
    check_stream(stream, head, contigs, body, want, se_qual_of(reads, body, list(range(len(body))), [True] * len(body)))


@pytest.mark.gpu
def test_bam_file_with_multi(api, bam_check, golden, tmp_path, monkeypatch):
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    name, alg = "mc", "ksw2"
    g = golden[name]
    out = str(tmp_path / "m.bam")
    map_to_bam(api, g, alg, out, multi=True)
    reads = golden_reads(g)
    head, body, contigs = split_golden(g["sam"][alg])
    extras = read_extras(name, alg)
    want, _ = host_encode(bam_check, reads, n_pairs_part(len(reads), True), body, contigs, extras)
    lines, _, _ = lines_with_extras(body, extras)
    assert len(lines) > len(body)
    check_stream(bam_stream(out)[0], head, contigs, lines, want)


@pytest.mark.gpu
def test_bam_file_of_two_libraries(api, bam_check, io_golden, tmp_path, monkeypatch):
    """the second library starts over the first's EOF block and writes no second header: one header, one EOF block, at the end"""
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    g = io_golden
    ix = api.Index(g["prefix"], device=0)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1000)
    out = str(tmp_path / "lib.bam")
    mp.map_files(g["a1"], g["a2"], out, bam=True)
    first = open(out, "rb").read()
    bam_stream(first)
    mp.map_files(g["b1"], g["b2"], out, bam=True, append_sam=True)
    mp.close(); ix.close()
    both = open(out, "rb").read()
    assert both[:len(first) - 28] == first[:-28] and len(both) > len(first)
    stream, _ = bam_stream(both)
    assert stream.count(b"BAM\1") == 1
    reads, paired = io_case(g, "lib")
    head, body, contigs = split_golden(g["ref.lib.sam"])
    # (each library is mapped by itself: its own pairs' part)
    n_a = len(reads) - 2 * (len(open(g["b1"], "rb").read().split(b"\n")) // 4)
    want = host_encode(bam_check, reads[:n_a], n_a, body[:n_a], contigs)[0] + host_encode(bam_check, reads[n_a:], len(reads) - n_a, body[n_a:], contigs)[0]
    check_stream(stream, head, contigs, body, want)


@pytest.mark.gpu
def test_bam_file_on_the_resident_route(api, bam_check, golden, tmp_path, monkeypatch):
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    monkeypatch.setenv("MCX_RESIDENT_LAUNCH_BYTES", "65536")
    g = golden["toy"]
    files = []
    for k, t in enumerate(tb.read_texts(g, "toy")):
        files.append(str(tmp_path / f"toy_{k + 1}.fq.gz"))
        tb.write_bgzf(files[-1], t, 3000)
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=800)
    out = str(tmp_path / "res.bam")
    mp.map_files(files[0], files[1], out, device_inflate=True, device_parse=True, bam=True)
    everything = tb.ALL_FOUR | api.ROUTE_BGZF | api.ROUTE_BAM
    assert mp.last_route() == (everything, everything)
    mp.close(); ix.close()
    reads = golden_reads(g)
    head, body, contigs = split_golden(g["sam"]["ksw2"])
    want, _ = host_encode(bam_check, reads, len(reads), body, contigs)
    check_stream(bam_stream(out)[0], head, contigs, body, want)


@pytest.mark.gpu
def test_two_runs_give_the_same_bam(api, golden, tmp_path):
    g = golden["mc"]
    digests = []
    for k in range(2):
        out = str(tmp_path / f"run{k}.bam")
        map_to_bam(api, g, "nw", out, batch=1 << 14)
        digests.append(hashlib.md5(open(out, "rb").read()).hexdigest())
    assert digests[0] == digests[1]


@pytest.mark.gpu
def test_cli_bam(bam_check, golden, tmp_path):
    g = golden["toy"]
    out = str(tmp_path / "cli.bam")
    args = [EXE, "-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-alg", "ksw2", "-no_vcf"]
    r = subprocess.run(args + ["-bam", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, MCX_TIMING="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert b"[mcx_map_files] bam:" in r.stderr and b"0 lines made none" in r.stderr and b"made no BAM record" not in r.stderr
    reads = golden_reads(g)
    head, body, contigs = split_golden(g["sam"]["ksw2"])
    want, _ = host_encode(bam_check, reads, len(reads), body, contigs)
    check_stream(bam_stream(out)[0], head, contigs, body, want)
    # to stdout: the same stream
    r = subprocess.run(args + ["-bam", "-"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(out, "rb").read()
    # -sam x -bam y: one output, the later switch's
    x, y = str(tmp_path / "x.sam"), str(tmp_path / "y.bam")
    r = subprocess.run(args + ["-sam", x, "-bam", y], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and not os.path.exists(x) and open(y, "rb").read() == open(out, "rb").read()
    # -gpus 2 is refused before anything is opened
    bad = str(tmp_path / "bad.bam")
    r = subprocess.run(args + ["-bam", bad, "-gpus", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode != 0 and b"-bam" in r.stderr and not os.path.exists(bad)


@pytest.mark.gpu
def test_sharded_bam_is_refused(api, golden, tmp_path):
    g = golden["toy"]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1000)
    out = str(tmp_path / "sharded.bam")
    L = api.lib()
    links = (api.Exchange * 2)()
    assert L.mcx_exchange_local(2, links) == 0
    fo = api.FileOpts()
    L.mcx_file_opts_default(C.byref(fo))
    fo.device_sam = api.SAM_BAM
    fo.shard_rank, fo.shard_count = 0, 2
    fo.exchange = C.pointer(links[0])
    st = api.Stats()
    rc = L.mcx_map_files_ex(mp._h, g["r1"].encode(), g["r2"].encode(), C.byref(fo), out.encode(), C.byref(st))
    assert rc == api.ERR_UNSUPPORTED and b"BAM" in L.mcx_last_error() and not os.path.exists(out)
    L.mcx_exchange_local_free(links)
    mp.close(); ix.close()
