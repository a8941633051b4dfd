"""-sort on the device: mcx_bam_sort_dev on synthetic record streams, and the file front end's sorted BAM (runs, plan, merge) on the golden sets.

The operation is held against a Python stable sort by the key (tests/test_bam_sort_host.py's formula), byte for byte, on torch tensors with guard bytes round
exactly n_bytes, for every source and destination offset class mod 16; the front end's inflated file against mcx_bam_header_sorted's bytes plus the stable
sort of the records the host build of the encoder (tests/hostemu/bam_check.cpp) makes of the golden lines — whatever the batch, block and chunk size."""
import ctypes as C
import glob
import hashlib
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import test_bgzf_resident as tb
from conftest import ROOT, SETS
from test_bam_device import bam_stream
from test_bam_host import bam_check, decode_header, golden_reads, host_encode, sq_lines  # noqa: F401 (fixtures)
from test_bam_sort_host import key_of, pack_record
from test_multi import read_extras
from test_sam_device import n_pairs_part, split_golden

EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
GUARD = 64
HD = b"@HD\tVN:1.6\tSO:coordinate\n"


@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


@pytest.fixture(scope="module")
def mapper(api, golden):
    ix = api.Index(golden["toy"]["prefix"], device=0)
    mp = api.Mapper(ix, alg="nw", max_batch_reads=2000)
    yield mp
    mp.close(); ix.close()


# ---- records and their order, in Python -----------------------------------------------------------------------------------------------
def split_records(data, at=0):
    out = []
    while at < len(data):
        n = 4 + struct.unpack_from("<I", data, at)[0]
        assert n >= 36 and at + n <= len(data)
        out.append(data[at:at + n])
        at += n
    return out


def rec_key(rec):
    ref_id, pos = struct.unpack_from("<ii", rec, 4)
    return key_of(ref_id, pos, struct.unpack_from("<H", rec, 18)[0])


def stable_sorted(records):
    return sorted(records, key=rec_key)  # (Python's sort is stable)


def random_record(rng, k, heavy_key=None):
    """lengths from the 38-byte minimum (a one-byte name, no bases) to beyond 2048 bytes"""
    if heavy_key:
        ref_id, pos, flag = heavy_key
    else:
        ref_id = rng.choice((-1, 0, 0, 1, 2, 24))
        pos = -1 if ref_id < 0 else rng.choice((0, 5, 5, 5, 1000, rng.randrange(0, 3000), (1 << 31) - 2))
        flag = rng.choice((0, 0x10, 0x63, 0x93)) | (4 if ref_id < 0 else 0)
    kind = rng.randrange(6)
    name = b"r" if kind == 0 else b"q%d" % k
    seq_len = (0, 0, 150, rng.randrange(1, 200), 250, rng.choice((1400, 2500, 5000)))[kind]
    rec = pack_record(ref_id, pos, flag, name=name, seq_len=seq_len, extra=b"" if kind == 0 else b"NMC\1")
    assert kind or len(rec) == 38
    return rec


def make_stream(rng, n):
    """n records in groups of 0, 1 and 3; 200 of 1000 share one key, forward and reverse lie on one position, refID -1 is mixed in"""
    recs = [random_record(rng, k, (1, 777, 0x10) if n >= 1000 and k % 5 == 0 else None) for k in range(n)]
    groups, k = [], 0
    while k < n:
        take = rng.choice((0, 1, 1, 1, 3))
        groups.append(recs[k:k + take])
        k += len(groups[-1])
    groups += [[], []] if n == 0 else [[]]
    return groups


def run_sort(api, mp, groups, src_shift=0, dst_shift=0, cap=None, want_rc=0, data=None, grp_off=None):
    """the call between guard bytes on both sides of both buffers: (rc, out bytes, keys, lens, n_records, the absolute addresses of source and destination)"""
    import torch
    if data is None:
        data = b"".join(r for g in groups for r in g)
        grp_off = np.cumsum([0] + [sum(len(r) for r in g) for g in groups]).astype(np.uint64)
    n_bytes = len(data)
    src = torch.full((GUARD + 16 + n_bytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    dst = torch.full((GUARD + 16 + n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    s0, d0 = GUARD + src_shift, GUARD + dst_shift
    if n_bytes:
        src[s0:s0 + n_bytes] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    off = torch.from_numpy(np.asarray(grp_off, dtype=np.uint64).view(np.int64).copy()).cuda()
    most = n_bytes // 36 + 1
    keys = torch.full((most,), -1, dtype=torch.int64, device="cuda")
    lens = torch.full((most,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = C.c_uint64(99)
    rc = api.lib().mcx_bam_sort_dev(mp._h, src.data_ptr() + s0, n_bytes, off.data_ptr(), len(grp_off) - 1, dst.data_ptr() + d0, n_bytes if cap is None else cap,
                                    keys.data_ptr(), lens.data_ptr(), C.byref(n))
    assert rc == want_rc, api.lib().mcx_last_error()
    got = dst.cpu().numpy()
    assert (got[:d0] == 0xA5).all() and (got[d0 + n_bytes:] == 0xA5).all()  # not a byte outside exactly n_bytes
    assert (src.cpu().numpy()[s0:s0 + n_bytes].tobytes()) == data
    return rc, got[d0:d0 + n_bytes].tobytes(), keys.cpu().numpy().view(np.uint64), lens.cpu().numpy(), n.value, src.data_ptr() + s0, dst.data_ptr() + d0, got


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_the_operation_is_a_stable_sort_by_the_key(api, mapper, n):
    rng = random.Random(1000 + n)
    groups = make_stream(rng, n)
    records = [r for g in groups for r in g]
    assert len(records) == n and {len(g) for g in groups} >= ({0} if n < 3 else {0, 1, 3})
    want = stable_sorted(records)
    if n >= 1000:  # (the stream is what the issue asks for)
        keys = [rec_key(r) for r in records]
        assert max(keys.count(k) for k in set(keys)) >= 200
        assert any(k >> 32 == 0xFFFFFFFF for k in keys) and any((k ^ 1) in set(keys) for k in keys)
        assert min(map(len, records)) == 38 and max(map(len, records)) > 2048
    src_classes, dst_classes = set(), set()
    for shift in range(16) if n in (65, 1000) else (0, 5):
        rc, out, keys, lens, n_rec, src_at, dst_at, _ = run_sort(api, mapper, groups, src_shift=shift, dst_shift=(shift * 7 + 3) % 16)
        assert n_rec == n
        assert out == b"".join(want)
        assert [int(k) for k in keys[:n]] == [rec_key(r) for r in want] and [int(v) for v in lens[:n]] == [len(r) for r in want]
        at = 0
        for r in records:
            src_classes.add((src_at + at) % 16)
            at += len(r)
        at = 0
        for r in want:
            dst_classes.add((dst_at + at) % 16)
            at += len(r)
    if n >= 65:
        assert len(src_classes) == 16 and len(dst_classes) == 16  # every offset class mod 16, on both sides
    assert all(v >= 0 for v in mapper.bam_sort_last_ms())


@pytest.mark.gpu
def test_the_python_wrapper(api, mapper):
    import torch
    groups = make_stream(random.Random(7), 64)
    records = [r for g in groups for r in g]
    recs = torch.from_numpy(np.frombuffer(b"".join(records), dtype=np.uint8).copy()).cuda()
    off = torch.from_numpy(np.cumsum([0] + [sum(len(r) for r in g) for g in groups]).astype(np.int64)).cuda()
    keys, lens = torch.zeros(len(records), dtype=torch.int64, device="cuda"), torch.zeros(len(records), dtype=torch.int32, device="cuda")
    out, n = mapper.bam_sort(recs, off, keys, lens)
    want = stable_sorted(records)
    assert n == 64 and out.cpu().numpy().tobytes() == b"".join(want)
    assert [int(v) for v in keys.cpu().numpy().view(np.uint64)] == [rec_key(r) for r in want]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["chain leaves its group", "block_size 8", "offsets do not reach n_bytes", "offsets descend"])
def test_broken_input_is_an_argument_error(api, mapper, how):
    rng = random.Random(3)
    records = [random_record(rng, k) for k in range(40)]
    data = b"".join(records)
    ends = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
    if how == "chain leaves its group":
        ends[20] += 5  # group 19 ends inside record 20: its chain runs out of it
    elif how == "block_size 8":
        at = int(ends[7])
        data = data[:at] + struct.pack("<I", 8) + data[at + 4:]
    elif how == "offsets do not reach n_bytes":
        ends = ends[:-1]
    else:
        ends[10], ends[11] = ends[11], ends[10]
    rc, out, keys, lens, n_rec, _, _, whole = run_sort(api, mapper, None, src_shift=3, dst_shift=9, want_rc=api.ERR_ARG, data=data, grp_off=ends)
    assert (whole == 0xA5).all() and n_rec == 0  # the output is untouched too


@pytest.mark.gpu
def test_capacity_and_the_empty_call(api, mapper):
    import torch
    groups = make_stream(random.Random(11), 10)
    n_bytes = sum(len(r) for g in groups for r in g)
    rc, out, _, _, n_rec, _, _, whole = run_sort(api, mapper, groups, cap=n_bytes - 1, want_rc=api.ERR_CAPACITY)
    assert (whole == 0xA5).all() and n_rec == 0
    L = api.lib()
    n = C.c_uint64(5)
    d = torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    assert L.mcx_bam_sort_dev(mapper._h, d.data_ptr(), 100, d.data_ptr(), 0, d.data_ptr() + 128, 100, None, None, C.byref(n)) == 0 and n.value == 0  # no group: nothing to do
    assert bool((d == 0xA5).all())
    assert L.mcx_bam_sort_dev(None, d.data_ptr(), 100, d.data_ptr(), 1, d.data_ptr(), 100, None, None, C.byref(n)) == api.ERR_ARG
    assert L.mcx_bam_sort_dev(mapper._h, None, 100, d.data_ptr(), 1, d.data_ptr(), 100, None, None, C.byref(n)) == api.ERR_ARG
    assert L.mcx_bam_sort_dev(mapper._h, d.data_ptr(), 100, None, 1, d.data_ptr(), 100, None, None, C.byref(n)) == api.ERR_ARG
    assert L.mcx_bam_sort_dev(mapper._h, d.data_ptr(), 100, d.data_ptr(), 1, None, 100, None, None, C.byref(n)) == api.ERR_ARG
    ms = (C.c_float * 4)()
    assert L.mcx_bam_sort_last_ms(mapper._h, None) == api.ERR_ARG and L.mcx_bam_sort_last_ms(None, ms) == api.ERR_ARG


@pytest.mark.gpu
def test_the_sorted_header(api, golden):
    ix = api.Index(golden["mc"]["prefix"], device=0)
    plain, got = api.bam_header(ix), api.bam_header(ix, sorted=True)
    text, contigs, at = decode_header(got)
    plain_text, plain_contigs, plain_at = decode_header(plain)
    assert text == HD + plain_text and contigs == plain_contigs and got[at:] == plain[plain_at:] and at == len(got)
    buf, nb = np.full(len(got), 0xA5, dtype=np.uint8), C.c_uint64()
    assert api.lib().mcx_bam_header_sorted(ix._h, buf.ctypes.data, len(got) - 1, C.byref(nb)) == api.ERR_CAPACITY and nb.value == len(got) and (buf == 0xA5).all()
    assert api.lib().mcx_bam_header_sorted(None, buf.ctypes.data, len(got), C.byref(nb)) == api.ERR_ARG
    ix.close()


# ---- the front end ---------------------------------------------------------------------------------------------------------------------
def map_sorted(api, g, alg, out, batch, multi=False, files=None, **kw):
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg=alg, multi=multi, max_batch_reads=batch)
    header = api.bam_header(ix, sorted=True)
    r1, r2 = files or (g["r1"], g["r2"])
    try:
        st = mp.map_files(r1, r2, out, bam=True, sort=True, **kw)
        return st, mp.last_route(), mp.sort_stats(), header
    finally:
        mp.close(); ix.close()


_WANT = {}


def want_sorted(bam_check, golden, name, alg, multi=False):
    """the stable sort of the records the host build makes of the golden lines (once per set)"""
    key = (name, alg, multi)
    if key not in _WANT:
        g = golden[name]
        reads = golden_reads(g)
        _, body, contigs = split_golden(g["sam"][alg])
        data, dropped = host_encode(bam_check, reads, n_pairs_part(len(reads), SETS[name]), body, contigs, read_extras(name, alg) if multi else None)
        assert dropped == 0
        _WANT[key] = (split_records(data), len(body))
    records, n_lines = _WANT[key]
    return b"".join(stable_sorted(records)), records, n_lines


def no_temporary_file(tmp_path):
    return not glob.glob(str(tmp_path / "*.tmp")) and not glob.glob(str(tmp_path / "*.sort*"))


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ("nw", "ksw2"))
def test_sorted_bam_of_the_golden_set_mc(api, bam_check, golden, tmp_path, monkeypatch, alg):
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    monkeypatch.setenv("MCX_SORT_CHUNK", "200000")
    want, records, n_lines = want_sorted(bam_check, golden, "mc", alg)
    # the set exercises what it is here for: 4000 lines, 3 contigs, unmapped lines, tied keys
    keys = [rec_key(r) for r in records]
    mapped = [k for k in keys if k >> 32 != 0xFFFFFFFF]
    tied = sum(1 for k in set(mapped) if mapped.count(k) > 1)
    assert n_lines == 4000 and len({k >> 32 for k in mapped}) == 3
    assert (len(keys) - len(mapped), tied) == {"ksw2": (46, 9), "nw": (75, 8)}[alg]  # (unmapped lines, keys that several mapped lines share)
    assert want != b"".join(records)
    out = str(tmp_path / "o.bam")
    st, route, stats, header = map_sorted(api, golden["mc"], alg, out, 1000)
    assert st["reads"] == 4000 and route[0] & api.ROUTE_SORT and route[0] & api.ROUTE_BAM
    assert stats["runs"] >= 3 and stats["chunks"] >= 3 and stats["slices_inside_a_block"] >= 1, stats
    stream, members = bam_stream(out)
    assert stream[:len(header)] == header and header[8:8 + len(HD)] == HD
    assert stream[len(header):] == want
    assert no_temporary_file(tmp_path)


@pytest.mark.gpu
def test_the_file_does_not_depend_on_batch_or_chunk_size(api, bam_check, golden, tmp_path, monkeypatch):
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    want, _, _ = want_sorted(bam_check, golden, "mc", "ksw2")
    streams = []
    for k, (batch, chunk) in enumerate(((1000, "200000"), (1 << 14, None), (400, "50000"))):
        if chunk:
            monkeypatch.setenv("MCX_SORT_CHUNK", chunk)
        else:
            monkeypatch.delenv("MCX_SORT_CHUNK", raising=False)
        out = str(tmp_path / f"o{k}.bam")
        st, route, stats, header = map_sorted(api, golden["mc"], "ksw2", out, batch)
        if chunk is None:
            assert stats["runs"] == 1 and stats["chunks"] == 1, stats
        streams.append(bam_stream(out)[0])
        assert streams[-1] == header + want
    assert streams[0] == streams[1] == streams[2]


@pytest.mark.gpu
def test_sorted_bam_with_multi(api, bam_check, golden, tmp_path, monkeypatch):
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    monkeypatch.setenv("MCX_SORT_CHUNK", "200000")
    want, records, n_lines = want_sorted(bam_check, golden, "mc", "ksw2", multi=True)
    assert len(records) > n_lines
    out = str(tmp_path / "m.bam")
    st, route, stats, header = map_sorted(api, golden["mc"], "ksw2", out, 1000, multi=True)
    assert bam_stream(out)[0] == header + want


@pytest.mark.gpu
def test_sorted_bam_single_end(api, bam_check, golden, tmp_path, monkeypatch):
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    monkeypatch.setenv("MCX_SORT_CHUNK", "100000")
    want, _, _ = want_sorted(bam_check, golden, "se", "ksw2")
    out = str(tmp_path / "se.bam")
    st, route, stats, header = map_sorted(api, golden["se"], "ksw2", out, 400)
    assert stats["runs"] >= 2
    assert bam_stream(out)[0] == header + want


@pytest.mark.gpu
def test_sorted_bam_on_the_resident_route(api, bam_check, golden, tmp_path, monkeypatch):
    monkeypatch.setenv("MCX_BGZF_BLOCK", "4096")
    monkeypatch.setenv("MCX_RESIDENT_LAUNCH_BYTES", "65536")
    monkeypatch.setenv("MCX_SORT_CHUNK", "100000")
    g = golden["toy"]
    files = []
    for k, t in enumerate(tb.read_texts(g, "toy")):
        files.append(str(tmp_path / f"toy_{k + 1}.fq.gz"))
        tb.write_bgzf(files[-1], t, 3000)
    want, _, _ = want_sorted(bam_check, golden, "toy", "ksw2")
    out = str(tmp_path / "res.bam")
    st, route, stats, header = map_sorted(api, g, "ksw2", out, 800, files=files, device_inflate=True, device_parse=True)
    everything = tb.ALL_FOUR | api.ROUTE_BGZF | api.ROUTE_BAM | api.ROUTE_SORT
    assert route == (everything, everything)
    assert bam_stream(out)[0] == header + want
    assert no_temporary_file(tmp_path)


@pytest.mark.gpu
def test_two_runs_give_the_same_sorted_file(api, golden, tmp_path, monkeypatch):
    monkeypatch.setenv("MCX_SORT_CHUNK", "300000")
    digests = []
    for k in range(2):
        out = str(tmp_path / f"run{k}.bam")
        map_sorted(api, golden["mc"], "nw", out, 1000)
        digests.append(hashlib.md5(open(out, "rb").read()).hexdigest())
    assert digests[0] == digests[1]


@pytest.mark.gpu
def test_the_temporary_file_is_gone_after_a_run_that_fails(api, golden, tmp_path):
    g = golden["toy"]
    # the output cannot be written: nothing is left behind, not even beside it
    with pytest.raises(Exception):
        map_sorted(api, g, "ksw2", str(tmp_path / "no_such_dir" / "o.bam"), 1000)
    assert no_temporary_file(tmp_path) and not os.path.exists(str(tmp_path / "no_such_dir"))
    # the input breaks off in the middle of the run (file 2 ends inside a record, after the temporary file was made)
    text = open(g["r2"], "rb").read()
    cut = str(tmp_path / "r2_cut.fq")
    open(cut, "wb").write(text[:len(text) // 2 + 7])
    out = str(tmp_path / "cut.bam")
    try:
        map_sorted(api, g, "ksw2", out, 400, files=(g["r1"], cut))
    except Exception:
        pass
    assert no_temporary_file(tmp_path)


@pytest.mark.gpu
def test_the_refusals(api, golden, tmp_path):
    g = golden["toy"]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1000)
    L = api.lib()
    out = str(tmp_path / "refused.bam")

    def call(device_sam, append=0, shards=None):
        fo = api.FileOpts()
        L.mcx_file_opts_default(C.byref(fo))
        fo.device_sam, fo.append_sam = device_sam, append
        links = None
        if shards:
            links = (api.Exchange * 2)()
            assert L.mcx_exchange_local(2, links) == 0
            fo.shard_rank, fo.shard_count, fo.exchange = 0, 2, C.pointer(links[0])
        st = api.Stats()
        rc = L.mcx_map_files_ex(mp._h, g["r1"].encode(), g["r2"].encode(), C.byref(fo), out.encode(), C.byref(st))
        err = L.mcx_last_error()
        if links is not None:
            L.mcx_exchange_local_free(links)
        assert not os.path.exists(out) and no_temporary_file(tmp_path)
        return rc, err

    rc, err = call(api.SAM_SORT | api.SAM_DEVICE | api.SAM_BGZF)
    assert rc == api.ERR_UNSUPPORTED and b"needs -bam" in err
    rc, err = call(api.SAM_SORT | api.SAM_BAM, append=1)
    assert rc == api.ERR_UNSUPPORTED and b"cannot be appended to" in err
    rc, err = call(api.SAM_SORT | api.SAM_BAM, shards=2)
    assert rc == api.ERR_UNSUPPORTED and b"sharded" in err and b"sorted" in err
    mp.close(); ix.close()


@pytest.mark.gpu
def test_cli_sort(api, bam_check, golden, tmp_path):
    g = golden["toy"]
    want, _, _ = want_sorted(bam_check, golden, "toy", "ksw2")
    out = str(tmp_path / "cli.bam")
    args = [EXE, "-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-alg", "ksw2", "-no_vcf", "-batch", "1000"]
    env = dict(os.environ, MCX_TIMING="1", MCX_SORT_CHUNK="100000", TMPDIR=str(tmp_path))
    r = subprocess.run(args + ["-bam", out, "-sort"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert b"[mcx_map_files] sort:" in r.stderr and b" runs" in r.stderr and b"chunks" in r.stderr and b"bytes read back" in r.stderr
    stream, _ = bam_stream(out)
    text, contigs, at = decode_header(stream)
    assert text.split(b"\n")[0] == HD[:-1]  # the header's first line
    assert stream[at:] == want
    # to stdout: the same file, and nothing left in $TMPDIR
    r = subprocess.run(args + ["-sort", "-bam", "-"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(out, "rb").read()
    assert no_temporary_file(tmp_path)
    # the three refusals, in words, before anything is opened
    bad = str(tmp_path / "bad.bam")
    for extra, words in ((["-sam", bad, "-sort"], b"needs -bam"), (["-bam", bad, "-sort", "-gpus", "2"], b"-gpus"), (["-bam", bad, "-sort", "-f", g["r1"], "-f2", g["r2"]], b"cannot be appended to")):
        r = subprocess.run(args + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode != 0 and b"-sort" in r.stderr and words in r.stderr, r.stderr[-500:]
        assert not os.path.exists(bad)
