"""Read-group and mate tags made on the device: the two formatters with a mcx_sam_tags beside their input, the headers with an @RG line, and mapcaller-mi355x
-rg / -mc on every output route.

GPU: the kernels against the host build of the same headers (tests/hostemu/tags_check.cpp, which tests/test_tags_host.py holds against the rule restated in
Python) on the golden sets and the hand-made records under the four combinations of the switches; lines whose length crosses the kernels' staging only because
of the tags; the refusals; the command line through -sam, -gpu_sam, -bgzf, -bam and the sorted, duplicate-marked, indexed BAM."""
import bisect
import ctypes as C
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_bai_host import V, decoded, parse_bai, restated_index
from test_bam_host import decode_header, golden_parts
from test_md_device import bgzf_members, to_device
from test_md_host import GOLDEN_CASES, host_md, index_ref, load_case, md_check  # noqa: F401 (md_check: a fixture)
from test_sam_device import n_pairs_part
from test_tags_host import (CIGAR_300, COMBOS, RG_ARG, RG_ID, hand_batch, hand_slots, host_bam, host_sam, py_bam_tags, py_tags, split_records, tags_check,  # noqa: F401 (tags_check: a fixture)
                            tags_of)

EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
STAGE = 2048  # bytes of LDS a wavefront stages a line (a record) in: kSamStage of mcx_sam.hip, kBamStage of mcx_bam.hip
RG_LINE = b"@RG\tID:lane1\tSM:na12878\tLB:lib1\tPL:ILLUMINA"


@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


@pytest.fixture(scope="module")
def mapper(api):
    """a mapper on the mc index, which has three contigs: the formatters take nothing of an index but the contigs' names"""
    ix = api.Index(os.path.join(ROOT, "tests", "golden", "mc", "idx"), device=0)
    mp = api.Mapper(ix, alg="nw", max_read_len=256, max_batch_reads=2000)
    yield ix, mp
    mp.close(); ix.close()


_MAPPERS = {}


@pytest.fixture(scope="module")
def mapper_of(api):
    def get(prefix):
        if prefix not in _MAPPERS:
            ix = api.Index(prefix, device=0)
            _MAPPERS[prefix] = (ix, api.Mapper(ix, alg="nw", max_read_len=256, max_batch_reads=2000))
        return _MAPPERS[prefix][1]
    yield get
    for ix, mp in _MAPPERS.values():
        mp.close(); ix.close()
    _MAPPERS.clear()


def device_sam(api, mp, si, tg):
    """mcx_sam_format_tags on the host arrays of si (staged inside: the kernels): the size query (cap = 0) first, then into a buffer with guard bytes behind exactly that size"""
    L = api.lib()
    ref = C.byref(tg) if tg is not None else None
    nb = C.c_uint64()
    rc = L.mcx_sam_format_tags(mp._h, C.byref(si), ref, None, 0, None, C.byref(nb))
    total = nb.value
    assert rc == (api.ERR_CAPACITY if total else 0)
    out = np.full(total + 64, 0x5A, dtype=np.uint8)
    line_off = np.zeros(si.n_reads + 1, dtype=np.uint64)
    assert L.mcx_sam_format_tags(mp._h, C.byref(si), ref, out.ctypes.data, total, line_off.ctypes.data, C.byref(nb)) == 0, L.mcx_last_error()
    assert nb.value == total == int(line_off[-1]) and (out[total:] == 0x5A).all()
    return out[:total].tobytes(), line_off


def device_bam(api, mp, si, tg):
    L = api.lib()
    ref = C.byref(tg) if tg is not None else None
    nb, nd = C.c_uint64(), C.c_uint64()
    rc = L.mcx_bam_format_tags(mp._h, C.byref(si), ref, None, 0, None, C.byref(nb), C.byref(nd))
    total = nb.value
    assert rc == (api.ERR_CAPACITY if total else 0)
    out = np.full(total + 64, 0x5A, dtype=np.uint8)
    rec_off = np.zeros(si.n_reads + 1, dtype=np.uint64)
    assert L.mcx_bam_format_tags(mp._h, C.byref(si), ref, out.ctypes.data, total, rec_off.ctypes.data, C.byref(nb), C.byref(nd)) == 0, L.mcx_last_error()
    assert nb.value == total == int(rec_off[-1]) and nd.value == 0 and (out[total:] == 0x5A).all()
    return out[:total].tobytes(), rec_off


def check_against_host(api, mp, tags_check, si, contigs, keep, combos, md_pool=None):
    """both formatters on the device against the host build, under every combination of `combos`"""
    for name in combos:
        rg_id, mate_tags, with_md = COMBOS[name]
        if with_md:
            si.md, si.md_off = md_pool[0].ctypes.data, md_pool[1].ctypes.data
        tg = tags_of(api, rg_id, mate_tags, keep)
        want = host_sam(tags_check, si, tg, contigs)
        got, _ = device_sam(api, mp, si, tg)
        assert got == want, name
        want_recs = b"".join(host_bam(tags_check, si, tg))
        got_recs, _ = device_bam(api, mp, si, tg)
        assert got_recs == want_recs, name
        if rg_id:
            assert want.count(b"\tRG:Z:" + rg_id + b"\n") == want.count(b"\n") and want_recs.count(b"RGZ" + rg_id + b"\0") >= si.n_reads
        si.md, si.md_off = None, None


# ---- the kernels against the host build ---------------------------------------------------------------------------------------------------
KERNEL_CASES = {"toy-nw": list(COMBOS), "mc-ksw2": list(COMBOS), "long-nw": ["both", "both_md"], "se-nw": ["both", "rg"], "opt-pe250-ksw2": ["both"], "opt-pe150-nw": ["mc", "both_md"],
                "var-nw": ["both_md"]}


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in GOLDEN_CASES if c[0] in KERNEL_CASES], ids=lambda c: c[0])
def test_the_formatters_on_the_golden_parts(api, mapper_of, tags_check, md_check, tmp_path, case):
    reads, body, contigs, extras, paired, prefix, genome = load_case(case, tmp_path)
    mp = mapper_of(prefix)
    ref = index_ref(prefix)
    combos = KERNEL_CASES[case[0]]
    for si, n, keep in golden_parts(reads, n_pairs_part(len(reads), paired), body, contigs, None):
        pool = host_md(md_check, si, ref, keep) if "both_md" in combos else None
        check_against_host(api, mp, tags_check, si, contigs, keep, combos, pool)


@pytest.mark.gpu
@pytest.mark.parametrize("n_reads", [9, 2])
def test_the_formatters_on_hand_made_records(api, mapper, tags_check, n_reads):
    """an odd paired batch whose last read has no mate, a batch of two reads; an ID of 1 byte and of 255; a mate's MAPQ 0 and 255, its CIGAR of 1 operation and of 300"""
    ix, mp = mapper
    contigs = [c for c, _ in ix.chromosomes]
    for rg_id in (b"G", b"g" * 255, None):
        keep = []
        si = hand_batch(api, hand_slots()[:n_reads], True, keep)
        tg = tags_of(api, rg_id, True, keep)
        want = host_sam(tags_check, si, tg, contigs)
        got, _ = device_sam(api, mp, si, tg)
        assert got == want and (b"\tMC:Z:" + CIGAR_300.encode() + b"\tMQ:i:255") in got and b"\tMC:Z:50M\tMQ:i:0" in got
        got_recs, _ = device_bam(api, mp, si, tg)
        assert got_recs == b"".join(host_bam(tags_check, si, tg)) and (b"MCZ" + CIGAR_300.encode() + b"\0MQC\xff") in got_recs
    # with both switches off — a null mcx_sam_tags, or one that says nothing — the bytes of mcx_sam_format / mcx_bam_format
    L = api.lib()
    nb, nd = C.c_uint64(), C.c_uint64()
    plain, _ = device_sam(api, mp, si, None)
    old = np.zeros(len(plain) + 1, dtype=np.uint8)
    assert L.mcx_sam_format(mp._h, C.byref(si), old.ctypes.data, len(plain), None, C.byref(nb)) == 0 and old[:nb.value].tobytes() == plain
    assert device_sam(api, mp, si, api.SamTags())[0] == plain == host_sam(tags_check, si, None, contigs)
    recs, _ = device_bam(api, mp, si, None)
    old = np.zeros(len(recs) + 1, dtype=np.uint8)
    assert L.mcx_bam_format(mp._h, C.byref(si), old.ctypes.data, len(recs), None, C.byref(nb), C.byref(nd)) == 0 and old[:nb.value].tobytes() == recs
    assert device_bam(api, mp, si, api.SamTags())[0] == recs


@pytest.mark.gpu
def test_the_extras_of_multi_get_the_read_group_and_mate_tags_are_refused(api, mapper, tags_check):
    ix, mp = mapper
    contigs = [c for c, _ in ix.chromosomes]
    keep = []
    extras = [(0, (1, 700, "50M", 0, 99, 50)), (0, (0, 800, "20M1D30M", 0, 99, 50)), (2, (1, 60, "50M", 17, 73, 50))]
    si = hand_batch(api, hand_slots()[:4], True, keep, extras)
    tg = tags_of(api, RG_ID, False, keep)
    got, _ = device_sam(api, mp, si, tg)
    assert got == host_sam(tags_check, si, tg, contigs) and got.count(b"\tRG:Z:lane1\n") == 7
    assert device_bam(api, mp, si, tg)[0] == b"".join(host_bam(tags_check, si, tg))
    # mate_tags with a non-null x_index: MCX_ERR_UNSUPPORTED, the size not said, not a byte written
    L = api.lib()
    bad = tags_of(api, RG_ID, True, keep)
    out = np.full(4096, 0x5A, dtype=np.uint8)
    off = np.full(8, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    nb, nd = C.c_uint64(7), C.c_uint64(7)
    for f in (L.mcx_sam_format_tags, L.mcx_sam_format_tags_dev):
        nb.value = 7
        assert f(mp._h, C.byref(si), C.byref(bad), out.ctypes.data, out.size, off.ctypes.data, C.byref(nb)) == api.ERR_UNSUPPORTED and nb.value == 0
        assert b"-m" in L.mcx_last_error()
    for f in (L.mcx_bam_format_tags, L.mcx_bam_format_tags_dev):
        nb.value = nd.value = 7
        assert f(mp._h, C.byref(si), C.byref(bad), out.ctypes.data, out.size, off.ctypes.data, C.byref(nb), C.byref(nd)) == api.ERR_UNSUPPORTED and nb.value == 0 and nd.value == 0
    assert (out == 0x5A).all() and (off == 0x5A5A5A5A5A5A5A5A).all()


@pytest.mark.gpu
def test_the_device_forms_take_the_id_from_hbm(api, mapper, tags_check):
    """mcx_sam_format_tags_dev / mcx_bam_format_tags_dev: every pointer, the ID's too, a device pointer; and Mapper.sam_text / bam_records with the two arguments"""
    import torch
    ix, mp = mapper
    contigs = [c for c, _ in ix.chromosomes]
    L = api.lib()
    dev = torch.device("cuda", 0)
    keep = []
    si = hand_batch(api, hand_slots(), True, keep)
    tg = tags_of(api, RG_ID, True, keep)
    want, want_recs = host_sam(tags_check, si, tg, contigs), b"".join(host_bam(tags_check, si, tg))
    di, held = to_device(api, si, keep)
    d_id = torch.from_numpy(np.frombuffer(RG_ID, dtype=np.uint8).copy()).to(dev)
    dt = api.SamTags()
    dt.rg, dt.rg_len, dt.mate_tags = d_id.data_ptr(), len(RG_ID), 1
    nb, nd = C.c_uint64(), C.c_uint64()
    assert L.mcx_sam_format_tags_dev(mp._h, C.byref(di), C.byref(dt), None, 0, None, C.byref(nb)) == api.ERR_CAPACITY and nb.value == len(want)
    d_text = torch.full((len(want) + 64,), 0x5A, dtype=torch.uint8, device=dev)
    assert L.mcx_sam_format_tags_dev(mp._h, C.byref(di), C.byref(dt), d_text.data_ptr(), len(want), None, C.byref(nb)) == 0, L.mcx_last_error()
    assert d_text[:nb.value].cpu().numpy().tobytes() == want and bool((d_text[nb.value:] == 0x5A).all())
    assert L.mcx_bam_format_tags_dev(mp._h, C.byref(di), C.byref(dt), None, 0, None, C.byref(nb), C.byref(nd)) == api.ERR_CAPACITY and nb.value == len(want_recs)
    d_recs = torch.full((len(want_recs) + 64,), 0x5A, dtype=torch.uint8, device=dev)
    assert L.mcx_bam_format_tags_dev(mp._h, C.byref(di), C.byref(dt), d_recs.data_ptr(), len(want_recs), None, C.byref(nb), C.byref(nd)) == 0, L.mcx_last_error()
    assert d_recs[:nb.value].cpu().numpy().tobytes() == want_recs and bool((d_recs[nb.value:] == 0x5A).all())
    del held
    # the Python surface over the same batch
    n = si.n_reads
    off = np.ctypeslib.as_array(C.cast(si.off, C.POINTER(C.c_uint32)), shape=(n + 1,)).copy()
    name_off = np.ctypeslib.as_array(C.cast(si.name_off, C.POINTER(C.c_uint32)), shape=(n + 1,))
    bases = np.ctypeslib.as_array(C.cast(si.bases, C.POINTER(C.c_uint8)), shape=(int(off[-1]),)).copy()
    names_buf = np.ctypeslib.as_array(C.cast(si.names, C.POINTER(C.c_uint8)), shape=(int(name_off[-1]),)).tobytes()
    quals_buf = np.ctypeslib.as_array(C.cast(si.qual, C.POINTER(C.c_uint8)), shape=(int(off[-1]),)).tobytes()
    names = [names_buf[int(a):int(b)] for a, b in zip(name_off[:-1], name_off[1:])]
    quals = [quals_buf[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
    aln = np.ctypeslib.as_array(C.cast(si.aln, C.POINTER(C.c_uint8)), shape=(n * 64,)).view(api.ALN_DTYPE).copy()
    pool = next(a for a in keep if isinstance(a, np.ndarray) and a.ctypes.data == si.cigar)
    assert mp.sam_text(bases, off, names, quals, True, aln, pool, read_group=RG_ARG, mate_tags=True) == want
    assert mp.bam_records(bases, off, names, quals, True, aln, pool, read_group=RG_ARG, mate_tags=True) == (want_recs, 0)
    assert mp.sam_text(bases, off, names, quals, True, aln, pool) == host_sam(tags_check, si, None, contigs)


# ---- the staging border --------------------------------------------------------------------------------------------------------------------
def border_batch(api, n_ops, lead, keep):
    """two pairs: a first pair whose first name (of `lead` bytes) sets where the second pair begins within 16 bytes, then a read of 900 bases whose mate's CIGAR
    has n_ops operations"""
    slots = [(0, 100, "50M", 60, 99, 50), (0, 300, "50M", 60, 147, 50),
             (1, 1000, "20S860M20S", 47, 99, 900), (1, 1500, "1M1I" * (n_ops // 2) + "2M", 23, 147, 900)]
    names = [b"n" * lead, b"q", b"border/r900", b"border/r900"]
    return hand_batch(api, slots, True, keep, name_of=lambda i: names[i])


def border_case(api, tags_check, contigs, want_sh, delta, bam):
    """(mcx_sam_in, tags, keep) such that line (record) 2 begins at want_sh within 16 bytes and its length L has want_sh + L == STAGE + delta — only because of its tags"""
    measure = (lambda si, tg: [len(r) for r in host_bam(tags_check, si, tg)]) if bam else \
              (lambda si, tg: [len(l) + 1 for l in host_sam(tags_check, si, tg, contigs).split(b"\n")[:-1]])
    target = STAGE + delta - want_sh
    for n_ops in range(2, 700, 2):  # the mate's CIGAR brings the line near the border, the ID's length onto it
        keep = []
        id_len = target - measure(border_batch(api, n_ops, 4, keep), tags_of(api, b"x" * 100, True, keep))[2] + 100
        if id_len in range(1, 256):
            break
    else:
        raise AssertionError("no CIGAR brings the line to the border")
    for lead in range(4, 20):  # the first pair's first name moves the start of line 2, byte by byte
        keep = []
        si = border_batch(api, n_ops, lead, keep)
        tg = tags_of(api, b"x" * id_len, True, keep)
        lens = measure(si, tg)
        if (lens[0] + lens[1]) % 16 == want_sh:
            plain = measure(si, None)
            assert want_sh + lens[2] == STAGE + delta and plain[2] + 15 < STAGE - 64  # without its tags the line is staged wherever it begins, with room to spare
            return si, tg, keep
    raise AssertionError("no first pair puts line 2 at this place")


@pytest.mark.gpu
@pytest.mark.parametrize("bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("want_sh", [5, 12])
def test_lines_that_cross_the_staging_only_because_of_their_tags(api, mapper, tags_check, want_sh, bam):
    """sh + L <= kSamStage decides between the staged and the direct write: L - 1, L and L + 1 around it, at two places of the destination within 16 bytes"""
    ix, mp = mapper
    contigs = [c for c, _ in ix.chromosomes]
    for delta in (-1, 0, 1):
        si, tg, keep = border_case(api, tags_check, contigs, want_sh, delta, bam)
        if bam:
            got, off = device_bam(api, mp, si, tg)
            assert got == b"".join(host_bam(tags_check, si, tg))
        else:
            got, off = device_sam(api, mp, si, tg)
            assert got == host_sam(tags_check, si, tg, contigs)
        assert int(off[2]) % 16 == want_sh and want_sh + int(off[3]) - int(off[2]) == STAGE + delta  # (the staged buffer is 256-byte aligned: the text's offset is the address's)


# ---- the headers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_headers_end_with_the_read_group_line(api, mapper):
    ix, mp = mapper
    L = api.lib()
    plain = api.sam_header(ix)
    assert api.sam_header(ix, RG_ARG) == plain + RG_LINE + b"\n"
    nb = C.c_uint64()
    buf = C.create_string_buffer(len(plain) + 8)
    assert L.mcx_sam_header_rg(ix._h, None, buf, len(plain), C.byref(nb)) == 0 and buf.raw[:nb.value] == plain  # a null line: the old bytes
    assert L.mcx_sam_header_rg(ix._h, RG_LINE, buf, len(plain), C.byref(nb)) == api.ERR_CAPACITY and nb.value == len(plain) + len(RG_LINE) + 1
    assert L.mcx_sam_header_rg(ix._h, RG_ARG.encode(), None, 0, C.byref(nb)) == api.ERR_ARG  # (the line itself, with real TABs: not the argument's form)
    for is_sorted in (False, True):
        old = api.bam_header(ix, sorted=is_sorted)
        new = api.bam_header(ix, sorted=is_sorted, read_group=RG_ARG)
        l_text, = struct.unpack_from("<i", old, 4)
        text = old[8:8 + l_text]
        assert old[:4] == b"BAM\1" and text.endswith(b"\n") and (text.startswith(b"@HD\tVN:1.6\tSO:coordinate\n") == is_sorted)
        assert new == b"BAM\1" + struct.pack("<i", l_text + len(RG_LINE) + 1) + text + RG_LINE + b"\n" + old[8 + l_text:]
        assert decode_header(new)[1] == decode_header(old)[1]
        buf = C.create_string_buffer(len(old) + 8)
        assert L.mcx_bam_header_rg(ix._h, None, int(is_sorted), buf, len(old), C.byref(nb)) == 0 and buf.raw[:nb.value] == old
    assert L.mcx_bam_header_rg(ix._h, b"@RG\tSM:x", 0, None, 0, C.byref(nb)) == api.ERR_ARG and b"ID" in L.mcx_last_error()


# ---- the command line --------------------------------------------------------------------------------------------------------------------
ROUTES = {
    "sam": (["-sam", "{out}"], "sam"), "gpu_sam": (["-sam", "{out}", "-gpu_sam"], "sam"), "bgzf": (["-sam", "{out}", "-bgzf"], "sam.gz"), "bam": (["-bam", "{out}"], "bam"),
    "sorted": (["-bam", "{out}", "-sort", "-markdup", "-index", "-md"], "bam"),
}
_RUNS = {}


def cli_run(golden, tmp_path_factory, name, route, tagged):
    """the output file of golden set `name` through one route, with -rg ... -mc or without: its path and its bytes after gzip -d (a small -batch: several parts; small BGZF blocks)"""
    key = (name, route, tagged)
    if key not in _RUNS:
        g = golden[name]
        d = tmp_path_factory.mktemp(f"tags_{name}_{route}_{int(tagged)}")
        args, ext = ROUTES[route]
        out = str(d / f"out.{ext}")
        cmd = [EXE, "-i", g["prefix"], "-f", g["r1"]] + (["-f2", g["r2"]] if g["r2"] else []) + ["-alg", "ksw2", "-no_vcf", "-t", "2", "-batch", "1000"]
        cmd += [a.format(out=out) for a in args] + (["-rg", RG_ARG, "-mc"] if tagged else [])
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600, env=dict(os.environ, MCX_BGZF_BLOCK="4096"))
        blob = open(out, "rb").read()
        data = blob if ext == "sam" else gzip.decompress(blob) if ext == "sam.gz" else b"".join(m[1] for m in bgzf_members(blob))
        _RUNS[key] = (out, data)
    return _RUNS[key]


def sam_parts(data):
    lines = data.decode("latin-1").split("\n")
    assert lines[-1] == ""
    return [l for l in lines[:-1] if l.startswith("@")], [l for l in lines[:-1] if not l.startswith("@")]


def plain_body(golden, tmp_path_factory, name):
    """the lines of the set as the switch-less -sam run writes them: what the Python tags are computed from"""
    return sam_parts(cli_run(golden, tmp_path_factory, name, "sam", False)[1])[1]


def bam_parts(stream):
    text, contigs, at = decode_header(stream)
    return stream[:at], (text if isinstance(text, bytes) else text.encode("latin-1")), split_records(stream[at:])


def rec_key(rec):
    """(QNAME, first / second of its pair) of a record"""
    l_name, flag = rec[12], struct.unpack_from("<H", rec, 18)[0]
    return rec[36:36 + l_name - 1].decode("latin-1"), flag & 0xC0


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sam", "gpu_sam", "bgzf"])
def test_cli_tags_on_the_text_routes(golden, tmp_path_factory, route):
    head, body = sam_parts(cli_run(golden, tmp_path_factory, "mc", route, True)[1])
    plain_head, plain = sam_parts(cli_run(golden, tmp_path_factory, "mc", route, False)[1])
    assert plain == plain_body(golden, tmp_path_factory, "mc") and len(plain) == 4000
    assert head == plain_head + [RG_LINE.decode()]  # the header ends with the @RG line
    want = [l + py_tags(plain, i, True, RG_ID, True) for i, l in enumerate(plain)]
    bad = [(g, w) for g, w in zip(body, want) if g != w]
    assert len(body) == len(want) and not bad, bad[:2]
    assert sum("\tMC:Z:" in l for l in body) > 3000 and all(l.endswith("\tRG:Z:lane1") for l in body)


@pytest.mark.gpu
def test_cli_tags_in_the_bam_file(golden, tmp_path_factory):
    new_head, new_text, recs = bam_parts(cli_run(golden, tmp_path_factory, "mc", "bam", True)[1])
    old_head, old_text, plain_recs = bam_parts(cli_run(golden, tmp_path_factory, "mc", "bam", False)[1])
    plain = plain_body(golden, tmp_path_factory, "mc")
    assert len(recs) == len(plain_recs) == len(plain) == 4000
    l_text, = struct.unpack_from("<i", old_head, 4)
    assert new_head == b"BAM\1" + struct.pack("<i", l_text + len(RG_LINE) + 1) + old_head[8:8 + l_text] + RG_LINE + b"\n" + old_head[8 + l_text:]
    for i, (a, b) in enumerate(zip(plain_recs, recs)):  # the file differs only by the header line, the tag bytes and block_size
        tag = py_bam_tags(py_tags(plain, i, True, RG_ID, True))
        assert rec_key(a)[0] == plain[i].split("\t")[0] and b == struct.pack("<i", len(a) - 4 + len(tag)) + a[4:] + tag, plain[i]


@pytest.mark.gpu
def test_cli_tags_in_the_sorted_marked_indexed_bam_file(golden, tmp_path_factory):
    out, stream = cli_run(golden, tmp_path_factory, "mc", "sorted", True)
    new_head, _, recs = bam_parts(stream)
    old_head, _, plain_recs = bam_parts(cli_run(golden, tmp_path_factory, "mc", "sorted", False)[1])
    plain = plain_body(golden, tmp_path_factory, "mc")
    tags = {}
    for i, l in enumerate(plain):
        f = l.split("\t")
        tags[(f[0], int(f[1]) & 0xC0)] = py_bam_tags(py_tags(plain, i, True, RG_ID, True))
    assert len(tags) == len(plain) == len(recs) == len(plain_recs) == 4000
    l_text, = struct.unpack_from("<i", old_head, 4)
    assert old_head[8:].startswith(b"@HD\tVN:1.6\tSO:coordinate\n")
    assert new_head == b"BAM\1" + struct.pack("<i", l_text + len(RG_LINE) + 1) + old_head[8:8 + l_text] + RG_LINE + b"\n" + old_head[8 + l_text:]
    n_dup = 0
    for a, b in zip(plain_recs, recs):  # the order and the 0x400 bits of the run without the switches; every record the old one (its MD tag included) and the tags
        tag = tags[rec_key(a)]
        assert b == struct.pack("<i", len(a) - 4 + len(tag)) + a[4:] + tag, rec_key(a)
        n_dup += bool(struct.unpack_from("<H", b, 18)[0] & 0x400)
    assert n_dup > 0 and any(b"MDZ" in r for r in recs)
    # the .bai is the index of this file: the restatement of tests/test_bai_host.py over its records and its blocks
    members = bgzf_members(open(out, "rb").read())
    text = []
    u = 0
    for coff, inflated in members:
        if inflated:
            text.append((coff, u))
        u += len(inflated)
    starts = [s for _, s in text]
    tuples, at = [], len(new_head)
    for r in recs:
        k = bisect.bisect_right(starts, at) - 1
        tuples.append(decoded(r) + (V(text[k][0], at - starts[k]),))
        at += len(r)
    assert members[-1][1] == b"" and at == u
    n_ref = len(decode_header(stream)[1])
    assert parse_bai(open(out + ".bai", "rb").read()) == restated_index(n_ref, tuples, V(members[-1][0]))


@pytest.mark.gpu
def test_cli_single_reads_get_the_read_group_alone(golden, tmp_path_factory):
    head, body = sam_parts(cli_run(golden, tmp_path_factory, "se", "gpu_sam", True)[1])
    plain_head, plain = sam_parts(cli_run(golden, tmp_path_factory, "se", "gpu_sam", False)[1])
    assert head == plain_head + [RG_LINE.decode()] and body == [l + "\tRG:Z:lane1" for l in plain] and len(body) > 1000
    assert sam_parts(cli_run(golden, tmp_path_factory, "se", "sam", True)[1])[1] == body  # ... from the host formatter too


@pytest.mark.gpu
@pytest.mark.parametrize("what,args", [
    ("-mc with -m", ["-mc", "-m"]), ("no ID", ["-rg", r"@RG\tSM:x"]), ("no @RG", ["-rg", "ID:x"]), ("a newline", ["-rg", "@RG\\tID:x\nSM:y"]),
    ("-rg on two GPUs", ["-rg", RG_ARG, "-gpus", "2"]), ("-mc on two GPUs", ["-mc", "-gpus", "2"]),
])
def test_cli_refusals(golden, tmp_path, what, args):
    g = golden["mc"]
    out = str(tmp_path / "o.sam")
    r = subprocess.run([EXE, "-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-no_vcf", "-sam", out] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    last = r.stderr.strip().split(b"\n")[-1]
    assert r.returncode == 1 and last.startswith(b"Error!") and len(last) > 30, (what, r.stderr[-300:])
    assert (b"-mc" in last) if "-mc" in what else (b"-rg" in last)
    assert not os.path.exists(out)


@pytest.mark.gpu
def test_map_files_refuses_before_anything_is_opened(api, golden, tmp_path):
    g = golden["toy"]
    ix = api.Index(g["prefix"], device=0)
    out = str(tmp_path / "o.sam")
    mp = api.Mapper(ix, alg="nw", max_read_len=256, max_batch_reads=2000, multi=True)
    with pytest.raises(api.McxError) as e:
        mp.map_files(g["r1"], g["r2"], out, mate_tags=True)
    assert "(%d)" % api.ERR_UNSUPPORTED in str(e.value) and not os.path.exists(out)
    st = mp.map_files(g["r1"], g["r2"], out, read_group=RG_ARG)  # -rg works with -m
    head, body = sam_parts(open(out, "rb").read())
    assert head[-1] == RG_LINE.decode() and all(l.endswith("\tRG:Z:lane1") for l in body) and len(body) >= st["reads"]
    mp.close()
    mp = api.Mapper(ix, alg="nw", max_read_len=256, max_batch_reads=2000)
    os.remove(out)
    with pytest.raises(api.McxError) as e:
        mp.map_files(g["r1"], g["r2"], out, read_group="@RG\\tSM:x")
    assert "(%d)" % api.ERR_ARG in str(e.value) and not os.path.exists(out)
    fo = api.FileOpts()
    api.lib().mcx_file_opts_default(C.byref(fo))
    fo.shard_rank, fo.shard_count, fo.device_sam = 0, 2, api.SAM_MC
    x = api.Exchange()
    x.rank, x.size, x.allgather = 0, 2, api.ALLGATHER(lambda *a: 0)
    fo.exchange = C.pointer(x)
    st = api.Stats()
    for rg, bits in ((None, api.SAM_MC), (RG_LINE, 0)):
        fo.device_sam = bits
        rc = api.lib().mcx_map_files_rg(mp._h, g["r1"].encode(), g["r2"].encode(), C.byref(fo), rg, out.encode(), C.byref(st))
        assert rc == api.ERR_UNSUPPORTED and not os.path.exists(out)
    mp.close(); ix.close()
