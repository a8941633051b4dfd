"""MD:Z strings made on the device: mcx_md_dev / mcx_md, the two formatters with a pool of strings, and mapcaller-mi355x -md on every output route.

GPU: the kernels against the host build of the same header (tests/hostemu/md_check.cpp, which tests/test_md_host.py holds against the definition restated in
Python) on every golden SAM and on the hand-made records — the hole cases on an index the project's own builder makes of the test's FASTA; the formatters'
text and records with the tags; the command line through -sam, -gpu_sam, -bgzf, -bam, the sorted, duplicate-marked, indexed BAM and -m."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from test_bam_host import decode_header, golden_parts
from test_md_host import (GOLDEN_CASES, MD_TAG, hand_batches, hand_genome, hand_want, host_md, host_sam_with_md, index_ref, load_case, load_fasta, md_check,  # noqa: F401 (md_check: a fixture)
                          md_of_line, part_lines, py_md, strings_of)
from test_sam_device import n_pairs_part

EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")


@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


_MAPPERS = {}


@pytest.fixture(scope="module")
def mapper_of(api):
    """index prefix -> a mapper on it (one per golden directory for the whole module)"""
    def get(prefix):
        if prefix not in _MAPPERS:
            ix = api.Index(prefix, device=0)
            _MAPPERS[prefix] = (ix, api.Mapper(ix, alg="nw", max_read_len=256, max_batch_reads=2000))
        return _MAPPERS[prefix][1]
    yield get
    for ix, mp in _MAPPERS.values():
        mp.close(); ix.close()
    _MAPPERS.clear()


def device_md(api, mp, si, n_lines):
    """mcx_md on the host arrays of si (staged inside: the kernels of mcx_md_dev): the size alone first, then into a buffer with guard bytes behind exactly that size"""
    L = api.lib()
    md_off = np.full(n_lines + 2, 0xA5A5A5A5, dtype=np.uint32)
    nb = C.c_uint64()
    rc = L.mcx_md(mp._h, C.byref(si), None, 0, md_off.ctypes.data, C.byref(nb))
    total = nb.value
    assert rc == (api.ERR_CAPACITY if total else 0) and int(md_off[n_lines]) == total and md_off[n_lines + 1] == 0xA5A5A5A5
    out = np.full(total + 64, 0xA5, dtype=np.uint8)
    assert L.mcx_md(mp._h, C.byref(si), out.ctypes.data, total, md_off.ctypes.data, C.byref(nb)) == 0, L.mcx_last_error()
    assert nb.value == total and (out[total:] == 0xA5).all()
    return out, md_off[:n_lines + 1]


def bam_records_of(api, mp, si):
    L = api.lib()
    nb, nd = C.c_uint64(), C.c_uint64()
    rec_off = np.zeros(si.n_reads + 1, dtype=np.uint64)
    L.mcx_bam_format(mp._h, C.byref(si), None, 0, rec_off.ctypes.data, C.byref(nb), C.byref(nd))
    out = np.zeros(nb.value + 1, dtype=np.uint8)
    assert L.mcx_bam_format(mp._h, C.byref(si), out.ctypes.data, nb.value, rec_off.ctypes.data, C.byref(nb), C.byref(nd)) == 0, L.mcx_last_error()
    assert nd.value == 0
    return out[:nb.value].tobytes()


def split_records(data, at=0):
    out = []
    while at < len(data):
        n = 4 + struct.unpack_from("<i", data, at)[0]
        out.append(data[at:at + n])
        at += n
    assert at == len(data)
    return out


# ---- device against host, and the two formatters ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_device_md_and_the_formatters_on_the_golden_sam(api, mapper_of, md_check, tmp_path, case):
    reads, body, contigs, extras, paired, prefix, genome = load_case(case, tmp_path)
    ref, mp = index_ref(prefix), mapper_of(prefix)
    n_pr = n_pairs_part(len(reads), paired)
    L = api.lib()
    for (si, n, keep), lines in zip(golden_parts(reads, n_pr, body, contigs, extras), part_lines(len(reads), n_pr, body, extras)):
        plain = split_records(bam_records_of(api, mp, si))
        pool, md_off = host_md(md_check, si, ref, keep)
        got, got_off = device_md(api, mp, si, len(lines))
        assert (got_off == md_off).all() and got[:int(md_off[-1])].tobytes() == pool[:int(md_off[-1])].tobytes()
        # SAM text with the pool: the host build's; BAM records: those without it, block_size grown, one trailing MD:Z tag with the Python value
        si.md, si.md_off = got.ctypes.data, got_off.ctypes.data
        want_text = host_sam_with_md(md_check, si, contigs, keep)
        nb = C.c_uint64()
        text = np.full(len(want_text) + 64, 0x5A, dtype=np.uint8)
        assert L.mcx_sam_format(mp._h, C.byref(si), text.ctypes.data, len(want_text), None, C.byref(nb)) == 0, L.mcx_last_error()
        assert nb.value == len(want_text) and text[:nb.value].tobytes() == want_text and (text[nb.value:] == 0x5A).all()
        with_md = split_records(bam_records_of(api, mp, si))
        # (records in line order: a read's own, then its extras — the pool's entries are the part's own lines first, then all extras)
        order = list(range(n))
        if extras is not None:
            x_index = np.ctypeslib.as_array(C.cast(si.x_index, C.POINTER(C.c_uint32)), shape=(n + 1,))
            order = [e for r in range(n) for e in [r] + [n + i for i in range(int(x_index[r]), int(x_index[r + 1]))]]
        assert len(plain) == len(with_md) == len(order) == len(lines)
        for a, b, e in zip(plain, with_md, order):
            md = md_of_line(lines[e], genome)
            tag = b"MDZ" + md + b"\0" if md else b""
            assert b == struct.pack("<i", len(a) - 4 + len(tag)) + a[4:] + tag, lines[e]
        si.md, si.md_off = None, None


@pytest.fixture(scope="module")
def hand_index(api, tmp_path_factory):
    """the hand-made genome as a FASTA file, indexed by the project's own builder"""
    d = tmp_path_factory.mktemp("md_hand")
    genome = hand_genome()
    fa = d / "hand.fa"
    fa.write_text("".join(f">{n}\n" + "\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + "\n" for n, s in genome))
    prefix = str(d / "idx")
    api.Index.build(str(fa), prefix, 0)
    ix = api.Index(prefix, device=0)
    mp = api.Mapper(ix, alg="nw", max_read_len=1000, max_batch_reads=2000)
    yield genome, prefix, mp
    mp.close(); ix.close()


def to_device(api, si, keep):
    """mcx_sam_in with every array of si in HBM (torch tensors, kept in the returned list)"""
    import torch
    dev = torch.device("cuda", 0)
    di, held = api.SamIn(), []
    by_ptr = {a.ctypes.data: a for a in keep if isinstance(a, np.ndarray)}
    for f, _ in api.SamIn._fields_:
        v = getattr(si, f)
        if f in ("n_reads", "paired"):
            setattr(di, f, v)
        elif v:
            t = torch.from_numpy(by_ptr[v].view(np.uint8).reshape(-1)).to(dev)
            held.append(t)
            setattr(di, f, t.data_ptr())
    return di, held


@pytest.mark.gpu
def test_md_dev_on_hand_made_records_holes_capacity_and_the_empty_batch(api, hand_index, md_check):
    import torch
    genome, prefix, mp = hand_index
    ref = index_ref(prefix)  # (the files the builder wrote: its .pac holds its own random bases inside the holes, its .amb the holes)
    assert ref["n_holes"] == 3 and [int(x) for x in ref["hole_len"][:3]] == [30, 3, 1]
    L = api.lib()
    dev = torch.device("cuda", 0)
    for si, keep, lines in hand_batches(genome, api):
        pool, md_off = host_md(md_check, si, ref, keep)
        want = hand_want(lines, genome)
        assert strings_of(pool, md_off) == want
        total, n = int(md_off[-1]), len(lines)
        di, held = to_device(api, si, keep)
        nb = C.c_uint64(77)
        d_off = torch.full((n + 2,), -1, dtype=torch.int32, device=dev)
        assert L.mcx_md_dev(mp._h, C.byref(di), None, 0, d_off.data_ptr(), C.byref(nb)) == api.ERR_CAPACITY and nb.value == total  # cap = 0 asks for the size
        d_md = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device=dev)
        nb = C.c_uint64()
        assert L.mcx_md_dev(mp._h, C.byref(di), d_md.data_ptr(), total - 1, d_off.data_ptr(), C.byref(nb)) == api.ERR_CAPACITY
        assert nb.value == total and bool((d_md == 0x5A).all())  # a short cap: the size again, and not a byte written
        assert L.mcx_md_dev(mp._h, C.byref(di), d_md.data_ptr(), total, d_off.data_ptr(), C.byref(nb)) == 0, L.mcx_last_error()
        assert nb.value == total and bool((d_md[total:] == 0x5A).all()) and int(d_off[n + 1]) == -1
        assert d_md[:total].cpu().numpy().tobytes() == pool[:total].tobytes()
        assert (d_off[:n + 1].cpu().numpy().view(np.uint32) == md_off).all()
        ms = mp.md_last_ms()
        assert all(m >= 0 for m in ms) and ms[0] > 0 and ms[2] > 0
        # the formatters' device forms with the pool in HBM: the host build's text, and records that end in the tag
        di.md, di.md_off = d_md.data_ptr(), d_off.data_ptr()
        si.md, si.md_off = pool.ctypes.data, md_off.ctypes.data
        want_text = host_sam_with_md(md_check, si, ["hA", "hB"], keep)
        d_text = torch.full((len(want_text) + 64,), 0x5A, dtype=torch.uint8, device=dev)
        assert L.mcx_sam_format_dev(mp._h, C.byref(di), d_text.data_ptr(), len(want_text), None, C.byref(nb)) == 0, L.mcx_last_error()
        assert nb.value == len(want_text) and d_text[:nb.value].cpu().numpy().tobytes() == want_text and bool((d_text[nb.value:] == 0x5A).all())
        rec_off = np.zeros(n + 1, dtype=np.uint64)
        assert md_check.md_check_bam(C.byref(si), None, 0, rec_off.ctypes.data) == -1
        want_recs = np.zeros(int(rec_off[-1]) + 1, dtype=np.uint8)
        assert md_check.md_check_bam(C.byref(si), want_recs.ctypes.data, int(rec_off[-1]), rec_off.ctypes.data) == int(rec_off[-1])
        d_recs = torch.full((int(rec_off[-1]) + 64,), 0x5A, dtype=torch.uint8, device=dev)
        nd = C.c_uint64()
        assert L.mcx_bam_format_dev(mp._h, C.byref(di), d_recs.data_ptr(), int(rec_off[-1]), None, C.byref(nb), C.byref(nd)) == 0, L.mcx_last_error()
        assert nb.value == int(rec_off[-1]) and nd.value == 0 and d_recs[:nb.value].cpu().numpy().tobytes() == want_recs[:nb.value].tobytes()
        for rec, md in zip(split_records(want_recs[:nb.value].tobytes()), want):
            assert rec.endswith(b"MDZ" + md + b"\0") if md else b"MDZ" not in rec[-8:]
        del held
    # no reads: no bytes, the offsets' one entry
    empty = api.SamIn()
    d_off = torch.full((2,), -1, dtype=torch.int32, device=dev)
    nb = C.c_uint64(5)
    assert L.mcx_md_dev(mp._h, C.byref(empty), None, 0, d_off.data_ptr(), C.byref(nb)) == 0 and nb.value == 0
    assert d_off.cpu().tolist() == [0, -1]


# ---- the command line --------------------------------------------------------------------------------------------------------------------
ROUTES = {
    "sam": (["-sam", "{out}"], "sam"), "gpu_sam": (["-sam", "{out}", "-gpu_sam"], "sam"), "bgzf": (["-sam", "{out}", "-bgzf"], "sam.gz"), "bam": (["-bam", "{out}"], "bam"),
    "sorted": (["-bam", "{out}", "-sort", "-markdup", "-index"], "bam"), "multi": (["-sam", "{out}", "-m"], "sam"),
}
_ROUTE_RUNS = {}
SEQ_LETTERS = "=ACMGRSVTWYHKDBN"


def bgzf_members(blob):
    """[(offset in the file, inflated bytes)] of a BGZF file's members"""
    out, at = [], 0
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12:at + 16] == b"BC\x02\x00"
        size = struct.unpack_from("<H", blob, at + 16)[0] + 1
        out.append((at, zlib.decompress(blob[at + 18:at + size - 8], -15)))
        assert zlib.crc32(out[-1][1]) == struct.unpack_from("<I", blob, at + size - 8)[0]
        at += size
    return out


def bam_lines(stream):
    """(header end, per record: its bytes without a trailing MD tag, the tag's value or None, (name, flag, contig, pos, CIGAR ops, SEQ))"""
    _, contigs, at = decode_header(stream)
    out = []
    for rec in split_records(stream, at):
        ref, pos, l_name, _, _, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
        p = 36 + l_name
        ops = [(w >> 4, "MIDNSHP=X"[w & 15]) for w in struct.unpack_from("<%dI" % n_cigar, rec, p)]
        p += 4 * n_cigar
        seq = "".join(SEQ_LETTERS[(rec[p + (k >> 1)] >> (0 if k & 1 else 4)) & 15] for k in range(l_seq))
        p += (l_seq + 1) // 2 + l_seq
        md, cut = None, len(rec)
        while p < len(rec):
            t = chr(rec[p + 2])
            if t == "Z":
                end = rec.index(b"\0", p + 3)
                assert rec[p:p + 2] == b"MD" and end + 1 == len(rec)  # the one string tag, and the last
                md, cut = rec[p + 3:end], p
                p = end + 1
            else:
                p += 3 + {"C": 1, "c": 1, "S": 2, "s": 2, "I": 4, "i": 4}[t]
        assert p == len(rec)
        plain = struct.pack("<i", cut - 4) + rec[4:cut]
        out.append((plain, md, (rec[36:36 + l_name - 1].decode("latin-1"), flag, contigs[ref][0] if ref >= 0 else "*", pos + 1, ops, seq)))
    return at, out


def route_run(golden, tmp_path_factory, route):
    """mc through one output route with -md and without: (key -> MD of every line, the output without -md, the output with -md less its tags, extra)"""
    if route in _ROUTE_RUNS:
        return _ROUTE_RUNS[route]
    g = golden["mc"]
    genome = dict(load_fasta(os.path.join(ROOT, "tests", "golden", "mc", "genome.fa.gz")))
    d = tmp_path_factory.mktemp("md_" + route)
    args, ext = ROUTES[route]
    outs = []
    for tag, more in (("md", ["-md"]), ("plain", [])):
        out = str(d / f"{tag}.{ext}")
        cmd = [EXE, "-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-alg", "ksw2", "-no_vcf", "-t", "2", "-batch", "1000"] + [a.format(out=out) for a in args] + more
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600, env=dict(os.environ, MCX_BGZF_BLOCK="4096"))
        outs.append(out)
    mds, extra = {}, None

    def note(key, md):
        mds.setdefault(key, []).append(md)
    if ext == "bam":
        s_md, s_plain = (b"".join(m[1] for m in bgzf_members(open(o, "rb").read())) for o in outs)
        at, recs = bam_lines(s_md)
        for plain, md, (name, flag, contig, pos, ops, seq) in recs:
            want = py_md(pos, ops, seq, genome[contig]).encode() if contig != "*" and ops else None
            assert md == want, (name, flag, md, want)
            note((name, flag & ~0x400, contig, pos, "".join(f"{n}{c}" for n, c in ops)), md)  # (-markdup's bit aside)
        stripped, plain_out = s_md[:at] + b"".join(r[0] for r in recs), s_plain
        extra = (outs[0], s_md, at, recs)
    else:
        t_md, t_plain = ((gzip.decompress(open(o, "rb").read()) if ext == "sam.gz" else open(o, "rb").read()).decode("latin-1") for o in outs)
        for line in t_md.split("\n"):
            if line and not line.startswith("@"):
                f = line.split("\t")
                md = [t[5:].encode() for t in f[11:] if t.startswith("MD:Z:")]
                want = md_of_line(line, genome)
                assert md == ([want] if want else []) and (not md or f[-1].startswith("MD:Z:")), line
                note((f[0], int(f[1]) | (4 if f[2] == "*" else 0), f[2], int(f[3]), f[5] if f[5] != "*" else ""), want)  # (a BAM record of an unmapped line carries flag bit 4)
        stripped, plain_out = MD_TAG.sub("", t_md), t_plain
    _ROUTE_RUNS[route] = (mds, plain_out, stripped, extra)
    return _ROUTE_RUNS[route]


def read_bai(data):
    """[(bin -> [(begin, end)], linear offsets)] per contig, from the format's description"""
    assert data[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", data, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", data, at)
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, at)
            bins[b] = [struct.unpack_from("<QQ", data, at + 8 + 16 * k) for k in range(n_chunk)]
            at += 8 + 16 * n_chunk
        n_intv, = struct.unpack_from("<i", data, at)
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, data, at + 4))))
        at += 4 + 8 * n_intv
    assert at in (len(data), len(data) - 8)
    return refs


def reg2bin(beg, end):
    end -= 1
    for first, shift in ((4681, 14), (585, 17), (73, 20), (9, 23), (1, 26)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_cli_md_on_every_route(golden, tmp_path_factory, route):
    mds, plain_out, stripped, extra = route_run(golden, tmp_path_factory, route)
    assert sum(m is not None for v in mds.values() for m in v) > 3000  # (mc: 4000 reads, 46 of them unmapped)
    assert stripped == plain_out  # without its tags the file is the one the route writes without -md
    base = route_run(golden, tmp_path_factory, "sam")[0]
    if route == "multi":  # every line of the run without -m is among them, with the same string
        assert all(k in mds and v[0] in mds[k] for k, v in base.items()) and sum(len(v) for v in mds.values()) > sum(len(v) for v in base.values())
    else:
        assert {k: sorted(v, key=repr) for k, v in mds.items()} == {k: sorted(v, key=repr) for k, v in base.items()}
    if route == "sorted":  # still sorted, duplicates flagged, and the index speaks of this file
        out, stream, at, recs = extra
        names = [c for c, _ in decode_header(stream)[1]]
        keys = [((1 << 40) if c == "*" else names.index(c), p) for _, _, (_, _, c, p, _, _) in recs]
        assert keys == sorted(keys)
        members = bgzf_members(open(out, "rb").read())
        u_of, u = {}, 0
        for coff, text in members:
            u_of[coff] = u
            u += len(text)
        starts, a = {}, at
        for rec in split_records(stream, at):
            starts[a] = rec
            a += len(rec)
        refs = read_bai(open(out + ".bai", "rb").read())
        assert len(refs) == len(names)
        covered = set()
        for tid, (bins, linear) in enumerate(refs):
            for b, chunks in bins.items():
                if b == 37450:
                    continue
                for beg, end in chunks:  # a chunk begins and ends where records of this contig begin and end (chunks that lie close are joined, so other bins' records may lie between the bin's)
                    a, stop = u_of[beg >> 16] + (beg & 0xFFFF), u_of[end >> 16] + (end & 0xFFFF)
                    while a < stop:
                        rec = starts[a]
                        ref, pos, _, _, bin_ = struct.unpack_from("<iiBBH", rec, 4)
                        assert ref == tid
                        up = bin_
                        while up != b and up:  # (a small bin's chunks are kept in a bin above it: a reader looks in every bin that overlaps its region)
                            up = (up - 1) >> 3
                        if up == b:
                            covered.add(a)
                        a += len(rec)
                    assert a == stop
        on_contig = {a for a, rec in starts.items() if struct.unpack_from("<i", rec, 4)[0] >= 0}
        assert covered == on_contig  # ... and every record on a contig is found through its bin
        for a, rec in starts.items():  # the bin of a record with its longer tag block is still that of its interval
            ref, pos, _, _, bin_, n_cigar, flag = struct.unpack_from("<iiBBHHH", rec, 4)
            if ref >= 0:
                l_name = rec[12]
                span = sum(w >> 4 for w in struct.unpack_from("<%dI" % n_cigar, rec, 36 + l_name) if (w & 15) in (0, 2, 3, 7, 8))
                assert bin_ == reg2bin(pos, pos + (span if span and not flag & 4 else 1))


@pytest.mark.gpu
def test_cli_md_is_refused_on_two_gpus(golden, tmp_path):
    g = golden["mc"]
    out = str(tmp_path / "o.sam")
    r = subprocess.run([EXE, "-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-no_vcf", "-sam", out, "-md", "-gpus", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0 and b"-md" in r.stderr.strip().split(b"\n")[-1]
    assert not os.path.exists(out)
