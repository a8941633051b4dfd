"""Ordinary gzip streams inflated on the device (mcx_gunzipper_*, mcx_gunzip_round_dev / _text_dev, mcx_gz_inflate_dev; -gpu_gz on the resident route).

The kernels are held against the host build of the same header (tests/hostemu/gz_dev_check.cpp: mcx_gz_dev.h with one lane) round by round — text, end bit,
CRC-32, starts found, chain, overflows — on the vectors of tests/gz_dev_vectors.py, each of which is zlib's own output; the reader by itself against gzip.open
on the golden read files; and the front end with device_gz against the golden SAM, against the host route where the switch does not apply, and on damaged files."""
import ctypes as C
import gzip
import os
import subprocess
import threading

import numpy as np
import pytest

import gz_dev_vectors as V
import test_bgzf_resident as tr
from conftest import ROOT, sam_diff

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available()
    from mapcaller_amd import api as a
    a.lib()
    return a


def device_rounds(api, raw, stretch, stretches, arena=0, z=None):
    """V.rounds_of through the object (z: the caller's, reset here for a new member): ([figures], text, [ms])"""
    import contextlib
    import torch
    d_src = torch.frombuffer(bytearray(raw + b"\0" * 8), dtype=torch.uint8).cuda()
    ms = []
    with (contextlib.nullcontext(z) if z is not None else api.Gunzipper(0, stretch, stretches, arena)) as z:
        z.reset()
        at = [0]

        def rnd(src, bit, end, info):
            got = z.round_dev(d_src, at[0], len(src), bit, bool(end))
            C.memmove(C.byref(info), C.byref(got), C.sizeof(info))
            at[0] += info.end_bit >> 3

        def txt(info):
            d_dst = torch.full((info.text_bytes + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            mine = api.GzRound()
            C.memmove(C.byref(mine), C.byref(info), C.sizeof(info))
            z.text_dev(d_dst[:info.text_bytes] if info.text_bytes else d_dst[:1], mine)
            C.memmove(C.byref(info), C.byref(mine), C.sizeof(info))
            ms.append(tuple(info.ms))
            host = d_dst.cpu().numpy()
            assert (host[info.text_bytes:] == 0x5A).all()  # (nothing behind the text)
            return host[:info.text_bytes].tobytes()
        figs, text = V.rounds_of(rnd, txt, raw, stretch)
    return figs, text, ms


def raw_of(blob):
    """the deflate stream of a one-member file made by the vectors"""
    return blob[V.header_len(blob):-8]


KERNEL_CASES = [("v1", lambda: V.v1()[:2], 4096, 32, 0.75, None), ("v2 level 1", lambda: V.v2(1), 65536, 64, 0.75, None), ("v2 level 6", lambda: V.v2(6), 65536, 64, 0.75, None),
                ("v2 level 9", lambda: V.v2(9), 65536, 64, 0.75, None), ("v3", lambda: V.v3()[:2], 65536, 32, None, 12), ("v4", lambda: V.v4(), 65536, 32, None, None)]
KERNEL_CASES += [(name, (lambda name=name: next((f, t) for n, f, t, _, _ in V.v5() if n == name)), s, n, None, None) for name, s, n in
                 (("stored", 65536, 8), ("fixed", 16384, 8), ("tiny", 4096, 4), ("named", 16384, 8), ("urandom", 65536, 8))]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_kernels_equal_the_host_build_round_by_round(api, case):
    """Every vector through mcx_gunzip_round_dev / mcx_gunzip_text_dev: zlib's text, and every round's end_bit, text_bytes, crc32, final, status, stretches,
    starts, chain and overflowed as the host build has them.  So that the parallel path cannot hide behind stretch 0: V1 and V2 have chain >= 3/4 stretches in
    every full round, V3 a chain of at least 12 of its 21 stretches; V4 has a stretch out of room in some round."""
    name, make, stretch, stretches, chain_share, chain_min = case
    blob, text = make()
    raw = raw_of(blob)
    want_figs, want_text = V.host_rounds(raw, stretch, stretches)
    assert want_text == text, name  # (the host build against zlib)
    figs, got, ms = device_rounds(api, raw, stretch, stretches)
    print(name, "rounds", len(figs), "chain / stretches", [(f[7], f[5]) for f in figs], "ms", [tuple(round(x, 3) for x in m) for m in ms][:4])
    assert got == text, name
    assert figs == want_figs, (name, [(a, b) for a, b in zip(figs, want_figs) if a != b][:2])
    assert figs[-1][3] == 1 and all(f[4] == V.OK for f in figs)
    if chain_share:
        full = [f for f in figs if f[5] == stretches and not f[3]] if name == "v1" else figs
        assert full and all(f[7] >= chain_share * f[5] for f in full), [(f[7], f[5]) for f in figs]
    if chain_min:
        assert len(figs) == 1 and figs[0][5] >= 21 and figs[0][7] >= chain_min, figs
    if name == "v4":
        assert any(f[8] >= 1 for f in figs), figs


def test_kernels_on_members_behind_one_another(api):
    """V5's four members with an empty one among them through the two calls, ONE object, mcx_gunzipper_reset between members: every member's text and every
    round's figures as the host build has them (a window left over from the member before would show in both)"""
    blob, text = next((f, t) for n, f, t, _, _ in V.v5() if n == "members")
    members = V.members_of(blob)
    assert len(members) == 5 and b"".join(t for _, t in members) == text and [len(t) for _, t in members].count(0) == 1
    with api.Gunzipper(0, 16384, 8) as z:
        for k, (raw, want) in enumerate(members):
            want_figs, host_text = V.host_rounds(raw, 16384, 8)
            figs, got, _ = device_rounds(api, raw, 16384, 8, z=z)
            assert host_text == got == want and figs == want_figs and figs[-1][3] == 1, (k, figs, want_figs)


@pytest.mark.parametrize("name", ["toy", "var", "mc", "long"])
def test_the_reader_on_the_golden_read_files(api, name):
    p = os.path.join(GOLD, name, "r1.fq.gz")
    want = gzip.open(p, "rb").read()
    for stretch, stretches in ((0, 0), (4096, 16)):
        r, got = api.gz_inflate_dev(p, 0, stretch, stretches, len(want))
        assert r == len(want) and got == want, (name, stretch, r)


def test_the_reader_on_odd_files_and_damaged_ones(api, tmp_path):
    """V5 through mcx_gz_inflate_dev — stored and fixed blocks, a 15-byte text, a header with name and comment, four members with an empty one among them,
    bytes in which no start is accepted — and the documented return values on the damaged list, with what the host build delivers before the damage"""
    for name, blob, text, stretch, stretches in V.v5():
        p = tmp_path / "odd.gz"
        p.write_bytes(blob)
        r, got = api.gz_inflate_dev(str(p), 0, stretch, stretches, len(text))
        assert r == len(text) and got == text, (name, r)
    for name, blob, ret, text in V.damaged():
        p = tmp_path / "bad.gz"
        p.write_bytes(blob)
        r, got = api.gz_inflate_dev(str(p), 0, 16384, 8, len(text))
        want = V.host_file(blob, 16384, 8, len(text))
        assert r == ret and (r, got) == (want[0], want[1]), (name, r, len(got), len(want[1]))
        if name in ("trailer", "cut"):
            assert text.startswith(got) and len(got) < len(text), name
    assert api.gz_inflate_dev(str(tmp_path / "none.gz"), 0) == (-1, b"")
    # the next round's bytes are in HBM when it begins: every round of a one-member file but its first
    blob, text = V.v1()
    p = tmp_path / "v1.gz"
    p.write_bytes(blob)
    r, got = api.gz_inflate_dev(str(p), 0, 4096, 32, len(text))
    rounds, hits = api.gz_inflate_dev_last()
    assert r == len(text) and got == text and (rounds, hits) == V.host_staging(blob, 4096, 32) and rounds >= 5 and hits == rounds - 1, (rounds, hits)


def test_the_object_refuses_what_breaks_its_contract(api):
    import torch
    with pytest.raises(api.McxError):
        api.Gunzipper(0, 1000)
    blob, text = V.v2(6)
    raw = raw_of(blob)[:200_000]
    d_src = torch.frombuffer(bytearray(raw + b"\0" * 8), dtype=torch.uint8).cuda()
    with api.Gunzipper(0, 65536, 4) as z:
        with pytest.raises(api.McxError):
            api._check(api.lib().mcx_gunzip_round_dev(z._h, d_src.data_ptr(), len(raw), 8, 1, C.byref(api.GzRound())), "mcx_gunzip_round_dev")
        # bytes that end inside a block and are not the file's end: pass more
        info = z.round_dev(d_src, 0, 20_000, 0, False)
        assert info.status == api.GZ_MORE and info.text_bytes == 0 and info.chain == 0
        z.reset()
        info = z.round_dev(d_src, 0, len(raw), 0, True)
        assert info.status == api.GZ_OK and info.text_bytes > 0
        small = torch.zeros(16, dtype=torch.uint8, device="cuda")
        assert api.lib().mcx_gunzip_text_dev(z._h, small.data_ptr(), small.numel(), C.byref(info)) == api.ERR_CAPACITY
        d_dst = torch.zeros(info.text_bytes, dtype=torch.uint8, device="cuda")
        z.text_dev(d_dst, info)
        assert d_dst.cpu().numpy().tobytes() == text[:info.text_bytes]
    # one stretch with an arena too small for what it makes: CAPACITY, in words
    blob, text = V.v4()
    raw = raw_of(blob)
    d_src = torch.frombuffer(bytearray(raw + b"\0" * 8), dtype=torch.uint8).cuda()
    with api.Gunzipper(0, 65536, 1, 1 << 20) as z:
        bit, status = 0, api.GZ_OK
        for _ in range(64):
            info = z.round_dev(d_src, bit >> 3, len(raw) - (bit >> 3), bit & 7, True)
            status = info.status
            if status != api.GZ_OK or info.final:
                break
            z.text_dev(torch.zeros(max(info.text_bytes, 1), dtype=torch.uint8, device="cuda"), info)
            bit = (bit >> 3) * 8 + info.end_bit
        assert status == api.GZ_CAPACITY and "arena" in api.lib().mcx_last_error().decode()


# ---- the front end ----

GZ_ALL = None


def write_gz(path, text):
    """an ordinary gzip stream with many blocks a stretch of 4096 bytes (V1's recipe: level 6, memLevel 3)"""
    open(path, "wb").write(V.gz_level(text, 6, 3))


class Front(tr.Front):
    def run(self, files, out, gz=True, inflate=False, parse=True, device_sam=True, **kw):
        self.mp.reset()
        files = list(files) + [None] * (2 - len(files))
        try:
            st = self.mp.map_files(files[0], files[1], out, device_gz=gz, device_inflate=inflate, device_parse=parse, device_sam=device_sam, **kw)
            return st["reads"], "", open(out, "rb").read() if out else None, self.mp.last_route()
        except self.api.McxError as e:
            return None, str(e), None, self.mp.last_route()


@pytest.fixture()
def small_rounds(monkeypatch):
    monkeypatch.setenv("MCX_GZ_STRETCH", "4096")
    monkeypatch.setenv("MCX_GZ_ROUND_STRETCHES", "16")


@pytest.mark.parametrize("name", ["toy", "var"])
def test_front_end_gz_route_equals_the_golden_sam(api, golden, tmp_path, small_rounds, name):
    """The golden pairs as ordinary .gz with device_gz, device_parse, device_sam, stretches of 4096 bytes and 16 a round: the golden SAM, and every file's
    route is GZ | PARSE | ROWS | SAM.  The same with -bam against the host-route file's gzip -d bytes."""
    g = golden[name]
    texts = tr.read_texts(g, name)
    want_route = api.ROUTE_GZ | api.ROUTE_PARSE | api.ROUTE_ROWS | api.ROUTE_SAM
    files = [str(tmp_path / f"{name}_{k + 1}.fq.gz") for k in range(2)]
    for f, t in zip(files, texts):
        write_gz(f, t)
    fr = Front(api, g)
    out = str(tmp_path / "gz.sam")
    reads, err, sam, route = fr.run(files, out)
    assert err == "" and reads == sum(t.count(b"\n") // 4 for t in texts), (err, reads)
    assert route == (want_route, want_route), route
    nd, ex = sam_diff(g["sam"]["ksw2"], out)
    assert nd == 0, ex
    # BAM: the host readers' file against this route's
    host = fr.run(files, str(tmp_path / "host.bam"), gz=False, parse=False, bam=True)
    got = fr.run(files, str(tmp_path / "gz.bam"), bam=True)
    bam_bits = api.ROUTE_SAM | api.ROUTE_BGZF | api.ROUTE_BAM
    assert host[1] == got[1] == "" and host[3] == (bam_bits, bam_bits) and got[3] == (want_route | bam_bits, want_route | bam_bits), (host[3], got[3])
    assert gzip.decompress(got[2]) == gzip.decompress(host[2])
    fr.close()


def test_front_end_a_pair_of_one_bgzf_and_one_ordinary_file(api, golden, tmp_path, small_rounds):
    g = golden["toy"]
    texts = tr.read_texts(g, "toy")
    files = [str(tmp_path / "b1.fq.gz"), str(tmp_path / "o2.fq.gz")]
    tr.write_bgzf(files[0], texts[0], 3000); write_gz(files[1], texts[1])
    fr = Front(api, g)
    out = str(tmp_path / "mixed.sam")
    reads, err, sam, route = fr.run(files, out, inflate=True)
    rest = api.ROUTE_PARSE | api.ROUTE_ROWS | api.ROUTE_SAM
    assert err == "" and route == (api.ROUTE_INFLATE | rest, api.ROUTE_GZ | rest), (err, route)
    assert sam_diff(g["sam"]["ksw2"], out)[0] == 0
    # bit 2 alone does not take a BGZF file: the call runs as without the switch
    reads, err, sam, route = fr.run(files, str(tmp_path / "mixed2.sam"))
    assert err == "" and route == (api.ROUTE_SAM, api.ROUTE_SAM) and sam_diff(g["sam"]["ksw2"], str(tmp_path / "mixed2.sam"))[0] == 0
    fr.close()


def test_where_the_route_does_not_apply(api, golden, io_golden, tmp_path, small_rounds):
    """In each case today's routes and today's bytes: bit 2 without device_parse, -p, the host formatter with a SAM file, files the search cannot cut (urandom,
    stored only), and device_inflate = 1 alone on an ordinary file"""
    g = golden["toy"]
    texts = tr.read_texts(g, "toy")
    files = [str(tmp_path / "t1.fq.gz"), str(tmp_path / "t2.fq.gz")]
    for f, t in zip(files, texts):
        write_gz(f, t)
    fr = Front(api, g)
    want = fr.run(files, str(tmp_path / "host.sam"), gz=False, parse=False, device_sam=False)
    assert want[1] == "" and want[3] == (0, 0) and sam_diff(g["sam"]["ksw2"], str(tmp_path / "host.sam"))[0] == 0
    got = fr.run(files, str(tmp_path / "a.sam"), parse=False, device_sam=False)
    assert got[3] == (0, 0) and got[:3] == want[:3]
    got = fr.run(files, str(tmp_path / "b.sam"), device_sam=False)  # the host formatter
    assert got[3] == (0, 0) and got[:3] == want[:3]
    got = fr.run(files, str(tmp_path / "c.sam"), gz=False, inflate=True)  # device_inflate = 1 alone, as test_bgzf_resident.py has it
    assert got[3] == (api.ROUTE_SAM, api.ROUTE_SAM) and got[:3] == want[:3]
    # stored only: no start is found, the chain is stretch 0 alone
    stored = [str(tmp_path / "s1.fq.gz"), str(tmp_path / "s2.fq.gz")]
    for f, t in zip(stored, texts):
        open(f, "wb").write(V.gz_level(t, 0))
    got = fr.run(stored, str(tmp_path / "d.sam"))
    assert got[3] == (api.ROUTE_SAM, api.ROUTE_SAM) and got[:3] == want[:3]
    # -p
    il = str(tmp_path / "il.fq.gz")
    write_gz(il, open(io_golden["il.fq"], "rb").read())
    host = fr.run([il], str(tmp_path / "il_host.sam"), gz=False, parse=False, device_sam=False, interleaved=True)
    got = fr.run([il], str(tmp_path / "il.sam"), interleaved=True)
    assert host[3] == (0, 0) and got[3] == (api.ROUTE_SAM, 0) and got[0] == host[0] > 0 and got[2] == host[2]
    # bytes that are no text: the host reader's verdict
    noise = str(tmp_path / "n1.fq.gz")
    open(noise, "wb").write(V.gz_level(os.urandom(1 << 18), 6))
    host = fr.run([noise], str(tmp_path / "n_host.sam"), gz=False, parse=False, device_sam=False)
    got = fr.run([noise], str(tmp_path / "n.sam"))
    assert got[:3] == host[:3], (got[:2], host[:2])  # reads, error text and the SAM file's bytes
    assert not got[3][0] & (api.ROUTE_GZ | api.ROUTE_PARSE | api.ROUTE_ROWS) and (got[1] != "" or got[3] == (api.ROUTE_SAM, 0)), got[3]
    fr.close()


def test_a_sharded_call_runs_as_without_the_switch(api, golden, tmp_path, small_rounds):
    """two shards on one device, each a mapper of its own on a thread, one output file: the host readers' routes and the golden SAM, switch on or off"""
    g = golden["toy"]
    texts = tr.read_texts(g, "toy")
    files = [str(tmp_path / "t1.fq.gz"), str(tmp_path / "t2.fq.gz")]
    for f, t in zip(files, texts):
        write_gz(f, t)
    for switch in (False, True):
        links = (api.Exchange * 2)()
        assert api.lib().mcx_exchange_local(2, links) == 0
        out = str(tmp_path / f"sh_{int(switch)}.sam")
        res = [None, None]

        def shard(r):
            ix = api.Index(g["prefix"], device=0, full_sa=True)
            mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1 << 13)
            try:
                st = mp.map_files(files[0], files[1], out, shard=(r, 2), exchange=links[r], device_gz=switch, device_parse=switch, device_sam=True)
                res[r] = (st["reads"], mp.last_route())
            except api.McxError as e:
                res[r] = (str(e), None)
            mp.close(); ix.close()
        ts = [threading.Thread(target=shard, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        api.lib().mcx_exchange_local_free(links)
        assert all(r is not None and r[1] == (api.ROUTE_SAM, api.ROUTE_SAM) for r in res), res
        assert sam_diff(g["sam"]["ksw2"], out)[0] == 0, switch


def test_damaged_input_on_the_route(golden, tmp_path):
    """A file cut short, a file with a wrong trailer CRC and a file with one byte flipped, each as file 1 of a pair, through the host readers and through the route.  The call ends as the
    host route's does: no error, the input ends at the damaged place.  Every read delivered is a true read of the files, in order (the SAM's read names are the
    files' first names, mate by mate); fewer reads are delivered than the file has; one line on stderr names the file and the bytes of text delivered.
    How many reads come before the damaged place depends on the round size on both routes, so the two counts are not compared with one another.  The host
    reader's rounds are 2 MB of compressed bytes a thread: the files hold 6 MB, and both runs are processes of their own with MCX_HOST_CPUS=6 (two inflate
    threads: the count is read once per process), so that the host reader, too, delivers a round before the damage."""
    g = golden["toy"]
    r1, r2 = tr.read_texts(g, "toy")
    reps = 70
    n = reps * (r1.count(b"\n") // 4)

    def renamed(text, k):  # (distinct names in every copy)
        return b"\n".join(l[:1] + b"c%d_" % k + l[1:] if i % 4 == 0 and l else l for i, l in enumerate(text.split(b"\n")))
    t1 = b"".join(renamed(r1, k) for k in range(reps))
    t2 = b"".join(renamed(r2, k) for k in range(reps))
    whole = V.gz_level(t1, 1)
    assert len(whole) > (5 << 20)
    f2 = str(tmp_path / "w2.fq.gz")
    open(f2, "wb").write(V.gz_level(t2, 1))
    names1 = [l.split()[0][1:].decode() for l in t1.split(b"\n")[0::4] if l]
    crc = bytearray(whole); crc[-6] ^= 1
    env = dict(os.environ, MCX_TIMING="1", MCX_HOST_CPUS="6", MCX_GZ_ROUND_STRETCHES="16")
    flipped = bytearray(whole); flipped[len(whole) * 11 // 12] ^= 0x55
    for tag, blob in (("cut", whole[:len(whole) * 11 // 12]), ("trailer", bytes(crc)), ("flipped", bytes(flipped))):
        f1 = str(tmp_path / f"{tag}_1.fq.gz")
        open(f1, "wb").write(blob)
        seen = {}
        for leg, switches in (("host", []), ("gz", ["-gpu_gz", "-gpu_parse", "-gpu_sam"])):
            out = str(tmp_path / f"{tag}_{leg}.sam")
            r = subprocess.run([EXE, "-i", g["prefix"], "-f", f1, "-f2", f2, "-alg", "ksw2", "-sam", out, "-no_vcf"] + switches, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
            qnames = [l.split("\t", 1)[0] for l in open(out) if not l.startswith("@")] if os.path.exists(out) else []
            seen[leg] = (r.returncode, qnames, r.stderr)
        (hrc, hq, herr), (grc, gq, gerr) = seen["host"], seen["gz"]
        assert hrc == grc == 0, (tag, hrc, grc, herr[-800:], gerr[-800:])
        assert "file 1 526, file 2 526" in gerr and "file 1 0, file 2 0" in herr, (tag, gerr[-800:])
        for leg, q in (("host", hq), ("gz", gq)):
            assert 0 < len(q) < 2 * n and len(q) % 2 == 0, (tag, leg, len(q))
            assert q[0::2] == names1[:len(q) // 2] and q[1::2] == names1[:len(q) // 2], (tag, leg)
        line = [l for l in gerr.split("\n") if "-gpu_gz" in l and os.path.basename(f1) in l]
        assert len(line) == 1 and "bytes of text" in line[0], (tag, gerr[-800:])
        assert not [l for l in herr.split("\n") if "-gpu_gz:" in l]


def test_cli_gpu_gz(golden, tmp_path):
    g = golden["toy"]
    texts = tr.read_texts(g, "toy")
    f1, f2 = str(tmp_path / "t1.fq.gz"), str(tmp_path / "t2.fq.gz")
    write_gz(f1, texts[0]); write_gz(f2, texts[1])
    out = str(tmp_path / "cli.sam")
    env = dict(os.environ, MCX_TIMING="1", MCX_GZ_STRETCH="4096", MCX_GZ_ROUND_STRETCHES="16")
    r = subprocess.run([EXE, "-i", g["prefix"], "-f", f1, "-f2", f2, "-alg", "ksw2", "-sam", out, "-no_vcf", "-gpu_gz", "-gpu_parse", "-gpu_sam"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "file 1 526, file 2 526" in r.stderr, r.stderr[-2000:]
    nd, ex = sam_diff(g["sam"]["ksw2"], out)
    assert nd == 0, ex
