"""-m (MapCaller's bUnique = false): a SAM line for every candidate that holds a read's best score.

The expected -m SAM of a golden set is rebuilt from two committed files: the unique-mode SAM (ref.<alg>.sam.gz) and
the reference's further lines (ref.<alg>.m.extra.gz, scripts/make_golden_multi.py: "<index of the read's first line>\\t<line>").
The reference leaves FLAG unset on the further lines of single-end reads (it printed 32755 or 32535); the product prints 0 or 16
by strand there (deviation 4), so that field is masked on those lines only."""
import gzip
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT, SETS, sam_diff, vcf_alg, vcf_body

MULTI_SETS = ("mc", "se", "long", "var")
CASES = [(n, a) for n in MULTI_SETS for a in ("nw", "ksw2")]


def read_extras(name, alg):
    """[(index of the primary line, extra line)] of a golden set"""
    out = []
    for line in gzip.open(os.path.join(GOLD, name, f"ref.{alg}.m.extra.gz")).read().decode("latin-1").split("\n"):
        if line:
            i, rest = line.split("\t", 1)
            out.append((int(i), rest))
    return out


def rebuild_multi(unique_text, extras):
    """The -m SAM: every extra line right behind its primary line (header lines are not counted by the index)."""
    lines = unique_text.split("\n")
    head = [l for l in lines if l.startswith("@")]
    body = [l for l in lines if l and not l.startswith("@")]
    by = {}
    for i, l in extras:
        by.setdefault(i, []).append(l)
    out = list(head)
    for i, l in enumerate(body):
        out.append(l)
        out.extend(by.get(i, []))
    return "\n".join(out) + "\n"


def mask_se_extra_flags(text, paired):
    """(single-end) FLAG of every line after a read's first is '?'; returns (masked text, [(the flag it hid, the strand the line's
    SEQ shows: 16 when it is the reverse complement of the first line's SEQ on the other strand, else the first line's)])."""
    if paired:
        return text, []
    out, hidden, prev = [], [], None
    for l in text.split("\n"):
        f = l.split("\t")
        if l and not l.startswith("@") and len(f) > 9:
            if prev is not None and f[0] == prev[0]:
                first_rev = int(prev[1]) & 0x10
                hidden.append((f[1], first_rev if f[9] == prev[9] else 0x10 - first_rev))
                f[1] = "?"
            else:
                prev = f
        out.append("\t".join(f))
    return "\n".join(out), hidden


def expected_multi(name, alg):
    unique = gzip.open(os.path.join(GOLD, name, f"ref.{alg}.sam.gz")).read().decode("latin-1")
    return rebuild_multi(unique, read_extras(name, alg))


def compare(name, alg, out_path):
    paired = SETS[name]
    want, _ = mask_se_extra_flags(expected_multi(name, alg), paired)
    got, flags = mask_se_extra_flags(open(out_path, "rb").read().decode("latin-1"), paired)
    assert all(f == str(strand) for f, strand in flags), [x for x in flags if x[0] != str(x[1])][:3]
    a, b = want.split("\n"), got.split("\n")
    bad = [(x, y) for x, y in zip(a, b) if x != y]
    assert len(a) == len(b) and not bad, (len(a), len(b), bad[:2])


# ---- CPU ------------------------------------------------------------------------------------------------
def test_library_exports_the_multi_calls():
    from mapcaller_amd import api
    for s in ("mcx_ctx_set_multi", "mcx_multi_lines", "mcx_multi_copy", "mcx_stream_multi"):
        assert s in api.SYMBOLS
        assert s in open(os.path.join(ROOT, "include", "mcx.h")).read()
    if os.path.exists(api.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for s in ("mcx_ctx_set_multi", "mcx_multi_lines", "mcx_multi_copy", "mcx_stream_multi"):
            assert f" {s}\n" in nm, s


def test_mapper_accepts_multi():
    from mapcaller_amd import api, run
    sig = inspect.signature(api.Mapper.__init__)
    assert sig.parameters["multi"].default is False and sig.parameters["multi_cap"].default == 0
    assert run.parse(["-i", "x", "-f", "a.fq", "-m"]).multi and not run.parse(["-i", "x", "-f", "a.fq"]).multi


@pytest.mark.parametrize("name,alg", CASES)
def test_multi_fixtures_are_well_formed(name, alg):
    paired = SETS[name]
    body = [l for l in gzip.open(os.path.join(GOLD, name, f"ref.{alg}.sam.gz")).read().decode("latin-1").split("\n") if l and not l.startswith("@")]
    ex = read_extras(name, alg)
    assert ex, "a golden set without ties"
    idx = [i for i, _ in ex]
    assert idx == sorted(idx) and idx[-1] < len(body)
    tied = set(idx)
    for i, l in ex:
        p, f = body[i].split("\t"), l.split("\t")
        assert f[0] == p[0]
        if paired:
            assert int(f[1]) & 0xC0 == int(p[1]) & 0xC0  # the same mate
        # (single-end: FLAG is the reference's unset one, whatever the stack held — DESIGN §6)
        assert f[4] == "0" and p[4] == "0"  # MAPQ 0 on every line of a read with several
        assert f[-2:] == p[-2:]  # AS, XS are the read's
    assert all(body[i].split("\t")[4] == "0" for i in tied)


def test_rebuild_and_mask_on_hand_made_lines():
    unique = "@HD\tVN:1.4\n@SQ\tSN:c\tLN:9\nr1\t0\tc\t1\t0\t4M\t*\t0\t0\tACGT\t*\nr2\t16\tc\t5\t60\t4M\t*\t0\t0\tACGT\t*\n"
    extras = [(0, "r1\t32755\tc\t7\t0\t4M\t*\t0\t0\tACGT\t*"), (0, "r1\t32755\tc\t9\t0\t4M\t*\t0\t0\tACGT\t*")]
    m = rebuild_multi(unique, extras)
    assert m.split("\n")[2:6] == ["r1\t0\tc\t1\t0\t4M\t*\t0\t0\tACGT\t*", extras[0][1], extras[1][1], "r2\t16\tc\t5\t60\t4M\t*\t0\t0\tACGT\t*"]
    masked, hidden = mask_se_extra_flags(m, paired=False)
    assert hidden == [("32755", 0), ("32755", 0)]
    rc = m.replace("r1\t32755\tc\t9\t0\t4M\t*\t0\t0\tACGT", "r1\t16\tc\t9\t0\t4M\t*\t0\t0\tACGG")
    assert mask_se_extra_flags(rc, paired=False)[1] == [("32755", 0), ("16", 16)]
    lines = masked.split("\n")
    assert lines[2].split("\t")[1] == "0" and lines[3].split("\t")[1] == "?" and lines[5].split("\t")[1] == "16"
    assert mask_se_extra_flags(m, paired=True) == (m, [])
    assert rebuild_multi(unique, []) == unique


# ---- GPU ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


def _map(api, golden, name, alg, out, **kw):
    g = golden[name]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg=alg, multi=True, **kw)
    st = mp.map_files(g["r1"], g["r2"], out)
    mp.close(); ix.close()
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name,alg", CASES)
def test_multi_sam_equals_reference(api, golden, tmp_path, name, alg):
    out = str(tmp_path / "m.sam")
    _map(api, golden, name, alg, out)
    compare(name, alg, out)


@pytest.mark.gpu
@pytest.mark.parametrize("name,alg", [("mc", "ksw2"), ("se", "nw"), ("var", "nw")])
def test_multi_sam_on_the_large_batch_paths(api, golden, tmp_path, monkeypatch, name, alg):
    monkeypatch.setenv("MCX_ORDER_MIN", "1")
    monkeypatch.setenv("MCX_DP_LANE_ALWAYS", "1")
    out = str(tmp_path / "m.sam")
    _map(api, golden, name, alg, out, max_batch_reads=1 << 14)
    compare(name, alg, out)


@pytest.mark.gpu
@pytest.mark.parametrize("name,alg", [("mc", "nw"), ("var", "ksw2"), ("se", "ksw2")])
def test_multi_sam_with_small_batches(api, golden, tmp_path, name, alg):
    """batch seams and avgDist replays re-run tied pairs: each takes fresh extras, the stale ones stay unreferenced"""
    out = str(tmp_path / "m.sam")
    st = _map(api, golden, name, alg, out, max_batch_reads=400)
    compare(name, alg, out)
    if SETS[name] and name == "var":
        assert st["replayed_pairs"] > 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("name,alg", [("var", "nw"), ("se", "nw")])
def test_multi_pool_overflow_grows_and_gives_the_same_sam(api, golden, tmp_path, name, alg):
    out = str(tmp_path / "m.sam")
    _map(api, golden, name, alg, out, multi_cap=3)
    compare(name, alg, out)


@pytest.mark.gpu
def test_multi_keeps_the_profile(golden, tmp_path):
    """-m with -vcf: the VCF is the reference's (-m changes nothing but the SAM)"""
    name = "mc"
    alg = vcf_alg(name, "default")
    g = golden[name]
    exe = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
    sam, vcf = str(tmp_path / "o.sam"), str(tmp_path / "o.vcf")
    subprocess.run([exe, "-i", g["prefix"], "-f", g["r1"], "-f2", g["r2"], "-alg", alg, "-sam", sam, "-vcf", vcf, "-m", "-t", "2"],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    assert vcf_body(vcf) == vcf_body(g["vcf"]["default"])
    compare(name, alg, sam)


@pytest.mark.gpu
def test_map_batch_returns_the_extras(api, golden):
    """api.Mapper(multi=True).map_batch: the third element holds the reference's further lines, read by read"""
    name, alg = "var", "nw"
    g = golden[name]
    r1 = [l for i, l in enumerate(open(g["r1"], "rb").read().split(b"\n")) if i % 4 == 1]
    r2 = [l for i, l in enumerate(open(g["r2"], "rb").read().split(b"\n")) if i % 4 == 1]
    seqs = [x for p in range(len(r1)) for x in (r1[p], r2[p])]
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg=alg, multi=True, max_batch_reads=len(seqs))
    off = np.zeros(len(seqs) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    aln, cig, (index, recs, rcig) = mp.map_batch(np.frombuffer(b"".join(seqs), dtype=np.uint8), off, True)
    plain = api.Mapper(ix, alg=alg, max_batch_reads=len(seqs))
    aln0, cig0 = plain.map_batch(np.frombuffer(b"".join(seqs), dtype=np.uint8), off, True)
    assert (aln0[[f for f in aln0.dtype.names if f != "cigar_off"]] == aln[[f for f in aln.dtype.names if f != "cigar_off"]]).all()
    ex = read_extras(name, alg)
    assert len(recs) == len(ex) and index[-1] == len(ex) and (np.diff(index.astype(np.int64)) >= 0).all()
    for k, (i, line) in enumerate(ex):
        f = line.split("\t")
        r = int(np.searchsorted(index, k, side="right")) - 1
        assert r == i
        a = recs[k]
        ops = "".join(f"{int(w) >> 4}{'MIDNSHP='[int(w) & 7]}" for w in rcig[k])
        assert (int(a["flag"]), int(a["pos"]), int(a["mapq"]), ops, int(a["tlen"])) == (int(f[1]), int(f[3]), int(f[4]), f[5], int(f[8])), (k, line[:100])
    mp.close(); plain.close(); ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["0", "0,0"])
@pytest.mark.parametrize("name,alg", [("mc", "nw"), ("se", "ksw2")])
def test_native_cli_multi_equals_reference(golden, tmp_path, devices, name, alg):
    g = golden[name]
    exe = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
    sam = str(tmp_path / "o.sam")
    cmd = [exe, "-i", g["prefix"], "-f", g["r1"]] + (["-f2", g["r2"]] if g["r2"] else []) + ["-alg", alg, "-sam", sam, "-no_vcf", "-m", "-t", "2",
                                                                                            "-devices", devices, "-batch", "400"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    compare(name, alg, sam)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True])
def test_stream_paths_carry_the_same_extras(api, golden, packed):
    """mcx_stream_* with three batches in flight — the 64-byte path (mcx_stream_map) and the packed 32-byte one (submit_packed +
    mcx_stream_map32) —: every collected batch's extras (mcx_stream_multi) equal map_batch's, read by read"""
    import torch
    g = golden["var"]
    r1 = [l for i, l in enumerate(open(g["r1"], "rb").read().split(b"\n")) if i % 4 == 1]
    r2 = [l for i, l in enumerate(open(g["r2"], "rb").read().split(b"\n")) if i % 4 == 1]
    n_pairs, per = 1000, 5
    batches = []
    for b in range(per):
        seqs = [x for p in range(b * n_pairs, (b + 1) * n_pairs) for x in (r1[p], r2[p])]
        off = np.zeros(len(seqs) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(x) for x in seqs])
        batches.append((seqs, np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), off))
    ix = api.Index(g["prefix"], device=0, full_sa=True)
    mp = api.Mapper(ix, alg="nw", max_batch_reads=2 * n_pairs, multi=True)
    want = [mp.map_batch(bb, oo, True)[2] for _, bb, oo in batches]
    assert sum(len(w[1]) for w in want) > 0
    mp.reset()
    if packed:
        pk = []
        for seqs, _, _ in batches:
            t = torch.tensor(np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), -1).copy())
            pk.append(api.pack_reads(t))
        keep = pk
        arg = [(c.data_ptr(), rw, l.data_ptr(), o.data_ptr(), no) for c, l, o, no, rw in pk]
        _, d2h = mp.map_stream_packed(arg, 2 * n_pairs, True, out32=True)
    else:
        keep = []
        for _, bb, oo in batches:
            tb = torch.zeros(bb.size + 64, dtype=torch.uint8).pin_memory(); tb[:bb.size] = torch.from_numpy(bb)
            keep.append(tb)
        to = torch.from_numpy(batches[0][2].astype(np.int64)).to(torch.int32).pin_memory()
        _, d2h = mp.map_stream([t.data_ptr() for t in keep], to.data_ptr(), 2 * n_pairs, True)
    got = mp.stream_multi
    assert len(got) == per
    rec_bytes = 32 if packed else 64
    assert d2h >= per * 2 * n_pairs * rec_bytes + sum(4 * (2 * n_pairs + 1) + 32 * len(w[1]) for w in want)  # the extras count in bytes_out
    fields = ("pos", "mate_pos", "chr", "flag", "mapq", "tlen", "nm", "as", "xs", "n_cigar", "fwd", "has_mate")
    for b in range(per):
        (wi, wr, wc), (gi, gr, gc) = want[b], got[b]
        assert np.array_equal(wi, gi), b
        for f in fields:
            assert np.array_equal(wr[f], gr[f]), (b, f)
        assert all(np.array_equal(x, y) for x, y in zip(wc, gc)), b
    mp.close(); ix.close()


@pytest.mark.gpu
def test_bench_genome_slice_equals_compiled_reference(api, tmp_path_factory):
    """60 k pairs of bench.py's workload (the 3.1 Gbp human-like genome: reads from repeats with hundreds of seed hits, mate rescue,
    the large tier) through -m, ksw2, against the compiled reference's -m SAM, byte for byte: candidate order behind `best` through
    rescue and the large tier.  Skipped where the compiled reference did not travel."""
    import argparse
    import sys
    import torch
    ref_bin = os.path.join(ROOT, "oracle", "_ref", "MapCaller")
    if not os.path.exists(ref_bin):
        pytest.skip("the compiled reference (oracle/_ref) is not on this machine")
    from mapcaller_amd import synth
    sys.path.insert(0, ROOT)
    import bench
    dev = torch.device("cuda", 0)
    codes, lens, _ = bench.make_genome(argparse.Namespace(genome_mbp=3100.0, contigs=24, repeats=2000, genome="human"), dev, seed=1234)
    ix = api.Index.from_codes(codes.data_ptr(), lens, device=0, full_sa=2)
    d = tmp_path_factory.mktemp("mslice")
    prefix = str(d / "big")
    ix.save(prefix)
    n_pairs = 60_000
    reads = bench.make_reads(codes, lens, n_pairs, 150, seed=1001, device=dev).reshape(2 * n_pairs, 150).cpu()
    del codes
    f1, f2 = str(d / "r1.fq"), str(d / "r2.fq")
    synth.write_fastq(f1, reads, 0, 2); synth.write_fastq(f2, reads, 1, 2)
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=2 * n_pairs, multi=True)
    out = str(d / "gpu.sam")
    mp.map_files(f1, f2, out)
    mp.close(); ix.close()
    ref = str(d / "ref.sam")
    subprocess.run([ref_bin, "-i", prefix, "-f", f1, "-f2", f2, "-alg", "ksw2", "-sam", ref, "-m", "-no_vcf", "-t", "1", "-log", str(d / "job.log")],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    nd, ex = sam_diff(ref, out)
    n_lines = sum(1 for l in open(out, "rb") if not l.startswith(b"@"))
    print(f"bench slice -m: {2 * n_pairs} reads, {n_lines - 2 * n_pairs} extra lines")
    assert n_lines > 2 * n_pairs  # ties in the large tier
    assert nd == 0, ex
