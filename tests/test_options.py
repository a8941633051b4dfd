"""-indel (MaxPosDiff, 30 unless said, clamped to 100) and -maxmm (MaxMisMatchRate, 0.05 unless said) away from their defaults.

tests/golden/opt (scripts/make_golden_opts.py) holds the compiled reference's `-t 1` output on one genome with repeats, tandem and N runs,
a donor with insertions and deletions of 1..90 bases, and three read sets with 3 % substitutions per base — 150 bp pairs, 250 bp pairs,
250 bp single-end reads as FASTA — at every setting of MANIFEST.json's "settings", for both algorithms.  The default run's SAM is kept
in full, every other run as the lines that differ from it (rebuild_sam below).  The oracle, the device headers compiled for the host
(tests/hostemu) and, under `-m gpu`, libmcx.so and the native command line must give those bytes.

The oracle has no -m: the -m lines at -indel 60 are checked against the GPU path alone, as tests/test_multi.py does for the defaults."""
import ctypes
import gzip
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, VcfOpts, maps_canon, vcf_body

OPT = os.path.join(GOLD, "opt")
MANIFEST = json.load(open(os.path.join(OPT, "MANIFEST.json")))
SETS_OPT = MANIFEST["sets"]          # name -> {reads, rlen, paired, fastq}
TAGS = ["default"] + [t for t in MANIFEST["settings"] if t != "default"]
ALGS = ("nw", "ksw2")
CASES = [(n, a, t) for n in SETS_OPT for a in ALGS for t in TAGS]
AGAIN = ("indel0", "indel60", "indel100", "maxmm0.02", "maxmm0.1")  # the settings the index / kernel variants are run at
EXE = os.path.join(ROOT, "mapcaller_amd", "mapcaller-mi355x")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "MapCaller")


def setting(tag):
    """tag -> (max_pos_diff, max_mismatch_rate) as the reference's command line takes them: atoi, and atof narrowed to float"""
    f = MANIFEST["settings"][tag]
    kv = dict(zip(f[::2], f[1::2]))
    return int(kv.get("-indel", 30)), float(kv.get("-maxmm", 0.05))


def read_gz(name):
    return gzip.open(os.path.join(OPT, name), "rb").read().decode("latin-1")


def rebuild_sam(default_text, diff_text):
    """A run's SAM from the default run's and the kept lines `<index among all lines>\\t<line>`; SEQ and QUAL written `=` are the default line's."""
    lines = default_text.split("\n")
    for rec in diff_text.split("\n"):
        if not rec:
            continue
        i, line = rec.split("\t", 1)
        f = line.split("\t")
        if len(f) > 10 and f[9] == "=" and f[10] == "=":
            f[9:11] = lines[int(i)].split("\t")[9:11]
        lines[int(i)] = "\t".join(f)
    return "\n".join(lines)


def expected_sam(name, alg, tag):
    base = read_gz(f"{name}.{alg}.default.sam.gz")
    return base if tag == "default" else rebuild_sam(base, read_gz(f"{name}.{alg}.{tag}.diff.gz"))


def assert_sam(path, name, alg, tag):
    got = open(path, "rb").read().decode("latin-1").split("\n")
    want = expected_sam(name, alg, tag).split("\n")
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(want, got)) if x != y]
    assert len(got) == len(want) and not bad, (name, alg, tag, len(want), len(got), len(bad), bad[:2])


@pytest.fixture(scope="module")
def opt(tmp_path_factory):
    """tests/golden/opt unpacked: prefix, and per set its read files"""
    d = tmp_path_factory.mktemp("opt")
    for ext in ("bwt", "sa", "pac", "ann", "amb"):
        shutil.copy(os.path.join(OPT, f"idx.{ext}"), d / f"idx.{ext}")
    out = {"prefix": str(d / "idx"), "dir": d}
    for name, s in SETS_OPT.items():
        ext = "fq" if s["fastq"] else "fa"
        files = []
        for k in (1, 2) if s["paired"] else (1,):
            p = d / f"{name}.r{k}.{ext}"
            p.write_bytes(gzip.open(os.path.join(OPT, f"{name}.r{k}.{ext}.gz"), "rb").read())
            files.append(str(p))
        out[name] = (files[0], files[1] if s["paired"] else None)
    for fn in ("pe150.ksw2.indel60.prof", "pe150.ksw2.indel60.maps", "pe150.vcf.indel60", "pe150.vcf.maxmm0.1"):
        (d / fn).write_bytes(gzip.open(os.path.join(OPT, fn + ".gz"), "rb").read())
        out[fn] = str(d / fn)
    return out


# ---- CPU: the fixtures ---------------------------------------------------------------------------------------------------------------
def test_rebuild_on_hand_made_lines():
    base = "@SQ\tSN:c\tLN:9\nr1\t0\tc\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\nr2\t16\tc\t5\t60\t4M\t*\t0\t0\tAAAA\tJJJJ\n"
    diff = "1\tr1\t0\tc\t3\t0\t4M\t*\t0\t0\t=\t=\n2\tr2\t4\t*\t0\t0\t*\t*\t0\t0\tTTTT\tJJJJ\n"
    got = rebuild_sam(base, diff).split("\n")
    assert got == ["@SQ\tSN:c\tLN:9", "r1\t0\tc\t3\t0\t4M\t*\t0\t0\tACGT\tIIII", "r2\t4\t*\t0\t0\t*\t*\t0\t0\tTTTT\tJJJJ", ""]
    assert rebuild_sam(base, "") == base


@pytest.mark.parametrize("name,alg", [(n, a) for n in SETS_OPT for a in ALGS])
def test_opt_fixtures_are_well_formed(name, alg):
    s = SETS_OPT[name]
    base = expected_sam(name, alg, "default").split("\n")
    assert base[-1] == "" and sum(1 for l in base if l and not l.startswith("@")) == s["reads"]
    for tag in TAGS[1:]:
        run = expected_sam(name, alg, tag).split("\n")
        assert len(run) == len(base)
        m = MANIFEST["runs"][f"{name}.{alg}.{tag}"]
        differ = sum(1 for x, y in zip(base, run) if x != y)
        assert (m["lines"], m["differ"]) == (len(base) - 1, differ), (tag, m, differ)
        assert differ >= 0.02 * m["lines"], (tag, differ, m["lines"])  # a setting that hardly changes the output pins nothing
        for x, y in zip(base, run):  # the same reads in the same order, whole lines
            fx, fy = x.split("\t"), y.split("\t")
            assert fx[0] == fy[0] and (len(fy) < 11 or (len(fy[9]) == s["rlen"] and (fy[10] == "*" if not s["fastq"] else len(fy[10]) == s["rlen"]))), y[:80]
    assert MANIFEST["runs"][f"{name}.{alg}.indel100"]["equals_indel150"] is True  # the clamp, recorded when the fixtures were made
    assert setting("indel100") == (100, pytest.approx(0.05)) and setting("indel60_maxmm0.1") == (60, 0.1)


def test_opt_fixture_sizes():
    largest_elsewhere = max(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(GOLD) if os.path.basename(r) != "opt" for f in fs)
    sizes = {f: os.path.getsize(os.path.join(OPT, f)) for f in os.listdir(OPT)}
    assert max(sizes.values()) <= min(largest_elsewhere, 1 << 20), max(sizes, key=sizes.get)
    assert sum(sizes.values()) <= 3 * 1000 * 1000, sum(sizes.values())


def test_clamp_fact_against_the_compiled_reference(opt, tmp_path, record_property):
    """-indel 150 gives the -indel 100 SAM: asked of the compiled reference again where it is built"""
    if not os.path.exists(REF_BIN):
        record_property("checker", "manifest only (no compiled reference on this machine)")
        return
    f1, f2 = opt["pe150"]
    out = str(tmp_path / "r.sam")
    subprocess.run([REF_BIN, "-i", opt["prefix"], "-f", f1, "-f2", f2, "-alg", "ksw2", "-sam", out, "-no_vcf", "-t", "1", "-indel", "150",
                    "-log", str(tmp_path / "job.log")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    assert_sam(out, "pe150", "ksw2", "indel100")
    record_property("checker", "compiled reference")


# ---- CPU: the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def oracle_opts(oracle_lib):
    """sets the oracle's -indel / -maxmm for a test and puts the defaults back after it"""
    oracle_lib.mcxo_set_mapping_opts.argtypes = [ctypes.c_int, ctypes.c_float]
    oracle_lib.mcxo_set_mapping_opts.restype = None
    yield lambda tag: oracle_lib.mcxo_set_mapping_opts(*setting(tag))
    oracle_lib.mcxo_set_mapping_opts(30, 0.05)


@pytest.mark.parametrize("name,alg,tag", CASES)
def test_oracle_sam_equals_reference(oracle_lib, oracle_opts, opt, tmp_path, name, alg, tag):
    f1, f2 = opt[name]
    oracle_opts(tag)
    ix = oracle_lib.mcxo_index_load(opt["prefix"].encode())
    out = str(tmp_path / "o.sam")
    n = oracle_lib.mcxo_map_files(ix, f1.encode(), (f2 or "").encode(), 0 if alg == "nw" else 1, out.encode(), 1, None)
    oracle_lib.mcxo_index_free(ix)
    assert n == SETS_OPT[name]["reads"]
    assert_sam(out, name, alg, tag)


def test_oracle_profile_equals_reference_at_indel_60(oracle_lib, oracle_opts, opt, tmp_path):
    f1, f2 = opt["pe150"]
    oracle_opts("indel60")
    ix = oracle_lib.mcxo_index_load(opt["prefix"].encode())
    out = str(tmp_path / "p")
    n = oracle_lib.mcxo_map_files_profile(ix, f1.encode(), f2.encode(), 1, out.encode())
    oracle_lib.mcxo_index_free(ix)
    assert n > 0
    assert open(out + ".prof", "rb").read() == open(opt["pe150.ksw2.indel60.prof"], "rb").read()
    assert maps_canon(open(out + ".maps", encoding="latin-1").read()) == maps_canon(open(opt["pe150.ksw2.indel60.maps"], encoding="latin-1").read())


@pytest.mark.parametrize("tag", ["indel60", "maxmm0.1"])
def test_oracle_vcf_equals_reference(oracle_lib, oracle_opts, opt, tmp_path, tag):
    f1, f2 = opt["pe150"]
    oracle_opts(tag)
    ix = oracle_lib.mcxo_index_load(opt["prefix"].encode())
    out = str(tmp_path / "o.vcf")
    n = oracle_lib.mcxo_map_files_vcf(ix, f1.encode(), f2.encode(), 1, out.encode(), VcfOpts([]).ref)
    oracle_lib.mcxo_index_free(ix)
    assert n > 0
    assert vcf_body(out) == vcf_body(opt[f"pe150.vcf.{tag}"])
    assert vcf_body(opt["pe150.vcf.indel60"]) != vcf_body(opt["pe150.vcf.maxmm0.1"])


def test_oracle_pair_totals_follow_the_options(oracle_lib, oracle_opts, hostemu_variants_lib, opt, tmp_path):
    """The run totals at -indel 60 with the reference's profile dump of that run through the product's variant-calling host logic: the
    reference's VCF of that run (the totals set the fragment size the caller works with); and they are not the default run's."""
    f1, f2 = opt["pe150"]
    ix = oracle_lib.mcxo_index_load(opt["prefix"].encode())
    tot0, tot = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    assert oracle_lib.mcxo_pair_totals(ix, f1.encode(), f2.encode(), 1, tot0) > 0
    oracle_opts("indel60")
    assert oracle_lib.mcxo_pair_totals(ix, f1.encode(), f2.encode(), 1, tot) > 0
    oracle_lib.mcxo_index_free(ix)
    assert list(tot) != list(tot0)
    out = str(tmp_path / "o.vcf")
    rc = hostemu_variants_lib.hostemu_call_variants(opt["prefix"].encode(), opt["pe150.ksw2.indel60.prof"].encode(), opt["pe150.ksw2.indel60.maps"].encode(),
                                                    tot[0], tot[1], tot[2], VcfOpts([]).ref, out.encode())
    assert rc == 0, hostemu_variants_lib.hostemu_vc_error()
    assert vcf_body(out) == vcf_body(opt["pe150.vcf.indel60"])


def test_oracle_command_line_takes_the_options(oracle_lib, opt, tmp_path):
    """mcx_oracle -indel / -maxmm; -indel 150 is clamped to 100 with the reference's warning; the VCF run takes them too"""
    exe = os.path.join(ROOT, "oracle", "mcx_oracle")
    f1, f2 = opt["pe250"]
    out = str(tmp_path / "o.sam")
    r = subprocess.run([exe, "-i", opt["prefix"], "-f", f1, "-f2", f2, "-alg", "nw", "-sam", out, "-indel", "150"], stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and "The maximal indel size is 100" in r.stderr
    assert_sam(out, "pe250", "nw", "indel100")
    subprocess.run([exe, "-i", opt["prefix"], "-f", f1, "-f2", f2, "-alg", "ksw2", "-sam", out, "-indel", "60", "-maxmm", "0.1"], check=True, stderr=subprocess.DEVNULL, timeout=600)
    assert_sam(out, "pe250", "ksw2", "indel60_maxmm0.1")
    f1, f2 = opt["pe150"]
    vcf = str(tmp_path / "o.vcf")
    subprocess.run([exe, "-i", opt["prefix"], "-f", f1, "-f2", f2, "-alg", "ksw2", "-vcf", vcf, "-maxmm", "0.1"], check=True, stderr=subprocess.DEVNULL, timeout=600)
    assert vcf_body(vcf) == vcf_body(opt["pe150.vcf.maxmm0.1"])


# ---- CPU: the device headers compiled for the host -----------------------------------------------------------------------------------
def _emu(lib, opt, name, alg, tag, out, batch=1 << 20):
    lib.hostemu_map_files_opts.restype = ctypes.c_int64
    lib.hostemu_map_files_opts.argtypes = [ctypes.c_char_p] * 3 + [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                           ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_int64)]
    f1, f2 = opt[name]
    st = (ctypes.c_int64 * 12)()
    indel, mm = setting(tag)
    n = lib.hostemu_map_files_opts(opt["prefix"].encode(), f1.encode(), (f2 or "").encode(), 0 if alg == "nw" else 1, out.encode(), batch, None, 256, indel, mm, st)
    assert n == SETS_OPT[name]["reads"]
    return list(st)


@pytest.mark.parametrize("name,alg,tag", CASES)
def test_device_glue_on_host_equals_reference(hostemu_lib, opt, tmp_path, monkeypatch, name, alg, tag):
    """mcx_glue.h / mcx_simple.h on the host at the setting: as the product runs them (straight-line pairs with their own DP problems), with
    the straight-line path kept to the pairs that need no DP, and with every pair on the general path — the reference's SAM each time."""
    out = str(tmp_path / "e.sam")
    st = _emu(hostemu_lib, opt, name, alg, tag, out)
    assert_sam(out, name, alg, tag)
    monkeypatch.setenv("MCX_EMU_SIMPLE_NO_DP", "1")
    st_no_dp = _emu(hostemu_lib, opt, name, alg, tag, out)
    assert_sam(out, name, alg, tag)
    monkeypatch.setenv("MCX_EMU_NO_SIMPLE", "1")
    st_general = _emu(hostemu_lib, opt, name, alg, tag, out)
    assert_sam(out, name, alg, tag)
    assert st_general[11] == 0
    if tag in ("indel10", "indel100", "default"):
        assert st[11] >= st_no_dp[11] > 0, (st[11], st_no_dp[11])  # the straight-line path did take pairs


@pytest.mark.parametrize("tag", ["indel60", "maxmm0.1"])
def test_device_glue_on_host_with_small_batches(hostemu_lib, opt, tmp_path, tag):
    out = str(tmp_path / "e.sam")
    _emu(hostemu_lib, opt, "pe150", "ksw2", tag, out, batch=400)
    assert_sam(out, "pe150", "ksw2", tag)


def test_existing_hostemu_entry_point_still_runs_the_defaults(hostemu_lib, opt, tmp_path):
    f1, f2 = opt["pe250"]
    out = str(tmp_path / "e.sam")
    st = (ctypes.c_int64 * 12)()
    assert hostemu_lib.hostemu_map_files(opt["prefix"].encode(), f1.encode(), f2.encode(), 1, out.encode(), 1 << 20, None, 256, st) > 0
    assert_sam(out, "pe250", "ksw2", "default")


# ---- CPU: the Python command line ----------------------------------------------------------------------------------------------------
def test_run_parse_hands_the_options_to_the_contexts(capsys):
    import inspect
    from mapcaller_amd import api, run
    a = run.parse(["-i", "x", "-f", "a.fq"])
    assert (a.indel, a.maxmm) == (30, 0.05)
    sig = inspect.signature(api.Mapper.__init__).parameters
    assert (sig["max_pos_diff"].default, sig["max_mismatch_rate"].default) == (a.indel, a.maxmm)
    a = run.parse(["-i", "x", "-f", "a.fq", "-indel", "60", "-maxmm", "0.1", "-maxlen", "256"])
    kw = run.mapper_kwargs(a)
    assert (kw["max_pos_diff"], kw["max_mismatch_rate"]) == (60, 0.1)
    assert set(kw) <= set(sig)
    a = run.parse(["-i", "x", "-f", "a.fq", "-indel", "150", "-maxmm", "0"])
    assert (a.indel, a.maxmm) == (100, 0.0) and "maximal indel size is 100" in capsys.readouterr().err
    assert run.parse(["-i", "x", "-f", "a.fq", "-indel", "0"]).indel == 0


# ---- CPU: the fuzzer against the compiled reference ----------------------------------------------------------------------------------
def test_fuzz_draws_the_options_after_everything_else():
    """--opts leaves every earlier draw of a round as it was (the usual rounds keep their inputs) and hands the options to all three programs"""
    import random
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import fuzz_parity as fp
    try:
        fp.OPTS = False
        plain = fp.draw(random.Random(5))
        fp.OPTS = True
        seen = set()
        rng = random.Random(5)
        first = fp.draw(rng)
        for _ in range(300):
            d = fp.draw(rng)
            seen.add((d["indel"], d["maxmm"]))
            assert fp.opt_flags(d) == ["-indel", str(d["indel"]), "-maxmm", d["maxmm"]]
    finally:
        fp.OPTS = False
    assert fp.opt_flags(plain) == []
    extra = {"indel": first.pop("indel"), "maxmm": first.pop("maxmm"), "max_indel": first["donor"].pop("max_indel")}
    assert first == plain and extra["max_indel"] in (8, 40, 90)
    assert {i for i, _ in seen} == {0, 5, 10, 30, 60, 100} and {m for _, m in seen} == {"0", "0.02", "0.05", "0.1", "0.2"}


def test_fuzz_rounds_with_options_oracle_equals_compiled_reference(record_property):
    """scripts/fuzz_parity.py --ref --opts, 20 rounds with a fixed seed: the oracle's SAM and VCF against the compiled reference's where this machine has it"""
    if not os.path.exists(REF_BIN):
        record_property("checker", "none (no compiled reference on this machine: the golden vectors above pin the oracle)")
        print("[checker] no compiled reference on this machine")
        return
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), "--ref", "--opts", "--rounds", "20", "--seed", "4242", "--keep", ""]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1400)
    assert r.returncode == 0 and "20 of 20 rounds identical" in r.stdout, r.stdout[-3000:]
    record_property("checker", "compiled reference")
    print("[checker] compiled reference")


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()
    assert a.device_count() >= 1, "no GPU visible"
    return a


def _mapper(api, ix, alg, tag, **kw):
    indel, mm = setting(tag)
    return api.Mapper(ix, alg=alg, max_pos_diff=indel, max_mismatch_rate=mm, **kw)


def _map(api, opt, name, alg, tag, out, full_sa=True, **kw):
    ix = api.Index(opt["prefix"], device=0, full_sa=full_sa)
    mp = _mapper(api, ix, alg, tag, **kw)
    st = mp.map_files(opt[name][0], opt[name][1], out)
    mp.close(); ix.close()
    assert st["reads"] == SETS_OPT[name]["reads"]
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name,alg,tag", CASES)
def test_mapper_sam_equals_reference(api, opt, tmp_path, name, alg, tag):
    out = str(tmp_path / "g.sam")
    _map(api, opt, name, alg, tag, out, max_batch_reads=1 << 14)
    assert_sam(out, name, alg, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("full_sa", [2, False])
@pytest.mark.parametrize("name,alg,tag", [c for c in CASES if c[2] in AGAIN])
def test_mapper_sam_on_the_other_index_forms(api, opt, tmp_path, name, alg, tag, full_sa):
    """full_sa=2: the two-base walk over the pair records; False: the sampled suffix array"""
    out = str(tmp_path / "g.sam")
    _map(api, opt, name, alg, tag, out, full_sa=full_sa, max_batch_reads=1 << 14)
    assert_sam(out, name, alg, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("name,alg,tag", [c for c in CASES if c[2] in AGAIN])
def test_mapper_sam_on_the_large_batch_paths(api, opt, tmp_path, monkeypatch, name, alg, tag):
    """k_simple and the one-problem-per-lane DP kernels forced onto these small batches: the long skewed DP problems of a large -indel on the lane kernels"""
    monkeypatch.setenv("MCX_ORDER_MIN", "1")
    monkeypatch.setenv("MCX_DP_LANE_ALWAYS", "1")
    out = str(tmp_path / "g.sam")
    st = _map(api, opt, name, alg, tag, out, max_batch_reads=1 << 14)
    assert_sam(out, name, alg, tag)
    assert st["simple_pairs"] > 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("name,alg", [("pe150", "nw"), ("pe250", "ksw2"), ("se", "ksw2")])
@pytest.mark.parametrize("tag", ["indel60", "maxmm0.1"])
def test_mapper_sam_with_small_batches(api, opt, tmp_path, name, alg, tag):
    """400-read batches: several batches, the insert-size estimate crossing their seams"""
    out = str(tmp_path / "g.sam")
    _map(api, opt, name, alg, tag, out, max_batch_reads=400)
    assert_sam(out, name, alg, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ALGS)
def test_two_mappers_on_one_index_keep_their_own_options(api, opt, tmp_path, alg):
    """A context with the defaults and one with -indel 100 -maxmm 0.1 on the same index, used in turn: each gives its own fixture every time
    (nothing of the options may live in what the contexts share: constant memory, statics, the index)."""
    ix = api.Index(opt["prefix"], device=0, full_sa=True)
    a = _mapper(api, ix, alg, "default", max_batch_reads=1 << 14)
    b = _mapper(api, ix, alg, "indel100_maxmm0.1", max_batch_reads=1 << 14)
    out = str(tmp_path / "g.sam")
    for name in ("pe150", "pe250", "se", "pe150"):
        for mp, tag in ((a, "default"), (b, "indel100_maxmm0.1"), (a, "default")):
            mp.reset()
            mp.map_files(opt[name][0], opt[name][1], out)
            assert_sam(out, name, alg, tag)
    a.close(); b.close(); ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("straight_line", [False, True])
def test_alignment_profile_equals_reference_at_indel_60(api, opt, monkeypatch, straight_line):
    if straight_line:
        monkeypatch.setenv("MCX_ORDER_MIN", "1")
    ix = api.Index(opt["prefix"], device=0, full_sa=True)
    G = ix.genome_size
    mp = _mapper(api, ix, "ksw2", "indel60", max_batch_reads=1000)
    planes = api.planes_alloc(G, "cuda")
    mp.profile_attach(planes.data_ptr())
    mp.map_files(opt["pe150"][0], opt["pe150"][1], None)
    mp.profile_finalize(planes.data_ptr())
    got = api.planes_view(planes, G).t().contiguous().cpu().numpy().astype(np.uint16)
    want = np.frombuffer(open(opt["pe150.ksw2.indel60.prof"], "rb").read(), dtype=np.uint16).reshape(-1, 10)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (bad[:5], got[bad[:5, 0]], want[bad[:5, 0]])
    text = api.sparse_to_maps_text(mp.profile_sparse())
    assert maps_canon(text) == maps_canon(open(opt["pe150.ksw2.indel60.maps"], encoding="latin-1").read())
    mp.close(); ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("straight_line", [False, True])
@pytest.mark.parametrize("tag", ["indel60", "maxmm0.1"])
def test_vcf_equals_reference(api, opt, tmp_path, monkeypatch, tag, straight_line):
    if straight_line:
        monkeypatch.setenv("MCX_ORDER_MIN", "1")
    o = VcfOpts([]).struct
    ix = api.Index(opt["prefix"], device=0, full_sa=True)
    mp = _mapper(api, ix, "ksw2", tag, max_batch_reads=4000)
    planes = api.planes_alloc(ix.genome_size, "cuda")
    mp.profile_attach(planes.data_ptr(), max_dup=o.max_dup, max_clip=o.max_clip)
    st = mp.map_files(opt["pe150"][0], opt["pe150"][1], None)
    mp.profile_finalize(planes.data_ptr())
    out = str(tmp_path / "o.vcf")
    switches = {k: getattr(o, k) for k in ("ploidy", "min_allele_depth", "min_cnv", "min_gap", "fragment_size", "filter", "gvcf", "monomorphic", "somatic")}
    ix.call_variants(planes.data_ptr(), mp.profile_sparse(), st["pairs"], st["pair_dist_sum"], st["pair_len_sum"], out,
                     sample_id="unknown", ref_name="ref", cmdline="test", **switches)
    got, want = vcf_body(out), vcf_body(opt[f"pe150.vcf.{tag}"])
    bad = [(x, y) for x, y in zip(got, want) if x != y]
    assert not bad and len(got) == len(want), (len(got), len(want), bad[:3])
    mp.close(); ix.close()


@pytest.mark.gpu
def test_multi_lines_at_indel_60(api, opt, tmp_path):
    """-m -indel 60: the further lines depend on the candidate list that clustering makes"""
    from test_multi import rebuild_multi
    extras = []
    for line in read_gz("pe150.ksw2.indel60.m.extra.gz").split("\n"):
        if line:
            i, rest = line.split("\t", 1)
            extras.append((int(i), rest))
    assert len(extras) == MANIFEST["multi"]["pe150.ksw2.indel60"] > 0
    want = rebuild_multi(expected_sam("pe150", "ksw2", "indel60"), extras).split("\n")
    out = str(tmp_path / "m.sam")
    _map(api, opt, "pe150", "ksw2", "indel60", out, multi=True)
    got = open(out, "rb").read().decode("latin-1").split("\n")
    bad = [(x, y) for x, y in zip(want, got) if x != y]
    assert len(got) == len(want) and not bad, (len(want), len(got), bad[:2])


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ["0", "0,0"])
@pytest.mark.parametrize("name,alg", [("pe150", "nw"), ("pe250", "ksw2"), ("se", "ksw2")])
def test_native_cli_takes_the_options(opt, tmp_path, devices, name, alg):
    """mapcaller-mi355x -indel 60 -maxmm 0.1 on one shard and on two with small batches: every shard's contexts carry the options"""
    f1, f2 = opt[name]
    sam = str(tmp_path / "o.sam")
    cmd = [EXE, "-i", opt["prefix"], "-f", f1] + (["-f2", f2] if f2 else []) + ["-alg", alg, "-sam", sam, "-no_vcf", "-t", "2", "-indel", "60", "-maxmm", "0.1",
                                                                               "-devices", devices, "-batch", "400"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    assert_sam(sam, name, alg, "indel60_maxmm0.1")


@pytest.mark.gpu
def test_native_cli_vcf_with_the_options(opt, tmp_path):
    f1, f2 = opt["pe150"]
    sam, vcf = str(tmp_path / "o.sam"), str(tmp_path / "o.vcf")
    subprocess.run([EXE, "-i", opt["prefix"], "-f", f1, "-f2", f2, "-alg", "ksw2", "-sam", sam, "-vcf", vcf, "-t", "2", "-maxmm", "0.1", "-devices", "0,0", "-batch", "600"],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    assert_sam(sam, "pe150", "ksw2", "maxmm0.1")
    assert vcf_body(vcf) == vcf_body(opt["pe150.vcf.maxmm0.1"])


@pytest.mark.gpu
def test_native_cli_clamps_indel_150(opt, tmp_path):
    f1, f2 = opt["pe250"]
    sam = str(tmp_path / "o.sam")
    r = subprocess.run([EXE, "-i", opt["prefix"], "-f", f1, "-f2", f2, "-alg", "nw", "-sam", sam, "-no_vcf", "-t", "2", "-indel", "150"],
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and "The maximal indel size is 100" in r.stderr, r.stderr[-500:]
    assert_sam(sam, "pe250", "nw", "indel100")


@pytest.mark.gpu
@pytest.mark.parametrize("alg,tag", [("ksw2", "indel100_maxmm0.1"), ("nw", "indel0"), ("ksw2", "maxmm0.02")])
def test_stream_boundary_on_a_context_with_options(api, opt, alg, tag):
    """mcx_stream_submit_packed / mcx_stream_map32 (three batches in flight) on a context created with the options: the records of mcx_map_batch on
    the same context, and FLAG, POS and CIGAR of every read are the fixture's."""
    import torch
    f1, f2 = opt["pe150"]
    r1 = [l for i, l in enumerate(open(f1, "rb").read().split(b"\n")) if i % 4 == 1]
    r2 = [l for i, l in enumerate(open(f2, "rb").read().split(b"\n")) if i % 4 == 1]
    n_pairs, per = 400, 3
    batches = []
    for b in range(per):
        seqs = [x for p in range(b * n_pairs, (b + 1) * n_pairs) for x in (r1[p], r2[p])]
        off = np.zeros(len(seqs) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(x) for x in seqs])
        batches.append((seqs, np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), off))
    ix = api.Index(opt["prefix"], device=0, full_sa=True)
    mp = _mapper(api, ix, alg, tag, max_batch_reads=2 * n_pairs)
    want = [mp.map_batch(bb, oo, True) for _, bb, oo in batches]
    mp.reset()
    pk = [api.pack_reads(torch.tensor(np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), -1).copy())) for seqs, _, _ in batches]
    arg = [(c.data_ptr(), rw, l.data_ptr(), o.data_ptr(), no) for c, l, o, no, rw in pk]
    outs = mp.stream_outputs(2 * n_pairs, per, 32)
    mp.map_stream_packed(arg, 2 * n_pairs, True, outputs=outs, out32=True)
    body = [l.split("\t") for l in expected_sam("pe150", alg, tag).split("\n") if l and not l.startswith("@")]
    for b in range(per):
        aln = api.aln32_unpack(np.frombuffer(outs[b][0].numpy().tobytes(), dtype=api.ALN32_DTYPE))
        pool = outs[b][1].numpy().view(np.uint32)
        w_aln, w_cig = want[b]
        for f in ("pos", "mate_pos", "chr", "flag", "mapq", "tlen", "nm", "as", "xs", "n_cigar", "fwd", "has_mate"):
            assert np.array_equal(aln[f], w_aln[f]), (b, f)
        for r in range(2 * n_pairs):
            words = pool[aln["cigar_off"][r]:aln["cigar_off"][r] + aln["n_cigar"][r]]
            assert np.array_equal(words, w_cig[r]), (b, r)
            f = body[b * 2 * n_pairs + r]
            ops = "".join(f"{int(w) >> 4}{'MIDNSHP='[int(w) & 7]}" for w in words) or "*"
            assert (int(aln["flag"][r]), int(aln["pos"][r]), ops) == (int(f[1]), int(f[3]), f[5]), (b, r, f[:9])
    mp.close(); ix.close()


@pytest.mark.gpu
def test_fuzz_rounds_with_options_equal_oracle():
    """scripts/fuzz_parity.py --opts, 40 rounds with a fixed seed: the CLI's SAM and VCF against the oracle's with -indel / -maxmm drawn per round"""
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), "--opts", "--rounds", "40", "--seed", "6060"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1400)
    assert r.returncode == 0 and "40 of 40 rounds identical" in r.stdout, r.stdout[-3000:]


@pytest.mark.gpu
def test_fuzz_rounds_with_options_on_the_large_batch_paths_equal_oracle(monkeypatch):
    """the same generator, mapping alone, with k_simple and the lane DP kernels forced onto the small batches: 40 rounds, the SAM against the oracle's"""
    monkeypatch.setenv("MCX_ORDER_MIN", "1")
    monkeypatch.setenv("MCX_DP_LANE_ALWAYS", "1")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "fuzz_parity.py"), "--opts", "--rounds", "40", "--seed", "7070", "--no-vcf"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1400)
    assert r.returncode == 0 and "40 of 40 rounds identical" in r.stdout, r.stdout[-3000:]
