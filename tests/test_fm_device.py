"""The GPU index builder, the loader's derived tables and the seeding walk against a plain suffix array (tests/fm_ref.py) on the
texts of tests/fm_cases.py: sizes that leave short last words, samples and blocks, texts whose suffixes stay tied until the
terminator decides, intervals of exactly 50 and of more than 50 rows, reads over the strand junction, the text's end and the
16- and 32-base word edges.  Everything is integers and bytes: nothing has a tolerance.

The files the builder writes are compared with the ones the reference's indexer wrote (tests/golden/fm_edges), or with the
plain restatement where the reference cannot index the text (below 15 bases); the searches and walks with the restatement,
which tests/test_fm_host.py holds against the reference's own BWT_Search results."""

import pytest

import fm_cases
import fm_ref
from test_fm_host import EXTS, fixture_files

pytestmark = pytest.mark.gpu

CASES = fm_cases.cases()
WALK_CASES = [n for n, c in CASES.items() if c.has_reads]
BUCKET_CASES = [n for n, c in CASES.items() if c.kind == "deep" or n in ("g129", "g4099")]
SEARCH_CASES = [n for n, c in CASES.items() if c.kind in ("deep", "threshold")]
CAP = 1024
BUDGETS = (1, 3, 1 << 30)


@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()  # raises if the HIP extension is missing: there is no fallback
    assert a.device_count() >= 1, "no GPU visible"
    return a


def expected_files(case):
    """ext -> bytes: the reference-made files where there are any, the plain restatement's otherwise"""
    want = dict(case.files())
    want.update(fixture_files(case) if case.has_fixture else {})
    return want


def resolved_contigs(case):
    """the contigs as Index.from_codes sees them: letters outside ACGT already drawn, no comments"""
    fwd, _holes, anns = fm_ref.forward_codes(case.contigs)
    return [(name, None, "".join("ACGT"[c] for c in fwd[off:off + ln])) for (name, _c, _s), (off, ln, _a) in zip(case.contigs, anns)]


def device_codes(case):
    import torch
    return torch.from_numpy(fm_ref.forward_codes(case.contigs)[0].copy()).cuda()


# ---- builder ------------------------------------------------------------------------------------
def _build_and_compare(api, case, tmp_path):
    fa = str(tmp_path / ("ref.fa.gz" if case.gz else "ref.fa"))
    with open(fa, "wb") as fh:
        fh.write(case.fasta_file_bytes())
    prefix = str(tmp_path / "built")
    api.Index.build(fa, prefix, 0)
    want = expected_files(case)
    for e in EXTS:
        assert open(f"{prefix}.{e}", "rb").read() == want[e], e


@pytest.mark.parametrize("name", list(CASES))
def test_builder_writes_the_reference_files(api, tmp_path, monkeypatch, name):
    monkeypatch.delenv("MCX_BUILD_BUCKET_BASES", raising=False)
    _build_and_compare(api, CASES[name], tmp_path)


@pytest.mark.parametrize("bucket_bases", ["1", "3", "4"])
@pytest.mark.parametrize("name", BUCKET_CASES)
def test_builder_by_buckets_writes_the_reference_files(api, tmp_path, monkeypatch, name, bucket_bases):
    """buckets of the first 1, 3 and 4 bases: empty ones, ones that hold nearly everything, ones that finish in different rounds"""
    monkeypatch.setenv("MCX_BUILD_BUCKET_BASES", bucket_bases)
    _build_and_compare(api, CASES[name], tmp_path)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c.note])
def test_from_codes_saves_the_reference_files(api, tmp_path, monkeypatch, name):
    monkeypatch.delenv("MCX_BUILD_BUCKET_BASES", raising=False)
    case = CASES[name]
    codes = device_codes(case)
    ix = api.Index.from_codes(codes.data_ptr(), [len(c[2]) for c in case.contigs], [c[0] for c in case.contigs], device=0, full_sa=1)
    try:
        prefix = str(tmp_path / "saved")
        ix.save(prefix)
    finally:
        ix.close()
    want = expected_files(case)
    plain = fm_ref.index_files(resolved_contigs(case))
    for e in ("bwt", "sa", "pac"):
        assert open(f"{prefix}.{e}", "rb").read() == want[e], e
    for e in ("ann", "amb"):  # (an index made from codes has no comments and no holes to tell of)
        assert open(f"{prefix}.{e}", "rb").read() == plain[e], e


# ---- loader and derived tables ------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c.note and c.G <= fm_cases.MAX_WALK_G])
def test_every_text_loads_at_every_level(api, tmp_path, monkeypatch, name):
    """levels 0, 1, 2: the expanded suffix array, the jump table, the rank records and the pair records are made for every size;
    at level 2 the pair records' self-check runs 4096 trials"""
    case = CASES[name]
    prefix = fm_cases.write_index(case, str(tmp_path / "idx"))
    for e, data in (fixture_files(case) if case.has_fixture else {}).items():
        assert case.files()[e] == data, e  # (the files loaded are the reference's own)
    monkeypatch.setenv("MCX_RANK2_CHECK", "4096")
    for level in (0, 1, 2):
        ix = api.Index(prefix, device=0, full_sa=level)
        try:
            assert ix.genome_size == case.G
            assert ix.chromosomes == [(c[0], len(c[2])) for c in case.contigs]
        finally:
            ix.close()


# ---- search ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SEARCH_CASES)
def test_bwt_search_equals_the_plain_search(api, tmp_path, name):
    case, text = CASES[name], CASES[name].text()
    queries = []
    for _tag, codes in fm_cases.reads_for(case):
        pos, starts = 0, []
        while pos < len(codes) - 16:  # the walk's own starts, and the read's first base
            if codes[pos] > 3:
                pos += 1
                continue
            starts.append(pos)
            pos += fm_ref.search(text, codes, pos)[0] + 1
        if codes[0] <= 3 and 0 not in starts:
            starts.append(0)
        queries += [(codes, s) for s in starts]
    assert len(queries) >= 300
    ix = api.Index(fm_cases.write_index(case, str(tmp_path / "idx")), device=0)
    mp = api.Mapper(ix, max_batch_reads=1 << 10)
    try:
        ln, fr, loc = mp.bwt_search([q for q, _s in queries], [s for _q, s in queries])
    finally:
        mp.close()
        ix.close()
    bad = []
    for i, (codes, s) in enumerate(queries):
        w_len, w_freq, w_loc, _n = fm_ref.search(text, codes, s)
        if (int(ln[i]), int(fr[i]), [int(x) for x in loc[i, :int(fr[i])]]) != (w_len, w_freq, w_loc):
            bad.append((i, s, w_len, w_freq, int(ln[i]), int(fr[i])))
    assert not bad, (len(bad), bad[:3])


# ---- walk -----------------------------------------------------------------------------------------------
def _walk_and_compare(api, ix, case, what, budgets=BUDGETS):
    seqs = [fm_cases.ascii_of(codes) for _tag, codes in fm_cases.reads_for(case)]
    mp = api.Mapper(ix, max_batch_reads=1 << 10)
    try:
        for fm_budget in budgets:
            n_hits, hits = mp.seed_walk(seqs, fm_budget=fm_budget, cap=CAP)
            assert int(n_hits.max()) <= CAP
            bad = fm_cases.compare_walks(case, n_hits, hits, CAP)
            assert not bad, (what, fm_budget, len(bad), bad[:2])
    finally:
        mp.close()


# (level, MCX_KTAB_K, MCX_NO_RANK): one index and one context per case — a context takes seconds to make now and then
WALK_SETTINGS = [(level, k, False) for level in (0, 1, 2) for k in (None, "4")] + [(1, k, True) for k in (None, "4")]


@pytest.mark.parametrize("setting", WALK_SETTINGS, ids=[f"level{l}" + ("-k4" if k else "") + ("-norank" if nr else "") for l, k, nr in WALK_SETTINGS])
@pytest.mark.parametrize("name", WALK_CASES)
def test_seed_walk_equals_the_plain_walk(api, tmp_path, monkeypatch, name, setting):
    """Mapper.seed_walk on an index loaded from files: the jump table at its own K and at K = 4, at level 1 also without the rank
    records (the walk then counts in the .bwt blocks), each with 1, 3 and 2^30 FM steps per turn; every triple in order"""
    case = CASES[name]
    level, ktab_k, no_rank = setting
    prefix = fm_cases.write_index(case, str(tmp_path / "idx"))
    monkeypatch.delenv("MCX_KTAB_K", raising=False)
    monkeypatch.delenv("MCX_NO_RANK", raising=False)
    if ktab_k:
        monkeypatch.setenv("MCX_KTAB_K", ktab_k)
    if no_rank:
        monkeypatch.setenv("MCX_NO_RANK", "1")
    ix = api.Index(prefix, device=0, full_sa=level)
    try:
        _walk_and_compare(api, ix, case, setting)
    finally:
        ix.close()


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("name", WALK_CASES)
def test_seed_walk_on_an_index_built_from_codes(api, monkeypatch, name, level):
    for v in ("MCX_KTAB_K", "MCX_NO_RANK", "MCX_BUILD_BUCKET_BASES"):
        monkeypatch.delenv(v, raising=False)
    case = CASES[name]
    codes = device_codes(case)
    ix = api.Index.from_codes(codes.data_ptr(), [len(c[2]) for c in case.contigs], [c[0] for c in case.contigs], device=0, full_sa=level)
    try:
        _walk_and_compare(api, ix, case, ("from_codes", level), budgets=(1, 1 << 30))
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["threshold", "homopolymer", "g129"])
def test_seed_walk_counts_past_its_capacity(api, tmp_path, name):
    """cap = 8: the first eight hits and the full count"""
    case = CASES[name]
    seqs = [fm_cases.ascii_of(codes) for _tag, codes in fm_cases.reads_for(case)]
    want = fm_cases.expected_walks(case)
    if name == "threshold":
        assert max(len(w) for w in want) > 8
    ix = api.Index(fm_cases.write_index(case, str(tmp_path / "idx")), device=0, full_sa=2)
    mp = api.Mapper(ix, max_batch_reads=1 << 10)
    try:
        n_hits, hits = mp.seed_walk(seqs, fm_budget=3, cap=8)
    finally:
        mp.close()
        ix.close()
    bad = fm_cases.compare_walks(case, n_hits, hits, 8)
    assert not bad, (len(bad), bad[:2])
