"""The dense half of -vcf on the GPU (mcx_variants.hip: k_vc_depth, k_vc_scan, the key / radix-sort / permute step, k_vc_gather,
k_vc_range — through mcx_vc_dense_dev) against the one-position-at-a-time stand-in (hostemu_vc_dense, itself held against numpy in
test_vc_dense_host.py), record by record and field by field, on the synthetic planes of vc_planes.py: tile, wave, group and block
edges, the several-tile path with its carried neighbour and mid-loop flush (G = 4 194 604: three tiles a group), the repeat after
the record list ran over.  Then the whole call on the small planes, and mcx_profile_settle / _finalize on synthetic differences
against numpy in int64."""
import numpy as np
import pytest

import vc_planes as vp
from conftest import VcfOpts, vcf_body

pytestmark = pytest.mark.gpu

TINY = [f"tiny{G}-{what}" for G in vp.TINY_SIZES for what in ("gap", "covered", "feature")]


@pytest.fixture(scope="module")
def api():
    from mapcaller_amd import api as a
    a.lib()  # raises if the HIP extension is missing: there is no fallback
    assert a.device_count() >= 1, "no GPU visible"
    return a


class Dev:
    """a case with its planes and packed genome in HBM"""

    def __init__(self, api, case):
        import torch
        self.api, self.case = api, case
        self.planes = api.planes_from_rows(torch.from_numpy(case.rows).cuda())
        self.pac = torch.from_numpy(case.pac).cuda()
        torch.cuda.synchronize()

    def dense(self, switch="default", positions=(), ranges=()):
        return self.api.vc_dense(self.pac.data_ptr(), self.case.G, self.planes.data_ptr(), positions, ranges, **vp.SWITCHES[switch][1])


def make_case(name):
    if name == "small":
        return vp.small()
    G, what = name[4:].split("-")
    return vp.tiny(int(G), what)


def check_all(dev, host_lib, switch):
    """records, columns and range values of one call against the stand-in's"""
    case = dev.case
    pos, rq = vp.positions_for(case), vp.ranges_for(case)
    want_sites, want_cols, want_vals = vp.host_dense(host_lib, case, switch, pos, rq)
    sites, cols, vals = dev.dense(switch, pos, rq)
    assert vp.same_sites(sites, want_sites) is None, (switch, vp.same_sites(sites, want_sites))
    for f in ("v", "depth", "ref"):
        assert np.array_equal(cols[f], want_cols[f]), (switch, f, pos[np.flatnonzero((cols[f] != want_cols[f]).reshape(len(pos), -1).any(axis=1))[:5]])
    assert np.array_equal(vals, want_vals), (switch, rq[np.flatnonzero(vals != want_vals)[:5]])
    return len(sites)


@pytest.mark.parametrize("name", TINY + ["small"])
def test_dense_equals_stand_in(api, hostemu_variants_lib, name):
    """every switch set the scan reads, columns at the fixed positions and every feature edge, ranges in both modes"""
    dev = Dev(api, make_case(name))
    counts = {s: check_all(dev, hostemu_variants_lib, s) for s in vp.SWITCHES}
    if name == "small":
        assert counts["mono"] > counts["gvcf"] > counts["default"] > 0 and counts["somatic"] > counts["default"] and counts["ad3"] > counts["default"]


# ---- the large size: one set of planes for the module ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large(api):
    dev = Dev(api, vp.large())
    yield dev
    del dev.planes, dev.pac


@pytest.mark.parametrize("switch", ["default", "gvcf", "mono"])
def test_large_dense_equals_stand_in(large, hostemu_variants_lib, switch):
    """Three tiles a group: the neighbour's class carried from tile to tile, records staged across tiles, the flush in the middle
    of a group's walk (-gvcf, -monomorphic: the windows), and — with every switch set — a list longer than its first sizing."""
    G = large.case.G
    n = check_all(large, hostemu_variants_lib, switch)
    print(f"large {switch}: {n} records against cap0 {vp.cap0(G)}")
    assert vp.per_group(G) >= 3 and n > vp.cap0(G)
    if switch == "default":
        assert n < 1.25 * vp.cap0(G)  # a little over


def test_overflow_twice_then_a_small_call(api, hostemu_variants_lib):
    """More than twice the first sizing; and the process is none the worse for it: a small call afterwards is still right."""
    import torch
    case = vp.large(overflow=1_100_000)
    dev = Dev(api, case)
    want, _, _ = vp.host_dense(hostemu_variants_lib, case)
    sites, _, _ = dev.dense()
    print(f"large-twice default: {len(sites)} records against cap0 {vp.cap0(case.G)}")
    assert len(want) > 2 * vp.cap0(case.G)
    assert vp.same_sites(sites, want) is None, vp.same_sites(sites, want)
    del dev, sites, want
    torch.cuda.empty_cache()
    small = Dev(api, vp.small())
    for s in ("default", "mono"):
        check_all(small, hostemu_variants_lib, s)


# ---- the whole call at the small size --------------------------------------------------------------------------------------------
def test_whole_call_on_small_planes(api, hostemu_variants_lib, tmp_path):
    """mcx_call_variants over the small planes (two contigs, 6 000 + 4 001) with a few insert / delete / clip records at a wave
    edge, a tile edge and the contig edge: the VCF of the GPU path equals the VCF of the host logic over the stand-in, line for line."""
    import torch
    case = vp.small()
    codes = torch.from_numpy(case.codes).cuda()
    ix = api.Index.from_codes(codes.data_ptr(), [6000, 4001], ["c1", "c2"], device=0)
    prefix = str(tmp_path / "small")
    ix.save(prefix)
    planes = api.planes_from_rows(torch.from_numpy(case.rows).cuda())
    torch.cuda.synchronize()
    prof, maps = str(tmp_path / "small.prof"), str(tmp_path / "small.maps")
    np.ascontiguousarray(case.rows.T).astype(np.uint16).tofile(prof)
    sparse = [("I", 255, "AC")] * 8 + [("D", 256, "G")] * 8 + [("I", 5999, "T")] * 9 + [("D", 6000, "CA")] * 8 + [("I", 4351, "GG")] * 12 \
        + [("B", 255, "")] * 3 + [("B", 256, "")] * 2 + [("B", 6000, "")] * 4
    open(maps, "w").write(api.sparse_to_maps_text(sparse))
    n_lines = {}
    for name, (args, fields) in vp.SWITCHES.items():
        got, want = str(tmp_path / f"gpu.{name}.vcf"), str(tmp_path / f"host.{name}.vcf")
        ix.call_variants(planes.data_ptr(), sparse, 0, 0, 0, got, ref_name="ref", cmdline="test", **fields)
        rc = hostemu_variants_lib.hostemu_call_variants(prefix.encode(), prof.encode(), maps.encode(), 0, 0, 0, VcfOpts(args).ref, want.encode())
        assert rc == 0, hostemu_variants_lib.hostemu_vc_error()
        a, b = vcf_body(got), vcf_body(want)
        assert a == b, (name, [(x, y) for x, y in zip(a, b) if x != y][:3], len(a), len(b))
        n_lines[name] = sum(1 for l in a if l and not l.startswith("#"))
    assert n_lines["default"] > 10 and n_lines["mono"] > 3000 and n_lines["gvcf"] > n_lines["default"]
    assert any("TYPE=ins" in l for l in a) and any("TYPE=del" in l for l in a)
    ix.close()


# ---- settle and finalize on synthetic differences --------------------------------------------------------------------------------
def _difference_planes(api, G, seed):
    """The planes' words as a run leaves them before mcx_profile_settle, and what settle + finalize must make of them (numpy, int64).
    Strand planes: words (L + 65536 H) mod 2^32 with the true differences L in [-32768, 32767] in the low half and H in [0, 65535]
    in the high one.  multi_hit: differences whose running sum stays >= 0 and crosses 4095.  A C G T, readCount: counts."""
    rng = np.random.default_rng(seed)
    stride = api.planes_stride(G)
    words = np.zeros(stride * 11 // 2, dtype=np.uint32)
    half_words = words[stride:].reshape(9, stride // 2)
    half = words[stride:].view(np.uint16).reshape(9, stride)
    want = np.zeros((10, G), dtype=np.int64)
    nw = (G + 1) // 2
    for k in (vp.F1, vp.R2, vp.F2, vp.R1):
        L = rng.integers(-32768, 32768, nw, dtype=np.int64)
        H = rng.integers(0, 65536, nw, dtype=np.int64)
        head = [(-1, 0), (-1, 65535), (0, 0), (0, 0), (-32768, 65535), (32767, 0), (-1, 1), (0, 65535), (-32768, 0)]
        for i, (lo, hi) in enumerate(head[:nw]):
            L[i], H[i] = lo, hi
        if k == vp.R2:  # mostly zeros, as a real run leaves the planes: the few words travel far before the next
            quiet = rng.random(nw) < 0.97
            quiet[:len(head)] = False
            L[quiet] = 0
            H[quiet] = 0
        if G & 1:
            H[-1] = 0  # (the high half of the last word lies behind the genome)
        half_words[k - 1, :nw] = ((L + 65536 * H) % (1 << 32)).astype(np.uint32)
        d = np.stack([L, H], axis=1).reshape(-1)[:G]
        want[k] = np.cumsum(d) & 0xFFFF
    # multi_hit: the differences of a level that is never negative and, over an eighth of the genome, lies on both sides of 4095
    level = rng.integers(0, 3000, G, dtype=np.int64)
    level[G // 2:G // 2 + G // 8] += 2500
    level[G // 4] = 4095; level[G // 4 + 1] = 4096; level[G // 4 + 2] = 1 << 20
    d = np.diff(np.concatenate([[0], level]))
    assert level.min() >= 0 and (level > 4095).sum() > G // 32 and (d < 0).any()
    words[:G] = (d % (1 << 32)).astype(np.uint32)
    words[G:stride] = 777  # behind the genome: neither scanned nor clamped
    want[vp.MULTI] = np.minimum(level, 4095)
    # counts: a half over the cap beside one at or under it, both, neither, the cap itself and one more
    for k in (vp.A, vp.C, vp.G_, vp.T, vp.READ_COUNT):
        top = 4095 if k != vp.READ_COUNT else 5
        v = rng.integers(0, 3 * top, G, dtype=np.int64)
        v[rng.random(G) < 0.5] //= 4
        edge = np.array([top + 1, top, top, top + 1, top + 1, top + 1, top - 1, top, 0, 14999 if k != vp.READ_COUNT else 15, 0, 0], dtype=np.int64)
        v[:min(G, len(edge))] = edge[:G]
        half[k if k < vp.MULTI else k - 1, :G] = v.astype(np.uint16)
        want[k] = np.minimum(v, top)
    return words, want


@pytest.fixture(scope="module")
def big_index(api):
    """an index of the large size's order: 4 194 604 random bases in two contigs, built on the GPU"""
    import torch
    g = torch.Generator().manual_seed(5)
    codes = torch.randint(0, 4, (vp.LARGE_G,), generator=g, dtype=torch.uint8).cuda()
    ix = api.Index.from_codes(codes.data_ptr(), [3_000_000, vp.LARGE_G - 3_000_000], device=0)
    print(f"index of {vp.LARGE_G} bases built in {ix.build_seconds:.2f} s")
    yield ix
    ix.close()


@pytest.mark.parametrize("size", ["small", "large"])
def test_settle_and_finalize_on_synthetic_differences(api, request, size):
    """No batch mapped: mcx_profile_settle decodes the strand planes' words and scans them modulo 2^16, scans multi_hit in 32 bits;
    mcx_profile_finalize clamps multi_hit and A C G T at 4095 and readCount at -dup, half by half."""
    import torch
    if size == "small":
        case = vp.small()
        codes = torch.from_numpy(case.codes).cuda()
        ix = api.Index.from_codes(codes.data_ptr(), [6000, 4001], device=0)
    else:
        ix = request.getfixturevalue("big_index")
    G = ix.genome_size
    words, want = _difference_planes(api, G, 21 if size == "small" else 22)
    planes = torch.from_numpy(words.view(np.int32)).cuda()
    torch.cuda.synchronize()
    mp = api.Mapper(ix, alg="ksw2", max_batch_reads=1 << 10)
    mp.profile_attach(planes.data_ptr(), max_dup=5)
    mp.profile_settle()
    mp.profile_finalize(planes.data_ptr())
    torch.cuda.synchronize()
    got = api.planes_view(planes, G).cpu().numpy().astype(np.int64)
    for k, name in enumerate(api.PLANES):
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (name, bad[:5], got[k][bad[:5]], want[k][bad[:5]])
    stride = api.planes_stride(G)
    assert (planes[G:stride].cpu().numpy() == 777).all()  # multi_hit behind the genome: untouched
    mp.close()
    if size == "small":
        ix.close()
