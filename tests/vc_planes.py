"""Synthetic alignment-profile planes for the dense half of variant calling (mapcaller_amd/csrc/mcx_variants.hip): finalized
counters as int32 [10, G] in api.PLANES order, built from seeded numpy so that features sit on the edges of the kernels' parallel
structure.  A plain module (like dp_problems.py): the CPU test holds the stand-in against numpy restatements on these inputs and
checks their premises; the GPU test holds the kernels against the stand-in on the same inputs.

The launch arithmetic of GpuProfile::scan / k_vc_scan, restated from the source so that a case can check its own premise:
a lane per position, 256-position tiles, at most 8192 workgroups, each walking `per_group` consecutive tiles and staging up to 1024
records in LDS; the record list is first sized max(2^20, G / 64) and the scan repeated when it runs over; block depth is per 100."""
import math
from types import SimpleNamespace

import numpy as np

TILE, MAX_GROUPS, STAGE, BLOCK = 256, 256 * 32, 1024, 100
A, C, G_, T, MULTI, READ_COUNT, F1, R2, F2, R1 = range(10)
# SiteRec types (mcx_variants_host.h)
SUB, MON, GAP_START, GAP_END, DUP_START, DUP_END, NORM_START, NORM_END = 0, 11, 100, 101, 102, 103, 104, 105
RUN_LENGTHS = (1, 49, 50, 51)  # around -min_gap / -min_cnv (50)
LONG_RUN = 2000                # spans several groups
COV = 30                       # coverage of the background

TINY_SIZES = (1, 63, 64, 65, 255, 256, 257)
SMALL_G = 10_001      # 40 tiles, the last one partial, one tile a group; no multiple of 64 or 100
LARGE_G = 4_194_604   # 16 386 tiles, three a group, 5 462 groups; the last tile has 44 live lanes


def n_tiles(G):
    return -(-G // TILE)


def per_group(G):
    return -(-n_tiles(G) // min(n_tiles(G), MAX_GROUPS))


def n_groups(G):
    return -(-n_tiles(G) // per_group(G))


def cap0(G):
    return max(1 << 20, G // 64)


def pack_pac(codes):
    """codes 0..3 four a byte, the first in the two highest bits (the .pac layout ref_code reads)."""
    c = np.concatenate([codes.astype(np.uint8), np.zeros(-len(codes) % 4, dtype=np.uint8)]).reshape(-1, 4)
    return (c[:, 0] << 6 | c[:, 1] << 4 | c[:, 2] << 2 | c[:, 3]).astype(np.uint8)


def freq_floor(cov, min_ad=5):
    """eval_site's `ft`: the reads an ALT allele needs at a column of `cov` reads (FrequencyThr is a float 0.2 widened to double)."""
    return max(math.ceil(cov * float(np.float32(0.2))), min_ad)


def snv_kinds():
    """name -> ((reference reads, first ALT, second ALT), called with default switches?)."""
    f30, ad = freq_floor(30), 5
    assert freq_floor(19) == ad and freq_floor(19, 3) < ad  # at 19 reads -ad is what binds
    return {
        "over_freq": ((30 - f30, f30, 0), True), "under_freq": ((31 - f30, f30 - 1, 0), False),
        "over_ad": ((19 - ad, ad, 0), True), "under_ad": ((20 - ad, ad - 1, 0), False),
        "two_over": ((15, 8, 7), True), "two_under": ((16, 7, 7), False),  # both over `ft`; together half the column or one less
        "hom": ((0, 30, 0), True),
    }


class _Painter:
    def __init__(self, G, seed):
        rng = np.random.default_rng(seed)
        self.G = G
        self.codes = rng.integers(0, 4, G, dtype=np.uint8)
        rows = np.zeros((10, G), dtype=np.int32)
        rows[self.codes, np.arange(G)] = COV
        rows[MULTI] = rng.integers(0, 3, G, dtype=np.int32) * rng.integers(0, 40, G, dtype=np.int32)  # (beside coverage it decides nothing)
        rows[READ_COUNT] = rng.integers(0, 16, G, dtype=np.int32)
        rows[F1:R1 + 1] = rng.integers(0, 65536, (4, G), dtype=np.int32)
        self.rows = rows
        self.features = []  # (kind, first, last)
        self.snvs = []      # (position, kind)
        self.cursor = 0
        self.hi = G

    def note(self, kind, a, b):
        self.features.append((kind, a, b - 1))

    def gap(self, a, b, kind="gap"):
        self.rows[A:T + 1, a:b] = 0
        self.rows[MULTI, a:b] = 0
        self.note(kind, a, b)

    def dup(self, a, b, kind="dup"):
        self.rows[A:T + 1, a:b] = 0
        self.rows[MULTI, a:b] = 1 + np.arange(a, b) % 9
        self.note(kind, a, b)

    def column(self, p, counts):
        r = int(self.codes[p])
        self.rows[A:T + 1, p] = 0
        self.rows[r, p], self.rows[(r + 1) & 3, p], self.rows[(r + 2) & 3, p] = counts

    def snv(self, p, kind):
        self.column(p, snv_kinds()[kind][0])
        self.snvs.append((p, kind))
        self.note("snv:" + kind, p, p + 1)

    def alternate(self, a, b, even, odd, kind):
        """positions a, a + 2, .. take `even`, the others `odd`: 'c' covered, 'g' gap, 'd' dup"""
        for off, what in ((0, even), (1, odd)):
            s = slice(a + off, b, 2)
            if what != "c":
                self.rows[A:T + 1, s] = 0
                self.rows[MULTI, s] = 0 if what == "g" else 3
            else:
                self.rows[MULTI, s] = 0
        self.note(kind, a, b)

    def deep_step(self, edge, deep_left):
        """A 100-block of 400 reads a position beside one of the background's, the same ALT column on either side of the block edge:
        it is called in the shallow block only (cov_threshold is half the BLOCK's depth)."""
        assert edge % BLOCK == 0
        a = edge - BLOCK if deep_left else edge
        self.rows[A:T + 1, a:a + BLOCK] = 0
        self.rows[self.codes[a:a + BLOCK], np.arange(a, a + BLOCK)] = 400
        for p in (edge - 1, edge):
            self.column(p, snv_kinds()["over_freq"][0])
            self.snvs.append((p, "deep" if (p < edge) == deep_left else "over_freq"))
        self.note("deep_left" if deep_left else "deep_right", a, a + BLOCK)
        self.note("snv:step", edge - 1, edge + 1)

    # where the next feature of `length` goes so that its first (or last) position is `res` modulo `mod`; None when there is no room
    def place(self, length, anchor, mod, res, margin=3):
        base = self.cursor + margin
        t = base if anchor == "first" else base + length - 1
        t += (res - t) % mod
        first = t if anchor == "first" else t - length + 1
        if first + length + margin > self.hi:
            return None
        self.cursor = first + length
        return first


def _constraints(G):
    span = TILE * per_group(G)
    c = [(TILE, r) for r in (0, 1, 63, 64, 255)] + [(span, 0), (span, span - 1), (BLOCK, 0), (BLOCK, BLOCK - 1)]
    return list(dict.fromkeys(c))


def _edge_pass(p, full, shift=0):
    """Runs and ALT columns whose first / last positions sit on every constraint.  full: every kind x length x anchor at every
    constraint; otherwise kinds and lengths take turns.  False as soon as the region is full."""
    cons = _constraints(p.G)
    n = shift
    for mod, res in cons:
        for anchor in ("first", "last"):
            combos = [(k, ln) for k in ("gap", "dup") for ln in RUN_LENGTHS] if full else [(("gap", "dup")[n % 2], RUN_LENGTHS[(n // 2) % 4])]
            for kind, ln in combos:
                a = p.place(ln, anchor, mod, res)
                if a is None:
                    return False
                (p.gap if kind == "gap" else p.dup)(a, a + ln)
                n += 1
    kinds = list(snv_kinds())
    for i, (mod, res) in enumerate(cons):
        for kind in (kinds if full else [kinds[(i + shift) % len(kinds)]]):
            a = p.place(1, "first", mod, res)
            if a is None:
                return False
            p.snv(a, kind)
    return True


def _pairs(p):
    """gap directly followed by dup and the reverse: an end and a start record at one position, the seam at a tile edge."""
    for first, second in ((p.gap, p.dup), (p.dup, p.gap)):
        a = p.place(101, "first", TILE, TILE - 50)
        assert a is not None
        first(a, a + 50); second(a + 50, a + 101)


def _step(p, deep_left, group_edge):
    """a block-depth step; group_edge: where the block edge is a group edge as well"""
    mod = math.lcm(BLOCK, TILE * per_group(p.G)) if group_edge else BLOCK
    a = p.place(2 * BLOCK, "first", mod, (-BLOCK) % mod, margin=BLOCK)
    assert a is not None
    p.deep_step(a + BLOCK, deep_left)


def _finish(p, **extra):
    edges = sorted({q for _, a, b in p.features for q in (a - 1, a, b, b + 1) if 0 <= q < p.G})
    return SimpleNamespace(G=p.G, rows=p.rows, codes=p.codes, pac=pack_pac(p.codes), features=p.features, snvs=p.snvs, edges=np.array(edges, dtype=np.int64), **extra)


def tiny(G, what):
    """what: 'gap' (nothing mapped anywhere), 'covered', 'feature' (a dup run in the middle third, an ALT column on the last position)."""
    p = _Painter(G, 1000 + G)
    if what == "gap":
        p.gap(0, G)
    elif what == "feature":
        if G >= 3:
            p.dup(G // 3, 2 * G // 3)
        p.snv(G - 1, "hom")
    else:
        assert what == "covered"
    return _finish(p)


def small():
    """G = 10 001: runs open at both genome ends, every edge constraint, the long run over eight groups."""
    G = SMALL_G
    p = _Painter(G, 7)
    p.gap(0, 51, "gap:open_start")
    p.cursor = 51
    p.hi = G - 60
    p.dup(G - 60, G, "dup:open_end")
    _pairs(p)
    _step(p, False, False)
    p.hi = 6200
    assert _edge_pass(p, full=False), "the pass over the edge constraints did not fit"
    _edge_pass(p, full=False, shift=5)  # (as much of another turn of kinds and lengths as fits)
    p.hi = G - 60
    _step(p, True, True)  # (at 6400, the one place where a block edge is a tile edge)
    a = p.place(LONG_RUN, "first", TILE, 63)
    assert a is not None
    p.gap(a, a + LONG_RUN, "gap:long")
    shift = 3
    while _edge_pass(p, full=False, shift=shift):  # (as many more turns of kinds and lengths as fit)
        shift += 3
    return _finish(p)


def large(overflow=600_000):
    """G = 4 194 604, three tiles a group.  Dense windows (covered / gap in turn: two records a position under -gvcf, three every
    two under -monomorphic) over the first group, a middle one and the last whole one, an ALT column in each; the overflow stretch
    (gap / dup in turn: two boundary records a position with any switches) with covered islands every 50 000 positions; every
    edge constraint in full before the stretch and after it."""
    G = LARGE_G
    span = TILE * per_group(G)
    assert per_group(G) == 3 and n_groups(G) == 5462 and G % TILE == 44
    p = _Painter(G, 11)
    groups = (0, n_groups(G) // 2, n_groups(G) - 2)
    windows = [(g * span, (g + 1) * span) for g in groups]
    # before the stretch
    p.cursor, p.hi = windows[0][1], 400_000
    _pairs(p)
    _step(p, True, True)
    _step(p, False, False)
    assert _edge_pass(p, full=True)
    # the stretch
    ov = (400_001, 400_001 + overflow)  # (an odd start: the pairs straddle tiles, groups and blocks both ways)
    assert ov[1] + 200_000 < windows[1][0]
    p.alternate(ov[0], ov[1], "g", "d", "overflow")
    for k, at in enumerate(range(ov[0] + 50_000, ov[1] - 400, 50_000)):
        a = at + 7 * k
        p.rows[A:T + 1, a:a + 300] = 0
        p.rows[p.codes[a:a + 300], np.arange(a, a + 300)] = COV
        p.note("island", a, a + 300)
        p.snv(a + 100, "hom")
        p.gap(a + 150, a + 150 + RUN_LENGTHS[k % 4])
    # behind it
    p.cursor, p.hi = ov[1] + 10, windows[1][0]
    a = p.place(LONG_RUN, "last", span, 5)
    p.dup(a, a + LONG_RUN, "dup:long")
    _pairs(p)
    _step(p, False, True)
    _step(p, True, False)
    assert _edge_pass(p, full=True, shift=1)
    # the last group: its tiles' edges, the partial tile, a run that reaches the genome end
    p.cursor, p.hi = windows[2][1], G - 30
    _edge_pass(p, full=False)  # (as far as it fits)
    p.dup(G - 30, G, "dup:open_end")
    for (a, b), kind in zip(windows, ("over_freq", "two_over", "hom")):
        p.alternate(a, b, "g", "c", "window")  # (the first window opens a run at position 0)
        q = a + span // 2 + 1
        assert (q - a) % 2 == 1
        p.snv(q, kind)
    return _finish(p, windows=windows, overflow=ov, span=span)


# ---- what the tests ask of a case --------------------------------------------------------------------------------------------
# name -> (the switches as MapCaller's command line spells them, the same as fields of mcx_vcf_opts)
SWITCHES = {
    "default": ([], {}), "gvcf": (["-gvcf"], {"gvcf": 1}), "mono": (["-monomorphic"], {"monomorphic": 1}),
    "somatic": (["-somatic"], {"somatic": 1}), "ploidy1": (["-ploidy", "1"], {"ploidy": 1}), "ad3": (["-ad", "3"], {"min_allele_depth": 3}),
}
SITE_FIELDS = ("pos", "type", "geno", "qscore", "alt", "DP", "AD_ref", "AD_alt", "pad")


def positions_for(case):
    """columns: the fixed positions (outside the genome too) and every feature edge"""
    G = case.G
    return np.concatenate([np.array([-1, 0, 99, 100, 255, 256, G - 1, G, G + 1000], dtype=np.int64), case.edges])


def ranges_for(case):
    """(beg, end, mode) rows: lengths 1, 63, 64, 65, 1000 from fixed starts and feature edges, ranges that begin before the genome,
    end behind it or lie outside it, and the uncovered runs themselves (a minimum over nothing: ~0)."""
    G = case.G
    starts = [0, 1, 63, 64, 100, 255, 256, G // 2, G - 65, G - 1] + [int(e) for e in case.edges[:: max(1, len(case.edges) // 24)]]
    out = []
    for mode in (0, 1):
        out += [(s, s + ln - 1, mode) for ln in (1, 63, 64, 65, 1000) for s in starts]
        out += [(-5, 10, mode), (-64, -1, mode), (-1000, 999, mode), (G, G + 63, mode), (G - 3, G + 1000, mode), (G + 5, G + 5, mode), (-70, min(G, 3000) + 70, mode)]
        out += [(a, b, mode) for kind, a, b in case.features if kind.split(":")[0] in ("gap", "dup")][:40]
    return np.array(out, dtype=np.int64)


def same_sites(got, want):
    """None, or where two record lists first differ (every field, in order)."""
    if len(got) != len(want):
        return f"{len(got)} records for {len(want)}"
    for f in SITE_FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        if bad.size:
            i = int(bad[0])
            return f"record {i} ({f}): {got[i]} for {want[i]}; {bad.size} differ"
    return None


def host_dense(L, case, switch="default", positions=(), ranges=np.zeros((0, 3), dtype=np.int64)):
    """hostemu_vc_dense (tests/hostemu/hostemu_variants.cpp; L: the hostemu_variants_lib fixture) on a case with a switch set of
    SWITCHES: (records, columns, range values) as numpy arrays in the dtypes of api.vc_dense."""
    import ctypes as C
    from conftest import VcfOpts
    from mapcaller_amd.api import VC_SITE_DTYPE as site_dtype, VC_COLUMN_DTYPE as column_dtype, VC_RANGE_DTYPE as range_dtype
    opts = VcfOpts(SWITCHES[switch][0])
    L.hostemu_vc_dense.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
    L.hostemu_vc_dense.restype = C.c_int
    rows = np.ascontiguousarray(case.rows, dtype=np.int32)
    pos = np.ascontiguousarray(positions, dtype=np.int64)
    rq = np.zeros(len(ranges), dtype=range_dtype)
    if len(ranges):
        rq["beg"], rq["end"], rq["mode"] = ranges[:, 0], ranges[:, 1], ranges[:, 2]
    cols = np.zeros(len(pos), dtype=column_dtype)
    vals = np.zeros(len(rq), dtype=np.uint64)
    p_sites, n_sites = C.c_void_p(), C.c_uint64()
    rc = L.hostemu_vc_dense(case.pac.ctypes.data, case.G, rows.ctypes.data, opts.ref, pos.ctypes.data, len(pos), rq.ctypes.data, len(rq),
                            C.byref(p_sites), C.byref(n_sites), cols.ctypes.data, vals.ctypes.data)
    assert rc == 0, L.hostemu_vc_error()
    sites = np.empty(int(n_sites.value), dtype=site_dtype)
    if len(sites):
        C.memmove(sites.ctypes.data, p_sites.value, sites.nbytes)
    return sites, cols, vals
