// tests/hostemu/cluster_regs_check.cpp — k_cluster's register path (mapcaller_amd/csrc/mcx_glue.h cluster_read<CAP>, stage_cluster_pair_regs<CAP>;
// mcx_types.h hit_pack, packed_hits_fit) on the host, against the memory path it replaces.
//
// For each CAP in {4, 8, 16, 32} and each hit list, cluster_read<CAP> must leave what prep_seeds + cluster_seeds leave: the same count of kept hits, the
// same bytes in the whole hit list (the sorted front and the untouched rest), the same candidates, the same number of clusters (hence the same overflow
// outcome).  Lists: n = 0, 1, CAP - 1, CAP, CAP + 1 (the memory path by itself); every hit dropped (PosDiff <= 0) and mixes of kept and dropped; sorted,
// reversed and suffix-array-like order; equal keys; a tandem run (score >= rlen); clusters split by a contig end and by max_pos_diff; more clusters than
// cand_seed; gPos at 2^34 - 1 with rPos and len at 1023; and a few thousand random lists per CAP from a fixed seed.  Pairs of such lists go through
// stage_cluster_pair_regs<CAP> and through stage_cluster_pair + the two stores k_cluster used to add: the records must be equal byte for byte, and the
// flags and the two lists' decisions handed back must be what the kernel read from the header before.  The guard is asked around its bounds.
//
// Built with -fsanitize=address,undefined (tests/test_cluster_regs_host.py); the buffers are exactly as long as the capacities.
//   cluster_regs_check     exit status 0 when every case agrees
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mapcaller_amd/csrc/mcx_glue.h"

using namespace mcx;

static int g_bad = 0;
static long g_cases = 0, g_sorted = 0, g_tandem = 0, g_over = 0, g_fallback = 0, g_dropped = 0;

struct Rng { // xorshift64*: the lists depend on the seed alone
    uint64_t s;
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 2685821657736338717ull; }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

static const int64_t kEnds[] = {1000000, 2000000, ((int64_t)1 << 33), ((int64_t)1 << 34) + 2000}; // contig ends ("positions" run past 2^34 - 1 for the packing's own bounds)
static IndexView make_index()
{
    IndexView ix;
    memset(&ix, 0, sizeof ix);
    ix.end_pos = kEnds; ix.n_ends = 4; ix.G2 = kEnds[3] + 1; ix.G = ix.G2 / 2;
    return ix;
}

static Hit mk(int64_t gPos, int rPos, int len) { Hit h; h.gPos = gPos; h.rPos = rPos; h.len = len; return h; }

static void fail(const char *what, int cap, const std::vector<Hit> &in, int rlen)
{
    g_bad++;
    if (g_bad > 12) return;
    fprintf(stderr, "CAP %d, rlen %d, n %zu: %s\n ", cap, rlen, in.size(), what);
    for (const Hit &h : in) fprintf(stderr, " (%lld,%d,%d)", (long long)h.gPos, h.rPos, h.len);
    fprintf(stderr, "\n");
}

template <int CAP>
static void check_list(const IndexView &ix, const Params &pm, const std::vector<Hit> &in, int rlen, int cand_cap)
{
    const int n = (int)in.size();
    g_cases++;
    // buffers exactly as long as the list and the capacity: a step past either is the sanitizer's to see
    Hit *a = (Hit *)aligned_alloc(16, sizeof(Hit) * (size_t)(n ? n : 1)), *b = (Hit *)aligned_alloc(16, sizeof(Hit) * (size_t)(n ? n : 1));
    Cand *ca = (Cand *)aligned_alloc(16, sizeof(Cand) * (size_t)cand_cap), *cb = (Cand *)aligned_alloc(16, sizeof(Cand) * (size_t)cand_cap);
    if (n) { memcpy(a, in.data(), sizeof(Hit) * (size_t)n); memcpy(b, in.data(), sizeof(Hit) * (size_t)n); }
    memset(ca, 0xAB, sizeof(Cand) * (size_t)cand_cap); memset(cb, 0xAB, sizeof(Cand) * (size_t)cand_cap);
    const int m_ref = prep_seeds(a, n);
    const int nc_ref = cluster_seeds(ix, pm, rlen, a, m_ref, ca, cand_cap);
    int m = -1;
    const int nc = cluster_read<CAP>(ix, pm, rlen, b, n, cb, cand_cap, m);
    if (m != m_ref) fail("kept hits differ", CAP, in, rlen);
    if (nc != nc_ref) fail("clusters differ", CAP, in, rlen);
    if (n && memcmp(a, b, sizeof(Hit) * (size_t)n)) fail("hit lists differ", CAP, in, rlen);
    if (memcmp(ca, cb, sizeof(Cand) * (size_t)cand_cap)) fail("candidates differ", CAP, in, rlen);
    if (n > CAP) g_fallback++;
    if (m_ref < n) g_dropped++;
    if (n && memcmp(a, in.data(), sizeof(Hit) * (size_t)n)) g_sorted++;
    if (nc_ref > cand_cap) g_over++;
    for (int k = 0; k < nc_ref && k < cand_cap; k++) if (ca[k].score >= rlen) g_tandem++;
    free(a); free(b); free(ca); free(cb);
}

// both reads of a pair: the stage as k_cluster ran it before (stage_cluster_pair, the header fetched back, kDispatched / kAwaitRescue stored on top) against
// stage_cluster_pair_regs<CAP>
template <int CAP>
static void check_pair(const IndexView &ix, const Params &pm, const std::vector<Hit> &h0, const std::vector<Hit> &h1, int rl0, int rl1, int est, bool early)
{
    Ctx cx;
    memset((void *)&cx, 0, sizeof cx);
    cx.ix = ix; cx.pm = pm;
    cx.caps.hit_cap = 88; cx.caps.hit_seed = 56; cx.caps.cand_cap = 24; cx.caps.cand_seed = 12; cx.caps.frag_cap = 96; cx.caps.ops_cap = 2048; cx.caps.job_cap = 32;
    cx.lay = make_layout(cx.caps);
    std::vector<uint8_t> sa((size_t)cx.lay.stride + 64, 0xCD), sb;
    uint8_t *pa = (uint8_t *)(((uintptr_t)sa.data() + 63) & ~(uintptr_t)63);
    cx.state = pa;
    PairState st = pair_state(cx.state, cx.lay, cx.caps, 0);
    const int nr = pm.paired ? 2 : 1;
    for (size_t i = 0; i < h0.size(); i++) st.hits[0][i] = h0[i];
    if (nr == 2) for (size_t i = 0; i < h1.size(); i++) st.hits[1][i] = h1[i];
    sb.assign(sa.size(), 0);
    uint8_t *pb = (uint8_t *)(((uintptr_t)sb.data() + 63) & ~(uintptr_t)63);
    memcpy(pb, pa, (size_t)cx.lay.stride);
    ReadRef rd[2];
    rd[0].ascii = nullptr; rd[0].rlen = rl0; rd[0].flipped = 0; rd[1].ascii = nullptr; rd[1].rlen = rl1; rd[1].flipped = 0;
    const int nh[2] = {(int)h0.size(), nr == 2 ? (int)h1.size() : 0};
    // as it was
    stage_cluster_pair(cx, 0, rd, est, nh);
    const uint32_t fl = st.hdr->flags;
    const bool need = pm.paired && !(fl & kOvAny) && st.hdr->n_paired == 0, over = early && (fl & kOvAny);
    if (over) st.hdr->flags = fl | kDispatched; else if (need) st.hdr->flags = fl | kAwaitRescue;
    // as it is
    cx.state = pb;
    uint32_t fl2 = 0xFFFFFFFFu, need2 = 7, over2 = 7;
    stage_cluster_pair_regs<CAP>(cx, 0, rd, est, nh, early, fl2, need2, over2);
    g_cases++;
    if (fl2 != fl || need2 != (need ? 1u : 0u) || over2 != (over ? 1u : 0u)) { g_bad++; if (g_bad < 12) fprintf(stderr, "CAP %d: pair outcome differs (flags %x / %x, need %d / %u, over %d / %u)\n", CAP, fl, fl2, (int)need, need2, (int)over, over2); }
    if (memcmp(pa, pb, (size_t)cx.lay.stride)) {
        g_bad++;
        if (g_bad < 12) { size_t at = 0; while (pa[at] == pb[at]) at++; fprintf(stderr, "CAP %d: pair records differ at byte %zu (n %zu, %zu)\n", CAP, at, h0.size(), h1.size()); }
    }
}

// a list of n hits around a few loci: PosDiff from a small set per locus (equal keys, tandem runs), len a function of the key (equal keys are equal seeds)
static std::vector<Hit> random_list(Rng &r, int n, int rlen, int shape)
{
    std::vector<Hit> v;
    const int loci = 1 + r.below(4);
    int64_t base[4];
    for (int k = 0; k < loci; k++) {
        const int where = r.below(8);
        base[k] = where == 0 ? kEnds[0] - r.below(300) : where == 1 ? (int64_t)r.below(200) : where == 2 ? ((int64_t)1 << 34) - 1 - r.below(1200) : 1000 + (int64_t)(r.next() % 3000000);
    }
    for (int i = 0; i < n; i++) {
        const int k = r.below(loci);
        const int rPos = r.below(rlen);
        int64_t pd = base[k] + (r.below(3) == 0 ? r.below(80) - 40 : r.below(3) - 1) - (r.below(12) == 0 ? base[k] + r.below(50) : 0); // (now and then PosDiff <= 0)
        if (pd + rPos > ((int64_t)1 << 34) - 1) pd = ((int64_t)1 << 34) - 1 - rPos; // (a text the guard admits: gPos below 2^34)
        const int len = 16 + (int)(((uint64_t)pd * 2654435761u + (uint64_t)rPos * 40503u) % (uint64_t)(rlen < 40 ? 8 : rlen - 16 > 120 ? 120 : rlen - 16));
        v.push_back(mk(pd + rPos, rPos, len > 1023 ? 1023 : len));
    }
    auto key_less = [](const Hit &x, const Hit &y) { const int64_t a = hit_pd(x), b = hit_pd(y); return a < b || (a == b && x.rPos < y.rPos); };
    if (shape == 1 || shape == 2) { // sorted / reversed
        for (size_t i = 1; i < v.size(); i++) for (size_t j = i; j > 0 && key_less(v[j], v[j - 1]); j--) std::swap(v[j], v[j - 1]);
        if (shape == 2) for (size_t i = 0; i < v.size() / 2; i++) std::swap(v[i], v[v.size() - 1 - i]);
    } else if (shape == 3) { // suffix-array-like: seed by seed along the read, each seed's occurrences in an order of their own
        for (size_t i = 1; i < v.size(); i++) for (size_t j = i; j > 0 && v[j].rPos < v[j - 1].rPos; j--) std::swap(v[j], v[j - 1]);
    }
    return v;
}

template <int CAP>
static void run_cap(const IndexView &ix, const Params &pm)
{
    const int cand = 12;
    // the named lists
    const int sizes[] = {0, 1, CAP - 1, CAP, CAP + 1};
    for (int n : sizes) {
        std::vector<Hit> up, down, drop, mix, same, sa_like;
        for (int i = 0; i < n; i++) {
            up.push_back(mk(5000 + 3 * i + i, i, 20));
            down.push_back(mk(5000 + 3 * (n - i) + i, i, 20));
            drop.push_back(mk(i / 2, i + 7, 17));                                     // PosDiff <= 0, all of them
            mix.push_back(i % 3 == 1 ? mk(i, i + 1, 16) : mk(7000 - 2 * i + i, i, 18)); // kept ones out of order, dropped ones between
            same.push_back(mk(9000 + 5, 5, 30));                                      // equal keys
            sa_like.push_back(mk(1000 + 977 * ((i * 7) % (n ? n : 1)) + i / 4 * 20, i / 4 * 20, 19));
        }
        for (const auto *l : {&up, &down, &drop, &mix, &same, &sa_like}) { check_list<CAP>(ix, pm, *l, 150, cand); check_list<CAP>(ix, pm, *l, 40, cand); }
    }
    { // a tandem run: one locus, three PosDiffs, the scores of a run past the read length
        std::vector<Hit> t;
        for (int i = 0; i < CAP; i++) t.push_back(mk(50000 + (i % 3) * 4 + (CAP - 1 - i) * 2, (CAP - 1 - i) * 2, 30));
        check_list<CAP>(ix, pm, t, 60, cand);
        check_list<CAP>(ix, pm, t, 100, cand);
    }
    { // split by a contig end (kEnds[0]) and by max_pos_diff; each part scores above the threshold
        std::vector<Hit> s;
        s.push_back(mk(kEnds[0] - 10, 0, 60)); s.push_back(mk(kEnds[0] + 55, 65, 60));
        s.push_back(mk(1500000, 0, 60)); s.push_back(mk(1500000 + 70 + pm.max_pos_diff + 1, 70, 60));
        s.push_back(mk(1600000, 0, 60)); s.push_back(mk(1600000 + 70 + pm.max_pos_diff, 70, 60));
        s.resize(CAP < 6 ? CAP : 6);
        check_list<CAP>(ix, pm, s, 150, cand);
        std::swap(s[0], s[s.size() - 1]);
        check_list<CAP>(ix, pm, s, 150, cand);
    }
    if (CAP > cand) { // more clusters than cand_seed
        std::vector<Hit> many;
        for (int i = 0; i < CAP; i++) many.push_back(mk(100000 + 5000 * (int64_t)((i * 5) % CAP), 3, 100));
        check_list<CAP>(ix, pm, many, 150, cand);
    }
    { // the packing's bounds: gPos at 2^34 - 1, rPos and len at 1023
        std::vector<Hit> edge;
        edge.push_back(mk(((int64_t)1 << 34) - 1, 1023, 1023));
        edge.push_back(mk(((int64_t)1 << 34) - 1, 0, 1023));
        edge.push_back(mk(((int64_t)1 << 34) - 1 - 500, 523, 1023));
        edge.push_back(mk(1024, 1023, 1));
        edge.resize(CAP < 4 ? CAP : 4);
        check_list<CAP>(ix, pm, edge, 1023, cand);
        check_list<CAP>(ix, pm, edge, 4000, cand);
        const uint64_t w = hit_pack(((int64_t)1 << 34) - 1, 1023, 1022);
        const Hit back = hit_unpack(w);
        if (w >= kHitPad || back.gPos != ((int64_t)1 << 34) + 1022 || back.rPos != 1023 || back.len != 1022) { g_bad++; fprintf(stderr, "the packed word's round trip at its bounds\n"); }
    }
    // random lists, fixed seed
    Rng r; r.s = 0x9E3779B97F4A7C15ull + (uint64_t)CAP;
    for (int it = 0; it < 4000; it++) {
        const int n = it % 9 == 0 ? CAP + 1 + r.below(6) : r.below(CAP + 1);
        const int rlen = it % 5 == 0 ? 40 + r.below(30) : 150;
        check_list<CAP>(ix, pm, random_list(r, n, rlen, r.below(4)), rlen, cand);
    }
    // pairs of random lists through the whole stage (paired and single-end, with and without an early list; now and then a read past the seeding capacity)
    Params se = pm; se.paired = 0;
    for (int it = 0; it < 1500; it++) {
        const int n0 = it % 97 == 0 ? 57 + r.below(8) : it % 11 == 0 ? CAP + 1 + r.below(4) : r.below(CAP + 1), n1 = r.below(CAP + 1);
        const int rlen = it % 7 == 0 ? 50 : 150;
        const std::vector<Hit> h0 = random_list(r, n0, rlen, r.below(4)), h1 = random_list(r, n1, rlen, r.below(4));
        check_pair<CAP>(ix, it % 13 == 0 ? se : pm, h0, h1, rlen, rlen, 300 + r.below(500), it % 2 == 0);
    }
}

static void guard(int64_t text_len, int max_read_len, bool want)
{
    const bool got = packed_hits_fit(text_len, max_read_len);
    printf("text length %lld, max_read_len %d: register path %s\n", (long long)text_len, max_read_len, got ? "allowed" : "refused");
    if (got != want) { g_bad++; fprintf(stderr, "  packed_hits_fit = %d, want %d\n", (int)got, (int)want); }
}

int main()
{
    const IndexView ix = make_index();
    Params pm; pm.max_pos_diff = 30; pm.max_mm_rate = 0.05f; pm.use_nw = 0; pm.paired = 1;
    run_cap<4>(ix, pm); run_cap<8>(ix, pm); run_cap<16>(ix, pm); run_cap<32>(ix, pm);
    printf("%ld cases: %ld sorted or closed up, %ld with a dropped hit, %ld tandem candidates, %ld past cand_seed, %ld on the memory path by their length\n",
           g_cases, g_sorted, g_dropped, g_tandem, g_over, g_fallback);
    if (!g_sorted || !g_dropped || !g_tandem || !g_over || !g_fallback) { g_bad++; fprintf(stderr, "a kind of list was never seen\n"); }
    const int64_t lim = (int64_t)1 << 34;
    guard(6200000000ll, 256, true);   // a human genome, both strands
    guard(lim - 1, 1023, true);       // at the bounds
    guard(lim, 1023, false);
    guard(lim + 1, 150, false);
    guard(lim - 1, 1024, false);
    guard(1000, 1024, false);
    guard(0, 0, true);
    guard(-1, 150, false);
    if (g_bad) { fprintf(stderr, "cluster_regs_check: %d mismatches\n", g_bad); return 1; }
    printf("cluster_regs_check: all cases agree\n");
    return 0;
}
