// mapcaller_amd/csrc/mcx_pipeline.hip — the batch pipeline: its kernels (but the DP stage's), the context, the tiers and the batch ABI.
//
// One batch of reads goes through (all on one stream, no host round trip inside a tier):
//   k_pack_reads  ASCII -> 2-bit words + N masks, mate 2 reverse-complemented (ReadMapping.cpp:447,451)
//   k_seed        jump table + FM steps + direct comparison, one read per lane (IdentifySimplePairs/BWT_Search)
//   k_sa          hits that are still BWT rows -> text positions            (bwt_sa)
//   k_simple      the straight-line pairs of a whole batch from their seeds to their records (mcx_simple.h), k_simple_dp their small gaps;
//                 k_order_* deal what is left to the lanes by weight
//   k_cluster     one pair per lane: sort, cluster, pair by distance        (SimplePairClustering, CheckPairedAlignmentDistance);
//                 the large tier: k_cluster_wave, a pair per wavefront
//   k_rescue_plan / _eval / _apply   mate rescue window by window; k_rescue: pairs with an N in a read (AlignmentRescue)
//   k_build       mask, fragment lists, DP job emission by size class       (ProduceReadAlignment up to ProcessNormalPair);
//                 the large tier: k_build_wave
//   launch_dp()   the gapped extensions of the job lists: mcx_dp_stage.hip   (ksw2_alignment / nw_alignment)
//   k_finish      gates, scores, pair stats, flags, MAPQ, CIGAR, records    (ProduceReadAlignment tail, SamReport.cpp)
// Pairs that overflow the tier-0 pair-state capacities are re-run in tier 1 (hard bounds).
// The reference's per-chunk avgDist feedback is then replayed: per-chunk sums on the device, the
// trajectory on the host, and only the pairs whose decision depends on the exact estimate re-run.
// The -vcf bookkeeping of a batch (mcx_profile.hip) follows when a profile is attached.
//
// Also here: the error string of the library (mcx_last_error, mcx_set_error), the context (mcx_ctx_create / _free; its layout is
// mcx_ctx.h's), -m (mcx_ctx_set_multi, mcx_multi_*), mcx_bwt_search_batch and mcx_cigar_words.  The other units of the library
// reach this one through the ABI, pack_reads() and reserve_tier0().
#include "mcx_ctx.h"
#include "mcx_pack.h"
#include <hipcub/hipcub.hpp>

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
int mcx_set_error(int code, const std::string &msg) { return fail(code, msg); }
extern "C" const char *mcx_last_error(void) { return g_err.c_str(); }
extern "C" int mcx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// The chromosome tables (PosChrIdMap as sorted arrays) are binary-searched several times per
// pair; each probe is a dependent load.  Blocks copy them to LDS once (when they fit) and the
// per-pair code then searches LDS through the same pointers.
struct EndsLds { int64_t pos[kLdsEnds]; int32_t chr[kLdsEnds]; };

static __device__ __forceinline__ void stage_ends(IndexView &ix, EndsLds &l)
{
    if (ix.n_ends <= kLdsEnds) { // uniform over the grid
        for (int i = threadIdx.x; i < ix.n_ends; i += blockDim.x) { l.pos[i] = ix.end_pos[i]; l.chr[i] = ix.end_chr[i]; }
        __syncthreads();
        ix.end_pos = l.pos; ix.end_chr = l.chr;
    }
}

// (a read without N also carries its 2-bit words — k_pack_reads' form, in HBM: a base then costs a shift of a word that
//  sits in L1 instead of a byte fetch and a table look-up, and gap fragments are compared sixteen bases at a time)
static __device__ __forceinline__ void make_reads(const Ctx &cx, const ReadBatch &rb, uint32_t pair, ReadRef rd[2])
{
    const int nr = cx.pm.paired ? 2 : 1;
    for (int s = 0; s < nr; s++) {
        uint32_t r = pair * nr + s;
        rd[s].ascii = rb.bases + rb.off[r];
        rd[s].rlen = (int32_t)(rb.off[r + 1] - rb.off[r]);
        rd[s].flipped = (cx.pm.paired && s == 1) ? 1 : 0;
        rd[s].codes = (cx.packed && !(cx.read_ext[r] >> 31)) ? cx.packed + (uint64_t)r * cx.wpad : nullptr;
#ifdef MCX_DEBUG_NO_CODES
        rd[s].codes = nullptr;
#endif
    }
}

struct SeedOut {
    uint2 *tasks;            // (local read, hit index) per hit to resolve
    uint32_t *n_tasks;
    uint32_t task_cap;
    uint32_t *read_ext;      // per batch read: extension steps, blocks touched
    uint32_t *read_blocks;
    const uint32_t *packed;  // 2-bit reads of the batch (k_pack_reads), wpad words each
    int wpad;
    uint32_t *queue;         // next read of the pass that no wavefront has taken yet
    // the late pairs' pass: their seed hits are already there, complete, in the records of the tier that listed them (pair = record:
    // the main pass) — a read without N takes them from there instead of searching again (null: every read is searched)
    const uint8_t *src_state; Layout src_lay; Caps src_caps;
};

// The packed form of every read of a batch (mcx_fm.h pack_read: 16 bases per code word, one zero
// word, 32 N flags per mask word, one all-ones word; the arithmetic is mcx_pack.h's).  Mate 2 is packed
// reverse-complemented (ReadMapping.cpp:451).
// (any_n: set when a read of the batch holds a byte that is not one of ACGT — the passes of the large tier, which are queued after the
//  host has looked at the batch's counters anyway, leave out the kernel for such reads when there is none)
// (odd_flag, with the -vcf bookkeeping: bit 1 of the read's flag byte is set when the read holds a byte that is not an upper-case A C G T)
//
// part m of read r straight from HBM: 32 bases (m < mask words of the read); the thread of a read's last part writes the row's two constant words as well
// (kOdd: with the odd flags, for -vcf; off[r] and off[r+1] are read once)
template <bool kOdd>
static __device__ __forceinline__ void pack_read_part(const ReadBatch &rb, uint32_t r, int m, int paired, int wpad, uint32_t *out, uint32_t *any_n, uint8_t *odd_flag)
{
    const uint32_t a = rb.off[r], e = rb.off[r + 1];
    const int rlen = (int)(e - a), flipped = (paired && (r & 1)) ? 1 : 0, nmw = (rlen + 31) >> 5;
    if (packed_words(rlen) > wpad) return; // (a read longer than the context was sized for: the batch is refused before this runs, k_max_read_len)
    uint32_t *o = out + (uint64_t)r * wpad;
    if (m == (nmw > 0 ? nmw - 1 : 0)) pack_row_ends(rlen, o);
    if (m >= nmw) return;
    const uint8_t *p = rb.bases + a;
    const uint32_t sh = (uint32_t)((uintptr_t)p & 15);
    uint32_t has_n, odd;
    pack_unit32<kOdd>((const U4 *)(p - sh), (uint64_t)sh, rlen, flipped, m, o, has_n, odd);
    if (kOdd && odd) atomicOr((uint32_t *)(odd_flag + (r & ~3u)), 2u << (8 * (r & 3)));
    if (has_n) atomicOr(any_n, 1u);
}

// One thread per 32 bases of a read, parts = ceil(longest read / 32) threads per read, in workgroups of parts x (256 / parts) threads: threadIdx.x is the part and
// threadIdx.y the read, so that no thread divides, and neighbouring threads fetch neighbouring bytes of the batch.  A read of 16 bytes or more is fetched 16 bytes
// at a time from byte addresses of its own, its last bases included, so every span of a wavefront takes one path, and both spans of a part are asked for before either
// is packed (mcx_pack.h).  With the look-up pack4 that path is 273 vector instructions as compiled where the kernel had 673: 0.49 ms for 8 M reads of 150 bases where
// it took 0.72, against 0.30 for its 1.9 GB at the copy rate.  What is left is neither the arithmetic alone (some 0.25 ms of vector issue) nor loads in flight (the
// same part of two reads per thread, four loads in flight: no faster); tiles of reads staged in LDS were measured slower before.
// (kFlat: one row of threads numbered through 64 bits — more parts than a workgroup has threads, or more workgroups than a grid has in x)
template <bool kOdd, bool kFlat>
__global__ void __launch_bounds__(256) k_pack_reads(ReadBatch rb, int paired, int wpad, int parts, uint32_t *out, uint32_t *any_n, uint8_t *odd_flag)
{
    uint32_t r; int m;
    if (kFlat) {
        const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, q = t / (uint32_t)parts;
        if (q >= rb.n_reads) return;
        r = (uint32_t)q; m = (int)(t - q * (uint32_t)parts);
    } else {
        r = blockIdx.x * blockDim.y + threadIdx.y; m = (int)threadIdx.x;
        if (r >= rb.n_reads) return;
    }
    pack_read_part<kOdd>(rb, r, m, paired, wpad, out, any_n, odd_flag);
}

// (launched from two units: a batch's own step — mcx_batch_begin — and a batch on its way in — mcx_stream.hip)
// tpr: ceil(longest read / 32) + 1 (a thread per 32 bases: tpr - 1 of them per read); wpad: words from one row to the next
void pack_reads(const ReadBatch &rb, int paired, int wpad, int tpr, uint32_t *out, uint32_t *any_n, uint8_t *odd_flag, hipStream_t s)
{
    const int parts = std::max(tpr - 1, 1);
    const uint32_t rpb = parts <= 256 ? 256u / (uint32_t)parts : 0u; // reads per workgroup
    const uint64_t n_wg = rpb ? ((uint64_t)rb.n_reads + rpb - 1) / rpb : 0;
    if (rpb && n_wg <= 0x7FFFFFFFull && rb.n_reads <= 0xFFFFFFFFu - 256u) { // (r = blockIdx.x * rpb + threadIdx.y < n_reads + rpb then fits 32 bits)
        const dim3 wg((unsigned)parts, rpb);
        if (odd_flag) k_pack_reads<true, false><<<(unsigned)n_wg, wg, 0, s>>>(rb, paired, wpad, parts, out, any_n, odd_flag);
        else k_pack_reads<false, false><<<(unsigned)n_wg, wg, 0, s>>>(rb, paired, wpad, parts, out, any_n, odd_flag);
    } else {
        const unsigned n_flat = (unsigned)(((uint64_t)rb.n_reads * (uint64_t)parts + 255) / 256);
        if (odd_flag) k_pack_reads<true, true><<<n_flat, 256, 0, s>>>(rb, paired, wpad, parts, out, any_n, odd_flag);
        else k_pack_reads<false, true><<<n_flat, 256, 0, s>>>(rb, paired, wpad, parts, out, any_n, odd_flag);
    }
}

// Reads are handed to lanes as the lanes become free: a read is one to six searches (many more steps each inside a
// repeat), and a wave whose lanes each owned one read would run as long as its longest read while most lanes idle.
// The reads of a pass form one queue; a wavefront takes a chunk of it with one atomic whenever its lanes run dry, and a
// lane that has finished a read takes the chunk's next one — every search iteration of the wave finds (nearly) all
// lanes with work, and the launch ends when the queue does, not block by block.
constexpr int kSeedReadsPerLane = 4; // reads per lane and chunk (small selections: one, their launch is as long as its longest chain of reads)

// FM steps a lane takes before the wave looks at its other lanes again (MCX_SEED_FM_BUDGET for experiments)

static inline int seed_reads_per_lane(uint64_t n_reads) { return n_reads >= (uint64_t)1 << 21 ? kSeedReadsPerLane : (n_reads >= (uint64_t)1 << 19 ? 2 : 1); }

#ifndef MCX_SEED_WAVES
#define MCX_SEED_WAVES 1
#endif
#ifdef MCX_SEED_STATS
__device__ unsigned long long g_seed_hist[2][24]; // reads / index blocks by blocks per read (bucket = bit length of the count)
#endif
__global__ void __launch_bounds__(256, MCX_SEED_WAVES) k_seed(Ctx cx, ReadBatch rb, PairSel sel, SeedOut so, int pk_words, int reads_per_lane, int fm_budget)
{
    extern __shared__ uint32_t pk_lds[]; // packed reads: word k of lane t at pk_lds[k * blockDim.x + t]
    const int nr = cx.pm.paired ? 2 : 1;
    const uint32_t total = sel.n * nr;
    const int lane = threadIdx.x & 63;
    const uint64_t lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const uint32_t chunk = 64u * (uint32_t)reads_per_lane;
    PackedRead pk; pk.w = pk_lds + threadIdx.x; pk.stride = blockDim.x; pk.n_code = 0;
    bool have = false;
    uint32_t lr = 0, r = 0, nm = 0;
    int rlen = 0, p = 0, n = 0;
    int64_t ext = 0, blocks = 0;
    Hit *hits = nullptr;
    // the read is done: counters, and SA tasks for the hits that are still BWT rows (the others carry their text position)
    uint32_t has_n = 0;
    int cap = cx.caps.hit_seed;
    auto finish_read = [&]() {
        so.read_ext[r] = (uint32_t)ext | (has_n << 31); so.read_blocks[r] = (uint32_t)blocks | ((uint32_t)n << 20); // (ext < 2^31; blocks < 2^20; n < 2^12)
#ifdef MCX_SEED_STATS
        { const int bk = blocks ? 64 - __clzll((unsigned long long)blocks) : 0; atomicAdd(&g_seed_hist[0][bk], 1ull); atomicAdd(&g_seed_hist[1][bk], (unsigned long long)blocks); }
#endif
        if (cx.ix.sa_full) return; // every hit already carries its text position (seed_search)
        const int keep = n <= cx.caps.hit_seed ? n : 0; // overflowing reads are re-run in the next tier
        int todo = 0;
        for (int i = 0; i < keep; i++) if (!(hits[i].len & kHitResolved)) todo++;
        uint32_t at = todo ? atomicAdd(so.n_tasks, (uint32_t)todo) : 0u;
        for (int i = 0; i < keep; i++) {
            if (hits[i].len & kHitResolved) { hits[i].len &= ~kHitResolved; continue; }
            if (at < so.task_cap) so.tasks[at] = make_uint2(lr, (uint32_t)i);
            at++;
        }
    };
    SeedWalk walk; walk.phase = 0;
    uint32_t q_next = 0, q_end = 0; // the wave's chunk of the queue (the same in every lane)
    bool dry = false;               // the queue has nothing left
    for (;;) {
        // ---- lanes without a read take the next ones of the wave's chunk (the whole wave passes here every iteration) ----
        const uint64_t need = __ballot(!have);
        bool fresh = false;
        if (need && !dry) {
            const uint32_t rank = (uint32_t)__popcll(need & lt_mask), want = (uint32_t)__popcll(need);
            uint32_t given = 0;
            while (given < want) {
                if (q_next == q_end) {
                    uint32_t b = 0;
                    if (lane == 0) b = atomicAdd(so.queue, chunk);
                    b = __shfl(b, 0, 64);
                    if (b >= total) { dry = true; break; }
                    q_next = b; q_end = min(b + chunk, total);
                }
                const uint32_t take = min(want - given, q_end - q_next);
                if (!have && !fresh && rank >= given && rank < given + take) { lr = q_next + (rank - given); fresh = true; }
                q_next += take; given += take;
            }
        }
        if (fresh) {
            r = sel_pair(sel, lr / nr) * nr + lr % nr;
            rlen = (int)(rb.off[r + 1] - rb.off[r]);
            hits = pair_state(cx.state, cx.lay, cx.caps, lr / nr).hits[lr % nr];
            n = 0; p = 0; ext = 0; blocks = 0; has_n = 0; walk.phase = 0;
            const int words = packed_words(rlen);
            // (only when neither read of the pair holds an N: such a pair went through k_rescue in tier 0, whose rescue_mate appends seeds to the
            //  N-free read's hits — the same test as k_rescue_plan's)
            if (so.src_state && !((so.read_ext[r] | (nr == 2 ? so.read_ext[r ^ 1u] : 0u)) >> 31)) {
                // (the list as k_cluster left it: PosDiff > 0 only, sorted — clustering it again gives the same candidates; the entries the
                //  filter dropped are made up by entries it drops again, so that the read's hit count, a statistic, stays what the search found)
                const PairState src = pair_state((uint8_t *)so.src_state, so.src_lay, so.src_caps, r / nr);
                const int m = src.hdr->n_hits[r % nr], n0 = (int)(so.read_blocks[r] >> 20);
                for (int i = 0; i < m; i++) hits[i] = src.hits[r % nr][i];
                Hit none; none.gPos = 0; none.rPos = 0; none.len = 0;
                for (int i = m; i < n0; i++) hits[i] = none;
                fresh = false; // (counters untouched: they are the search's)
            } else
            if (rlen > 0 && words <= pk_words) {
                const U4 *src = (const U4 *)(so.packed + (uint64_t)r * so.wpad);
                for (int k = 0; k < words; k += 4) {
                    const U4 v = src[k >> 2];
                    pk.w[k * pk.stride] = v.x;
                    if (k + 1 < words) pk.w[(k + 1) * pk.stride] = v.y;
                    if (k + 2 < words) pk.w[(k + 2) * pk.stride] = v.z;
                    if (k + 3 < words) pk.w[(k + 3) * pk.stride] = v.w;
                }
                pk.n_code = ((rlen + 15) >> 4) + 1;
                { // does the read hold an N?  (mask words: bit 31-s of word s/32; bases past the end are flagged too)
                    const int nmw = (rlen + 31) >> 5;
                    uint32_t any = 0;
                    for (int m = 0; m < nmw; m++) {
                        uint32_t w = pk.w[(pk.n_code + m) * pk.stride];
                        if (m == nmw - 1 && (rlen & 31)) w &= ~(0xFFFFFFFFu >> (rlen & 31));
                        any |= w;
                    }
                    has_n = any ? 1u : 0u;
                }
                have = seed_next_start(pk, rlen, p, nm);
            }
            if (!have && fresh) finish_read(); // (nothing to search in it: the lane takes another one next time round)
        }
        if (!__ballot(have)) { if (dry) break; continue; }
        // ---- every lane that holds a read moves its search on: each phase with a budget, so that a lane deep inside a repeat
        //      (dozens of FM steps) holds the wave up for a few steps at a time while the others finish searches and take new reads ----
        if (have && walk.phase == 0) seed_begin(cx.ix, pk, rlen, nm, p, walk);
        if (have && walk.phase == 1) seed_fm(cx.ix, pk, rlen, p, walk, blocks, fm_budget);
        if (have && walk.phase == 2) seed_compare_wide(cx.ix, pk, rlen, p, walk, 1 << 30);
        if (have && walk.phase == 3) {
            seed_take(cx.ix, p, walk, hits, cap, n, ext);
            if (!seed_next_start(pk, rlen, p, nm)) { finish_read(); have = false; }
        }
    }
}

__global__ void __launch_bounds__(256) k_sa(Ctx cx, SeedOut so, int paired, uint32_t *lf_total)
{
    const uint32_t n = min(*so.n_tasks, so.task_cap);
    const int nr = paired ? 2 : 1;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
        const uint2 task = so.tasks[t];
        PairState st = pair_state(cx.state, cx.lay, cx.caps, task.x / nr);
        Hit &h = st.hits[task.x % nr][task.y];
        int lf = 0;
        h.gPos = (int64_t)fm_sa(cx.ix, (uint64_t)h.gPos, lf);
        if (lf_total && lf) atomicAdd(lf_total, (uint32_t)lf);
    }
}

struct RescueList { uint32_t *ids; uint32_t *n; uint32_t cap; };
// pairs that ran over the tier-0 capacities while clustering are listed right there, with their estimate: the large tier maps
// them on a stream of its own while the rest of the pass is still under way (ids null: no such list)
struct EarlyList { uint32_t *ids; int32_t *est; uint32_t *n; uint32_t cap; uint32_t *n_hits; };

// The per-pair kernels give every lane one pair, and a wavefront is as slow as its heaviest lane: next to a pair from a repeat
// (dozens of hits to sort and cluster, a dozen candidates to build and score) sixty-three ordinary pairs wait.  So the pairs
// of a pass are dealt to the lanes by weight — total seed hits, known once k_seed is done — heaviest class first: like sits
// with like, and the long wavefronts start early.  Two small passes (count, place) make the permutation `order`.
// Classes 0 .. kHeavyClasses - 1 are the heavy pairs: more than kLightHits hits (mcx_types.h — the bound light_pairs_fit() holds against the
// tier's capacities), so more than kSimpleHits in one read at least: k_simple never takes such a pair, and its class, its place in the order and its
// clustering depend on k_seed alone.  run_pairs lists and clusters them on a side stream beside the straight-line path (passes H and L below).
constexpr int kWorkClasses = 6, kHeavyClasses = 4;
constexpr uint32_t kAsideGatePairs = 1u << 16; // passes of at least this many pairs tell the next pass whether the aside path pays (mcx_ctx::aside_pays)
static __device__ __forceinline__ int work_class(uint32_t hits) { return hits > 64 ? 0 : hits > 32 ? 1 : hits > 16 ? 2 : hits > (uint32_t)kLightHits ? 3 : hits > 4 ? 4 : 5; }
static_assert(kLightHits >= 2 * kSimpleHits, "a heavy pair must hold a read with more than kSimpleHits hits: k_simple leaves its hits alone while k_cluster sorts them");

static __device__ __forceinline__ int pair_work_class(const PairSel &sel, uint32_t local, const uint32_t *read_blocks, int nr, const uint8_t *done = nullptr)
{
    if (done && done[local]) return -1; // k_simple took the pair from its seeds to its records: no lane of the per-pair kernels for it
    const uint32_t pair = sel_pair(sel, local);
    return work_class((read_blocks[pair * nr] >> 20) + (nr == 2 ? read_blocks[pair * nr + 1] >> 20 : 0u));
}

constexpr int kOrderTile = 16; // pairs per thread of the two passes: a block of 256 settles 4096 pairs with one global atomic per class

// (cls_lo .. cls_hi: the classes this pass lists; a pair of another class is left out like one that k_simple took.  The order is made in one pass over
//  all classes, or in two into the one array and the one set of counts: pass H, the heavy classes, without `done` — behind k_seed, beside k_simple —
//  and pass L, the light ones, behind both: its stretches begin where H's final counts end.)
__global__ void __launch_bounds__(256) k_order_count(PairSel sel, const uint32_t *read_blocks, int nr, uint32_t *counts, const uint8_t *done, int cls_lo, int cls_hi)
{
    __shared__ uint32_t n_cls[kWorkClasses];
    if (threadIdx.x < kWorkClasses) n_cls[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * (256u * kOrderTile);
    for (int t = 0; t < kOrderTile; t++) {
        const uint32_t local = base + t * 256u + threadIdx.x;
        int cls = local < sel.n ? pair_work_class(sel, local, read_blocks, nr, done) : -1;
        if (cls < cls_lo || cls > cls_hi) cls = -1;
#pragma unroll
        for (int k = 0; k < kWorkClasses; k++) {
            const uint64_t m = __ballot(cls == k);
            if ((threadIdx.x & 63) == 0 && m) atomicAdd(&n_cls[k], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    if (threadIdx.x < kWorkClasses && n_cls[threadIdx.x]) atomicAdd(counts + threadIdx.x * kCntPad, n_cls[threadIdx.x]);
}

// counts[k * kCntPad]: pairs of class k; counts[(8 + k) * kCntPad]: how many of them were placed so far
__global__ void __launch_bounds__(256) k_order_place(PairSel sel, const uint32_t *read_blocks, int nr, uint32_t *counts, uint32_t *order, const uint8_t *done, int cls_lo, int cls_hi)
{
    __shared__ uint32_t n_cls[kWorkClasses], at_cls[kWorkClasses];
    if (threadIdx.x < kWorkClasses) n_cls[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * (256u * kOrderTile);
    const int lane = threadIdx.x & 63;
    int cls[kOrderTile];
#pragma unroll
    for (int t = 0; t < kOrderTile; t++) {
        const uint32_t local = base + t * 256u + threadIdx.x;
        cls[t] = local < sel.n ? pair_work_class(sel, local, read_blocks, nr, done) : -1;
        if (cls[t] < cls_lo || cls[t] > cls_hi) cls[t] = -1;
#pragma unroll
        for (int k = 0; k < kWorkClasses; k++) {
            const uint64_t m = __ballot(cls[t] == k);
            if (lane == 0 && m) atomicAdd(&n_cls[k], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    if (threadIdx.x < kWorkClasses) { // the block's stretch of every class: where the class begins + what other blocks took before
        uint32_t first = 0;
        for (int k = 0; k < (int)threadIdx.x; k++) first += counts[k * kCntPad];
        const uint32_t mine = n_cls[threadIdx.x];
        at_cls[threadIdx.x] = first + (mine ? atomicAdd(counts + (8 + threadIdx.x) * kCntPad, mine) : 0u);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kOrderTile; t++) {
        const uint32_t local = base + t * 256u + threadIdx.x;
#pragma unroll
        for (int k = 0; k < kWorkClasses; k++) {
            const uint64_t m = __ballot(cls[t] == k);
            uint32_t b = 0;
            if (lane == 0 && m) b = atomicAdd(&at_cls[k], (uint32_t)__popcll(m));
            b = __shfl(b, 0, 64);
            if (cls[t] == k) order[b + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = local;
        }
    }
}

// The straight-line pairs of a pass, from their seeds to their records (mcx_simple.h): one pair per lane, in pair order (their
// work is even: no dealing by weight, and neighbouring lanes write neighbouring records).  What a lane needs — at most four
// seeds per read, the 2-bit words of its reads, a few words of the genome under the gaps — stays in registers; the CIGAR
// operations wait word-major in LDS until the wave has reserved its words of the pool with one atomic.  done[pair] tells the
// per-pair kernels behind this one which pairs are left to them (k_order_*).
// A pair whose only obstacle is a small gapped extension or two (mcx_simple.h SimpleJob) writes the problems down and waits
// (done = 2): k_simple_dp solves them one per lane, k_simple_rest makes the pass again with the results at hand.
struct SimpleLater {        // the pairs that wait, and their problems
    uint32_t *pairs;        // [cap]
    SimpleJob *jobs;        // [cap * kSimpleJobs]: waiting pair i's at i * kSimpleJobs
    SimpleRes *res;         // the same places
    uint32_t *job_list;     // [cap * kSimpleJobs]: the places that hold a problem
    uint32_t *n_pairs, *n_jobs;
    uint32_t cap;
};

// DETAIL (the -vcf bookkeeping is on): the pair's two detail records — what write_detail leaves for a read with one surviving candidate, and
// pair_stats' discordant-pair fields in read 1's — come from here too (mcx_simple.h SimpleDetail), so that the profile does not switch the path off.
template <bool NW, int MODE, bool DETAIL>
__global__ void __launch_bounds__(256) k_simple(Ctx cx, ReadBatch rb, uint32_t n_pairs, const int32_t *est, const uint32_t *read_blocks, AlnRec *recs, PairOut *pout,
                                                uint8_t *done, uint32_t *pool_over, uint32_t *n_done, SimpleLater sl)
{
    __shared__ EndsLds ends;
    __shared__ uint16_t cig_stage[256 * 2 * kSimpleRuns]; // operation k of thread t at [k * 256 + t] (16 bits: a run is at most 4095 long)
    __shared__ uint32_t job_stage[MODE == kDpCollect ? 3 * kSimpleJobs * 256 : 1]; // word w of thread t's problem k at [(3 * k + w) * 256 + t]
    stage_ends(cx.ix, ends);
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; // collect: the pair; replay: the waiting pair
    const int nr = cx.pm.paired ? 2 : 1;
    uint16_t *stage = cig_stage + threadIdx.x;
    const uint32_t n_slots = MODE == kDpReplay ? min(*sl.n_pairs, sl.cap) : n_pairs;
    bool ok = slot < n_slots;
    const uint32_t pair = MODE == kDpReplay ? (ok ? sl.pairs[slot] : 0u) : slot;
    SimpleRead sr[2];
    int rl[2] = {0, 0};
    typename std::conditional<DETAIL, SimpleDetail, SimpleNoDetail>::type det;
    SimpleDpIo io;
    io.mode = MODE == kDpCollect && !sl.pairs ? kDpNone : MODE;
    io.jobs = MODE == kDpCollect ? job_stage + threadIdx.x : nullptr; io.job_stride = 256;
    io.res = MODE == kDpReplay ? sl.res + (uint64_t)slot * kSimpleJobs : nullptr;
    io.n = 0; io.read = 0;
    bool later = false;
    if (ok) {
        const PairState st = pair_state(cx.state, cx.lay, cx.caps, pair);
        // both reads' counts before the first fetch of a hit: a pair with a read of more than kSimpleHits hits is not this kernel's, and its hits are
        // not looked at — the clustering kernel may be sorting a heavy pair's in place at this moment (run_pairs: the heavy pairs aside)
        int nhs[2] = {0, 0};
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (s < nr) {
                const uint32_t r = pair * nr + s;
                nhs[s] = (int)(read_blocks[r] >> 20);
                ok = ok && nhs[s] >= 1 && nhs[s] <= kSimpleHits && !(cx.read_ext[r] >> 31);
            }
        }
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (s < nr && ok) {
                const uint32_t r = pair * nr + s;
                rl[s] = (int)(rb.off[r + 1] - rb.off[r]);
                io.read = r;
                if constexpr (DETAIL) { uint8_t *rec = cx.detail + (uint64_t)r * cx.dlay.stride; det.frags = (Frag *)(rec + sizeof(DetailHdr)); det.ops = rec + cx.dlay.off_ops; }
                const int how = simple_read<NW, uint16_t>(cx.ix, cx.pm, rl[s], cx.packed + (uint64_t)r * cx.wpad, st.hits[s], nhs[s], sr[s], stage + s * kSimpleRuns * 256, 256, io, det);
                ok = how != kSimpleNo;
                later = later || how == kSimpleLater;
            }
        }
        if (ok && nr == 2) ok = simple_pair_ok(sr[0], sr[1], est[pair]);
    }
    if (MODE == kDpCollect) { // the pairs that wait: a place among them, their problems into it
        const bool wait = ok && later;
        const uint32_t at = wave_reserve(sl.n_pairs, wait ? 1u : 0u);
        const bool kept = wait && at < sl.cap;
        const uint32_t jat = wave_reserve(sl.n_jobs, kept ? (uint32_t)io.n : 0u);
        if (kept) {
            sl.pairs[at] = pair;
            for (int k = 0; k < io.n; k++) {
                const uint32_t *w = job_stage + (3 * k) * 256 + threadIdx.x;
                sl.jobs[(uint64_t)at * kSimpleJobs + k] = simple_job_unpack(w[0], w[256], w[512], pair * (uint32_t)nr, nr);
                sl.job_list[jat + k] = at * kSimpleJobs + (uint32_t)k;
            }
            done[pair] = 2;
        }
        if (wait) ok = false; // (not kept: the general path)
        later = kept;
    }
    const uint32_t want = ok ? (uint32_t)sr[0].n_cig + (nr == 2 ? (uint32_t)sr[1].n_cig : 0u) : 0u;
    const uint32_t at = wave_reserve(cx.cig_pool_n, want);
    const uint64_t took = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && took) atomicAdd(n_done, (uint32_t)__popcll(took));
    if (slot >= n_slots) return;
    if (ok && at + want > cx.cig_pool_cap) { atomicOr(pool_over, 1u); ok = false; } // (the batch fails; the general path reports it)
    if (!later) done[pair] = ok ? 1 : 0;
    if (!ok) return;
    const uint32_t off[2] = {at, at + (uint32_t)sr[0].n_cig};
#pragma unroll
    for (int s = 0; s < 2; s++) {
        if (s >= nr) break;
        for (int k = 0; k < sr[s].n_cig; k++) cx.cig_pool[off[s] + k] = (uint32_t)stage[(s * kSimpleRuns + k) * 256];
    }
    AlnRec rec2[2];
    PairOut po;
    simple_pair(cx, nr == 2, sr[0], sr[nr - 1], rl[0], rl[nr - 1], est[pair], rec2, off, po);
    recs[(uint64_t)pair * nr] = rec2[0];
    if (nr == 2) recs[(uint64_t)pair * nr + 1] = rec2[1];
    pout[pair] = po;
    if constexpr (DETAIL) {
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (s >= nr) break;
            const DetailHdr d = simple_detail_hdr(cx.ix, nr == 2, s, sr[0], sr[nr - 1]);
            *(DetailHdr *)(cx.detail + ((uint64_t)pair * nr + s) * cx.dlay.stride) = d;
        }
    }
}

// the problems the straight-line pairs wrote down, one per lane (mcx_simple.h simple_dp_job): a strip of 16 columns, the lane's
// traceback words word-major in LDS
template <bool NW>
__global__ void __launch_bounds__(256) k_simple_dp(Ctx cx, SimpleLater sl)
{
    constexpr int W = 2 + kSimpleDp * LaneDir<16, NW>::words;
    __shared__ uint32_t words[W * 256];
    const uint32_t n = min(*sl.n_jobs, sl.cap * kSimpleJobs);
    LaneMem mem; mem.base = words; mem.stride = 256; mem.lane = threadIdx.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { // (the list's length stays on the device)
        const uint32_t at = sl.job_list[i];
        const SimpleJob j = sl.jobs[at];
        sl.res[at] = simple_dp_job<NW>(cx.ix, j, cx.packed + (uint64_t)j.read * cx.wpad, mem);
    }
}

// pairs the per-pair kernels work on: all of the selection, or — with k_simple ahead of them — those the order lists (its class counts)
static __device__ __forceinline__ uint32_t listed_pairs(const PairSel &sel, const uint32_t *order_cnt)
{
    if (!order_cnt) return sel.n;
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < kWorkClasses; k++) n += order_cnt[k * kCntPad];
    return n;
}

// (cls_lo .. cls_hi: with the pairs listed by weight, the launch takes the pairs of these classes only: all classes in one launch, heaviest
//  first inside it, or — run_pairs, the heavy pairs aside — the heavy classes on a side stream beside k_simple and the light ones behind it)
// (regs: tier 0, with the packed form's guard passed (mcx_ctx::regs_fit) and without MCX_CLUSTER_MEM — a read's seeds are sorted and clustered in registers
//  (mcx_glue.h cluster_read<CAP>) and the header is stored once.  CAP is the workgroup's: a weight class bounds a read's hits — 4, 8, 16, 32 for classes
//  5, 4, 3, 2 — and the workgroup's first slot holds its heaviest pair, so the class counts say which one will do for every lane; classes 0 and 1 keep
//  the memory path, a pass without the order takes 4 (a read with more hits takes the memory path by itself).)
__global__ void __launch_bounds__(256) k_cluster(Ctx cx, ReadBatch rb, PairSel sel, RescueList rl, const uint32_t *read_blocks, EarlyList el, const uint32_t *order,
                                                 const uint32_t *order_cnt, int cls_lo, int cls_hi, int regs)
{
    __shared__ EndsLds ends;
    uint32_t first = 0, n_listed = listed_pairs(sel, order_cnt);
    int cap = regs ? 4 : 0;
    if (order_cnt && order) {
        uint32_t at = 0;
        for (int k = 0; k < kWorkClasses; k++) { if (k == cls_lo) first = at; at += order_cnt[k * kCntPad]; if (k == cls_hi) n_listed = at; }
        int cls = 0; // of the block's first slot: the classes that end at or before it
        at = 0;
        for (int k = 0; k < kWorkClasses - 1; k++) { at += order_cnt[k * kCntPad]; if (first + blockIdx.x * blockDim.x >= at) cls = k + 1; }
        if (regs) cap = cls >= 2 ? 4 << (kWorkClasses - 1 - cls) : 0; // classes 5, 4, 3, 2: 4, 8, 16, 32
    }
    if (first + blockIdx.x * blockDim.x >= n_listed) return; // (uniform over the block)
    stage_ends(cx.ix, ends);
    const uint32_t slot = first + blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = slot < n_listed;
    const uint32_t local = in ? (order ? order[slot] : slot) : 0u;
    uint32_t need = 0, over = 0;
    if (in) {
        ReadRef rd[2];
        make_reads(cx, rb, sel_pair(sel, local), rd);
        PairState st = pair_state(cx.state, cx.lay, cx.caps, local);
        const uint32_t pair = sel_pair(sel, local);
        const int nr = cx.pm.paired ? 2 : 1;
        int nh[2] = {(int)(read_blocks[pair * nr] >> 20), nr == 2 ? (int)(read_blocks[pair * nr + 1] >> 20) : 0}; // k_seed's hit counts
        if (cap) { // (uniform over the block)
            uint32_t fl = 0;
            const int e = sel.est[local];
            const bool early = el.ids != nullptr;
            switch (cap) {
            case 4: stage_cluster_pair_regs<4>(cx, local, rd, e, nh, early, fl, need, over); break;
            case 8: stage_cluster_pair_regs<8>(cx, local, rd, e, nh, early, fl, need, over); break;
            case 16: stage_cluster_pair_regs<16>(cx, local, rd, e, nh, early, fl, need, over); break;
            default: stage_cluster_pair_regs<32>(cx, local, rd, e, nh, early, fl, need, over); break;
            }
            if (over && (fl & kOvHits)) atomicAdd(el.n_hits, 1u);
        } else {
            stage_cluster_pair(cx, local, rd, sel.est[local], nh);
            const uint32_t fl = st.hdr->flags;
            need = (cx.pm.paired && !(fl & kOvAny) && st.hdr->n_paired == 0) ? 1u : 0u;
            over = (el.ids && (fl & kOvAny)) ? 1u : 0u;
            if (over && (fl & kOvHits)) atomicAdd(el.n_hits, 1u); // (diagnosis: how many of the listed pairs were known to run over once k_seed was done)
            if (over) st.hdr->flags = fl | kDispatched; // the later stages of this tier leave the pair alone (they skip kOvAny) and k_finish writes nothing for it
            else if (need) st.hdr->flags = fl | kAwaitRescue;
        }
    }
    const uint32_t at = wave_reserve(rl.n, need);
    if (need && at < rl.cap) rl.ids[at] = local;
    if (el.ids) {
        const uint32_t ea = wave_reserve(el.n, over);
        if (over && ea < el.cap) { el.ids[ea] = sel_pair(sel, local); el.est[ea] = sel.est[local]; }
    }
}

// behind k_cluster on its stream: the list's length — and whether the batch holds a read with an N — into page-locked host memory, so that the host,
// which drives the large tier for the listed pairs, needs no copy of its own behind the kernel (such a copy is a blit kernel that waits for a free CU on a chip
// the pass is filling: 0.3 to 0.9 ms before the large tier's first kernel could start).  (Counting the clustering kernel's workgroups as they end, so
// that the last one could write the words, cost the kernel 0.5 ms: 15 000 atomics on one address.)
__global__ void k_publish_early(const uint32_t *n, const uint32_t *any_n, volatile uint32_t *host)
{
    if (threadIdx.x == 0) { host[0] = *n; host[1] = *any_n; __threadfence_system(); }
}

// ---- clustering and pairing of a heavy pair by a whole wavefront -----------------------------------------------------------
// The large tier's pairs come from repeats: hundreds of seed hits per read, hundreds of candidates.  One lane that sorts 800
// hits and pairs 300 x 300 candidates in its pair record (every step a dependent fetch from HBM) takes milliseconds, and the
// launch is as long as its slowest lane.  Here a wavefront takes a pair: a read's hits are brought into LDS, sorted there by all
// 64 lanes (bitonic, keys (PosDiff, rPos)), clustered by one lane out of LDS (the scan is serial by nature — its threshold
// moves with every cluster — but a step is an LDS access now, not a trip to HBM), and the candidates of the two reads are paired
// with the candidates of read 1 spread over the lanes.  Same functions, same results as stage_cluster_pair.
struct ClusterLds { // per-wave arrays in dynamic LDS (cap = the tier's candidate capacity per read)
    Hit *hits;          // [hit_cap]: the read being clustered
    int64_t *pd[2];     // [cand_cap] per read: PosDiff of the candidate's first seed
    int32_t *score[2];  // score (0: dropped)
    uint32_t *span[2];  // first seed | seeds << 16
    int32_t *mate[2];   // PairedAlnCanIdx
    int32_t *pick;      // [cand_cap]: the partner a candidate of read 1 chose (pairing scratch)
};

static inline MCX_HD int cluster_sort_room(int hit_cap) { int p = 1; while (p < hit_cap) p <<= 1; return p; } // (the sort works on a power of two)
static inline size_t cluster_lds_bytes(int hit_cap, int cand_cap) { return (size_t)cluster_sort_room(hit_cap) * sizeof(Hit) + (size_t)cand_cap * (2 * (8 + 4 + 4 + 4) + 4) + 64; }
constexpr int kClusterSmall = 192; // hits per read up to which a pair takes the launch with the small share of LDS (more wavefronts per CU)

// (hits_lo < hits <= hits_hi: the pairs of this launch, by the larger hit count of their reads; lds_hits / lds_cands: what its LDS holds)
__global__ void __launch_bounds__(64) k_cluster_wave(Ctx cx, ReadBatch rb, PairSel sel, RescueList rl, const uint32_t *read_blocks, int hits_lo, int hits_hi, int lds_hits,
                                                     int lds_cands)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t cl_lds[];
    __shared__ EndsLds ends;
    stage_ends(cx.ix, ends);
    const int lane = threadIdx.x;
    const int nr = cx.pm.paired ? 2 : 1;
    ClusterLds L;
    {
        uint8_t *p = cl_lds;
        L.hits = (Hit *)p; p += (size_t)cluster_sort_room(lds_hits) * sizeof(Hit);
        for (int s = 0; s < 2; s++) { L.pd[s] = (int64_t *)p; p += (size_t)lds_cands * 8; }
        for (int s = 0; s < 2; s++) { L.score[s] = (int32_t *)p; p += (size_t)lds_cands * 4; }
        for (int s = 0; s < 2; s++) { L.span[s] = (uint32_t *)p; p += (size_t)lds_cands * 4; }
        for (int s = 0; s < 2; s++) { L.mate[s] = (int32_t *)p; p += (size_t)lds_cands * 4; }
        L.pick = (int32_t *)p;
    }
    auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_s_barrier(); };
    for (uint32_t local = blockIdx.x; local < sel.n; local += gridDim.x) {
        const uint32_t pair = sel_pair(sel, local);
        {
            const int h0 = (int)(read_blocks[pair * nr] >> 20), h1 = nr == 2 ? (int)(read_blocks[pair * nr + 1] >> 20) : 0, hm = h0 > h1 ? h0 : h1;
            if (hm <= hits_lo || hm > hits_hi) continue; // another launch's pair
        }
        PairState st = pair_state(cx.state, cx.lay, cx.caps, local);
        uint32_t flags = 0;
        int n_hits[2] = {0, 0}, n_cands[2] = {0, 0};
        for (int s = 0; s < nr; s++) {
            const uint32_t r = pair * nr + s;
            const int rlen = (int)(rb.off[r + 1] - rb.off[r]);
            int nh = (int)(read_blocks[r] >> 20);
            if (nh > cx.caps.hit_seed) { flags |= kOvHits; nh = 0; }
            Hit *g_hits = st.hits[s];
            // the read's hits with PosDiff > 0 into LDS, closed up (IdentifySimplePairs' tail, ReadMapping.cpp:141-152)
            wave_sync();
            int m = 0;
            for (int base = 0; base < nh; base += 64) {
                const int i = base + lane;
                Hit x; x.gPos = 0; x.rPos = 0; x.len = 0;
                bool keep = false;
                if (i < nh) { x = g_hits[i]; keep = hit_pd(x) > 0; }
                const uint64_t mask = __ballot(keep);
                if (keep) L.hits[m + __popcll(mask & ((1ull << lane) - 1ull))] = x;
                m += __popcll(mask);
            }
            int P = 1;
            while (P < m) P <<= 1;
            for (int i = m + lane; i < P; i += 64) { Hit x; x.gPos = (int64_t)1 << 62; x.rPos = 0; x.len = 0; L.hits[i] = x; } // (sort to the end)
            wave_sync();
            for (int k = 2; k <= P; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = lane; i < P; i += 64) {
                        const int o = i ^ j;
                        if (o > i) {
                            const Hit a = L.hits[i], b = L.hits[o];
                            const int64_t pa = hit_pd(a), pb = hit_pd(b);
                            const bool a_gt = pa > pb || (pa == pb && a.rPos > b.rPos);
                            if (((i & k) == 0) == a_gt) { L.hits[i] = b; L.hits[o] = a; }
                        }
                    }
                    wave_sync();
                }
            for (int i = lane; i < m; i += 64) g_hits[i] = L.hits[i]; // the later stages read the seeds in this order
            // clusters: a serial scan (its threshold moves with every cluster it keeps), out of LDS
            int nc = 0;
            if (lane == 0)
                nc = cluster_seeds_to(cx.ix, cx.pm, rlen, L.hits, m, [&](int k, int score, int first, int count, int64_t pd0) {
                    if (k < cx.caps.cand_seed) { L.pd[s][k] = pd0; L.score[s][k] = score; L.span[s][k] = (uint32_t)first | ((uint32_t)count << 16); }
                });
            nc = __shfl(nc, 0, 64);
            if (nc > cx.caps.cand_seed) { flags |= kOvCands; nc = 0; }
            n_hits[s] = m; n_cands[s] = nc;
            wave_sync();
        }
        for (int s = 0; s < 2; s++) for (int i = lane; i < n_cands[s]; i += 64) L.mate[s][i] = -1;
        wave_sync();
        // CheckPairedAlignmentDistance (pair_by_distance): read 1's candidates over the lanes
        int n_paired = 0, lo = 0, hi = 0x7fffffff;
        if (cx.pm.paired && !(flags & kOvAny)) {
            const int n1 = n_cands[0], n2 = n_cands[1];
            const int64_t est = (int64_t)sel.est[local];
            if (n1 * n2 > 100) // RemoveRedundantAlnCan on both
                for (int s = 0; s < 2; s++) {
                    int best = 0;
                    for (int i = lane; i < n_cands[s]; i += 64) best = max(best, L.score[s][i]);
                    for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
                    if (n_cands[s] > 1) for (int i = lane; i < n_cands[s]; i += 64) if (L.score[s][i] < best) L.score[s][i] = 0;
                }
            wave_sync();
            int64_t max_lt = -1, min_ge = 0x7fffffff, top = 0;
            for (int i = lane; i < n1; i += 64) {
                const int sa = L.score[0][i];
                const int64_t pa = L.pd[0][i];
                int pick = -1, ps = 0;
                if (sa != 0)
                    for (int j = 0; j < n2; j++) {
                        const int sj = L.score[1][j];
                        const int64_t pj = L.pd[1][j];
                        if (sj == 0 || pj < pa) continue;
                        const int64_t d = pj - pa;
                        if (d < est) { if (d > max_lt) max_lt = d; if (sj > ps) { pick = j; ps = sj; } }
                        else if (d < min_ge) min_ge = d;
                    }
                L.pick[i] = pick;
                if (pick >= 0 && (int64_t)sa + ps > top) top = (int64_t)sa + ps;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const int64_t a = __shfl_xor(max_lt, o, 64), b = __shfl_xor(min_ge, o, 64), c = __shfl_xor(top, o, 64);
                if (a > max_lt) max_lt = a;
                if (b < min_ge) min_ge = b;
                if (c > top) top = c;
            }
            wave_sync();
            if (top > 0)
                for (int i = lane; i < n1; i += 64) {
                    const int pick = L.pick[i];
                    if (pick >= 0 && (int64_t)L.score[0][i] + L.score[1][pick] == top) {
                        n_paired++;
                        L.mate[0][i] = pick;
                        atomicMax(&L.mate[1][pick], i); // (read 1's candidates are gone through in order: the last one that picks it stays)
                    }
                }
            for (int o = 32; o > 0; o >>= 1) n_paired += __shfl_xor(n_paired, o, 64);
            lo = (int)(max_lt + 1); hi = (int)min_ge;
            wave_sync();
        }
        // the candidates as the later stages find them in the pair record
        for (int s = 0; s < nr; s++)
            for (int i = lane; i < n_cands[s]; i += 64) {
                Cand c;
                c.score = L.score[s][i]; c.mate = (int16_t)L.mate[s][i]; c.first = (int16_t)(L.span[s][i] & 0xFFFFu); c.count = (int16_t)(L.span[s][i] >> 16); c.pd0 = L.pd[s][i];
                c.frag_off = 0; c.n_frags = 0; c.flag = 0; c.fwd = 1; c.in_pool = 0; c.pad = 0; c.pool_off = 0;
                st.cands[s][i] = c;
            }
        if (lane == 0) {
            PairHdr h;
            h.flags = flags; h.n_frags = 0; h.n_ops = 0; h.pair_dist = 0; h.n_jobs = 0; h.pair_ok = 0; h.mapped = 0; h.pad[0] = h.pad[1] = 0;
            h.n_hits[0] = (int16_t)n_hits[0]; h.n_hits[1] = (int16_t)n_hits[1]; h.n_cands[0] = (int16_t)n_cands[0]; h.n_cands[1] = (int16_t)n_cands[1];
            h.sum[0].best = h.sum[1].best = -1; h.sum[0].score = h.sum[1].score = 0; h.sum[0].sub = h.sum[1].sub = 0;
            h.est = sel.est[local]; h.est_lo = lo; h.est_hi = hi; h.n_paired = (int16_t)n_paired;
            if (cx.pm.paired && !(flags & kOvAny) && n_paired == 0) h.flags |= kAwaitRescue;
            *st.hdr = h;
            if (cx.pm.paired && !(flags & kOvAny) && n_paired == 0) {
                const uint32_t at = atomicAdd(rl.n, 1u);
                if (at < rl.cap) rl.ids[at] = local;
            }
        }
    }
}

constexpr int kRescueThreads = 256;
constexpr unsigned kRescueBlocks = 4096;
// HBM scratch per workgroup for reads with N (RescueWave::window_ids): the read's ids, the longest window's ids and bytes
constexpr size_t kRescueScratchWords = 1024 + (4096 + 64 + 8) + (4096 + 64) / 16 + 8;

// KG: the longest window the tier evaluates (caps.kmer_cap)
template <int KG>
#ifndef MCX_RESCUE_WAVES
#define MCX_RESCUE_WAVES 1
#endif
__global__ void __launch_bounds__(kRescueThreads, MCX_RESCUE_WAVES) k_rescue(Ctx cx, ReadBatch rb, PairSel sel, RescueList rl, uint32_t *kscratch)
{
    // one workgroup per unpaired pair (they are few, and one pair's windows are a long serial chain
    // for a single wavefront); read and window live in LDS as bit planes (RescueWave)
    __shared__ uint32_t q[3 * kRescueQWords];
    __shared__ uint32_t w[2 * rescue_wwords(KG)];
    __shared__ uint32_t ew[kRescueQWords];
    __shared__ int red[2 * (kRescueThreads / 64) + 5];
    const uint32_t n = min(*rl.n, rl.cap);
    RescueWave ev; ev.q = q; ev.w = w; ev.ew = ew; ev.wstride = rescue_wwords(KG); ev.red = red;
    ev.kq = kscratch + (size_t)blockIdx.x * kRescueScratchWords; ev.kg = ev.kq + 1024;
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t local = rl.ids[i];
        ReadRef rd[2];
        make_reads(cx, rb, sel_pair(sel, local), rd);
        stage_rescue(cx, local, rd, ev);
        __syncthreads();
    }
}

// ---- mate rescue, window by window ---------------------------------------------------------------------------------------
// k_rescue gives a pair to one workgroup, which evaluates the pair's windows one after the other: a launch is as long as the
// pair with the most candidates to try (hundreds in the large tier) and its barriers.  But a window's evaluation depends on
// nothing but the candidate it lies beside — only *taking* the results is ordered (the mate's candidate and seed lists grow in
// window order, AlignmentRescue.cpp:28-111).  So: k_rescue_plan lists the windows of every listed pair (one lane per pair: the
// tests of rescue_mate up to the evaluation), k_rescue_eval evaluates the windows, one wavefront each, on bit planes in its
// share of LDS, and k_rescue_apply takes the results pair by pair in window order (one lane per pair: the rest of rescue_mate).
// Pairs with a read that holds an N keep k_rescue (the reference's 8-mer ids fall out of step after an N: RescueWave::window_ids).
struct RescueTask {
    uint32_t local;      // the pair (index in the pass)
    uint16_t side, ci;   // side 0: read 2 next to candidate ci of read 1; side 1: the other way round
    int32_t slen, sb;    // window length; the score a window has to beat
    int64_t left;
    int32_t pad[2];
};
static_assert(sizeof(RescueTask) == 32, "RescueTask is two 16-byte records");
struct RescueRes { int32_t score, d, n_seeds; uint32_t seed_off; }; // (seeds: n_seeds entries of the pass's seed pool from seed_off on)
struct RescuePlan { uint32_t local, first, n, flags; }; // a listed pair's windows [first, first + n) and the flags rescue_mate adds

struct RescueWork {
    RescueTask *tasks; RescueRes *res; Hit *seeds; RescuePlan *plans;
    uint32_t *n_tasks, *n_plans, *n_seeds;
    uint32_t task_cap, seed_cap; // windows the list holds; seeds the pool holds
    uint32_t *ids_n, *n_ids_n; // pairs left to k_rescue (a read with N)
};

__global__ void __launch_bounds__(256) k_rescue_plan(Ctx cx, ReadBatch rb, PairSel sel, RescueList rl, RescueWork rw)
{
    __shared__ EndsLds ends;
    stage_ends(cx.ix, ends);
    const IndexView &ix = cx.ix;
    const uint32_t n = min(*rl.n, rl.cap);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t local = rl.ids[i];
        const uint32_t pair = sel_pair(sel, local);
        PairState st = pair_state(cx.state, cx.lay, cx.caps, local);
        const PairHdr h = *st.hdr;
        if ((h.flags & kOvAny) || h.n_paired != 0) continue; // (stage_rescue's test)
        if ((cx.read_ext[2 * pair] | cx.read_ext[2 * pair + 1]) >> 31) { // a read with N: the id path
            const uint32_t at = atomicAdd(rw.n_ids_n, 1u);
            rw.ids_n[at] = local; // (as long as the list of listed pairs)
            continue;
        }
        const int rlen[2] = {(int)(rb.off[2 * pair + 1] - rb.off[2 * pair]), (int)(rb.off[2 * pair + 2] - rb.off[2 * pair + 1])};
        const int n1 = h.n_cands[0], n2 = h.n_cands[1];
        const Cand *c1 = st.cands[0], *c2 = st.cands[1];
        int s1 = 0, s2 = 0;
        for (int k = 0; k < n1; k++) { const int sc = c1[k].score; if (sc > s1) s1 = sc; }
        for (int k = 0; k < n2; k++) { const int sc = c2[k].score; if (sc > s2) s2 = sc; }
        int mode;
        if (s1 < (rlen[0] >> 2) && s2 < (rlen[1] >> 2)) continue; // rescue_mate returns 0 and leaves the pair alone
        else if (s1 - s2 > (rlen[1] >> 2)) mode = 1;
        else if (s2 - s1 > (rlen[0] >> 2)) mode = 2;
        else mode = 3;
        uint32_t flags = kRescueUsedEst;
        const int64_t est = (int64_t)(uint32_t)h.est;
        // two passes over the candidates: count the windows, reserve their places, write them
        uint32_t first = 0, count = 0;
        for (int pass = 0; pass < 2; pass++) {
            uint32_t at = first;
            for (int side = 0; side < 2; side++) {
                if (side == 0 && !(mode == 1 || mode == 3)) continue;
                if (side == 1 && !(mode == 2 || mode == 3)) continue;
                const int qlen = side == 0 ? rlen[1] : rlen[0];
                const Cand *ca = side == 0 ? c1 : c2;
                const int na = side == 0 ? n1 : n2, sa = side == 0 ? s1 : s2, sb = side == 0 ? s2 : s1;
                const int thr = sa >> 1;
                for (int ci = 0; ci < na; ci++) {
                    const Cand c = ca[ci];
                    if (c.score < thr || c.mate != -1) continue;
                    const int64_t left = side == 0 ? c.pd0 : c.pd0 - est;
                    int64_t right = side == 0 ? c.pd0 + est + qlen : c.pd0 + qlen;
                    if (right > ix.G2) right = ix.G2;
                    if (left < 0 || right >= ix.G2) continue;
                    const int e1 = end_slot(ix, left), e2 = end_slot(ix, right);
                    if (e1 < 0 || e2 < 0 || ix.end_chr[e1] != ix.end_chr[e2]) continue;
                    const int slen = (int)(right - left);
                    if (slen < qlen) continue;
                    if (slen > cx.caps.kmer_cap) { flags |= kOvKmer; continue; }
                    if (pass == 0) count++;
                    else {
                        if (at < rw.task_cap) {
                            RescueTask t; t.local = local; t.side = (uint16_t)side; t.ci = (uint16_t)ci; t.slen = slen; t.sb = sb; t.left = left; t.pad[0] = t.pad[1] = 0;
                            rw.tasks[at] = t;
                        }
                        at++;
                    }
                }
            }
            if (pass == 0) first = count ? atomicAdd(rw.n_tasks, count) : 0u;
        }
        RescuePlan pl; pl.local = local; pl.first = first; pl.n = count; pl.flags = flags;
        rw.plans[atomicAdd(rw.n_plans, 1u)] = pl; // (as long as the list of listed pairs)
    }
}

template <int KG>
__global__ void __launch_bounds__(256) k_rescue_eval(Ctx cx, ReadBatch rb, PairSel sel, RescueWork rw)
{
    constexpr int kWaves = 4, kW = rescue_wwords(KG);
    __shared__ uint32_t q_all[kWaves][3 * kRescueQWords];
    __shared__ uint32_t w_all[kWaves][2 * kW];
    __shared__ uint32_t ew_all[kWaves][kRescueQWords];
    __shared__ uint16_t ss_all[kWaves][128]; // where the seeds of a window's best diagonal begin (a read of 1024 bases has at most 94)
    const IndexView &ix = cx.ix;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    RescueWave ev; ev.q = q_all[wv]; ev.w = w_all[wv]; ev.ew = ew_all[wv]; ev.wstride = kW; ev.red = nullptr; ev.kq = ev.kg = nullptr;
    uint32_t *ql = ev.q, *qh = ev.q + kRescueQWords, *qv = ev.q + 2 * kRescueQWords, *wl = ev.w, *wh = ev.w + kW;
    const uint32_t n = min(*rw.n_tasks, rw.task_cap);
    auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    for (uint32_t t = blockIdx.x * kWaves + wv; t < n; t += gridDim.x * kWaves) {
        const RescueTask task = rw.tasks[t];
        const uint32_t pair = sel_pair(sel, task.local), r = 2 * pair + (task.side == 0 ? 1u : 0u);
        const int qlen = (int)(rb.off[r + 1] - rb.off[r]), slen = task.slen;
        const uint32_t *codes = cx.packed + (uint64_t)r * cx.wpad; // the read as mapped: mate 2 reverse-complemented (no N: k_rescue_plan)
        wave_sync();
        // the read's planes (base i at bit i & 31 of word i >> 5) and where a base counts (inside the read)
        for (int k = lane; k < kRescueQWords; k += 64) {
            uint32_t lo = 0, hi = 0, in = 0;
            if (32 * k < qlen) {
                const uint32_t a = codes[2 * k], b = 32 * k + 16 < qlen ? codes[2 * k + 1] : 0u;
                lo = (__brev(even_bits16(a)) >> 16) | (__brev(even_bits16(b)) & 0xFFFF0000u);
                hi = (__brev(even_bits16(a >> 1)) >> 16) | (__brev(even_bits16(b >> 1)) & 0xFFFF0000u);
                in = qlen - 32 * k >= 32 ? ~0u : ((1u << (qlen - 32 * k)) - 1u);
                lo &= in; hi &= in;
            }
            ql[k] = lo; qh[k] = hi; qv[k] = in;
        }
        wave_sync();
        uint32_t v8 = 0;
        if (lane < kRescueQWords) { // an 8-mer starts where eight bases of the read follow one another
            const uint32_t v = qv[lane], vn = lane + 1 < kRescueQWords ? qv[lane + 1] : 0u;
            v8 = v;
#pragma unroll
            for (int j = 1; j < kKmerSize; j++) v8 &= __funnelshift_r(v, vn, j);
        }
        wave_sync();
        if (lane < kRescueQWords) qv[lane] = v8;
        // the window's planes (RescueWave::window)
        const int pad = ((qlen + 31) & ~31) + 32;
        const int n_words = (pad + slen + qlen) / 32 + 3;
        for (int j = lane; j < n_words; j += 64) {
            uint32_t lo = 0, hi = 0;
            const int p0 = 32 * j - pad;
            if (p0 >= 0 && p0 < slen) {
#pragma unroll
                for (int half = 0; half < 2; half++) {
                    const int p = p0 + 16 * half;
                    if (p >= slen) break;
                    const uint32_t x = ref_codes16(ix, task.left + p);
                    uint32_t l16 = __brev(even_bits16(x)) >> 16, h16 = __brev(even_bits16(x >> 1)) >> 16;
                    if (slen - p < 16) { const uint32_t keep = (1u << (slen - p)) - 1u; l16 &= keep; h16 &= keep; }
                    lo |= l16 << (16 * half); hi |= h16 << (16 * half);
                }
            }
            wl[j] = lo; wh[j] = hi;
        }
        wave_sync();
        const int d_lo = -(qlen - kKmerSize - 2), n_diag = slen - kKmerSize - 2 - d_lo + 1;
        uint32_t key = 0;
        for (int g = lane; g < n_diag; g += 64) {
            const int total = ev.diagonal(d_lo + g, qlen, slen, pad, false);
            const uint32_t k2 = ((uint32_t)total << 13) | (uint32_t)(8191 - g);
            if (total > 0 && k2 > key) key = k2;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t other = (uint32_t)__shfl_xor((int)key, o, 64); if (other > key) key = other; }
        RescueRes res; res.score = (int)(key >> 13); res.d = 0; res.n_seeds = 0; res.seed_off = 0;
        if (key != 0) {
            res.d = d_lo + (8191 - (int)(key & 8191u));
            if (res.score > task.sb) { // (a window that does not beat the mate's best is dropped whatever its seeds)
                for (int k = lane; k < kRescueQWords; k += 64) ev.ew[k] = 0u;
                wave_sync();
                if (lane == 0) ev.diagonal(res.d, qlen, slen, pad, true); // the best diagonal's 8-mer match words, a word per 32 rows
                wave_sync();
                // The seeds of the diagonal: runs of three or more 8-mer matches (ten or more matching bases), in the order of their rows.  A lane per
                // word: where such a run begins and where it ends are two bit masks, the j-th beginning and the j-th end of the wavefront are one run's, and
                // two counts summed across the lanes number them.  (One lane walked the read's rows before, twice — counting, then writing —, a dependent
                // LDS read per row: some 7 000 instructions of a wavefront's time per window that beat its mate, more than the window's 1 300 diagonals cost.)
                uint32_t S = 0, E = 0;
                if (lane < kRescueQWords) {
                    const uint32_t e0 = ev.ew[lane], e1 = lane + 1 < kRescueQWords ? ev.ew[lane + 1] : 0u, ep = lane > 0 ? ev.ew[lane - 1] : 0u;
                    const uint32_t t = e0 & __funnelshift_r(e0, e1, 1) & __funnelshift_r(e0, e1, 2); // a triple of matches begins here
                    const uint32_t t_before = (ep >> 31) & e0 & (e0 >> 1) & 1u;                      // ... at the last row of the word before
                    const uint32_t t_after = e1 & (e1 >> 1) & (e1 >> 2) & 1u;                         // ... at the first row of the word after
                    S = t & ~((t << 1) | t_before);
                    E = t & ~((t >> 1) | (t_after << 31));
                }
                const int cs = __popc(S), ce = __popc(E);
                int is = cs, ie = ce;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int vs = __shfl_up(is, o, 64), ve = __shfl_up(ie, o, 64);
                    if (lane >= o) { is += vs; ie += ve; }
                }
                const int n_seeds = __shfl(is, 63, 64);
                uint32_t off = 0;
                if (lane == 0) off = atomicAdd(rw.n_seeds, (uint32_t)n_seeds);
                off = (uint32_t)__shfl((int)off, 0, 64);
                res.n_seeds = n_seeds; res.seed_off = off;
                if ((uint64_t)off + (uint64_t)n_seeds <= rw.seed_cap) { // (else the pool ran over: the pass is repeated in halves)
                    uint16_t *ss = ss_all[wv];
                    int j = is - cs;
                    for (uint32_t m = S; m; m &= m - 1u) ss[j++] = (uint16_t)(32 * lane + __ffs((int)m) - 1);
                    wave_sync();
                    Hit *out = rw.seeds + off;
                    j = ie - ce;
                    for (uint32_t m = E; m; m &= m - 1u, j++) {
                        const int start = ss[j], end = 32 * lane + __ffs((int)m) - 1; // the run's first and last triple: its 8-mer matches end two rows later
                        Hit h; h.rPos = start; h.gPos = (int64_t)(start + res.d) + task.left; h.len = end - start + 1 + kKmerSize + 1;
                        out[j] = h;
                    }
                }
            }
        }
        if (lane == 0) rw.res[t] = res;
    }
}

__global__ void __launch_bounds__(256) k_rescue_apply(Ctx cx, RescueWork rw)
{
    const uint32_t n = *rw.n_plans;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const RescuePlan pl = rw.plans[i];
        PairState st = pair_state(cx.state, cx.lay, cx.caps, pl.local);
        PairHdr h = *st.hdr;
        int nc[2] = {h.n_cands[0], h.n_cands[1]}, nh[2] = {h.n_hits[0], h.n_hits[1]};
        uint32_t flags = pl.flags;
        int paired = 0;
        for (uint32_t k = 0; k < pl.n; k++) {
            const uint32_t t = pl.first + k;
            if (t >= rw.task_cap) break; // (the list ran over: the pass is repeated in halves)
            const RescueRes res = rw.res[t];
            if (res.n_seeds == 0) continue;
            const RescueTask task = rw.tasks[t];
            if (res.score <= task.sb) continue;
            const int a = task.side, b = 1 - task.side; // candidate ci of read a gets a mate among read b's
            if ((uint64_t)res.seed_off + (uint64_t)res.n_seeds > rw.seed_cap) break; // (the pool ran over)
            if (nc[b] >= cx.caps.cand_cap) { flags |= kOvCands; continue; }
            paired++;
            // the new candidate's seeds stay in the pool (stage_build reads them there): no copy, and no bound on how many
            // seeds mate rescue may add to a read (a candidate per window, up to rlen / 11 seeds each)
            st.cands[a][task.ci].mate = (int16_t)nc[b];
            Cand nw;
            nw.score = res.score; nw.mate = (int16_t)task.ci; nw.first = 0; nw.count = (int16_t)res.n_seeds; nw.pd0 = (int64_t)res.d + task.left;
            nw.frag_off = 0; nw.n_frags = 0; nw.flag = 0; nw.fwd = 1; nw.in_pool = 1; nw.pad = 0; nw.pool_off = (int32_t)res.seed_off;
            st.cands[b][nc[b]] = nw;
            nc[b]++;
        }
        h.flags |= flags;
        h.n_cands[0] = (int16_t)nc[0]; h.n_cands[1] = (int16_t)nc[1];
        h.n_hits[0] = (int16_t)nh[0]; h.n_hits[1] = (int16_t)nh[1];
        h.n_paired = (int16_t)paired;
        *st.hdr = h;
    }
}

// fragment lists + DP problems of every pair; the problems are appended to one list per size
// class (mcx_glue.h dp_class) with one atomic per wave and class
// (late: the pairs that ran over this tier's capacities since clustering — mate rescue's additions, fragment lists, DP
//  columns, job lists — are listed like the early ones, for a second pass of the large tier beside the rest of this one)
#ifndef MCX_BUILD_WAVES
#define MCX_BUILD_WAVES 4 // (with the light pairs gone to k_simple what is left is heavier per lane: 128 registers, no spills, beat five waves at 96 with 51 spilled)
#endif
// (mode 0: every listed pair.  Mate rescue touches one pair in eighty, and the other seventy-nine need nothing from it: mode 1 builds
//  the pairs that do not await it — beside the rescue kernels, on another stream — and mode 2, once those are through, the pairs of
//  the rescue list rl.)
__global__ void __launch_bounds__(256, MCX_BUILD_WAVES) k_build(Ctx cx, ReadBatch rb, PairSel sel, JobSinks sinks, uint32_t *cells, uint32_t *unsupported, EarlyList late,
                                               const uint32_t *order, const uint32_t *order_cnt, int mode, RescueList rl)
{
    __shared__ EndsLds ends;
    const uint32_t n_listed = mode == 2 ? min(*rl.n, rl.cap) : listed_pairs(sel, order_cnt);
    if (blockIdx.x * blockDim.x >= n_listed) return; // (uniform over the block)
    stage_ends(cx.ix, ends);
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    bool in = slot < n_listed;
    const uint32_t local = in ? (mode == 2 ? rl.ids[slot] : (order ? order[slot] : slot)) : 0u;
    // (the rescue list's pairs are mode 2's: told by a flag the clustering set and nobody clears — the rescue, which runs beside mode 1,
    //  rewrites those pairs' headers and candidates meanwhile)
    if (in && mode == 1 && (pair_state(cx.state, cx.lay, cx.caps, local).hdr->flags & kAwaitRescue)) in = false;
    int nj = 0;
    uint32_t fl = 0, n_mask = 0; // n_mask: bit s = read s of the pair holds a byte that is not ACGT (a DP problem of it says so: DpJob::score on its way in)
    if (in) {
        ReadRef rd[2];
        make_reads(cx, rb, sel_pair(sel, local), rd);
        n_mask = (rd[0].codes ? 0u : 1u) | ((cx.pm.paired && !rd[1].codes) ? 2u : 0u);
        nj = stage_build(cx, local, rd, &fl);
    }
    const bool over = late.ids && (fl & kOvAny) && !(fl & kDispatched);
    if (__ballot(over)) { // (a handful of pairs per batch)
        if (over) {
            const uint32_t at = atomicAdd(late.n, 1u);
            // past the room kept for them the pair stays undispatched: k_finish lists it and it is mapped after the pass
            if (at < late.cap) { late.ids[at] = sel_pair(sel, local); late.est[at] = sel.est[local]; pair_state(cx.state, cx.lay, cx.caps, local).hdr->flags = fl | kDispatched; }
        }
    }
    // (the per-class counters are updated under a compile-time index: an array indexed by a run-time class lives in scratch memory)
    uint32_t per_class[kDpClasses] = {0, 0, 0, 0, 0, 0}, my_cells = 0, bad = 0;
    for (int k = 0; k < nj; k++) {
        const DpJob j = pair_job(cx, local, k);
        const int c = job_class(j);
        if (c < 0) bad++; else my_cells += (uint32_t)(j.rLen * j.gLen);
#pragma unroll
        for (int q = 0; q < kDpClasses; q++) per_class[q] += c == q ? 1u : 0u;
    }
    uint32_t base[kDpClasses];
#pragma unroll
    for (int c = 0; c < kDpClasses; c++) base[c] = wave_reserve(sinks.s[c].count, per_class[c]);
    for (int k = 0; k < nj; k++) {
        DpJob j = pair_job(cx, local, k);
        j.score = (int32_t)((n_mask >> j.slot) & 1u);
        const int c = job_class(j);
        if (c < 0) continue;
        uint32_t at = 0;
#pragma unroll
        for (int q = 0; q < kDpClasses; q++) if (c == q) { at = base[q]++; if (at < sinks.s[q].cap) sinks.s[q].jobs[at] = j; }
    }
    for (int o = 32; o > 0; o >>= 1) { my_cells += __shfl_down(my_cells, o, 64); bad += __shfl_down(bad, o, 64); }
    // (64 bits: the problems of one pass of BASELINE config 5 hold 5 x 10^10 cells)
    if ((threadIdx.x & 63) == 0) { if (my_cells) atomicAdd((unsigned long long *)cells, (unsigned long long)my_cells); if (bad) atomicAdd(unsupported, bad); }
}

// ---- the large tier's build: a wavefront per pair ---------------------------------------------------------------------------
// The large tier's pairs come from repeats: hundreds of candidates each, and k_build gives a pair to ONE lane, which builds them one
// after the other — the launch is as long as that lane (1.9 ms for 30 k pairs: the step waited for it).  Here a wavefront takes the
// pair and a lane a candidate, sixty-four at a time in the order stage_build goes through them:
//   * scores and mates of both reads' candidates in LDS: keep_top_scores / mask_unpaired with wave-wide maxima;
//   * a candidate's fragments go where an exclusive scan over the candidates' bounds (2 seeds + 2) puts them — holes of a fragment
//     or two instead of the serial running count: nothing reads the pool but through a candidate's (frag_off, n_frags) —, its gap
//     fragments are classified as ProcessNormalPair does, its DP problems counted by list;
//   * scans over those counts give every lane its stretch of the pair's column area (64 bytes for the summary + the columns, in
//     multiples of 8) and its places in the pass's job lists (one atomic per list and round), and the lane writes its problems there.
// Same fragments, same kinds, same DP problems as stage_build; only where they lie in the pair's pools differs, which no result sees.
// mode: as k_build's.
// lane_limit: the pairs whose bounds come to more than this are built by one lane as well (tests: 0 sends every pair that way)
__global__ void __launch_bounds__(64) k_build_wave(Ctx cx, ReadBatch rb, PairSel sel, JobSinks sinks, uint32_t *cells, uint32_t *unsupported, int mode, RescueList rl, int lane_limit)
{
    extern __shared__ int32_t bw_lds[]; // score[2][cand_cap], mate[2][cand_cap], seeds[2][cand_cap]
    __shared__ EndsLds ends;
    stage_ends(cx.ix, ends);
    const int lane = threadIdx.x;
    const int nr = cx.pm.paired ? 2 : 1, cap = cx.caps.cand_cap;
    int32_t *sc[2] = {bw_lds, bw_lds + cap}, *mt[2] = {bw_lds + 2 * cap, bw_lds + 3 * cap}, *cn[2] = {bw_lds + 4 * cap, bw_lds + 5 * cap};
    auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_s_barrier(); };
    auto wave_max = [](int v) { for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64)); return v; };
    auto wave_sum = [](uint32_t v) { for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64); return v; };
    auto excl_scan = [&](uint32_t v) { uint32_t in = v; for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)in, o, 64); if (lane >= o) in += t; } return in - v; };
    const uint32_t n_listed = mode == 2 ? min(*rl.n, rl.cap) : sel.n;
    uint32_t my_cells = 0, bad = 0;
    for (uint32_t slot = blockIdx.x; slot < n_listed; slot += gridDim.x) {
        const uint32_t local = mode == 2 ? rl.ids[slot] : slot;
        PairState st = pair_state(cx.state, cx.lay, cx.caps, local);
        PairHdr h = *st.hdr; // (every lane the same words: one fetch)
        if (mode == 1 && (h.flags & kAwaitRescue)) continue;
        auto put_hdr = [&](uint32_t flags, int n_frags, int n_ops, int n_jobs) {
            if (lane == 0) { st.hdr->flags = flags; st.hdr->n_frags = n_frags; st.hdr->n_ops = n_ops; st.hdr->n_jobs = (int16_t)n_jobs; }
        };
        if (h.flags & kOvAny) { put_hdr(h.flags, 0, 0, 0); continue; }
        const int n_c[2] = {h.n_cands[0], nr == 2 ? h.n_cands[1] : 0};
        ReadRef rd[2];
        make_reads(cx, rb, sel_pair(sel, local), rd);
        // ---- scores and mates into LDS; the masks of ReadMapping.cpp:469-470 (keep_top_scores / mask_unpaired)
        wave_sync();
        for (int s = 0; s < nr; s++) for (int i = lane; i < n_c[s]; i += 64) { const Cand c = st.cands[s][i]; sc[s][i] = c.score; mt[s][i] = c.mate; cn[s][i] = c.count; }
        wave_sync();
        auto keep_top = [&](int s) {
            if (n_c[s] <= 1) return;
            int best = 0;
            for (int i = lane; i < n_c[s]; i += 64) best = max(best, sc[s][i]);
            best = wave_max(best);
            for (int i = lane; i < n_c[s]; i += 64) if (sc[s][i] < best) sc[s][i] = 0;
        };
        if (cx.pm.paired && h.n_paired != 0) {
            int top = 0;
            for (int i = lane; i < n_c[0]; i += 64) if (mt[0][i] != -1) top = max(top, sc[0][i] + sc[1][mt[0][i]]);
            top = wave_max(top);
            for (int i = lane; i < n_c[0]; i += 64) if (mt[0][i] == -1 || sc[0][i] + sc[1][mt[0][i]] < top) sc[0][i] = 0; // (read 2's scores are still what they were)
            wave_sync();
            for (int j = lane; j < n_c[1]; j += 64) if (mt[1][j] == -1 || sc[1][j] + sc[0][mt[1][j]] < top) sc[1][j] = 0;  // (read 1's as the loop above left them)
        } else { keep_top(0); if (cx.pm.paired) keep_top(1); }
        wave_sync();
        // ---- the fragments are placed by their bounds (2 seeds + 2 per live candidate), stage_build places them densely: when the bounds of
        //      all live candidates fit the pool both ways fit; when they do not, the pair is built stage_build's way, by one lane — the same
        //      fragments wherever they lie, and the same answer to "does this pair fit the tier" (a pair that does not is fatal for the batch)
        {
            uint32_t tb = 0;
            for (int s = 0; s < nr; s++) for (int i = lane; i < n_c[s]; i += 64) if (sc[s][i] != 0) tb += 2u * (uint32_t)cn[s][i] + 2u;
            tb = wave_sum(tb);
            if (tb > (uint32_t)min(cx.caps.frag_cap, lane_limit)) {
                if (lane == 0) {
                    const int nj = stage_build(cx, local, rd);
                    for (int k = 0; k < nj; k++) {
                        DpJob j = pair_job(cx, local, k);
                        j.score = rd[j.slot].codes ? 0 : 1;
                        const int q = job_class(j);
                        if (q < 0) { bad++; continue; }
                        my_cells += (uint32_t)(j.rLen * j.gLen);
#pragma unroll
                        for (int c = 0; c < kDpClasses; c++) if (q == c) { const uint32_t at = atomicAdd(sinks.s[c].count, 1u); if (at < sinks.s[c].cap) sinks.s[c].jobs[at] = j; }
                    }
                }
                continue;
            }
        }
        // ---- the candidates, a lane each, in stage_build's order
        uint32_t flags = h.flags, n_frags = 0, n_ops = 0, n_jobs = 0;
        const int total = n_c[0] + n_c[1];
        for (int base = 0; base < total && !(flags & kOvAny); base += 64) {
            const int t = base + lane;
            const bool mine = t < total;
            const int s = (mine && t >= n_c[0]) ? 1 : 0, ci = mine ? t - (s ? n_c[0] : 0) : 0;
            Cand c; c.count = 0; c.first = 0; c.in_pool = 0; c.pool_off = 0; c.score = 0;
            bool live = false;
            if (mine) { c = st.cands[s][ci]; live = sc[s][ci] != 0; }
            const uint32_t bound = live ? 2u * (uint32_t)c.count + 2u : 0u;
            const uint32_t off = n_frags + excl_scan(bound);
            const uint32_t round_frags = wave_sum(bound);
            if (n_frags + round_frags > (uint32_t)cx.caps.frag_cap) { flags |= kOvFrags; break; } // (uniform)
            Frag *f = st.frags + off;
            int nf = 0;
            uint32_t my_ops = 0, my_cls[kDpClasses] = {0, 0, 0, 0, 0, 0};
            if (mine) {
                if (live) {
                    nf = build_frags(cx.ix, rd[s].rlen, c.in_pool ? cx.seed_pool + c.pool_off : st.hits[s] + c.first, c.count, f);
                    // ProcessNormalPair (:155-191): classify each gap fragment; a DP problem's place in the column area comes later
                    for (int i = 0; i < nf; i++) {
                        Frag x = f[i];
                        if (x.kind == kSimple) continue;
                        if (x.rLen > 0 && x.gLen > 0) {
                            bool dp = x.rLen != x.gLen;
                            int mm = -1;
                            if (!dp) { mm = frag_mismatches(cx.ix, x, rd[s]); dp = mm > 1 && mm >= (int)(x.rLen * 0.2); }
                            if (dp) {
                                x.kind = kDp; x.ops_off = 0; x.ops_len = 0; x.meta = 0;
                                my_ops += (uint32_t)kDpSum + (((uint32_t)(x.rLen + x.gLen) + 7u) & ~7u);
                                DpJob j; j.rLen = x.rLen; j.gLen = x.gLen;
                                const int q = job_class(j);
                                if (q < 0) bad++; else my_cells += (uint32_t)(x.rLen * x.gLen);
#pragma unroll
                                for (int k = 0; k < kDpClasses; k++) my_cls[k] += q == k ? 1u : 0u;
                            } else { x.kind = kPlain; x.ops_len = x.rLen; x.meta = (uint32_t)(mm + 1); }
                        } else if (x.rLen > 0) { x.kind = kIns; x.ops_len = x.rLen; }
                        else { x.kind = kDel; x.ops_len = x.gLen; }
                        f[i] = x;
                    }
                }
                // (what changed of the candidate: its place in the fragment pool, and its score when a mask or the validity check dropped it)
                Cand *g = st.cands[s] + ci;
                g->frag_off = (int16_t)off; g->n_frags = (int16_t)(nf < 0 ? 0 : nf);
                const int new_score = (live && nf >= 0) ? c.score : 0;
                if (new_score != c.score) g->score = new_score;
            }
            // ---- places: the column area of the pair, the job lists of the pass
            uint32_t my_jobs = 0;
#pragma unroll
            for (int k = 0; k < kDpClasses; k++) my_jobs += my_cls[k];
            uint32_t cur = n_ops + excl_scan(my_ops);
            const uint32_t round_ops = wave_sum(my_ops), round_jobs = wave_sum(my_jobs);
            if (n_ops + round_ops > (uint32_t)cx.caps.ops_cap) { flags |= kOvOps; break; }
            if (n_jobs + round_jobs > (uint32_t)cx.caps.job_cap) { flags |= kOvJobs; break; }
            uint32_t at_cls[kDpClasses];
#pragma unroll
            for (int k = 0; k < kDpClasses; k++) at_cls[k] = wave_reserve(sinks.s[k].count, my_cls[k]);
            if (my_jobs) {
                for (int i = 0; i < nf; i++) {
                    Frag x = f[i];
                    if (x.kind != kDp) continue;
                    x.ops_off = (int64_t)(cur + (uint32_t)kDpSum);
                    cur += (uint32_t)kDpSum + (((uint32_t)(x.rLen + x.gLen) + 7u) & ~7u);
                    f[i] = x;
                    DpJob j;
                    j.pair = local; j.slot = (uint16_t)s; j.rev = x.gPos >= cx.ix.G ? 1 : 0;
                    j.rPos = x.rPos; j.rLen = x.rLen; j.gPos = x.gPos; j.gLen = x.gLen;
                    j.ops_off = (int32_t)x.ops_off; j.frag = (int32_t)(off + (uint32_t)i); j.score = rd[s].codes ? 0 : 1;
                    const int q = job_class(j);
#pragma unroll
                    for (int k = 0; k < kDpClasses; k++) if (q == k) { const uint32_t at = at_cls[k]++; if (at < sinks.s[k].cap) sinks.s[k].jobs[at] = j; }
                }
            }
            n_frags += round_frags; n_ops += round_ops; n_jobs += round_jobs;
        }
        put_hdr(flags, (int)n_frags, (int)n_ops, (int)n_jobs);
    }
    my_cells = wave_sum(my_cells); bad = wave_sum(bad);
    if (lane == 0) { if (my_cells) atomicAdd((unsigned long long *)cells, (unsigned long long)my_cells); if (bad) atomicAdd(unsupported, bad); }
}

// -m: the lines of a read after its first (emit_extra) go to an extras pool that the finish kernel fills in no particular order; per read
// {record offset, records, word offset, words} says where its lines went.  A re-run pair writes a fresh entry (what it took before is left
// unreferenced); a pair that did not fit says so with kMxOver in its count and is mapped again once the pool has grown (multi_close).
constexpr uint32_t kMxOver = 0x80000000u;
struct MultiOut {
    AlnRec *recs = nullptr; uint32_t *cig = nullptr; // the pool
    uint32_t *cnt = nullptr;                          // [0] records taken, [1] CIGAR words taken (both count on past the capacity)
    uint32_t rec_cap = 0, word_cap = 0;
    uint4 *ref = nullptr;                             // per batch read
};

#ifndef MCX_FINISH_WAVES
#define MCX_FINISH_WAVES 4 // (109 registers, no spills; five waves at 96 spilled 16)
#endif
// kMulti: -m — a read's lines after the first are counted and written in the same pass (the default instantiation never looks at mo)
template <bool kMulti>
__global__ void __launch_bounds__(256, MCX_FINISH_WAVES) k_finish(Ctx cx, ReadBatch rb, PairSel sel, AlnRec *recs, PairOut *pout, uint32_t *ov_ids, uint32_t *n_ov,
                                                uint32_t ov_cap, uint32_t *pool_over, const uint32_t *order, const uint32_t *order_cnt, MultiOut mo)
{
    __shared__ EndsLds ends;
    __shared__ uint32_t cig_stage[256 * 2 * kCigStage]; // the first operations of every read, word-major: word k of thread t at [k * 256 + t] (neighbouring lanes, neighbouring banks)
    if (blockIdx.x * blockDim.x >= listed_pairs(sel, order_cnt)) return; // (uniform over the block)
    stage_ends(cx.ix, ends);
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t *stage = cig_stage + threadIdx.x;
    const bool active = slot < listed_pairs(sel, order_cnt); // (no early exit within a wave: it reserves its CIGAR words together)
    const uint32_t local = active ? (order ? order[slot] : slot) : 0u;
    const int nr = cx.pm.paired ? 2 : 1;
    uint32_t pair = 0;
    ReadRef rd[2];
    PairState st;
    PairHdr h; // the final header stays in registers: nothing reads the pair state after this kernel
    h.flags = 0;
    int n_cig[2] = {0, 0};
    uint8_t *detail2 = nullptr;
    if (active) {
        pair = sel_pair(sel, local);
        make_reads(cx, rb, pair, rd);
        st = pair_state(cx.state, cx.lay, cx.caps, local);
        h = *st.hdr;
        st.hdr = &h;
        detail2 = cx.detail ? cx.detail + (int64_t)pair * nr * cx.dlay.stride : nullptr; // records are indexed by batch read
        finish_scores(cx, st, rd, (DetailHdr *)detail2, n_cig, nullptr, stage, 256);
    }
    const uint32_t want = (uint32_t)(n_cig[0] + n_cig[1]);
    const uint32_t at = wave_reserve(cx.cig_pool_n, want);
    // (-m) the extra lines of the pair's reads: counted here, reserved like the CIGAR words — one atomic per wavefront for each count
    const bool own = active && !(h.flags & (kDispatched | kOvAny));
    int n_ext[2] = {0, 0}, n_extw[2] = {0, 0};
    uint32_t at_ext = 0, at_extw = 0;
    if (kMulti) {
        if (own) for (int s = 0; s < nr; s++) n_ext[s] = extra_lines(st, s, rd, &n_extw[s]);
        at_ext = wave_reserve(mo.cnt, (uint32_t)(n_ext[0] + n_ext[1]));
        at_extw = wave_reserve(mo.cnt + 1, (uint32_t)(n_extw[0] + n_extw[1]));
    }
    if (!active || (h.flags & kDispatched)) return; // (a dispatched pair is the large tier's: its records and summary come from there)
    const bool fits = at + want <= cx.cig_pool_cap;
    if (!fits) atomicOr(pool_over, 1u);
    const uint32_t off[2] = {at, at + (uint32_t)n_cig[0]};
    finish_records(cx, st, rd, recs + (int64_t)pair * nr, fits ? cx.cig_pool : nullptr, off, n_cig, detail2, stage, 256);
    if (kMulti && own) {
        const bool room = at_ext + (uint32_t)(n_ext[0] + n_ext[1]) <= mo.rec_cap && at_extw + (uint32_t)(n_extw[0] + n_extw[1]) <= mo.word_cap;
        for (int s = 0; s < nr; s++) {
            const uint32_t ro = at_ext + (s ? (uint32_t)n_ext[0] : 0u), wo = at_extw + (s ? (uint32_t)n_extw[0] : 0u);
            mo.ref[(int64_t)pair * nr + s] = room || n_ext[0] + n_ext[1] == 0 ? make_uint4(ro, (uint32_t)n_ext[s], wo, (uint32_t)n_extw[s]) : make_uint4(0u, (uint32_t)n_ext[s] | kMxOver, 0u, 0u);
            if (room && n_ext[s]) emit_extra(cx, st, s, rd, mo.recs + ro, mo.cig + wo, wo);
        }
    }
    PairOut o;
    o.flags = h.flags; o.est = h.est; o.est_lo = h.est_lo; o.est_hi = h.est_hi;
    o.pair_dist = h.pair_dist; o.pair_ok = (int16_t)h.pair_ok; o.mapped = (int16_t)h.mapped;
    pout[pair] = o;
    if (h.flags & kOvAny) {
        const uint32_t at2 = atomicAdd(n_ov, 1u);
        if (at2 < ov_cap) ov_ids[at2] = pair;
    }
}

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
static Knobs knobs_read()
{
    Knobs k;
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    k.timing = on("MCX_TIMING"); k.seed_one_base = on("MCX_SEED_ONE_BASE"); k.dp_by_wave = on("MCX_DP_BY_WAVE"); k.dp_lane_always = on("MCX_DP_LANE_ALWAYS");
    k.late_reseed = on("MCX_LATE_RESEED"); k.no_work_order = on("MCX_NO_WORK_ORDER"); k.no_simple = on("MCX_NO_SIMPLE"); k.simple_no_dp = on("MCX_SIMPLE_NO_DP");
    k.cluster_by_lane = on("MCX_CLUSTER_BY_LANE"); k.rescue_in_line = on("MCX_RESCUE_IN_LINE"); k.build_by_lane = on("MCX_BUILD_BY_LANE");
    k.no_sums_cache = on("MCX_NO_SUMS_CACHE"); k.prof_by_column = on("MCX_PROF_BY_COLUMN"); k.tier1_hist = on("MCX_TIER1_HIST"); k.dp_hist = on("MCX_DP_HIST");
    k.no_tier_overlap = on("MCX_NO_TIER_OVERLAP"); k.no_late_overlap = on("MCX_NO_LATE_OVERLAP"); k.no_prof_overlap = on("MCX_NO_PROF_OVERLAP"); k.no_tier1_grow = on("MCX_NO_TIER1_GROW");
    k.cluster_in_line = on("MCX_CLUSTER_IN_LINE"); k.cluster_split = on("MCX_CLUSTER_SPLIT");
    k.cluster_mem = on("MCX_CLUSTER_MEM"); // (A/B tests, measurements: k_cluster sorts and clusters in the pair record, as the other tiers do)
    // A batch packed on its way in (mcx_stream_submit_packed; MCX_PREPACK=1) pays on runtimes whose copies in and out overlap: 16.2-16.3 against 16.7-16.8 ms per
    // step on ROCm 7.2's; on one that puts both directions on one SDMA engine (HIP 7.0, what torch's wheel carries) the copy in ends late and the longer chain
    // behind it reaches into the next step: 17.5 against 17.1.  Off unless asked for: one fuzz round in 480 of the CLI with it on did not come out
    // identical to the oracle's (a difference or a failed command — the run kept only its count) and did not come back in 780 repeats; until that round is
    // understood the step packs its own reads.
    k.no_prepack = !on("MCX_PREPACK");
    if (const char *e = getenv("MCX_SEED_FM_BUDGET")) k.seed_fm_budget = std::max(1, atoi(e));
    if (const char *e = getenv("MCX_BUILD_WAVE_LIMIT")) k.build_wave_limit = atoi(e); // (tests: the bound sum from which k_build_wave hands a pair to one lane)
    if (const char *e = getenv("MCX_ORDER_MIN")) k.order_min = (uint32_t)std::max(1, atoi(e)); // (tests: small batches through k_simple and the order too)
    return k;
}

constexpr uint32_t kPoutSel = 1u << 16; // pair outcomes gathered per copy (run_selection)
static MultiOut multi_out(const mcx_ctx *c)
{
    MultiOut m;
    m.recs = c->mx.d_pool; m.cig = c->mx.d_pool_cig; m.cnt = c->mx.d_cnt; m.rec_cap = c->mx.rec_cap; m.word_cap = c->mx.word_cap; m.ref = c->mx.d_ref;
    return m;
}

extern "C" void mcx_opts_default(mcx_opts *o)
{
    o->alg = 0; o->max_pos_diff = 30; o->max_mismatch_rate = 0.05f; o->max_read_len = 256; o->max_batch_reads = 1 << 20;
}

static Caps tier0_caps()
{
    // (hit_seed above OCC_Thr: one seed at the occurrence limit plus the read's other seeds still fit)
    Caps c; c.hit_cap = 88; c.hit_seed = 56; c.cand_cap = 24; c.cand_seed = 12; // (rescue adds at most one candidate per candidate of the mate)
    c.frag_cap = 96; c.ops_cap = 2048; c.job_cap = 32;
    c.cig_cap = MCX_CIGAR_STRIDE; c.kmer_cap = 2048;
    return c;
}
static Caps tier1_caps(int rlen_max)
{
    Caps c;
    int seeds = rlen_max / (kMinSeedLength + 1) + 1;
    c.hit_cap = seeds * kOccThr + rlen_max / 8 + 16;
    c.cand_cap = c.hit_cap;
    c.hit_seed = c.hit_cap; c.cand_seed = c.cand_cap; // (hard bounds already count what the rescue can add)
    c.frag_cap = 7 * c.hit_cap / 2 + 16; // (k_build_wave places a candidate's fragments by their bound, 2 seeds + 2: a sixth more room than 3 per hit)
    c.ops_cap = 96 * 1024; c.job_cap = 2048;
    c.cig_cap = MCX_CIGAR_STRIDE; c.kmer_cap = 4096;
    return c;
}

std::atomic<size_t> g_dmalloc_bytes(0);

static int ctx_fill(mcx_ctx *c, const mcx_index *idx, const mcx_opts &o);

extern "C" int mcx_ctx_create(const mcx_index *idx, const mcx_opts *opts, mcx_ctx **out)
{
    if (!idx || !out) return fail(MCX_ERR_ARG, "mcx_ctx_create: null argument");
    mcx_opts o;
    if (opts) o = *opts; else mcx_opts_default(&o);
    if (o.max_read_len < 32) o.max_read_len = 32;
    if (o.max_read_len > 1000) return fail(MCX_ERR_UNSUPPORTED, "max_read_len > 1000 is not supported");
    if (o.max_batch_reads < 2) o.max_batch_reads = 2;
    mcx_ctx *c = new mcx_ctx();
    c->kn = knobs_read();
    const size_t before = g_dmalloc_bytes.load();
    const int rc = ctx_fill(c, idx, o);
    if (c->kn.timing) fprintf(stderr, "[mcx_ctx_create] %.2f GB of HBM for batches of %lld reads of up to %d bases\n", (double)(g_dmalloc_bytes.load() - before) / 1e9, (long long)o.max_batch_reads, (int)o.max_read_len);
    if (rc) { mcx_ctx_free(c); return rc; } // (every pointer of the context starts null: a caller that retries with a smaller batch finds the HBM free again)
    idx->n_ctx++; c->counted = true;
    *out = c;
    return 0;
}

// the window lists of mate rescue for a set of pass resources that lists up to `pairs` pairs
static int rescue_alloc(PassRes &t, uint64_t pairs, bool large)
{
    int rc;
    // (the large tier's pairs have hundreds of candidates: many more windows per pair than tier 0's, whose lists stay short)
    t.rtask_cap = large ? 1u << 22 : (uint32_t)std::min<uint64_t>(std::max<uint64_t>(pairs, 1u << 18), 1u << 21);
    if (const char *e = getenv("MCX_RESCUE_TASK_CAP")) t.rtask_cap = (uint32_t)std::max(16, atoi(e)); // (tests: make the list run over)
    t.rseed_cap = large ? t.rtask_cap * 4 : t.rtask_cap; // seeds are kept only of windows that beat the mate's best candidate (a few per pair; a heavy pair's windows mostly do)
    if ((rc = dmalloc(&t.d_rtasks, t.rtask_cap))) return rc;
    if ((rc = dmalloc(&t.d_rres, t.rtask_cap))) return rc;
    if ((rc = dmalloc(&t.d_rseeds, (size_t)t.rseed_cap))) return rc;
    if ((rc = dmalloc(&t.d_rplans, pairs))) return rc;
    if ((rc = dmalloc(&t.d_rescue_n, pairs))) return rc;
    return 0;
}

// what differs between the sets of pass resources (PassRes): tier 0's, and the side sets beside it (the large tier's, the late pairs')
struct PassSizes {
    bool tier0 = false;              // tier 0's stream is the context's: a blocking stream at default priority (callers' copies on the null stream order against it)
    int priority = 0;                // a side set's streams
    int n_side = 0;                  // side streams for the DP lists
    uint64_t pairs = 0, sel_cap = 0; // pairs a pass lists at a time (rescue lists); selections (ids, estimates, overflow list)
    bool rescue_large = false;       // the large tier's window lists (rescue_alloc)
    uint32_t task_cap = 0;           // SA tasks (0: no list — a side set runs only with every suffix-array entry resident)
    uint32_t job_cap[kDpClasses] = {0, 0, 0, 0, 0, 0};
    uint64_t dp_stride[3] = {0, 0, 0}; uint32_t dp_blocks[3] = {0, 0, 0}, dp_lane_blocks = 0;
    uint32_t h_cnt_words = CNT_COPY;
};

static PassSizes tier0_sizes(const mcx_ctx *c)
{
    PassSizes z;
    z.tier0 = true; z.n_side = 2;
    z.pairs = z.sel_cap = c->max_reads;
    z.task_cap = (uint32_t)std::min<uint64_t>(c->max_reads * 24, 0x7fffffffu);
    for (int k = 0; k < kDpClasses; k++) {
        z.job_cap[k] = (uint32_t)std::min<uint64_t>(c->max_reads * ((k == 0 || k == 4) ? 4 : ((k == 1 || k == 5) ? 2 : 1)) + 1024, 0x7fffffffu);
        if (const char *e = getenv("MCX_JOB_CAP")) z.job_cap[k] = std::min<uint32_t>(z.job_cap[k], (uint32_t)std::max(1024, atoi(e))); // (tests: make the lists run over)
    }
    // DP traceback spill per block: 4 KB of sequences + (qlen + tlen - 1) * tlen direction bytes
    // (the two grouped classes: a wavefront's stretch holds the strings and traceback bytes of a group of problems — k_dp_group —,
    //  at least those of the class's largest one)
    const uint64_t spill[3] = {(uint64_t)512 << 10, (uint64_t)1 << 20, kDpSpillSeq + (uint64_t)(2048 + 1024) * 1024};
    uint32_t blocks[3] = {8192, 4096, 512}; // (the 65-256-column class at 2048 or 8192 wavefronts: the same DP stage, 3.3-3.8 ms)
    if (const char *e = getenv("MCX_DP_BLOCKS1")) blocks[1] = (uint32_t)std::max(256, atoi(e)); // (experiments; a size that was asked for stays: dp_scratch_grow)
    for (int k = 0; k < 3; k++) { z.dp_stride[k] = spill[k]; z.dp_blocks[k] = blocks[k]; }
    z.dp_lane_blocks = 4096;
    z.h_cnt_words = CNT_COPY + 8; // (+8: the seeding statistics of a batch, on their way to batch_close)
    return z;
}

// a side set: work lists for `pairs` pairs at a time, selections of up to `sel_cap`
static PassSizes side_sizes(const mcx_ctx *c, uint64_t pairs, uint64_t sel_cap, int priority)
{
    PassSizes z;
    z.priority = priority;
    // side streams for the DP lists only where lists are long enough to share the chip: a stream that exists lands on one of the
    // runtime's few hardware queues, and a queue that waits for an event holds up every stream folded onto it (the late pairs' pass
    // once sat 4 ms behind the large tier's DP fork that way)
    z.n_side = pairs >= 4096 ? 2 : 0;
    z.pairs = pairs; z.sel_cap = sel_cap; z.rescue_large = pairs >= 4096;
    for (int k = 0; k < kDpClasses; k++) z.job_cap[k] = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(pairs * 16, 1u << 20), c->t0.job_cap[k]);
    const uint32_t blocks1[3] = {pairs >= 4096 ? 2048u : 256u, pairs >= 4096 ? 2048u : 128u, 256};
    for (int k = 0; k < 3; k++) { z.dp_stride[k] = c->t0.dp_stride[k]; z.dp_blocks[k] = blocks1[k]; }
    z.dp_lane_blocks = pairs >= 4096 ? 2048u : 256u;
    return z;
}

static int passres_alloc(PassRes &t, const PassSizes &z)
{
    int rc;
    if (z.tier0) HIP_TRY(hipStreamCreate(&t.stream));
    else HIP_TRY(hipStreamCreateWithPriority(&t.stream, hipStreamNonBlocking, z.priority));
    for (int k = 0; k < z.n_side; k++) {
        if (z.tier0) HIP_TRY(hipStreamCreateWithFlags(&t.dp_stream[k], hipStreamNonBlocking));
        else HIP_TRY(hipStreamCreateWithPriority(&t.dp_stream[k], hipStreamNonBlocking, z.priority));
        HIP_TRY(hipEventCreateWithFlags(&t.dp_join[k], hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&t.dp_fork, hipEventDisableTiming));
    if (z.tier0 && z.n_side) for (hipEvent_t *e : {&t.ev_seeded, &t.ev_order_h, &t.ev_heavy}) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    for (auto &e : t.ev) HIP_TRY(hipEventCreate(&e));
    t.task_cap = z.task_cap;
    if (t.task_cap && (rc = dmalloc(&t.d_tasks, t.task_cap))) return rc;
    for (int k = 0; k < kDpClasses; k++) {
        t.job_cap[k] = z.job_cap[k];
        if ((rc = dmalloc(&t.d_jobs[k], t.job_cap[k]))) return rc;
    }
    if ((rc = dmalloc(&t.d_cnt, CNT_ALL))) return rc;
    HIP_TRY(hipHostMalloc((void **)&t.h_cnt, z.h_cnt_words * sizeof(uint32_t)));
    t.rescue_cap = (uint32_t)z.pairs;
    if ((rc = dmalloc(&t.d_rescue, t.rescue_cap))) return rc;
    if ((rc = rescue_alloc(t, z.pairs, z.rescue_large))) return rc;
    for (int k = 0; k < 3; k++) {
        t.dp_stride[k] = z.dp_stride[k]; t.dp_blocks[k] = z.dp_blocks[k];
        if ((rc = dmalloc(&t.d_dp_scratch[k], (size_t)t.dp_stride[k] * t.dp_blocks[k]))) return rc;
    }
    t.dp_lane_blocks = z.dp_lane_blocks;
    if ((rc = dmalloc(&t.d_dp_lane, (size_t)(lane_short_words(0) + lane_short_words(1) + lane_short_words(2)) * t.dp_lane_blocks))) return rc;
    for (int k = 0; k < 2; k++) if ((rc = dmalloc(&t.d_dp_order[k], t.job_cap[1 + k]))) return rc;
    t.ov_cap = (uint32_t)z.sel_cap;
    if ((rc = dmalloc(&t.d_ov, t.ov_cap))) return rc;
    if ((rc = dmalloc(&t.d_sel_ids, z.sel_cap))) return rc;
    if ((rc = dmalloc(&t.d_est, z.sel_cap))) return rc;
    return 0;
}

// (d_kscratch is the context's)
static void passres_free(PassRes &t)
{
    void *q[] = {t.d_cnt, t.d_tasks, t.d_jobs[0], t.d_jobs[1], t.d_jobs[2], t.d_jobs[3], t.d_jobs[4], t.d_jobs[5], t.d_rescue, t.d_dp_scratch[0], t.d_dp_scratch[1],
                 t.d_dp_scratch[2], t.d_ov, t.d_sel_ids, t.d_est, t.d_rtasks, t.d_rres, t.d_rseeds, t.d_rplans, t.d_rescue_n, t.d_dp_lane, t.d_dp_order[0], t.d_dp_order[1]};
    for (void *x : q) if (x) (void)hipFree(x);
    if (t.h_cnt) (void)hipHostFree(t.h_cnt);
    for (auto &e : t.ev) if (e) (void)hipEventDestroy(e);
    for (int k = 0; k < 5; k++) { if (t.dp_stream[k]) (void)hipStreamDestroy(t.dp_stream[k]); if (t.dp_join[k]) (void)hipEventDestroy(t.dp_join[k]); }
    if (t.dp_fork) (void)hipEventDestroy(t.dp_fork);
    for (hipEvent_t e : {t.ev_seeded, t.ev_order_h, t.ev_heavy}) if (e) (void)hipEventDestroy(e);
    if (t.stream) (void)hipStreamDestroy(t.stream);
}

static int ctx_fill(mcx_ctx *c, const mcx_index *idx, const mcx_opts &o)
{
    c->idx = idx; c->opts = o;
    c->pm.max_pos_diff = o.max_pos_diff; c->pm.max_mm_rate = o.max_mismatch_rate; c->pm.use_nw = o.alg == 0; c->pm.paired = 1;
    c->rlen_max = o.max_read_len;
    c->max_reads = (uint64_t)o.max_batch_reads;
    c->max_bases = c->max_reads * (uint64_t)c->rlen_max;
    HIP_TRY(hipSetDevice(idx->device));
    for (auto &e : c->ev_pack) HIP_TRY(hipEventCreate(&e));
    int rc = 0;
    c->tier[0].caps = tier0_caps(); c->light_fit = light_pairs_fit(c->tier[0].caps); c->regs_fit = packed_hits_fit(idx->view.G2, c->rlen_max); c->tier[0].lay = make_layout(c->tier[0].caps); c->tier[0].max_pairs = (uint32_t)c->max_reads;
    c->tier[1].caps = tier1_caps(c->rlen_max); c->tier[1].lay = make_layout(c->tier[1].caps);
    // (the heavy pairs of a batch in as few passes as possible — a pass is bound by its slowest pair, not by its size, and passes follow
    //  one another: BASELINE config 5 sends 4.5 % of its pairs here, five passes of 36 k pairs with 8 GB of records — with room in
    //  proportion to the batch: 3 KB per read, 2-24 GB (MCX_TIER1_GB overrides))
    uint64_t t1_bytes = std::min<uint64_t>(std::max<uint64_t>(c->max_reads * 3072, (uint64_t)2 << 30), (uint64_t)24 << 30);
    const uint64_t t1_limit = std::min<uint64_t>(c->max_reads, 262144);
    if (const char *e = getenv("MCX_TIER1_GB")) t1_bytes = (uint64_t)std::max(1, atoi(e)) << 30;
    else if (const char *e2 = getenv("MCX_TIER1_START_GB")) t1_bytes = (uint64_t)(std::max(0.05, atof(e2)) * (double)(1 << 30)); // (tests: a small start that may grow)
    c->tier[1].max_pairs = (uint32_t)std::max<uint64_t>(1024, std::min<uint64_t>(t1_limit, t1_bytes / (uint64_t)c->tier[1].lay.stride));
    // (a batch whose heavy pairs do not fit these records in one pass makes them grow, HBM permitting: tier1_grow().  A size that was asked for stays)
    c->tier[1].grow_to = getenv("MCX_TIER1_GB") || c->kn.no_tier1_grow ? 0u : (uint32_t)std::max<uint64_t>(t1_limit, c->tier[1].max_pairs);
    // (tier 0's records are allocated by the first batch: a paired batch of max_reads reads is max_reads / 2 pairs, and at 8 KB a
    //  record the other half is 33 GB at 8 M reads — only single-end batches need a record per read)
    c->tier[0].max_pairs = 0;
    if ((rc = dmalloc(&c->tier[1].state, (size_t)c->tier[1].lay.stride * c->tier[1].max_pairs))) return rc;
    if ((rc = passres_alloc(c->t0, tier0_sizes(c)))) return rc;
    if ((rc = dmalloc(&c->d_kscratch, 3 * (size_t)kRescueBlocks * kRescueScratchWords))) return rc; // (one part per set of pass resources)
    c->t0.d_kscratch = c->d_kscratch;
    if ((rc = dmalloc(&c->d_read_ext, c->max_reads))) return rc;
    if ((rc = dmalloc(&c->d_read_blocks, c->max_reads))) return rc;
    if ((rc = dmalloc(&c->d_batch_flags, 4))) return rc;
    HIP_TRY(hipMemset(c->d_batch_flags, 0, 4 * sizeof(uint32_t)));
    c->wpad = (packed_words(c->rlen_max) + 3) & ~3;
    if ((rc = dmalloc(&c->d_packed, c->max_reads * (uint64_t)c->wpad))) return rc;
    if ((rc = dmalloc(&c->d_pout, c->max_reads))) return rc;
    if ((rc = dmalloc(&c->d_pout_sel, kPoutSel))) return rc;
    if ((rc = dmalloc(&c->d_order, c->max_reads))) return rc;
    if ((rc = dmalloc(&c->d_done, c->max_reads))) return rc;
    c->sl_cap = (uint32_t)std::max<uint64_t>(c->max_reads / 4, 1024);
    if ((rc = dmalloc(&c->d_sl_pairs, c->sl_cap))) return rc;
    if ((rc = dmalloc(&c->d_sl_list, (uint64_t)c->sl_cap * kSimpleJobs))) return rc;
    if ((rc = dmalloc(&c->d_sl_jobs, (uint64_t)c->sl_cap * kSimpleJobs))) return rc;
    if ((rc = dmalloc(&c->d_sl_res, (uint64_t)c->sl_cap * kSimpleJobs))) return rc;
    // EvaluateMAPQ (SamReport.cpp:86-101) tabulated on the host so that the double-precision
    // log() is the host libm's, exactly as in the reference
    c->mapq_rows = c->rlen_max + 64;
    std::vector<uint8_t> tab((size_t)c->mapq_rows * 6, 0);
    for (int s = 1; s < c->mapq_rows; s++)
        for (int d = 1; d <= 5 && d < s; d++) {
            int sub = s - d;
            int q = (int)(30 * (1 - (float)(s - sub) / s) * log(s) + 0.4999);
            tab[(size_t)s * 6 + d] = (uint8_t)(q > 60 ? 60 : q);
        }
    if ((rc = dmalloc(&c->d_mapq, tab.size()))) return rc;
    HIP_TRY(hipMemcpy(c->d_mapq, tab.data(), tab.size(), hipMemcpyHostToDevice));
    // the large tier's own stream, counters and lists: with them it maps the heavy pairs of a pass while the pass goes on
    // (without the full suffix array it would also need an SA task list of its own: then the tiers run one after the other)
    if (idx->view.sa_full && !c->kn.no_tier_overlap) {
        // its kernels are as long as their slowest pair, and the batch waits for them: their waves go first
        // (human-like bench genome: 40.0 -> 37.4 ms per step)
        int pr_lo = 0, pr_hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi));
        if ((rc = passres_alloc(c->t1, side_sizes(c, std::max(c->tier[1].max_pairs, c->tier[1].grow_to), c->max_reads, pr_hi)))) return rc; // (lists for as many pairs as the records may grow to)
        c->t1.d_kscratch = c->d_kscratch + (size_t)kRescueBlocks * kRescueScratchWords;
        HIP_TRY(hipEventCreate(&c->ev_clustered));
        c->overlap_tiers = true;
        {
            void *h = nullptr, *d = nullptr;
            if (hipHostMalloc(&h, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&d, h, 0) == hipSuccess) { c->h_early = (volatile uint32_t *)h; c->d_early = (uint32_t *)d; }
            else { (void)hipGetLastError(); if (h) (void)hipHostFree(h); } // (without it: the copies behind the kernel, as before)
        }
        // and a small third set for the pairs that run over after clustering: they go through the large tier while the pass's
        // DP and finish stages run, in the last kLateRoom records of the tier, instead of in a pass of their own after it
        if (c->tier[1].max_pairs >= 4 * kLateRoom && !c->kn.no_late_overlap) {
            if ((rc = passres_alloc(c->t2, side_sizes(c, kLateRoom, kLateRoom, pr_hi)))) return rc;
            c->t2.d_kscratch = c->d_kscratch + 2 * (size_t)kRescueBlocks * kRescueScratchWords;
            HIP_TRY(hipEventCreateWithFlags(&c->ev_built, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&c->ev_late_done, hipEventDisableTiming));
            c->overlap_late = true;
        }
    }
    return 0;
}

extern "C" void mcx_ctx_free(mcx_ctx *c)
{
    if (!c) return;
    if (c->counted && c->idx && --c->idx->n_ctx == 0 && c->idx->orphan.load()) delete c->idx; // (the index was freed first: its host object waited for this)
    if (c->files_state && c->files_drop) c->files_drop(c->files_state);
    if (c->sam_state && c->sam_drop) c->sam_drop(c->sam_state);
    void *p[] = {c->tier[0].state, c->tier[1].state, c->d_kscratch, c->d_read_ext, c->d_read_blocks, c->d_pout, c->d_mapq,
                 c->d_bases, c->d_off, c->d_recs, c->d_cig, c->d_detail, c->d_keys[0], c->d_keys[1], c->d_admit, c->d_sort_tmp, c->d_sparse, c->d_pout_sel, c->d_order, c->d_done, c->d_sl_pairs, c->d_sl_list, c->d_sl_jobs, c->d_sl_res, c->d_packed, c->d_batch_flags, c->d_scan_tmp, c->d_prof_match, c->d_prof_items};
    for (void *q : p) if (q) (void)hipFree(q);
    if (c->h_keys) (void)hipHostFree(c->h_keys);
    if (c->h_sparse_pin) (void)hipHostFree(c->h_sparse_pin);
    if (c->arch.d) (void)hipFree(c->arch.d);
    if (c->arch_ev.d) (void)hipFree(c->arch_ev.d);
    passres_free(c->t1); passres_free(c->t2);
    for (hipEvent_t e : {c->ev_clustered, c->ev_built, c->ev_late_done, c->tail.ev[0], c->tail.ev[1]}) if (e) (void)hipEventDestroy(e);
    {
        auto &L = c->later;
        if (L.stream) (void)hipStreamSynchronize(L.stream);
        for (void *q : {(void *)L.d_detail_alt, (void *)L.d_admit_alt, (void *)L.d_keep_bases, (void *)L.d_keep_off, (void *)L.d_keep_bases_alt, (void *)L.d_keep_off_alt, (void *)L.d_cnt, (void *)L.d_ev}) if (q) (void)hipFree(q);
        if (L.h_cnt) (void)hipHostFree(L.h_cnt);
        for (hipEvent_t e : {L.go, L.done, L.kept, L.begun}) if (e) (void)hipEventDestroy(e);
        if (L.stream) (void)hipStreamDestroy(L.stream);
        if (L.keep_stream) (void)hipStreamDestroy(L.keep_stream);
    }
    if (c->h_early) (void)hipHostFree((void *)c->h_early);
    for (void *q : {(void *)c->mx.d_pool, (void *)c->mx.d_pool_cig, (void *)c->mx.d_cnt, (void *)c->mx.d_ref, (void *)c->mx.d_counts, (void *)c->mx.d_index,
                    (void *)c->mx.d_windex, (void *)c->mx.d_out, (void *)c->mx.d_out_cig, c->mx.d_tmp}) if (q) (void)hipFree(q);
    if (c->tail.d) (void)hipFree(c->tail.d);
    if (c->tail.h) (void)hipHostFree(c->tail.h);
    for (auto &sl : c->slot) {
        void *q[] = {sl.d_bases, sl.d_off, sl.d_recs, sl.d_cig, sl.d_codes, sl.d_len, sl.d_odd, sl.d_err, sl.d_recs32, sl.d_prepack, sl.d_any_n,
                     sl.mx.d_index, sl.mx.d_cig, sl.mx.d_recs};
        for (void *x : q) if (x) (void)hipFree(x);
        mcx_pinned_free(sl.mx.h_index); mcx_pinned_free(sl.mx.h_cig); mcx_pinned_free(sl.mx.h_recs);
        if (sl.h_err) (void)hipHostFree(sl.h_err);
        for (hipEvent_t e : {sl.in_ready, sl.mapped, sl.out_done}) if (e) (void)hipEventDestroy(e);
    }
    if (c->h2d_stream) (void)hipStreamDestroy(c->h2d_stream);
    if (c->d2h_stream) (void)hipStreamDestroy(c->d2h_stream);
    passres_free(c->t0);
    for (auto &e : c->ev_pack) if (e) (void)hipEventDestroy(e);
    delete c;
}

static Ctx make_ctx(const mcx_ctx *c, int tier, int paired)
{
    Ctx cx;
    cx.ix = c->idx->view; cx.pm = c->pm; cx.pm.paired = paired;
    if (c->kn.seed_one_base) cx.ix.rank2 = nullptr; // (experiments, tests: the walk one base per step although the pair records are there)
    cx.caps = c->tier[tier].caps; cx.lay = c->tier[tier].lay; cx.state = c->tier[tier].state;
    cx.mapq_tab = c->d_mapq; cx.mapq_rows = c->mapq_rows; cx.dp_summary = 1;
    cx.detail = c->prof_planes ? c->d_detail : nullptr; cx.dlay = c->dlay;
    cx.cig_pool = c->run.cig; cx.cig_pool_n = c->d_batch_flags; cx.cig_pool_cap = c->run.cig_cap;
    cx.packed = c->packed_now ? c->packed_now : c->d_packed; cx.wpad = c->packed_now ? c->wpad_now : c->wpad; cx.read_ext = c->d_read_ext; cx.seed_pool = nullptr;
    return cx;
}

// ---------------------------------------------------------------------------------------------
// one tier over a selection of pairs
// ---------------------------------------------------------------------------------------------
struct StageMs { float seed, sa, cluster, rescue, build, dp, finish; };

constexpr int kListOverflow = 1; // (internal) a work list of run_pairs was too short for the selection

// The large tier's records grow when a batch sends it more pairs than one pass holds.  Its passes follow one another, each as long as its slowest pair,
// and only the first runs beside tier 0: BASELINE config 5 (185 k heavy pairs of 4 M, 260 KB of records each) took two passes of 99 k and 86 k with the
// 24 GB the context starts with, the second one alone on the chip for 17 ms after tier 0 had finished — one pass of 185 k: 117.2 -> 108.5 ms a step.
// Called between passes (nothing of the tier is under way: every earlier pass was waited for by tier1_pass_end), with the batch's tier-0 kernels queued:
// hipFree waits for the device, once or twice in a run.  Grows only into HBM that is free beyond kGrowKeep, so that what a caller allocates later (a
// profile's planes are attached before the first batch; a second set of detail records is not) still finds room; never shrinks.
constexpr uint64_t kGrowKeep = (uint64_t)16 << 30;
static int tier1_grow(mcx_ctx *c, uint64_t pairs_wanted)
{
    Tier &t = c->tier[1];
    if (!t.grow_to || pairs_wanted <= t.max_pairs || t.max_pairs >= t.grow_to) return 0;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (const char *e = getenv("MCX_HBM_CAP_GB")) { // (tests: as if the device had this much)
        const uint64_t cap = (uint64_t)std::max(1, atoi(e)) << 30, used = total_b - free_b;
        free_b = cap > used ? cap - used : 0;
    }
    const uint64_t have = (uint64_t)t.lay.stride * t.max_pairs;
    uint64_t want = std::min<uint64_t>(t.grow_to, pairs_wanted + pairs_wanted / 8 + 1024); // (an eighth more: the next batch's count differs a little)
    const uint64_t room = free_b + have > kGrowKeep ? (free_b + have - kGrowKeep) / (uint64_t)t.lay.stride : 0;
    want = std::min(want, room);
    if (want < pairs_wanted || want <= t.max_pairs) return 0; // (not in one pass anyway: what is there stays)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipFree(t.state)); t.state = nullptr;
    uint8_t *p = nullptr;
    if (hipMalloc((void **)&p, (size_t)t.lay.stride * want) != hipSuccess) {
        (void)hipGetLastError();
        if (hipMalloc((void **)&p, (size_t)have) != hipSuccess) { (void)hipGetLastError(); t.max_pairs = 0; return fail(MCX_ERR_DEVICE, "the large tier's records: out of device memory"); }
        t.state = p; t.grow_to = 0;
        return 0;
    }
    if (c->kn.timing || getenv("MCX_ALLOC_LOG")) fprintf(stderr, "[mcx] the large tier's records grow from %u to %llu pairs (%.1f -> %.1f GB): %llu heavy pairs in this batch\n",
                                                       t.max_pairs, (unsigned long long)want, (double)have / 1e9, (double)t.lay.stride * want / 1e9, (unsigned long long)pairs_wanted);
    g_dmalloc_bytes += (size_t)t.lay.stride * want - have;
    t.state = p; t.max_pairs = (uint32_t)want;
    return 0;
}

// The scratch of the 65-256-column list grows when a batch fills it.  A wavefront of k_dp_lane2 keeps the traceback bits of its 128 problems in a stretch
// sized for the list's largest shape (2.2 MB at 250 bp), and the 4 GB a context starts with hold 1920 of them — fewer than two per SIMD, and this list's
// kernel is the DP stage's last to end at config 5 (1.3 M problems: 106.8 / 109.6 ms a step with 4 GB, 100.8 / 102.9 with 8).  Called from batch_close()
// with the batch's own kernels through; into HBM that is free beyond kGrowKeep, at most 12 GB, once.
static int dp_scratch_grow(mcx_ctx *c, uint32_t list_len)
{
    if (c->dp_grown || getenv("MCX_DP_BLOCKS1") || c->kn.no_tier1_grow) return 0;
    const bool nw = c->pm.use_nw != 0;
    const uint64_t w2 = lane_stride_words(nw, c->rlen_max, 16) * 4; // bytes a wavefront's stretch takes
    const uint64_t have = c->t0.dp_stride[1] * c->t0.dp_blocks[1];
    uint64_t enough = 2 * 128 * (have / w2); // (fewer than two groups per wavefront there is room for: short enough)
    if (const char *e = getenv("MCX_DP_GROW_MIN")) enough = (uint64_t)std::max(0, atoi(e)); // (tests)
    if ((uint64_t)list_len <= enough) return 0;
    c->dp_grown = true; // (one attempt)
    const uint64_t want_bytes = std::min<uint64_t>(4096 * w2, (uint64_t)12 << 30);
    const uint32_t want = (uint32_t)((want_bytes + c->t0.dp_stride[1] - 1) / c->t0.dp_stride[1]);
    if (want <= c->t0.dp_blocks[1]) return 0;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (const char *e = getenv("MCX_HBM_CAP_GB")) { const uint64_t cap = (uint64_t)std::max(1, atoi(e)) << 30, used = total_b - free_b; free_b = cap > used ? cap - used : 0; }
    if (free_b + have < (uint64_t)want * c->t0.dp_stride[1] + kGrowKeep) return 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipFree(c->t0.d_dp_scratch[1])); c->t0.d_dp_scratch[1] = nullptr;
    uint8_t *p = nullptr;
    uint32_t got = want;
    if (hipMalloc((void **)&p, (size_t)want * c->t0.dp_stride[1]) != hipSuccess) {
        (void)hipGetLastError();
        got = c->t0.dp_blocks[1];
        if (hipMalloc((void **)&p, (size_t)have) != hipSuccess) { (void)hipGetLastError(); return fail(MCX_ERR_DEVICE, "the DP lists' scratch: out of device memory"); }
    }
    if (got != c->t0.dp_blocks[1] && (c->kn.timing || getenv("MCX_ALLOC_LOG")))
        fprintf(stderr, "[mcx] the 65-256-column DP list's scratch grows from %.1f to %.1f GB: %u problems in this batch\n", (double)have / 1e9, (double)got * c->t0.dp_stride[1] / 1e9, list_len);
    g_dmalloc_bytes += (size_t)got * c->t0.dp_stride[1] - have;
    c->t0.d_dp_scratch[1] = p; c->t0.dp_blocks[1] = got;
    return 0;
}

static int tier1_error(mcx_ctx *c, const PassRes &R);
static int tier1_pass_end(mcx_ctx *c, const PassRes &T, uint32_t m, mcx_stats *t1, mcx_stats *stats, int e);

// One tier over a selection of pairs.  early (tier 0 only): the pairs that run over the tier's capacities while clustering
// are listed on the device; once the rest of the pass is queued, the large tier maps them on its own stream — its kernels
// are bound by their slowest pair, not by the chip, so they hide behind the pass instead of following it.
// state_off: the pass's pair records start at record state_off of the tier.  queue_only: the kernels are queued on R's stream
// and that is all — the caller goes on and calls pass_finish() for the pass later (*queued = its timing events).
static int pass_finish(mcx_ctx *c, int tier, const PassRes &R, uint32_t n_sel, mcx_stats *stats, bool timing, int e);
static int queue_batch_tail(mcx_ctx *c);
static int tail_reserve(mcx_ctx *c);

static int run_pairs(mcx_ctx *c, int tier, const PassRes &R, const ReadBatch &rb, int paired, PairSel sel, AlnRec *d_recs,
                     uint32_t *d_cig, mcx_stats *stats, bool timing, bool early = false, uint32_t state_off = 0, int *queued = nullptr, bool hits_from_tier0 = false, bool no_n_reads = false)
{
    if (sel.n == 0) return 0;
    hipStream_t s = R.stream;
    const Knobs &kn = c->kn;
    Ctx cx = make_ctx(c, tier, paired);
    cx.state += (size_t)state_off * (size_t)cx.lay.stride;
    cx.seed_pool = R.d_rseeds;
    const int nr = paired ? 2 : 1;
    early = early && tier == 0 && c->overlap_tiers;
    HIP_TRY(hipMemsetAsync(R.d_cnt, 0, CNT_ALL * sizeof(uint32_t), s)); // (the pass's counters, the class counts of its order, the bucket counts of its DP lists)
    SeedOut so; so.tasks = R.d_tasks; so.n_tasks = R.d_cnt + CNT_TASKS; so.task_cap = R.task_cap;
    so.read_ext = c->d_read_ext; so.read_blocks = c->d_read_blocks;
    so.packed = c->packed_now ? c->packed_now : c->d_packed; so.wpad = c->packed_now ? c->wpad_now : c->wpad; so.queue = R.d_cnt + CNT_QUEUE;
    so.src_state = nullptr; so.src_lay = c->tier[0].lay; so.src_caps = c->tier[0].caps;
    if (hits_from_tier0 && tier == 1 && cx.ix.sa_full && !kn.late_reseed) so.src_state = c->tier[0].state;
    RescueList rl; rl.ids = R.d_rescue; rl.n = R.d_cnt + CNT_RESCUE; rl.cap = R.rescue_cap;
    EarlyList el; el.ids = nullptr; el.est = nullptr; el.n = R.d_cnt + CNT_EARLY; el.cap = 0; el.n_hits = R.d_cnt + CNT_EARLY_HITS;
    if (early) { el.ids = c->t1.d_sel_ids; el.est = c->t1.d_est; el.cap = (uint32_t)c->max_reads; }
    const bool late = early && c->overlap_late;
    EarlyList ll; ll.ids = nullptr; ll.est = nullptr; ll.n = R.d_cnt + CNT_LATE; ll.cap = 0; ll.n_hits = R.d_cnt + CNT_EARLY_HITS;
    if (late) { ll.ids = c->t2.d_sel_ids; ll.est = c->t2.d_est; ll.cap = kLateRoom; }
    JobSinks sinks;
    for (int k = 0; k < kDpClasses; k++) { sinks.s[k].jobs = R.d_jobs[k]; sinks.s[k].count = R.d_cnt + CNT_JOB0 + k * kCntPad; sinks.s[k].cap = R.job_cap[k]; }
    sinks.unsupported = R.d_cnt + CNT_UNSUP;
    const unsigned pb = (sel.n + 255) / 256;
    int e = 0, rc2 = 0;
    if (timing) HIP_TRY(hipEventRecord(R.ev[e++], s));
    {
        // LDS for the packed reads: words per lane for the longest read x lanes; narrower blocks for long reads
        const int pkw = packed_words(c->rlen_max);
        const int threads = pkw * 256 * 4 <= 48 * 1024 ? 256 : (pkw * 128 * 4 <= 48 * 1024 ? 128 : 64);
        const int rpl = seed_reads_per_lane((uint64_t)sel.n * nr);
        const unsigned blocks_s = std::min<unsigned>((sel.n * nr + threads * rpl - 1) / (threads * rpl), 4096u); // (the queue feeds whatever grid runs)
        k_seed<<<blocks_s, threads, (size_t)pkw * threads * 4, s>>>(cx, rb, sel, so, pkw, rpl, kn.seed_fm_budget);
#ifdef MCX_SEED_STATS
        if (tier == 0 && sel.n > 100000) {
            unsigned long long h[2][24];
            (void)hipStreamSynchronize(s);
            (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_seed_hist), sizeof h);
            fprintf(stderr, "[k_seed] index blocks per read, by bit length of the count: reads");
            for (int k = 0; k < 12; k++) fprintf(stderr, " %llu", h[0][k]);
            fprintf(stderr, " | blocks");
            for (int k = 0; k < 12; k++) fprintf(stderr, " %llu", h[1][k]);
            fprintf(stderr, "\n");
            memset(h, 0, sizeof h);
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_seed_hist), h, sizeof h);
        }
#endif
    }
    if (timing) HIP_TRY(hipEventRecord(R.ev[e++], s));
    if (R.d_tasks) k_sa<<<4096, 256, 0, s>>>(cx, so, paired, R.d_cnt + CNT_LF);
    if (timing) HIP_TRY(hipEventRecord(R.ev[e++], s));
    // the pairs in the order of their weight (k_order_*): worth two small passes when the pass is a large one
    const uint32_t *order = nullptr, *order_cnt = nullptr;
    bool split = false; // (time stamps 10 and 11 were taken: the straight-line path's and the order's share of the stage before clustering)
    const bool ordered = tier == 0 && sel.n >= kn.order_min && c->d_order && !kn.no_work_order;
    // The heavy pairs aside: their order (pass H) and their clustering need k_seed's output alone — k_simple never takes a pair with more than kLightHits
    // hits and does not look at its hits —, so they go onto a side stream right behind the seeding, beside the straight-line path; the main stream lists
    // and clusters the light pairs behind k_simple and joins.  Every pair that can run over while clustering is a heavy one (light_pairs_fit, asked where
    // the capacities were made), so the early list, its length and ev_clustered come from the side stream: the large tier starts from there.
    // MCX_CLUSTER_IN_LINE: one launch over all classes on the pass's stream, as it is for the other tiers, without the order, and without side streams.
    // Not where there is nothing to hide behind: with hardly a straight-line pair in the batch (250-base reads at 5 % indels: nearly every pair is heavy)
    // k_simple ends in 0.2 ms, the two clustering launches only share the chip, and the step was measured 1 % longer.  What the last large pass saw decides.
    const int regs = tier == 0 && c->regs_fit && !kn.cluster_mem ? 1 : 0; // k_cluster: a read's seeds in registers (tier 0 only)
    const bool aside = ordered && R.dp_stream[0] && R.ev_seeded && c->light_fit && c->aside_pays && !kn.cluster_in_line && !kn.cluster_split;
    hipStream_t hs = aside ? R.dp_stream[0] : s;
    if (aside) {
        const unsigned ob = (sel.n + 256 * kOrderTile - 1) / (256 * kOrderTile);
        HIP_TRY(hipEventRecord(R.ev_seeded, s)); // (behind k_sa, which rewrites the hits where the suffix array is sampled)
        HIP_TRY(hipStreamWaitEvent(hs, R.ev_seeded, 0));
        k_order_count<<<ob, 256, 0, hs>>>(sel, so.read_blocks, nr, R.d_cnt + CNT_ORDER, nullptr, 0, kHeavyClasses - 1);
        k_order_place<<<ob, 256, 0, hs>>>(sel, so.read_blocks, nr, R.d_cnt + CNT_ORDER, c->d_order, nullptr, 0, kHeavyClasses - 1);
        HIP_TRY(hipEventRecord(R.ev_order_h, hs));
        // (a grid for every pair of the pass: how many are heavy stays on the device, and a block past the launch's classes ends at once)
        k_cluster<<<pb, 256, 0, hs>>>(cx, rb, sel, rl, so.read_blocks, el, c->d_order, R.d_cnt + CNT_ORDER, 0, kHeavyClasses - 1, regs);
        if (early && c->h_early) k_publish_early<<<1, 64, 0, hs>>>(R.d_cnt + CNT_EARLY, c->d_batch_flags + 3, c->d_early);
        if (early) HIP_TRY(hipEventRecord(c->ev_clustered, hs));
        HIP_TRY(hipEventRecord(R.ev_heavy, hs));
    }
    if (ordered) {
        // ahead of them, on a whole batch: the straight-line pairs from their seeds to their records (k_simple); what is left is listed
        // by weight for the per-pair kernels.  (Not without the suffix array in HBM — the seeds must be text positions —, not on a
        // selection: k_simple takes pair = record.  With the -vcf bookkeeping on it writes the pairs' detail records as well.)
        const bool no_simple = kn.no_simple;
        const uint8_t *done = nullptr;
        if (!no_simple && !sel.ids && cx.ix.sa_full && cx.packed) {
            // collect (every pair) -> solve (the problems written down) -> replay (the pairs that wrote some down); MCX_SIMPLE_NO_DP: a pair
            // with such a problem takes the general path
            SimpleLater sl; sl.pairs = kn.simple_no_dp ? nullptr : c->d_sl_pairs; sl.jobs = c->d_sl_jobs; sl.res = c->d_sl_res; sl.job_list = c->d_sl_list;
            sl.n_pairs = R.d_cnt + CNT_SIMPLE_LATER; sl.n_jobs = R.d_cnt + CNT_SIMPLE_JOBS; sl.cap = std::min<uint32_t>(c->sl_cap, std::max<uint32_t>(sel.n / 2, 1024u));
            const unsigned lb = (sl.cap + 255) / 256, jb = std::min<unsigned>((sl.cap * kSimpleJobs + 255) / 256, 3072u); // (launched for what the lists may hold: their lengths stay on the device)
            auto launch = [&](auto nw, auto detail) {
                constexpr bool NW = decltype(nw)::value, DT = decltype(detail)::value;
                k_simple<NW, kDpCollect, DT><<<pb, 256, 0, s>>>(cx, rb, sel.n, sel.est, so.read_blocks, d_recs, c->d_pout, c->d_done, c->d_batch_flags + 2, R.d_cnt + CNT_SIMPLE, sl);
                if (sl.pairs) {
                    k_simple_dp<NW><<<jb, 256, 0, s>>>(cx, sl);
                    k_simple<NW, kDpReplay, DT><<<lb, 256, 0, s>>>(cx, rb, sel.n, sel.est, so.read_blocks, d_recs, c->d_pout, c->d_done, c->d_batch_flags + 2, R.d_cnt + CNT_SIMPLE, sl);
                }
            };
            if (cx.pm.use_nw) { if (cx.detail) launch(std::true_type(), std::true_type()); else launch(std::true_type(), std::false_type()); }
            else { if (cx.detail) launch(std::false_type(), std::true_type()); else launch(std::false_type(), std::false_type()); }
            done = c->d_done;
        }
        if (timing) HIP_TRY(hipEventRecord(R.ev[10], s));
        uint32_t *cls_cnt = R.d_cnt + CNT_ORDER; // (cleared with the pass's counters)
        order_cnt = cls_cnt; // (the class counts: how many pairs the order lists — all of them without k_simple — and where a class begins)
        const unsigned ob = (sel.n + 256 * kOrderTile - 1) / (256 * kOrderTile);
        // (aside: pass L — its stretches of the order begin where pass H's final counts end; that event is long past by now)
        if (aside) HIP_TRY(hipStreamWaitEvent(s, R.ev_order_h, 0));
        k_order_count<<<ob, 256, 0, s>>>(sel, so.read_blocks, nr, cls_cnt, done, aside ? kHeavyClasses : 0, kWorkClasses - 1);
        k_order_place<<<ob, 256, 0, s>>>(sel, so.read_blocks, nr, cls_cnt, c->d_order, done, aside ? kHeavyClasses : 0, kWorkClasses - 1);
        order = c->d_order;
        if (timing) { HIP_TRY(hipEventRecord(R.ev[11], s)); split = true; }
    }
    const size_t cl_bytes = cluster_lds_bytes(cx.caps.hit_cap, cx.caps.cand_cap);
    if (tier == 1 && cl_bytes <= 60 * 1024 && !kn.cluster_by_lane) { // the large tier's pairs: a wavefront each, in two launches by size
        const int small = std::min(kClusterSmall, cx.caps.hit_cap);
        k_cluster_wave<<<std::min<unsigned>(sel.n, 16384u), 64, cluster_lds_bytes(small, small), s>>>(cx, rb, sel, rl, so.read_blocks, -1, small, small, small);
        if (small < cx.caps.hit_cap)
            k_cluster_wave<<<std::min<unsigned>(sel.n, 8192u), 64, cl_bytes, s>>>(cx, rb, sel, rl, so.read_blocks, small, 1 << 30, cx.caps.hit_cap, cx.caps.cand_cap);
    } else if (aside) { // the light pairs; none of them can run over: no early list.  Then the heavy side joins (the time stamp below: behind the join)
        EarlyList none = el; none.ids = nullptr; none.est = nullptr; none.cap = 0;
        k_cluster<<<pb, 256, 0, s>>>(cx, rb, sel, rl, so.read_blocks, none, order, order_cnt, kHeavyClasses, kWorkClasses - 1, regs);
        HIP_TRY(hipStreamWaitEvent(s, R.ev_heavy, 0));
    } else if (ordered && kn.cluster_split) { // (MCX_CLUSTER_SPLIT, measurements: the two launches of the aside path one after the other on the pass's stream)
        k_cluster<<<pb, 256, 0, s>>>(cx, rb, sel, rl, so.read_blocks, el, order, order_cnt, 0, kHeavyClasses - 1, regs);
        k_cluster<<<pb, 256, 0, s>>>(cx, rb, sel, rl, so.read_blocks, el, order, order_cnt, kHeavyClasses, kWorkClasses - 1, regs);
    } else k_cluster<<<pb, 256, 0, s>>>(cx, rb, sel, rl, so.read_blocks, el, order, order_cnt, 0, kWorkClasses - 1, regs);
    if (!aside) {
        if (early && c->h_early) k_publish_early<<<1, 64, 0, s>>>(R.d_cnt + CNT_EARLY, c->d_batch_flags + 3, c->d_early);
        if (early) HIP_TRY(hipEventRecord(c->ev_clustered, s));
    }
    if (timing) HIP_TRY(hipEventRecord(R.ev[e++], s));
    // mate rescue beside the build of the pairs that do not await it (k_build's modes), when the set has a side stream for it
    const bool rescue_aside = paired && R.dp_stream[0] && !kn.rescue_in_line;
    hipStream_t rs = rescue_aside ? R.dp_stream[0] : s;
    if (rescue_aside) { HIP_TRY(hipEventRecord(R.dp_fork, s)); HIP_TRY(hipStreamWaitEvent(rs, R.dp_fork, 0)); }
    if (paired) {
        {
            RescueWork rw; rw.tasks = R.d_rtasks; rw.res = R.d_rres; rw.seeds = R.d_rseeds; rw.plans = R.d_rplans; rw.n_tasks = R.d_cnt + CNT_RTASK; rw.n_plans = R.d_cnt + CNT_RPLAN; rw.n_seeds = R.d_cnt + CNT_RSEED;
            rw.task_cap = R.rtask_cap; rw.seed_cap = R.rseed_cap; rw.ids_n = R.d_rescue_n; rw.n_ids_n = R.d_cnt + CNT_RESCUE_N;
            RescueList rn; rn.ids = R.d_rescue_n; rn.n = R.d_cnt + CNT_RESCUE_N; rn.cap = R.rescue_cap;
            const unsigned gb = std::min<unsigned>(std::max<unsigned>((sel.n + 255) / 256, 1u), 1024u);
            k_rescue_plan<<<gb, 256, 0, rs>>>(cx, rb, sel, rl, rw);
            if (tier == 0) k_rescue_eval<2048><<<4096, 256, 0, rs>>>(cx, rb, sel, rw);
            else k_rescue_eval<4096><<<4096, 256, 0, rs>>>(cx, rb, sel, rw);
            k_rescue_apply<<<gb, 256, 0, rs>>>(cx, rw);
            // the pairs with an N in a read (none in most batches: the launch then ends at once — once it gets onto the chip, which beside
            // the other tier's long-lived wavefronts took the large tier half a millisecond: left out where the batch is known to hold no N)
            if (no_n_reads) {}
            else if (tier == 0) k_rescue<2048><<<256, kRescueThreads, 0, rs>>>(cx, rb, sel, rn, R.d_kscratch);
            else k_rescue<4096><<<256, kRescueThreads, 0, rs>>>(cx, rb, sel, rn, R.d_kscratch);
        }
    }
    // three time stamps: in line they bracket rescue | nothing | build, with the rescue aside build (others) | what is left of the wait for the rescue | build (its pairs)
    // (the large tier's pairs: a wavefront each — k_build_wave; MCX_BUILD_BY_LANE: a lane each there too)
    const size_t bw_bytes = (size_t)6 * cx.caps.cand_cap * sizeof(int32_t);
    const bool build_wave = tier == 1 && bw_bytes <= 48 * 1024 && !kn.build_by_lane;
    const int build_wave_limit = kn.build_wave_limit;
    auto build = [&](int mode) {
        if (build_wave) k_build_wave<<<std::min<unsigned>(sel.n, 8192u), 64, bw_bytes, s>>>(cx, rb, sel, sinks, R.d_cnt + CNT_CELLS, R.d_cnt + CNT_UNSUP, mode, rl, build_wave_limit);
        else k_build<<<pb, 256, 0, s>>>(cx, rb, sel, sinks, R.d_cnt + CNT_CELLS, R.d_cnt + CNT_UNSUP, ll, order, order_cnt, mode, rl);
    };
    if (rescue_aside) {
        HIP_TRY(hipEventRecord(R.dp_join[0], rs));
        build(1);
        if (timing) HIP_TRY(hipEventRecord(R.ev[e++], s));
        HIP_TRY(hipStreamWaitEvent(s, R.dp_join[0], 0));
        if (timing) HIP_TRY(hipEventRecord(R.ev[e++], s));
        build(2);
    } else {
        if (timing) { HIP_TRY(hipEventRecord(R.ev[e++], s)); HIP_TRY(hipEventRecord(R.ev[e++], s)); }
        build(0);
    }
    if (late) HIP_TRY(hipEventRecord(c->ev_built, s));
    if (timing) HIP_TRY(hipEventRecord(R.ev[e++], s));
    if ((rc2 = launch_dp(kn, R, cx, sinks, rb, sel, c->rlen_max))) return rc2;
    if (timing) HIP_TRY(hipEventRecord(R.ev[e++], s));
    if (c->mx.on) k_finish<true><<<pb, 256, 0, s>>>(cx, rb, sel, d_recs, c->d_pout, R.d_ov, R.d_cnt + CNT_OV, R.ov_cap, c->d_batch_flags + 2, order, order_cnt, multi_out(c));
    else k_finish<false><<<pb, 256, 0, s>>>(cx, rb, sel, d_recs, c->d_pout, R.d_ov, R.d_cnt + CNT_OV, R.ov_cap, c->d_batch_flags + 2, order, order_cnt, MultiOut());
    if (timing) HIP_TRY(hipEventRecord(R.ev[e++], s));
    HIP_TRY(hipGetLastError());
    static_assert(CNT_COPY == CNT_ORDER + kWorkClasses * kCntPad, "the order's class counts come back with the pass's counters");
    HIP_TRY(hipMemcpyAsync(R.h_cnt, R.d_cnt, CNT_COPY * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    const int e_flag = e | (rescue_aside ? 0x100 : 0) | (split ? 0x200 : 0) | (aside ? 0x400 : 0); // (for pass_finish: which stage a time stamp closes; the heavy pairs went aside)
    if (queued) { *queued = e_flag; return 0; }
    hipEvent_t ev_dbg[2] = {nullptr, nullptr}; // (MCX_TIMING: when tier 0 and the large tier beside it were done)
    if (early && kn.timing) {
        for (int k = 0; k < 2; k++) HIP_TRY(hipEventCreate(&ev_dbg[k]));
        HIP_TRY(hipEventRecord(ev_dbg[0], s));
    }
    uint32_t n_late = 0;
    if (early) { // the pairs k_cluster listed: through the large tier now, while the kernels above run
        const PassRes &T = c->t1;
        uint32_t n_early = 0;
        HIP_TRY(hipStreamWaitEvent(T.stream, c->ev_clustered, 0));
        bool no_n;
        if (c->h_early) { // k_publish_early wrote both numbers into page-locked memory
            HIP_TRY(timed_wait(kn.timing, "wait for k_cluster (the early list's length)", __LINE__, [&] { return hipEventSynchronize(c->ev_clustered); }));
            n_early = c->h_early[0]; no_n = c->h_early[1] == 0;
        } else {
            HIP_TRY(hipMemcpyAsync(T.h_cnt, R.d_cnt + CNT_EARLY, sizeof(uint32_t), hipMemcpyDeviceToHost, T.stream));
            HIP_TRY(hipMemcpyAsync(T.h_cnt + 1, c->d_batch_flags + 3, sizeof(uint32_t), hipMemcpyDeviceToHost, T.stream)); // (k_pack_reads is long done)
            HIP_TRY(hipStreamSynchronize(T.stream));
            n_early = T.h_cnt[0]; no_n = T.h_cnt[1] == 0;
        }
        if (n_early > el.cap) { (void)hipStreamSynchronize(s); return fail(MCX_ERR_CAPACITY, "overflow list overflow"); }
        if (stats) stats->tier1_pairs += n_early;
        const bool t1_timing = kn.timing;
        if (n_early + (late ? kLateRoom : 0) > c->tier[1].max_pairs) { if (int r = tier1_grow(c, (uint64_t)n_early + (late ? kLateRoom : 0))) { (void)hipStreamSynchronize(s); return r; } }
        const uint32_t room = c->tier[1].max_pairs - (late ? kLateRoom : 0); // (the last records are the late list's)
        mcx_stats t1;
        uint32_t m = 0;
        int e1 = -1, e2 = -1;
        for (uint32_t lo = 0; lo < n_early && rc2 == 0; lo += room) {
            // (all but the last pass are waited for here; the last one is left under way while the late list is seen to)
            m = std::min<uint32_t>(room, n_early - lo);
            const bool last = lo + room >= n_early;
            PairSel s1; s1.n = m; s1.ids = T.d_sel_ids + lo; s1.est = T.d_est + lo;
            memset(&t1, 0, sizeof t1);
            rc2 = run_pairs(c, 1, T, rb, paired, s1, d_recs, d_cig, t1_timing ? &t1 : stats, t1_timing, false, 0, last ? &e1 : nullptr, false, no_n);
            if (!last && rc2 == 0) rc2 = tier1_pass_end(c, T, m, t1_timing ? &t1 : nullptr, stats, -1);
        }
        if (late && rc2 == 0) {
            // what ran over after clustering (k_build's list): known once tier 0 has built; a handful of pairs, which take the
            // large tier on the third set of resources while tier 0's DP and finish stages run
            const PassRes &U = c->t2;
            HIP_TRY(timed_wait(kn.timing, "wait for k_build (the late list's length)", __LINE__, [&] { return hipEventSynchronize(c->ev_built); }));
            HIP_TRY(hipMemcpyAsync(U.h_cnt, R.d_cnt + CNT_LATE, sizeof(uint32_t), hipMemcpyDeviceToHost, U.stream));
            HIP_TRY(hipStreamSynchronize(U.stream));
            n_late = std::min<uint32_t>(U.h_cnt[0], kLateRoom);
            if (n_late) {
                PairSel s2; s2.n = n_late; s2.ids = U.d_sel_ids; s2.est = U.d_est;
                // (their seed hits are in this pass's records — pair = record when the pass is a whole batch — and complete: what ran over came later)
                rc2 = run_pairs(c, 1, U, rb, paired, s2, d_recs, d_cig, stats, false, false, c->tier[1].max_pairs - kLateRoom, &e2, sel.ids == nullptr && state_off == 0, no_n);
                if (stats) stats->tier1_pairs += n_late;
            }
        }
        // (everything of the batch is queued: what follows its kernels goes behind them now, before the host waits for any of the passes)
        if (rc2 == 0 && c->tail.want && !sel.ids && state_off == 0) rc2 = queue_batch_tail(c);
        if (e1 >= 0) { const int r = tier1_pass_end(c, T, m, t1_timing ? &t1 : nullptr, stats, e1); if (rc2 == 0) rc2 = r; }
        if (e2 >= 0) { const int r = tier1_pass_end(c, c->t2, n_late, nullptr, stats, e2); if (rc2 == 0) rc2 = r; }
    }
    if (ev_dbg[0]) HIP_TRY(hipEventRecord(ev_dbg[1], c->t1.stream));
    if (!early && tier == 0 && rc2 == 0 && c->tail.want && !sel.ids && state_off == 0) rc2 = queue_batch_tail(c);
    HIP_TRY(timed_wait(kn.timing, "wait for the pass's stream", __LINE__, [&] { return hipStreamSynchronize(s); }));
    if (ev_dbg[0]) {
        float a = 0, b = 0;
        HIP_TRY(hipEventSynchronize(ev_dbg[1]));
        HIP_TRY(hipEventElapsedTime(&a, c->ev_clustered, ev_dbg[0])); HIP_TRY(hipEventElapsedTime(&b, c->ev_clustered, ev_dbg[1]));
        fprintf(stderr, "[run_pairs] after clustering: tier 0 done at %.2f ms, the large tier beside it by %.2f ms\n", a, b);
        for (int k = 0; k < 2; k++) (void)hipEventDestroy(ev_dbg[k]);
    }
    if (rc2) return rc2;
    return pass_finish(c, tier, R, sel.n, stats, timing, e_flag);
}

// what follows a pass once its stream has been joined: the work lists' overflow checks, counts and stage times
static int pass_finish(mcx_ctx *c, int tier, const PassRes &R, uint32_t n_sel, mcx_stats *stats, bool timing, int e)
{
    if (tier == 1 && c->kn.tier1_hist) { // experiments: how heavy are the pairs of the large tier?
        std::vector<PairHdr> hd(n_sel);
        HIP_TRY(hipMemcpy2D(hd.data(), sizeof(PairHdr), c->tier[1].state, (size_t)c->tier[1].lay.stride, sizeof(PairHdr), n_sel, hipMemcpyDeviceToHost));
        const int edges[8] = {16, 32, 64, 128, 256, 512, 1024, 1 << 30};
        uint32_t hh[8] = {0}, hc[8] = {0}, hf[8] = {0};
        for (const PairHdr &h : hd) {
            const int nh = std::max(h.n_hits[0], h.n_hits[1]), nc = std::max(h.n_cands[0], h.n_cands[1]);
            for (int b = 0; b < 8; b++) if (nh <= edges[b]) { hh[b]++; break; }
            for (int b = 0; b < 8; b++) if (nc <= edges[b]) { hc[b]++; break; }
            for (int b = 0; b < 8; b++) if (h.n_frags <= edges[b]) { hf[b]++; break; }
        }
        fprintf(stderr, "[tier 1 hist] %u pairs; per-read maximum <=16,32,64,128,256,512,1024,more: hits", n_sel);
        for (int b = 0; b < 8; b++) fprintf(stderr, " %u", hh[b]);
        fprintf(stderr, " | candidates");
        for (int b = 0; b < 8; b++) fprintf(stderr, " %u", hc[b]);
        fprintf(stderr, " | fragments");
        for (int b = 0; b < 8; b++) fprintf(stderr, " %u", hf[b]);
        fprintf(stderr, "\n");
    }
    const uint32_t *n = R.h_cnt;
    if (c->kn.dp_hist && n_sel >= 1024) { // experiments: the sizes of the pass's DP problems (query x target, by bit length), per list
        static const char *names[kDpClasses] = {"small", "wave1", "wave4", "wave16", "tiny", "half"};
        for (int k = 0; k < kDpClasses; k++) {
            const uint32_t m = std::min(n[CNT_JOB0 + k * kCntPad], R.job_cap[k]);
            if (!m) continue;
            std::vector<DpJob> jobs(m);
            HIP_TRY(hipMemcpy(jobs.data(), R.d_jobs[k], (size_t)m * sizeof(DpJob), hipMemcpyDeviceToHost));
            unsigned long long hist[12][12] = {{0}}, cells = 0, diag = 0;
            for (const DpJob &j : jobs) {
                const int a = std::min(11, j.rLen ? 32 - __builtin_clz((unsigned)j.rLen) : 0), b = std::min(11, j.gLen ? 32 - __builtin_clz((unsigned)j.gLen) : 0);
                hist[a][b]++; cells += (unsigned long long)j.rLen * j.gLen; diag += (unsigned long long)(j.rLen + j.gLen - 1);
            }
            fprintf(stderr, "[dp hist] tier %d list %s: %u problems, %llu cells (mean %.1f), mean anti-diagonals %.1f; rows = bit length of the query, columns = of the target\n", tier, names[k], m, cells,
                    (double)cells / m, (double)diag / m);
            for (int a = 0; a < 12; a++) {
                bool any = false;
                for (int b = 0; b < 12; b++) any |= hist[a][b] != 0;
                if (!any) continue;
                fprintf(stderr, "[dp hist]   q<2^%-2d", a);
                for (int b = 0; b < 12; b++) fprintf(stderr, " %9llu", hist[a][b]);
                fprintf(stderr, "\n");
            }
        }
    }
    if (tier == 0) { // mcx_pass_last_shape: the class counts (all zero without the order), the two launches' pairs, whether the heavy ones went aside, the early list
        uint32_t *sh = c->last_shape;
        sh[6] = sh[7] = 0;
        for (int k = 0; k < kWorkClasses; k++) { sh[k] = n[CNT_ORDER + k * kCntPad]; sh[k < kHeavyClasses ? 6 : 7] += sh[k]; }
        sh[8] = (e & 0x400) ? 1u : 0u; sh[9] = n[CNT_EARLY];
        // (run_pairs: the heavy pairs aside) a large ordered pass says whether the next one has a straight-line path worth hiding behind: an eighth of its pairs
        if ((e & 0x200) && n_sel >= kAsideGatePairs) c->aside_pays = (uint64_t)n[CNT_SIMPLE] * 8 >= n_sel;
    }
    if (tier == 0 && !c->dp_grown) c->job2_seen = std::max(c->job2_seen, n[CNT_JOB2]); // (batch_close: dp_scratch_grow)
    // a work list that ran over: nothing of this pass is kept, the caller maps the selection in two halves
    if ((R.d_tasks && n[CNT_TASKS] > R.task_cap) || n[CNT_RESCUE] > R.rescue_cap || n[CNT_RTASK] > R.rtask_cap || n[CNT_RSEED] > R.rseed_cap) return kListOverflow;
    for (int k = 0; k < kDpClasses; k++) if (n[CNT_JOB0 + k * kCntPad] > R.job_cap[k]) return kListOverflow;
    if (n[CNT_UNSUP]) return fail(MCX_ERR_UNSUPPORTED, "a gapped fragment exceeds 2048 x 1024 cells per side");
    if (timing && c->kn.timing)
        fprintf(stderr, "[run_pairs] pairs %u: sa tasks %u, rescue pairs %u (windows %u), dp jobs by class (tiny) %u %u (half) %u %u %u %u, cells %llu, overflow pairs %u (+ %u listed while clustering, %u of them for their seed hits), %u straight-line pairs (k_simple)\n", n_sel,
                n[CNT_TASKS], n[CNT_RESCUE], n[CNT_RTASK], n[CNT_JOB4], n[CNT_JOB0], n[CNT_JOB5], n[CNT_JOB1], n[CNT_JOB2], n[CNT_JOB3], *(const unsigned long long *)(n + CNT_CELLS), n[CNT_OV], n[CNT_EARLY], n[CNT_EARLY_HITS], n[CNT_SIMPLE]);
    if (stats) {
        stats->dp_jobs += (int64_t)n[CNT_JOB0] + n[CNT_JOB1] + n[CNT_JOB2] + n[CNT_JOB3] + n[CNT_JOB4] + n[CNT_JOB5];
        stats->dp_cells += (int64_t)(*(const unsigned long long *)(n + CNT_CELLS));
        stats->simple_pairs += n[CNT_SIMPLE];
        if (timing) {
            float ms[10];
            const bool aside = (e & 0x100) != 0;
            const int n_ev = e & 0xFF;
            for (int i = 0; i + 1 < n_ev; i++) HIP_TRY(hipEventElapsedTime(&ms[i], R.ev[i], R.ev[i + 1]));
            stats->ms_seed += ms[0]; stats->ms_sa += ms[1];
            if (e & 0x200) { // ev[2] .. ev[10]: the straight-line path; ev[10] .. ev[11]: the order; ev[11] .. ev[3]: k_cluster
                float a = 0, b = 0, d = 0;
                HIP_TRY(hipEventElapsedTime(&a, R.ev[2], R.ev[10])); HIP_TRY(hipEventElapsedTime(&b, R.ev[10], R.ev[11])); HIP_TRY(hipEventElapsedTime(&d, R.ev[11], R.ev[3]));
                stats->ms_simple += a; stats->ms_order += b; stats->ms_cluster += d;
            } else stats->ms_cluster += ms[2];
            // (run_pairs: in line ms[3] is the rescue, ms[4] nothing, ms[5] the build; with the rescue on a stream of its own ms[3] and ms[5] are the
            //  build's two launches and ms[4] what was left to wait for the rescue)
            if (aside) { stats->ms_build += ms[3] + ms[5]; stats->ms_rescue += ms[4]; }
            else { stats->ms_rescue += ms[3] + ms[4]; stats->ms_build += ms[5]; }
            stats->ms_dp += ms[6]; stats->ms_finish += ms[7];
        }
    }
    return 0;
}

extern "C" int mcx_pass_last_shape(mcx_ctx *c, uint32_t out[10])
{
    if (!c || !out) return mcx_set_error(MCX_ERR_ARG, "mcx_pass_last_shape: null argument");
    memcpy(out, c->last_shape, sizeof c->last_shape);
    return 0;
}

// end of a pass of the large tier that was left under way beside tier 0 (e: its timing events, -1: it was waited for already)
static int tier1_pass_end(mcx_ctx *c, const PassRes &T, uint32_t m, mcx_stats *t1, mcx_stats *stats, int e)
{
    int rc = 0;
    if (e >= 0) {
        HIP_TRY(hipStreamSynchronize(T.stream));
        rc = pass_finish(c, 1, T, m, t1 ? t1 : stats, t1 != nullptr, e);
    }
    if (t1) {
        fprintf(stderr, "[tier 1, beside tier 0] %u pairs: seed %.2f sa %.2f cluster %.2f rescue %.2f build %.2f dp %.2f finish %.2f ms\n", m, t1->ms_seed, t1->ms_sa,
                t1->ms_cluster, t1->ms_rescue, t1->ms_build, t1->ms_dp, t1->ms_finish);
        if (stats) { stats->dp_jobs += t1->dp_jobs; stats->dp_cells += t1->dp_cells; }
    }
    if (rc == kListOverflow) rc = fail(MCX_ERR_CAPACITY, "work list overflow in tier 1");
    if (rc == 0 && T.h_cnt[CNT_OV]) rc = tier1_error(c, T);
    return rc;
}

// a pair that does not even fit the large tier: say which and why
static int tier1_error(mcx_ctx *c, const PassRes &R)
{
    uint32_t first = 0;
    PairOut po; memset(&po, 0, sizeof po);
    if (hipMemcpy(&first, R.d_ov, sizeof first, hipMemcpyDeviceToHost) == hipSuccess)
        (void)hipMemcpy(&po, c->d_pout + first, sizeof po, hipMemcpyDeviceToHost);
    return fail(MCX_ERR_CAPACITY, "a pair exceeded the tier-1 capacities (pair " + std::to_string(first) + ", overflow flags " + std::to_string(po.flags & kOvAny) +
                                  ": 1 hits 2 candidates 4 fragments 8 ops 16 jobs 32 cigar 64 rescue window)");
}

__global__ void k_fill_i32(int32_t *p, int32_t v, uint32_t n)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// the sum of a 64-bit count over a workgroup of 256: in wave 0's lane 0 (s: four words of LDS per count in use)
static __device__ __forceinline__ unsigned long long block_sum_256(unsigned long long v, unsigned long long *s)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return s[0] + s[1] + s[2] + s[3];
}

// the seeding statistics of a batch: the per-read words 16 bytes at a time (both arrays are 16-byte aligned), three atomics per workgroup
constexpr unsigned kReduceStatsBlocks = 1024;
__global__ void __launch_bounds__(256) k_reduce_stats(const uint32_t *a, const uint32_t *b, uint32_t n, unsigned long long *out)
{
    __shared__ unsigned long long s_sum[3][4];
    unsigned long long sa = 0, sb = 0, sh = 0; // extension steps, blocks touched, hits (H of SURVEY.md §8d)
    const uint32_t n4 = n >> 2, T = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t i = t; i < n4; i += T) {
        const U4 x = ((const U4 *)a)[i], y = ((const U4 *)b)[i];
        sa += (unsigned long long)(x.x & 0x7FFFFFFFu) + (x.y & 0x7FFFFFFFu) + (x.z & 0x7FFFFFFFu) + (x.w & 0x7FFFFFFFu);
        sb += (unsigned long long)(y.x & 0xFFFFFu) + (y.y & 0xFFFFFu) + (y.z & 0xFFFFFu) + (y.w & 0xFFFFFu);
        sh += (unsigned long long)(y.x >> 20) + (y.y >> 20) + (y.z >> 20) + (y.w >> 20);
    }
    for (uint32_t i = 4 * n4 + t; i < n; i += T) { sa += a[i] & 0x7FFFFFFFu; sb += b[i] & 0xFFFFFu; sh += b[i] >> 20; }
    sa = block_sum_256(sa, s_sum[0]); sb = block_sum_256(sb, s_sum[1]); sh = block_sum_256(sh, s_sum[2]);
    if (threadIdx.x == 0) { if (sa) atomicAdd(out, sa); if (sb) atomicAdd(out + 1, sb); if (sh) atomicAdd(out + 2, sh); }
}

// ---- avgDist replay on the device (the host only walks the per-chunk sums) ---------------------
// per chunk of 100 pairs: number of proper pairs and their summed distance (ReadMapping.cpp:527-531)
// A wavefront per chunk: neighbouring lanes read neighbouring records (the eight bytes that hold the distance and the two flags) and the pair's two offsets,
// all fetched before any is looked at; the lanes' sums are folded with shuffles — integer sums, the same in any order.  One atomic per workgroup: the
// count of mapped reads has one address, and atomics on one address queue behind one another.
// (lens: the batch is paired, off[2 p + 2] exists for every pair; a single-end batch has no proper pairs and no lengths to sum)
static inline unsigned chunk_sums_blocks(uint32_t n_chunks) { return std::max(1u, std::min((n_chunks + 3u) / 4u, 1024u)); }
__global__ void __launch_bounds__(256) k_chunk_sums(const PairOut *po, const uint32_t *off, uint32_t n_pairs, uint32_t chunk, int lens, uint32_t *ok_cnt, uint32_t *dist_sum,
                                                    uint32_t *len_sum, uint32_t *mapped)
{
    static_assert(sizeof(PairOut) == 32 && offsetof(PairOut, pair_dist) == 16 && offsetof(PairOut, pair_ok) == 20 && offsetof(PairOut, mapped) == 22, "k_chunk_sums reads bytes 16..23 of a record");
    __shared__ uint32_t s_m[4];
    const uint32_t n_chunks = (n_pairs + chunk - 1) / chunk;
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    uint32_t m = 0;
    for (uint32_t c = wave; c < n_chunks; c += n_waves) {
        uint32_t ok = 0, ds = 0, ls = 0;
        const uint32_t p1 = min(n_pairs, (c + 1) * chunk);
        for (uint32_t p = c * chunk + lane; p < p1; p += 128) { // (two records a lane and round: a chunk of 100 is one round)
            const uint32_t q = p + 64;
            const bool two = q < p1;
            const uint2 v = *(const uint2 *)((const uint8_t *)(po + p) + 16); // {pair_dist, pair_ok | mapped << 16}
            const uint2 v2 = two ? *(const uint2 *)((const uint8_t *)(po + q) + 16) : make_uint2(0u, 0u);
            const uint32_t l = lens ? off[2 * p + 2] - off[2 * p] : 0u, l2 = lens && two ? off[2 * q + 2] - off[2 * q] : 0u; // myReadLengthSum, ReadMapping.cpp:529-530
            if ((int16_t)(v.y & 0xFFFFu)) { ok++; ds += v.x; ls += l; }
            if ((int16_t)(v2.y & 0xFFFFu)) { ok++; ds += v2.x; ls += l2; }
            m += (uint32_t)(int16_t)(v.y >> 16) + (uint32_t)(int16_t)(v2.y >> 16);
        }
        for (int o = 32; o > 0; o >>= 1) { ok += __shfl_down(ok, o, 64); ds += __shfl_down(ds, o, 64); ls += __shfl_down(ls, o, 64); }
        if (lane == 0) { ok_cnt[c] = ok; dist_sum[c] = ds; len_sum[c] = ls; }
    }
    for (int o = 32; o > 0; o >>= 1) m += __shfl_down(m, o, 64);
    if (lane == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0 && (m = s_m[0] + s_m[1] + s_m[2] + s_m[3])) atomicAdd(mapped, m);
}

// pairs whose chunk estimate lies outside their validity interval -> redo list (avg_replay's test)
// (-m) the reads of listed pairs have no extra lines (yet)
__global__ void __launch_bounds__(256) k_mx_clear(const uint32_t *ids, uint32_t n, int nr, uint4 *ref)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        for (int s = 0; s < nr; s++) ref[(int64_t)ids[i] * nr + s] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ void k_check_est(const PairOut *po, uint32_t n_pairs, uint32_t chunk, const int32_t *est_chunk, uint32_t *redo_ids,
                            int32_t *redo_est, uint32_t *n_redo, uint32_t cap)
{
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += gridDim.x * blockDim.x) {
        const PairOut o = po[p];
        const int32_t e = est_chunk[p / chunk];
        const bool ok = (o.flags & kRescueUsedEst) ? o.est == e : (e >= o.est_lo && e <= o.est_hi);
        if (!ok) { const uint32_t at = atomicAdd(n_redo, 1u); if (at < cap) { redo_ids[at] = p; redo_est[at] = e; } }
    }
}

// mcx_avg_walk on the device: the estimate every chunk of the batch is checked against.  The walk is no chain: the estimate before chunk k is
// the run's when the batch began (k = 0, or no more than 1000 proper pairs so far — the count only grows, so nothing moved it yet) or the
// rounded mean over everything before k (ReadMapping.cpp:538-539) — prefix sums of the chunks' pairs and distances.  A chunk per thread, 1024
// chunks per workgroup: a workgroup sums everything before its stretch itself (neighbouring lanes, neighbouring words: tens of thousands of
// numbers at the most, out of L2) and scans its own chunks with shuffles, so that no workgroup waits for another and none walks a chain.
// (first: the batch is the first of its round — of a run on one stream, every batch —: its first chunk takes cur0 as it is; a batch behind
//  others of the round starts from their totals, tp0 / td0 then hold them too)
static inline unsigned avg_walk_blocks(uint32_t n_chunks) { return std::max(1u, (n_chunks + 1023u) / 1024u); }
__global__ void __launch_bounds__(1024) k_avg_walk(const uint32_t *ok, const uint32_t *ds, uint32_t nc, long long cur0, long long tp0, long long td0, int first, int32_t *est_chunk)
{
    __shared__ long long s_bp[16], s_bd[16], s_wp[16], s_wd[16]; // per wavefront: its share of what lies before the stretch, its own chunks' sums
    const uint32_t lo = blockIdx.x * 1024u, k = lo + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    long long bp = 0, bd = 0;
    for (uint32_t i = threadIdx.x; i < lo; i += 1024u) { bp += ok[i]; bd += ds[i]; }
    for (int o = 32; o > 0; o >>= 1) { bp += __shfl_down(bp, o, 64); bd += __shfl_down(bd, o, 64); }
    const long long mp = k < nc ? (long long)ok[k] : 0, md = k < nc ? (long long)ds[k] : 0;
    long long ip = mp, id = md; // inclusive scan over the wavefront
    for (int o = 1; o < 64; o <<= 1) {
        const long long a = __shfl_up(ip, o, 64), b = __shfl_up(id, o, 64);
        if (lane >= o) { ip += a; id += b; }
    }
    if (lane == 0) { s_bp[w] = bp; s_bd[w] = bd; }
    if (lane == 63) { s_wp[w] = ip; s_wd[w] = id; }
    __syncthreads();
    long long tp = tp0 + ip - mp, td = td0 + id - md; // what lies before chunk k
    for (int j = 0; j < 16; j++) { tp += s_bp[j]; td += s_bd[j]; if (j < w) { tp += s_wp[j]; td += s_wd[j]; } }
    if (k < nc) {
        uint32_t cur = (uint32_t)cur0;
        if ((k > 0 || !first) && tp > 1000) cur = (uint32_t)(int)(1. * (double)td / (double)tp + .5);
        est_chunk[k] = (int32_t)(cur * 1.5);
    }
}

// What follows the kernels of a whole-batch pass, queued behind them BEFORE the host waits for the pass (the large tier's passes beside
// it included: their streams' events) instead of in three round trips after it: the seeding statistics, the per-chunk sums, the walk
// and the check of every pair's estimate against its chunk's, everything the host wants of them in one copy to page-locked memory.
// Used when the pass went the plain way (no halved selection, no pair left over for the large tier afterwards: run_selection);
// the caller walks the sums itself too (a few thousand scalars) and takes the device's list only when both walks agree.
static int tail_reserve(mcx_ctx *c)
{
    mcx_ctx::Tail &t = c->tail;
    const uint32_t want = 8 + 4 + 6 + 4 * (uint32_t)((c->max_reads + kReadChunkSize / 2 - 1) / (kReadChunkSize / 2));
    if (t.cap >= want) return 0;
    HIP_TRY(hipMalloc((void **)&t.d, (size_t)want * 4));
    HIP_TRY(hipHostMalloc((void **)&t.h, (size_t)want * 4));
    t.cap = want;
    for (auto &e : t.ev) if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return 0;
}

static int queue_batch_tail(mcx_ctx *c)
{
    BatchRun &br = c->run;
    mcx_ctx::Tail &t = c->tail;
    hipStream_t s = c->t0.stream;
    const uint32_t nc = br.n_chunks, n_reads = br.rb.n_reads;
    if (int rc = tail_reserve(c)) return rc;
    if (c->overlap_tiers) { // the passes of the large tier beside this one write records and outcomes of their own pairs
        HIP_TRY(hipEventRecord(t.ev[0], c->t1.stream)); HIP_TRY(hipStreamWaitEvent(s, t.ev[0], 0));
        if (c->overlap_late) { HIP_TRY(hipEventRecord(t.ev[1], c->t2.stream)); HIP_TRY(hipStreamWaitEvent(s, t.ev[1], 0)); }
    }
    // (the sums in the tail's own words, behind the walk's estimates: the per-read statistics stay as the passes left them — a batch whose tail does not
    //  stand in the end, because pairs went on to the large tier or the selection was halved, reduces them again once every pass has run, like a batch
    //  without a tail: round 5 took the tail's snapshot then, made before those passes searched their reads again)
    unsigned long long *d_sum = (unsigned long long *)(t.d + 2); // counters [2..8): three 64-bit sums
    int32_t *d_est = (int32_t *)(t.d + 8);
    uint32_t *d_ok = t.d + 8 + nc, *d_ds = d_ok + nc, *d_ls = d_ds + nc;
    HIP_TRY(hipMemsetAsync(t.d, 0, 8 * sizeof(uint32_t), s));
    k_reduce_stats<<<kReduceStatsBlocks, 256, 0, s>>>(c->d_read_ext, c->d_read_blocks, n_reads, d_sum);
    k_chunk_sums<<<chunk_sums_blocks(nc), 256, 0, s>>>(c->d_pout, br.rb.off, br.n_pairs, kReadChunkSize / 2, br.paired ? 1 : 0, d_ok, d_ds, d_ls, t.d + 1);
    if (br.paired) {
        k_avg_walk<<<avg_walk_blocks(nc), 1024, 0, s>>>(d_ok, d_ds, nc, (long long)t.state0[0], (long long)t.state0[1], (long long)t.state0[2], 1, d_est);
        k_check_est<<<2048, 256, 0, s>>>(c->d_pout, br.n_pairs, kReadChunkSize / 2, d_est, c->t0.d_sel_ids, c->t0.d_est, t.d, c->t0.ov_cap);
    }
    HIP_TRY(hipGetLastError());
    uint32_t *h = t.h;
    HIP_TRY(hipMemcpyAsync(h, t.d, 8 * 4, hipMemcpyDeviceToHost, s));                       // n_redo, mapped, statistics
    HIP_TRY(hipMemcpyAsync(h + 8, c->d_batch_flags, 4 * 4, hipMemcpyDeviceToHost, s));      // the CIGAR pool's words, its overflow flag
    HIP_TRY(hipMemcpyAsync(h + 18, d_ok, (size_t)nc * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h + 18 + nc, d_ds, 2 * (size_t)nc * 4, hipMemcpyDeviceToHost, s)); // (distance sums, then length sums)
    if (br.paired) HIP_TRY(hipMemcpyAsync(h + 18 + 3 * nc, d_est, (size_t)nc * 4, hipMemcpyDeviceToHost, s));
    t.queued = t.ran = true;
    br.d_ok = d_ok; br.d_ds = d_ds;
    return 0;
}

extern "C" void mcx_avg_init(int64_t a[4]) { a[0] = 1000; a[1] = 0; a[2] = 0; a[3] = 0; }

// ReadMapping.cpp:462 / :538-539 over consecutive chunks
extern "C" void mcx_avg_walk(int64_t st[3], const uint32_t *pairs, const uint32_t *dist, uint32_t n_chunks, int32_t *est_chunk)
{
    uint32_t cur = (uint32_t)st[0];
    int64_t tp = st[1], td = st[2];
    for (uint32_t k = 0; k < n_chunks; k++) {
        if (est_chunk) est_chunk[k] = (int32_t)(cur * 1.5);
        tp += pairs[k]; td += dist[k];
        if (tp > 1000) cur = (uint32_t)(int)(1. * td / tp + .5);
    }
    st[0] = cur; st[1] = tp; st[2] = td;
}

// runs the tiers for the pairs in `ids` (null: all pairs of the batch) with per-pair estimates
__global__ void k_gather_pout(const PairOut *pout, const uint32_t *ids, uint32_t n, PairOut *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pout[ids[i]];
}

static int run_selection(mcx_ctx *c, const ReadBatch &rb, int paired, const std::vector<uint32_t> *ids,
                         const std::vector<int32_t> *est, int32_t est_all, uint32_t n_pairs, AlnRec *d_recs,
                         uint32_t *d_cig, mcx_stats *stats, bool timing)
{
    hipStream_t s = c->t0.stream;
    const uint32_t n = ids ? (uint32_t)ids->size() : n_pairs;
    if (n == 0) return 0;
    PairSel sel; sel.n = n; sel.ids = nullptr; sel.est = c->t0.d_est;
    if (ids) {
        HIP_TRY(hipMemcpyAsync(c->t0.d_sel_ids, ids->data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        sel.ids = c->t0.d_sel_ids;
    }
    if (est) HIP_TRY(hipMemcpyAsync(c->t0.d_est, est->data(), n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    else k_fill_i32<<<(n + 255) / 256, 256, 0, s>>>(c->t0.d_est, est_all, n);
    if (c->mx.on) { // (-m) the selection's reads have no extra lines until k_finish<true> says otherwise: a pair that k_simple finishes this time keeps none from an earlier pass
        const int nr = paired ? 2 : 1;
        if (ids) k_mx_clear<<<(n + 255) / 256, 256, 0, s>>>(c->t0.d_sel_ids, n, nr, c->mx.d_ref);
        else HIP_TRY(hipMemsetAsync(c->mx.d_ref, 0, (size_t)n * nr * sizeof(uint4), s));
    }
    const PassRes &R0 = c->t0;
    int rc = run_pairs(c, 0, R0, rb, paired, sel, d_recs, d_cig, stats, timing, true);
    // (the batch's tail, if the pass queued it, stands only when the pass is all there was: no halves, no pairs left for the large tier)
    if (rc != 0 || c->t0.h_cnt[CNT_OV] != 0) c->tail.queued = false;
    if (rc == kListOverflow) {
        // unusually many hits or DP problems per read (e.g. indel-heavy long reads): halve the selection
        if (n < 2) return fail(MCX_ERR_CAPACITY, "work list overflow for a single pair");
        if (stats) stats->halved_selections++;
        for (int half = 0; half < 2; half++) {
            const uint32_t lo = half ? n / 2 : 0, hi = half ? n : n / 2;
            std::vector<uint32_t> sub_ids(hi - lo);
            std::vector<int32_t> sub_est(hi - lo);
            for (uint32_t i = lo; i < hi; i++) { sub_ids[i - lo] = ids ? (*ids)[i] : i; sub_est[i - lo] = est ? (*est)[i] : est_all; }
            if ((rc = run_selection(c, rb, paired, &sub_ids, &sub_est, 0, n_pairs, d_recs, d_cig, stats, timing))) return rc;
        }
        return 0;
    }
    if (rc) return rc;
    uint32_t n_ov = c->t0.h_cnt[CNT_OV];
    if (n_ov == 0) return 0;
    if (n_ov > c->t0.ov_cap) return fail(MCX_ERR_CAPACITY, "overflow list overflow");
    // tier 1: the overflowed pairs again, with capacities that are hard bounds for the read length
    std::vector<uint32_t> ov(n_ov);
    HIP_TRY(hipMemcpy(ov.data(), c->t0.d_ov, n_ov * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::sort(ov.begin(), ov.end());
    std::vector<int32_t> ov_est(n_ov);
    // their estimates (and flags): gathered on the device — the whole PairOut array is 128 MB at 4 M pairs
    std::vector<PairOut> ov_out(n_ov);
    for (uint32_t lo = 0; lo < n_ov; lo += kPoutSel) {
        const uint32_t m = std::min<uint32_t>(kPoutSel, n_ov - lo);
        HIP_TRY(hipMemcpyAsync(c->t0.d_sel_ids, ov.data() + lo, m * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        k_gather_pout<<<(m + 255) / 256, 256, 0, s>>>(c->d_pout, c->t0.d_sel_ids, m, c->d_pout_sel);
        HIP_TRY(hipMemcpyAsync(ov_out.data() + lo, c->d_pout_sel, m * sizeof(PairOut), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (uint32_t i = 0; i < n_ov; i++) ov_est[i] = ov_out[i].est;
    if (stats) stats->tier1_pairs += n_ov;
    if (c->kn.timing) { // what sent them here
        uint32_t by_flag[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < n_ov; i++) for (int b = 0; b < 8; b++) if (ov_out[i].flags & (1u << b)) by_flag[b]++;
        fprintf(stderr, "[tier 1] %u pairs over the tier-0 capacities: hits %u candidates %u fragments %u ops %u jobs %u cigar %u rescue window %u detail %u\n", n_ov, by_flag[0],
                by_flag[1], by_flag[2], by_flag[3], by_flag[4], by_flag[5], by_flag[6], by_flag[7]);
    }
    // (the pairs that ran over while clustering went through the large tier beside this pass already — run_pairs; what is
    //  left ran over later: column strings, job lists)
    for (uint32_t lo = 0; lo < n_ov; lo += c->tier[1].max_pairs) {
        uint32_t m = std::min<uint32_t>(c->tier[1].max_pairs, n_ov - lo);
        HIP_TRY(hipMemcpyAsync(c->t0.d_sel_ids, ov.data() + lo, m * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(c->t0.d_est, ov_est.data() + lo, m * sizeof(int32_t), hipMemcpyHostToDevice, s));
        PairSel s1; s1.n = m; s1.ids = c->t0.d_sel_ids; s1.est = c->t0.d_est;
        if (c->kn.timing) { // where the time of the large-capacity tier goes (not added to the caller's stage times)
            mcx_stats t1; memset(&t1, 0, sizeof t1);
            rc = run_pairs(c, 1, R0, rb, paired, s1, d_recs, d_cig, &t1, true);
            fprintf(stderr, "[tier 1] %u pairs: seed %.2f sa %.2f cluster %.2f rescue %.2f build %.2f dp %.2f finish %.2f ms\n", m, t1.ms_seed, t1.ms_sa, t1.ms_cluster,
                    t1.ms_rescue, t1.ms_build, t1.ms_dp, t1.ms_finish);
            if (stats) { stats->dp_jobs += t1.dp_jobs; stats->dp_cells += t1.dp_cells; }
        } else
        rc = run_pairs(c, 1, R0, rb, paired, s1, d_recs, d_cig, stats, false);
        if (rc == kListOverflow) return fail(MCX_ERR_CAPACITY, "work list overflow in tier 1");
        if (rc) return rc;
        if (c->t0.h_cnt[CNT_OV]) return tier1_error(c, R0);
    }
    return 0;
}

// longest read of the batch (a read past max_read_len would overrun the per-read slots of every stage)
__global__ void k_max_read_len(const uint32_t *off, uint32_t n_reads, uint32_t *out)
{
    uint32_t m = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += gridDim.x * blockDim.x) m = max(m, off[r + 1] - off[r]);
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// a batch's reads into the context's own copy (bases 16 bytes at a time: d_bases is 16-byte aligned, the copy's room ends on a multiple of 16)
__global__ void k_keep_reads(const uint8_t *__restrict__ bases, const uint32_t *__restrict__ off, uint32_t n_reads, uint8_t *__restrict__ to_bases, uint32_t *__restrict__ to_off)
{
    const uint64_t total = off[n_reads], n16 = (total + 15) / 16, T = (uint64_t)gridDim.x * blockDim.x, t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = t; i < n16; i += T) ((U4 *)to_bases)[i] = ((const U4 *)bases)[i];
    for (uint64_t i = t; i <= n_reads; i += T) to_off[i] = off[i];
}

// tier 0's pair records: one per pair of the largest batch of this kind (allocated by the first batch that needs them, or ahead of it by mcx_ctx_create_fit)
int reserve_tier0(mcx_ctx *c, int paired, uint64_t n_reads)
{
    const uint64_t half = (c->max_reads + 1) / 2;
    const uint64_t want = (paired || n_reads <= half) ? half : c->max_reads; // (the single-end tail of an interleaved file fits the pairs' records)
    if (c->tier[0].max_pairs < want) {
        HIP_TRY(hipDeviceSynchronize());
        if (c->tier[0].state) { (void)hipFree(c->tier[0].state); c->tier[0].state = nullptr; c->tier[0].max_pairs = 0; }
        if (int rc = dmalloc(&c->tier[0].state, (size_t)c->tier[0].lay.stride * want)) return rc;
        c->tier[0].max_pairs = (uint32_t)want;
    }
    return 0;
}

extern "C" int mcx_batch_begin(mcx_ctx *c, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired, int32_t est0,
                               int64_t read_base, mcx_aln *d_aln, uint32_t *d_cigar, mcx_stats *stats)
{
    static_assert(sizeof(mcx_aln) == sizeof(AlnRec), "mcx_aln and AlnRec must have one layout");
    if (!c) return fail(MCX_ERR_ARG, "mcx_batch_begin: null argument");
    // what mcx_stream_next said of the batch it gave out: taken here, before anything can return, so that no later batch inherits it; it counts for the slot's own buffers only
    const bool vouched = c->lens_checked && d_off && d_off == c->lens_checked_off && d_bases == c->lens_checked_bases;
    c->lens_checked = false; c->lens_checked_off = nullptr; c->lens_checked_bases = nullptr;
    const mcx_ctx::PrePacked pre = c->pre;
    c->pre = mcx_ctx::PrePacked();
    if (!d_bases || !d_off || !d_aln || !d_cigar) return fail(MCX_ERR_ARG, "mcx_batch_begin: null argument");
    BatchRun &br = c->run;
    br.open = false;
    if (n_reads == 0) return fail(MCX_ERR_ARG, "mcx_batch_begin: empty batch");
    if (n_reads > c->max_reads) return fail(MCX_ERR_ARG, "batch larger than max_batch_reads");
    if (paired && (n_reads & 1)) return fail(MCX_ERR_ARG, "paired batch with an odd number of reads");
    if (paired && (read_base & 1)) return fail(MCX_ERR_ARG, "paired batch at an odd read_base");
    if ((uintptr_t)d_bases & 15) return fail(MCX_ERR_ARG, "mcx_batch_begin: d_bases must be 16-byte aligned");
    // (refused before anything is mapped or counted: readCount would move in profile_keys / profile_foreign before profile_accumulate refuses)
    if (c->prof_planes && c->prof_settled) return fail(MCX_ERR_ARG, "the profile has been settled (mcx_profile_settle / _finalize): attach it again before mapping more reads");
    HIP_TRY(hipSetDevice(c->idx->device));
    br.t0 = std::chrono::steady_clock::now();
    hipStream_t s = c->t0.stream;
    if (int rc = reserve_tier0(c, paired, n_reads)) return rc;
    br.rb.bases = d_bases; br.rb.off = d_off; br.rb.n_reads = n_reads;
    br.paired = paired; br.read_base = read_base;
    br.recs = (AlnRec *)d_aln; br.cig = d_cigar; br.stats = stats;
    br.cig_cap = (uint32_t)std::min<uint64_t>((uint64_t)MCX_CIGAR_POOL_WORDS(n_reads), 0xFFFFFFFFu); br.cig_words = 0;
    br.n_pairs = paired ? n_reads / 2 : n_reads;
    br.n_chunks = (br.n_pairs + kReadChunkSize / 2 - 1) / (kReadChunkSize / 2);
    br.mapped = 0; br.sums_valid = false; br.d_ok = br.d_ds = nullptr;
    c->tail.queued = c->tail.ran = false;
    HIP_TRY(hipMemsetAsync(c->d_batch_flags, 0, 4 * sizeof(uint32_t), s));
    c->mx.ready = false;
    if (c->mx.on) HIP_TRY(hipMemsetAsync(c->mx.d_cnt, 0, 4 * sizeof(uint32_t), s)); // (-m: the extras pool starts empty with every batch)
    c->last_paired = paired ? 1 : 0;
    if (vouched) c->t0.h_cnt[1] = (uint32_t)c->rlen_max; // (vouched for: no kernel, no wait at the start of the step — under the copies of the neighbouring batches such a wait takes milliseconds)
    else { // every read must fit the slots the context was sized for
        k_max_read_len<<<512, 256, 0, s>>>(d_off, n_reads, c->d_batch_flags + 1);
        HIP_TRY(hipMemcpyAsync(c->t0.h_cnt, c->d_batch_flags, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (c->t0.h_cnt[1] > (uint32_t)c->rlen_max)
            return fail(MCX_ERR_UNSUPPORTED, "a read of " + std::to_string(c->t0.h_cnt[1]) + " bases is longer than max_read_len (" + std::to_string(c->rlen_max) + ")");
    }
    { // the batch in 2-bit form, once; every seeding pass (tiers, replay) reads it
        HIP_TRY(hipEventRecord(c->ev_pack[0], s));
        const int tpr = ((int)c->t0.h_cnt[1] + 31) / 32 + 1; // (threads per read: for the batch's longest read, found above)
        br.longest = c->t0.h_cnt[1];
        // (the reads' flag bytes of the -vcf bookkeeping start here: bit 1 — a byte that is not an upper-case ACGT — is k_pack_reads'; MCX_PROF_BY_COLUMN:
        //  tests — every read is treated as if it held one, so that exact seeds are walked column by column like every other fragment)
        if (c->prof_planes) HIP_TRY(hipMemsetAsync(c->d_admit, c->kn.prof_by_column ? 2 : 0, ((size_t)n_reads + 3) & ~(size_t)3, s));
        if (vouched && pre.packed && pre.bases == d_bases && pre.paired == (paired ? 1 : 0) && !c->prof_planes) {
            // packed on its way in, under the batch before it (mcx_stream_submit_packed): the step starts with the search; the any-N word comes along
            c->packed_now = pre.packed; c->wpad_now = c->wpad; // (rows made on the way in keep the context's stride)
            HIP_TRY(hipMemcpyAsync(c->d_batch_flags + 3, pre.any_n, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        } else {
            // rows as long as the batch's longest read needs, not the context's: 80 bytes instead of 112 for 150 bases under max_read_len 256 — every pass of the
            // batch (tiers, late pairs, replays, the -vcf bookkeeping) strides over them by wpad_now
            c->packed_now = c->d_packed; c->wpad_now = std::min(c->wpad, (packed_words((int)br.longest) + 3) & ~3);
            pack_reads(br.rb, paired, c->wpad_now, tpr, c->d_packed, c->d_batch_flags + 3, c->prof_planes ? c->d_admit : nullptr, s);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev_pack[1], s));
    }
    c->later.kept_now = false;
    if (c->prof_planes && c->later.have && c->tail.want) { // (mcx_map_batch_dev's batches: one shard.)  The batch's reads for its bookkeeping, which runs when this call has long returned: copied beside the first kernels
        auto &L = c->later;
        L.kept_now = true;
        HIP_TRY(hipEventRecord(L.begun, s)); // (behind what the stream waits for: the batch's reads are in place)
        HIP_TRY(hipStreamWaitEvent(L.keep_stream, L.begun, 0));
        k_keep_reads<<<2048, 256, 0, L.keep_stream>>>(d_bases, d_off, n_reads, L.d_keep_bases, L.d_keep_off);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(L.kept, L.keep_stream));
    }
    int rc;
    br.ms_setup = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - br.t0).count();
    rc = run_selection(c, br.rb, paired, nullptr, nullptr, est0, br.n_pairs, br.recs, d_cigar, stats, true);
    br.t_begun = std::chrono::steady_clock::now();
    if (rc) return rc;
    if (c->tail.queued) memcpy(c->t0.h_cnt + CNT_COPY, c->tail.h + 2, sizeof br.hs); // (the pass queued the batch's tail and it stands: the statistics came with it)
    else { // seeding statistics (E, blocks, H of SURVEY.md 8d) before the per-read arrays are reused for the chunk sums
        unsigned long long *d_sum = (unsigned long long *)c->t0.d_cnt;
        HIP_TRY(hipMemsetAsync(c->t0.d_cnt, 0, CNT_N * sizeof(uint32_t), s));
        k_reduce_stats<<<kReduceStatsBlocks, 256, 0, s>>>(c->d_read_ext, c->d_read_blocks, n_reads, d_sum);
        HIP_TRY(hipMemcpyAsync(c->t0.h_cnt + CNT_COPY, d_sum, sizeof br.hs, hipMemcpyDeviceToHost, s)); // (read by batch_close, behind the sums' synchronisation: no round trip of its own)
    }
    br.open = true;
    return 0;
}

// Replay of the reference's avgDist feedback (ReadMapping.cpp:462, :538-539).  The
// device reduces the batch to per-chunk sums; the caller walks the chunk trajectory (a few thousand
// scalars; over all shards when there are several); the device lists the pairs whose chunk estimate
// falls outside their validity interval; those are re-run with the exact estimate until none is left.
extern "C" int mcx_batch_sums(mcx_ctx *c, uint32_t *n_chunks, const uint32_t **pairs, const uint32_t **dist, const uint32_t **len)
{
    if (!c || !c->run.open) return fail(MCX_ERR_ARG, "mcx_batch_sums: no batch in flight");
    BatchRun &br = c->run;
    hipStream_t s = c->t0.stream;
    HIP_TRY(hipSetDevice(c->idx->device));
    const uint32_t nc = br.n_chunks;
    if (br.sums_valid && br.ok.size() == nc && !c->kn.no_sums_cache) { // nothing was re-run since the last call (the closing round of a sharded step): the sums still stand
        if (n_chunks) *n_chunks = nc;
        if (pairs) *pairs = br.ok.data();
        if (dist) *dist = br.ds.data();
        if (len) *len = br.ds.data() + nc;
        return 0;
    }
    uint32_t *d_ok = c->d_read_ext, *d_ds = c->d_read_blocks; // the per-read stat arrays were reduced by mcx_batch_begin
    uint32_t *d_ls = d_ds + nc;                               // (2 * n_chunks <= n_reads)
    br.ok.resize(nc); br.ds.resize(2 * (size_t)nc);
    HIP_TRY(hipMemsetAsync(c->t0.d_cnt, 0, CNT_N * sizeof(uint32_t), s));
    k_chunk_sums<<<chunk_sums_blocks(nc), 256, 0, s>>>(c->d_pout, br.rb.off, br.n_pairs, kReadChunkSize / 2, br.paired ? 1 : 0, d_ok, d_ds, d_ls, c->t0.d_cnt + CNT_LF);
    HIP_TRY(hipMemcpyAsync(br.ok.data(), d_ok, nc * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(br.ds.data(), d_ds, 2 * (size_t)nc * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(c->t0.h_cnt, c->t0.d_cnt, CNT_N * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    br.mapped = c->t0.h_cnt[CNT_LF];
    br.sums_valid = true; br.d_ok = d_ok; br.d_ds = d_ds;
    if (n_chunks) *n_chunks = nc;
    if (pairs) *pairs = br.ok.data();
    if (dist) *dist = br.ds.data();
    if (len) *len = br.ds.data() + nc;
    return 0;
}

static int replay_listed(mcx_ctx *c, uint32_t n_redo, mcx_stats *stats);
extern "C" int mcx_batch_replay(mcx_ctx *c, const int32_t *est_chunk, uint32_t *n_redone, mcx_stats *stats)
{
    if (!c || !c->run.open || !est_chunk) return fail(MCX_ERR_ARG, "mcx_batch_replay: no batch in flight");
    BatchRun &br = c->run;
    hipStream_t s = c->t0.stream;
    HIP_TRY(hipSetDevice(c->idx->device));
    if (n_redone) *n_redone = 0;
    if (!br.paired) return 0;
    int32_t *d_est_chunk = (int32_t *)c->d_read_ext; // the sums are on the host
    HIP_TRY(hipMemcpyAsync(d_est_chunk, est_chunk, br.n_chunks * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(c->t0.d_cnt, 0, CNT_N * sizeof(uint32_t), s));
    k_check_est<<<2048, 256, 0, s>>>(c->d_pout, br.n_pairs, kReadChunkSize / 2, d_est_chunk, c->t0.d_sel_ids, c->t0.d_est, c->t0.d_cnt + CNT_OV, c->t0.ov_cap);
    HIP_TRY(hipMemcpyAsync(c->t0.h_cnt, c->t0.d_cnt, CNT_N * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t n_redo = c->t0.h_cnt[CNT_OV];
    if (n_redo == 0) return 0;
    if (int rc = replay_listed(c, n_redo, stats)) return rc;
    if (n_redone) *n_redone = n_redo;
    return 0;
}

// the pairs k_check_est listed (d_sel_ids, d_est: n_redo of them) through the path again, with their chunk's estimate
static int replay_listed(mcx_ctx *c, uint32_t n_redo, mcx_stats *stats)
{
    BatchRun &br = c->run;
    br.sums_valid = false;
    c->tail.queued = false; // (what the batch's tail brought is no longer the batch's state)
    if (n_redo > c->t0.ov_cap) return fail(MCX_ERR_CAPACITY, "avgDist replay: redo list overflow");
    if (stats) stats->replayed_pairs += (int64_t)n_redo;
    std::vector<uint32_t> redo(n_redo); std::vector<int32_t> redo_est(n_redo);
    HIP_TRY(hipMemcpy(redo.data(), c->t0.d_sel_ids, n_redo * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(redo_est.data(), c->t0.d_est, n_redo * 4, hipMemcpyDeviceToHost));
    // the list was appended with atomics: bring it into pair order (results do not depend on it)
    std::vector<std::pair<uint32_t, int32_t>> ord(n_redo);
    for (uint32_t i = 0; i < n_redo; i++) ord[i] = std::make_pair(redo[i], redo_est[i]);
    std::sort(ord.begin(), ord.end());
    for (uint32_t i = 0; i < n_redo; i++) { redo[i] = ord[i].first; redo_est[i] = ord[i].second; }
    return run_selection(c, br.rb, br.paired, &redo, &redo_est, 0, br.n_pairs, br.recs, br.cig, stats, false);
}

// The same feedback for a run on several shards with nothing but totals on the wire: a shard's chunks are checked against the
// trajectory that starts from the round's state plus the totals of the shards before it — the walk has a closed form (k_avg_walk), so nobody
// needs anybody else's chunks.
extern "C" int mcx_batch_totals(mcx_ctx *c, int64_t totals[2])
{
    if (!c || !totals) return fail(MCX_ERR_ARG, "mcx_batch_totals: null argument");
    totals[0] = totals[1] = 0;
    if (!c->run.open) return fail(MCX_ERR_ARG, "mcx_batch_totals: no batch in flight");
    uint32_t nc = 0;
    const uint32_t *ok = nullptr, *ds = nullptr;
    if (int rc = mcx_batch_sums(c, &nc, &ok, &ds, nullptr)) return rc;
    for (uint32_t k = 0; k < nc; k++) { totals[0] += ok[k]; totals[1] += ds[k]; }
    return 0;
}

extern "C" int mcx_batch_check(mcx_ctx *c, const int64_t state_before[3], int first_of_round, uint32_t *n_redone, mcx_stats *stats)
{
    if (!c || !state_before || !c->run.open) return fail(MCX_ERR_ARG, "mcx_batch_check: no batch in flight");
    BatchRun &br = c->run;
    if (n_redone) *n_redone = 0;
    if (!br.paired) return 0;
    HIP_TRY(hipSetDevice(c->idx->device));
    int rc;
    if ((!br.sums_valid || !br.d_ok) && (rc = mcx_batch_sums(c, nullptr, nullptr, nullptr, nullptr))) return rc; // (the chunk sums lie at br.d_ok / br.d_ds behind it)
    if ((rc = tail_reserve(c))) return rc;
    hipStream_t s = c->t0.stream;
    int32_t *d_est = (int32_t *)(c->tail.d + 8);
    HIP_TRY(hipMemsetAsync(c->tail.d, 0, 8 * sizeof(uint32_t), s));
    k_avg_walk<<<avg_walk_blocks(br.n_chunks), 1024, 0, s>>>(br.d_ok, br.d_ds, br.n_chunks, (long long)state_before[0], (long long)state_before[1], (long long)state_before[2], first_of_round ? 1 : 0, d_est);
    k_check_est<<<2048, 256, 0, s>>>(c->d_pout, br.n_pairs, kReadChunkSize / 2, d_est, c->t0.d_sel_ids, c->t0.d_est, c->tail.d, c->t0.ov_cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->tail.h, c->tail.d, 8 * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t n_redo = c->tail.h[0];
    if (n_redo == 0) return 0;
    if ((rc = replay_listed(c, n_redo, stats))) return rc;
    if (n_redone) *n_redone = n_redo;
    return 0;
}

// the state after a round whose batches held `pairs` proper pairs at the summed distance `dist` (mcx_avg_walk's end state in closed form)
extern "C" void mcx_avg_advance(int64_t st[3], int64_t pairs, int64_t dist, int64_t n_chunks)
{
    st[1] += pairs; st[2] += dist;
    if (n_chunks > 0 && st[1] > 1000) st[0] = (int64_t)(uint32_t)(int)(1. * (double)st[2] / (double)st[1] + .5);
}

// ---- -m: the extras of a batch in read order --------------------------------------------------------
// The finish kernel filled the pool in whatever order its wavefronts ran; per read it left {record offset, records, word offset, words}.
// count -> exclusive scan -> gather (the way k_dp_sort_count / _scan / _place order the DP lists) puts every read's lines behind the
// lines of the reads before it, and its CIGAR words likewise: the result does not depend on the order the pool was filled in.
__global__ void __launch_bounds__(256) k_mx_count(const uint4 *ref, uint32_t n_reads, uint32_t *recs, uint32_t *words)
{
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r <= n_reads; r += gridDim.x * blockDim.x) {
        const uint4 e = r < n_reads ? ref[r] : make_uint4(0u, 0u, 0u, 0u);
        recs[r] = e.y; words[r] = e.w;
    }
}

__global__ void __launch_bounds__(256) k_mx_gather(const uint4 *ref, uint32_t n_reads, const uint32_t *index, const uint32_t *windex, const AlnRec *pool,
                                                   const uint32_t *pool_cig, AlnRec *out, uint32_t *out_cig)
{
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += gridDim.x * blockDim.x) {
        const uint4 e = ref[r];
        const uint32_t at = index[r], wat = windex[r];
        for (uint32_t i = 0; i < e.y; i++) {
            AlnRec a = pool[e.x + i];
            a.pad[0] = (int32_t)(wat + ((uint32_t)a.pad[0] - e.z)); // cigar_off: into the ordered words
            out[at + i] = a;
        }
        for (uint32_t j = 0; j < e.w; j++) out_cig[wat + j] = pool_cig[e.z + j];
    }
}

// the pairs whose extras did not fit the pool, with the estimate they were mapped with (they are mapped again as they were)
__global__ void __launch_bounds__(256) k_mx_over(const uint4 *ref, uint32_t n_pairs, int nr, const PairOut *po, uint32_t *ids, int32_t *est, uint32_t *n, uint32_t cap)
{
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += gridDim.x * blockDim.x) {
        bool over = false;
        for (int s = 0; s < nr; s++) over |= (ref[(int64_t)p * nr + s].y & kMxOver) != 0;
        if (over) { const uint32_t at = atomicAdd(n, 1u); if (at < cap) { ids[at] = p; est[at] = po[p].est; } }
    }
}

static int mx_alloc_pool(mcx_ctx *c, uint32_t recs, uint32_t words, bool keep)
{
    auto &m = c->mx;
    AlnRec *p = nullptr; uint32_t *w = nullptr;
    int rc;
    if ((rc = dmalloc(&p, recs))) return rc;
    if ((rc = dmalloc(&w, words))) { (void)hipFree(p); return rc; }
    if (keep && m.d_pool) { // (what the batch's pairs wrote so far stays where their entries point)
        HIP_TRY(hipMemcpyAsync(p, m.d_pool, (size_t)std::min(m.rec_cap, recs) * sizeof(AlnRec), hipMemcpyDeviceToDevice, c->t0.stream));
        HIP_TRY(hipMemcpyAsync(w, m.d_pool_cig, (size_t)std::min(m.word_cap, words) * 4, hipMemcpyDeviceToDevice, c->t0.stream));
        HIP_TRY(hipStreamSynchronize(c->t0.stream));
    }
    if (m.d_pool) (void)hipFree(m.d_pool);
    if (m.d_pool_cig) (void)hipFree(m.d_pool_cig);
    m.d_pool = p; m.d_pool_cig = w; m.rec_cap = recs; m.word_cap = words;
    return 0;
}

extern "C" int mcx_ctx_set_multi(mcx_ctx *c, int on, uint32_t extra_cap)
{
    if (!c) return fail(MCX_ERR_ARG, "mcx_ctx_set_multi: null argument");
    if (c->run.open) return fail(MCX_ERR_ARG, "mcx_ctx_set_multi: a batch is in flight");
    HIP_TRY(hipSetDevice(c->idx->device));
    auto &m = c->mx;
    m.on = on != 0; m.ready = false;
    if (!m.on) return 0;
    int rc;
    const uint64_t nr1 = c->max_reads + 1;
    if (!m.d_ref) {
        if ((rc = dmalloc(&m.d_ref, c->max_reads))) return rc;
        if ((rc = dmalloc(&m.d_cnt, 4))) return rc;
        if ((rc = dmalloc(&m.d_counts, 2 * nr1))) return rc;
        if ((rc = dmalloc(&m.d_index, nr1))) return rc;
        if ((rc = dmalloc(&m.d_windex, nr1))) return rc;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, m.tmp_bytes, m.d_counts, m.d_index, (int64_t)nr1));
        if ((rc = dmalloc((uint8_t **)&m.d_tmp, m.tmp_bytes))) return rc;
    }
    // (default: a line for every 16th read — the bench genome's batches need far fewer —, eight CIGAR words a line; a batch that needs more makes it grow)
    const uint32_t recs = std::min<uint32_t>(extra_cap ? extra_cap : (uint32_t)std::max<uint64_t>(4096, c->max_reads / 16), 1u << 28);
    const uint32_t words = recs * 8u; // (below 2^31)
    if (recs != m.rec_cap || words != m.word_cap) return mx_alloc_pool(c, recs, words, false);
    return 0;
}

// (-m, at the close of a batch) pairs whose extras did not fit are mapped again into a grown pool; then the extras are put in read order
static int multi_close(mcx_ctx *c)
{
    auto &m = c->mx;
    BatchRun &br = c->run;
    hipStream_t s = c->t0.stream;
    const uint32_t n_reads = br.rb.n_reads, nr = br.paired ? 2 : 1;
    int rc;
    for (int round = 0;; round++) {
        uint32_t h[4];
        HIP_TRY(hipMemcpyAsync(h, m.d_cnt, sizeof h, hipMemcpyDeviceToHost, s)); // (behind the batch's last finish kernel)
        HIP_TRY(hipStreamSynchronize(s));
        if (h[0] <= m.rec_cap && h[1] <= m.word_cap) break;
        if (round == 4) return fail(MCX_ERR_CAPACITY, "-m: the extras pool did not settle");
        // everything taken so far (stale entries of re-run pairs included) plus as much again for the pairs that are mapped again
        const uint32_t recs = std::max(m.rec_cap, 2 * h[0] + 1024), words = std::max(m.word_cap, 2 * h[1] + 8192);
        if (c->kn.timing || getenv("MCX_ALLOC_LOG")) fprintf(stderr, "[mcx] the -m extras pool grows from %u to %u lines (%u to %u CIGAR words): the batch asked for %u lines, %u words\n",
                                                             m.rec_cap, recs, m.word_cap, words, h[0], h[1]);
        if ((rc = mx_alloc_pool(c, recs, words, true))) return rc;
        HIP_TRY(hipMemsetAsync(m.d_cnt + 2, 0, 4, s));
        k_mx_over<<<(br.n_pairs + 255) / 256, 256, 0, s>>>(m.d_ref, br.n_pairs, (int)nr, c->d_pout, c->t0.d_sel_ids, c->t0.d_est, m.d_cnt + 2, c->t0.ov_cap);
        HIP_TRY(hipGetLastError());
        uint32_t n_over = 0;
        HIP_TRY(hipMemcpyAsync(&n_over, m.d_cnt + 2, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (n_over && (rc = replay_listed(c, n_over, nullptr))) return rc;
    }
    if ((uint64_t)n_reads + 1 > c->max_reads + 1) return fail(MCX_ERR_ARG, "-m: batch larger than the context");
    uint32_t *cr = m.d_counts, *cw = m.d_counts + c->max_reads + 1;
    const unsigned gb = std::min<uint32_t>(4096u, (n_reads + 256) / 256);
    k_mx_count<<<gb, 256, 0, s>>>(m.d_ref, n_reads, cr, cw);
    HIP_TRY(hipGetLastError());
    size_t tb = m.tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(m.d_tmp, tb, cr, m.d_index, (int64_t)n_reads + 1, s));
    tb = m.tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(m.d_tmp, tb, cw, m.d_windex, (int64_t)n_reads + 1, s));
    uint32_t tot[2];
    HIP_TRY(hipMemcpyAsync(&tot[0], m.d_index + n_reads, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&tot[1], m.d_windex + n_reads, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (tot[0] > m.out_cap || tot[1] > m.out_wcap) {
        if (m.d_out) (void)hipFree(m.d_out);
        if (m.d_out_cig) (void)hipFree(m.d_out_cig);
        m.d_out = nullptr; m.d_out_cig = nullptr; m.out_cap = m.out_wcap = 0;
        const uint32_t want = std::max(tot[0], m.rec_cap / 4), wwant = std::max(tot[1], m.word_cap / 4);
        if ((rc = dmalloc(&m.d_out, (size_t)want + 1))) return rc;
        if ((rc = dmalloc(&m.d_out_cig, (size_t)wwant + 1))) return rc;
        m.out_cap = want; m.out_wcap = wwant;
    }
    if (tot[0]) k_mx_gather<<<gb, 256, 0, s>>>(m.d_ref, n_reads, m.d_index, m.d_windex, m.d_pool, m.d_pool_cig, m.d_out, m.d_out_cig);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    m.n_reads = n_reads; m.n_recs = tot[0]; m.n_words = tot[1]; m.ready = true;
    return 0;
}

extern "C" int mcx_multi_lines(mcx_ctx *c, const uint32_t **d_index, const mcx_aln **d_recs, const uint32_t **d_cigar, uint32_t *n_recs, uint32_t *n_words)
{
    if (!c) return fail(MCX_ERR_ARG, "mcx_multi_lines: null argument");
    if (!c->mx.on || !c->mx.ready) return fail(MCX_ERR_ARG, "mcx_multi_lines: no batch was mapped with -m on (mcx_ctx_set_multi)");
    if (d_index) *d_index = c->mx.d_index;
    if (d_recs) *d_recs = (const mcx_aln *)c->mx.d_out;
    if (d_cigar) *d_cigar = c->mx.d_out_cig;
    if (n_recs) *n_recs = c->mx.n_recs;
    if (n_words) *n_words = c->mx.n_words;
    return 0;
}

extern "C" int mcx_multi_copy(mcx_ctx *c, uint32_t *index, mcx_aln *recs, uint32_t *cigar)
{
    if (!c || !index) return fail(MCX_ERR_ARG, "mcx_multi_copy: null argument");
    if (!c->mx.on || !c->mx.ready) return fail(MCX_ERR_ARG, "mcx_multi_copy: no batch was mapped with -m on (mcx_ctx_set_multi)");
    const auto &m = c->mx;
    if ((m.n_recs && !recs) || (m.n_words && !cigar)) return fail(MCX_ERR_ARG, "mcx_multi_copy: null argument");
    HIP_TRY(hipSetDevice(c->idx->device));
    HIP_TRY(hipMemcpyAsync(index, m.d_index, ((size_t)m.n_reads + 1) * 4, hipMemcpyDeviceToHost, c->t0.stream));
    if (m.n_recs) HIP_TRY(hipMemcpyAsync(recs, m.d_out, (size_t)m.n_recs * sizeof(AlnRec), hipMemcpyDeviceToHost, c->t0.stream));
    if (m.n_words) HIP_TRY(hipMemcpyAsync(cigar, m.d_out_cig, (size_t)m.n_words * 4, hipMemcpyDeviceToHost, c->t0.stream));
    HIP_TRY(hipStreamSynchronize(c->t0.stream));
    return 0;
}

bool mcx_ctx_multi(const mcx_ctx *c) { return c->mx.on; }

// what both ways of closing a batch share: the long-CIGAR pool, statistics
static int batch_close(mcx_ctx *c, mcx_stats *stats)
{
    BatchRun &br = c->run;
    int rc = 0;
    if (c->mx.on && (rc = multi_close(c))) return rc; // (-m: before the sums — pairs it maps again mark them stale)
    if (!br.sums_valid && (rc = mcx_batch_sums(c, nullptr, nullptr, nullptr, nullptr))) return rc;
    {
        uint32_t fl[4] = {0, 0, 0, 0};
        if (c->tail.queued) memcpy(fl, c->tail.h + 8, sizeof fl); // (nothing ran since the batch's tail was copied back)
        else HIP_TRY(hipMemcpy(fl, c->d_batch_flags, sizeof fl, hipMemcpyDeviceToHost));
        if (fl[2] || fl[0] > br.cig_cap) return fail(MCX_ERR_CAPACITY, "the batch's CIGAR pool (" + std::to_string(MCX_CIGAR_STRIDE) + " operations per read on average + " + std::to_string(MCX_CIGAR_SLACK) + ") ran over");
        br.cig_words = fl[0];
    }
    if (stats) {
        int64_t pairs = 0, dist_sum = 0, len_sum = 0;
        if (br.paired) for (uint32_t k = 0; k < br.n_chunks; k++) { pairs += br.ok[k]; dist_sum += br.ds[k]; len_sum += br.ds[br.n_chunks + k]; }
        stats->reads += br.rb.n_reads; stats->mapped += br.mapped; stats->pairs += pairs; stats->pair_dist_sum += dist_sum; stats->pair_len_sum += len_sum;
        memcpy(br.hs, c->t0.h_cnt + CNT_COPY, sizeof br.hs);
        stats->fm_ext_steps += (int64_t)br.hs[0]; stats->fm_blocks += (int64_t)br.hs[1]; stats->sa_hits += (int64_t)br.hs[2];
        float ms_pack = 0;
        if (hipEventElapsedTime(&ms_pack, c->ev_pack[0], c->ev_pack[1]) == hipSuccess) stats->ms_encode += ms_pack; // k_pack_reads
    }
    if (!c->dp_grown && c->job2_seen) return dp_scratch_grow(c, c->job2_seen); // (the batch is through: nothing holds the scratch)
    return 0;
}

extern "C" int mcx_batch_end(mcx_ctx *c, mcx_stats *stats)
{
    if (!c || !c->run.open) return fail(MCX_ERR_ARG, "mcx_batch_end: no batch in flight");
    HIP_TRY(hipSetDevice(c->idx->device));
    int rc = batch_close(c, stats);
    if (rc == 0 && c->prof_planes && c->later.have && c->later.kept_now) rc = profile_queue(c); // one shard: the batch's own keys decide the duplicate cap — behind the batch, under the next one's kernels
    else if (rc == 0 && c->prof_planes && (rc = profile_collect(c)) == 0) {
        const auto t0 = std::chrono::steady_clock::now();
        rc = profile_keys(c);
        const auto t1 = std::chrono::steady_clock::now();
        if (rc == 0) rc = profile_accumulate(c, nullptr, 0, 0, 0);
        if (c->kn.timing) {
            auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            fprintf(stderr, "[mcx profile] mapping %.2f ms, keys %.2f ms, accumulate %.2f ms\n", ms(c->run.t0, t0), ms(t0, t1), ms(t1, std::chrono::steady_clock::now()));
        }
    }
    c->run.open = false;
    if (rc == 0 && stats) stats->ms_total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c->run.t0).count();
    return rc;
}

extern "C" int mcx_batch_end_keys(mcx_ctx *c, mcx_stats *stats, const uint64_t **keys, uint64_t *n_keys)
{
    if (!c || !c->run.open || !keys || !n_keys) return fail(MCX_ERR_ARG, "mcx_batch_end_keys: no batch in flight");
    if (!c->prof_planes) return fail(MCX_ERR_ARG, "mcx_batch_end_keys: no profile attached");
    HIP_TRY(hipSetDevice(c->idx->device));
    if (int e = profile_collect(c)) { c->run.open = false; return e; }
    int rc = batch_close(c, stats);
    if (rc == 0) rc = profile_keys(c);
    if (rc) { c->run.open = false; return rc; }
    // the valid keys sort to the front
    if (c->h_keys_cap < c->run.n_keys) {
        mcx_pinned_free(c->h_keys);
        c->h_keys_cap = std::max<uint64_t>(c->run.n_keys, c->max_reads);
        c->h_keys = (uint64_t *)mcx_pinned_alloc(c->h_keys_cap * sizeof(uint64_t));
        if (!c->h_keys) { c->h_keys_cap = 0; c->run.open = false; return fail(MCX_ERR_DEVICE, "cannot allocate pinned host memory"); }
    }
    if (c->run.n_keys) HIP_TRY(hipMemcpy(c->h_keys, c->run.d_sorted_keys, c->run.n_keys * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *keys = c->h_keys; *n_keys = c->run.n_keys;
    c->run.keys_out = true;
    return 0;
}

extern "C" int mcx_batch_accumulate(mcx_ctx *c, const uint64_t *all_keys, uint64_t n_all, uint32_t slot_stride, uint32_t own_slot)
{
    if (!c || !c->prof_planes) return fail(MCX_ERR_ARG, "mcx_batch_accumulate: no profile attached");
    HIP_TRY(hipSetDevice(c->idx->device));
    if (int e = profile_collect(c)) return e;
    if (own_slot == 0xFFFFFFFFu) { // a shard without reads in this round: the others' admissions still count
        if (c->run.open) return fail(MCX_ERR_ARG, "mcx_batch_accumulate: a batch is in flight");
        return profile_foreign(c, all_keys, n_all);
    }
    if (!c->run.open || !c->run.keys_out) return fail(MCX_ERR_ARG, "mcx_batch_accumulate: call mcx_batch_end_keys first");
    int rc = profile_accumulate(c, all_keys, n_all, slot_stride, own_slot);
    c->run.open = false; c->run.keys_out = false;
    if (rc == 0 && c->run.stats) c->run.stats->ms_total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c->run.t0).count();
    return rc;
}

extern "C" int mcx_map_batch_dev(mcx_ctx *c, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired,
                                 int64_t avg[4], mcx_aln *d_aln, uint32_t *d_cigar, mcx_stats *stats)
{
    if (!c) return fail(MCX_ERR_ARG, "mcx_map_batch_dev: null argument");
    auto unvouch = [&]() { c->lens_checked = false; c->lens_checked_off = nullptr; c->lens_checked_bases = nullptr; c->pre = mcx_ctx::PrePacked(); }; // (a return before mcx_batch_begin: nothing said of this batch outlives it)
    if (!d_bases || !d_off || !d_aln || !d_cigar || !avg) { unvouch(); return fail(MCX_ERR_ARG, "mcx_map_batch_dev: null argument"); }
    if (n_reads == 0) { unvouch(); return 0; }
    if (paired && (avg[3] % kReadChunkSize)) { unvouch(); return fail(MCX_ERR_ARG, "batches must start on a 200-read chunk boundary"); }
    // (one stream, one trajectory: what follows the batch's kernels — statistics, per-chunk sums, the walk, the check of every pair's estimate —
    //  is queued behind them by the pass itself, queue_batch_tail)
    c->tail.want = true; c->tail.state0[0] = avg[0]; c->tail.state0[1] = avg[1]; c->tail.state0[2] = avg[2];
    const auto t_in = std::chrono::steady_clock::now();
    int rc = mcx_batch_begin(c, d_bases, d_off, n_reads, paired, (int32_t)((uint32_t)avg[0] * 1.5), avg[3], d_aln, d_cigar, stats);
    c->tail.want = false;
    if (rc) return rc;
    int64_t after[3] = {avg[0], avg[1], avg[2]};
    bool tail = c->tail.queued;
    if (tail) { // the sums are here already (and the mapped reads' count, the CIGAR pool's state)
        BatchRun &br = c->run;
        const uint32_t nc = br.n_chunks, *h = c->tail.h;
        br.ok.assign(h + 18, h + 18 + nc); br.ds.assign(h + 18 + nc, h + 18 + 3 * nc);
        br.mapped = h[1]; br.sums_valid = true;
    }
    if (paired) {
        std::vector<int32_t> est(c->run.n_chunks);
        for (int iter = 0;; iter++) {
            uint32_t nc = 0, n_redo = 0;
            const uint32_t *ok = nullptr, *ds = nullptr;
            if ((rc = mcx_batch_sums(c, &nc, &ok, &ds, nullptr))) return rc;
            after[0] = avg[0]; after[1] = avg[1]; after[2] = avg[2];
            mcx_avg_walk(after, ok, ds, nc, est.data());
            if (tail && iter == 0 && memcmp(est.data(), c->tail.h + 18 + 3 * nc, (size_t)nc * 4) == 0) {
                // the device walked the same trajectory: its list of the pairs whose estimate moved is the list
                n_redo = c->tail.h[0];
                const auto tq = std::chrono::steady_clock::now();
                if (n_redo && (rc = replay_listed(c, n_redo, stats))) return rc;
                if (n_redo && c->kn.timing) fprintf(stderr, "[mcx] avgDist: %u pairs of the batch re-run (the device's list), %.2f ms\n", n_redo, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq).count());
                if (n_redo == 0) break;
                continue;
            }
            if (tail && iter == 0 && c->kn.timing) fprintf(stderr, "[mcx] the device's walk of the batch's chunks differs from the host's: the host's is taken\n");
            const auto tq = std::chrono::steady_clock::now();
            if ((rc = mcx_batch_replay(c, est.data(), &n_redo, stats))) return rc;
            if (c->kn.timing && (n_redo || iter)) fprintf(stderr, "[mcx] avgDist: pass %d, %u pairs re-run, %.2f ms\n", iter, n_redo, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tq).count());
            if (n_redo == 0) break;
            if (iter == 63) return fail(MCX_ERR_CAPACITY, "avgDist replay did not converge");
        }
    }
    const auto t_loop = std::chrono::steady_clock::now();
    if ((rc = mcx_batch_end(c, stats))) return rc;
    if (c->kn.timing) {
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        const auto t_out = std::chrono::steady_clock::now();
        if (ms(t_in, t_out) > 30) fprintf(stderr, "[mcx] a slow batch (%u reads): set-up %.2f ms, first pass %.2f ms, avgDist %.2f ms, closing %.2f ms\n", n_reads, c->run.ms_setup, ms(t_in, c->run.t_begun) - c->run.ms_setup, ms(c->run.t_begun, t_loop), ms(t_loop, t_out));
    }
    avg[0] = after[0]; avg[1] = after[1]; avg[2] = after[2];
    avg[3] += n_reads;
    return 0;
}

// host buffers -> the context's staging arrays in HBM (what mcx_map_batch and the file front end hand the step API)
int mcx_stage_in(mcx_ctx *c, const uint8_t *bases, const uint32_t *off, uint32_t n_reads, const uint8_t **d_bases, const uint32_t **d_off,
                 mcx_aln **d_aln, uint32_t **d_cigar)
{
    if (n_reads > c->max_reads) return fail(MCX_ERR_ARG, "batch larger than max_batch_reads");
    HIP_TRY(hipSetDevice(c->idx->device));
    int rc;
    if (!c->d_bases) {
        if ((rc = dmalloc(&c->d_bases, c->max_bases + 64))) return rc;
        if ((rc = dmalloc(&c->d_off, c->max_reads + 1))) return rc;
        if ((rc = dmalloc(&c->d_recs, c->max_reads))) return rc;
        if ((rc = dmalloc(&c->d_cig, MCX_CIGAR_POOL_WORDS(c->max_reads)))) return rc;
    }
    if (off[n_reads] > c->max_bases) return fail(MCX_ERR_ARG, "batch holds more bases than max_batch_reads * max_read_len");
    HIP_TRY(hipMemcpyAsync(c->d_bases, bases, off[n_reads], hipMemcpyHostToDevice, c->t0.stream));
    HIP_TRY(hipMemcpyAsync(c->d_off, off, (size_t)(n_reads + 1) * 4, hipMemcpyHostToDevice, c->t0.stream));
    *d_bases = c->d_bases; *d_off = c->d_off; *d_aln = (mcx_aln *)c->d_recs; *d_cigar = c->d_cig;
    return 0;
}

int mcx_stage_out(mcx_ctx *c, uint32_t n_reads, mcx_aln *aln, uint32_t *cigar)
{
    HIP_TRY(hipSetDevice(c->idx->device));
    HIP_TRY(hipMemcpyAsync(aln, c->d_recs, (size_t)n_reads * sizeof(AlnRec), hipMemcpyDeviceToHost, c->t0.stream));
    if (c->run.cig_words) HIP_TRY(hipMemcpyAsync(cigar, c->d_cig, (size_t)c->run.cig_words * 4, hipMemcpyDeviceToHost, c->t0.stream));
    HIP_TRY(hipStreamSynchronize(c->t0.stream));
    return 0;
}

extern "C" int mcx_map_batch(mcx_ctx *c, const uint8_t *bases, const uint32_t *off, uint32_t n_reads, int paired,
                             int64_t avg[4], mcx_aln *aln, uint32_t *cigar, mcx_stats *stats)
{
    if (!c || !bases || !off || !aln || !cigar) return fail(MCX_ERR_ARG, "mcx_map_batch: null argument");
    if (n_reads == 0) return 0;
    const uint8_t *d_bases; const uint32_t *d_off; mcx_aln *d_aln; uint32_t *d_cig;
    int rc = mcx_stage_in(c, bases, off, n_reads, &d_bases, &d_off, &d_aln, &d_cig);
    if (rc) return rc;
    if ((rc = mcx_map_batch_dev(c, d_bases, d_off, n_reads, paired, avg, d_aln, d_cig, stats))) return rc;
    return mcx_stage_out(c, n_reads, aln, cigar);
}

// ---------------------------------------------------------------------------------------------
// per-call drop-ins: BWT_Search and nw/ksw2 alignment as batches
// ---------------------------------------------------------------------------------------------
__global__ void k_bwt_search(IndexView ix, const uint8_t *seqs, const uint32_t *off, const int32_t *start, uint32_t n,
                             int32_t *len, int32_t *freq, uint64_t *loc)
{
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *seq = seqs + off[i];
    const int stop = (int)(off[i + 1] - off[i]);
    // BWT_Search (bwt_search.cpp:121-164), one call
    int p0 = start[i], c0 = seq[p0];
    uint64_t x0 = ix.L2[c0] + 1, x1 = ix.L2[3 - c0] + 1, x2 = ix.L2[c0 + 1] - ix.L2[c0];
    int pos;
    for (pos = p0 + 1; pos < stop; pos++) {
        int c = seq[pos];
        if (c > 3) break;
        uint64_t tk[4], tl[4]; int nb;
        fm_2occ4(ix, x1 - 1, x1 - 1 + x2, tk, tl, nb);
        int b = 3 - c;
        uint64_t n2 = tl[b] - tk[b];
        if (n2 == 0) break;
        uint64_t n0 = x0 + ((x1 <= ix.primary && x1 + x2 - 1 >= ix.primary) ? 1 : 0);
        for (int bb = 3; bb > b; bb--) n0 += tl[bb] - tk[bb];
        x0 = n0; x1 = ix.L2[b] + 1 + tk[b]; x2 = n2;
    }
    int l = pos - p0, f = 0;
    if (l >= kMinSeedLength && x2 <= (uint64_t)kOccThr) f = (int)x2;
    len[i] = l; freq[i] = f;
    for (int k = 0; k < f; k++) { int lf = 0; loc[(uint64_t)i * kOccThr + k] = fm_sa(ix, x0 + k, lf); }
}

extern "C" int mcx_bwt_search_batch(mcx_ctx *c, const uint8_t *seqs, const uint32_t *seq_off, const int32_t *start,
                                    uint32_t n, int32_t *len, int32_t *freq, uint64_t *loc)
{
    if (!c || !seqs || !seq_off || !start || !len || !freq || !loc) return fail(MCX_ERR_ARG, "mcx_bwt_search_batch: null argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->idx->device));
    uint8_t *d_seq = nullptr; uint32_t *d_off = nullptr; int32_t *d_start = nullptr, *d_len = nullptr, *d_freq = nullptr; uint64_t *d_loc = nullptr;
    int rc = 0;
    size_t nb = seq_off[n];
    if ((rc = dmalloc(&d_seq, nb + 16)) || (rc = dmalloc(&d_off, (size_t)n + 1)) || (rc = dmalloc(&d_start, n)) ||
        (rc = dmalloc(&d_len, n)) || (rc = dmalloc(&d_freq, n)) || (rc = dmalloc(&d_loc, (size_t)n * kOccThr))) return rc;
    HIP_TRY(hipMemcpy(d_seq, seqs, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_off, seq_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_start, start, (size_t)n * 4, hipMemcpyHostToDevice));
    k_bwt_search<<<(n + 255) / 256, 256, 0, c->t0.stream>>>(c->idx->view, d_seq, d_off, d_start, n, d_len, d_freq, d_loc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->t0.stream));
    HIP_TRY(hipMemcpy(len, d_len, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(freq, d_freq, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(loc, d_loc, (size_t)n * kOccThr * 8, hipMemcpyDeviceToHost));
    (void)hipFree(d_seq); (void)hipFree(d_off); (void)hipFree(d_start); (void)hipFree(d_len); (void)hipFree(d_freq); (void)hipFree(d_loc);
    return 0;
}

// ---------------------------------------------------------------------------------------------
// files in, SAM out: MapCaller -i <prefix> -f A [-f2 B] -sam out  (main.cpp:212-321, Mapping() ReadMapping.cpp:689-747)
// ---------------------------------------------------------------------------------------------
extern "C" int mcx_cigar_words(mcx_ctx *c, uint32_t *n_words)
{
    if (!c || !n_words) return fail(MCX_ERR_ARG, "mcx_cigar_words: null argument");
    *n_words = c->run.cig_words;
    return 0;
}

const mcx_index *mcx_ctx_index(const mcx_ctx *c) { return c->idx; }
int mcx_ctx_max_read_len(const mcx_ctx *c) { return c->rlen_max; }
bool mcx_ctx_has_profile(const mcx_ctx *c) { return c->prof_planes != nullptr; }
uint64_t mcx_ctx_max_reads(const mcx_ctx *c) { return c->max_reads; }
void **mcx_ctx_files_slot(mcx_ctx *c, void (*drop)(void *)) { c->files_drop = drop; return &c->files_state; }
void **mcx_ctx_sam_slot(mcx_ctx *c, void (*drop)(void *)) { c->sam_drop = drop; return &c->sam_state; }
void *mcx_ctx_stream(mcx_ctx *c) { return (void *)c->t0.stream; }
void *mcx_pinned_alloc(size_t bytes) { void *p = nullptr; return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr; }
void mcx_pinned_free(void *p) { if (p) (void)hipHostFree(p); }
