// mapcaller_amd/csrc/mcx_dp_stage.hip — the gapped extensions of a pass (ksw2_alignment / nw_alignment): the DP job lists that
// k_build / k_build_wave filled, one kernel per size class.
//   k_dp_lane2<K, NW>        two problems per lane in 16-bit halves (mcx_dp_lane2.h): the three short lists, and the two long ones
//                            from kDpLaneMin problems on, dealt to the wavefronts by shape (k_dp_sort_count / _scan / _place)
//   k_dp_group<K>            a wavefront per problem, the walks of a group at once: the two long lists while they are short
//   k_dp_sel<16>             a wavefront per problem: the largest problems
//   k_dp_small / _tiny / _half   MCX_DP_BY_WAVE: the wavefront forms of the short lists (mcx_dp.h), the reference path of the parity tests
//   k_extend<K>              mcx_extend_batch: the same sweeps on strings the caller hands over
// Reached through launch_dp(), the sizing helpers lane_short_words() / lane_stride_words() (mcx_ctx.h) and the mcx_extend_batch ABI.
#include "mcx_ctx.h"

// LDS per problem is sized per class: the small classes are latency-bound (a chain of dependent
// fetches per problem), so what counts is how many problems a CU holds at once; the rare problem
// that does not fit its class's LDS keeps its sequences / traceback in the workgroup's HBM scratch.
template <int K> struct DpLds { static constexpr int seq = kDpLdsSeq, dir = kDpLdsDir; };
template <> struct DpLds<1> { static constexpr int seq = 512, dir = 4096; }; // targets <= 64: e.g. 48 x 48 fits
template <> struct DpLds<4> { static constexpr int seq = 1024, dir = 3072; }; // targets 65..256: the traceback of most does not fit 12 KB either — more problems per CU instead

// one problem on the W lanes of a group (W = 64: the wave; 32: a half wave): stage the two strings,
// sweep, trace back, hand the column string to the fragment
template <int K, int W>
static __device__ __forceinline__ void dp_run_job(const Ctx &cx, const JobSink &sink, uint32_t jb, const DpJob &job, const ReadBatch &rb,
                                                  const PairSel &sel, const DpBuf &b)
{
    const int nr = cx.pm.paired ? 2 : 1;
    const int lane = threadIdx.x & (W - 1);
    const uint32_t read = sel_pair(sel, job.pair) * nr + job.slot;
    ReadRef rd;
    rd.ascii = rb.bases + rb.off[read]; rd.rlen = (int)(rb.off[read + 1] - rb.off[read]); rd.flipped = (cx.pm.paired && job.slot == 1) ? 1 : 0;
    // q = read fragment, t = genome fragment; both reversed on the reverse strand (the
    // reference also complements both, which no comparison can see)
    for (int i = lane; i < job.rLen; i += W) b.q[i] = (uint8_t)read_code(rd, job.rev ? job.rPos + job.rLen - 1 - i : job.rPos + i);
    for (int i = lane; i < job.gLen; i += W) b.t[i] = (uint8_t)ref_code(cx.ix, job.rev ? job.gPos + job.gLen - 1 - i : job.gPos + i);
    dp_sync<W>();
    PairState st = pair_state(cx.state, cx.lay, cx.caps, job.pair);
    int score = 0;
    DpSummary *sum = cx.dp_summary ? (DpSummary *)(st.ops + job.ops_off - kDpSum) : nullptr; // (stage_build left room for it)
    const int w = dp_core<K, W>(cx.pm.use_nw != 0, job.rLen, job.gLen, b, st.ops + job.ops_off, &score, sum, (uint32_t)job.ops_off);
    if (lane == 0) {
        Frag f = st.frags[job.frag]; // one fetch, one store (the fields share two words)
        f.ops_off = job.ops_off + w;
        f.ops_len = job.rLen + job.gLen - w;
        f.meta = sum ? (uint32_t)((job.ops_off - kDpSum) >> 3) + 1u : 0u;
        st.frags[job.frag] = f;
        sink.jobs[jb].score = score;
    }
    dp_sync<W>();
}

template <int K>
__global__ void __launch_bounds__(64) k_dp_sel(Ctx cx, JobSink sink, ReadBatch rb, PairSel sel, uint8_t *scratch,
                                               uint64_t scratch_stride)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[DpLds<K>::seq + DpLds<K>::dir];
    uint8_t *spill = scratch + (uint64_t)blockIdx.x * scratch_stride;
    const uint32_t n = min(*sink.count, sink.cap);
    for (uint32_t jb = blockIdx.x; jb < n; jb += gridDim.x) {
        const DpJob job = sink.jobs[jb];
        dp_run_job<K, 64>(cx, sink, jb, job, rb, sel, dp_buffers(job.rLen, job.gLen, lds, spill, DpLds<K>::seq, DpLds<K>::dir));
    }
}

// The one-wavefront classes, a group of problems at a time.  k_dp_sel sweeps a problem and then lets lane 0 walk its traceback
// while 63 lanes look on — as many vector instructions as the sweep itself.  Here a wavefront sweeps up to 64 problems one after
// the other, every sweep leaving its traceback bytes (and the two strings) in the wavefront's stretch of an HBM scratch that
// stays in L2, and then walks the 64 tracebacks at once, one per lane.  Same bytes, same walks, same column strings.
constexpr int kDpGroup = 64;
struct DpGroupSlot { uint32_t off; int32_t score; }; // where a problem's strings and traceback bytes lie in the wave's scratch; its sweep's score

template <int K>
__global__ void __launch_bounds__(64) k_dp_group(Ctx cx, JobSink sink, ReadBatch rb, PairSel sel, uint8_t *scratch, uint64_t scratch_stride, uint32_t max_n)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[DpLds<K>::seq];
    __shared__ DpGroupSlot slot[kDpGroup];
    uint8_t *mine = scratch + (uint64_t)blockIdx.x * scratch_stride;
    const uint32_t n = min(*sink.count, sink.cap);
    if (n >= max_n) return; // (a long list: k_dp_lane2's)
    const int nr = cx.pm.paired ? 2 : 1;
    const int lane = threadIdx.x;
    const bool nw = cx.pm.use_nw != 0;
    // (few problems: small groups, so that every wavefront of the launch gets some; many: whole groups of 64)
    uint32_t group = (n + 2 * gridDim.x - 1) / (2 * gridDim.x);
    group = group < 8 ? 8 : (group > (uint32_t)kDpGroup ? (uint32_t)kDpGroup : group);
    for (uint32_t slice = blockIdx.x * group; slice < n; slice += gridDim.x * group) {
        const uint32_t slice_end = min(slice + group, n);
        for (uint32_t jb0 = slice; jb0 < slice_end;) {
            // ---- the sweeps, one problem after the other, all lanes on each; the group ends when the wave's stretch of scratch is full ----
            uint32_t used = 0;
            int g_n = 0;
            for (; jb0 + g_n < slice_end; g_n++) {
                const DpJob job = sink.jobs[jb0 + g_n];
                const uint32_t need = (uint32_t)((job.rLen + job.gLen + 15) & ~15) + (uint32_t)(job.rLen + job.gLen - 1) * (uint32_t)job.gLen;
                if (g_n > 0 && used + need > scratch_stride) break; // (a stretch holds the largest problem of its class)
                const uint32_t read = sel_pair(sel, job.pair) * nr + job.slot;
                ReadRef rd;
                rd.ascii = rb.bases + rb.off[read]; rd.rlen = (int)(rb.off[read + 1] - rb.off[read]); rd.flipped = (cx.pm.paired && job.slot == 1) ? 1 : 0;
                uint8_t *gq = mine + used, *gt = gq + job.rLen, *gdir = gq + ((job.rLen + job.gLen + 15) & ~15);
                DpBuf b;
                const bool in_lds = job.rLen <= DpLds<K>::seq / 2 && job.gLen <= DpLds<K>::seq / 2;
                b.q = in_lds ? lds : gq; b.t = in_lds ? lds + DpLds<K>::seq / 2 : gt; b.dir = gdir;
                for (int i = lane; i < job.rLen; i += 64) { const uint8_t c = (uint8_t)read_code(rd, job.rev ? job.rPos + job.rLen - 1 - i : job.rPos + i); b.q[i] = c; if (in_lds) gq[i] = c; }
                for (int i = lane; i < job.gLen; i += 64) { const uint8_t c = (uint8_t)ref_code(cx.ix, job.rev ? job.gPos + job.gLen - 1 - i : job.gPos + i); b.t[i] = c; if (in_lds) gt[i] = c; }
                __syncthreads();
                int score = 0;
                dp_sweep<K, 64>(nw, job.rLen, job.gLen, b, &score);
                if (lane == 0) { slot[g_n].off = used; slot[g_n].score = score; }
                used += need;
                __syncthreads();
            }
            __threadfence_block();
            __syncthreads();
            // ---- the walks, one problem per lane ----
            if (lane < g_n) {
                const uint32_t jb = jb0 + (uint32_t)lane;
                const DpJob job = sink.jobs[jb];
                const uint8_t *gq = mine + slot[lane].off, *gt = gq + job.rLen, *gdir = gq + ((job.rLen + job.gLen + 15) & ~15);
                PairState st = pair_state(cx.state, cx.lay, cx.caps, job.pair);
                DpSummary *sum = cx.dp_summary ? (DpSummary *)(st.ops + job.ops_off - kDpSum) : nullptr;
                const int w = dp_trace(nw, job.rLen, job.gLen, gq, gt, gdir, st.ops + job.ops_off, sum, (uint32_t)job.ops_off);
                Frag f = st.frags[job.frag];
                f.ops_off = job.ops_off + w;
                f.ops_len = job.rLen + job.gLen - w;
                f.meta = sum ? (uint32_t)((job.ops_off - kDpSum) >> 3) + 1u : 0u;
                st.frags[job.frag] = f;
                sink.jobs[jb].score = slot[lane].score;
            }
            __syncthreads();
            jb0 += (uint32_t)g_n;
        }
    }
}

constexpr int kDpHalfT = 32, kDpHalfQ = 64, kDpHalfLds = kDpHalfQ + kDpHalfT + (kDpHalfQ + kDpHalfT - 1) * kDpHalfT + 32;
// TWO problems per lane (mcx_dp_lane2.h): a wavefront takes 128 problems of its list at a time, lane l the neighbours 2l and 2l + 1 of the (shape-sorted)
// list; every value of both recurrences in the sixteen bits it needs, problem A in the low half of a register and problem B in the high one, so that one
// v_pk_*_i16 instruction advances both — the arithmetic width of the reference's own vectors (ksw2_alignment.cpp:70-248: sixteen int8 lanes).  Same words
// per problem in the wavefront's stretch of scratch, same column strings and summaries as the one-per-lane form of mcx_dp_lane.h (mcx_extend_lanes runs both on the device).
template <int K, bool NW>
__global__ void __launch_bounds__(64) k_dp_lane2(Ctx cx, JobSink sink, const uint32_t *order, ReadBatch rb, PairSel sel, uint32_t *scratch, uint64_t stride_words, uint32_t *unsupported,
                                                 uint32_t min_n)
{
    const uint32_t n = min(*sink.count, sink.cap);
    if (n < min_n) return; // (a short list: k_dp_group's)
    const int lane = threadIdx.x;
    const int nr = cx.pm.paired ? 2 : 1;
    LaneMem mem; mem.base = scratch + (uint64_t)blockIdx.x * stride_words; mem.stride = 64; mem.lane = (uint32_t)lane;
    for (uint32_t g0 = blockIdx.x * 128u; g0 < n; g0 += gridDim.x * 128u) {
        const uint32_t ja = g0 + 2u * (uint32_t)lane, jb = ja + 1u;
        const bool have_a = ja < n, have_b = jb < n;
        const uint32_t at_a = have_a ? (order ? order[ja] : ja) : 0u, at_b = have_b ? (order ? order[jb] : jb) : at_a;
        DpJob job_a, job_b;
        if (have_a) job_a = sink.jobs[at_a]; else { job_a.rLen = 0; job_a.gLen = 0; }
        if (have_b) job_b = sink.jobs[at_b]; else job_b = job_a;
        int rows = max(job_a.rLen, job_b.rLen), strips = (max(job_a.gLen, job_b.gLen) + K - 1) / K;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { rows = max(rows, __shfl_xor(rows, o, 64)); strips = max(strips, __shfl_xor(strips, o, 64)); }
        const LaneLayout2 l = lane_layout2<K, NW>(rows, strips);
        if ((uint64_t)l.words * 64u > stride_words) { if (lane == 0) atomicAdd(unsupported, 1u); continue; } // (cannot happen: the lists' size limits are the strides')
        if (!have_a) continue;
        ReadRef rd[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const DpJob &job = h ? job_b : job_a;
            const uint32_t read = sel_pair(sel, job.pair) * nr + job.slot;
            rd[h].flipped = (cx.pm.paired && job.slot == 1) ? 1 : 0;
            // (the job says whether its read holds an N — k_build knew —: a read without one is its 2-bit words and nothing else, no look at its offsets or its flags)
            if (cx.packed && job.score == 0) { rd[h].codes = cx.packed + (uint64_t)read * cx.wpad; rd[h].ascii = nullptr; rd[h].rlen = 0; }
            else { rd[h].codes = nullptr; rd[h].ascii = rb.bases + rb.off[read]; rd[h].rlen = (int)(rb.off[read + 1] - rb.off[read]); }
        }
        int sc[2];
        lane_dp_job2<K, NW>(cx, mem, l, job_a, rd[0], have_b, job_b, rd[1], sc);
        sink.jobs[at_a].score = sc[0];
        if (have_b) sink.jobs[at_b].score = sc[1];
    }
}

// the three short lists (job_class): tiny <= 8 x 8 in strips of 8; small: targets <= 16, queries <= 32; half: targets <= 32, queries <= 64
uint64_t lane_short_words(int which) // ksw2's flags take more words than nw's: sized for them; a lane of k_dp_lane2 keeps two problems
{
    return which == 0 ? 64ull * lane_layout2<8, false>(kDpTiny, 1).words : which == 1 ? 64ull * lane_layout2<16, false>(kDpSmallQ, 1).words : 64ull * lane_layout2<16, false>(kDpHalfQ, 2).words;
}
// (per lane 50, 194 and 644 words; the one-per-lane layout of mcx_dp_lane.h, which these sizes once also covered, takes 18, 100 and 328)

// ---- the problems of a long list by shape ------------------------------------------------------------------------------------
// A wavefront of k_dp_lane2 runs as long as the longest query times the most strips among its problems.  The two long lists
// (targets of 17-64 and of 65-256 bases, queries of any length) are therefore dealt to the wavefronts by shape: 1024 buckets of
// (strips, query length in 64 classes), largest first; within a bucket the problems differ by less than 4 rows for reads of up
// to 256 bases (8 / 16 rows for longer ones).  With the 16 row classes this began with, a wavefront's rows were the class's
// largest — 7.5 rows above its problems' mean, a sixth of the cells of config 5's 45-row problems computed for nothing.  Three
// small passes — count per bucket, start of every bucket, place — over the list's 40-byte records; the order among equals is
// whatever the atomics give (no result depends on it).
constexpr int kDpRowClasses = 64, kDpSortTile = 8;
static __device__ __forceinline__ int dp_bucket(const DpJob &j, int row_shift)
{
    const int strips = (j.gLen + 15) >> 4, rows = min(kDpRowClasses - 1, j.rLen >> row_shift);
    return (min(16, max(strips, 1)) - 1) * kDpRowClasses + rows; // (0..1023; the largest shapes get the largest numbers)
}

__global__ void __launch_bounds__(256) k_dp_sort_count(JobSink sink, int row_shift, uint32_t *counts, uint32_t min_n)
{
    __shared__ uint32_t h[kDpBuckets];
    const uint32_t n = min(*sink.count, sink.cap);
    if (n < min_n) return;
    for (int b = threadIdx.x; b < kDpBuckets; b += 256) h[b] = 0u;
    __syncthreads();
    for (uint32_t base = blockIdx.x * (256u * kDpSortTile); base < n; base += gridDim.x * (256u * kDpSortTile))
        for (int t = 0; t < kDpSortTile; t++) {
            const uint32_t i = base + t * 256u + threadIdx.x;
            if (i < n) atomicAdd(&h[dp_bucket(sink.jobs[i], row_shift)], 1u);
        }
    __syncthreads();
    for (int b = threadIdx.x; b < kDpBuckets; b += 256) if (h[b]) atomicAdd(&counts[b], h[b]);
}

// counts[0..1024) -> cursor[b] = where bucket b begins when the buckets are laid out from the largest shape down
__global__ void __launch_bounds__(256) k_dp_sort_scan(const uint32_t *counts, uint32_t *cursor)
{
    __shared__ uint32_t c[kDpBuckets], part[256];
    constexpr int per = kDpBuckets / 256;
    // thread t owns the buckets kDpBuckets-1 - (per t .. per t + per-1): the largest shapes first
    uint32_t mine[per], sum = 0;
    for (int k = 0; k < per; k++) { mine[k] = counts[kDpBuckets - 1 - (per * (int)threadIdx.x + k)]; sum += mine[k]; }
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t at = 0; for (int k = 0; k < 256; k++) { const uint32_t m = part[k]; part[k] = at; at += m; } }
    __syncthreads();
    uint32_t at = part[threadIdx.x];
    for (int k = 0; k < per; k++) { c[per * threadIdx.x + k] = at; at += mine[k]; }
    for (int k = 0; k < per; k++) cursor[kDpBuckets - 1 - (per * (int)threadIdx.x + k)] = c[per * threadIdx.x + k];
}

__global__ void __launch_bounds__(256) k_dp_sort_place(JobSink sink, int row_shift, uint32_t *cursor, uint32_t *order, uint32_t min_n)
{
    __shared__ uint32_t h[kDpBuckets], at[kDpBuckets];
    const uint32_t n = min(*sink.count, sink.cap);
    if (n < min_n) return;
    for (uint32_t base = blockIdx.x * (256u * kDpSortTile); base < n; base += gridDim.x * (256u * kDpSortTile)) {
        for (int b = threadIdx.x; b < kDpBuckets; b += 256) h[b] = 0u;
        __syncthreads();
        int b[kDpSortTile];
        uint32_t rank[kDpSortTile];
#pragma unroll
        for (int t = 0; t < kDpSortTile; t++) {
            const uint32_t i = base + t * 256u + threadIdx.x;
            b[t] = i < n ? dp_bucket(sink.jobs[i], row_shift) : -1;
            rank[t] = b[t] >= 0 ? atomicAdd(&h[b[t]], 1u) : 0u;
        }
        __syncthreads();
        for (int q = threadIdx.x; q < kDpBuckets; q += 256) at[q] = h[q] ? atomicAdd(&cursor[q], h[q]) : 0u;
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kDpSortTile; t++) if (b[t] >= 0) order[at[b[t]] + rank[t]] = base + t * 256u + threadIdx.x;
        __syncthreads();
    }
}

// words a wavefront's stretch of scratch must hold for a list whose problems have at most `rows` query bases and `strips` strips
// (the long lists': strips of 16 columns)
uint64_t lane_stride_words(bool nw, int rows, int strips)
{
    return 64ull * (nw ? lane_layout2<16, true>(rows, strips).words : lane_layout2<16, false>(rows, strips).words);
}

template <int K>
static void launch_dp_lane(bool nw, unsigned blocks, hipStream_t s, const Ctx &cx, const JobSink &sink, const uint32_t *order, const ReadBatch &rb, const PairSel &sel,
                           uint32_t *scratch, uint64_t stride_words, uint32_t *unsupported, uint32_t min_n)
{
    if (nw) k_dp_lane2<K, true><<<blocks, 64, 0, s>>>(cx, sink, order, rb, sel, scratch, stride_words, unsupported, min_n);
    else k_dp_lane2<K, false><<<blocks, 64, 0, s>>>(cx, sink, order, rb, sel, scratch, stride_words, unsupported, min_n);
}

// targets <= 32 (queries <= 64) of the one-column-per-lane class: two problems per wave, 32 lanes each — the
// class is bound by vector instructions issued, and most of its targets are that short

__global__ void __launch_bounds__(256) k_dp_half(Ctx cx, JobSink sink, ReadBatch rb, PairSel sel)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[8 * kDpHalfLds];
    const int group = threadIdx.x >> 5;
    uint8_t *mine = lds + group * kDpHalfLds;
    DpBuf b; b.q = mine; b.t = mine + kDpHalfQ; b.dir = mine + kDpHalfQ + kDpHalfT;
    const uint32_t n = min(*sink.count, sink.cap);
    for (uint32_t jb = blockIdx.x * 8 + group; jb < n; jb += gridDim.x * 8)
        dp_run_job<1, 32>(cx, sink, jb, sink.jobs[jb], rb, sel, b);
}

// one tiny problem per lane (mcx_dp.h kDpTiny)
__global__ void __launch_bounds__(256) k_dp_tiny(Ctx cx, JobSink sink, ReadBatch rb, PairSel sel)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[256 * kDpTinyLds];
    uint8_t *mine = lds + threadIdx.x * kDpTinyLds;
    DpBuf b; b.q = mine; b.t = mine + kDpTiny; b.dir = mine + 2 * kDpTiny;
    const uint32_t n = min(*sink.count, sink.cap);
    for (uint32_t jb = blockIdx.x * blockDim.x + threadIdx.x; jb < n; jb += gridDim.x * blockDim.x)
        dp_run_job<kDpTiny, 1>(cx, sink, jb, sink.jobs[jb], rb, sel, b);
}

// four small problems per wave, sixteen per block; each 16-lane group owns 800 bytes of LDS
__global__ void __launch_bounds__(256) k_dp_small(Ctx cx, JobSink sink, ReadBatch rb, PairSel sel)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[16 * kDpSmallLds];
    const int nr = cx.pm.paired ? 2 : 1;
    const int group = threadIdx.x >> 4, lane = threadIdx.x & 15;
    uint8_t *mine = lds + group * kDpSmallLds;
    const uint32_t n = min(*sink.count, sink.cap);
    for (uint32_t jb = blockIdx.x * 16 + group; jb < n; jb += gridDim.x * 16) {
        const DpJob job = sink.jobs[jb];
        const uint32_t read = sel_pair(sel, job.pair) * nr + job.slot;
        ReadRef rd;
        rd.ascii = rb.bases + rb.off[read]; rd.rlen = (int)(rb.off[read + 1] - rb.off[read]); rd.flipped = (cx.pm.paired && job.slot == 1) ? 1 : 0;
        DpBuf b; b.q = mine; b.t = mine + kDpSmallQ; b.dir = mine + 64;
        for (int i = lane; i < job.rLen; i += 16) b.q[i] = (uint8_t)read_code(rd, job.rev ? job.rPos + job.rLen - 1 - i : job.rPos + i);
        if (lane < job.gLen) b.t[lane] = (uint8_t)ref_code(cx.ix, job.rev ? job.gPos + job.gLen - 1 - lane : job.gPos + lane);
        dp_sync<16>();
        PairState st = pair_state(cx.state, cx.lay, cx.caps, job.pair);
        int score = 0;
        DpSummary *sum = cx.dp_summary ? (DpSummary *)(st.ops + job.ops_off - kDpSum) : nullptr;
        const int w = dp_core<1, 16>(cx.pm.use_nw != 0, job.rLen, job.gLen, b, st.ops + job.ops_off, &score, sum, (uint32_t)job.ops_off);
        if (lane == 0) {
            Frag f = st.frags[job.frag]; // one fetch, one store (the fields share two words)
            f.ops_off = job.ops_off + w;
            f.ops_len = job.rLen + job.gLen - w;
            f.meta = sum ? (uint32_t)((job.ops_off - kDpSum) >> 3) + 1u : 0u;
            st.frags[job.frag] = f;
            sink.jobs[jb].score = score;
        }
        dp_sync<16>();
    }
}

// the DP job lists of a pass, one kernel per size class: they work on disjoint lists and are each bound by latency at
// modest occupancy, so side streams let them share the chip instead of queueing behind one another
// A long list is worth a lane per problem; a short one (the large tier's, a replay's, the late pairs': a few thousand problems of
// 100 x 100 cells) is done sooner with a wavefront per problem — fewer problems than the chip has lanes, each 60 times quicker
// that way.  The list's length is known on the device only, so both kernels are launched and the one whose turn it is not leaves at
// once: k_dp_group below kDpLaneMin problems, k_dp_lane2 from there on.
constexpr uint32_t kDpLaneMin[2] = {65536, 131072}; // targets of 17-64 bases (mean 45 x 45 cells), of 65-256 (95 x 95): two wavefronts per SIMD's worth of problems

int launch_dp(const Knobs &kn, const PassRes &R, const Ctx &cx, const JobSinks &sinks, const ReadBatch &rb, const PairSel &sel, int rlen_max)
{
    hipStream_t s = R.stream;
    // three chains of about the same length (the runtime folds streams onto a few hardware queues anyway: more streams only
    // make the pairing of kernels on a queue a matter of luck); a set of pass resources without side streams runs them in turn
    const int n_side = R.dp_stream[1] ? 2 : 0;
    hipStream_t side0 = n_side ? R.dp_stream[0] : s, side1 = n_side ? R.dp_stream[1] : s;
    HIP_TRY(hipEventRecord(R.dp_fork, s));
    for (int k = 0; k < n_side; k++) HIP_TRY(hipStreamWaitEvent(R.dp_stream[k], R.dp_fork, 0));
    const bool by_wave = kn.dp_by_wave; // (experiments, and the A/B of the parity tests: the wavefront-per-problem kernels of mcx_dp.h)
    if (!by_wave) {
        // every list but the largest problems': one problem per lane (mcx_dp_lane.h).  A list's stretch of scratch per wavefront is
        // sized for its largest possible group; the two long lists share the wavefront kernels' buffers
        const bool nw = cx.pm.use_nw != 0;
        uint32_t *unsup = sinks.unsupported;
        const bool always = kn.dp_lane_always;
        uint32_t lane_min[2] = {always ? 0u : kDpLaneMin[0], always ? 0u : kDpLaneMin[1]};
        // two problems per lane in 16-bit halves (k_dp_lane2): the scores fit them with room to spare — queries + targets (at most 1000 + 256: mcx_ctx_create) far below
        // kNeg2's reach, and a cell's s~ (never below -2 (i + j) - 2: mismatches down the diagonal and one gap) within the fourteen bits a strip's edge word keeps of it
        const uint64_t w1 = lane_stride_words(nw, rlen_max, 4), w2 = lane_stride_words(nw, rlen_max, 16);
        const unsigned b1 = (unsigned)std::min<uint64_t>(4096, R.dp_stride[0] * R.dp_blocks[0] / (w1 * 4)), b2 = (unsigned)std::min<uint64_t>(4096, R.dp_stride[1] * R.dp_blocks[1] / (w2 * 4));
        // (a set of pass resources whose scratch does not hold one lane group for reads this long — the small sets with a large max_read_len —
        //  leaves that list to the wavefront kernel whatever its length)
        if (b1 == 0) lane_min[0] = 0xFFFFFFFFu;
        if (b2 == 0) lane_min[1] = 0xFFFFFFFFu;
        const uint32_t *ord[2] = {nullptr, nullptr};
        hipStream_t st[2] = {s, side1};
        const int row_shift = rlen_max <= 256 ? 2 : (rlen_max <= 512 ? 3 : (rlen_max <= 1024 ? 4 : 6)); // (64 row classes cover the longest query)
        for (int k = 0; k < 2; k++) {
            if (lane_min[k] == 0xFFFFFFFFu) continue;
            uint32_t *counts = R.d_cnt + CNT_DP_SORT + 2 * kDpBuckets * k, *cursor = counts + kDpBuckets; // (cleared with the pass's counters)
            k_dp_sort_count<<<1024, 256, 0, st[k]>>>(sinks.s[1 + k], row_shift, counts, lane_min[k]);
            k_dp_sort_scan<<<1, 256, 0, st[k]>>>(counts, cursor);
            k_dp_sort_place<<<1024, 256, 0, st[k]>>>(sinks.s[1 + k], row_shift, cursor, R.d_dp_order[k], lane_min[k]);
            ord[k] = R.d_dp_order[k];
        }
        if (b1) launch_dp_lane<16>(nw, b1, st[0], cx, sinks.s[1], ord[0], rb, sel, (uint32_t *)R.d_dp_scratch[0], w1, unsup, lane_min[0]);
        k_dp_group<1><<<R.dp_blocks[0], 64, 0, st[0]>>>(cx, sinks.s[1], rb, sel, R.d_dp_scratch[0], R.dp_stride[0], lane_min[0]);
        if (b2) launch_dp_lane<16>(nw, b2, st[1], cx, sinks.s[2], ord[1], rb, sel, (uint32_t *)R.d_dp_scratch[1], w2, unsup, lane_min[1]);
        k_dp_group<4><<<R.dp_blocks[1], 64, 0, st[1]>>>(cx, sinks.s[2], rb, sel, R.d_dp_scratch[1], R.dp_stride[1], lane_min[1]);
        uint32_t *p = R.d_dp_lane;
        launch_dp_lane<8>(nw, R.dp_lane_blocks, side0, cx, sinks.s[4], nullptr, rb, sel, p, lane_short_words(0), unsup, 0u);
        p += lane_short_words(0) * R.dp_lane_blocks;
        launch_dp_lane<16>(nw, R.dp_lane_blocks, side0, cx, sinks.s[0], nullptr, rb, sel, p, lane_short_words(1), unsup, 0u);
        p += lane_short_words(1) * R.dp_lane_blocks;
        launch_dp_lane<16>(nw, R.dp_lane_blocks, side0, cx, sinks.s[5], nullptr, rb, sel, p, lane_short_words(2), unsup, 0u);
        k_dp_sel<16><<<R.dp_blocks[2], 64, 0, side1>>>(cx, sinks.s[3], rb, sel, R.d_dp_scratch[2], R.dp_stride[2]);
    } else {
    k_dp_group<1><<<R.dp_blocks[0], 64, 0, s>>>(cx, sinks.s[1], rb, sel, R.d_dp_scratch[0], R.dp_stride[0], 0xFFFFFFFFu);
    k_dp_small<<<2560, 256, 0, side0>>>(cx, sinks.s[0], rb, sel);
    k_dp_group<4><<<R.dp_blocks[1], 64, 0, side1>>>(cx, sinks.s[2], rb, sel, R.d_dp_scratch[1], R.dp_stride[1], 0xFFFFFFFFu);
    // (the half-wave class behind the 65-256-column class looks like the long pole on a timeline; moved behind the shorter chains
    //  the stage takes the same 3.3-3.4 ms: the kernels share the chip, the stage is the sum of their work)
    k_dp_tiny<<<2048, 256, 0, s>>>(cx, sinks.s[4], rb, sel);
    k_dp_half<<<2048, 256, 0, side1>>>(cx, sinks.s[5], rb, sel);
    k_dp_sel<16><<<R.dp_blocks[2], 64, 0, side0>>>(cx, sinks.s[3], rb, sel, R.d_dp_scratch[2], R.dp_stride[2]);
    }
    for (int k = 0; k < n_side; k++) { HIP_TRY(hipEventRecord(R.dp_join[k], R.dp_stream[k])); HIP_TRY(hipStreamWaitEvent(s, R.dp_join[k], 0)); }
    return 0;
}

// stand-alone extension (nw_alignment / ksw2_alignment as a batch): strings come from user buffers
struct ExtArgs {
    const uint8_t *q, *t;
    const uint32_t *q_off, *t_off;
    uint8_t *ops; int32_t *ops_len, *score;
    uint32_t n;
    int use_nw;
};

template <int K>
__global__ void __launch_bounds__(64) k_extend(ExtArgs a, uint8_t *scratch, uint64_t stride, int t_lo, int t_hi)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kDpLdsSeq + kDpLdsDir];
    uint8_t *spill = scratch + (uint64_t)blockIdx.x * stride;
    const int lane = threadIdx.x;
    for (uint32_t jb = blockIdx.x; jb < a.n; jb += gridDim.x) {
        const int m = (int)(a.q_off[jb + 1] - a.q_off[jb]), n = (int)(a.t_off[jb + 1] - a.t_off[jb]);
        if (n <= t_lo || n > t_hi || m <= 0) continue;
        const DpBuf b = dp_buffers(m, n, lds, spill);
        for (int i = lane; i < m; i += 64) b.q[i] = (uint8_t)nt4_code(a.q[a.q_off[jb] + i]);
        for (int i = lane; i < n; i += 64) b.t[i] = (uint8_t)nt4_code(a.t[a.t_off[jb] + i]);
        __syncthreads();
        uint8_t *dst = a.ops + a.q_off[jb] + a.t_off[jb];
        int score = 0;
        const int w = dp_core<K, 64, true>(a.use_nw != 0, m, n, b, dst, &score, nullptr, 0u);
        const int L = m + n - w;
        for (int base = 0; base < L; base += 64) { // move the string to the front of its area
            uint8_t v = base + lane < L ? dst[w + base + lane] : 0;
            __syncthreads();
            if (base + lane < L) dst[base + lane] = v;
            __syncthreads();
        }
        if (lane == 0) { a.ops_len[jb] = L; a.score[jb] = score; }
    }
}

extern "C" int mcx_extend_batch(mcx_ctx *c, int alg, const uint8_t *q, const uint32_t *q_off, const uint8_t *t,
                                const uint32_t *t_off, uint32_t n, uint8_t *ops, int32_t *ops_len, int32_t *score)
{
    if (!c || !q || !q_off || !t || !t_off || !ops || !ops_len || !score) return mcx_set_error(MCX_ERR_ARG, "mcx_extend_batch: null argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->idx->device));
    for (uint32_t i = 0; i < n; i++) {
        if (t_off[i + 1] - t_off[i] > 1024 || q_off[i + 1] - q_off[i] > 2048 || t_off[i + 1] == t_off[i] || q_off[i + 1] == q_off[i])
            return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_extend_batch: fragments must be 1..2048 (read) x 1..1024 (genome)");
    }
    ExtArgs a; a.n = n; a.use_nw = alg == 0;
    uint8_t *d_q = nullptr, *d_t = nullptr, *d_ops = nullptr; uint32_t *d_qo = nullptr, *d_to = nullptr; int32_t *d_len = nullptr, *d_sc = nullptr;
    const size_t nq = q_off[n], nt = t_off[n];
    int rc = 0;
    if ((rc = dmalloc(&d_q, nq + 16)) || (rc = dmalloc(&d_t, nt + 16)) || (rc = dmalloc(&d_ops, nq + nt + 16)) ||
        (rc = dmalloc(&d_qo, (size_t)n + 1)) || (rc = dmalloc(&d_to, (size_t)n + 1)) || (rc = dmalloc(&d_len, n)) || (rc = dmalloc(&d_sc, n))) return rc;
    HIP_TRY(hipMemcpy(d_q, q, nq, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_t, t, nt, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_qo, q_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_to, t_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice));
    a.q = d_q; a.t = d_t; a.q_off = d_qo; a.t_off = d_to; a.ops = d_ops; a.ops_len = d_len; a.score = d_sc;
    k_extend<1><<<c->t0.dp_blocks[0], 64, 0, c->t0.stream>>>(a, c->t0.d_dp_scratch[0], c->t0.dp_stride[0], 0, 64);
    k_extend<4><<<c->t0.dp_blocks[1], 64, 0, c->t0.stream>>>(a, c->t0.d_dp_scratch[1], c->t0.dp_stride[1], 64, 256);
    k_extend<16><<<c->t0.dp_blocks[2], 64, 0, c->t0.stream>>>(a, c->t0.d_dp_scratch[2], c->t0.dp_stride[2], 256, 1024);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->t0.stream));
    HIP_TRY(hipMemcpy(ops, d_ops, nq + nt, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ops_len, d_len, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(score, d_sc, (size_t)n * 4, hipMemcpyDeviceToHost));
    (void)hipFree(d_q); (void)hipFree(d_t); (void)hipFree(d_ops); (void)hipFree(d_qo); (void)hipFree(d_to); (void)hipFree(d_len); (void)hipFree(d_sc);
    return 0;
}

