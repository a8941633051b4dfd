// mapcaller_amd/csrc/mcx_extend_lanes.hip — mcx_extend_lanes: the lane forms of the gapped extension (mcx_dp_lane.h: one problem
// per lane; mcx_dp_lane2.h: two per lane in 16-bit halves) on strings the caller hands over, in the caller's order.
//
// What the batch pipeline gives these forms is what a mapping run happens to produce, dealt by shape (k_dp_sort_*), so that the two
// halves of a register and the 64 lanes of a wavefront almost always hold like problems.  Here the caller chooses the problems, who
// shares a lane and a wavefront with whom, and how many groups a wavefront takes one after the other in the same stretch of scratch.
// The kernels are k_dp_lane's / k_dp_lane2's plumbing around the very templates those call — layout from the wave-wide maximum,
// words lane-interleaved (stride 64), staging, sweep, walk, summary — with the strings fetched from the caller's ASCII instead of
// the read's 2-bit words and the 2-bit genome.  No arithmetic is restated here.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mcx.h"
#include "mcx_dp_lane2.h"
#include "mcx_internal.h"

using namespace mcx;

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace {

struct LaneArgs {
    const uint8_t *q, *t;          // the strings (ASCII), concatenated
    const uint32_t *q_off, *t_off; // n + 1 entries each
    const uint32_t *area_off;      // where a problem's columns are walked into: word-aligned, rounded up to a word (the walks store four columns at a time)
    uint8_t *area;
    uint8_t *ops; int32_t *ops_len, *score; // the results, laid out as mcx_extend_batch's
    DpSummary *sums;               // null: no summaries
    uint32_t n;
};

// one problem's strings as the sweeps and walks take them
struct LaneStr {
    const uint8_t *q, *t; int m, n;
    __device__ void get16(int p, uint32_t &codes, uint32_t &flags) const
    {
        codes = 0; flags = 0;
        for (int k = 0; k < 16 && p + k < m; k++) { const int c = nt4_code(q[p + k]); codes |= (uint32_t)(c & 3) << (30 - 2 * k); flags |= (uint32_t)(c > 3) << (15 - k); }
    }
    __device__ uint32_t tgt16(int b0) const // (the host refused targets with a letter outside ACGT)
    {
        uint32_t v = 0;
        for (int k = 0; k < 16; k++) v = (v << 2) | (b0 + k < n ? (uint32_t)nt4_code(t[b0 + k]) & 3u : 0u);
        return v;
    }
};

__device__ LaneStr lane_str(const LaneArgs &a, uint32_t j)
{
    LaneStr s;
    s.q = a.q + a.q_off[j]; s.t = a.t + a.t_off[j];
    s.m = (int)(a.q_off[j + 1] - a.q_off[j]); s.n = (int)(a.t_off[j + 1] - a.t_off[j]);
    return s;
}

// the column string from where the walk left it (area + w) to the front of the problem's place in ops
__device__ void lane_result(const LaneArgs &a, uint32_t j, const LaneStr &s, const uint8_t *area, int w, int score)
{
    const int L = s.m + s.n - w;
    uint8_t *dst = a.ops + a.q_off[j] + a.t_off[j];
    for (int k = 0; k < L; k++) dst[k] = area[w + k];
    a.ops_len[j] = L;
    a.score[j] = score;
}

// k_dp_lane with the caller's strings: lane l of group g takes problem 64 g + l
template <int K, bool NW>
__global__ void __launch_bounds__(64) k_extend_lane(LaneArgs a, uint32_t *scratch, uint64_t stride_words, uint32_t *unsupported)
{
    const int lane = threadIdx.x;
    LaneMem mem; mem.base = scratch + (uint64_t)blockIdx.x * stride_words; mem.stride = 64; mem.lane = (uint32_t)lane;
    for (uint32_t g0 = blockIdx.x * 64u; g0 < a.n; g0 += gridDim.x * 64u) {
        const uint32_t jb = g0 + (uint32_t)lane;
        const bool have = jb < a.n;
        LaneStr s; s.q = s.t = nullptr; s.m = s.n = 0;
        if (have) s = lane_str(a, jb);
        int rows = s.m, strips = (s.n + K - 1) / K;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { rows = max(rows, __shfl_xor(rows, o, 64)); strips = max(strips, __shfl_xor(strips, o, 64)); }
        const LaneLayout l = lane_layout<K, NW>(rows, strips);
        if ((uint64_t)l.words * 64u > stride_words) { if (lane == 0) atomicAdd(unsupported, 1u); continue; } // (cannot happen: the host sized the stretches with the same layouts)
        if (!have) continue;
        lane_stage_query(mem, l, s.m, [&](int p, uint32_t &codes, uint32_t &flags) { s.get16(p, codes, flags); });
        auto tgt16 = [&](int b0) -> uint32_t { return s.tgt16(b0); };
        uint8_t *area = a.area + a.area_off[jb];
        DpSummary *sum = a.sums ? a.sums + jb : nullptr;
        int score = 0, w;
        if (NW) {
            score = lane_sweep_nw<K>(mem, l, s.m, s.n, tgt16);
            w = lane_trace_nw<K>(mem, l, s.m, s.n, tgt16, area, sum, 0u);
        } else {
            lane_sweep_ksw2<K>(mem, l, s.m, s.n, tgt16);
            w = lane_trace_ksw2<K>(mem, l, s.m, s.n, tgt16, area, sum, 0u);
        }
        lane_result(a, jb, s, area, w, score);
    }
}

// k_dp_lane2 with the caller's strings: lane l of group g takes problem 128 g + 2 l in the low halves and 128 g + 2 l + 1 in the high ones
template <int K, bool NW>
__global__ void __launch_bounds__(64) k_extend_lane2(LaneArgs a, uint32_t *scratch, uint64_t stride_words, uint32_t *unsupported)
{
    const int lane = threadIdx.x;
    LaneMem mem; mem.base = scratch + (uint64_t)blockIdx.x * stride_words; mem.stride = 64; mem.lane = (uint32_t)lane;
    for (uint32_t g0 = blockIdx.x * 128u; g0 < a.n; g0 += gridDim.x * 128u) {
        const uint32_t ja = g0 + 2u * (uint32_t)lane, jb = ja + 1u;
        const bool have_a = ja < a.n, have_b = jb < a.n;
        LaneStr sa, sb; sa.q = sa.t = nullptr; sa.m = sa.n = 0;
        if (have_a) sa = lane_str(a, ja);
        if (have_b) sb = lane_str(a, jb); else { sb = sa; sb.m = sb.n = 0; } // (lane_dp_job2: the lane holds one problem, its second half runs on nothing)
        int rows = max(sa.m, sb.m), strips = (max(sa.n, sb.n) + K - 1) / K;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { rows = max(rows, __shfl_xor(rows, o, 64)); strips = max(strips, __shfl_xor(strips, o, 64)); }
        const LaneLayout2 l = lane_layout2<K, NW>(rows, strips);
        if ((uint64_t)l.words * 64u > stride_words) { if (lane == 0) atomicAdd(unsupported, 1u); continue; } // (cannot happen: the host sized the stretches with the same layouts)
        if (!have_a) continue;
        auto tgt_a = [&](int b0) -> uint32_t { return b0 < sa.n ? sa.tgt16(b0) : 0u; };
        auto tgt_b = [&](int b0) -> uint32_t { return b0 < sb.n ? sb.tgt16(b0) : 0u; };
        const uint32_t ta0 = tgt_a(0), tb0 = tgt_b(0);
        lane_stage_query2_words(mem, l, sa.m, sb.m, [&](int p, uint32_t &cw, uint32_t &fw) { sa.get16(p, cw, fw); }, [&](int p, uint32_t &cw, uint32_t &fw) { sb.get16(p, cw, fw); });
        int sc[2] = {0, 0};
        if (NW) lane_sweep_nw2<K>(mem, l, sa.m, sa.n, sb.m, sb.n, tgt_a, tgt_b, &sc[0], &sc[1], ta0, tb0);
        else lane_sweep_ksw2_2<K>(mem, l, sa.m, sa.n, sb.m, sb.n, tgt_a, tgt_b, ta0, tb0);
        LaneWalk2<K, NW> wa(mem, l, 0), wb(mem, l, 1);
        uint8_t *area_a = a.area + a.area_off[ja], *area_b = have_b ? a.area + a.area_off[jb] : area_a;
        wa.begin(sa.m, sa.n, area_a, a.sums ? a.sums + ja : nullptr);
        if (have_b) wb.begin(sb.m, sb.n, area_b, a.sums ? a.sums + jb : nullptr);
        lane_walk2(wa, wb);
        wa.sink.end(0u, sa.m + sa.n);
        lane_result(a, ja, sa, area_a, wa.sink.w, NW ? sc[0] : 0);
        if (have_b) {
            wb.sink.end(0u, sb.m + sb.n);
            lane_result(a, jb, sb, area_b, wb.sink.w, NW ? sc[1] : 0);
        }
    }
}

template <int K>
uint64_t group_words(bool nw, int form, int rows, int strips)
{
    if (form == 2) return nw ? lane_layout2<K, true>(rows, strips).words : lane_layout2<K, false>(rows, strips).words;
    return nw ? lane_layout<K, true>(rows, strips).words : lane_layout<K, false>(rows, strips).words;
}

template <int K>
void launch(bool nw, int form, unsigned blocks, hipStream_t s, const LaneArgs &a, uint32_t *scratch, uint64_t stride_words, uint32_t *unsupported)
{
    if (form == 2) {
        if (nw) k_extend_lane2<K, true><<<blocks, 64, 0, s>>>(a, scratch, stride_words, unsupported);
        else k_extend_lane2<K, false><<<blocks, 64, 0, s>>>(a, scratch, stride_words, unsupported);
        return;
    }
    if (nw) k_extend_lane<K, true><<<blocks, 64, 0, s>>>(a, scratch, stride_words, unsupported);
    else k_extend_lane<K, false><<<blocks, 64, 0, s>>>(a, scratch, stride_words, unsupported);
}

// everything the call holds in HBM, released when it returns (whichever way)
struct DevBufs {
    std::vector<void *> all;
    ~DevBufs() { for (void *p : all) (void)hipFree(p); }
    template <class T> bool take(T **p, size_t count)
    {
        void *v = nullptr;
        if (hipMalloc(&v, std::max<size_t>(count * sizeof(T), 16)) != hipSuccess) { (void)hipGetLastError(); return false; }
        all.push_back(v);
        *p = (T *)v;
        return true;
    }
};

} // namespace

extern "C" int mcx_extend_lanes(mcx_ctx *c, int alg, int form, int strip, uint32_t blocks, const uint8_t *q, const uint32_t *q_off, const uint8_t *t,
                                const uint32_t *t_off, uint32_t n, uint8_t *ops, int32_t *ops_len, int32_t *score, void *summaries)
{
    if (!c || !q || !q_off || !t || !t_off || !ops || !ops_len || !score) return mcx_set_error(MCX_ERR_ARG, "mcx_extend_lanes: null argument");
    if (alg != 0 && alg != 1) return mcx_set_error(MCX_ERR_ARG, "mcx_extend_lanes: alg must be 0 (nw) or 1 (ksw2)");
    if (form != 1 && form != 2) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_extend_lanes: form must be 1 (one problem per lane) or 2 (two per lane)");
    if (strip != 8 && strip != 16) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_extend_lanes: strip must be 8 or 16");
    if (n == 0) return 0;
    const bool nw = alg == 0;
    const uint32_t max_t = strip == 8 ? 64u : 256u, per_group = form == 2 ? 128u : 64u, groups = (n + per_group - 1) / per_group;
    std::vector<uint32_t> area_off((size_t)n + 1);
    uint64_t area_bytes = 0, words = 0;
    for (uint32_t g = 0; g < groups; g++) {
        int rows = 0, strips = 0;
        for (uint32_t i = g * per_group; i < std::min(n, (g + 1) * per_group); i++) {
            const uint32_t m = q_off[i + 1] - q_off[i], tl = t_off[i + 1] - t_off[i];
            if (q_off[i + 1] <= q_off[i] || t_off[i + 1] <= t_off[i]) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_extend_lanes: problem " + std::to_string(i) + " has an empty query or target");
            if (m > 2048) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_extend_lanes: problem " + std::to_string(i) + " has a query longer than 2048 bases");
            if (tl > max_t) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_extend_lanes: problem " + std::to_string(i) + " has a target longer than " + std::to_string(max_t) + " bases (strips of " + std::to_string(strip) + ")");
            for (uint32_t k = t_off[i]; k < t_off[i + 1]; k++)
                if (nt4_code(t[k]) > 3) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_extend_lanes: problem " + std::to_string(i) + " has a target letter outside ACGT (the lane forms' targets come from the 2-bit genome)");
            rows = std::max(rows, (int)m); strips = std::max(strips, (int)((tl + (uint32_t)strip - 1) / (uint32_t)strip));
            area_off[i] = (uint32_t)area_bytes;
            area_bytes += ((uint64_t)m + tl + 7) & ~7ull;
        }
        words = std::max(words, strip == 8 ? group_words<8>(nw, form, rows, strips) : group_words<16>(nw, form, rows, strips));
    }
    area_off[n] = (uint32_t)area_bytes;
    if (area_bytes >> 32) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_extend_lanes: the batch's strings exceed 4 GB");
    const unsigned waves = blocks == 0 ? groups : std::min(blocks, groups);
    const uint64_t stride_words = 64ull * words; // a wavefront's stretch: the batch's largest group
    const size_t nq = q_off[n], nt = t_off[n];

    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    DevBufs d;
    LaneArgs a; a.n = n;
    uint8_t *d_q = nullptr, *d_t = nullptr, *d_area = nullptr, *d_ops = nullptr;
    uint32_t *d_qo = nullptr, *d_to = nullptr, *d_ao = nullptr, *d_scratch = nullptr, *d_unsup = nullptr;
    int32_t *d_len = nullptr, *d_sc = nullptr;
    DpSummary *d_sum = nullptr;
    if (!d.take(&d_q, nq) || !d.take(&d_t, nt) || !d.take(&d_area, (size_t)area_bytes) || !d.take(&d_ops, nq + nt) || !d.take(&d_qo, (size_t)n + 1) ||
        !d.take(&d_to, (size_t)n + 1) || !d.take(&d_ao, (size_t)n + 1) || !d.take(&d_len, n) || !d.take(&d_sc, n) || !d.take(&d_unsup, 1) ||
        (summaries && !d.take(&d_sum, n)) || !d.take(&d_scratch, (size_t)(stride_words * waves)))
        return mcx_set_error(MCX_ERR_DEVICE, "mcx_extend_lanes: out of device memory (" + std::to_string(stride_words * waves * 4 >> 20) + " MB of scratch for " + std::to_string(waves) + " wavefronts)");
    HIP_TRY(hipMemcpyAsync(d_q, q, nq, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_t, t, nt, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_qo, q_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_to, t_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_ao, area_off.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_unsup, 0, 4, s));
    HIP_TRY(hipMemsetAsync(d_ops, 0, nq + nt, s));
    HIP_TRY(hipMemsetAsync(d_len, 0, (size_t)n * 4, s));
    HIP_TRY(hipMemsetAsync(d_sc, 0, (size_t)n * 4, s));
    if (d_sum) HIP_TRY(hipMemsetAsync(d_sum, 0, (size_t)n * sizeof(DpSummary), s));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_scratch, (int)0xDEADBEEFu, (size_t)(stride_words * waves), s)); // (no word of a stretch is what a sweep would have left there)
    a.q = d_q; a.t = d_t; a.q_off = d_qo; a.t_off = d_to; a.area_off = d_ao; a.area = d_area; a.ops = d_ops; a.ops_len = d_len; a.score = d_sc; a.sums = d_sum;
    if (strip == 8) launch<8>(nw, form, waves, s, a, d_scratch, stride_words, d_unsup);
    else launch<16>(nw, form, waves, s, a, d_scratch, stride_words, d_unsup);
    HIP_TRY(hipGetLastError());
    uint32_t unsup = 0;
    HIP_TRY(hipMemcpyAsync(&unsup, d_unsup, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ops, d_ops, nq + nt, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ops_len, d_len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(score, d_sc, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (d_sum) HIP_TRY(hipMemcpyAsync(summaries, d_sum, (size_t)n * sizeof(DpSummary), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (unsup) return mcx_set_error(MCX_ERR_DEVICE, "mcx_extend_lanes: " + std::to_string(unsup) + " group(s) did not fit their stretch of scratch");
    return 0;
}
