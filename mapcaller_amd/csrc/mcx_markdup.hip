// mapcaller_amd/csrc/mcx_markdup.hip — duplicate reads found and flagged in HBM (mcx_bam_dup_units_dev, mcx_dup_resolve_dev, mcx_bam_dup_mark_dev; the file front
// end's -markdup: every part's units before the part is sorted, one resolve behind the last batch, every chunk of the merge marked before it is deflated).  The
// rule's arithmetic is mcx_markdup.h's.
//
//   k_dup_units      LANES lanes per unit (16 by measurement, see units_lanes below).  Lane 0 walks the block_size chain of the unit's group(s) as k_sort_count does, bounded by the
//                    group, checks every record against its own name, CIGAR, SEQ and QUAL, and reads the first record's flag, end (the CIGAR walk) and the place of
//                    its QUAL; the lanes then share the QUAL bytes: those ahead of the first 16-byte boundary and behind the last as single bytes, a lane each,
//                    everything between in aligned 16-byte loads, and the sums meet by __shfl_xor.  Units go to scratch and reach the caller's array only when
//                    the error word stayed 0.  No byte outside d_recs[0 .. n_bytes) and the offsets is read.
//   resolve, pairs   three stable hipcub radix sorts, least significant key first, carrying the unit number: inverted score (32 bits), second end, first end.  Units
//                    that are no pairs carry all-ones and gather behind them.  The head of every run of equal (first, second) stays; the others are duplicates.
//   resolve, frags   one table of two entries a unit — a pair's two ends, a fragment's end, all-ones for the rest — sorted by (kind << 32 | inverted score), then by
//                    end: within an end pairs come first, then the fragments best first.  A fragment is a duplicate unless it is the head of its end's segment.
//                    No atomics anywhere; ties fall to the lower unit number because the sorts are stable and the entries start in that order.
//   k_dup_mark       a lane per record: byte 19 |= 4 where the record's byte says so (through the sort's permutation in the merge).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcx.h"
#include "mcx_markdup.h"
#include "mcx_internal.h"
#include "mcx_sam_state.h"

using namespace mcx;

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

static_assert(sizeof(mcx_dup_unit) == 24, "a unit is 24 bytes: two ends, score, kind");

namespace {

enum { kErrChain = 1, kErrRange = 2, kErrKind = 4 };

template <int LANES> __device__ inline uint32_t bcast32(uint32_t v) { return (uint32_t)__shfl((int)v, 0, LANES); }
template <int LANES> __device__ inline uint64_t bcast64(uint64_t v) { return (uint64_t)bcast32<LANES>((uint32_t)v) | (uint64_t)bcast32<LANES>((uint32_t)(v >> 32)) << 32; }

__device__ inline uint32_t score_word(uint32_t w)
{
    return dup_score_byte(w & 255u) + dup_score_byte((w >> 8) & 255u) + dup_score_byte((w >> 16) & 255u) + dup_score_byte(w >> 24);
}

// read g by the LANES lanes of its unit: is it placed, where does it end, what does it score; what is wrong with it goes to err (lane 0's)
template <int LANES> __device__ inline void read_of(const uint8_t *__restrict__ recs, uint64_t n_bytes, const uint64_t *__restrict__ grp_off, uint32_t g, uint32_t n_groups, uint32_t lane,
                                                    uint32_t &err, bool &placed, uint64_t &end, uint32_t &score)
{
    uint32_t state = 0, l_seq = 0; // state: 1 placed and in range
    uint64_t q_at = 0, e = kDupNoEnd;
    if (lane == 0) {
        const uint64_t a = grp_off[g], b = grp_off[g + 1];
        bool ok = !(a > b || b > n_bytes || (g == 0 && a != 0) || (g + 1 == n_groups && b != n_bytes));
        for (uint64_t p = a; ok && p < b;) { // (every turn advances by 36 bytes or more)
            if (b - p < 4 + (uint64_t)kBamMinBlock) { ok = false; break; }
            const uint64_t len = 4 + (uint64_t)bam_get32(recs + p);
            if (len < 4 + (uint64_t)kBamMinBlock || len > b - p || !dup_record_fits(recs + p, len)) { ok = false; break; }
            p += len;
        }
        if (!ok) err |= (uint32_t)kErrChain;
        else if (a < b && dup_placed(recs + a)) {
            const uint8_t *r = recs + a;
            l_seq = bam_get32(r + 20);
            if (l_seq >= (uint32_t)kDupSeqLimit || !dup_pack(dup_end(r), &e)) { err |= (uint32_t)kErrRange; e = kDupNoEnd; }
            else { state = 1; q_at = a + dup_qual_at(r); }
        }
    }
    state = bcast32<LANES>(state);
    placed = state == 1;
    end = bcast64<LANES>(e);
    score = 0;
    if (!placed) return; // (the whole unit's lanes)
    l_seq = bcast32<LANES>(l_seq);
    q_at = bcast64<LANES>(q_at);
    const uint8_t *q = recs + q_at; // [q, q + l_seq) lies inside the record: dup_record_fits
    const uint32_t to16 = (16u - (uint32_t)((uintptr_t)q & 15u)) & 15u;
    const uint32_t head = to16 < l_seq ? to16 : l_seq, n16 = (l_seq - head) >> 4, tail_at = head + (n16 << 4);
    uint32_t s = 0;
    if (lane < head) s += dup_score_byte(q[lane]); // (head and tail are below 16 bytes, LANES is 16 or more)
    if (tail_at + lane < l_seq) s += dup_score_byte(q[tail_at + lane]);
    const uint4 *q16 = (const uint4 *)(q + head);
    for (uint32_t j = lane; j < n16; j += LANES) {
        const uint4 v = q16[j];
        s += score_word(v.x) + score_word(v.y) + score_word(v.z) + score_word(v.w);
    }
    for (int o = LANES / 2; o; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o, LANES);
    score = s;
}

template <int LANES> __global__ void __launch_bounds__(256) k_dup_units(const uint8_t *__restrict__ recs, uint64_t n_bytes, const uint64_t *__restrict__ grp_off, uint32_t n_groups, int paired,
                                                                        uint32_t n_units, mcx_dup_unit *units, uint32_t *error)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t u = t / LANES;
    const uint32_t lane = (uint32_t)(t % LANES);
    if (u >= n_units) return;
    uint32_t err = 0, s0 = 0, s1 = 0;
    bool p0 = false, p1 = false;
    uint64_t e0 = kDupNoEnd, e1 = kDupNoEnd;
    const uint32_t g = paired ? (uint32_t)(2 * u) : (uint32_t)u;
    read_of<LANES>(recs, n_bytes, grp_off, g, n_groups, lane, err, p0, e0, s0);
    if (paired) read_of<LANES>(recs, n_bytes, grp_off, g + 1, n_groups, lane, err, p1, e1, s1);
    if (lane) return;
    if (err) atomicOr(error, err);
    mcx_dup_unit o;
    if (p0 && p1) { o.end0 = e0 < e1 ? e0 : e1; o.end1 = e0 < e1 ? e1 : e0; o.score = s0 + s1; o.kind = (uint32_t)kDupPair; }
    else if (p0) { o.end0 = e0; o.end1 = kDupNoEnd; o.score = s0; o.kind = (uint32_t)kDupFragment; }
    else if (p1) { o.end0 = e1; o.end1 = kDupNoEnd; o.score = s1; o.kind = (uint32_t)kDupFragment | (uint32_t)kDupSecondMate; }
    else { o.end0 = o.end1 = kDupNoEnd; o.score = 0; o.kind = (uint32_t)kDupNone; }
    units[u] = o;
}

// ---- the resolve ---------------------------------------------------------------------------------------------------------------------------------------
__device__ inline bool is_pair(const mcx_dup_unit &u) { return (u.kind & 3u) == (uint32_t)kDupPair; }
__device__ inline bool is_frag(const mcx_dup_unit &u) { return (u.kind & 3u) == (uint32_t)kDupFragment; }
__device__ inline bool same_pair(const mcx_dup_unit &a, const mcx_dup_unit &b) { return is_pair(a) && is_pair(b) && a.end0 == b.end0 && a.end1 == b.end1; }

__global__ void __launch_bounds__(256) k_pair_score(const mcx_dup_unit *__restrict__ units, uint32_t n, uint64_t *key, uint32_t *idx, uint32_t *error)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mcx_dup_unit u = units[i];
    const uint32_t k = u.kind & 3u;
    if (u.kind > 7u || k == 3u || ((u.kind & 4u) && k != (uint32_t)kDupFragment)) atomicOr(error, (uint32_t)kErrKind);
    key[i] = is_pair(u) ? (uint64_t)(uint32_t)~u.score : 0;
    idx[i] = i;
}
__global__ void __launch_bounds__(256) k_pair_key(const mcx_dup_unit *__restrict__ units, uint32_t n, const uint32_t *__restrict__ idx, int second, uint64_t *key)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = idx[i];
    if (at >= n) { key[i] = kDupNoEnd; return; } // (never: the indexes are a permutation)
    const mcx_dup_unit u = units[at];
    key[i] = !is_pair(u) ? kDupNoEnd : second ? u.end1 : u.end0;
}
// in sorted order: a pair that is not the first of its key is a duplicate; a unit of no kind is none; flag: the head of a key that two or more share
__global__ void __launch_bounds__(256) k_pair_heads(const mcx_dup_unit *__restrict__ units, uint32_t n, const uint32_t *__restrict__ idx, uint8_t *dup, uint32_t *flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = 0;
    const uint32_t at = idx[i];
    if (at >= n) return;
    const mcx_dup_unit u = units[at];
    if (is_frag(u)) return; // (the fragments' table says)
    if (!is_pair(u)) { dup[at] = 0; return; }
    const bool head = i == 0 || idx[i - 1] >= n || !same_pair(units[idx[i - 1]], u);
    dup[at] = head ? 0 : 1;
    if (head && i + 1 < n && idx[i + 1] < n && same_pair(units[idx[i + 1]], u)) flag[i] = 1;
}

// entry e of the table: e < n the first end of unit e, else the second end of unit e - n
__device__ inline uint64_t frag_sec(const mcx_dup_unit &u, bool first)
{
    if (is_pair(u)) return 0;
    if (is_frag(u) && first) return 1ull << 32 | (uint64_t)(uint32_t)~u.score;
    return 2ull << 32;
}
__device__ inline uint64_t frag_end(const mcx_dup_unit &u, bool first)
{
    if (is_pair(u)) return first ? u.end0 : u.end1;
    if (is_frag(u) && first) return u.end0;
    return kDupNoEnd;
}
__global__ void __launch_bounds__(256) k_frag_sec(const mcx_dup_unit *__restrict__ units, uint32_t n, uint64_t *key, uint32_t *idx)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * n) return;
    key[e] = frag_sec(units[e < n ? e : e - n], e < n);
    idx[e] = e;
}
__global__ void __launch_bounds__(256) k_frag_end(const mcx_dup_unit *__restrict__ units, uint32_t n, const uint32_t *__restrict__ idx, uint64_t *key)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * n) return;
    const uint32_t e = idx[i];
    key[i] = e >= 2 * n ? kDupNoEnd : frag_end(units[e < n ? e : e - n], e < n);
}
__device__ inline bool dup_frag_at(const mcx_dup_unit *units, uint32_t n, const uint64_t *key, const uint32_t *idx, uint32_t i) // the entry at place i is a fragment that is not its segment's head
{
    const uint32_t e = idx[i];
    return e < n && is_frag(units[e]) && i > 0 && key[i - 1] == key[i];
}
__global__ void __launch_bounds__(256) k_frag_heads(const mcx_dup_unit *__restrict__ units, uint32_t n, const uint64_t *__restrict__ key, const uint32_t *__restrict__ idx, uint8_t *dup, uint32_t *flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * n) return;
    flag[i] = 0;
    const uint32_t e = idx[i];
    if (e >= n || !is_frag(units[e])) return;
    const bool d = dup_frag_at(units, n, key, idx, i);
    dup[e] = d ? 1 : 0;
    if (d && !dup_frag_at(units, n, key, idx, i - 1)) flag[i] = 1; // the first duplicate fragment of its end: one per group
}

__global__ void __launch_bounds__(256) k_mark_check(const uint64_t *__restrict__ rec_off, uint32_t n, uint64_t n_bytes, uint32_t *error)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = rec_off[i], b = rec_off[i + 1];
    if (a > b || b > n_bytes || b - a < 20) atomicOr(error, (uint32_t)kErrChain);
}
// perm (may be null): record i's byte is dup[perm[i]] — the merge's bytes come in the order the records had before they were sorted
__global__ void __launch_bounds__(256) k_dup_mark(uint8_t *recs, const uint64_t *__restrict__ rec_off, uint32_t n, const uint8_t *__restrict__ dup, const uint32_t *__restrict__ perm)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = perm ? perm[i] : i;
    if (at >= n || !dup[at]) return;
    uint8_t *p = recs + rec_off[i] + 19;
    *p = (uint8_t)(*p | 4u);
}

int units_lanes()
{
    // 1 M reads' records (290 MB, 500 000 pair units; scripts/markdup_rate.py), 16 / 32 / 64 lanes a unit: 0.300 / 0.527 / 0.890 ms — a 150-base QUAL is ten
    // 16-byte pieces, which leave most of a wider group idle while lane 0 walks the chain.  MCX_DUP_LANES=32 or 64 is the debug switch the other two were measured with
    static const int lanes = [] { const char *e = getenv("MCX_DUP_LANES"); const int v = e ? atoi(e) : 0; return v == 32 || v == 64 ? v : 16; }();
    return lanes;
}

int dup_ready(SamState *st)
{
    DupBufs &b = st->dup;
    for (hipEvent_t &e : b.ev) if (!e) HIP_TRY(hipEventCreate(&e));
    if (!b.d_error) HIP_TRY(hipMalloc((void **)&b.d_error, 16));
    return 0;
}

// the units of n_groups groups into the state's scratch (b.d_units); the context's device is current
int units_dev(mcx_ctx *c, SamState *st, const uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_grp_off, uint32_t n_groups, int paired, uint32_t n_units)
{
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    DupBufs &b = st->dup;
    int rc;
    if ((rc = dup_ready(st)) || (rc = sam_grow(&b.d_units, &b.cap_units, n_units, "the duplicate units of a part"))) return rc;
    b.ms[0] = 0;
    HIP_TRY(hipMemsetAsync(b.d_error, 0, 16, s));
    HIP_TRY(hipEventRecord(b.ev[0], s));
    const int lanes = units_lanes();
    const unsigned blocks = (unsigned)(((uint64_t)n_units * (uint64_t)lanes + 255) / 256);
    if (lanes == 64) k_dup_units<64><<<blocks, 256, 0, s>>>(d_recs, n_bytes, d_grp_off, n_groups, paired, n_units, b.d_units, b.d_error);
    else if (lanes == 32) k_dup_units<32><<<blocks, 256, 0, s>>>(d_recs, n_bytes, d_grp_off, n_groups, paired, n_units, b.d_units, b.d_error);
    else k_dup_units<16><<<blocks, 256, 0, s>>>(d_recs, n_bytes, d_grp_off, n_groups, paired, n_units, b.d_units, b.d_error);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b.ev[1], s));
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, b.d_error, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&b.ms[0], b.ev[0], b.ev[1]));
    if (err & kErrChain) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_dup_units_dev: the records' chain is broken: a group's offsets do not ascend to n_bytes, a block_size is below 32, a record leaves its group or is shorter than its name, CIGAR, SEQ and QUAL");
    if (err & kErrRange) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_dup_units_dev: a placed read lies outside what a packed end holds apart: a refID below 0 or of 2^24 - 1 or more, an unclipped 5' position of 2^38 or more either way, or 2^23 bases or more");
    return 0;
}

int table_room(SamState *st, uint64_t n, hipStream_t s)
{
    DupBufs &b = st->dup;
    const uint64_t m = 2 * n;
    size_t need_sort = 0, need_sum = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, need_sort, b.d_ka, b.d_kb, b.d_ia, b.d_ib, (int)m, 0, 64, s) != hipSuccess ||
        hipcub::DeviceReduce::Sum(nullptr, need_sum, b.d_flag, b.d_error, (int)m, s) != hipSuccess)
        return mcx_set_error(MCX_ERR_DEVICE, "the sorts over the duplicate units cannot be sized");
    const size_t need_tmp = std::max(need_sort, need_sum) + 256;
    if (m <= b.cap && need_tmp <= b.tmp_bytes) return 0;
    // all or nothing, and in words when HBM does not hold it
    const uint64_t need = m * 28 + need_tmp;
    b.drop_tables();
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need + (64ull << 20) > free_b)
        return mcx_set_error(MCX_ERR_CAPACITY, "the duplicate units' tables take " + std::to_string(need) + " bytes of HBM for " + std::to_string(n) + " units: more than is free (" + std::to_string(free_b) + ")");
    bool ok = hipMalloc((void **)&b.d_ka, m * 8) == hipSuccess && hipMalloc((void **)&b.d_kb, m * 8) == hipSuccess && hipMalloc((void **)&b.d_ia, m * 4) == hipSuccess &&
              hipMalloc((void **)&b.d_ib, m * 4) == hipSuccess && hipMalloc((void **)&b.d_flag, m * 4) == hipSuccess && hipMalloc(&b.d_tmp, need_tmp) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        b.drop_tables();
        return mcx_set_error(MCX_ERR_CAPACITY, "the duplicate units' tables take " + std::to_string(need) + " bytes of HBM for " + std::to_string(n) + " units: more than is free");
    }
    b.cap = m; b.tmp_bytes = need_tmp;
    return 0;
}

int resolve_dev(mcx_ctx *c, SamState *st, const mcx_dup_unit *d_units, uint32_t n, uint8_t *d_dup)
{
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    DupBufs &b = st->dup;
    int rc;
    if ((rc = dup_ready(st)) || (rc = table_room(st, n, s))) return rc;
    b.ms[1] = 0; b.groups = 0;
    const unsigned g1 = (n + 255) / 256, g2 = (2 * n + 255) / 256;
    auto sort = [&](const uint64_t *k_in, uint64_t *k_out, const uint32_t *i_in, uint32_t *i_out, uint32_t m, int bits) {
        size_t tmp = b.tmp_bytes;
        return hipcub::DeviceRadixSort::SortPairs(b.d_tmp, tmp, k_in, k_out, i_in, i_out, (int)m, 0, bits, s);
    };
    HIP_TRY(hipMemsetAsync(b.d_error, 0, 16, s));
    HIP_TRY(hipEventRecord(b.ev[0], s));
    k_pair_score<<<g1, 256, 0, s>>>(d_units, n, b.d_ka, b.d_ia, b.d_error);
    HIP_TRY(hipGetLastError());
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, b.d_error, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err) return mcx_set_error(MCX_ERR_ARG, "mcx_dup_resolve_dev: a unit's kind is none of 0 (none), 1 (fragment), 1 + 4 (the second read as a fragment) and 2 (pair)");
    // pairs: inverted score, second end, first end
    HIP_TRY(sort(b.d_ka, b.d_kb, b.d_ia, b.d_ib, n, 32));
    k_pair_key<<<g1, 256, 0, s>>>(d_units, n, b.d_ib, 1, b.d_ka);
    HIP_TRY(hipGetLastError());
    HIP_TRY(sort(b.d_ka, b.d_kb, b.d_ib, b.d_ia, n, 64));
    k_pair_key<<<g1, 256, 0, s>>>(d_units, n, b.d_ia, 0, b.d_ka);
    HIP_TRY(hipGetLastError());
    HIP_TRY(sort(b.d_ka, b.d_kb, b.d_ia, b.d_ib, n, 64));
    k_pair_heads<<<g1, 256, 0, s>>>(d_units, n, b.d_ib, d_dup, b.d_flag);
    HIP_TRY(hipGetLastError());
    size_t tmp = b.tmp_bytes;
    HIP_TRY(hipcub::DeviceReduce::Sum(b.d_tmp, tmp, b.d_flag, b.d_error + 1, (int)n, s));
    // fragments: (kind, inverted score), then the end
    k_frag_sec<<<g2, 256, 0, s>>>(d_units, n, b.d_ka, b.d_ia);
    HIP_TRY(hipGetLastError());
    HIP_TRY(sort(b.d_ka, b.d_kb, b.d_ia, b.d_ib, 2 * n, 34));
    k_frag_end<<<g2, 256, 0, s>>>(d_units, n, b.d_ib, b.d_ka);
    HIP_TRY(hipGetLastError());
    HIP_TRY(sort(b.d_ka, b.d_kb, b.d_ib, b.d_ia, 2 * n, 64));
    k_frag_heads<<<g2, 256, 0, s>>>(d_units, n, b.d_kb, b.d_ia, d_dup, b.d_flag);
    HIP_TRY(hipGetLastError());
    tmp = b.tmp_bytes;
    HIP_TRY(hipcub::DeviceReduce::Sum(b.d_tmp, tmp, b.d_flag, b.d_error + 2, (int)(2 * n), s));
    HIP_TRY(hipEventRecord(b.ev[1], s));
    uint32_t groups[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(groups, b.d_error + 1, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&b.ms[1], b.ev[0], b.ev[1]));
    b.groups = (uint64_t)groups[0] + groups[1];
    return 0;
}

// the marks: dup / perm as k_dup_mark's; the offsets are known to be whole
int mark_dev(mcx_ctx *c, SamState *st, uint8_t *d_recs, const uint64_t *d_rec_off, uint32_t n, const uint8_t *d_dup, const uint32_t *d_perm)
{
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    DupBufs &b = st->dup;
    HIP_TRY(hipEventRecord(b.ev[0], s));
    k_dup_mark<<<(n + 255) / 256, 256, 0, s>>>(d_recs, d_rec_off, n, d_dup, d_perm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b.ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&b.ms[2], b.ev[0], b.ev[1]));
    return 0;
}

} // namespace

extern "C" int mcx_bam_dup_units_dev(mcx_ctx *c, const uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_grp_off, uint32_t n_groups, int paired, mcx_dup_unit *d_units, uint64_t *n_units)
{
    if (n_units) *n_units = 0;
    if (!c || !n_units) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_dup_units_dev: null argument");
    if (paired && (n_groups & 1u)) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_dup_units_dev: paired reads come two by two: an odd number of groups");
    if (n_groups == 0) return 0;
    if (!d_grp_off || !d_units || (n_bytes && !d_recs)) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_dup_units_dev: null argument");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    const uint32_t n = paired ? n_groups / 2 : n_groups;
    if (int rc = units_dev(c, st, d_recs, n_bytes, d_grp_off, n_groups, paired ? 1 : 0, n)) return rc;
    HIP_TRY(hipMemcpy(d_units, st->dup.d_units, (size_t)n * sizeof(mcx_dup_unit), hipMemcpyDeviceToDevice));
    *n_units = n;
    return 0;
}

extern "C" int mcx_dup_resolve_dev(mcx_ctx *c, const mcx_dup_unit *d_units, uint64_t n_units, uint8_t *d_dup)
{
    if (!c) return mcx_set_error(MCX_ERR_ARG, "mcx_dup_resolve_dev: null argument");
    if (n_units == 0) return 0;
    if (!d_units || !d_dup) return mcx_set_error(MCX_ERR_ARG, "mcx_dup_resolve_dev: null argument");
    if (n_units >= (1ull << 30)) return mcx_set_error(MCX_ERR_CAPACITY, "the duplicate units' tables take " + std::to_string(n_units * 56) + " bytes and two entries a unit: " + std::to_string(n_units) + " units are more than one call sorts (2^30)");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    return resolve_dev(c, st, d_units, (uint32_t)n_units, d_dup);
}

extern "C" int mcx_bam_dup_mark_dev(mcx_ctx *c, uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_rec_off, uint32_t n_records, const uint8_t *d_rec_dup)
{
    if (!c) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_dup_mark_dev: null argument");
    if (n_records == 0) return 0;
    if (!d_recs || !d_rec_off || !d_rec_dup) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_dup_mark_dev: null argument");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    int rc;
    if ((rc = sam_state_of(c, &st)) || (rc = dup_ready(st))) return rc;
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    DupBufs &b = st->dup;
    b.ms[2] = 0;
    HIP_TRY(hipMemsetAsync(b.d_error, 0, 16, s));
    k_mark_check<<<(n_records + 255) / 256, 256, 0, s>>>(d_rec_off, n_records, n_bytes, b.d_error);
    HIP_TRY(hipGetLastError());
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, b.d_error, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_dup_mark_dev: the records' offsets descend, leave n_bytes, or leave a record less than the 20 bytes that end with its flag");
    return mark_dev(c, st, d_recs, d_rec_off, n_records, d_rec_dup, nullptr);
}

extern "C" int mcx_markdup_last_ms(mcx_ctx *c, float ms[3])
{
    SamState *st;
    if (!c || !ms) return mcx_set_error(MCX_ERR_ARG, "mcx_markdup_last_ms: null argument");
    if (int rc = sam_state_of(c, &st)) return rc;
    memcpy(ms, st->dup.ms, sizeof st->dup.ms);
    return 0;
}

// ---- the file front end's side (-markdup) --------------------------------------------------------------------------------------------------------------
static double seconds_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); }

// sam_part, before the part is sorted: the units of its records in read order (st->d_text, the groups at st->d_off) behind the run's units on the host
int mcx_markdup_part(mcx_ctx *c, uint32_t n_reads, uint64_t n_bytes, int paired, mcx_dup_sink *k)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (paired && (n_reads & 1u)) return mcx_set_error(MCX_ERR_DEVICE, "-markdup: a part of a paired run holds an odd number of reads: a pair straddles two parts, which the units cannot say");
    SamState *st;
    int rc;
    if ((rc = sam_state_of(c, &st))) return rc;
    const uint32_t n = paired ? n_reads / 2 : n_reads;
    k->part_base = k->units.size(); k->part_paired = paired ? 1 : 0;
    if (n == 0) return 0;
    if ((rc = units_dev(c, st, st->d_text, n_bytes, st->d_off, n_reads, paired ? 1 : 0, n)))
        return mcx_set_error(rc == MCX_ERR_ARG ? MCX_ERR_DEVICE : rc, std::string("-markdup: the part's records do not give their units: ") + mcx_last_error());
    k->units.resize(k->part_base + n);
    HIP_TRY(hipMemcpy(k->units.data() + k->part_base, st->dup.d_units, (size_t)n * sizeof(mcx_dup_unit), hipMemcpyDeviceToHost));
    k->ms[0] += st->dup.ms[0];
    k->seconds[0] += seconds_since(t0);
    return 0;
}

// behind the last batch: all units to HBM, one resolve, one byte a unit back; the tables go again
int mcx_markdup_resolve(mcx_ctx *c, mcx_dup_sink *k, std::vector<uint8_t> *dup)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = k->units.size();
    dup->assign((size_t)n, 0);
    k->groups = 0;
    if (n == 0) return 0;
    if (n >= (1ull << 30)) return mcx_set_error(MCX_ERR_CAPACITY, "-markdup: " + std::to_string(n) + " units are more than one resolve sorts (2^30)");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    int rc;
    if ((rc = sam_state_of(c, &st))) return rc;
    DupBufs &b = st->dup;
    if ((rc = sam_grow(&b.d_units, &b.cap_units, n, "the run's duplicate units")) || (rc = sam_grow(&b.d_dup, &b.cap_dup, n, "the run's duplicate units")))
        return rc == MCX_ERR_DEVICE ? mcx_set_error(MCX_ERR_CAPACITY, std::string("-markdup: ") + mcx_last_error()) : rc;
    HIP_TRY(hipMemcpy(b.d_units, k->units.data(), (size_t)n * sizeof(mcx_dup_unit), hipMemcpyHostToDevice));
    rc = resolve_dev(c, st, b.d_units, (uint32_t)n, b.d_dup);
    if (rc == 0 && hipMemcpy(dup->data(), b.d_dup, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "-markdup: the units' duplicate bytes do not come back");
    b.drop_tables();
    b.drop_run();
    if (rc) return rc == MCX_ERR_CAPACITY ? mcx_set_error(rc, std::string("-markdup: ") + mcx_last_error()) : rc;
    k->groups = b.groups;
    k->ms[1] += b.ms[1];
    k->seconds[1] += seconds_since(t0);
    return 0;
}

// a chunk of the merge, sorted and not yet deflated: h_dup, one byte a record in the order the chunk's records came in, goes through the sort's permutation
int mcx_markdup_chunk(mcx_ctx *c, mcx_dup_sink *k, uint8_t *d_recs, const uint64_t *d_rec_off, uint32_t n, const uint8_t *h_dup, const uint32_t *d_perm)
{
    const auto t0 = std::chrono::steady_clock::now();
    SamState *st;
    int rc;
    if ((rc = sam_state_of(c, &st)) || (rc = dup_ready(st))) return rc;
    DupBufs &b = st->dup;
    if ((rc = sam_grow(&b.d_bits, &b.cap_bits, n, "a chunk's duplicate bytes"))) return rc;
    HIP_TRY(hipMemcpyAsync(b.d_bits, h_dup, n, hipMemcpyHostToDevice, (hipStream_t)mcx_ctx_stream(c)));
    if ((rc = mark_dev(c, st, d_recs, d_rec_off, n, b.d_bits, d_perm))) return rc;
    k->ms[2] += b.ms[2];
    k->seconds[2] += seconds_since(t0);
    return 0;
}
