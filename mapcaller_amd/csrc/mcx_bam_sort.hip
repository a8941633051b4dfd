// mapcaller_amd/csrc/mcx_bam_sort.hip — BAM records in HBM put into coordinate order (mcx_bam_sort_dev; the file front end's -sort: every part's run, and every
// chunk of the merge behind the last batch).  The order is mcx_bam_sort.h's.
//
//   k_sort_count   one lane per group (a read's records: none, one, a few under -m) walks the block_size chain inside its group and counts the records; the walk
//                  is bounded by the group: a chain that leaves it, a block_size below 32, offsets that do not ascend to n_bytes set an error word, the call
//                  returns MCX_ERR_ARG before anything else runs, and no byte outside [0, n_bytes) is read
//   (scan)         exclusive sum over the counts: the first record of every group, the last entry the number of records
//   k_sort_index   the same walk again: each record's source offset, length (4 + block_size), key and index
//   (sort)         hipcub::DeviceRadixSort::SortPairs over (key, index), all 64 bits (refID -1 sets the highest); stable
//   k_sort_lens    the lengths in sorted order; (scan) their exclusive sum: where every record goes
//   k_sort_gather  the records from their unaligned places to their unaligned places.  16 lanes share a record: the bytes ahead of the destination's first
//                  16-byte boundary and behind its last go as bytes, a lane each; everything between goes in aligned 16-byte stores, each made of the two
//                  aligned 16-byte words of the source that hold its bytes, shifted together in registers (no LDS: a record of any length takes the same
//                  path, piece by piece).  An aligned source word that reaches outside [0, n_bytes) — only the buffer's first and last — is read byte by byte,
//                  its bytes inside the buffer only.  Nothing wider than a byte touches an address that is not naturally aligned.
//                  A part of a wavefront per record, not a whole one, by measurement: at ~290 bytes a record has 18 pieces of 16 bytes, which leave 46 of 64
//                  lanes idle.  1 M reads' records, 16 / 32 / 64 lanes a record: 0.183 / 0.242 / 0.395 ms (scripts/sort_rate.py; MCX_SORT_LANES=32
//                  or 64 is the debug switch the other two were measured with).
// The merge's chunks come with stored lengths, not a chain to walk: sort_core takes per-record (offset, length, key) arrays, and both callers share every stage
// from the sort on.
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
#include "mcx_bam_sort.h"
#include "mcx_internal.h"
#include "mcx_sam_state.h"

using namespace mcx;

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace {

// the chain of group g: calls f(offset, length) for each record; false when the chain is broken (f is not called for the record that breaks it)
template <class F> __device__ inline bool walk_group(const uint8_t *recs, uint64_t n_bytes, const uint64_t *grp_off, uint32_t g, uint32_t n_groups, F f)
{
    const uint64_t a = grp_off[g], b = grp_off[g + 1];
    if (a > b || b > n_bytes || (g == 0 && a != 0) || (g + 1 == n_groups && b != n_bytes)) return false;
    uint64_t p = a;
    while (p < b) { // (every turn advances by 36 bytes or more)
        if (b - p < 4 + (uint64_t)kBamMinBlock) return false;
        const uint64_t len = 4 + (uint64_t)bam_get32(recs + p);
        if (len < 4 + (uint64_t)kBamMinBlock || len > b - p) return false;
        f(p, (uint32_t)len);
        p += len;
    }
    return true;
}

__global__ void __launch_bounds__(256) k_sort_count(const uint8_t *__restrict__ recs, uint64_t n_bytes, const uint64_t *__restrict__ grp_off, uint32_t n_groups, uint32_t *count, uint32_t *error)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > n_groups) return;
    uint32_t n = 0;
    if (g < n_groups && !walk_group(recs, n_bytes, grp_off, g, n_groups, [&n](uint64_t, uint32_t) { n++; })) { n = 0; atomicOr(error, 1u); }
    count[g] = n; // (one entry more: the scan leaves the total there)
}

__global__ void __launch_bounds__(256) k_sort_index(const uint8_t *__restrict__ recs, uint64_t n_bytes, const uint64_t *__restrict__ grp_off, uint32_t n_groups, const uint32_t *__restrict__ first,
                                                    uint64_t *src_off, uint32_t *len, uint64_t *key, uint32_t *idx)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    uint32_t i = first[g];
    const uint32_t end = first[g + 1]; // (the count pass found the chain whole; the bound keeps a buffer that changed in between from writing past the arrays)
    walk_group(recs, n_bytes, grp_off, g, n_groups, [&](uint64_t p, uint32_t l) {
        if (i < end) { src_off[i] = p; len[i] = l; key[i] = bam_sort_key(recs + p); idx[i] = i; i++; }
    });
}

// the merge: record i of a chunk lies in slice s (first[s] <= i < first[s + 1]) at base[s] + the lengths of the slice's records before it
__global__ void __launch_bounds__(256) k_sort_slice_index(const uint8_t *__restrict__ text, uint64_t text_bytes, const uint64_t *__restrict__ len_sum, const uint32_t *__restrict__ len, uint32_t n,
                                                          const uint64_t *__restrict__ slice_first, const uint64_t *__restrict__ slice_base, uint32_t n_slices,
                                                          uint64_t *src_off, uint64_t *key, uint32_t *idx, uint32_t *error)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t a = 0, z = n_slices;
    while (z - a > 1) { const uint32_t m = (a + z) / 2; if (slice_first[m] <= i) a = m; else z = m; }
    const uint64_t p = slice_base[a] + (len_sum[i] - len_sum[slice_first[a]]);
    const uint32_t l = len[i];
    idx[i] = i;
    if (l < 4u + (uint32_t)kBamMinBlock || p > text_bytes || l > text_bytes - p || 4 + (uint64_t)bam_get32(text + p) != l) { // (the blocks read back are not the ones written)
        atomicOr(error, 1u);
        src_off[i] = 0; key[i] = 0;
        return;
    }
    src_off[i] = p; key[i] = bam_sort_key(text + p);
}

__global__ void __launch_bounds__(256) k_sort_lens(const uint32_t *__restrict__ idx_sorted, const uint32_t *__restrict__ len, uint32_t n, uint32_t *len_sorted)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    len_sorted[i] = i < n ? len[idx_sorted[i]] : 0;
}

// -markdup: the group a sorted record came from — record r in read order lies in the last group g with first[g] <= r (the empty groups before it share its entry)
__global__ void __launch_bounds__(256) k_sort_groups(const uint32_t *__restrict__ idx_sorted, const uint32_t *__restrict__ first, uint32_t n_groups, uint32_t n, uint32_t *grp)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = idx_sorted[i];
    uint32_t a = 0, z = n_groups;
    while (z - a > 1) { const uint32_t m = (a + z) / 2; if (first[m] <= r) a = m; else z = m; }
    grp[i] = a;
}

// the aligned 16 bytes at p, of which only those inside [lo, hi) are read (the others come as 0)
__device__ inline uint4 load16_inside(const uint8_t *p, const uint8_t *lo, const uint8_t *hi)
{
    if (p >= lo && p + 16 <= hi) return *(const uint4 *)p;
    uint32_t w[4] = {0, 0, 0, 0};
    for (int k = 0; k < 16; k++) if (p + k >= lo && p + k < hi) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int LANES> __global__ void __launch_bounds__(256) k_sort_gather(const uint8_t *__restrict__ recs, uint64_t n_bytes, const uint32_t *__restrict__ idx_sorted, const uint64_t *__restrict__ src_off,
                                                                          const uint32_t *__restrict__ len_sorted, const uint64_t *__restrict__ dst_off, uint32_t n, uint8_t *out)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i = t / LANES;
    const uint32_t lane = (uint32_t)(t % LANES);
    if (i >= n) return;
    const uint32_t L = len_sorted[i];
    const uint8_t *src = recs + src_off[idx_sorted[i]];
    uint8_t *dst = out + dst_off[i];
    const uint32_t to16 = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
    const uint32_t head = to16 < L ? to16 : L, n16 = (L - head) >> 4, tail_at = head + (n16 << 4);
    if (lane < head) dst[lane] = src[lane];               // (head and tail are below 16 bytes, LANES is 16 or more)
    if (tail_at + lane < L) dst[tail_at + lane] = src[tail_at + lane];
    const uint8_t *s0 = src + head;                        // the source of the first aligned piece
    const uint32_t m = (uint32_t)((uintptr_t)s0 & 15u), q = m >> 2, r8 = (m & 3u) * 8;
    const uint8_t *sa = s0 - m;                            // ... and the aligned word that holds its first byte
    uint4 *d16 = (uint4 *)(dst + head);
    const uint8_t *lo = recs, *hi = recs + n_bytes;
    for (uint32_t j = lane; j < n16; j += LANES) {
        const uint4 A = load16_inside(sa + 16 * (size_t)j, lo, hi);
        uint4 B = make_uint4(0, 0, 0, 0);
        if (m) B = load16_inside(sa + 16 * (size_t)j + 16, lo, hi);
        // the 16 bytes from byte m of A|B: whole words first, then the bytes within a word
        uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
        if (q & 1u) { for (int k = 0; k < 7; k++) w[k] = w[k + 1]; }
        if (q & 2u) { for (int k = 0; k < 6; k++) w[k] = w[k + 2]; }
        uint4 o;
        if (r8) {
            o.x = (w[0] >> r8) | (w[1] << (32 - r8)); o.y = (w[1] >> r8) | (w[2] << (32 - r8));
            o.z = (w[2] >> r8) | (w[3] << (32 - r8)); o.w = (w[3] >> r8) | (w[4] << (32 - r8));
        } else o = make_uint4(w[0], w[1], w[2], w[3]);
        d16[j] = o;
    }
}

// the lengths are 32-bit, their sums are not: the scans read them as 64-bit values
struct To64 { __host__ __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; } };
typedef hipcub::TransformInputIterator<uint64_t, To64, const uint32_t *> Len64;

int sort_lanes()
{
    static const int lanes = [] { const char *e = getenv("MCX_SORT_LANES"); const int v = e ? atoi(e) : 0; return v == 32 || v == 64 ? v : 16; }();
    return lanes;
}

template <class T> int grow(T **p, uint64_t *cap, uint64_t need, const char *what) { return sam_grow(p, cap, need, what); }

int tmp_room(SortBufs &b, size_t need)
{
    if (need <= b.tmp_bytes) return 0;
    if (b.d_tmp) (void)hipFree(b.d_tmp);
    b.d_tmp = nullptr; b.tmp_bytes = 0;
    if (hipMalloc(&b.d_tmp, need) != hipSuccess) { (void)hipGetLastError(); return mcx_set_error(MCX_ERR_DEVICE, "no room in HBM for the sort over the records' keys"); }
    b.tmp_bytes = need;
    return 0;
}
// room for n records' arrays (and one entry more where a scan leaves a total) and for the scratch of hipcub's sort and scan at that size
int sort_room(SamState *st, uint64_t n, hipStream_t s)
{
    SortBufs &b = st->sort;
    int rc;
    uint64_t cap;
    const uint64_t m = n + 1;
    if (m <= b.cap) return 0;
    cap = b.cap; if ((rc = grow(&b.d_src_off, &cap, m, "the sort's record offsets"))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_dst_off, &cap, m, "the sort's record offsets"))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_key, &cap, m, "the sort's keys"))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_key_s, &cap, m, "the sort's keys"))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_len, &cap, m, "the sort's record lengths"))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_len_s, &cap, m, "the sort's record lengths"))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_idx, &cap, m, "the sort's record indexes"))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_idx_s, &cap, m, "the sort's record indexes"))) return rc;
    b.cap = cap;
    size_t need_sort = 0, need_scan = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, need_sort, b.d_key, b.d_key_s, b.d_idx, b.d_idx_s, (int)b.cap, 0, 64, s) != hipSuccess ||
        hipcub::DeviceScan::ExclusiveSum(nullptr, need_scan, Len64(b.d_len_s, To64()), b.d_dst_off, (int)b.cap, s) != hipSuccess)
        return mcx_set_error(MCX_ERR_DEVICE, "the sort over the records' keys cannot be sized");
    return tmp_room(b, std::max(need_sort, need_scan) + 256);
}
// ... and for the groups' counts
int group_room(SamState *st, uint64_t n_groups, hipStream_t s)
{
    SortBufs &b = st->sort;
    int rc;
    uint64_t cap = b.cap_groups;
    if (n_groups + 1 <= cap) return 0;
    if ((rc = grow(&b.d_count, &cap, n_groups + 1, "the sort's record counts"))) return rc;
    cap = b.cap_groups; if ((rc = grow(&b.d_first, &cap, n_groups + 1, "the sort's record counts"))) return rc;
    b.cap_groups = cap;
    size_t need = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, need, b.d_count, b.d_first, (int)b.cap_groups, s) != hipSuccess) return mcx_set_error(MCX_ERR_DEVICE, "the scan over the records' counts cannot be sized");
    return tmp_room(b, need + 256);
}
int sort_events(SamState *st)
{
    for (hipEvent_t &e : st->sort.ev) if (!e) HIP_TRY(hipEventCreate(&e));
    if (!st->sort.d_error) HIP_TRY(hipMalloc((void **)&st->sort.d_error, 8));
    return 0;
}

// From the sort on: n records of d_recs[0 .. n_bytes) at d_src_off[i] with d_len[i] and d_key[i] (d_idx[i] = i) in the state's arrays -> d_out, contiguous and in
// key order; d_keys / d_lens (may be null): per output record.  Events 1 .. 4 bracket sort, place and gather; the caller waits and reads them.
int sort_core(SamState *st, hipStream_t s, const uint8_t *d_recs, uint64_t n_bytes, uint32_t n, uint8_t *d_out, uint64_t *d_keys, uint32_t *d_lens)
{
    SortBufs &b = st->sort;
    uint64_t *key_s = d_keys ? d_keys : b.d_key_s;
    HIP_TRY(hipEventRecord(b.ev[1], s));
    size_t tmp = b.tmp_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(b.d_tmp, tmp, b.d_key, key_s, b.d_idx, b.d_idx_s, (int)n, 0, 64, s));
    HIP_TRY(hipEventRecord(b.ev[2], s));
    k_sort_lens<<<(n + 1 + 255) / 256, 256, 0, s>>>(b.d_idx_s, b.d_len, n, b.d_len_s);
    HIP_TRY(hipGetLastError());
    tmp = b.tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b.d_tmp, tmp, Len64(b.d_len_s, To64()), b.d_dst_off, (int)(n + 1), s));
    if (d_lens) HIP_TRY(hipMemcpyAsync(d_lens, b.d_len_s, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipEventRecord(b.ev[3], s));
    const int lanes = sort_lanes();
    const uint64_t threads = (uint64_t)n * (uint64_t)lanes;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    if (lanes == 64) k_sort_gather<64><<<blocks, 256, 0, s>>>(d_recs, n_bytes, b.d_idx_s, b.d_src_off, b.d_len_s, b.d_dst_off, n, d_out);
    else if (lanes == 32) k_sort_gather<32><<<blocks, 256, 0, s>>>(d_recs, n_bytes, b.d_idx_s, b.d_src_off, b.d_len_s, b.d_dst_off, n, d_out);
    else k_sort_gather<16><<<blocks, 256, 0, s>>>(d_recs, n_bytes, b.d_idx_s, b.d_src_off, b.d_len_s, b.d_dst_off, n, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b.ev[4], s));
    return 0;
}
int core_times(SamState *st)
{
    SortBufs &b = st->sort;
    for (int k = 0; k < 4; k++) HIP_TRY(hipEventElapsedTime(&b.ms[k], b.ev[k], b.ev[k + 1]));
    return 0;
}

int sort_dev(mcx_ctx *c, SamState *st, const uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_grp_off, uint32_t n_groups, uint8_t *d_out, uint64_t *d_keys, uint32_t *d_lens, uint64_t *n_records)
{
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    SortBufs &b = st->sort;
    int rc;
    if ((rc = sort_events(st)) || (rc = group_room(st, n_groups, s))) return rc;
    memset(b.ms, 0, sizeof b.ms);
    HIP_TRY(hipMemsetAsync(b.d_error, 0, 8, s));
    HIP_TRY(hipEventRecord(b.ev[0], s));
    k_sort_count<<<(unsigned)(((uint64_t)n_groups + 1 + 255) / 256), 256, 0, s>>>(d_recs, n_bytes, d_grp_off, n_groups, b.d_count, b.d_error);
    HIP_TRY(hipGetLastError());
    size_t tmp = b.tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b.d_tmp, tmp, b.d_count, b.d_first, (int)(n_groups + 1), s));
    uint32_t h[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&h[0], b.d_first + n_groups, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h[1], b.d_error, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h[1]) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_sort_dev: the records' chain is broken: a group's offsets do not ascend to n_bytes, a block_size is below 32, or a record leaves its group");
    const uint32_t n = h[0];
    if (n_records) *n_records = n;
    if (n == 0) return 0;
    if ((rc = sort_room(st, n, s))) return rc;
    k_sort_index<<<(n_groups + 255) / 256, 256, 0, s>>>(d_recs, n_bytes, d_grp_off, n_groups, b.d_first, b.d_src_off, b.d_len, b.d_key, b.d_idx);
    HIP_TRY(hipGetLastError());
    if ((rc = sort_core(st, s, d_recs, n_bytes, n, d_out, d_keys, d_lens))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return core_times(st);
}

} // namespace

extern "C" int mcx_bam_sort_dev(mcx_ctx *c, const uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_grp_off, uint32_t n_groups, uint8_t *d_out, uint64_t cap,
                                uint64_t *d_keys, uint32_t *d_lens, uint64_t *n_records)
{
    if (n_records) *n_records = 0;
    if (!c) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_sort_dev: null argument");
    if (n_groups == 0) return 0;
    if (!d_grp_off || (n_bytes && (!d_recs || !d_out))) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_sort_dev: null argument");
    if (cap < n_bytes) return mcx_set_error(MCX_ERR_CAPACITY, "the sorted records take " + std::to_string(n_bytes) + " bytes: more than the buffer holds");
    if (n_bytes / 36 >= 0xFFFFFFFFull) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_sort_dev: more records than one call sorts");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    return sort_dev(c, st, d_recs, n_bytes, d_grp_off, n_groups, d_out, d_keys, d_lens, n_records);
}

// the last call's device times in ms: index, sort, place, gather (scripts/sort_rate.py)
extern "C" int mcx_bam_sort_last_ms(mcx_ctx *c, float ms[4])
{
    SamState *st;
    if (!c || !ms) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_sort_last_ms: null argument");
    if (int rc = sam_state_of(c, &st)) return rc;
    memcpy(ms, st->sort.ms, sizeof st->sort.ms);
    return 0;
}

// sam_part with -sort: the part's records (st->d_text, the groups at st->d_off) in key order into the state's second buffer; keys and lengths to the run's sink
int mcx_bam_sort_part(mcx_ctx *c, uint32_t n_reads, uint64_t n_bytes, mcx_sort_sink *sink, const uint8_t **d_sorted)
{
    SamState *st;
    int rc;
    if ((rc = sam_state_of(c, &st))) return rc;
    SortBufs &b = st->sort;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = sam_grow(&b.d_sorted, &b.cap_sorted, n_bytes + 16, "the part's sorted BAM records"))) return rc;
    uint64_t n = 0;
    if ((rc = sort_dev(c, st, st->d_text, n_bytes, st->d_off, n_reads, b.d_sorted, nullptr, nullptr, &n))) return rc;
    sink->keys.resize((size_t)n); sink->lens.resize((size_t)n);
    if (n) {
        HIP_TRY(hipMemcpy(sink->keys.data(), b.d_key_s, (size_t)n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(sink->lens.data(), b.d_len_s, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    if (sink->dup) { // -markdup: which group each sorted record came from (d_idx, the sort's input, is free again)
        sink->dup->grp.resize((size_t)n);
        if (n) {
            k_sort_groups<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)mcx_ctx_stream(c)>>>(b.d_idx_s, b.d_first, n_reads, (uint32_t)n, b.d_idx);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(sink->dup->grp.data(), b.d_idx, (size_t)n * 4, hipMemcpyDeviceToHost));
        }
    }
    sink->run_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *d_sorted = b.d_sorted;
    return 0;
}

// The merge's chunk: the covering blocks of its slices (src: page-locked, src_bytes with 8 bytes of slack behind the last member) are inflated into HBM in one
// row (members: dst_off in that row, text_bytes of it), the records — lens[n_records] in (run, index) order; slice k's start at record slice_first[k], byte
// slice_base[k] of the row — are sorted by the core, deflated, and their blocks brought to (*h_out)[0 .. *n_out), a page-locked buffer that grows as needed.
// bai (-index; null: none): the chunk's blocks will lie at byte file_at of the file, and its records are indexed before they leave HBM (mcx_bai.hip).
// dup (-markdup; null: none): dup_bytes[n_records], in the lengths' order, say which records get flag bit 0x400 once they are sorted, before they are deflated.
int mcx_bam_sort_chunk(mcx_ctx *c, mcx_inflater *inf, mcx_deflater *def, uint32_t block, const uint8_t *src, uint64_t src_bytes, const mcx_deflate_member *members, uint32_t n_members,
                       uint64_t text_bytes, const uint32_t *lens, uint64_t n_records, const uint64_t *slice_first, const uint64_t *slice_base, uint32_t n_slices, uint64_t rec_bytes,
                       uint8_t **h_out, uint64_t *h_out_cap, uint64_t *n_out, double secs[4], mcx_bai_sink *bai, uint64_t file_at, mcx_dup_sink *dup, const uint8_t *dup_bytes)
{
    *n_out = 0;
    if (n_records == 0) return 0;
    if (n_records >= 0xFFFFFFFFull) return mcx_set_error(MCX_ERR_CAPACITY, "-sort: one chunk of the merge holds more records than a call sorts (a pile-up on one position)");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    int rc;
    if ((rc = sam_state_of(c, &st))) return rc;
    SortBufs &b = st->sort;
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    const uint32_t n = (uint32_t)n_records;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    const uint64_t bound = mcx_bgzf_bound(rec_bytes, block);
    const char *chunk_what = "a chunk of the merge (-sort; a pile-up on one position makes a chunk that HBM must hold whole)";
    if ((rc = sort_events(st)) || (rc = sort_room(st, n, s))) return rc;
    if ((rc = sam_grow(&b.d_src, &b.cap_src, src_bytes + 16, chunk_what)) || (rc = sam_grow(&b.d_members, &b.cap_members, (uint64_t)n_members + 1, chunk_what)) ||
        (rc = sam_grow(&b.d_status, &b.cap_status, (uint64_t)n_members + 1, chunk_what)) || (rc = sam_grow(&b.d_inflated, &b.cap_inflated, text_bytes + 16, chunk_what)) ||
        (rc = sam_grow(&b.d_sorted, &b.cap_sorted, rec_bytes + 16, chunk_what)) || (rc = sam_grow(&b.d_slices, &b.cap_slices, 2 * (uint64_t)n_slices + 2, chunk_what)) ||
        (rc = sam_grow(&st->d_bgzf, &st->cap_bgzf, bound, chunk_what)))
        return rc == MCX_ERR_DEVICE ? mcx_set_error(MCX_ERR_CAPACITY, std::string("-sort: ") + mcx_last_error()) : rc;
    // in: blocks, members, lengths, slices
    auto t0 = now();
    HIP_TRY(hipMemcpyAsync(b.d_src, src, src_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.d_members, members, (size_t)n_members * sizeof(mcx_deflate_member), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.d_len, lens, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(b.d_len + n, 0, 4, s));
    HIP_TRY(hipMemcpyAsync(b.d_slices, slice_first, (size_t)n_slices * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b.d_slices + n_slices, slice_base, (size_t)n_slices * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(b.d_error, 0, 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    secs[0] += since(t0);
    // inflate: as many members a launch as the inflater takes
    t0 = now();
    uint64_t max_src = 0, max_dst = 0; uint32_t max_members = 0;
    mcx_inflater_caps(inf, &max_src, &max_dst, &max_members);
    for (uint32_t k = 0; k < n_members; k += max_members)
        if ((rc = mcx_inflate_dev(inf, b.d_src, src_bytes, b.d_members + k, std::min(max_members, n_members - k), b.d_inflated, text_bytes, b.d_status + k)))
            return mcx_set_error(rc, std::string("-sort: the temporary file's blocks do not inflate: ") + mcx_last_error());
    secs[1] += since(t0);
    // sort
    t0 = now();
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    HIP_TRY(hipEventRecord(b.ev[0], s));
    size_t tmp = b.tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b.d_tmp, tmp, Len64(b.d_len, To64()), b.d_dst_off, (int)(n + 1), s));
    k_sort_slice_index<<<(n + 255) / 256, 256, 0, s>>>(b.d_inflated, text_bytes, b.d_dst_off, b.d_len, n, b.d_slices, b.d_slices + n_slices, n_slices, b.d_src_off, b.d_key, b.d_idx, b.d_error);
    HIP_TRY(hipGetLastError());
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, b.d_error, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err) return mcx_set_error(MCX_ERR_IO, "-sort: the records read back from the temporary file are not the ones written");
    if ((rc = sort_core(st, s, b.d_inflated, text_bytes, n, b.d_sorted, nullptr, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = core_times(st))) return rc;
    if (dup && (rc = mcx_markdup_chunk(c, dup, b.d_sorted, b.d_dst_off, n, dup_bytes, b.d_idx_s))) return rc;
    secs[2] += since(t0);
    // deflate and out
    t0 = now();
    uint64_t made = 0;
    if ((rc = mcx_bgzf_deflate_dev(def, b.d_sorted, rec_bytes, st->d_bgzf, st->cap_bgzf, &made))) return rc;
    // -index: the sorted records are still there, their destination offsets are the scan's, and the deflater knows where every block went
    if (bai) {
        const auto ti = now();
        if ((rc = mcx_bai_chunk(c, bai, b.d_sorted, rec_bytes, b.d_dst_off, n, block, def, file_at))) return rc;
        t0 += now() - ti; // (the sink keeps its own time)
    }
    if (made > *h_out_cap) {
        mcx_pinned_free(*h_out);
        *h_out_cap = 0;
        const uint64_t want = made + made / 8 + 4096;
        *h_out = (uint8_t *)mcx_pinned_alloc(want);
        if (!*h_out) return mcx_set_error(MCX_ERR_DEVICE, "-sort: cannot allocate pinned host memory for a chunk's blocks");
        *h_out_cap = want;
    }
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    HIP_TRY(hipMemcpyAsync(*h_out, st->d_bgzf, made, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    secs[3] += since(t0);
    *n_out = made;
    return 0;
}

extern "C" int mcx_bam_header_sorted(const mcx_index *ix, uint8_t *out, uint64_t cap, uint64_t *n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    if (!ix) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_header_sorted: null argument");
    // mcx_bam_header's bytes with one line ahead of the text: l_text grows by its length
    uint64_t n = 0;
    (void)mcx_bam_header(ix, nullptr, 0, &n);
    std::vector<uint8_t> h((size_t)n);
    if (n < 8) return mcx_set_error(MCX_ERR_UNSUPPORTED, std::string("mcx_bam_header_sorted: ") + mcx_last_error());
    if (int rc = mcx_bam_header(ix, h.data(), n, &n)) return rc;
    static const char hd[] = "@HD\tVN:1.6\tSO:coordinate\n";
    const uint32_t add = (uint32_t)(sizeof hd - 1), l_text = bam_get32(h.data() + 4) + add;
    std::vector<uint8_t> g;
    g.insert(g.end(), h.begin(), h.begin() + 4);
    for (int k = 0; k < 4; k++) g.push_back((uint8_t)(l_text >> (8 * k)));
    g.insert(g.end(), hd, hd + add);
    g.insert(g.end(), h.begin() + 8, h.end());
    if (n_bytes) *n_bytes = g.size();
    if (g.size() > cap || !out) return mcx_set_error(MCX_ERR_CAPACITY, "the BAM header takes " + std::to_string(g.size()) + " bytes: more than the buffer holds");
    memcpy(out, g.data(), g.size());
    return 0;
}
