// mapcaller_amd/csrc/mcx_bai.hip — what a .bai is made of, read off coordinate-sorted BAM records in HBM that have just been deflated (mcx_bam_index_dev; the
// file front end's -index: every chunk of -sort's merge).  The rules are mcx_bai.h's; the host half there makes the file of what these kernels leave.
//
//   k_bai_records   one lane per record, bytes read one by one (records are not aligned): the length against the offsets, refID / pos / flag, the CIGAR walk for
//                   the end, the bin, the virtual offset from offset / block and offset % block, the windows a mapped record touches, and — against the record
//                   before it, read again from its own bytes — the order.  Anything wrong sets a bit of an error word: the call returns MCX_ERR_ARG before a
//                   byte of the outputs is written, and no byte outside d_recs[0 .. n_bytes) and the offset arrays is read
//   k_bai_heads     head flag: (refID, bin) differs from the record before
//   (scan)          inclusive sum over head << 32 | mapped: the stretch a record lies in and the mapped records up to it, in one pass
//   k_bai_starts    a stretch's first record; k_bai_runs: a lane per stretch writes its entry, the counts as differences of the running sums
//   (scan)          exclusive running maximum over (refID + 1) << 32 | (end window + 1) of the mapped records — refID ascends, so the maximum is the last contig's
//   k_bai_windows   a mapped record writes the windows that no earlier record of its contig reaches: from max(first window, running maximum + 1) to its end window.
//                   Every window of a call has exactly one writer, the first record that touches it, which is the one with the smallest offset: no atomics, and at
//                   depth — thousands of records in one 16 kb window — one store instead of thousands of atomic minima on the same 8 bytes.  An entry an earlier
//                   call wrote holds a smaller offset (the calls follow the file) and stays: the store is skipped unless the new offset is smaller.
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
#include "mcx_bai.h"
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

static_assert(sizeof(mcx_bai_run) == 24 && sizeof(bai::Run) == 24, "a stretch is 24 bytes on both sides");

namespace {

enum { kErrChain = 1, kErrPlace = 2, kErrOrder = 4 };
const int64_t kMaxPos = 1ll << 29; // BAI's reach

// the smallest bin that holds [beg, end) — mcx_bai.h's reg2bin, here for the device
__device__ inline uint32_t dev_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}
// what the order is checked on: contigs ascending, records without one last, positions ascending within a contig
__device__ inline uint64_t order_key(int32_t tid, int32_t pos) { return tid < 0 ? ~0ull : (uint64_t)(uint32_t)tid << 32 | (uint32_t)(pos + 1); }

__global__ void __launch_bounds__(256) k_bai_records(const uint8_t *__restrict__ recs, uint64_t n_bytes, const uint64_t *__restrict__ rec_off, uint32_t n, uint32_t block,
                                                     const uint64_t *__restrict__ block_at, uint32_t n_blocks, uint64_t file_at, const uint64_t *__restrict__ lin_base, uint32_t n_ref,
                                                     uint64_t *tb, uint64_t *u, uint64_t *wpack, uint32_t *w0, uint64_t *hm, uint32_t *error)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    tb[i] = 0; u[i] = 0; wpack[i] = 0; w0[i] = 0; hm[i] = 0;
    const uint64_t a = rec_off[i], b = rec_off[i + 1];
    if (a > b || b > n_bytes || (i == 0 && a != 0) || (i + 1 == n && b != n_bytes) || b - a < 4 + (uint64_t)kBamMinBlock) { atomicOr(error, (uint32_t)kErrChain); return; }
    const uint8_t *r = recs + a;
    const uint64_t len = b - a;
    const uint32_t l_name = r[12], n_cigar = (uint32_t)r[16] | (uint32_t)r[17] << 8, flag = (uint32_t)r[18] | (uint32_t)r[19] << 8;
    if (4 + (uint64_t)bam_get32(r) != len || 36 + (uint64_t)l_name + 4 * (uint64_t)n_cigar > len) { atomicOr(error, (uint32_t)kErrChain); return; }
    const int32_t tid = (int32_t)bam_get32(r + 4), pos = (int32_t)bam_get32(r + 8);
    const bool mapped = !(flag & 4u);
    // the order, against the record before (whose own lane says so when its offsets are broken)
    if (i > 0) {
        const uint64_t p = rec_off[i - 1];
        if (p <= a && a - p >= 12 && order_key((int32_t)bam_get32(recs + p + 4), (int32_t)bam_get32(recs + p + 8)) > order_key(tid, pos)) { atomicOr(error, (uint32_t)kErrOrder); return; }
    }
    const uint64_t blk = a / block;
    if (blk >= n_blocks) { atomicOr(error, (uint32_t)kErrChain); return; } // (the host checked n_blocks against n_bytes: never)
    u[i] = (file_at + block_at[blk]) << 16 | (a % block);
    hm[i] = mapped ? 1u : 0u;
    if (tid < 0) { tb[i] = 0xFFFFFFFFull << 32 | (uint32_t)bai::kNoCoorBin; return; }
    if ((uint32_t)tid >= n_ref || pos < -1) { atomicOr(error, (uint32_t)kErrPlace); return; }
    int64_t beg = pos, end = (int64_t)pos + 1;
    if (mapped) {
        int64_t ref_len = 0;
        const uint8_t *cg = r + 36 + l_name;
        for (uint32_t k = 0; k < n_cigar; k++) {
            const uint32_t w = bam_get32(cg + 4 * k), op = w & 15u;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += w >> 4; // M, D, N, = and X take reference
        }
        if (ref_len) end = (int64_t)pos + ref_len;
        if (beg < 0) beg = 0;
        if (end <= 0) end = 1;
    }
    if (beg > kMaxPos || end > kMaxPos) { atomicOr(error, (uint32_t)kErrPlace); return; }
    tb[i] = (uint64_t)(uint32_t)tid << 32 | dev_reg2bin(beg, end);
    if (mapped) {
        const uint64_t first = (uint64_t)(beg >> bai::kMinShift), last = (uint64_t)((end - 1) >> bai::kMinShift);
        if (last >= lin_base[tid + 1] - lin_base[tid]) { atomicOr(error, (uint32_t)kErrPlace); return; }
        w0[i] = (uint32_t)first;
        wpack[i] = (uint64_t)((uint32_t)tid + 1u) << 32 | (uint32_t)(last + 1);
    }
}

__global__ void __launch_bounds__(256) k_bai_heads(const uint64_t *__restrict__ tb, uint32_t n, uint64_t *hm)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i == 0 || tb[i] != tb[i - 1]) hm[i] |= 1ull << 32;
}

__global__ void __launch_bounds__(256) k_bai_starts(const uint64_t *__restrict__ hm, const uint64_t *__restrict__ hs, uint32_t n, uint32_t n_runs, uint32_t *start)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { start[n_runs] = n; return; }
    if (hm[i] >> 32) { const uint64_t r = (hs[i] >> 32) - 1; if (r < n_runs) start[r] = i; }
}

__global__ void __launch_bounds__(256) k_bai_runs(const uint64_t *__restrict__ tb, const uint64_t *__restrict__ u, const uint64_t *__restrict__ hs, const uint32_t *__restrict__ start, uint32_t n,
                                                  uint32_t n_runs, mcx_bai_run *runs)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    const uint32_t a = start[r], b = start[r + 1];
    if (a >= b || b > n) return; // (the scan found n_runs heads: never)
    const uint32_t mapped = (uint32_t)hs[b - 1] - (a ? (uint32_t)hs[a - 1] : 0u);
    mcx_bai_run e;
    e.ref_id = (int32_t)(uint32_t)(tb[a] >> 32); e.bin = (uint32_t)tb[a]; e.u = u[a]; e.n_mapped = mapped; e.n_unmapped = (b - a) - mapped;
    runs[r] = e;
}

__global__ void __launch_bounds__(256) k_bai_windows(const uint64_t *__restrict__ u, const uint64_t *__restrict__ wpack, const uint64_t *__restrict__ wmax, const uint32_t *__restrict__ w0, uint32_t n,
                                                     const uint64_t *__restrict__ lin_base, uint32_t n_ref, uint64_t *lin)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t mine = wpack[i];
    if (!mine) return;
    const uint32_t t = (uint32_t)(mine >> 32) - 1, last = (uint32_t)mine - 1;
    if (t >= n_ref) return;
    const uint64_t before = wmax[i]; // the highest window an earlier mapped record reaches, + 1, on the highest contig so far
    uint32_t from = w0[i];
    if (before >> 32 == mine >> 32 && (uint32_t)before > from) from = (uint32_t)before;
    const uint64_t base = lin_base[t], room = lin_base[t + 1] - base;
    const uint64_t off = u[i];
    for (uint64_t w = from; w <= last && w < room; w++)
        if (off < lin[base + w]) lin[base + w] = off;
}

template <class T> int grow(T **p, uint64_t *cap, uint64_t need, const char *what) { return sam_grow(p, cap, need, what); }

int bai_room(SamState *st, uint64_t n, hipStream_t s)
{
    BaiBufs &b = st->bai;
    for (hipEvent_t &e : b.ev) if (!e) HIP_TRY(hipEventCreate(&e));
    if (!b.d_error) HIP_TRY(hipMalloc((void **)&b.d_error, 8));
    const uint64_t m = n + 1;
    if (m <= b.cap) return 0;
    int rc;
    uint64_t cap;
    const char *what = "the index's per-record arrays";
    cap = b.cap; if ((rc = grow(&b.d_tb, &cap, m, what))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_u, &cap, m, what))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_wpack, &cap, m, what))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_wmax, &cap, m, what))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_hm, &cap, m, what))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_hs, &cap, m, what))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_w0, &cap, m, what))) return rc;
    cap = b.cap; if ((rc = grow(&b.d_start, &cap, m, what))) return rc;
    b.cap = cap;
    size_t need_sum = 0, need_max = 0;
    if (hipcub::DeviceScan::InclusiveSum(nullptr, need_sum, b.d_hm, b.d_hs, (int)b.cap, s) != hipSuccess ||
        hipcub::DeviceScan::ExclusiveScan(nullptr, need_max, b.d_wpack, b.d_wmax, hipcub::Max(), (uint64_t)0, (int)b.cap, s) != hipSuccess)
        return mcx_set_error(MCX_ERR_DEVICE, "the index's scans cannot be sized");
    const size_t need = std::max(need_sum, need_max) + 256;
    if (need > b.tmp_bytes) {
        if (b.d_tmp) (void)hipFree(b.d_tmp);
        b.d_tmp = nullptr; b.tmp_bytes = 0;
        if (hipMalloc(&b.d_tmp, need) != hipSuccess) { (void)hipGetLastError(); return mcx_set_error(MCX_ERR_DEVICE, "no room in HBM for the index's scans"); }
        b.tmp_bytes = need;
    }
    return 0;
}

// The call.  block_at: where the blocks lie, counted from file_at.  sink (the front end): the run list goes to the sink's array, which grows to hold it;
// otherwise to d_runs[0 .. runs_cap).  The context's device is current.
int index_dev(mcx_ctx *c, SamState *st, const uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_rec_off, uint32_t n, uint32_t block, const uint64_t *d_block_at, uint32_t n_blocks, uint64_t file_at,
              uint64_t *d_lin, const uint64_t *d_lin_base, uint32_t n_ref, mcx_bai_run *d_runs, uint64_t runs_cap, mcx_bai_sink *sink, uint64_t *n_runs)
{
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    BaiBufs &b = st->bai;
    if (int rc = bai_room(st, n, s)) return rc;
    memset(b.ms, 0, sizeof b.ms);
    const unsigned grid = (n + 255) / 256;
    HIP_TRY(hipMemsetAsync(b.d_error, 0, 8, s));
    HIP_TRY(hipEventRecord(b.ev[0], s));
    k_bai_records<<<grid, 256, 0, s>>>(d_recs, n_bytes, d_rec_off, n, block, d_block_at, n_blocks, file_at, d_lin_base, n_ref, b.d_tb, b.d_u, b.d_wpack, b.d_w0, b.d_hm, b.d_error);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b.ev[1], s));
    k_bai_heads<<<grid, 256, 0, s>>>(b.d_tb, n, b.d_hm);
    HIP_TRY(hipGetLastError());
    size_t tmp = b.tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(b.d_tmp, tmp, b.d_hm, b.d_hs, (int)n, s));
    uint32_t err = 0;
    uint64_t sums = 0;
    HIP_TRY(hipMemcpyAsync(&err, b.d_error, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&sums, b.d_hs + (n - 1), 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err & kErrChain) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_index_dev: the records' chain is broken: offsets that do not ascend from 0 to n_bytes, or a record that is not 4 + its block_size long or shorter than its name and CIGAR");
    if (err & kErrPlace) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_index_dev: a record lies where the index cannot say: a refID of n_ref or more, a position below -1, beyond 2^29 or beyond its contig's windows");
    if (err & kErrOrder) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_index_dev: the records are not in coordinate order: (refID, pos) descend, or a record on a contig follows one without");
    const uint32_t runs = (uint32_t)(sums >> 32);
    *n_runs = runs;
    if (sink) {
        if (int rc = grow(&sink->d_runs, &sink->cap_runs, runs, "the index's stretches")) return rc;
        d_runs = sink->d_runs; runs_cap = sink->cap_runs;
    }
    if (runs > runs_cap) return mcx_set_error(MCX_ERR_CAPACITY, "mcx_bam_index_dev: the records make " + std::to_string(runs) + " stretches: more than the list holds");
    k_bai_starts<<<(n + 1 + 255) / 256, 256, 0, s>>>(b.d_hm, b.d_hs, n, runs, b.d_start);
    HIP_TRY(hipGetLastError());
    k_bai_runs<<<(runs + 255) / 256, 256, 0, s>>>(b.d_tb, b.d_u, b.d_hs, b.d_start, n, runs, d_runs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b.ev[2], s));
    tmp = b.tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveScan(b.d_tmp, tmp, b.d_wpack, b.d_wmax, hipcub::Max(), (uint64_t)0, (int)n, s));
    k_bai_windows<<<grid, 256, 0, s>>>(b.d_u, b.d_wpack, b.d_wmax, b.d_w0, n, d_lin_base, n_ref, d_lin);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b.ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 3; k++) HIP_TRY(hipEventElapsedTime(&b.ms[k], b.ev[k], b.ev[k + 1]));
    return 0;
}

} // namespace

extern "C" int mcx_bam_index_dev(mcx_ctx *c, const uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_rec_off, uint32_t n_records, uint32_t block_text_bytes, const uint64_t *d_block_coff,
                                 uint32_t n_blocks, uint64_t *d_lin, const uint64_t *d_lin_base, uint32_t n_ref, mcx_bai_run *d_runs, uint64_t runs_cap, uint64_t *n_runs)
{
    if (n_runs) *n_runs = 0;
    if (!c || !n_runs) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_index_dev: null argument");
    if (n_records == 0) return 0;
    if (!d_recs || !d_rec_off || !d_block_coff || !d_lin || !d_lin_base || (!d_runs && runs_cap)) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_index_dev: null argument");
    if (block_text_bytes < 1 || block_text_bytes > 65536) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_index_dev: a BGZF block holds 1 to 65536 bytes of text");
    if (n_bytes / 36 < n_records || n_records >= 0x7FFFFFFFu) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_index_dev: more records than n_bytes hold, or than one call takes");
    if ((n_bytes + block_text_bytes - 1) / block_text_bytes != n_blocks) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_index_dev: n_blocks is not the number of blocks that n_bytes of text make");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    return index_dev(c, st, d_recs, n_bytes, d_rec_off, n_records, block_text_bytes, d_block_coff, n_blocks, 0, d_lin, d_lin_base, n_ref, d_runs, runs_cap, nullptr, n_runs);
}

extern "C" int mcx_bam_index_last_ms(mcx_ctx *c, float ms[3])
{
    SamState *st;
    if (!c || !ms) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_index_last_ms: null argument");
    if (int rc = sam_state_of(c, &st)) return rc;
    memcpy(ms, st->bai.ms, sizeof st->bai.ms);
    return 0;
}

// ---- the file front end's side (-index) ---------------------------------------------------------------------------------------------------------------
static double seconds_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); }

int mcx_bai_begin(mcx_ctx *c, mcx_bai_sink *k)
{
    const auto t0 = std::chrono::steady_clock::now();
    const HostIndex &hx = mcx_ctx_index(c)->host;
    k->acc.runs.clear();
    k->lin_base.assign(1, 0);
    for (int32_t len : hx.chr_len) k->lin_base.push_back(k->lin_base.back() + bai::windows_of(len));
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    mcx_bai_free(c, k);
    HIP_TRY(hipMalloc((void **)&k->d_lin, std::max<uint64_t>(k->lin_base.back(), 1) * 8));
    HIP_TRY(hipMalloc((void **)&k->d_lin_base, k->lin_base.size() * 8));
    HIP_TRY(hipMemset(k->d_lin, 0xff, k->lin_base.back() * 8));
    HIP_TRY(hipMemcpy(k->d_lin_base, k->lin_base.data(), k->lin_base.size() * 8, hipMemcpyHostToDevice));
    k->seconds += seconds_since(t0);
    return 0;
}

int mcx_bai_chunk(mcx_ctx *c, mcx_bai_sink *k, const uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_rec_off, uint32_t n_records, uint32_t block, mcx_deflater *def, uint64_t file_at)
{
    if (n_records == 0) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t *d_block_at = nullptr;
    uint64_t n_blocks = 0;
    if (int rc = mcx_bgzf_deflate_blocks(def, &d_block_at, &n_blocks)) return rc;
    if (n_blocks != (n_bytes + block - 1) / block || !d_block_at) return mcx_set_error(MCX_ERR_DEVICE, "-index: the deflater's blocks are not those of the chunk just compressed");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    uint64_t n_runs = 0;
    if (int rc = index_dev(c, st, d_recs, n_bytes, d_rec_off, n_records, block, d_block_at, (uint32_t)n_blocks, file_at, k->d_lin, k->d_lin_base, (uint32_t)k->lin_base.size() - 1, nullptr, 0, k, &n_runs))
        return rc == MCX_ERR_ARG ? mcx_set_error(MCX_ERR_DEVICE, std::string("-index: the sorted records cannot be indexed: ") + mcx_last_error()) : rc;
    k->h_runs.resize((size_t)n_runs);
    HIP_TRY(hipMemcpy(k->h_runs.data(), k->d_runs, (size_t)n_runs * sizeof(mcx_bai_run), hipMemcpyDeviceToHost));
    if (!k->acc.push((const bai::Run *)k->h_runs.data(), n_runs)) return mcx_set_error(MCX_ERR_DEVICE, "-index: a chunk's records do not follow those of the chunk before");
    for (int j = 0; j < 3; j++) k->ms[j] += st->bai.ms[j];
    k->seconds += seconds_since(t0);
    return 0;
}

int mcx_bai_end(mcx_ctx *c, mcx_bai_sink *k, uint64_t eof_at, std::vector<uint8_t> *bytes)
{
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    std::vector<uint64_t> lin((size_t)k->lin_base.back());
    if (!lin.empty()) HIP_TRY(hipMemcpy(lin.data(), k->d_lin, lin.size() * 8, hipMemcpyDeviceToHost));
    if (!k->acc.finish((uint32_t)k->lin_base.size() - 1, eof_at << 16, lin.data(), k->lin_base.data(), bytes, &k->stats))
        return mcx_set_error(MCX_ERR_DEVICE, "-index: the stretches name a contig or a bin that does not exist");
    k->seconds += seconds_since(t0);
    return 0;
}

void mcx_bai_free(mcx_ctx *c, mcx_bai_sink *k)
{
    (void)hipSetDevice(mcx_ctx_index(c)->device);
    void *p[] = {k->d_lin, k->d_lin_base, k->d_runs};
    for (void *q : p) if (q) (void)hipFree(q);
    k->d_lin = k->d_lin_base = nullptr; k->d_runs = nullptr; k->cap_runs = 0;
}
