// mapcaller_amd/csrc/mcx_md.hip — a mapped batch's MD:Z strings made in HBM (mcx_md_dev, mcx_md, mcx_md_last_ms; the file front end's -md).
//
// The strings are mcx_md.h's (include/mcx.h defines them): what `samtools calmd` would add to the lines the formatters print.  The shape of mcx_sam.hip:
//   k_md<false>  one wavefront per line (a read's own record, then the -m extras): the exact bytes of its string
//   (scan)       exclusive 64-bit sum over the lengths, narrowed to the pool's 32-bit offsets: md_off[lines + 1], the last entry the batch's total
//   k_md<true>   the same walk again, every breaker's bytes stored at their place
// The walk: the lanes take the line's reference columns — the bases of its M, =, X and D operations — 64 at a time.  A lane finds its operation by moving a cursor of
// its own along the few CIGAR words (its columns only ascend), fetches its SEQ byte (reversal and complement applied) and its reference base — the round's 16 or 17
// .pac bytes are loaded by lanes 0-16 and handed round; only behind an N operation does a lane fetch its own — and classifies the column: match, mismatch, first or
// further column of a deletion.  The run ahead of a breaker is its column less the last breaker's, a wave max-scan with the earlier rounds' last breaker carried in a
// register; a mismatch takes digits(run) + 1 bytes, a deletion's first column digits(run) + 2, its further columns 1, and an exclusive wave sum places them behind
// the earlier rounds' bytes.  The final run's digits end the string.  No atomics, no LDS, no loop over a read's bytes in one lane.
// A line's holes (the .amb file's stretches that are not ACGT) are found by one binary search over its reference span; without any the table is never touched.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcx.h"
#include "mcx_md.h"
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

enum { kMdWaves = 4 }; // wavefronts (lines) per workgroup

__device__ inline int wave_max_incl(int v, uint32_t lane)
{
    for (int s = 1; s < 64; s <<= 1) { const int o = __shfl_up(v, s, 64); if (lane >= (uint32_t)s && o > v) v = o; }
    return v;
}
__device__ inline uint32_t wave_sum_incl(uint32_t v, uint32_t lane)
{
    for (int s = 1; s < 64; s <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)v, s, 64); if (lane >= (uint32_t)s) v += o; }
    return v;
}

// one line's string by one wavefront: its bytes (0: no tag), written at dst when kWrite
template <bool kWrite>
__device__ inline uint32_t wave_md(const MdRef &ref, const SamRead &d, const mcx_aln &rec, const uint32_t *cig, uint8_t *dst, uint32_t lane)
{
    if (!md_has(rec)) return 0; // (the whole wavefront: rec is the same in every lane)
    const SamTurn t = sam_turn(d, rec);
    const uint32_t nc = (uint32_t)rec.n_cigar;
    // the line's columns and its reference span, summed over the operations
    uint32_t cols = 0;
    unsigned long long span = 0;
    for (uint32_t k = lane; k < nc; k += 64) {
        const uint32_t takes = md_op_takes(cig[k] & 15u), len = cig[k] >> 4;
        if (takes & 4u) cols += len;
        if (takes & 2u) span += len;
    }
    for (int s = 32; s; s >>= 1) { cols += (uint32_t)__shfl_xor((int)cols, s, 64); span += (unsigned long long)__shfl_xor((long long)span, s, 64); }
    const int64_t g0 = md_g0(ref, rec);
    uint32_t h_lo, h_hi;
    md_holes_of(ref, g0, g0 + (int64_t)span, h_lo, h_hi);
    // the lane's cursor: operation k begins at column c_beg, x_beg reference bases and y_beg read bases into the line
    uint32_t k = 0, c_beg = 0, y_beg = 0;
    int64_t x_beg = 0;
    int last = -1;  // the last breaker's column so far
    uint32_t n = 0; // bytes so far
    for (uint32_t c0 = 0; c0 < cols; c0 += 64) {
        const uint32_t c = c0 + lane;
        const bool valid = c < cols;
        uint32_t op = 0;
        if (valid) {
            while (k < nc) {
                const uint32_t w = cig[k], takes = md_op_takes(w & 15u), len = w >> 4;
                op = w & 15u;
                if ((takes & 4u) && c - c_beg < len) break;
                if (takes & 4u) c_beg += len;
                if (takes & 2u) x_beg += len;
                if (takes & 1u) y_beg += len;
                k++;
            }
        }
        const uint32_t j = c - c_beg;
        const int64_t g = g0 + x_beg + (int64_t)j;
        // the round's .pac bytes: 64 columns lie in 16 or 17 of them from lane 0's on, unless an N operation jumps
        const int64_t b0 = __shfl((long long)(g >> 2), 0, 64);
        uint32_t mine = 0;
        if (lane < 17u) { const int64_t b = b0 + lane; if (b >= 0 && (b << 2) < ref.G) mine = ref.pac[b]; }
        const int64_t at = (g >> 2) - b0;
        const bool near = valid && at >= 0 && at < 17;
        uint32_t byte = (uint32_t)__shfl((int)mine, near ? (int)at : 0, 64);
        const bool inside = valid && g >= 0 && g < ref.G;
        if (inside && !near) byte = ref.pac[g >> 2];
        uint32_t kind = 0; // 0 match, 1 mismatch, 2 a deletion's first column, 3 its further ones
        uint8_t letter = 'N';
        if (valid) {
            letter = md_letter_of(ref, h_lo, h_hi, g, inside ? md_byte_code((uint8_t)byte, g) : 0u);
            if (op == 2u) kind = j == 0 ? 2u : 3u;
            else kind = md_matches(md_seq(d, t, y_beg + j), letter) ? 0u : 1u;
        }
        const int incl = wave_max_incl(kind ? (int)c : -1, lane);
        int prev = __shfl_up(incl, 1, 64);
        if (lane == 0 || prev < last) prev = last;
        const uint32_t run = (uint32_t)((int)c - 1 - prev);
        const uint32_t bytes = kind == 1u ? md_digits(run) + 1 : kind == 2u ? md_digits(run) + 2 : kind == 3u ? 1u : 0u;
        const uint32_t ends = wave_sum_incl(bytes, lane);
        if (kWrite && kind) {
            uint8_t *o = dst + n + (ends - bytes);
            if (kind != 3u) o = md_put_num(o, run);
            if (kind == 2u) *o++ = '^';
            *o = letter;
        }
        n += (uint32_t)__shfl((int)ends, 63, 64);
        const int top = __shfl(incl, 63, 64);
        if (top > last) last = top;
    }
    const uint32_t u = (uint32_t)((int)cols - 1 - last);
    if (kWrite && lane == 0) md_put_num(dst + n, u);
    return n + md_digits(u);
}

template <bool kWrite>
__global__ void __launch_bounds__(64 * kMdWaves) k_md(mcx_sam_in in, MdRef ref, uint32_t n_lines, uint64_t *len, const uint64_t *__restrict__ off, uint8_t *out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t e = blockIdx.x * kMdWaves + (threadIdx.x >> 6);
    if (e > n_lines) return; // (the whole wavefront)
    if (e == n_lines) { if (!kWrite && lane == 0) len[e] = 0; return; } // (one entry more: the scan leaves the total there)
    uint32_t r;
    mcx_aln rec;
    const uint32_t *cig;
    md_line_of(in, e, r, rec, cig);
    const SamRead d = sam_read_of(in, r);
    const uint32_t n = wave_md<kWrite>(ref, d, rec, cig, kWrite ? out + off[e] : nullptr, lane);
    if (!kWrite && lane == 0) len[e] = n;
}

__global__ void __launch_bounds__(256) k_md_narrow(const uint64_t *__restrict__ off, uint32_t entries, uint32_t *md_off)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < entries) md_off[i] = (uint32_t)off[i];
}

MdRef ref_of(const mcx_index *ix)
{
    MdRef ref;
    ref.pac = ix->view.pac; ref.G = ix->view.G; ref.chr_fwd = ix->view.chr_fwd;
    ref.hole_off = (const int64_t *)ix->d_hole_off; ref.hole_len = (const int32_t *)ix->d_hole_len; ref.hole_letter = (const uint8_t *)ix->d_hole_letter;
    ref.n_holes = ix->d_hole_off ? (uint32_t)ix->host.hole_off.size() : 0u;
    return ref;
}

// in: the struct in host memory, its pointers the device's; names, name_off and qual are not read (sam_read_of only computes their addresses)
int md_dev(mcx_ctx *c, SamState *st, const mcx_sam_in &in_, uint32_t n_extras, uint8_t *d_md, uint64_t cap, uint32_t *d_md_off, uint64_t *n_bytes)
{
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    mcx_sam_in in = in_;
    if (!in.names || !in.name_off) { in.names = in.bases; in.name_off = in.off; } // (never dereferenced: see above)
    in.md = nullptr; in.md_off = nullptr;
    const uint64_t n = (uint64_t)in.n_reads + n_extras;
    if (n + 1 > 0xffffffffull) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_md: more than 2^32 lines in one batch");
    if (int rc = sam_scan_room(st, n + 1, s)) return rc;
    const MdRef ref = ref_of(mcx_ctx_index(c));
    const unsigned grid = (unsigned)((n + 1 + kMdWaves - 1) / kMdWaves);
    HIP_TRY(hipEventRecord(st->ev[0], s));
    k_md<false><<<grid, 64 * kMdWaves, 0, s>>>(in, ref, (uint32_t)n, st->d_len, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st->ev[1], s));
    size_t tmp = st->tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(st->d_tmp, tmp, st->d_len, st->d_off, (int)(n + 1), s));
    if (d_md_off) {
        k_md_narrow<<<(unsigned)((n + 1 + 255) / 256), 256, 0, s>>>(st->d_off, (uint32_t)(n + 1), d_md_off);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(st->ev[2], s));
    HIP_TRY(hipMemcpyAsync(st->h_total, st->d_off + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t total = *st->h_total;
    if (n_bytes) *n_bytes = total;
    HIP_TRY(hipEventElapsedTime(&st->md_ms[0], st->ev[0], st->ev[1]));
    HIP_TRY(hipEventElapsedTime(&st->md_ms[1], st->ev[1], st->ev[2]));
    st->md_ms[2] = 0;
    if (total > 0xffffffffull) return mcx_set_error(MCX_ERR_UNSUPPORTED, "the batch's MD strings take " + std::to_string(total) + " bytes: more than the pool's 32-bit offsets say; map with a smaller -batch");
    if (total > cap || (total && !d_md)) return mcx_set_error(MCX_ERR_CAPACITY, "the batch's MD strings take " + std::to_string(total) + " bytes: more than the buffer holds");
    HIP_TRY(hipEventRecord(st->ev[2], s));
    k_md<true><<<grid, 64 * kMdWaves, 0, s>>>(in, ref, (uint32_t)n, nullptr, st->d_off, d_md);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st->ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&st->md_ms[2], st->ev[2], st->ev[3]));
    return 0;
}

bool in_ok(const mcx_sam_in *in)
{
    return in && in->bases && in->off && in->aln && in->cigar && (!in->x_index || (in->x_recs && in->x_cigar));
}

} // namespace

extern "C" int mcx_md_dev(mcx_ctx *c, const mcx_sam_in *d_in, uint8_t *d_md, uint64_t cap, uint32_t *d_md_off, uint64_t *n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    if (!c || !d_in) return mcx_set_error(MCX_ERR_ARG, "mcx_md_dev: null argument");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    if (d_in->n_reads == 0) { // no lines: the offsets' one entry
        if (d_md_off) { HIP_TRY(hipMemsetAsync(d_md_off, 0, 4, s)); HIP_TRY(hipStreamSynchronize(s)); }
        return 0;
    }
    if (!in_ok(d_in)) return mcx_set_error(MCX_ERR_ARG, "mcx_md_dev: null argument");
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    uint32_t n_extras = 0;
    if (d_in->x_index) { // how many extras there are is the index's last entry
        HIP_TRY(hipMemcpyAsync(st->h_total, d_in->x_index + d_in->n_reads, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        n_extras = *(const uint32_t *)st->h_total;
    }
    return md_dev(c, st, *d_in, n_extras, d_md, cap, d_md_off, n_bytes);
}

// mcx_sam.hip's sam_part with -md: the strings of the part's lines into the state's own pool, which in->md / in->md_off then point at (n_extras: the context's
// extras of the part, as mcx_multi_lines counts them); the context's device is current
int mcx_md_part_dev(mcx_ctx *c, mcx_sam_in *in, uint32_t n_extras, uint64_t *n_bytes)
{
    *n_bytes = 0;
    SamState *st;
    int rc;
    if ((rc = sam_state_of(c, &st))) return rc;
    if ((rc = sam_grow(&st->d_md_off, &st->cap_md_off, (uint64_t)in->n_reads + n_extras + 1, "the lines' MD offsets"))) return rc;
    rc = md_dev(c, st, *in, n_extras, st->d_md, st->cap_md, st->d_md_off, n_bytes);
    if (rc == MCX_ERR_CAPACITY) {
        if ((rc = sam_grow(&st->d_md, &st->cap_md, *n_bytes + 16, "the lines' MD strings"))) return rc;
        rc = md_dev(c, st, *in, n_extras, st->d_md, st->cap_md, st->d_md_off, n_bytes);
    }
    if (rc) return rc;
    if (!st->d_md && (rc = sam_grow(&st->d_md, &st->cap_md, 16, "the lines' MD strings"))) return rc; // (a part without a mapped line: a pool all the same)
    in->md = st->d_md; in->md_off = st->d_md_off;
    return 0;
}

void mcx_md_set(mcx_ctx *c, int on)
{
    SamState *st;
    if (sam_state_of(c, &st) == 0) st->want_md = on != 0;
}
bool mcx_md_wanted(mcx_ctx *c)
{
    SamState *st;
    return sam_state_of(c, &st) == 0 && st->want_md;
}

// the host formatter's -md: the strings of a part that still lies in its slot, to host memory with their offsets
int mcx_md_part_host(mcx_ctx *c, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired, const mcx_aln *d_aln, const uint32_t *d_cigar,
                     std::vector<uint8_t> *md, std::vector<uint32_t> *md_off)
{
    md->clear(); md_off->assign(1, 0);
    if (n_reads == 0) return 0;
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    mcx_sam_in in;
    memset(&in, 0, sizeof in);
    in.bases = d_bases; in.off = d_off; in.aln = d_aln; in.cigar = d_cigar; in.n_reads = n_reads; in.paired = paired;
    uint32_t n_recs = 0, n_words = 0;
    int rc;
    if (mcx_ctx_multi(c) && (rc = mcx_multi_lines(c, &in.x_index, &in.x_recs, &in.x_cigar, &n_recs, &n_words))) return rc;
    if (!in.x_index) n_recs = 0;
    uint64_t total = 0;
    if ((rc = mcx_md_part_dev(c, &in, n_recs, &total))) return rc;
    md->resize(total); md_off->resize((size_t)n_reads + n_recs + 1);
    if (total) HIP_TRY(hipMemcpy(md->data(), in.md, total, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(md_off->data(), in.md_off, md_off->size() * 4, hipMemcpyDeviceToHost));
    return 0;
}

// the last call's device times in ms: length kernel, scan, write kernel (scripts/md_rate.py)
extern "C" int mcx_md_last_ms(mcx_ctx *c, float ms[3])
{
    SamState *st;
    if (!c || !ms) return mcx_set_error(MCX_ERR_ARG, "mcx_md_last_ms: null argument");
    if (int rc = sam_state_of(c, &st)) return rc;
    memcpy(ms, st->md_ms, sizeof st->md_ms);
    return 0;
}

extern "C" int mcx_md(mcx_ctx *c, const mcx_sam_in *in, uint8_t *md, uint64_t cap, uint32_t *md_off, uint64_t *n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    if (!c || !in) return mcx_set_error(MCX_ERR_ARG, "mcx_md: null argument");
    const uint64_t n = in->n_reads;
    if (n == 0) { if (md_off) md_off[0] = 0; return 0; }
    if (!in_ok(in)) return mcx_set_error(MCX_ERR_ARG, "mcx_md: null argument");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    // the words of the pools the records point into
    uint64_t words = 0, x_words = 0;
    for (uint64_t r = 0; r < n; r++) words = std::max<uint64_t>(words, (uint64_t)(uint32_t)in->aln[r].cigar_off + (uint64_t)std::max(in->aln[r].n_cigar, 0));
    const uint64_t n_x = in->x_index ? in->x_index[n] : 0;
    for (uint64_t i = 0; i < n_x; i++) x_words = std::max<uint64_t>(x_words, (uint64_t)(uint32_t)in->x_recs[i].cigar_off + (uint64_t)std::max(in->x_recs[i].n_cigar, 0));
    struct Piece { const void *src; uint64_t bytes; void **dst; };
    mcx_sam_in d = *in;
    d.qual = nullptr; d.names = nullptr; d.name_off = nullptr;
    uint32_t *d_off32 = nullptr; uint8_t *d_md = nullptr;
    const Piece pieces[] = {
        {in->bases, in->off[n], (void **)&d.bases}, {in->off, (n + 1) * 4, (void **)&d.off},
        {in->aln, n * sizeof(mcx_aln), (void **)&d.aln}, {in->cigar, words * 4, (void **)&d.cigar},
        {in->x_index, in->x_index ? (n + 1) * 4 : 0, (void **)&d.x_index}, {in->x_recs, n_x * sizeof(mcx_aln), (void **)&d.x_recs}, {in->x_cigar, x_words * 4, (void **)&d.x_cigar},
    };
    uint64_t all = 0;
    for (const Piece &p : pieces) all += (p.bytes + 15) / 16 * 16 + 16;
    uint8_t *d_all = nullptr;
    if (hipMalloc((void **)&d_all, all) != hipSuccess) { (void)hipGetLastError(); return mcx_set_error(MCX_ERR_DEVICE, "mcx_md: no room in HBM for the batch"); }
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    int rc = 0;
    uint64_t at = 0;
    for (const Piece &p : pieces) {
        *p.dst = p.src ? (void *)(d_all + at) : nullptr;
        if (p.src && p.bytes && hipMemcpyAsync(d_all + at, p.src, p.bytes, hipMemcpyHostToDevice, s) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_md: copy to the device failed");
        at += (p.bytes + 15) / 16 * 16 + 16;
    }
    if (rc == 0 && md_off && hipMalloc((void **)&d_off32, (n + n_x + 1) * 4) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_md: no room in HBM for the strings' offsets");
    if (rc == 0 && cap && md && hipMalloc((void **)&d_md, cap) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_md: no room in HBM for the strings");
    uint64_t total = 0;
    if (rc == 0) rc = md_dev(c, st, d, (uint32_t)n_x, d_md, d_md ? cap : 0, d_off32, &total);
    if (n_bytes) *n_bytes = total;
    if (rc == 0 && total && hipMemcpy(md, d_md, total, hipMemcpyDeviceToHost) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_md: copy from the device failed");
    if ((rc == 0 || rc == MCX_ERR_CAPACITY) && md_off && hipMemcpy(md_off, d_off32, (n + n_x + 1) * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_md: copy from the device failed");
    (void)hipStreamSynchronize(s);
    (void)hipFree(d_all); (void)hipFree(d_off32); (void)hipFree(d_md);
    return rc;
}
