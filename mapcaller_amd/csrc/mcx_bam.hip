// mapcaller_amd/csrc/mcx_bam.hip — a mapped batch's BAM records made in HBM (mcx_bam_format_dev, mcx_bam_format, mcx_bam_header; the file front end's -bam).
//
// Replaces, for a whole batch, the reference's detour through text for -bam (sam_parse1 + sam_write1 on every SAM line, src/ReadMapping.cpp:548-606); the bytes
// are mcx_bam.h's.  The shape of mcx_sam.hip:
//   k_bam_len    one lane per read: the exact bytes of its record(s), and how many of its lines make none (counted into one word)
//   (scan)       exclusive 64-bit sum over the lengths: rec_off[n_reads + 1], the last entry the batch's total
//   k_bam_write  one wavefront per read: the lanes stream QNAME and the CIGAR words' bytes, lane k packs byte k of SEQ from bases 2k and 2k + 1 (complement and
//                reversal applied on the way), QUAL loses its 33 on the way, lane 0 writes the 36 fixed bytes and the tags; the record is staged in LDS at the same
//                offset within 16 bytes as its place in the stream, and leaves in aligned 16-byte stores with byte stores for its unaligned head and tail.  A
//                record that does not fit the staging (CIGARs of hundreds of operations, reads near a thousand bases) is written by the same lanes byte by byte
//                straight to its place: records are not aligned in the stream, so nothing wider than a byte is ever stored to an unaligned place.
// What leaves here is the uncompressed stream; mcx_bgzf_deflate_dev (mcx_deflate.hip) frames it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcx.h"
#include "mcx_bam.h"
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

enum { kBamWaves = 4, kBamStage = 2048 }; // wavefronts (reads) per workgroup; bytes of LDS a wavefront stages a record in

__global__ void __launch_bounds__(256) k_bam_len(mcx_sam_in in, uint64_t *len, unsigned long long *n_dropped)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > in.n_reads) return;
    uint32_t none = 0;
    len[r] = r < in.n_reads ? bam_rec_len(in, r, &none) : 0; // (one entry more: the scan leaves the total there)
    if (none) atomicAdd(n_dropped, (unsigned long long)none);  // (rare: a name of 252 bytes, a cut quality line)
}

// what one lane stored to LDS is read by the others of its wavefront (no other wavefront shares the staging)
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one record by one wavefront; returns its bytes (0: the line makes none)
__device__ inline uint32_t wave_record(const SamRead &d, const mcx_aln &rec, const uint32_t *cig, uint8_t *stage, uint8_t *dst, uint32_t lane, const uint8_t *md, uint32_t ml)
{
    const SamTurn t = sam_turn(d, rec);
    uint32_t ql = 1; // '*'
    if (d.qual) {    // the first NUL in printing order ends QUAL
        ql = d.rlen;
        for (uint32_t k = lane; k < d.rlen; k += 64) if (sam_qual_byte(d, t, k) == 0) { ql = k; break; }
        for (int s = 32; s; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)ql, s, 64); ql = o < ql ? o : ql; }
    }
    if (!bam_keep_ql(d, t, ql)) return 0; // (the whole wavefront: d, rec and ql are the same in every lane)
    const bool star = bam_qual_star(d, t, ql);
    const BamLayout l = bam_layout(d, rec, ml);
    const uint32_t L = l.total;
    const uint32_t sh = (uint32_t)((uintptr_t)dst & 15u);
    const bool staged = sh + L <= (uint32_t)kBamStage;
    uint8_t *o = staged ? stage + sh : dst; // (the staging is 16-byte aligned: o and dst sit alike within their 16 bytes; a record too long for it goes straight to its place)
    if (lane == 0) { bam_fixed_put(d, rec, cig, L, o); o[kBamFixed + d.name_len] = 0; bam_tags_put(rec, o + l.tags_at); }
    if (ml) { // the MD tag behind XS: its string is the pool's
        const uint32_t md_at = L - bam_md_len(ml);
        if (lane == 0) { o[md_at] = 'M'; o[md_at + 1] = 'D'; o[md_at + 2] = 'Z'; o[L - 1] = 0; }
        for (uint32_t k = lane; k < ml; k += 64) o[md_at + 3 + k] = md[k];
    }
    for (uint32_t k = lane; k < d.name_len; k += 64) o[kBamFixed + k] = d.name[k];
    for (uint32_t k = l.cigar_at + lane; k < l.seq_at; k += 64) o[k] = bam_cigar_byte(cig, k - l.cigar_at);
    for (uint32_t k = l.seq_at + lane; k < l.qual_at; k += 64) o[k] = bam_seq_out(d, t, k - l.seq_at);
    for (uint32_t k = lane; k < d.rlen; k += 64) o[l.qual_at + k] = bam_qual_out(d, t, star, k);
    if (!staged) return L;
    wave_sync();
    const uint32_t head = ((16u - sh) & 15u) < L ? ((16u - sh) & 15u) : L, n16 = (L - head) >> 4, tail_at = head + (n16 << 4);
    if (lane < head) dst[lane] = o[lane];
    const uint4 *s16 = (const uint4 *)(o + head);
    uint4 *d16 = (uint4 *)(dst + head);
    for (uint32_t i = lane; i < n16; i += 64) d16[i] = s16[i];
    if (tail_at + lane < L) dst[tail_at + lane] = o[tail_at + lane];
    wave_sync(); // (the next record is staged in the same bytes)
    return L;
}

__global__ void __launch_bounds__(64 * kBamWaves) k_bam_write(mcx_sam_in in, const uint64_t *__restrict__ rec_off, uint8_t *out)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kBamWaves][kBamStage];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * kBamWaves + w;
    if (r >= in.n_reads) return; // (the whole wavefront; nothing below waits for another one)
    const SamRead d = sam_read_of(in, r);
    uint8_t *dst = out + rec_off[r];
    const mcx_aln rec = in.aln[r];
    const uint8_t *md;
    uint32_t ml = sam_md_of(in, r, md);
    dst += wave_record(d, rec, in.cigar + (uint32_t)rec.cigar_off, stage[w], dst, lane, md, ml);
    uint32_t lo, hi;
    sam_extras_of(in, r, lo, hi);
    for (uint32_t i = lo; i < hi; i++) {
        const mcx_aln x = in.x_recs[i];
        ml = sam_md_of(in, in.n_reads + i, md);
        dst += wave_record(d, x, in.x_cigar + (uint32_t)x.cigar_off, stage[w], dst, lane, md, ml);
    }
}

// in: the struct in host memory, its pointers the device's
int format_dev(mcx_ctx *c, SamState *st, const mcx_sam_in &in, uint8_t *d_out, uint64_t cap, uint64_t *d_rec_off, uint64_t *n_bytes, uint64_t *n_dropped)
{
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    const uint64_t n = in.n_reads;
    if (int rc = sam_scan_room(st, n + 1, s)) return rc;
    uint64_t *off = d_rec_off ? d_rec_off : st->d_off;
    HIP_TRY(hipMemsetAsync(st->d_dropped, 0, 8, s));
    HIP_TRY(hipEventRecord(st->ev[0], s));
    k_bam_len<<<(unsigned)((n + 1 + 255) / 256), 256, 0, s>>>(in, st->d_len, st->d_dropped);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st->ev[1], s));
    size_t tmp = st->tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(st->d_tmp, tmp, st->d_len, off, (int)(n + 1), s));
    HIP_TRY(hipEventRecord(st->ev[2], s));
    HIP_TRY(hipMemcpyAsync(st->h_total, off + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(st->h_total + 1, st->d_dropped, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t total = st->h_total[0];
    if (n_bytes) *n_bytes = total;
    if (n_dropped) *n_dropped = st->h_total[1];
    HIP_TRY(hipEventElapsedTime(&st->ms[0], st->ev[0], st->ev[1]));
    HIP_TRY(hipEventElapsedTime(&st->ms[1], st->ev[1], st->ev[2]));
    st->ms[2] = 0;
    if (total > cap || (total && !d_out)) return mcx_set_error(MCX_ERR_CAPACITY, "the batch's BAM records take " + std::to_string(total) + " bytes: more than the buffer holds");
    HIP_TRY(hipEventRecord(st->ev[2], s));
    k_bam_write<<<(unsigned)((n + kBamWaves - 1) / kBamWaves), 64 * kBamWaves, 0, s>>>(in, off, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st->ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&st->ms[2], st->ev[2], st->ev[3]));
    return 0;
}

bool in_ok(const mcx_sam_in *in)
{
    return in && in->bases && in->off && in->names && in->name_off && in->aln && in->cigar && (!in->x_index || (in->x_recs && in->x_cigar));
}

} // namespace

extern "C" int mcx_bam_format_dev(mcx_ctx *c, const mcx_sam_in *d_in, uint8_t *d_out, uint64_t cap, uint64_t *d_rec_off, uint64_t *n_bytes, uint64_t *n_dropped)
{
    if (n_bytes) *n_bytes = 0;
    if (n_dropped) *n_dropped = 0;
    if (!c || !d_in) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_format_dev: null argument");
    if (d_in->n_reads == 0) return 0;
    if (!in_ok(d_in)) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_format_dev: null argument");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    return format_dev(c, st, *d_in, d_out, cap, d_rec_off, n_bytes, n_dropped);
}

// mcx_sam.hip's sam_part with -bam: the same call for the front end's own input (with -m on and no extra line in the part, the extras' pools may be null)
int mcx_bam_part_dev(mcx_ctx *c, const mcx_sam_in *d_in, uint8_t *d_out, uint64_t cap, uint64_t *n_bytes, uint64_t *n_dropped)
{
    *n_bytes = *n_dropped = 0;
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    return format_dev(c, st, *d_in, d_out, cap, nullptr, n_bytes, n_dropped);
}

// the last call's device times in ms: length kernel, scan, write kernel (scripts/bam_rate.py)
extern "C" int mcx_bam_last_ms(mcx_ctx *c, float ms[3])
{
    SamState *st;
    if (!c || !ms) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_last_ms: null argument");
    if (int rc = sam_state_of(c, &st)) return rc;
    memcpy(ms, st->ms, sizeof st->ms);
    return 0;
}

extern "C" int mcx_bam_format(mcx_ctx *c, const mcx_sam_in *in, uint8_t *out, uint64_t cap, uint64_t *rec_off, uint64_t *n_bytes, uint64_t *n_dropped)
{
    if (n_bytes) *n_bytes = 0;
    if (n_dropped) *n_dropped = 0;
    if (!c || !in) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_format: null argument");
    const uint64_t n = in->n_reads;
    if (n == 0) return 0;
    if (!in_ok(in)) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_format: null argument");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    // the words of the pools the records point into
    uint64_t words = 0, x_words = 0;
    for (uint64_t r = 0; r < n; r++) words = std::max<uint64_t>(words, (uint64_t)(uint32_t)in->aln[r].cigar_off + (uint64_t)std::max(in->aln[r].n_cigar, 0));
    const uint64_t n_x = in->x_index ? in->x_index[n] : 0;
    for (uint64_t i = 0; i < n_x; i++) x_words = std::max<uint64_t>(x_words, (uint64_t)(uint32_t)in->x_recs[i].cigar_off + (uint64_t)std::max(in->x_recs[i].n_cigar, 0));
    struct Piece { const void *src; uint64_t bytes; void **dst; };
    const bool with_md = in->md && in->md_off; // the lines' MD strings: one entry per read and per extra, and the total
    mcx_sam_in d = *in;
    uint64_t *d_off64 = nullptr; uint8_t *d_out = nullptr;
    const Piece pieces[] = {
        {in->bases, in->off[n], (void **)&d.bases}, {in->off, (n + 1) * 4, (void **)&d.off}, {in->qual, in->qual ? in->off[n] : 0, (void **)&d.qual},
        {in->names, in->name_off[n], (void **)&d.names}, {in->name_off, (n + 1) * 4, (void **)&d.name_off},
        {in->aln, n * sizeof(mcx_aln), (void **)&d.aln}, {in->cigar, words * 4, (void **)&d.cigar},
        {in->x_index, in->x_index ? (n + 1) * 4 : 0, (void **)&d.x_index}, {in->x_recs, n_x * sizeof(mcx_aln), (void **)&d.x_recs}, {in->x_cigar, x_words * 4, (void **)&d.x_cigar},
        {with_md ? in->md : nullptr, with_md ? in->md_off[n + n_x] : 0, (void **)&d.md}, {with_md ? in->md_off : nullptr, with_md ? (n + n_x + 1) * 4 : 0, (void **)&d.md_off},
    };
    uint64_t all = 0;
    for (const Piece &p : pieces) all += (p.bytes + 15) / 16 * 16 + 16;
    uint8_t *d_all = nullptr;
    if (hipMalloc((void **)&d_all, all) != hipSuccess) { (void)hipGetLastError(); return mcx_set_error(MCX_ERR_DEVICE, "mcx_bam_format: no room in HBM for the batch"); }
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    int rc = 0;
    uint64_t at = 0;
    for (const Piece &p : pieces) {
        *p.dst = p.src ? (void *)(d_all + at) : nullptr;
        if (p.src && p.bytes && hipMemcpyAsync(d_all + at, p.src, p.bytes, hipMemcpyHostToDevice, s) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_bam_format: copy to the device failed");
        at += (p.bytes + 15) / 16 * 16 + 16;
    }
    if (rc == 0 && rec_off && hipMalloc((void **)&d_off64, (n + 1) * 8) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_bam_format: no room in HBM for the records' offsets");
    if (rc == 0 && cap && out && hipMalloc((void **)&d_out, cap) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_bam_format: no room in HBM for the records");
    uint64_t total = 0;
    if (rc == 0) rc = format_dev(c, st, d, d_out, d_out ? cap : 0, d_off64, &total, n_dropped);
    if (n_bytes) *n_bytes = total;
    if (rc == 0 && total && hipMemcpy(out, d_out, total, hipMemcpyDeviceToHost) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_bam_format: copy from the device failed");
    if ((rc == 0 || rc == MCX_ERR_CAPACITY) && rec_off && hipMemcpy(rec_off, d_off64, (n + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_bam_format: copy from the device failed");
    (void)hipStreamSynchronize(s);
    (void)hipFree(d_all); (void)hipFree(d_off64); (void)hipFree(d_out);
    return rc;
}

extern "C" int mcx_bam_header(const mcx_index *ix, uint8_t *out, uint64_t cap, uint64_t *n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    if (!ix) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_header: null argument");
    const HostIndex &hx = ix->host;
    std::string text, h("BAM\1", 4);
    sam_header(hx, text);
    auto le32 = [&h](uint32_t v) { for (int k = 0; k < 4; k++) h += (char)(v >> (8 * k)); };
    le32((uint32_t)text.size());
    h += text;
    le32((uint32_t)hx.chr_name.size());
    for (size_t i = 0; i < hx.chr_name.size(); i++) {
        if ((int64_t)hx.chr_len[i] < 0 || (int64_t)hx.chr_len[i] > 0x7fffffffll) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_bam_header: contig " + hx.chr_name[i] + " is longer than 2^31 - 1 bases, which BAM cannot say");
        le32((uint32_t)hx.chr_name[i].size() + 1);
        h += hx.chr_name[i];
        h += '\0';
        le32((uint32_t)hx.chr_len[i]);
    }
    if (n_bytes) *n_bytes = h.size();
    if (h.size() > cap || !out) return mcx_set_error(MCX_ERR_CAPACITY, "the BAM header takes " + std::to_string(h.size()) + " bytes: more than the buffer holds");
    memcpy(out, h.data(), h.size());
    return 0;
}
