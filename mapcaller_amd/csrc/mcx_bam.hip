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
//                straight to its place: records are not aligned in the stream, so nothing wider than a byte is ever stored to an unaligned place.  The tags
//                behind XS (mcx_sam.h's SamTail: MD, MC and MQ, RG) are counted into the record before that choice; lane 0 writes the mate's CIGAR as text, the
//                lanes spread the MD string and the read group's ID.  With the tags off a kernel reads nothing it did not read before.
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
#include "mcx_tags.h"

using namespace mcx;

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace {

enum { kBamWaves = 4, kBamStage = 2048 }; // wavefronts (reads) per workgroup; bytes of LDS a wavefront stages a record in

// kTags false: the kernel of before — the tags' branches are folded away at compile time, not taken at run time (scripts/tags_rate.py measured the difference)
template <bool kTags> __global__ void __launch_bounds__(256) k_bam_len(mcx_sam_in in, mcx_sam_tags tg_in, uint64_t *len, unsigned long long *n_dropped)
{
    const mcx_sam_tags tg = kTags ? tg_in : mcx_sam_tags();
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > in.n_reads) return;
    uint32_t none = 0;
    len[r] = r < in.n_reads ? bam_rec_len(in, r, &none, tg) : 0; // (one entry more: the scan leaves the total there)
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
__device__ inline uint32_t wave_record(const SamRead &d, const mcx_aln &rec, const uint32_t *cig, uint8_t *stage, uint8_t *dst, uint32_t lane, const SamTail &tail)
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
    const BamLayout l = bam_layout(d, rec, tail);
    const uint32_t L = l.total;
    const uint32_t sh = (uint32_t)((uintptr_t)dst & 15u);
    const bool staged = sh + L <= (uint32_t)kBamStage;
    uint8_t *o = staged ? stage + sh : dst; // (the staging is 16-byte aligned: o and dst sit alike within their 16 bytes; a record too long for it goes straight to its place)
    if (lane == 0) { bam_fixed_put(d, rec, cig, L, o); o[kBamFixed + d.name_len] = 0; bam_tags_put(rec, o + l.tags_at); }
    const uint32_t ml = tail.md_len, gl = tail.rg_len;
    const uint32_t md_at = L - bam_tail_len(tail), mc_at = md_at + bam_md_len(ml), rg_at = mc_at + bam_mc_len(tail); // the tags behind XS
    if (ml) { // the MD string is the pool's
        if (lane == 0) { o[md_at] = 'M'; o[md_at + 1] = 'D'; o[md_at + 2] = 'Z'; o[mc_at - 1] = 0; }
        for (uint32_t k = lane; k < ml; k += 64) o[md_at + 3 + k] = tail.md[k];
    }
    if (tail.mc_n && lane == 0) bam_mc_put(o + mc_at, tail); // the mate's CIGAR through column 6's code, and its MAPQ
    if (gl) {
        if (lane == 0) { o[rg_at] = 'R'; o[rg_at + 1] = 'G'; o[rg_at + 2] = 'Z'; o[L - 1] = 0; }
        for (uint32_t k = lane; k < gl; k += 64) o[rg_at + 3 + k] = tail.rg[k];
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

template <bool kTags> __global__ void __launch_bounds__(64 * kBamWaves) k_bam_write(mcx_sam_in in, mcx_sam_tags tg_in, const uint64_t *__restrict__ rec_off, uint8_t *out)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kBamWaves][kBamStage];
    const mcx_sam_tags tg = kTags ? tg_in : mcx_sam_tags();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * kBamWaves + w;
    if (r >= in.n_reads) return; // (the whole wavefront; nothing below waits for another one)
    const SamRead d = sam_read_of(in, r);
    uint8_t *dst = out + rec_off[r];
    const mcx_aln rec = in.aln[r];
    dst += wave_record(d, rec, in.cigar + (uint32_t)rec.cigar_off, stage[w], dst, lane, sam_tail_of(in, tg, r, r, rec, false));
    uint32_t lo, hi;
    sam_extras_of(in, r, lo, hi);
    for (uint32_t i = lo; i < hi; i++) {
        const mcx_aln x = in.x_recs[i];
        dst += wave_record(d, x, in.x_cigar + (uint32_t)x.cigar_off, stage[w], dst, lane, sam_tail_of(in, tg, in.n_reads + i, r, x, true));
    }
}

// in: the struct in host memory, its pointers the device's
int format_dev(mcx_ctx *c, SamState *st, const mcx_sam_in &in, const mcx_sam_tags &tg, uint8_t *d_out, uint64_t cap, uint64_t *d_rec_off, uint64_t *n_bytes, uint64_t *n_dropped)
{
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    const uint64_t n = in.n_reads;
    if (int rc = sam_scan_room(st, n + 1, s)) return rc;
    uint64_t *off = d_rec_off ? d_rec_off : st->d_off;
    HIP_TRY(hipMemsetAsync(st->d_dropped, 0, 8, s));
    HIP_TRY(hipEventRecord(st->ev[0], s));
    const bool tags = tg.mate_tags || (tg.rg && tg.rg_len);
    (tags ? k_bam_len<true> : k_bam_len<false>)<<<(unsigned)((n + 1 + 255) / 256), 256, 0, s>>>(in, tg, st->d_len, st->d_dropped);
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
    (tags ? k_bam_write<true> : k_bam_write<false>)<<<(unsigned)((n + kBamWaves - 1) / kBamWaves), 64 * kBamWaves, 0, s>>>(in, tg, off, d_out);
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
    return mcx_bam_format_tags_dev(c, d_in, nullptr, d_out, cap, d_rec_off, n_bytes, n_dropped);
}
extern "C" int mcx_bam_format_tags_dev(mcx_ctx *c, const mcx_sam_in *d_in, const mcx_sam_tags *tags, uint8_t *d_out, uint64_t cap, uint64_t *d_rec_off, uint64_t *n_bytes, uint64_t *n_dropped)
{
    if (n_bytes) *n_bytes = 0;
    if (n_dropped) *n_dropped = 0;
    if (!c || !d_in) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_format_dev: null argument");
    if (!tags_ok(d_in, tags)) return mcx_set_error(MCX_ERR_UNSUPPORTED, std::string("mcx_bam_format_dev") + kTagsWithExtras);
    if (d_in->n_reads == 0) return 0;
    if (!in_ok(d_in)) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_format_dev: null argument");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    return format_dev(c, st, *d_in, tags ? *tags : mcx_sam_tags(), d_out, cap, d_rec_off, n_bytes, n_dropped);
}

// mcx_sam.hip's sam_part with -bam: the same call for the front end's own input (with -m on and no extra line in the part, the extras' pools may be null)
int mcx_bam_part_dev(mcx_ctx *c, const mcx_sam_in *d_in, const mcx_sam_tags *tags, uint8_t *d_out, uint64_t cap, uint64_t *n_bytes, uint64_t *n_dropped)
{
    *n_bytes = *n_dropped = 0;
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    return format_dev(c, st, *d_in, *tags, d_out, cap, nullptr, n_bytes, n_dropped);
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
    return mcx_bam_format_tags(c, in, nullptr, out, cap, rec_off, n_bytes, n_dropped);
}
extern "C" int mcx_bam_format_tags(mcx_ctx *c, const mcx_sam_in *in, const mcx_sam_tags *tags, uint8_t *out, uint64_t cap, uint64_t *rec_off, uint64_t *n_bytes, uint64_t *n_dropped)
{
    if (n_bytes) *n_bytes = 0;
    if (n_dropped) *n_dropped = 0;
    if (!c || !in) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_format: null argument");
    if (!tags_ok(in, tags)) return mcx_set_error(MCX_ERR_UNSUPPORTED, std::string("mcx_bam_format") + kTagsWithExtras);
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
    mcx_sam_tags tg = tags ? *tags : mcx_sam_tags();
    if (!tg.rg || !tg.rg_len) { tg.rg = nullptr; tg.rg_len = 0; }
    uint64_t *d_off64 = nullptr; uint8_t *d_out = nullptr;
    const Piece pieces[] = {
        {in->bases, in->off[n], (void **)&d.bases}, {in->off, (n + 1) * 4, (void **)&d.off}, {in->qual, in->qual ? in->off[n] : 0, (void **)&d.qual},
        {in->names, in->name_off[n], (void **)&d.names}, {in->name_off, (n + 1) * 4, (void **)&d.name_off},
        {in->aln, n * sizeof(mcx_aln), (void **)&d.aln}, {in->cigar, words * 4, (void **)&d.cigar},
        {in->x_index, in->x_index ? (n + 1) * 4 : 0, (void **)&d.x_index}, {in->x_recs, n_x * sizeof(mcx_aln), (void **)&d.x_recs}, {in->x_cigar, x_words * 4, (void **)&d.x_cigar},
        {with_md ? in->md : nullptr, with_md ? in->md_off[n + n_x] : 0, (void **)&d.md}, {with_md ? in->md_off : nullptr, with_md ? (n + n_x + 1) * 4 : 0, (void **)&d.md_off},
        {tg.rg, tg.rg_len, (void **)&tg.rg}, // the read group's ID
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
    if (rc == 0) rc = format_dev(c, st, d, tg, d_out, d_out ? cap : 0, d_off64, &total, n_dropped);
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

// a header's bytes with the read-group line as the last line of its text
static int rg_line_ok(const char *rg_line, const char *who)
{
    std::string line, id, why;
    if (!mcx::rg_parse(rg_line, line, id, why)) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": " + why);
    if (line != rg_line) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": the read-group line must hold real TABs (mcx_rg_parse's line)");
    return 0;
}
extern "C" int mcx_sam_header_rg(const mcx_index *ix, const char *rg_line, char *out, uint64_t cap, uint64_t *n_bytes)
{
    if (!rg_line) return mcx_sam_header(ix, out, cap, n_bytes);
    if (n_bytes) *n_bytes = 0;
    if (!ix) return mcx_set_error(MCX_ERR_ARG, "mcx_sam_header_rg: null argument");
    if (int rc = rg_line_ok(rg_line, "mcx_sam_header_rg")) return rc;
    std::string h;
    sam_header(ix->host, h);
    h += rg_line; h += '\n';
    if (n_bytes) *n_bytes = h.size();
    if (h.size() > cap || !out) return mcx_set_error(MCX_ERR_CAPACITY, "the SAM header takes " + std::to_string(h.size()) + " bytes: more than the buffer holds");
    memcpy(out, h.data(), h.size());
    return 0;
}
extern "C" int mcx_bam_header_rg(const mcx_index *ix, const char *rg_line, int sorted, uint8_t *out, uint64_t cap, uint64_t *n_bytes)
{
    auto base = sorted ? mcx_bam_header_sorted : mcx_bam_header;
    if (!rg_line) return base(ix, out, cap, n_bytes);
    if (n_bytes) *n_bytes = 0;
    if (!ix) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_header_rg: null argument");
    if (int rc = rg_line_ok(rg_line, "mcx_bam_header_rg")) return rc;
    uint64_t n = 0;
    (void)base(ix, nullptr, 0, &n);
    std::string h((size_t)n, '\0');
    if (n < 12) return mcx_set_error(MCX_ERR_UNSUPPORTED, std::string("mcx_bam_header_rg: ") + mcx_last_error());
    if (int rc = base(ix, (uint8_t *)&h[0], n, &n)) return rc;
    // "BAM\1", l_text, the text: the line goes behind the text, l_text grows by it
    uint32_t l_text = 0;
    for (int k = 0; k < 4; k++) l_text |= (uint32_t)(uint8_t)h[4 + k] << (8 * k);
    const std::string line = std::string(rg_line) + "\n";
    h.insert(8 + (size_t)l_text, line);
    l_text += (uint32_t)line.size();
    for (int k = 0; k < 4; k++) h[4 + k] = (char)(l_text >> (8 * k));
    if (n_bytes) *n_bytes = h.size();
    if (h.size() > cap || !out) return mcx_set_error(MCX_ERR_CAPACITY, "the BAM header takes " + std::to_string(h.size()) + " bytes: more than the buffer holds");
    memcpy(out, h.data(), h.size());
    return 0;
}
extern "C" int mcx_rg_parse(const char *arg, char *line, uint64_t cap, uint64_t *line_len, uint32_t *id_at, uint32_t *id_len)
{
    if (line_len) *line_len = 0;
    std::string l, id, why;
    if (!mcx::rg_parse(arg, l, id, why)) return mcx_set_error(MCX_ERR_ARG, "-rg: " + why);
    if (line_len) *line_len = l.size();
    const size_t at = l.find("\tID:") + 4; // (the one ID field; a field begins behind a TAB)
    if (id_at) *id_at = (uint32_t)at;
    if (id_len) *id_len = (uint32_t)id.size();
    if (l.size() > cap || !line) return mcx_set_error(MCX_ERR_CAPACITY, "the read-group line takes " + std::to_string(l.size()) + " bytes: more than the buffer holds");
    memcpy(line, l.data(), l.size());
    return 0;
}
