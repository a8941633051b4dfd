// mapcaller_amd/csrc/mcx_sam.hip — a mapped batch's SAM text made in HBM (mcx_sam_format_dev, mcx_sam_format, mcx_sam_header; the file front end's -gpu_sam).
//
// Replaces Generate{Paired,Single}SamStream (reference src/SamReport.cpp:324-488) for a whole batch; the bytes are mcx_sam.h's.
//   k_sam_len    one lane per read: the exact bytes of its line(s)
//   (scan)       exclusive 64-bit sum over the lengths: line_off[n_reads + 1], the last entry the batch's total
//   k_sam_write  one wavefront per read: every lane streams QNAME, SEQ and QUAL (complement and reversal applied on the way), lane 0
//                assembles the numeric fields and the tags; the line is staged in LDS at the same offset within 16 bytes as its place in
//                the text, and leaves in aligned 16-byte stores with byte stores for its unaligned head and tail.  A line that does not
//                fit the staging (reads of many hundred bases, CIGARs of hundreds of operations) is written by the same lanes byte by byte
//                straight to its place: never cut short.  The tags behind XS (mcx_sam.h's SamTail: MD, MC and MQ, RG) are counted into the line before that
//                choice; lane 0 writes the mate's CIGAR, the lanes spread the MD string and the read group's ID as they spread QNAME.  The mate's record is
//                fetched once per line, and only with mate_tags on: with the tags off a kernel reads nothing it did not read before.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcx.h"
#include "mcx_sam.h"
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

enum { kSamWaves = 4, kSamStage = 2048 }; // wavefronts (reads) per workgroup; bytes of LDS a wavefront stages a line in

// kTags false: the kernel of before — the tags' branches are folded away at compile time, not taken at run time (scripts/tags_rate.py measured the difference)
template <bool kTags> __global__ void __launch_bounds__(256) k_sam_len(mcx_sam_in in, mcx_sam_tags tg_in, SamContigs cn, uint64_t *len)
{
    const mcx_sam_tags tg = kTags ? tg_in : mcx_sam_tags();
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > in.n_reads) return;
    len[r] = r < in.n_reads ? sam_line_len(in, cn, r, tg) : 0; // (one entry more: the scan leaves the total there)
}

// what one lane stored to LDS is read by the others of its wavefront (no other wavefront shares the staging)
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one line by one wavefront; returns its bytes
__device__ inline uint32_t wave_line(const SamRead &d, const mcx_aln &rec, const uint32_t *cig, const SamContigs &cn, uint8_t *stage, uint8_t *dst, uint32_t lane, const SamTail &tail)
{
    const SamTurn t = sam_turn(d, rec);
    uint32_t ql = 1; // '*'
    if (d.qual) {    // the first NUL in printing order ends QUAL
        ql = d.rlen;
        for (uint32_t k = lane; k < d.rlen; k += 64) if (sam_qual_byte(d, t, k) == 0) { ql = k; break; }
        for (int s = 32; s; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)ql, s, 64); ql = o < ql ? o : ql; }
    }
    const uint32_t hl = sam_head_len(rec, cig, cn), tl = sam_tags_len(rec);
    const uint32_t ml = tail.md_len, gl = tail.rg_len, tail_len = sam_tail_len(tail);
    const uint32_t seq_at = d.name_len + hl, q_at = seq_at + d.rlen + 1, md_at = q_at + ql + tl - 1, L = q_at + ql + tl + tail_len; // (md_at: the tags' newline, where the tail begins)
    const uint32_t mc_at = md_at + sam_md_len(ml), rg_at = mc_at + sam_mc_len(tail);
    const uint32_t sh = (uint32_t)((uintptr_t)dst & 15u);
    const bool staged = sh + L <= (uint32_t)kSamStage;
    uint8_t *o = staged ? stage + sh : dst; // (the staging is 16-byte aligned: o and dst sit alike within their 16 bytes; a line too long for it goes straight to its place)
    for (uint32_t k = lane; k < d.name_len; k += 64) o[k] = d.name[k];
    if (lane == 0) {
        sam_head_put(rec, cig, cn, o + d.name_len); o[q_at - 1] = '\t'; sam_tags_put(rec, o + q_at + ql);
        if (tail_len) { // the tail goes over the newline; the MD string is the pool's, MC the mate's CIGAR through column 6's code
            if (ml) sam_md_lit(o + md_at);
            if (tail.mc_n) sam_mc_put(o + mc_at, tail);
            if (gl) sam_rg_lit(o + rg_at);
            o[L - 1] = '\n';
        }
    }
    for (uint32_t k = lane; k < ml; k += 64) o[md_at + 6 + k] = tail.md[k];
    for (uint32_t k = lane; k < gl; k += 64) o[rg_at + 6 + k] = tail.rg[k];
    for (uint32_t k = lane; k < d.rlen; k += 64) o[seq_at + k] = sam_seq_byte(d, t, k);
    for (uint32_t k = lane; k < ql; k += 64) o[q_at + k] = sam_qual_byte(d, t, k);
    if (!staged) return L;
    wave_sync();
    const uint32_t head = ((16u - sh) & 15u) < L ? ((16u - sh) & 15u) : L, n16 = (L - head) >> 4, tail_at = head + (n16 << 4);
    if (lane < head) dst[lane] = o[lane];
    const uint4 *s16 = (const uint4 *)(o + head);
    uint4 *d16 = (uint4 *)(dst + head);
    for (uint32_t i = lane; i < n16; i += 64) d16[i] = s16[i];
    if (tail_at + lane < L) dst[tail_at + lane] = o[tail_at + lane];
    wave_sync(); // (the next line is staged in the same bytes)
    return L;
}

template <bool kTags> __global__ void __launch_bounds__(64 * kSamWaves) k_sam_write(mcx_sam_in in, mcx_sam_tags tg_in, SamContigs cn, const uint64_t *__restrict__ line_off, uint8_t *text)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[kSamWaves][kSamStage];
    const mcx_sam_tags tg = kTags ? tg_in : mcx_sam_tags();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * kSamWaves + w;
    if (r >= in.n_reads) return; // (the whole wavefront; nothing below waits for another one)
    const SamRead d = sam_read_of(in, r);
    uint8_t *dst = text + line_off[r];
    const mcx_aln rec = in.aln[r];
    dst += wave_line(d, rec, in.cigar + (uint32_t)rec.cigar_off, cn, stage[w], dst, lane, sam_tail_of(in, tg, r, r, rec, false));
    uint32_t lo, hi;
    sam_extras_of(in, r, lo, hi);
    for (uint32_t i = lo; i < hi; i++) {
        const mcx_aln x = in.x_recs[i];
        dst += wave_line(d, x, in.x_cigar + (uint32_t)x.cigar_off, cn, stage[w], dst, lane, sam_tail_of(in, tg, in.n_reads + i, r, x, true));
    }
}

// in: the struct in host memory, its pointers the device's
int format_dev(mcx_ctx *c, SamState *st, const mcx_sam_in &in, const mcx_sam_tags &tg, uint8_t *d_text, uint64_t cap, uint64_t *d_line_off, uint64_t *n_bytes)
{
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    const uint64_t n = in.n_reads;
    if (int rc = sam_scan_room(st, n + 1, s)) return rc;
    const SamContigs cn = {st->d_cn_text, st->d_cn_off};
    uint64_t *off = d_line_off ? d_line_off : st->d_off;
    HIP_TRY(hipEventRecord(st->ev[0], s));
    const bool tags = tg.mate_tags || (tg.rg && tg.rg_len);
    (tags ? k_sam_len<true> : k_sam_len<false>)<<<(unsigned)((n + 1 + 255) / 256), 256, 0, s>>>(in, tg, cn, st->d_len);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st->ev[1], s));
    size_t tmp = st->tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(st->d_tmp, tmp, st->d_len, off, (int)(n + 1), s));
    HIP_TRY(hipEventRecord(st->ev[2], s));
    HIP_TRY(hipMemcpyAsync(st->h_total, off + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t total = *st->h_total;
    if (n_bytes) *n_bytes = total;
    HIP_TRY(hipEventElapsedTime(&st->ms[0], st->ev[0], st->ev[1]));
    HIP_TRY(hipEventElapsedTime(&st->ms[1], st->ev[1], st->ev[2]));
    st->ms[2] = 0;
    if (total > cap || (total && !d_text)) return mcx_set_error(MCX_ERR_CAPACITY, "the batch's SAM text takes " + std::to_string(total) + " bytes: more than the buffer holds");
    HIP_TRY(hipEventRecord(st->ev[2], s));
    (tags ? k_sam_write<true> : k_sam_write<false>)<<<(unsigned)((n + kSamWaves - 1) / kSamWaves), 64 * kSamWaves, 0, s>>>(in, tg, cn, off, d_text);
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

extern "C" int mcx_sam_format_tags_dev(mcx_ctx *c, const mcx_sam_in *d_in, const mcx_sam_tags *tags, uint8_t *d_text, uint64_t cap, uint64_t *d_line_off, uint64_t *n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    if (!c || !d_in) return mcx_set_error(MCX_ERR_ARG, "mcx_sam_format_dev: null argument");
    if (!tags_ok(d_in, tags)) return mcx_set_error(MCX_ERR_UNSUPPORTED, std::string("mcx_sam_format_dev") + kTagsWithExtras);
    if (d_in->n_reads == 0) return 0;
    if (!in_ok(d_in)) return mcx_set_error(MCX_ERR_ARG, "mcx_sam_format_dev: null argument");
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    return format_dev(c, st, *d_in, tags ? *tags : mcx_sam_tags(), d_text, cap, d_line_off, n_bytes);
}
extern "C" int mcx_sam_format_dev(mcx_ctx *c, const mcx_sam_in *d_in, uint8_t *d_text, uint64_t cap, uint64_t *d_line_off, uint64_t *n_bytes)
{
    return mcx_sam_format_tags_dev(c, d_in, nullptr, d_text, cap, d_line_off, n_bytes);
}

// the last call's device times in ms: length kernel, scan, write kernel (scripts/sam_rate.py)
extern "C" int mcx_sam_last_ms(mcx_ctx *c, float ms[3])
{
    SamState *st;
    if (!c || !ms) return mcx_set_error(MCX_ERR_ARG, "mcx_sam_last_ms: null argument");
    if (int rc = sam_state_of(c, &st)) return rc;
    memcpy(ms, st->ms, sizeof st->ms);
    return 0;
}

extern "C" int mcx_sam_format(mcx_ctx *c, const mcx_sam_in *in, uint8_t *text, uint64_t cap, uint64_t *line_off, uint64_t *n_bytes)
{
    return mcx_sam_format_tags(c, in, nullptr, text, cap, line_off, n_bytes);
}
extern "C" int mcx_sam_format_tags(mcx_ctx *c, const mcx_sam_in *in, const mcx_sam_tags *tags, uint8_t *text, uint64_t cap, uint64_t *line_off, uint64_t *n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    if (!c || !in) return mcx_set_error(MCX_ERR_ARG, "mcx_sam_format: null argument");
    if (!tags_ok(in, tags)) return mcx_set_error(MCX_ERR_UNSUPPORTED, std::string("mcx_sam_format") + kTagsWithExtras);
    const uint64_t n = in->n_reads;
    if (n == 0) return 0;
    if (!in_ok(in)) return mcx_set_error(MCX_ERR_ARG, "mcx_sam_format: null argument");
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
    uint64_t *d_off64 = nullptr; uint8_t *d_text = nullptr;
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
    if (hipMalloc((void **)&d_all, all) != hipSuccess) { (void)hipGetLastError(); return mcx_set_error(MCX_ERR_DEVICE, "mcx_sam_format: no room in HBM for the batch"); }
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    int rc = 0;
    uint64_t at = 0;
    for (const Piece &p : pieces) {
        *p.dst = p.src ? (void *)(d_all + at) : nullptr;
        if (p.src && p.bytes && hipMemcpyAsync(d_all + at, p.src, p.bytes, hipMemcpyHostToDevice, s) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_sam_format: copy to the device failed");
        at += (p.bytes + 15) / 16 * 16 + 16;
    }
    if (rc == 0 && line_off && hipMalloc((void **)&d_off64, (n + 1) * 8) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_sam_format: no room in HBM for the lines' offsets");
    if (rc == 0 && cap && text && hipMalloc((void **)&d_text, cap) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_sam_format: no room in HBM for the text");
    uint64_t total = 0;
    if (rc == 0) rc = format_dev(c, st, d, tg, d_text, d_text ? cap : 0, d_off64, &total);
    if (n_bytes) *n_bytes = total;
    if (rc == 0 && total && hipMemcpy(text, d_text, total, hipMemcpyDeviceToHost) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_sam_format: copy from the device failed");
    if ((rc == 0 || rc == MCX_ERR_CAPACITY) && line_off && hipMemcpy(line_off, d_off64, (n + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = mcx_set_error(MCX_ERR_DEVICE, "mcx_sam_format: copy from the device failed");
    (void)hipStreamSynchronize(s);
    (void)hipFree(d_all); (void)hipFree(d_off64); (void)hipFree(d_text);
    return rc;
}

extern "C" int mcx_sam_header(const mcx_index *ix, char *out, uint64_t cap, uint64_t *n_bytes)
{
    if (n_bytes) *n_bytes = 0;
    if (!ix) return mcx_set_error(MCX_ERR_ARG, "mcx_sam_header: null argument");
    std::string h;
    sam_header(ix->host, h);
    if (n_bytes) *n_bytes = h.size();
    if (h.size() > cap || !out) return mcx_set_error(MCX_ERR_CAPACITY, "the SAM header takes " + std::to_string(h.size()) + " bytes: more than the buffer holds");
    memcpy(out, h.data(), h.size());
    return 0;
}

// The file front end's -gpu_sam, for one mapped part of a batch still in its slot: names (name_off: n_reads + 1) and NUL-padded qualities (null: FASTA) from
// page-locked host memory go behind the reads, the text is made from the part's records, CIGAR pool and (-m) the context's extras, and arrives at
// (*text)[at ..], a page-locked buffer that grows as needed (*text_cap).  On the context's stream, waited for.
static int sam_part(mcx_ctx *c, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired, const uint8_t *names, const uint32_t *name_off,
                    const uint8_t *qual, uint64_t qual_bytes, bool on_device, const mcx_aln *d_aln, const uint32_t *d_cigar, uint8_t **text, uint64_t *text_cap, uint64_t at, uint64_t *n_bytes, mcx_sam_bgzf *bgzf);
int mcx_sam_part(mcx_ctx *c, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired, const uint8_t *names, const uint32_t *name_off,
                 const uint8_t *qual, uint64_t qual_bytes, const mcx_aln *d_aln, const uint32_t *d_cigar, uint8_t **text, uint64_t *text_cap, uint64_t at, uint64_t *n_bytes, mcx_sam_bgzf *bgzf)
{
    return sam_part(c, d_bases, d_off, n_reads, paired, names, name_off, qual, qual_bytes, false, d_aln, d_cigar, text, text_cap, at, n_bytes, bgzf);
}
// Its twin for names, name offsets and NUL-padded qualities that lie in HBM already (the resident route: mcx_fastq_parse_dev's outputs): nothing is copied in
int mcx_sam_part_dev(mcx_ctx *c, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired, const uint8_t *d_names, const uint32_t *d_name_off,
                     const uint8_t *d_qual, const mcx_aln *d_aln, const uint32_t *d_cigar, uint8_t **text, uint64_t *text_cap, uint64_t at, uint64_t *n_bytes, mcx_sam_bgzf *bgzf)
{
    return sam_part(c, d_bases, d_off, n_reads, paired, d_names, d_name_off, d_qual, 0, true, d_aln, d_cigar, text, text_cap, at, n_bytes, bgzf);
}
static int sam_part(mcx_ctx *c, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired, const uint8_t *names, const uint32_t *name_off,
                    const uint8_t *qual, uint64_t qual_bytes, bool on_device, const mcx_aln *d_aln, const uint32_t *d_cigar, uint8_t **text, uint64_t *text_cap, uint64_t at, uint64_t *n_bytes, mcx_sam_bgzf *bgzf)
{
    *n_bytes = 0;
    if (n_reads == 0) return 0;
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    int rc;
    if ((rc = sam_state_of(c, &st))) return rc;
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    if (!on_device) {
        const uint64_t name_bytes = name_off[n_reads];
        if ((rc = sam_grow(&st->d_names, &st->cap_names, name_bytes + 16, "the reads' names"))) return rc;
        if ((rc = sam_grow(&st->d_name_off, &st->cap_name_off, (uint64_t)n_reads + 1, "the reads' names"))) return rc;
        if (qual && (rc = sam_grow(&st->d_qual, &st->cap_qual, qual_bytes + 16, "the reads' qualities"))) return rc;
        HIP_TRY(hipMemcpyAsync(st->d_names, names, name_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(st->d_name_off, name_off, ((size_t)n_reads + 1) * 4, hipMemcpyHostToDevice, s));
        if (qual) HIP_TRY(hipMemcpyAsync(st->d_qual, qual, qual_bytes, hipMemcpyHostToDevice, s));
    }
    mcx_sam_in in;
    memset(&in, 0, sizeof in);
    in.bases = d_bases; in.off = d_off;
    in.qual = on_device ? qual : qual ? st->d_qual : nullptr; in.names = on_device ? names : st->d_names; in.name_off = on_device ? name_off : st->d_name_off;
    in.aln = d_aln; in.cigar = d_cigar; in.n_reads = n_reads; in.paired = paired;
    uint32_t n_recs = 0, n_words = 0;
    if (mcx_ctx_multi(c) && (rc = mcx_multi_lines(c, &in.x_index, &in.x_recs, &in.x_cigar, &n_recs, &n_words))) return rc;
    // -md: the lines' MD strings first, into a pool of the state's own that the formatter copies them from
    uint64_t md_bytes = 0;
    if (st->want_md && (rc = mcx_md_part_dev(c, &in, in.x_index ? n_recs : 0, &md_bytes))) return rc;
    // the size first (nothing is written into a text buffer that is too small), then room for it on both sides; -bam: the part's records instead of its text
    const bool bam = bgzf && bgzf->bam;
    uint64_t total = 0, dropped = 0;
    const mcx_sam_tags tg = st->tags; // -rg / -mc: the run's (mcx_tags_set); a part of single reads gets no mate tags by the rule
    auto make = [&] { return bam ? mcx_bam_part_dev(c, &in, &tg, st->d_text, st->cap_text, &total, &dropped) : format_dev(c, st, in, tg, st->d_text, st->cap_text, nullptr, &total); };
    rc = make();
    if (rc == MCX_ERR_CAPACITY) {
        if ((rc = sam_grow(&st->d_text, &st->cap_text, total + 16, bam ? "the batch's BAM records" : "the batch's SAM text"))) return rc;
        rc = make();
    }
    if (rc) return rc;
    if (bam) bgzf->dropped += dropped;
    // -sort: the part's records in coordinate order — a run of the merge — in a second buffer
    const uint8_t *d_plain = st->d_text;
    if (bam && bgzf->sort) {
        bgzf->sort->keys.clear(); bgzf->sort->lens.clear();
        // -markdup: the part's units while its records still lie in read order, a pair's mates side by side
        if (bgzf->sort->dup && (rc = mcx_markdup_part(c, n_reads, total, paired, bgzf->sort->dup))) return rc;
        if (total && (rc = mcx_bam_sort_part(c, n_reads, total, bgzf->sort, &d_plain))) return rc;
    }
    // -bgzf: the part's text is compressed where it lies (a fresh block at its start), and only the blocks leave the device
    const uint8_t *d_from = d_plain;
    if (bgzf && total) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t bound = mcx_bgzf_bound(total, bgzf->block);
        if ((rc = sam_grow(&st->d_bgzf, &st->cap_bgzf, bound, "the batch's BGZF blocks"))) return rc;
        uint64_t made = 0;
        if ((rc = mcx_bgzf_deflate_dev(bgzf->deflater, d_plain, total, st->d_bgzf, st->cap_bgzf, &made))) return rc;
        bgzf->text_bytes += total; bgzf->out_bytes += made;
        bgzf->seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        d_from = st->d_bgzf; total = made;
    }
    if (at + total > *text_cap) {
        const uint64_t want = (at + total) + (at + total) / 8 + 4096;
        uint8_t *p = (uint8_t *)mcx_pinned_alloc(want);
        if (!p) return mcx_set_error(MCX_ERR_DEVICE, "cannot allocate pinned host memory for the batch's SAM text: map with a smaller -batch");
        if (at) memcpy(p, *text, at);
        mcx_pinned_free(*text);
        *text = p; *text_cap = want;
    }
    HIP_TRY(hipMemcpyAsync(*text + at, d_from, total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n_bytes = total;
    return 0;
}

// -rg / -mc of the file front end: the read group's ID goes to HBM once per run, and the context's following mcx_sam_part[_dev] calls hand it and the mate-tag
// switch to their formatter; id null and mate_tags 0 (the end of the run): both off, the ID's bytes freed
int mcx_tags_set(mcx_ctx *c, const char *id, uint32_t id_len, int mate_tags)
{
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    SamState *st;
    if (int rc = sam_state_of(c, &st)) return rc;
    if (st->d_rg) { (void)hipFree(st->d_rg); st->d_rg = nullptr; }
    st->tags = mcx_sam_tags();
    st->tags.mate_tags = mate_tags ? 1 : 0;
    if (id && id_len) {
        HIP_TRY(hipMalloc((void **)&st->d_rg, id_len));
        HIP_TRY(hipMemcpy(st->d_rg, id, id_len, hipMemcpyHostToDevice));
        st->tags.rg = st->d_rg; st->tags.rg_len = id_len;
    }
    return 0;
}
