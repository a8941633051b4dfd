// mapcaller_amd/csrc/mcx_fastq.hip — FASTQ text parsed on the device (mcx_fastq_parser_create / _free / _set_rule, mcx_fastq_parse_dev, mcx_fastq_parse; the file
// front end's -gpu_parse goes through mcx_fastq_stage / mcx_fastq_staged_sizes / mcx_fastq_staged_out).
//
// Replaces, for text that lies in HBM, the reader's MappedFastq::parse + pack_row (mcx_files.cpp); the rules are mcx_fastq.h's.  Per call, on the
// parser's own stream, for each text (blockIdx.y):
//   k_count     newlines per 4 KB block of the text: a 16-byte load per lane, byte compares, a wave reduction
//   (hipCUB)    exclusive sum of the block counts; its last entry is the text's number of newlines
//   k_lines     the 32-bit start of every line up to 4 * max_records: a lane's rank in its block from a scan of the lanes' counts
//   (GZ rule)   k_count notes as well whether the text holds a NUL; k_line_pieces a lane per line: its pieces of 1023 bytes; an exclusive sum; k_pieces a lane
//               per piece: its line by search over the sums, its start — the piece table, which the kernels below take in the line table's place
//   k_records   one lane per record: record_of; the records that end the text feed a wave-min and one atomicMin per wave
//   k_finish    records taken, why no more, bytes consumed, reads
//   k_lens      rlen and name_len per read in output order; k_odd<false> the bytes per read that are not ACGT; three exclusive sums
// the host then reads the totals (the one wait in the middle), judges the caller's capacities, and queues
//   k_gather    a wavefront per read: bases, NUL-padded qualities, names to their offsets
//   k_rows      one lane per word of a row; k_odd<true> a wavefront per read writes its odd bytes in position order at the read's offset
// FASTA (mcx_fastq_parser_set_format).  Under the GZ rule the same kernels with two pieces to a record.  Under the plain rule a record has no fixed number of
// lines, so the line table covers the whole text — the host reads the text's newline count behind the first sum (one more wait) and grows the scratch — and
//   k_fa_lines   a lane per line: is it a header, how many bases does it give; two exclusive sums: every header's record number, every line's base offset
//   k_fa_heads   a lane per line: header number k lies in line hl[k]
//   k_fa_records a lane per record: fa_record_of — rlen is a difference of two sums; the stop as in k_records
//   k_fa_gather  a wavefront per read walks its lines into the contiguous layout, in scratch of the parser's: k_odd and k_rows then read the bases there
// No kernel waits for another workgroup; every loop is bounded by the text's or a record's length; every load lies inside text[0 .. bytes) — the
// 16-byte loads start at the 16-byte boundary at or before the text's first byte, and the chunks that hold the text's head and tail go byte by byte.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/mcx.h"
#include "mcx_fastq.h"
#include "mcx_internal.h"

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace {

using namespace mcx::fq;

enum : uint32_t { kThreads = 256, kBlockBytes = kThreads * 16 };

struct Text { // one text of a call, as the kernels see it
    const uint8_t *text;
    uint32_t bytes, lead;    // lead: bytes between the 16-byte boundary the blocks start at and the text's first byte
    uint32_t n_blocks;       // blocks of kBlockBytes from that boundary on
    uint32_t eff_max;        // min(max_records, bytes / 3 + 1): a record that is taken holds three bytes at least
    uint32_t *cnt, *pre;     // [n_blocks + 1] newlines per block, their exclusive sums (pre[n_blocks]: all of them)
    uint32_t *ls;            // [4 * eff_max + 1] line starts
    uint32_t *pc, *po, *ps;  // GZ rule, [4 * eff_max + 1] each: pieces per line, their exclusive sums, piece starts
    uint64_t ls_last;        // the last line start anyone asks for: 4 * eff_max; plain FASTA: n_nl
    uint32_t n_nl;           // plain FASTA: the text's newlines, as the host read them from pre[n_blocks]
    uint32_t *fh, *fp, *hn, *bo, *hl; // plain FASTA, [n_nl + 2] each: a line's header flag and payload, their exclusive sums, the headers' lines
    mcx_fastq_rec *recs;     // [eff_max]
};
struct Job {
    Text t[2];
    uint32_t nt, upper;      // texts; nt * eff_max(largest): the reads a call can give
    int32_t max_read_len, final;
    int32_t rule;            // MCX_FASTQ_RULE_*
    uint32_t stride;         // lines or pieces to a record: 4, FASTA under the GZ rule 2
    int32_t fa;              // plain FASTA: the kernels of its own
};
struct DevInfo { // what the kernels tell the host
    unsigned long long stop_key[2]; // (first record that ends the text << 8 | why), minimum over the records
    uint32_t any_nul[2];            // GZ rule: the text holds a NUL somewhere (k_count)
    uint32_t n_nl[2];               // (host side only) plain FASTA: where the texts' newline counts arrive
    mcx_fastq_info info;
};

// the 16 bytes at blocks' position v (a multiple of 16) as a mask of its bytes equal to kByte; bytes outside the text count as none
template <uint32_t kByte>
__device__ __forceinline__ uint32_t byte_mask(const Text &t, uint64_t v)
{
    const int64_t p0 = (int64_t)v - (int64_t)t.lead;
    uint32_t m = 0;
    if (p0 >= 0 && p0 + 16 <= (int64_t)t.bytes) {
        const uint4 q = *reinterpret_cast<const uint4 *>(t.text + p0); // (text + p0 is the boundary + v: aligned)
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        MCX_UNROLL
        for (int i = 0; i < 4; i++) {
            MCX_UNROLL
            for (int j = 0; j < 4; j++) m |= (((w[i] >> (8 * j)) & 0xFFu) == kByte ? 1u : 0u) << (4 * i + j);
        }
    } else { // the text's head or tail (or a chunk outside it altogether)
        for (int j = 0; j < 16; j++) {
            const int64_t p = p0 + j;
            if (p >= 0 && p < (int64_t)t.bytes && t.text[p] == (uint8_t)kByte) m |= 1u << j;
        }
    }
    return m;
}
__device__ __forceinline__ uint32_t newline_mask(const Text &t, uint64_t v) { return byte_mask<(uint32_t)'\n'>(t, v); }

__global__ void k_init(DevInfo *d, Job job)
{
    if (threadIdx.x || blockIdx.x) return;
    for (uint32_t t = 0; t < 2; t++) { d->stop_key[t] = ((unsigned long long)(t < job.nt ? job.t[t].eff_max : 0u) << 8) | MCX_FASTQ_MORE; d->any_nul[t] = 0; }
    d->info = mcx_fastq_info{};
    if (!job.fa) for (uint32_t t = 0; t < job.nt; t++) job.t[t].ls[0] = 0; // (plain FASTA: the line table is made once the text's lines are counted)
}

// kGz: whether the text holds a NUL is noted on the way (the same 16 bytes; one atomicOr per workgroup that saw one — a flag, no order hangs on it)
template <bool kGz>
__global__ void __launch_bounds__(kThreads) k_count(Job job, DevInfo *d)
{
    const Text &t = job.t[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b > t.n_blocks) return; // (the whole workgroup)
    __shared__ uint32_t part[kThreads / 64];
    uint32_t c = b < t.n_blocks ? __popc(newline_mask(t, (uint64_t)b * kBlockBytes + threadIdx.x * 16u)) : 0u;
    if (kGz) {
        const bool nul = b < t.n_blocks && byte_mask<0u>(t, (uint64_t)b * kBlockBytes + threadIdx.x * 16u) != 0;
        if (__syncthreads_or(nul) && threadIdx.x == 0) atomicOr(&d->any_nul[blockIdx.y], 1u);
    }
    for (int s = 32; s; s >>= 1) c += __shfl_xor(c, s);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) t.cnt[b] = part[0] + part[1] + part[2] + part[3]; // (block n_blocks: 0, so that the sums end with the total)
}

__global__ void __launch_bounds__(kThreads) k_lines(Job job)
{
    const Text &t = job.t[blockIdx.y];
    const uint32_t b = blockIdx.x;
    if (b >= t.n_blocks) return;
    __shared__ uint32_t part[kThreads / 64];
    const uint64_t v = (uint64_t)b * kBlockBytes + threadIdx.x * 16u;
    uint32_t m = newline_mask(t, v);
    const uint32_t c = __popc(m), lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = c;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if ((int)lane >= d) inc += o; }
    if (lane == 63) part[w] = inc;
    __syncthreads();
    uint64_t rank = (uint64_t)t.pre[b] + (inc - c); // newlines of the text before this lane's first
    for (uint32_t i = 0; i < w; i++) rank += part[i];
    const uint64_t last = t.ls_last; // the last line start anyone asks for
    const uint32_t p0 = (uint32_t)(v - t.lead); // (only used where a bit is set: the byte lies inside the text)
    while (m) {
        const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1;
        rank++;
        if (rank <= last) t.ls[rank] = p0 + j + 1;
    }
}

// GZ rule: a lane per line L <= 4 * eff_max: its pieces (0 behind the lines that count)
__global__ void __launch_bounds__(kThreads) k_line_pieces(Job job)
{
    const Text &t = job.t[blockIdx.y];
    const uint64_t L = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (L > 4ull * t.eff_max) return;
    const uint64_t n_nl = t.pre[t.n_blocks];
    t.pc[L] = gz_line_pieces(t.ls, n_nl, t.bytes, gz_lines_counted(t.ls, n_nl, t.bytes, t.eff_max), (uint32_t)L);
}

// GZ rule: a lane per entry q <= 4 * eff_max of the piece table — no lane walks a line's pieces, however long the line
__global__ void __launch_bounds__(kThreads) k_pieces(Job job)
{
    const Text &t = job.t[blockIdx.y];
    const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q > 4ull * t.eff_max) return;
    const uint64_t n_nl = t.pre[t.n_blocks];
    uint32_t start;
    if (gz_piece_entry(t.ls, n_nl, t.bytes, t.po, t.eff_max, gz_lines_counted(t.ls, n_nl, t.bytes, t.eff_max), (uint32_t)q, start)) t.ps[q] = start;
}

template <bool kGz>
__global__ void __launch_bounds__(kThreads) k_records(Job job, DevInfo *d)
{
    const Text &t = job.t[blockIdx.y];
    const uint64_t k64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t k = 0xFFFFFFFFu, why = MCX_FASTQ_MORE;
    bool ends = false;
    if (k64 < t.eff_max) {
        k = (uint32_t)k64;
        const uint64_t n_nl = kGz ? gz_pieces_counted(t.po, t.eff_max) : t.pre[t.n_blocks]; // (kGz: pieces, in t.ps)
        if (!job.final && !(kGz ? gz_record_whole(t.text, t.bytes, t.ps, n_nl, k, job.stride) : record_whole(n_nl, k))) ends = true;
        else {
            mcx_fastq_rec rec;
            rec.name = rec.name_len = rec.seq = rec.rlen = rec.qual = rec.q_take = 0;
            why = kGz ? gz_record_of(t.text, t.bytes, t.ps, n_nl, k, job.max_read_len, d->any_nul[blockIdx.y] != 0, rec, job.stride) : record_of(t.text, t.bytes, t.ls, n_nl, k, job.max_read_len, rec);
            if (why == MCX_FASTQ_MORE) t.recs[k] = rec; else ends = true;
        }
    }
    uint32_t first = ends ? k : 0xFFFFFFFFu;
    for (int s = 32; s; s >>= 1) first = min(first, (uint32_t)__shfl_xor(first, s));
    if (ends && k == first) atomicMin(&d->stop_key[blockIdx.y], ((unsigned long long)k << 8) | why);
}

// ---- plain FASTA ----------------------------------------------------------------------------------------------
// a lane per line L <= n_nl + 1: header flag and payload (0, 0 from the text's last line on, so that the sums end with the totals)
__global__ void __launch_bounds__(kThreads) k_fa_lines(Job job)
{
    const Text &t = job.t[blockIdx.y];
    const uint64_t L = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (L > (uint64_t)t.n_nl + 1) return;
    uint32_t h, pay;
    fa_line(t.text, t.bytes, t.ls, t.n_nl, fa_n_lines(t.ls, t.n_nl, t.bytes), (uint32_t)L, h, pay);
    t.fh[L] = h; t.fp[L] = pay;
}

// a lane per line: header number hn[L] lies in line L; behind the last header, the number of lines
__global__ void __launch_bounds__(kThreads) k_fa_heads(Job job)
{
    const Text &t = job.t[blockIdx.y];
    const uint64_t L = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t n_lines = fa_n_lines(t.ls, t.n_nl, t.bytes);
    if (L > n_lines) return;
    if (L == n_lines || t.fh[L]) t.hl[t.hn[L]] = (uint32_t)L; // (hn[L] <= L: inside hl[0 .. n_nl + 1])
}

// one lane per record, as k_records
__global__ void __launch_bounds__(kThreads) k_fa_records(Job job, DevInfo *d)
{
    const Text &t = job.t[blockIdx.y];
    const uint64_t k64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t k = 0xFFFFFFFFu, why = MCX_FASTQ_MORE;
    bool ends = false;
    if (k64 < t.eff_max) {
        k = (uint32_t)k64;
        mcx_fastq_rec rec;
        rec.name = rec.name_len = rec.seq = rec.rlen = rec.qual = rec.q_take = 0;
        bool taken;
        why = fa_record_of(t.text, t.bytes, t.ls, t.n_nl, t.bo, t.hl, t.hn[fa_n_lines(t.ls, t.n_nl, t.bytes)], k, job.max_read_len, job.final, rec, taken);
        if (taken) t.recs[k] = rec; else ends = true;
    }
    uint32_t first = ends ? k : 0xFFFFFFFFu;
    for (int s = 32; s; s >>= 1) first = min(first, (uint32_t)__shfl_xor(first, s));
    if (ends && k == first) atomicMin(&d->stop_key[blockIdx.y], ((unsigned long long)k << 8) | why);
}

__global__ void k_finish(Job job, DevInfo *d)
{
    if (threadIdx.x || blockIdx.x) return;
    mcx_fastq_info &f = d->info;
    for (uint32_t i = 0; i < job.nt; i++) {
        const Text &t = job.t[i];
        const uint32_t n = (uint32_t)(d->stop_key[i] >> 8);
        const bool gz = job.rule == MCX_FASTQ_RULE_GZ;
        f.n_records[i] = n; f.stop[i] = (uint32_t)(d->stop_key[i] & 0xFFu);
        if (job.fa) { f.consumed[i] = fa_consumed(t.ls, t.hl, t.hn[fa_n_lines(t.ls, t.n_nl, t.bytes)], n, t.bytes); continue; } // (the start of a header line)
        const uint64_t n_nl = gz ? gz_pieces_counted(t.po, t.eff_max) : t.pre[t.n_blocks], at = (uint64_t)job.stride * n;
        f.consumed[i] = at <= n_nl ? (gz ? t.ps : t.ls)[at] : t.bytes; // (GZ rule: a piece start of its line)
    }
    f.n_reads = job.nt == 2 ? 2u * min(f.n_records[0], f.n_records[1]) : f.n_records[0];
}

__device__ __forceinline__ const mcx_fastq_rec &rec_of(const Job &job, uint32_t r, uint32_t &t)
{
    t = job.nt == 2 ? (r & 1u) : 0u;
    return job.t[t].recs[job.nt == 2 ? (r >> 1) : r];
}

// rl, nl [upper + 1]: rlen and name_len of read r, 0 from n_reads on
__global__ void __launch_bounds__(kThreads) k_lens(Job job, DevInfo *d, uint32_t *rl, uint32_t *nl)
{
    const uint64_t r64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t a = 0, b = 0;
    if (r64 < d->info.n_reads) { uint32_t t; const mcx_fastq_rec &c = rec_of(job, (uint32_t)r64, t); a = c.rlen; b = c.name_len; }
    if (r64 <= job.upper) { rl[r64] = a; nl[r64] = b; }
    uint32_t longest = a;
    for (int s = 32; s; s >>= 1) longest = max(longest, (uint32_t)__shfl_xor(longest, s));
    if ((threadIdx.x & 63u) == 0 && longest) atomicMax(&d->info.longest, longest);
}

// A wavefront per read.  kWrite false: oc[r] = the read's bytes that are not upper-case ACGT (0 from n_reads on, oc [upper + 1]); true: those bytes'
// entries in position order at odd[ooff[r] ..).  fb: the reads' bases lie back to back at fb + foff[r] (plain FASTA), not in the text.
template <bool kWrite>
__global__ void __launch_bounds__(kThreads) k_odd(Job job, const DevInfo *d, uint32_t *oc, const uint32_t *ooff, uint64_t *odd, const uint8_t *fb, const uint32_t *foff)
{
    const uint64_t r64 = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (r64 > job.upper) return; // (the whole wavefront)
    uint32_t n = 0;
    if (r64 < d->info.n_reads) {
        const uint32_t r = (uint32_t)r64;
        uint32_t t;
        const mcx_fastq_rec c = rec_of(job, r, t);
        const uint8_t *seq = fb ? fb + foff[r] : job.t[t].text + c.seq;
        for (uint32_t i0 = 0; i0 < c.rlen; i0 += 64) {
            const uint32_t i = i0 + lane;
            const uint8_t ch = i < c.rlen ? seq[i] : (uint8_t)'A';
            const bool is = code_of(ch) > 3;
            const unsigned long long m = __ballot(is);
            if (kWrite && is) odd[(uint64_t)ooff[r] + n + __popcll(m & ((1ull << lane) - 1ull))] = odd_entry(r, i, ch);
            n += (uint32_t)__popcll(m);
        }
    }
    if (!kWrite && lane == 0) oc[r64] = n;
}

__global__ void k_totals(Job job, DevInfo *d, const uint32_t *off, const uint32_t *noff, const uint32_t *ooff)
{
    if (threadIdx.x || blockIdx.x) return;
    d->info.n_bases = off[job.upper]; d->info.n_name_bytes = noff[job.upper]; d->info.n_odd = ooff[job.upper];
}

// a wavefront per read: its bases, its quality bytes with NUL behind them, its name; a null destination is skipped
__global__ void __launch_bounds__(kThreads) k_gather(Job job, uint32_t n_reads, const uint32_t *off, const uint32_t *noff, uint8_t *bases, uint8_t *qual, uint8_t *names)
{
    const uint64_t r64 = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (r64 >= n_reads) return;
    uint32_t t;
    const mcx_fastq_rec c = rec_of(job, (uint32_t)r64, t);
    const uint8_t *text = job.t[t].text;
    if (bases) {
        uint8_t *b = bases + off[r64];
        for (uint32_t i = lane; i < c.rlen; i += 64) b[i] = text[c.seq + i];
        if (qual) {
            uint8_t *q = qual + off[r64];
            for (uint32_t i = lane; i < c.rlen; i += 64) q[i] = i < c.q_take ? text[c.qual + i] : (uint8_t)0;
        }
    }
    if (names) {
        uint8_t *nm = names + noff[r64];
        for (uint32_t i = lane; i < c.name_len; i += 64) nm[i] = text[c.name + i];
    }
}

// plain FASTA, a wavefront per read: its lines' bases back to back at bases + off[r] — one line per step, the lanes side by side over its bytes (lines of
// 60 bases keep 60 of 64 lanes busy; the starts and sums are the same words for the whole wavefront).  Bounded by the record's lines and their lengths.
__global__ void __launch_bounds__(kThreads) k_fa_gather(Job job, const DevInfo *d, const uint32_t *off, uint8_t *bases)
{
    const uint64_t r64 = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (r64 >= d->info.n_reads) return; // (the whole wavefront)
    const uint32_t tt = job.nt == 2 ? ((uint32_t)r64 & 1u) : 0u, k = job.nt == 2 ? (uint32_t)(r64 >> 1) : (uint32_t)r64;
    const Text &t = job.t[tt];
    const uint32_t h = t.hl[k], nx = t.hl[k + 1], b0 = t.bo[h];
    uint8_t *dst = bases + off[r64];
    for (uint32_t L = h + 1; L < nx; L++) {
        const uint32_t s = t.ls[L], at = t.bo[L], n = t.bo[L + 1] - at; // (n: the line less its last byte — every load inside the line)
        for (uint32_t i = lane; i < n; i += 64) dst[at - b0 + i] = t.text[s + i];
    }
}

// one lane per word of the rows; the lane of a row's first word writes the read's length
__global__ void __launch_bounds__(kThreads) k_rows(Job job, uint32_t n_reads, uint32_t row_words, uint32_t *rows, uint32_t *len, const uint8_t *fb, const uint32_t *foff)
{
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= (uint64_t)n_reads * row_words) return;
    const uint32_t r = (uint32_t)(g / row_words), w = (uint32_t)(g % row_words);
    uint32_t t;
    const mcx_fastq_rec c = rec_of(job, r, t);
    const uint64_t i = 16ull * w;
    uint32_t word = 0;
    if (i < c.rlen) word = pack_word(fb ? fb + foff[r] : job.t[t].text + c.seq, (uint32_t)i, c.rlen - (uint32_t)i < 16u ? c.rlen - (uint32_t)i : 16u);
    rows[g] = word;
    if (w == 0) len[r] = c.rlen;
}

struct Buf { // device memory that grows
    void *p = nullptr; size_t cap = 0;
};

} // namespace

struct mcx_fastq_parser {
    int device = 0;
    hipStream_t stream = nullptr;
    int rule = MCX_FASTQ_RULE_PLAIN, format = MCX_READS_FASTQ;
    int mates = 0, host_n_ref = 0; // MCX_READS_BAM: taken records count in twos (set_mates); the n_ref of the host form's call in hand
    mcx_bam_in *bam = nullptr;     // ... its scratch and counters (mcx_bam_in.hip), made by the first such call
    Buf fp[2], bo[2], fa_bases; // plain FASTA: the lines' payloads and their sums (flags, their sums and the headers' lines share pc, po, ps); the reads' bases back to back
    Buf cnt[2], pre[2], ls[2], pc[2], po[2], ps[2], recs[2], rl, nl, oc, off, noff, ooff, tmp, info;
    DevInfo *h_info = nullptr; // page-locked
    // the host forms: the texts' page-locked staging and their twin in HBM; the outputs' buffers in HBM
    uint8_t *h_text = nullptr; size_t h_text_cap = 0;
    Buf d_text, o_recs[2], o_bases, o_qual, o_off, o_names, o_noff, o_rows, o_len, o_odd;
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms = 0; // the last mcx_fastq_parse_dev, first kernel to last, by the events around them
    uint32_t grown = 0; // how often a buffer had to grow (the tests look at it)
    Job job;            // of the last sizes pass: what the output pass works on
};

namespace {

int grow(mcx_fastq_parser *p, Buf &b, size_t need, const char *what)
{
    if (need <= b.cap) return 0;
    if (b.p) { (void)hipStreamSynchronize(p->stream); (void)hipFree(b.p); p->grown++; }
    b.p = nullptr; b.cap = 0;
    const size_t cap = need + need / 8 + 256;
    if (hipMalloc(&b.p, cap) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return mcx_set_error(MCX_ERR_DEVICE, std::string("mcx_fastq: no room in HBM for ") + what + " (" + std::to_string(cap) + " bytes)"); }
    b.cap = cap;
    return 0;
}

int scan(mcx_fastq_parser *p, const uint32_t *in, uint32_t *out, uint64_t n)
{
    size_t tmp = p->tmp.cap;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(p->tmp.p, tmp, in, out, (int)n, p->stream));
    return 0;
}

} // namespace

extern "C" void mcx_fastq_parser_free(mcx_fastq_parser *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    Buf *all[] = {&p->cnt[0], &p->cnt[1], &p->pre[0], &p->pre[1], &p->ls[0], &p->ls[1], &p->pc[0], &p->pc[1], &p->po[0], &p->po[1], &p->ps[0], &p->ps[1], &p->recs[0], &p->recs[1], &p->rl, &p->nl, &p->oc, &p->off, &p->noff, &p->ooff, &p->tmp, &p->info,
                  &p->fp[0], &p->fp[1], &p->bo[0], &p->bo[1], &p->fa_bases, &p->d_text, &p->o_recs[0], &p->o_recs[1], &p->o_bases, &p->o_qual, &p->o_off, &p->o_names, &p->o_noff, &p->o_rows, &p->o_len, &p->o_odd};
    for (Buf *b : all) if (b->p) (void)hipFree(b->p);
    mcx_bam_in_free(p->bam);
    mcx_pinned_free(p->h_info); mcx_pinned_free(p->h_text);
    for (hipEvent_t e : p->ev) if (e) (void)hipEventDestroy(e);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

namespace {

// scratch for texts of these sizes and this many records per text
int reserve(mcx_fastq_parser *p, const uint64_t bytes[2], uint32_t nt, const uint32_t eff[2])
{
    int rc = 0;
    uint64_t most = 0;
    for (uint32_t t = 0; t < nt && !rc; t++) {
        const uint64_t nb = (bytes[t] + 15 + kBlockBytes - 1) / kBlockBytes + 1;
        most = std::max(most, nb);
        if ((rc = grow(p, p->cnt[t], nb * 4, "the block counts"))) break;
        if ((rc = grow(p, p->pre[t], nb * 4, "the block sums"))) break;
        const bool fa = p->format == MCX_READS_FASTA && p->rule == MCX_FASTQ_RULE_PLAIN; // (its line table is sized once the lines are counted: reserve_lines)
        if (!fa && (rc = grow(p, p->ls[t], (4ull * eff[t] + 1) * 4, "the line starts"))) break;
        if (p->rule == MCX_FASTQ_RULE_GZ) {
            most = std::max<uint64_t>(most, 4ull * eff[t] + 1);
            if ((rc = grow(p, p->pc[t], (4ull * eff[t] + 1) * 4, "the lines' pieces")) || (rc = grow(p, p->po[t], (4ull * eff[t] + 1) * 4, "the pieces' sums")) ||
                (rc = grow(p, p->ps[t], (4ull * eff[t] + 1) * 4, "the piece starts"))) break;
        }
        rc = grow(p, p->recs[t], std::max<uint64_t>(eff[t], 1) * sizeof(mcx_fastq_rec), "the records");
    }
    if (rc) return rc;
    const uint64_t upper1 = (uint64_t)nt * std::max(eff[0], nt == 2 ? eff[1] : 0u) + 1;
    most = std::max(most, upper1);
    Buf *per_read[] = {&p->rl, &p->nl, &p->oc, &p->off, &p->noff, &p->ooff};
    for (Buf *b : per_read) if ((rc = grow(p, *b, upper1 * 4, "the reads' lengths and offsets"))) return rc;
    size_t need = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)most, p->stream));
    return grow(p, p->tmp, need + 16, "the sums' scratch");
}

// plain FASTA: the tables of a text of n_nl newlines, and the sums' scratch for them
int reserve_lines(mcx_fastq_parser *p, uint32_t t, uint64_t n_nl)
{
    const uint64_t n = n_nl + 2;
    Buf *per_line[] = {&p->ls[t], &p->pc[t], &p->po[t], &p->ps[t], &p->fp[t], &p->bo[t]};
    for (Buf *b : per_line) if (int rc = grow(p, *b, n * 4, "the text's line table")) return rc;
    size_t need = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, p->stream));
    return grow(p, p->tmp, need + 16, "the sums' scratch");
}

uint32_t eff_max_of(uint32_t max_records, uint64_t bytes) { return (uint32_t)std::min<uint64_t>(max_records, bytes / 3 + 1); }
uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

} // namespace

extern "C" int mcx_fastq_parser_create(int device, uint64_t max_text_bytes, uint32_t max_records, mcx_fastq_parser **out)
{
    if (!out) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_parser_create: null argument");
    *out = nullptr;
    if (max_text_bytes >= (1ull << 32)) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_parser_create: a text holds less than 4 GiB");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { (void)hipGetLastError(); return mcx_set_error(MCX_ERR_DEVICE, "mcx_fastq_parser_create: no such device"); }
    HIP_TRY(hipSetDevice(device));
    mcx_fastq_parser *p = new mcx_fastq_parser();
    p->device = device;
    int rc = 0;
    if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess) rc = MCX_ERR_DEVICE;
    for (hipEvent_t &e : p->ev) if (rc == 0 && hipEventCreate(&e) != hipSuccess) rc = MCX_ERR_DEVICE;
    if (rc == 0 && !(p->h_info = (DevInfo *)mcx_pinned_alloc(sizeof(DevInfo)))) rc = MCX_ERR_DEVICE;
    if (rc) { (void)hipGetLastError(); mcx_fastq_parser_free(p); return mcx_set_error(MCX_ERR_DEVICE, "mcx_fastq_parser_create: no stream, events or page-locked memory"); }
    const uint64_t bytes[2] = {max_text_bytes ? max_text_bytes : (8ull << 20), 0};
    const uint32_t eff[2] = {eff_max_of(max_records ? max_records : 65536u, bytes[0]), 0};
    if ((rc = grow(p, p->info, sizeof(DevInfo), "the call's results")) || (rc = reserve(p, bytes, 1, eff))) { mcx_fastq_parser_free(p); return rc; }
    *out = p;
    return 0;
}

namespace {

// Everything up to the one wait: the records of both texts, the reads' lengths and offsets in the parser's scratch, the totals in *info.
int sizes_pass(mcx_fastq_parser *p, const mcx_fastq_in *in, mcx_fastq_info *info, const char *who)
{
    memset(info, 0, sizeof *info);
    if (p->format == MCX_READS_BAM) { // BAM records: kernels of their own (mcx_bam_in.hip) on this parser's stream; the rule setting is ignored
        memset(&p->job, 0, sizeof p->job);
        p->job.nt = 1; p->job.max_read_len = in->max_read_len;
        HIP_TRY(hipEventRecord(p->ev[0], p->stream));
        return mcx_bam_in_sizes(&p->bam, p->stream, in, p->mates, info, who);
    }
    const uint32_t nt = in->text[1] ? 2u : 1u;
    for (uint32_t t = 0; t < nt; t++) {
        if (!in->text[t] && in->bytes[t]) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": null text");
        if (in->bytes[t] >= (1ull << 32)) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": a text holds less than 4 GiB");
    }
    if (nt == 2 && in->bytes[0] + in->bytes[1] >= (1ull << 32)) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": the two texts together hold less than 4 GiB (32-bit offsets into the bases)");
    Job &job = p->job;
    memset(&job, 0, sizeof job);
    job.nt = nt; job.max_read_len = in->max_read_len; job.final = in->final; job.rule = p->rule;
    const bool gz = p->rule == MCX_FASTQ_RULE_GZ, fa = p->format == MCX_READS_FASTA && !gz;
    job.stride = gz && p->format == MCX_READS_FASTA ? 2u : 4u; job.fa = fa ? 1 : 0;
    uint32_t eff[2] = {0, 0}, most_blocks = 0, most_eff = 0;
    for (uint32_t t = 0; t < nt; t++) { eff[t] = eff_max_of(in->max_records, in->bytes[t]); most_eff = std::max(most_eff, eff[t]); }
    if ((uint64_t)nt * most_eff + 1 > 0x7FFFFFFFull) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": max_records is too large");
    if (gz && 4ull * most_eff + 1 > 0x7FFFFFFFull) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": max_records is too large (the GZ rule's piece table holds 4 * max_records + 1 entries)");
    if (int rc = reserve(p, in->bytes, nt, eff)) return rc;
    if (fa) if (int rc = grow(p, p->fa_bases, in->bytes[0] + (nt == 2 ? in->bytes[1] : 0) + 48, "the reads' bases")) return rc; // (a text holds no more bases than bytes)
    for (uint32_t t = 0; t < nt; t++) {
        Text &x = job.t[t];
        x.text = in->text[t]; x.bytes = (uint32_t)in->bytes[t];
        x.lead = (uint32_t)((uintptr_t)x.text & 15u);
        x.n_blocks = (uint32_t)(((uint64_t)x.bytes + x.lead + kBlockBytes - 1) / kBlockBytes);
        x.eff_max = eff[t]; x.ls_last = 4ull * eff[t];
        x.cnt = (uint32_t *)p->cnt[t].p; x.pre = (uint32_t *)p->pre[t].p; x.ls = (uint32_t *)p->ls[t].p; x.pc = (uint32_t *)p->pc[t].p; x.po = (uint32_t *)p->po[t].p; x.ps = (uint32_t *)p->ps[t].p; x.recs = (mcx_fastq_rec *)p->recs[t].p;
        most_blocks = std::max(most_blocks, x.n_blocks);
    }
    job.upper = nt * most_eff;
    DevInfo *d = (DevInfo *)p->info.p;
    uint32_t *rl = (uint32_t *)p->rl.p, *nl = (uint32_t *)p->nl.p, *oc = (uint32_t *)p->oc.p, *off = (uint32_t *)p->off.p, *noff = (uint32_t *)p->noff.p, *ooff = (uint32_t *)p->ooff.p;
    hipStream_t s = p->stream;

    HIP_TRY(hipEventRecord(p->ev[0], s));
    k_init<<<1, 64, 0, s>>>(d, job);
    if (gz) k_count<true><<<dim3(most_blocks + 1, nt), kThreads, 0, s>>>(job, d); else k_count<false><<<dim3(most_blocks + 1, nt), kThreads, 0, s>>>(job, d);
    HIP_TRY(hipGetLastError());
    for (uint32_t t = 0; t < nt; t++) if (int rc = scan(p, job.t[t].cnt, job.t[t].pre, (uint64_t)job.t[t].n_blocks + 1)) return rc;
    uint64_t most_lines = 0;
    if (fa) { // the host reads the texts' newline counts and sizes the line tables: the whole text's lines, whatever max_records is
        for (uint32_t t = 0; t < nt; t++) HIP_TRY(hipMemcpyAsync(&p->h_info->n_nl[t], job.t[t].pre + job.t[t].n_blocks, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint32_t t = 0; t < nt; t++) {
            Text &x = job.t[t];
            x.n_nl = p->h_info->n_nl[t]; x.ls_last = x.n_nl;
            if ((uint64_t)x.n_nl + 2 > 0x7FFFFFFFull) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": a text of more than 2^31 - 3 lines");
            if (int rc = reserve_lines(p, t, x.n_nl)) return rc;
            x.ls = (uint32_t *)p->ls[t].p; x.fh = (uint32_t *)p->pc[t].p; x.hn = (uint32_t *)p->po[t].p; x.hl = (uint32_t *)p->ps[t].p; x.fp = (uint32_t *)p->fp[t].p; x.bo = (uint32_t *)p->bo[t].p;
            HIP_TRY(hipMemsetAsync(x.ls, 0, 4, s));
            most_lines = std::max<uint64_t>(most_lines, (uint64_t)x.n_nl + 2);
        }
    }
    if (most_blocks) k_lines<<<dim3(most_blocks, nt), kThreads, 0, s>>>(job);
    if (fa) {
        const dim3 grid(blocks_for(most_lines, kThreads), nt);
        k_fa_lines<<<grid, kThreads, 0, s>>>(job);
        HIP_TRY(hipGetLastError());
        for (uint32_t t = 0; t < nt; t++) {
            if (int rc = scan(p, job.t[t].fh, job.t[t].hn, (uint64_t)job.t[t].n_nl + 2)) return rc;
            if (int rc = scan(p, job.t[t].fp, job.t[t].bo, (uint64_t)job.t[t].n_nl + 2)) return rc;
        }
        k_fa_heads<<<grid, kThreads, 0, s>>>(job);
        if (most_eff) k_fa_records<<<dim3(blocks_for(most_eff, kThreads), nt), kThreads, 0, s>>>(job, d);
    }
    if (gz) { // the piece table from the line table
        const dim3 grid(blocks_for(4ull * most_eff + 1, kThreads), nt);
        k_line_pieces<<<grid, kThreads, 0, s>>>(job);
        HIP_TRY(hipGetLastError());
        for (uint32_t t = 0; t < nt; t++) if (int rc = scan(p, job.t[t].pc, job.t[t].po, 4ull * job.t[t].eff_max + 1)) return rc;
        k_pieces<<<grid, kThreads, 0, s>>>(job);
    }
    if (most_eff && !fa) { if (gz) k_records<true><<<dim3(blocks_for(most_eff, kThreads), nt), kThreads, 0, s>>>(job, d); else k_records<false><<<dim3(blocks_for(most_eff, kThreads), nt), kThreads, 0, s>>>(job, d); }
    k_finish<<<1, 64, 0, s>>>(job, d);
    k_lens<<<blocks_for((uint64_t)job.upper + 1, kThreads), kThreads, 0, s>>>(job, d, rl, nl);
    if (fa) { // the bases back to back first: the odd bytes are counted there
        if (int rc = scan(p, rl, off, (uint64_t)job.upper + 1)) return rc;
        if (job.upper) k_fa_gather<<<blocks_for(job.upper, kThreads / 64), kThreads, 0, s>>>(job, d, off, (uint8_t *)p->fa_bases.p);
    }
    k_odd<false><<<blocks_for((uint64_t)job.upper + 1, kThreads / 64), kThreads, 0, s>>>(job, d, oc, nullptr, nullptr, fa ? (const uint8_t *)p->fa_bases.p : nullptr, off);
    HIP_TRY(hipGetLastError());
    if (!fa) if (int rc = scan(p, rl, off, (uint64_t)job.upper + 1)) return rc;
    if (int rc = scan(p, nl, noff, (uint64_t)job.upper + 1)) return rc;
    if (int rc = scan(p, oc, ooff, (uint64_t)job.upper + 1)) return rc;
    k_totals<<<1, 64, 0, s>>>(job, d, off, noff, ooff);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(p->h_info, d, sizeof(DevInfo), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s)); // the one wait in the middle: the host judges the capacities
    *info = p->h_info->info;
    return 0;
}

// The groups of `out` (device pointers) from the scratch of the sizes pass; a group whose capacity is too small is left alone and the call says so.
int output_pass(mcx_fastq_parser *p, const mcx_fastq_out *out, const mcx_fastq_info *info, const char *who)
{
    if (p->format == MCX_READS_BAM) {
        if (!p->bam) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": no sizes pass went before");
        const int rc = mcx_bam_in_out(p->bam, p->stream, out, info, who); // (waits for the stream)
        HIP_TRY(hipEventRecord(p->ev[1], p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        HIP_TRY(hipEventElapsedTime(&p->last_ms, p->ev[0], p->ev[1]));
        return rc;
    }
    const Job &job = p->job;
    const uint32_t n = info->n_reads;
    const uint32_t *off = (const uint32_t *)p->off.p, *noff = (const uint32_t *)p->noff.p, *ooff = (const uint32_t *)p->ooff.p;
    hipStream_t s = p->stream;
    int rc = 0;
    const bool want_bases = out->bases != nullptr, want_names = out->names != nullptr, want_rows = out->rows != nullptr;
    const bool do_bases = want_bases && out->bases_cap >= info->n_bases + 32, do_names = want_names && out->names_cap >= info->n_name_bytes, do_rows = want_rows && out->odd_cap >= info->n_odd;
    if (want_bases && !do_bases) rc = mcx_set_error(MCX_ERR_CAPACITY, std::string(who) + ": bases_cap is less than the " + std::to_string(info->n_bases) + " bases + 32");
    if (want_names && !do_names) rc = mcx_set_error(MCX_ERR_CAPACITY, std::string(who) + ": names_cap is less than the " + std::to_string(info->n_name_bytes) + " bytes of the names");
    if (want_rows && !do_rows) rc = mcx_set_error(MCX_ERR_CAPACITY, std::string(who) + ": odd_cap is less than the " + std::to_string(info->n_odd) + " bytes that are not ACGT");
    for (uint32_t t = 0; t < job.nt; t++)
        if (out->recs[t] && info->n_records[t]) HIP_TRY(hipMemcpyAsync(out->recs[t], job.t[t].recs, (size_t)info->n_records[t] * sizeof(mcx_fastq_rec), hipMemcpyDeviceToDevice, s));
    if (do_bases) HIP_TRY(hipMemcpyAsync(out->off, off, ((size_t)n + 1) * 4, hipMemcpyDeviceToDevice, s));
    if (do_names) HIP_TRY(hipMemcpyAsync(out->name_off, noff, ((size_t)n + 1) * 4, hipMemcpyDeviceToDevice, s));
    const uint8_t *fb = job.fa ? (const uint8_t *)p->fa_bases.p : nullptr; // plain FASTA: the sizes pass has left the bases back to back there; no quality: NULs
    if (fb && do_bases && info->n_bases) {
        HIP_TRY(hipMemcpyAsync(out->bases, fb, info->n_bases, hipMemcpyDeviceToDevice, s));
        if (out->qual) HIP_TRY(hipMemsetAsync(out->qual, 0, info->n_bases, s));
    }
    const bool g_bases = do_bases && !fb;
    if (n && (g_bases || do_names)) k_gather<<<blocks_for(n, kThreads / 64), kThreads, 0, s>>>(job, n, off, noff, g_bases ? out->bases : nullptr, g_bases ? out->qual : nullptr, do_names ? out->names : nullptr);
    if (n && do_rows) {
        if (out->row_words) k_rows<<<blocks_for((uint64_t)n * out->row_words, kThreads), kThreads, 0, s>>>(job, n, out->row_words, out->rows, out->len, fb, off);
        else HIP_TRY(hipMemcpyAsync(out->len, p->rl.p, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        if (info->n_odd) k_odd<true><<<blocks_for(n, kThreads / 64), kThreads, 0, s>>>(job, (const DevInfo *)p->info.p, nullptr, ooff, out->odd, fb, off);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(p->ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&p->last_ms, p->ev[0], p->ev[1]));
    return rc;
}

const char *rows_fault(const mcx_fastq_out *out, int32_t max_read_len)
{
    if ((out->bases && !out->off) || (out->names && !out->name_off) || (out->rows && (!out->len || (!out->odd && out->odd_cap)))) return "a group of outputs is given in part";
    if (out->rows && (int64_t)out->row_words * 16 < (int64_t)max_read_len) return "row_words is less than ceil(max_read_len / 16)";
    return nullptr;
}

} // namespace

extern "C" int mcx_fastq_parse_dev(mcx_fastq_parser *p, const mcx_fastq_in *in, const mcx_fastq_out *out, mcx_fastq_info *info)
{
    if (!p || !in || !out || !info) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_parse_dev: null argument");
    memset(info, 0, sizeof *info);
    if (const char *why = rows_fault(out, in->max_read_len)) return mcx_set_error(MCX_ERR_ARG, std::string("mcx_fastq_parse_dev: ") + why);
    if (out->bases && (((uintptr_t)out->bases & 15u) || (out->qual && ((uintptr_t)out->qual & 15u)))) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_parse_dev: bases and qual are 16-byte aligned");
    HIP_TRY(hipSetDevice(p->device));
    if (int rc = sizes_pass(p, in, info, "mcx_fastq_parse_dev")) return rc;
    return output_pass(p, out, info, "mcx_fastq_parse_dev");
}

extern "C" int mcx_fastq_parser_set_rule(mcx_fastq_parser *p, int rule)
{
    if (!p || (rule != MCX_FASTQ_RULE_PLAIN && rule != MCX_FASTQ_RULE_GZ)) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_parser_set_rule: null parser or no such rule");
    p->rule = rule;
    return 0;
}

extern "C" int mcx_fastq_parser_set_format(mcx_fastq_parser *p, int format)
{
    if (!p || (format != MCX_READS_FASTQ && format != MCX_READS_FASTA)) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_parser_set_format: null parser or no such format");
    p->format = format;
    return 0;
}

// set_format with the third format beside its two: MCX_READS_BAM is set here (mcx_fastq_parser_set_format keeps refusing every value but its own two)
extern "C" int mcx_fastq_parser_set_reads(mcx_fastq_parser *p, int format)
{
    if (!p || (format != MCX_READS_FASTQ && format != MCX_READS_FASTA && format != MCX_READS_BAM)) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_parser_set_reads: null parser or no such format");
    p->format = format;
    return 0;
}

// MCX_READS_BAM: taken records count in twos for the parser's following calls (sticky, like the rule)
extern "C" int mcx_fastq_parser_set_mates(mcx_fastq_parser *p, int mates)
{
    if (!p || (mates != 0 && mates != 1)) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_parser_set_mates: null parser, or a switch that is neither 0 nor 1");
    p->mates = mates;
    return 0;
}

// MCX_READS_BAM: the last call's records walked, taken, skipped for 0x900, the first taken record's flag, chunks, chunks whose searched start was off the chain
extern "C" int mcx_bam_reads_last(mcx_fastq_parser *p, uint64_t stats[6])
{
    if (!p || !stats) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_reads_last: null argument");
    mcx_bam_in_last(p->bam, stats, nullptr);
    return 0;
}

// ... and its search, walk, join and unpack on the device in ms, by events on the parser's stream (scripts/bam_in_rate.py)
extern "C" int mcx_bam_reads_last_ms(mcx_fastq_parser *p, float ms[4])
{
    if (!p || !ms) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_reads_last_ms: null argument");
    mcx_bam_in_last(p->bam, nullptr, ms);
    return 0;
}

// mcx_fastq_parse_dev in its two halves, for a caller inside the library that sizes its buffers between them (the resident route, mcx_resident.hip): sizes
// parses and fills *info; out writes the groups of `out` (device pointers) for the texts of the last sizes — a group whose capacity is too small is refused
int mcx_fastq_dev_sizes(mcx_fastq_parser *p, const mcx_fastq_in *in, mcx_fastq_info *info)
{
    HIP_TRY(hipSetDevice(p->device));
    return sizes_pass(p, in, info, "mcx_fastq_parse_dev");
}
int mcx_fastq_dev_out(mcx_fastq_parser *p, const mcx_fastq_out *out, const mcx_fastq_info *info)
{
    if (const char *why = rows_fault(out, p->job.max_read_len)) return mcx_set_error(MCX_ERR_ARG, std::string("mcx_fastq_parse_dev: ") + why);
    if (out->bases && (((uintptr_t)out->bases & 15u) || (out->qual && ((uintptr_t)out->qual & 15u)))) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_parse_dev: bases and qual are 16-byte aligned");
    HIP_TRY(hipSetDevice(p->device));
    return output_pass(p, out, info, "mcx_fastq_parse_dev");
}

// the last mcx_fastq_parse_dev on the device in ms, first kernel to last, by events on the parser's stream (scripts/fastq_rate.py)
extern "C" int mcx_fastq_last_ms(mcx_fastq_parser *p, float *ms)
{
    if (!p || !ms) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_last_ms: null argument");
    *ms = p->last_ms;
    return 0;
}

// how often one of the parser's buffers had to be replaced by a larger one
extern "C" int mcx_fastq_grown(mcx_fastq_parser *p, uint32_t *n)
{
    if (!p || !n) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_grown: null argument");
    *n = p->grown + mcx_bam_in_grown(p->bam);
    return 0;
}

// ---- the host form, in three steps that the file front end takes one by one ---------------------------------------------
// stage: page-locked staging for two texts of these sizes and its twin in HBM (the second text begins at a multiple of 16): the caller fills h[0], h[1].
int mcx_fastq_stage(mcx_fastq_parser *p, const uint64_t bytes[2], uint8_t *h[2])
{
    if (bytes[0] >= (1ull << 32) || bytes[1] >= (1ull << 32)) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq: a text holds less than 4 GiB");
    const uint64_t at1 = (bytes[0] + 15) & ~15ull, need = at1 + bytes[1] + 16;
    HIP_TRY(hipSetDevice(p->device));
    if (need > p->h_text_cap) {
        (void)hipStreamSynchronize(p->stream);
        mcx_pinned_free(p->h_text);
        p->h_text_cap = 0;
        const size_t cap = need + need / 8;
        if (!(p->h_text = (uint8_t *)mcx_pinned_alloc(cap))) return mcx_set_error(MCX_ERR_DEVICE, "mcx_fastq: no page-locked memory for " + std::to_string(cap) + " bytes of text");
        p->h_text_cap = cap;
    }
    if (int rc = grow(p, p->d_text, need, "the text")) return rc;
    h[0] = p->h_text; h[1] = p->h_text + at1;
    return 0;
}

// sizes: the staged texts go to HBM and through the sizes pass — *info holds everything but the outputs.  two: the second text counts even when it is empty.
int mcx_fastq_staged_sizes(mcx_fastq_parser *p, const uint64_t bytes[2], int two, uint32_t max_records, int32_t max_read_len, int32_t final, mcx_fastq_info *info)
{
    const uint64_t at1 = (bytes[0] + 15) & ~15ull;
    HIP_TRY(hipSetDevice(p->device));
    uint8_t *d_text = (uint8_t *)p->d_text.p;
    const uint64_t up = two ? at1 + bytes[1] : bytes[0];
    if (up) HIP_TRY(hipMemcpyAsync(d_text, p->h_text, up, hipMemcpyHostToDevice, p->stream));
    mcx_fastq_in in;
    memset(&in, 0, sizeof in);
    in.text[0] = d_text; in.bytes[0] = bytes[0];
    if (two) { in.text[1] = d_text + at1; in.bytes[1] = bytes[1]; }
    in.max_records = max_records; in.max_read_len = max_read_len; in.final = final; in.n_ref = p->host_n_ref;
    return sizes_pass(p, &in, info, "mcx_fastq_parse");
}

// out: the groups of `out` — HOST pointers; page-locked ones make the copies back asynchronous — for the texts of the last staged_sizes, through buffers in
// HBM of the results' sizes.  row_words 0 with rows: the rows are as wide as the longest read needs, ceil(info->longest / 16) words.
int mcx_fastq_staged_out(mcx_fastq_parser *p, const mcx_fastq_out *out, const mcx_fastq_info *info)
{
    HIP_TRY(hipSetDevice(p->device));
    const uint32_t n = info->n_reads, nt = p->job.nt;
    mcx_fastq_out o;
    memset(&o, 0, sizeof o);
    int rc = 0;
    for (uint32_t t = 0; t < nt; t++)
        if (out->recs[t]) { if ((rc = grow(p, p->o_recs[t], (size_t)info->n_records[t] * sizeof(mcx_fastq_rec) + 16, "the records"))) return rc; o.recs[t] = (mcx_fastq_rec *)p->o_recs[t].p; }
    // (a group whose capacity is too small goes to the output pass with that capacity and is refused there: nothing of it is written or copied back)
    if (out->bases) {
        o.bases_cap = out->bases_cap < info->n_bases + 32 ? out->bases_cap : info->n_bases + 32;
        if ((rc = grow(p, p->o_bases, info->n_bases + 32, "the bases")) || (rc = grow(p, p->o_off, ((size_t)n + 1) * 4, "the offsets"))) return rc;
        if (out->qual && (rc = grow(p, p->o_qual, info->n_bases + 32, "the qualities"))) return rc;
        o.bases = (uint8_t *)p->o_bases.p; o.off = (uint32_t *)p->o_off.p; o.qual = out->qual ? (uint8_t *)p->o_qual.p : nullptr;
    }
    if (out->names) {
        o.names_cap = out->names_cap < info->n_name_bytes ? out->names_cap : info->n_name_bytes;
        if ((rc = grow(p, p->o_names, info->n_name_bytes + 16, "the names")) || (rc = grow(p, p->o_noff, ((size_t)n + 1) * 4, "the names' offsets"))) return rc;
        o.names = (uint8_t *)p->o_names.p; o.name_off = (uint32_t *)p->o_noff.p;
    }
    if (out->rows) {
        o.row_words = out->row_words ? out->row_words : (info->longest + 15) / 16;
        o.odd_cap = out->odd_cap < info->n_odd ? out->odd_cap : info->n_odd;
        if ((rc = grow(p, p->o_rows, (size_t)n * o.row_words * 4 + 16, "the rows")) || (rc = grow(p, p->o_len, (size_t)n * 4 + 16, "the lengths")) || (rc = grow(p, p->o_odd, (size_t)info->n_odd * 8 + 16, "the odd bytes"))) return rc;
        o.rows = (uint32_t *)p->o_rows.p; o.len = (uint32_t *)p->o_len.p; o.odd = (uint64_t *)p->o_odd.p;
    }
    const int cap_rc = output_pass(p, &o, info, "mcx_fastq_parse");
    if (cap_rc && cap_rc != MCX_ERR_CAPACITY) return cap_rc;
    hipStream_t s = p->stream;
    for (uint32_t t = 0; t < nt; t++)
        if (o.recs[t] && info->n_records[t]) HIP_TRY(hipMemcpyAsync(out->recs[t], o.recs[t], (size_t)info->n_records[t] * sizeof(mcx_fastq_rec), hipMemcpyDeviceToHost, s));
    if (o.bases && o.bases_cap >= info->n_bases + 32) {
        if (info->n_bases) HIP_TRY(hipMemcpyAsync(out->bases, o.bases, info->n_bases, hipMemcpyDeviceToHost, s));
        if (o.qual && info->n_bases) HIP_TRY(hipMemcpyAsync(out->qual, o.qual, info->n_bases, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(out->off, o.off, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, s));
    }
    if (o.names && o.names_cap >= info->n_name_bytes) {
        if (info->n_name_bytes) HIP_TRY(hipMemcpyAsync(out->names, o.names, info->n_name_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(out->name_off, o.name_off, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, s));
    }
    if (o.rows && o.odd_cap >= info->n_odd && n) {
        if (o.row_words) HIP_TRY(hipMemcpyAsync(out->rows, o.rows, (size_t)n * o.row_words * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(out->len, o.len, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        if (info->n_odd) HIP_TRY(hipMemcpyAsync(out->odd, o.odd, (size_t)info->n_odd * 8, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return cap_rc;
}

extern "C" int mcx_fastq_parse(mcx_fastq_parser *p, const mcx_fastq_in *in, const mcx_fastq_out *out, mcx_fastq_info *info)
{
    if (!p || !in || !out || !info) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_parse: null argument");
    memset(info, 0, sizeof *info);
    const int two = in->text[1] != nullptr;
    for (int t = 0; t < (two ? 2 : 1); t++) if (!in->text[t] && in->bytes[t]) return mcx_set_error(MCX_ERR_ARG, "mcx_fastq_parse: null text");
    if (const char *why = rows_fault(out, in->max_read_len)) return mcx_set_error(MCX_ERR_ARG, std::string("mcx_fastq_parse: ") + why);
    const uint64_t bytes[2] = {in->bytes[0], two ? in->bytes[1] : 0};
    uint8_t *h[2];
    if (int rc = mcx_fastq_stage(p, bytes, h)) return rc;
    for (int t = 0; t < (two ? 2 : 1); t++) if (bytes[t]) memcpy(h[t], in->text[t], bytes[t]);
    p->host_n_ref = in->n_ref;
    if (int rc = mcx_fastq_staged_sizes(p, bytes, two, in->max_records, in->max_read_len, in->final, info)) return rc;
    return mcx_fastq_staged_out(p, out, info);
}
