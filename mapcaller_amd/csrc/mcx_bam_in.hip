// mapcaller_amd/csrc/mcx_bam_in.hip — BAM records as read input, found and unpacked on the device: the third format of mcx_fastq_parser (MCX_READS_BAM; reached
// from mcx_fastq.hip's sizes and output passes), and mcx_bam_reads_header.  The rules are mcx_bam_in.h's.
//
// A BAM stream has no newlines to find records by: a record's start is known only from the block_size of the one before.  Per call, on the parser's stream, with
// the text cut into chunks of 64 KB (MCX_BAM_CHUNK):
//   k_search    a wavefront per chunk: the first offset in the chunk where rule P holds, and holds again for the two records that follow inside the text — a lane
//               per candidate, 64 at a time, a ballot; chunk 0 starts at 0 by definition.  A guess: no result depends on it
//   k_walk      a wavefront per chunk follows the chain from that start to the first offset at or beyond the chunk's end: where it ended, the records it passed
//               and took, and what stopped it.  A chain of dependent loads, about 200 a chunk: the parallelism is the number of chunks, so every lane of the
//               wavefront computes the same walk (one fetch per load) and lane 0 writes
//   k_join      one wavefront takes the chunks in order, 64 chunks' results a load, handed from lane to lane in registers: a chunk is on the chain when the walk
//               before it ended exactly on its start; where it did not — a false start, none found, a record longer than a chunk — the chunk is walked again from
//               where the chain really arrives (or holds no start at all).  Behind the chain's stop no chunk counts.  No host round trip
//   (hipCUB)    exclusive sum of the chunks' taken counts
//   k_list      the walk once more, from the chain's real start in every chunk: the offsets and flags of the taken records, in order
//   k_recs      a lane per taken record (mates: per two): name, lengths and offsets by the rules, why the text's records end at it; the first such stop is the
//               minimum of the lanes' keys (hipCUB) — no atomics anywhere in this file
//   k_finish    records taken, why no more, bytes consumed; k_lens, k_odd<false>, three exclusive sums, the longest read (hipCUB): as mcx_fastq.hip
// the host then reads the totals (the one wait), judges the caller's capacities, and queues
//   k_gather    a wavefront per read: letters from the nibbles, qualities, names — neighbouring lanes on neighbouring bytes, neighbouring wavefronts on
//               neighbouring records; only the groups asked for
//   k_rows      a lane per word of a row, straight from the nibbles (no letters in HBM); k_odd<true> a wavefront per read writes its odd bytes in position order
// Reversed reads (flag 0x10) are read back to front and complemented by bit reversal in the same kernels.
// Every load lies inside text[0 .. bytes): record_at reads a field only behind a bounds check, and the kernels behind it read only inside records it accepted.
// Every loop is bounded by the text's, a chunk's or a record's length; no kernel waits for another workgroup.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/mcx.h"
#include "mcx_bam_in.h"
#include "mcx_fastq.h"
#include "mcx_internal.h"

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace {

using namespace mcx::bamin;

enum : uint32_t { kThreads = 256, kWaves = kThreads / 64, kNone = 0xFFFFFFFFu, kChunkDefault = 65536, kChunkLeast = 256 };
const unsigned long long kNoKey = ~0ull;

struct Job { // one call, as the kernels see it
    const uint8_t *text;
    uint32_t bytes;
    int32_t n_ref, max_read_len, final, mates;
    uint32_t chunk, n_chunks;
    uint32_t cap;              // max_records; under mates its even part
    uint32_t eff;              // min(cap, bytes / 37 + 1): a taken record holds 37 bytes at least
    uint32_t *c_start, *c_end, *c_walked, *c_taken, *c_code, *c_base; // [n_chunks] each
    uint32_t *toff, *tflag;    // [max(eff, 1)] where the taken records begin, their flags
    mcx_fastq_rec *recs;       // [max(eff, 1)]
    unsigned long long *keys;  // [units] (record that ends the text << 8 | why), kNoKey where none does
};
struct DevInfo { // what the kernels tell the host
    uint32_t chain_code, chain_pos, off_chain, first_flag; // how and where the chain of the whole text stops; chunks whose searched start was not on it
    unsigned long long walked, taken;                       // records of the chain, and those with flag & 0x900 == 0
    unsigned long long min_key;
    uint32_t longest, pad;
    mcx_fastq_info info;
};

struct Walk { uint32_t end, walked, taken, code; };

// The chain from `from` to the first offset at or beyond `upto`, or to what stops it.  kList: taken record base + i goes to toff / tflag when it is below lim.
// Every lane of the wavefront runs it with the same arguments; `writer` (one lane) stores.
template <bool kList>
__device__ __forceinline__ Walk walk(const Job &j, uint64_t from, uint64_t upto, uint32_t base, uint32_t lim, bool writer)
{
    Walk w = {0, 0, 0, kOk};
    uint64_t o = from;
    while (o < upto) { // (each step is 36 bytes at least: at most chunk / 36 + 1 steps, and one record that reaches past the chunk)
        Fixed r;
        const uint32_t st = record_at(j.text, j.bytes, o, j.n_ref, r);
        if (st != kOk) { w.code = st; break; }
        w.walked++;
        if (taken(r)) {
            if (kList && writer && base + w.taken < lim) { j.toff[base + w.taken] = (uint32_t)o; j.tflag[base + w.taken] = r.flag; }
            w.taken++;
        }
        o = next_of(o, r); // (<= bytes: the record lies inside the text)
    }
    w.end = (uint32_t)o;
    return w;
}

// rule P at o, and again for the two records that follow inside the text
__device__ __forceinline__ bool start_ok(const Job &j, uint64_t o)
{
    Fixed r;
    if (record_at(j.text, j.bytes, o, j.n_ref, r) != kOk) return false;
    for (int k = 0; k < 2; k++) {
        o = next_of(o, r);
        const uint32_t st = record_at(j.text, j.bytes, o, j.n_ref, r);
        if (st == kBad) return false;
        if (st != kOk) return true; // the text's end, or a record that runs past it: nothing more to hold it against
    }
    return true;
}

__global__ void k_init(DevInfo *d)
{
    if (threadIdx.x || blockIdx.x) return;
    *d = DevInfo{};
    d->min_key = kNoKey;
}

__global__ void __launch_bounds__(kThreads) k_search(Job j)
{
    const uint64_t c = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (c >= j.n_chunks) return; // (the whole wavefront)
    uint32_t found = c == 0 ? 0u : kNone;
    if (c) {
        const uint64_t lo = c * j.chunk, hi = lo + j.chunk < j.bytes ? lo + j.chunk : j.bytes;
        for (uint64_t o0 = lo; o0 < hi; o0 += 64) {
            const uint64_t o = o0 + lane;
            const unsigned long long m = __ballot(o < hi && start_ok(j, o));
            if (m) { found = (uint32_t)(o0 + (uint32_t)__ffsll((long long)m) - 1u); break; }
        }
    }
    if (lane == 0) j.c_start[c] = found;
}

__global__ void __launch_bounds__(kThreads) k_walk(Job j)
{
    const uint64_t c = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (c >= j.n_chunks) return;
    const uint32_t from = j.c_start[c];
    Walk w = {0, 0, 0, kOk};
    if (from != kNone) w = walk<false>(j, from, (c + 1) * j.chunk, 0, 0, false);
    if ((threadIdx.x & 63u) == 0) { j.c_end[c] = w.end; j.c_walked[c] = w.walked; j.c_taken[c] = w.taken; j.c_code[c] = w.code; }
}

// one wavefront: c_start becomes where the chain really enters each chunk (kNone: nowhere), c_walked / c_taken what it passes and takes there
__global__ void __launch_bounds__(64) k_join(Job j, DevInfo *d)
{
    const uint32_t lane = threadIdx.x;
    uint32_t a = 0, code = kOk, off_chain = 0; // where the chain arrives, what has stopped it: the same in every lane
    unsigned long long walked = 0, n_taken = 0;
    for (uint32_t c0 = 0; c0 < j.n_chunks; c0 += 64) {
        const uint32_t c = c0 + lane;
        const bool in = c < j.n_chunks;
        uint32_t st = in ? j.c_start[c] : kNone, en = in ? j.c_end[c] : 0u, wk = in ? j.c_walked[c] : 0u, tk = in ? j.c_taken[c] : 0u, cd = in ? j.c_code[c] : (uint32_t)kOk;
        const uint32_t m = j.n_chunks - c0 < 64u ? j.n_chunks - c0 : 64u;
        for (uint32_t i = 0; i < m; i++) {
            const uint64_t hi = ((uint64_t)c0 + i + 1) * j.chunk;
            const uint32_t s_i = __shfl(st, (int)i);
            uint32_t e_i = __shfl(en, (int)i), w_i = __shfl(wk, (int)i), t_i = __shfl(tk, (int)i), cd_i = __shfl(cd, (int)i);
            const uint32_t real = code != kOk || a >= hi ? (uint32_t)kNone : a; // (a >= hi: a record longer than a chunk — this one holds no start)
            if (code == kOk && s_i != real) off_chain++;
            if (real == kNone) w_i = t_i = 0;
            else {
                if (s_i != real) { const Walk w = walk<false>(j, real, hi, 0, 0, false); e_i = w.end; w_i = w.walked; t_i = w.taken; cd_i = w.code; }
                a = e_i; code = cd_i; walked += w_i; n_taken += t_i;
            }
            if (lane == i) { st = real; wk = w_i; tk = t_i; }
        }
        if (in) { j.c_start[c] = st; j.c_walked[c] = wk; j.c_taken[c] = tk; }
    }
    if (code == kOk) code = kEnd; // (the chain left the last chunk exactly on the text's end)
    if (lane == 0) { d->chain_code = code; d->chain_pos = a; d->off_chain = off_chain; d->walked = walked; d->taken = n_taken; }
}

__global__ void __launch_bounds__(kThreads) k_list(Job j)
{
    const uint64_t c = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (c >= j.n_chunks) return;
    const uint32_t from = j.c_start[c];
    if (from == kNone || j.c_taken[c] == 0) return;
    (void)walk<true>(j, from, (c + 1) * j.chunk, j.c_base[c], j.eff ? j.eff : 1u, (threadIdx.x & 63u) == 0);
}

// taken records (mates: pairs) that count: below the cap and inside the chain
__device__ __forceinline__ uint32_t n_counted(const Job &j, const DevInfo *d)
{
    const uint32_t n = (uint32_t)(d->taken < j.cap ? d->taken : j.cap);
    return j.mates ? n & ~1u : n;
}

__global__ void __launch_bounds__(kThreads) k_recs(Job j, const DevInfo *d, uint32_t units)
{
    const uint64_t u = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (u >= units) return;
    const uint32_t per = j.mates ? 2u : 1u, k = (uint32_t)u * per;
    unsigned long long key = kNoKey;
    if (k + per <= n_counted(j, d)) {
        mcx_fastq_rec rec[2];
        uint32_t flag[2] = {0, 0}, why = MCX_FASTQ_MORE;
        for (uint32_t i = 0; i < per && why == MCX_FASTQ_MORE; i++) {
            Fixed r;
            const uint64_t o = j.toff[k + i];
            (void)record_at(j.text, j.bytes, o, j.n_ref, r); // (kOk: the walk took it)
            flag[i] = r.flag;
            why = rec_of(j.text, o, r, j.max_read_len, rec[i]);
        }
        if (why == MCX_FASTQ_MORE && j.mates && !mates_ok(j.text, rec[0], flag[0], rec[1], flag[1])) why = MCX_FASTQ_UNPAIRED;
        if (why == MCX_FASTQ_MORE) for (uint32_t i = 0; i < per; i++) j.recs[k + i] = rec[i];
        else key = ((unsigned long long)k << 8) | why;
    }
    j.keys[u] = key;
}

__global__ void k_finish(Job j, DevInfo *d)
{
    if (threadIdx.x || blockIdx.x) return;
    mcx_fastq_info &f = d->info;
    const unsigned long long T = d->taken, key = d->min_key;
    uint32_t n, stop;
    uint64_t consumed;
    if (key != kNoKey) { n = (uint32_t)(key >> 8); stop = (uint32_t)(key & 0xFFu); consumed = j.toff[n]; } // a record (a pair) that ends the text: the skipped ones before it are consumed
    else if (T >= j.cap) { // max_records taken
        n = j.cap; stop = MCX_FASTQ_MORE; consumed = 0;
        if (n) { const uint64_t o = j.toff[n - 1]; consumed = o + 4 + rd32(j.text + o); }
    } else {
        const uint32_t code = d->chain_code;
        const uint32_t why = code == kEnd ? (uint32_t)MCX_FASTQ_END : code == kPast && !j.final ? (uint32_t)MCX_FASTQ_MORE : (uint32_t)MCX_FASTQ_DAMAGED;
        if (j.mates && (T & 1)) { n = (uint32_t)T - 1; consumed = j.toff[n]; stop = code == kEnd ? (j.final ? (uint32_t)MCX_FASTQ_UNPAIRED : (uint32_t)MCX_FASTQ_MORE) : why; } // a single record at the end
        else { n = (uint32_t)T; consumed = d->chain_pos; stop = why; }
    }
    f.n_records[0] = n; f.stop[0] = stop; f.consumed[0] = consumed; f.n_reads = n;
    d->first_flag = T ? j.tflag[0] : 0u;
}

// rl, nl [eff + 1]: rlen and name_len of read r, 0 from n_reads on
__global__ void __launch_bounds__(kThreads) k_lens(Job j, const DevInfo *d, uint32_t *rl, uint32_t *nl)
{
    const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r > j.eff) return;
    const bool is = r < d->info.n_reads;
    rl[r] = is ? j.recs[r].rlen : 0u; nl[r] = is ? j.recs[r].name_len : 0u;
}

// A wavefront per read.  kWrite false: oc[r] = the read's bases that are not A, C, G, T (0 from n_reads on, oc [eff + 1]); true: their entries in position order
// at odd[ooff[r] ..), the letter as the byte.  Neighbouring lanes read neighbouring nibbles.
template <bool kWrite>
__global__ void __launch_bounds__(kThreads) k_odd(Job j, const DevInfo *d, uint32_t *oc, const uint32_t *ooff, uint64_t *odd)
{
    const uint64_t r64 = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (r64 > j.eff) return; // (the whole wavefront)
    uint32_t n = 0;
    if (r64 < d->info.n_reads) {
        const uint32_t r = (uint32_t)r64;
        const mcx_fastq_rec c = j.recs[r];
        const bool rev = (j.tflag[r] & 0x10u) != 0;
        const uint8_t *seq = j.text + c.seq;
        for (uint32_t i0 = 0; i0 < c.rlen; i0 += 64) {
            const uint32_t i = i0 + lane;
            const uint32_t nb = i < c.rlen ? nibble_of(seq, c.rlen, rev, i) : 1u;
            const bool is = odd_nibble(nb);
            const unsigned long long m = __ballot(is);
            if (kWrite && is) odd[(uint64_t)ooff[r] + n + __popcll(m & ((1ull << lane) - 1ull))] = mcx::fq::odd_entry(r, i, letter_of(nb));
            n += (uint32_t)__popcll(m);
        }
    }
    if (!kWrite && lane == 0) oc[r64] = n;
}

__global__ void k_totals(Job j, DevInfo *d, const uint32_t *off, const uint32_t *noff, const uint32_t *ooff)
{
    if (threadIdx.x || blockIdx.x) return;
    d->info.n_bases = off[j.eff]; d->info.n_name_bytes = noff[j.eff]; d->info.n_odd = ooff[j.eff]; d->info.longest = d->longest;
}

// a wavefront per read: its letters, its quality bytes (NULs where the record has none), its name; a null destination is skipped
__global__ void __launch_bounds__(kThreads) k_gather(Job j, uint32_t n_reads, const uint32_t *off, const uint32_t *noff, uint8_t *bases, uint8_t *qual, uint8_t *names)
{
    const uint64_t r = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (r >= n_reads) return;
    const mcx_fastq_rec c = j.recs[r];
    const bool rev = (j.tflag[r] & 0x10u) != 0;
    if (bases) {
        uint8_t *b = bases + off[r];
        const uint8_t *seq = j.text + c.seq;
        for (uint32_t i = lane; i < c.rlen; i += 64) b[i] = letter_of(nibble_of(seq, c.rlen, rev, i));
        if (qual) {
            uint8_t *q = qual + off[r];
            const uint8_t *src = j.text + c.qual;
            for (uint32_t i = lane; i < c.rlen; i += 64) q[i] = c.q_take ? qual_of(src, c.rlen, rev, i) : (uint8_t)0;
        }
    }
    if (names) {
        uint8_t *nm = names + noff[r];
        for (uint32_t i = lane; i < c.name_len; i += 64) nm[i] = j.text[c.name + i];
    }
}

// one lane per word of the rows: sixteen nibbles — eight bytes of the record, neighbouring lanes on neighbouring bytes — to sixteen 2-bit codes
__global__ void __launch_bounds__(kThreads) k_rows(Job j, uint32_t n_reads, uint32_t row_words, uint32_t *rows, uint32_t *len)
{
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= (uint64_t)n_reads * row_words) return;
    const uint32_t r = (uint32_t)(g / row_words), w = (uint32_t)(g % row_words);
    const mcx_fastq_rec c = j.recs[r];
    const uint64_t i = 16ull * w;
    uint32_t word = 0;
    if (i < c.rlen) word = row_word(j.text + c.seq, c.rlen, (j.tflag[r] & 0x10u) != 0, (uint32_t)i, c.rlen - (uint32_t)i < 16u ? c.rlen - (uint32_t)i : 16u);
    rows[g] = word;
    if (w == 0) len[r] = c.rlen;
}

struct Buf { void *p = nullptr; size_t cap = 0; };

uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

} // namespace

struct mcx_bam_in {
    Buf c_start, c_end, c_walked, c_taken, c_code, c_base, toff, tflag, recs, keys, rl, nl, oc, off, noff, ooff, tmp, info;
    DevInfo *h_info = nullptr; // page-locked
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float ms[4] = {0, 0, 0, 0};
    uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
    uint32_t grown = 0;
    Job job;
};

namespace {

int grow(mcx_bam_in *b, hipStream_t s, Buf &x, size_t need, const char *what)
{
    if (need <= x.cap) return 0;
    if (x.p) { (void)hipStreamSynchronize(s); (void)hipFree(x.p); b->grown++; }
    x.p = nullptr; x.cap = 0;
    const size_t cap = need + need / 8 + 256;
    if (hipMalloc(&x.p, cap) != hipSuccess) { (void)hipGetLastError(); x.p = nullptr; return mcx_set_error(MCX_ERR_DEVICE, std::string("mcx_bam_in: no room in HBM for ") + what + " (" + std::to_string(cap) + " bytes)"); }
    x.cap = cap;
    return 0;
}

int create(mcx_bam_in **out)
{
    mcx_bam_in *b = new mcx_bam_in();
    bool ok = (b->h_info = (DevInfo *)mcx_pinned_alloc(sizeof(DevInfo))) != nullptr;
    for (hipEvent_t &e : b->ev) if (ok && hipEventCreate(&e) != hipSuccess) ok = false;
    if (!ok) { (void)hipGetLastError(); mcx_bam_in_free(b); return mcx_set_error(MCX_ERR_DEVICE, "mcx_bam_in: no events or page-locked memory"); }
    *out = b;
    return 0;
}

uint32_t chunk_bytes()
{
    const char *env = getenv("MCX_BAM_CHUNK"); // a debug override: no result depends on it
    const long long v = env ? atoll(env) : 0;
    return v > 0 ? (uint32_t)std::min<long long>(std::max<long long>(v, kChunkLeast), 1ll << 30) : (uint32_t)kChunkDefault;
}

} // namespace

void mcx_bam_in_free(mcx_bam_in *b)
{
    if (!b) return;
    Buf *all[] = {&b->c_start, &b->c_end, &b->c_walked, &b->c_taken, &b->c_code, &b->c_base, &b->toff, &b->tflag, &b->recs, &b->keys, &b->rl, &b->nl, &b->oc, &b->off, &b->noff, &b->ooff, &b->tmp, &b->info};
    for (Buf *x : all) if (x->p) (void)hipFree(x->p);
    mcx_pinned_free(b->h_info);
    for (hipEvent_t e : b->ev) if (e) (void)hipEventDestroy(e);
    delete b;
}

// Everything up to the one wait: the chain, the taken records, the reads' lengths and offsets in the state's scratch, the totals in *info.
int mcx_bam_in_sizes(mcx_bam_in **state, void *stream, const mcx_fastq_in *in, int mates, mcx_fastq_info *info, const char *who)
{
    memset(info, 0, sizeof *info);
    if (in->text[1]) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": BAM records come as one text (pairs are two records of it)");
    if (!in->text[0] && in->bytes[0]) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": null text");
    if (in->bytes[0] >= (1ull << 32)) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": a text holds less than 4 GiB");
    if (!*state) if (int rc = create(state)) return rc;
    mcx_bam_in *b = *state;
    hipStream_t s = (hipStream_t)stream;
    Job &j = b->job;
    memset(&j, 0, sizeof j);
    j.text = in->text[0]; j.bytes = (uint32_t)in->bytes[0];
    j.n_ref = in->n_ref; j.max_read_len = in->max_read_len; j.final = in->final; j.mates = mates ? 1 : 0;
    j.chunk = chunk_bytes();
    j.n_chunks = std::max<uint32_t>(1, (uint32_t)(((uint64_t)j.bytes + j.chunk - 1) / j.chunk));
    j.cap = mates ? in->max_records & ~1u : in->max_records;
    j.eff = (uint32_t)std::min<uint64_t>(j.cap, (uint64_t)j.bytes / 37 + 1);
    if ((uint64_t)j.eff + 1 > 0x7FFFFFFFull) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": max_records is too large");
    const uint64_t n_rec = std::max<uint32_t>(j.eff, 1), per_read = (uint64_t)j.eff + 1;
    const uint32_t units = (uint32_t)std::max<uint64_t>(1, j.mates ? j.eff / 2 : j.eff);
    int rc = 0;
    Buf *per_chunk[] = {&b->c_start, &b->c_end, &b->c_walked, &b->c_taken, &b->c_code, &b->c_base};
    for (Buf *x : per_chunk) if ((rc = grow(b, s, *x, (size_t)j.n_chunks * 4, "the chunks' tables"))) return rc;
    if ((rc = grow(b, s, b->toff, n_rec * 4, "the records' offsets")) || (rc = grow(b, s, b->tflag, n_rec * 4, "the records' flags")) ||
        (rc = grow(b, s, b->recs, n_rec * sizeof(mcx_fastq_rec), "the records")) || (rc = grow(b, s, b->keys, (size_t)units * 8, "the records' stops")) ||
        (rc = grow(b, s, b->info, sizeof(DevInfo), "the call's results"))) return rc;
    Buf *reads[] = {&b->rl, &b->nl, &b->oc, &b->off, &b->noff, &b->ooff};
    for (Buf *x : reads) if ((rc = grow(b, s, *x, per_read * 4, "the reads' lengths and offsets"))) return rc;
    size_t need = 0, need2 = 0, need3 = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)std::max<uint64_t>(per_read, j.n_chunks), s));
    HIP_TRY(hipcub::DeviceReduce::Min(nullptr, need2, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)units, s));
    HIP_TRY(hipcub::DeviceReduce::Max(nullptr, need3, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)per_read, s));
    if ((rc = grow(b, s, b->tmp, std::max(need, std::max(need2, need3)) + 16, "the sums' scratch"))) return rc;
    j.c_start = (uint32_t *)b->c_start.p; j.c_end = (uint32_t *)b->c_end.p; j.c_walked = (uint32_t *)b->c_walked.p; j.c_taken = (uint32_t *)b->c_taken.p;
    j.c_code = (uint32_t *)b->c_code.p; j.c_base = (uint32_t *)b->c_base.p;
    j.toff = (uint32_t *)b->toff.p; j.tflag = (uint32_t *)b->tflag.p; j.recs = (mcx_fastq_rec *)b->recs.p; j.keys = (unsigned long long *)b->keys.p;
    DevInfo *d = (DevInfo *)b->info.p;
    uint32_t *rl = (uint32_t *)b->rl.p, *nl = (uint32_t *)b->nl.p, *oc = (uint32_t *)b->oc.p, *off = (uint32_t *)b->off.p, *noff = (uint32_t *)b->noff.p, *ooff = (uint32_t *)b->ooff.p;
    size_t tmp = b->tmp.cap;
    const uint32_t chunk_grid = blocks_for(j.n_chunks, kWaves);

    HIP_TRY(hipEventRecord(b->ev[0], s));
    k_init<<<1, 64, 0, s>>>(d);
    k_search<<<chunk_grid, kThreads, 0, s>>>(j);
    HIP_TRY(hipEventRecord(b->ev[1], s));
    k_walk<<<chunk_grid, kThreads, 0, s>>>(j);
    HIP_TRY(hipEventRecord(b->ev[2], s));
    k_join<<<1, 64, 0, s>>>(j, d);
    HIP_TRY(hipEventRecord(b->ev[3], s));
    HIP_TRY(hipGetLastError());
    tmp = b->tmp.cap;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b->tmp.p, tmp, j.c_taken, j.c_base, (int)j.n_chunks, s));
    k_list<<<chunk_grid, kThreads, 0, s>>>(j);
    k_recs<<<blocks_for(units, kThreads), kThreads, 0, s>>>(j, d, units);
    HIP_TRY(hipGetLastError());
    tmp = b->tmp.cap;
    HIP_TRY(hipcub::DeviceReduce::Min(b->tmp.p, tmp, j.keys, &d->min_key, (int)units, s));
    k_finish<<<1, 64, 0, s>>>(j, d);
    k_lens<<<blocks_for(per_read, kThreads), kThreads, 0, s>>>(j, d, rl, nl);
    k_odd<false><<<blocks_for(per_read, kWaves), kThreads, 0, s>>>(j, d, oc, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    tmp = b->tmp.cap;
    HIP_TRY(hipcub::DeviceReduce::Max(b->tmp.p, tmp, rl, &d->longest, (int)per_read, s));
    tmp = b->tmp.cap;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b->tmp.p, tmp, rl, off, (int)per_read, s));
    tmp = b->tmp.cap;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b->tmp.p, tmp, nl, noff, (int)per_read, s));
    tmp = b->tmp.cap;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(b->tmp.p, tmp, oc, ooff, (int)per_read, s));
    k_totals<<<1, 64, 0, s>>>(j, d, off, noff, ooff);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev[4], s));
    HIP_TRY(hipMemcpyAsync(b->h_info, d, sizeof(DevInfo), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s)); // the one wait in the middle: the host judges the capacities
    *info = b->h_info->info;
    const DevInfo &h = *b->h_info;
    b->stats[0] = h.walked; b->stats[1] = h.taken; b->stats[2] = h.walked - h.taken; b->stats[3] = h.first_flag; b->stats[4] = j.n_chunks; b->stats[5] = h.off_chain;
    for (int i = 0; i < 3; i++) HIP_TRY(hipEventElapsedTime(&b->ms[i], b->ev[i], b->ev[i + 1]));
    HIP_TRY(hipEventElapsedTime(&b->ms[3], b->ev[3], b->ev[4]));
    return 0;
}

// The groups of `out` (device pointers) from the scratch of the sizes pass; a group whose capacity is too small is left alone and the call says so.
int mcx_bam_in_out(mcx_bam_in *b, void *stream, const mcx_fastq_out *out, const mcx_fastq_info *info, const char *who)
{
    const Job &j = b->job;
    const uint32_t n = info->n_reads;
    const uint32_t *off = (const uint32_t *)b->off.p, *noff = (const uint32_t *)b->noff.p, *ooff = (const uint32_t *)b->ooff.p;
    hipStream_t s = (hipStream_t)stream;
    int rc = 0;
    const bool want_bases = out->bases != nullptr, want_names = out->names != nullptr, want_rows = out->rows != nullptr;
    const bool do_bases = want_bases && out->bases_cap >= info->n_bases + 32, do_names = want_names && out->names_cap >= info->n_name_bytes, do_rows = want_rows && out->odd_cap >= info->n_odd;
    if (want_bases && !do_bases) rc = mcx_set_error(MCX_ERR_CAPACITY, std::string(who) + ": bases_cap is less than the " + std::to_string(info->n_bases) + " bases + 32");
    if (want_names && !do_names) rc = mcx_set_error(MCX_ERR_CAPACITY, std::string(who) + ": names_cap is less than the " + std::to_string(info->n_name_bytes) + " bytes of the names");
    if (want_rows && !do_rows) rc = mcx_set_error(MCX_ERR_CAPACITY, std::string(who) + ": odd_cap is less than the " + std::to_string(info->n_odd) + " bytes that are not ACGT");
    HIP_TRY(hipEventRecord(b->ev[5], s));
    if (out->recs[0] && info->n_records[0]) HIP_TRY(hipMemcpyAsync(out->recs[0], j.recs, (size_t)info->n_records[0] * sizeof(mcx_fastq_rec), hipMemcpyDeviceToDevice, s));
    if (do_bases) HIP_TRY(hipMemcpyAsync(out->off, off, ((size_t)n + 1) * 4, hipMemcpyDeviceToDevice, s));
    if (do_names) HIP_TRY(hipMemcpyAsync(out->name_off, noff, ((size_t)n + 1) * 4, hipMemcpyDeviceToDevice, s));
    if (n && (do_bases || do_names)) k_gather<<<blocks_for(n, kWaves), kThreads, 0, s>>>(j, n, off, noff, do_bases ? out->bases : nullptr, do_bases ? out->qual : nullptr, do_names ? out->names : nullptr);
    if (n && do_rows) {
        if (out->row_words) k_rows<<<blocks_for((uint64_t)n * out->row_words, kThreads), kThreads, 0, s>>>(j, n, out->row_words, out->rows, out->len);
        else HIP_TRY(hipMemcpyAsync(out->len, b->rl.p, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        if (info->n_odd) k_odd<true><<<blocks_for(n, kWaves), kThreads, 0, s>>>(j, (const DevInfo *)b->info.p, nullptr, ooff, out->odd);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev[6], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, b->ev[5], b->ev[6]));
    b->ms[3] += ms; // (unpack: what follows the join in the sizes pass, and the output pass)
    return rc;
}

void mcx_bam_in_last(const mcx_bam_in *b, uint64_t stats[6], float ms[4])
{
    for (int i = 0; i < 6; i++) if (stats) stats[i] = b ? b->stats[i] : 0;
    for (int i = 0; i < 4; i++) if (ms) ms[i] = b ? b->ms[i] : 0;
}
uint32_t mcx_bam_in_grown(const mcx_bam_in *b) { return b ? b->grown : 0; }

extern "C" int mcx_bam_reads_header(const uint8_t *text, uint64_t bytes, uint64_t *records_at, int32_t *n_ref)
{
    if ((!text && bytes) || !records_at || !n_ref) return mcx_set_error(MCX_ERR_ARG, "mcx_bam_reads_header: null argument");
    return reads_header(text, bytes, records_at, n_ref);
}
