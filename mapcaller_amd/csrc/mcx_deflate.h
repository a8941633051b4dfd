// mapcaller_amd/csrc/mcx_deflate.h — up to 65 280 bytes of text (one BGZF block: bgzip's cut) compressed to one raw deflate stream by one wavefront; for the
// device (k_deflate, mcx_deflate.hip) and, with one lane, for the host (tests/hostemu/deflate_check.cpp).  The twin of mcx_inflate.h, whose conventions, CRC-32
// and RFC 1951 tables it uses.  No code of zlib's.
//
// The same text gives the same bytes on every run and in both builds: whatever the 64 lanes of the device decide together is defined over 64 POSITIONS, which
// the host's one lane walks in order (kPer positions per lane: 1 on the device, 64 on the host).
//   matching  the block's own bytes only.  The wavefront takes the 64 positions from the parse position on: every lane hashes the 4 bytes at its position,
//             looks the last earlier position with that hash up (a table of 16-bit positions, 8 KB) and measures the match (4 .. 258 bytes, distance 1 .. 32 768);
//             then the 64 positions enter the table, the highest one winning a slot.  The greedy parse — which positions start a token — is the set reachable
//             from position 0 over next = i + max(1, len): pointer doubling, six rounds.  The token that crosses the 64th position says where the next 64 begin.
//   codes     literal / length and distance counts in the wavefront's Work; code lengths by Moffat and Katajainen's in-place construction over the symbols
//             ranked by (count, symbol) (the ranking by all lanes, the construction by lane 0: at most 286 symbols); a code longer than 15 bits (7 for the
//             code-length code) halves the counts, rounding up, and builds again — every result is a complete Huffman code.  The code lengths are run-length
//             coded with 16 / 17 / 18.  A block without a match declares one distance code of zero bits; a single distance code is one bit long.
//   tokens    are not kept: the matcher is deterministic and runs twice, once for the counts and once — dynamic or fixed codes chosen, whichever is shorter —
//             to emit.  A token's bits (at most 48) go to their place by a prefix sum of the bit lengths over the lanes, OR-ed into a staging row of words,
//             and whole 32-bit words leave for the slot from as many lanes.
//   choice    the exact sizes of the dynamic and the fixed form are known from the counts; the smallest of dynamic, fixed and stored is written, so a payload
//             never exceeds n + 5 bytes.  Should an emission ever want more than the slot holds (it cannot) nothing is written there and the block is stored.
// Every access is checked: the text is read inside text[0 .. n) only, the slot written inside slot[0 .. slot_bytes) only.
#ifndef MCX_DEFLATE_H
#define MCX_DEFLATE_H
#include "mcx_inflate.h"

#define MCX_DEF_HD MCX_INF_HD

namespace mcx {
namespace def {

using inf::kLanes;
using inf::uni32;

enum : uint32_t { kMaxBlock = 65280, kHashBits = 12, kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768, kPer = 64 / kLanes, kStageWords = 104,
                  kMemberExtra = 26 /* header 18 + CRC-32 + ISIZE */, kStoredExtra = 5 };

// what one wavefront works in (LDS on the device): 14.3 KB
struct Work {
    uint16_t head[1u << kHashBits];      // position + 1 of the last text position with this hash; 0: none
    uint32_t lit_freq[288], dist_freq[32];
    uint32_t wf[288], w[288];            // (build_lengths) the counts being halved; the construction's array
    uint16_t order[288];                 // symbols by (count, symbol)
    uint8_t lens[288 + 32];              // literal / length code lengths, the distance codes' from 288 on
    uint16_t code[288 + 32];             // the codes, bit-reversed: as they enter the stream
    uint32_t cl_freq[20];
    uint8_t cl_lens[20];
    uint16_t cl_code[20];
    uint16_t cl_tok[288 + 32];           // the run-length coded lengths: symbol | extra bits' value << 5
    uint32_t stage[kStageWords];         // a step's token bits on their way out; all zero between steps
    uint8_t flag[64];                    // (parse) positions reached in a doubling round
    uint32_t misc[8];                    // lane 0's results for all: hlit, hdist, hclen, tokens, bits of the dynamic form, of the fixed form
};

// ---- what the lanes of a wavefront do together, over kPer positions a lane -----------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
static MCX_DEF_HD void sync_work() { inf::sync_tables(); }
static MCX_DEF_HD uint64_t ballot_of(const bool *p) { return __ballot(p[0]); }
static MCX_DEF_HD void gather_of(const uint32_t *v, const uint32_t *src, uint32_t *out) { out[0] = (uint32_t)__shfl((int)v[0], (int)(src[0] & 63u), 64); }
static MCX_DEF_HD uint32_t value_at(const uint32_t *v, uint32_t k) { return uni32((uint32_t)__shfl((int)v[0], (int)k, 64)); }
static MCX_DEF_HD uint32_t scan_of(const uint32_t *v, uint32_t *excl, uint32_t lane) // exclusive prefix sums over the positions; returns the total
{
    uint32_t x = v[0];
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64); if (lane >= d) x += y; }
    excl[0] = x - v[0];
    return uni32((uint32_t)__shfl((int)x, 63, 64));
}
static MCX_DEF_HD void count_one(uint32_t *p) { atomicAdd(p, 1u); }
static MCX_DEF_HD void or_into(uint32_t *p, uint32_t v) { atomicOr(p, v); }
#else
static MCX_DEF_HD void sync_work() {}
static MCX_DEF_HD uint64_t ballot_of(const bool *p) { uint64_t m = 0; for (uint32_t q = 0; q < kPer; q++) m |= (uint64_t)(p[q] ? 1u : 0u) << q; return m; }
static MCX_DEF_HD void gather_of(const uint32_t *v, const uint32_t *src, uint32_t *out) { for (uint32_t q = 0; q < kPer; q++) out[q] = v[src[q] & 63u]; }
static MCX_DEF_HD uint32_t value_at(const uint32_t *v, uint32_t k) { return v[k]; }
static MCX_DEF_HD uint32_t scan_of(const uint32_t *v, uint32_t *excl, uint32_t) { uint32_t s = 0; for (uint32_t q = 0; q < kPer; q++) { excl[q] = s; s += v[q]; } return s; }
static MCX_DEF_HD void count_one(uint32_t *p) { ++*p; }
static MCX_DEF_HD void or_into(uint32_t *p, uint32_t v) { *p |= v; }
#endif
static MCX_DEF_HD uint32_t ctz64(uint64_t m) { return (uint32_t)__builtin_ctzll(m); }
static MCX_DEF_HD uint32_t log2_of(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); } // v > 0

// ---- the output: whole 32-bit words to the slot; the state is the same in every lane ----------------------------------------------
struct Out {
    uint32_t *dst; uint32_t cap_words, words, acc, acc_bits; // acc: the acc_bits (< 32) bits behind the last whole word
    bool fail;                                               // more was wanted than cap_words: nothing further is stored
};
static MCX_DEF_HD void put(Out &o, uint32_t v, uint32_t nb, uint32_t lane) // nb <= 16 bits, by lane 0
{
    uint64_t a = (uint64_t)o.acc | ((uint64_t)v << o.acc_bits);
    o.acc_bits += nb;
    if (o.acc_bits >= 32) {
        if (o.words < o.cap_words) { if (lane == 0) o.dst[o.words] = (uint32_t)a; } else o.fail = true;
        o.words++; a >>= 32; o.acc_bits -= 32;
    }
    o.acc = (uint32_t)a;
}
static MCX_DEF_HD uint32_t finish(Out &o, uint32_t lane) // the last bits; returns the stream's bytes
{
    const uint32_t bytes = o.words * 4 + (o.acc_bits + 7) / 8;
    if (o.acc_bits) { if (o.words < o.cap_words) { if (lane == 0) o.dst[o.words] = o.acc; } else o.fail = true; }
    return bytes;
}

// RFC 1951 3.2.5 backwards: the length code (257 + i) of a match length and the distance code of a distance, with the extra bits' count and value
static MCX_DEF_HD uint32_t len_code(uint32_t len, uint32_t &extra, uint32_t &value)
{
    const uint32_t l = len - 3;
    if (len == 258) { extra = 0; value = 0; return 28; }
    if (l < 8) { extra = 0; value = 0; return l; }
    extra = log2_of(l) - 2; value = l & ((1u << extra) - 1);
    return 4 + 4 * extra + ((l >> extra) & 3u);
}
static MCX_DEF_HD uint32_t dist_code(uint32_t dist, uint32_t &extra, uint32_t &value)
{
    const uint32_t m = dist - 1;
    if (m < 4) { extra = 0; value = 0; return m; }
    extra = log2_of(m) - 1; value = m & ((1u << extra) - 1);
    return 2 + 2 * extra + ((m >> extra) & 1u);
}

static MCX_DEF_HD uint32_t load32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static MCX_DEF_HD uint32_t match_len(const uint8_t *a, const uint8_t *b, uint32_t most) // how many of the first `most` bytes agree
{
    uint32_t i = 0;
    while (i + 4 <= most) {
        const uint32_t x = load32(a + i) ^ load32(b + i);
        if (x) return i + ((uint32_t)__builtin_ctz(x) >> 3);
        i += 4;
    }
    while (i < most && a[i] == b[i]) i++;
    return i;
}

// One pass of the matcher over text[0 .. n).  Emit false: the tokens are counted (W.lit_freq, W.dist_freq; the end-of-block symbol is the caller's).  Emit true:
// their bits, by W.code / W.lens, leave through o.  Both passes find the same tokens: the table starts empty and nothing else enters the decisions.
template <bool Emit>
static MCX_DEF_HD void parse(const uint8_t *text, uint32_t n, Work &W, Out &o, uint32_t lane)
{
    for (uint32_t i = lane; i < (1u << kHashBits); i += kLanes) W.head[i] = 0;
    sync_work();
    uint32_t base = 0;
    while (base < n) {
        uint32_t hash[kPer], len[kPer], dist[kPer], jump[kPer], next[kPer];
        bool valid[kPer], reach[kPer], has[kPer], tok[kPer];
        // every position's candidate, from the positions before `base`
        for (uint32_t q = 0; q < kPer; q++) {
            const uint32_t k = q * kLanes + lane, p = base + k;
            valid[q] = p < n && n - p >= kMinMatch;
            hash[q] = valid[q] ? (load32(text + p) * 2654435761u) >> (32 - kHashBits) : 0u;
            len[q] = 0; dist[q] = 0;
            const uint32_t cand = valid[q] ? W.head[hash[q]] : 0u;
            if (cand) {
                const uint32_t c = cand - 1, d = p - c; // (c < base <= p)
                if (c < p && d <= kMaxDist) {
                    const uint32_t most = n - p < kMaxMatch ? n - p : (uint32_t)kMaxMatch;
                    const uint32_t l = match_len(text + c, text + p, most);
                    if (l >= kMinMatch) { len[q] = l; dist[q] = d; }
                }
            }
            has[q] = len[q] != 0;
        }
        sync_work();
        // the 64 positions enter the table in position order: the highest of a slot stays
        {
            bool need[kPer];
            for (uint32_t q = 0; q < kPer; q++) need[q] = valid[q];
            for (uint32_t round = 0; round < 64; round++) {
                for (uint32_t q = 0; q < kPer; q++) if (need[q]) W.head[hash[q]] = (uint16_t)(base + q * kLanes + lane + 1);
                sync_work();
                for (uint32_t q = 0; q < kPer; q++) need[q] = valid[q] && W.head[hash[q]] < base + q * kLanes + lane + 1;
                sync_work();
                if (ballot_of(need) == 0) break;
            }
        }
        // which positions start a token: those reached from position 0
        for (uint32_t q = 0; q < kPer; q++) {
            const uint32_t k = q * kLanes + lane;
            next[q] = k + (len[q] ? len[q] : 1u);
            jump[q] = base + k >= n || next[q] >= 64 ? 64u : next[q];
            reach[q] = k == 0;
        }
        if (ballot_of(has) == 0) { for (uint32_t q = 0; q < kPer; q++) reach[q] = true; } // (literals only)
        else {
            for (uint32_t round = 0; round < 6; round++) {
                for (uint32_t q = 0; q < kPer; q++) W.flag[q * kLanes + lane] = 0;
                sync_work();
                for (uint32_t q = 0; q < kPer; q++) if (reach[q] && jump[q] < 64) W.flag[jump[q]] = 1;
                sync_work();
                uint32_t two[kPer];
                gather_of(jump, jump, two);
                for (uint32_t q = 0; q < kPer; q++) { reach[q] = reach[q] || W.flag[q * kLanes + lane] != 0; if (jump[q] < 64) jump[q] = two[q]; }
                sync_work();
            }
        }
        for (uint32_t q = 0; q < kPer; q++) tok[q] = reach[q] && base + q * kLanes + lane < n;
        // where the next 64 positions begin: behind the token that leaves these (none: the text ends here)
        uint32_t new_base = n;
        {
            bool leaves[kPer];
            for (uint32_t q = 0; q < kPer; q++) leaves[q] = tok[q] && next[q] >= 64;
            const uint64_t m = ballot_of(leaves);
            if (m) new_base = base + value_at(next, ctz64(m));
        }
        if (!Emit) {
            for (uint32_t q = 0; q < kPer; q++) {
                if (!tok[q]) continue;
                if (len[q]) { uint32_t e, v; count_one(&W.lit_freq[257 + len_code(len[q], e, v)]); count_one(&W.dist_freq[dist_code(dist[q], e, v)]); }
                else count_one(&W.lit_freq[text[base + q * kLanes + lane]]);
            }
        } else {
            uint64_t bits[kPer];
            uint32_t nb[kPer], at[kPer];
            for (uint32_t q = 0; q < kPer; q++) {
                bits[q] = 0; nb[q] = 0;
                if (!tok[q]) continue;
                if (len[q]) {
                    uint32_t e, v;
                    const uint32_t ls = 257 + len_code(len[q], e, v);
                    bits[q] = W.code[ls]; nb[q] = W.lens[ls];
                    bits[q] |= (uint64_t)v << nb[q]; nb[q] += e;
                    const uint32_t ds = 288 + dist_code(dist[q], e, v);
                    bits[q] |= (uint64_t)W.code[ds] << nb[q]; nb[q] += W.lens[ds];
                    bits[q] |= (uint64_t)v << nb[q]; nb[q] += e;
                } else { const uint32_t s = text[base + q * kLanes + lane]; bits[q] = W.code[s]; nb[q] = W.lens[s]; }
            }
            const uint32_t total = scan_of(nb, at, lane);
            if (lane == 0) W.stage[0] = o.acc;
            sync_work();
            for (uint32_t q = 0; q < kPer; q++) {
                if (!nb[q]) continue;
                const uint32_t off = o.acc_bits + at[q], wd = off >> 5, s = off & 31u;
                const uint64_t lo = bits[q] << s;
                const uint32_t hi = s ? (uint32_t)(bits[q] >> (64 - s)) : 0u;
                if ((uint32_t)lo) or_into(&W.stage[wd], (uint32_t)lo);
                if ((uint32_t)(lo >> 32)) or_into(&W.stage[wd + 1], (uint32_t)(lo >> 32));
                if (hi) or_into(&W.stage[wd + 2], hi);
            }
            sync_work();
            const uint32_t end = o.acc_bits + total, full = end >> 5; // (at most 31 + 64 * 48 bits: 96 whole words and a part)
            if (o.words + full > o.cap_words) o.fail = true;
            if (!o.fail) for (uint32_t i = lane; i < full; i += kLanes) o.dst[o.words + i] = W.stage[i];
            o.acc = uni32(W.stage[full]); o.acc_bits = end & 31u; o.words += full;
            sync_work();
            for (uint32_t i = lane; i <= full; i += kLanes) W.stage[i] = 0;
            sync_work();
        }
        base = uni32(new_base);
    }
}

// Moffat and Katajainen's in-place minimum-redundancy code lengths: A[0 .. n) the weights in ascending order, n >= 2; A[i] becomes the length of symbol i's code
static MCX_DEF_HD void code_lengths_in_place(uint32_t *A, int n)
{
    A[0] += A[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < n - 1; next++) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (next = n - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
    int avail = 1, used = 0;
    uint32_t depth = 0;
    root = n - 2; next = n - 1;
    while (avail > 0) {
        while (root >= 0 && A[root] == depth) { used++; root--; }
        while (avail > used) { A[next--] = depth; avail--; }
        avail = 2 * used; depth++; used = 0;
    }
}

// lens[0 .. n) from freq[0 .. n) (n <= 288), no code longer than `limit`; a symbol that does not occur gets 0.  Returns how many occur.  One symbol alone gets a
// code of one bit.  By the whole wavefront.
static MCX_DEF_HD uint32_t build_lengths(const uint32_t *freq, uint32_t n, uint32_t limit, uint8_t *lens, Work &W, uint32_t lane)
{
    for (uint32_t i = lane; i < n; i += kLanes) { W.wf[i] = freq[i]; lens[i] = 0; }
    sync_work();
    uint32_t used = 0;
    for (uint32_t i = 0; i < n; i++) used += uni32(W.wf[i]) != 0;
    if (used == 0) return 0;
    for (uint32_t iter = 0; iter < 24; iter++) {
        for (uint32_t s = lane; s < n; s += kLanes) {
            const uint32_t f = W.wf[s];
            if (!f) continue;
            uint32_t r = 0;
            for (uint32_t t = 0; t < n; t++) { const uint32_t ft = W.wf[t]; r += ft && (ft < f || (ft == f && t < s)); }
            W.order[r] = (uint16_t)s; W.w[r] = f;
        }
        sync_work();
        if (used == 1) { if (lane == 0) lens[W.order[0]] = 1; sync_work(); return 1; }
        if (lane == 0) code_lengths_in_place(W.w, (int)used);
        sync_work();
        if (uni32(W.w[0]) <= limit) break; // (the rarest symbol's code is the longest)
        for (uint32_t s = lane; s < n; s += kLanes) W.wf[s] = (W.wf[s] + 1) >> 1;
        sync_work();
    }
    for (uint32_t i = lane; i < used; i += kLanes) lens[W.order[i]] = (uint8_t)W.w[i];
    sync_work();
    return used;
}

// the canonical codes of lens[0 .. n), bit-reversed (lane 0)
static MCX_DEF_HD void assign_codes(const uint8_t *lens, uint32_t n, uint16_t *code)
{
    uint32_t count[16], next[16];
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (uint32_t s = 0; s < n; s++) count[lens[s]]++;
    count[0] = 0; next[0] = 0;
    for (int l = 1; l < 16; l++) next[l] = (next[l - 1] + count[l - 1]) << 1;
    for (uint32_t s = 0; s < n; s++) code[s] = lens[s] ? (uint16_t)inf::rev16(next[lens[s]]++, lens[s]) : (uint16_t)0;
}

static MCX_DEF_HD uint32_t fixed_len(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }
static MCX_DEF_HD uint32_t cl_order(uint32_t i) // RFC 1951 3.2.7: the order in which the code-length code's lengths are sent
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// (lane 0) the code lengths W.lens[0 .. hlit) and W.lens[288 .. 288 + hdist) as one sequence, run-length coded into W.cl_tok and counted in W.cl_freq
static MCX_DEF_HD void code_the_lengths(Work &W)
{
    uint32_t hlit = 286, hdist = 30;
    while (hlit > 257 && W.lens[hlit - 1] == 0) hlit--;
    while (hdist > 1 && W.lens[288 + hdist - 1] == 0) hdist--;
    for (int i = 0; i < 20; i++) W.cl_freq[i] = 0;
    const uint32_t total = hlit + hdist;
    uint32_t n_tok = 0;
    for (uint32_t i = 0; i < total;) {
        const uint32_t v = W.lens[i < hlit ? i : 288 + i - hlit];
        uint32_t run = 1;
        while (i + run < total && W.lens[i + run < hlit ? i + run : 288 + i + run - hlit] == v) run++;
        i += run;
        if (v) { W.cl_tok[n_tok++] = (uint16_t)v; W.cl_freq[v]++; run--; }
        while (run >= 3) {
            uint32_t sym, take, ext;
            if (v) { sym = 16; take = run < 6 ? run : 6; ext = take - 3; }
            else if (run >= 11) { sym = 18; take = run < 138 ? run : 138; ext = take - 11; }
            else { sym = 17; take = run; ext = take - 3; }
            W.cl_tok[n_tok++] = (uint16_t)(sym | (ext << 5)); W.cl_freq[sym]++; run -= take;
        }
        for (; run; run--) { W.cl_tok[n_tok++] = (uint16_t)v; W.cl_freq[v]++; }
    }
    // (a code-length code of one symbol would be incomplete: a second one, never sent, completes it)
    uint32_t used = 0, only = 0;
    for (uint32_t s = 0; s < 19; s++) if (W.cl_freq[s]) { used++; only = s; }
    if (used == 1) W.cl_freq[only ? 0 : 1] = 1;
    W.misc[0] = hlit; W.misc[1] = hdist; W.misc[3] = n_tok;
}

// (lane 0) every code, and the exact bits of the dynamic and of the fixed form of the block (header bits, tokens, end of block)
static MCX_DEF_HD void codes_and_costs(Work &W)
{
    assign_codes(W.lens, 288, W.code);
    assign_codes(W.lens + 288, 32, W.code + 288);
    assign_codes(W.cl_lens, 19, W.cl_code);
    uint32_t hclen = 19;
    while (hclen > 4 && W.cl_lens[cl_order(hclen - 1)] == 0) hclen--;
    uint32_t extra = 0, dyn = 3 + 14 + 3 * hclen, fix = 3;
    for (uint32_t s = 0; s < 286; s++) {
        const uint32_t f = W.lit_freq[s];
        if (s > 256) extra += f * inf::len_extra(s - 257);
        dyn += f * W.lens[s]; fix += f * fixed_len(s);
    }
    for (uint32_t s = 0; s < 30; s++) { const uint32_t f = W.dist_freq[s]; extra += f * inf::dist_extra(s); dyn += f * W.lens[288 + s]; fix += f * 5; }
    for (uint32_t i = 0; i < W.misc[3]; i++) { const uint32_t s = W.cl_tok[i] & 31u; dyn += W.cl_lens[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u); }
    W.misc[2] = hclen; W.misc[4] = dyn + extra; W.misc[5] = fix + extra;
}

static MCX_DEF_HD void store_block(const uint8_t *text, uint32_t n, uint8_t *slot, uint32_t lane) // BFINAL = 1, BTYPE = 00, LEN, NLEN, the bytes
{
    if (lane == 0) { slot[0] = 1; slot[1] = (uint8_t)n; slot[2] = (uint8_t)(n >> 8); slot[3] = (uint8_t)~n; slot[4] = (uint8_t)(~n >> 8); }
    for (uint32_t i = lane; i < n; i += kLanes) slot[5 + i] = text[i];
}

// One block: text[0 .. n), 1 <= n <= 65 280, to a raw deflate stream at slot (4-byte aligned, slot_bytes >= n + 5, a multiple of 4); *crc: the text's CRC-32.
// Called by every lane of a wavefront with the same arguments (on the host: by the one lane 0); crc_tab as for inflate_member.  Returns the stream's bytes
// (<= n + 5), the same in every lane.
static MCX_DEF_HD uint32_t deflate_block(const uint8_t *text, uint32_t n, uint8_t *slot, uint32_t slot_bytes, Work &W, const uint32_t *crc_tab, uint32_t lane, uint32_t *crc)
{
    *crc = inf::crc_of(text, n, crc_tab, lane);
    for (uint32_t i = lane; i < 288; i += kLanes) W.lit_freq[i] = i == 256 ? 1u : 0u;
    for (uint32_t i = lane; i < 32; i += kLanes) W.dist_freq[i] = 0;
    for (uint32_t i = lane; i < kStageWords; i += kLanes) W.stage[i] = 0;
    sync_work();
    Out o;
    o.dst = (uint32_t *)slot; o.cap_words = slot_bytes / 4; o.words = 0; o.acc = 0; o.acc_bits = 0; o.fail = false;
    parse<false>(text, n, W, o, lane);
    sync_work();
    build_lengths(W.lit_freq, 286, 15, W.lens, W, lane);
    for (uint32_t i = lane; i < 34; i += kLanes) W.lens[i < 2 ? 286 + i : 288 + i - 2] = 0;
    sync_work();
    build_lengths(W.dist_freq, 30, 15, W.lens + 288, W, lane);
    if (lane == 0) code_the_lengths(W);
    sync_work();
    build_lengths(W.cl_freq, 19, 7, W.cl_lens, W, lane);
    if (lane == 0) codes_and_costs(W);
    sync_work();
    const uint32_t hlit = uni32(W.misc[0]), hdist = uni32(W.misc[1]), hclen = uni32(W.misc[2]), n_tok = uni32(W.misc[3]);
    const uint32_t dyn_bytes = (uni32(W.misc[4]) + 7) / 8, fix_bytes = (uni32(W.misc[5]) + 7) / 8, stored = n + kStoredExtra;
    const bool dynamic = dyn_bytes <= fix_bytes;
    const uint32_t want = dynamic ? dyn_bytes : fix_bytes;
    if (want < stored && want <= slot_bytes) {
        put(o, 1, 1, lane);
        put(o, dynamic ? 2 : 1, 2, lane);
        if (dynamic) {
            put(o, hlit - 257, 5, lane); put(o, hdist - 1, 5, lane); put(o, hclen - 4, 4, lane);
            for (uint32_t i = 0; i < hclen; i++) put(o, uni32(W.cl_lens[cl_order(i)]), 3, lane);
            for (uint32_t i = 0; i < n_tok; i++) {
                const uint32_t t = uni32(W.cl_tok[i]), s = t & 31u;
                put(o, uni32(W.cl_code[s]), uni32(W.cl_lens[s]), lane);
                if (s >= 16) put(o, t >> 5, s == 16 ? 2 : s == 17 ? 3 : 7, lane);
            }
        } else {
            sync_work();
            if (lane == 0) {
                for (uint32_t s = 0; s < 288; s++) W.lens[s] = (uint8_t)fixed_len(s);
                for (uint32_t s = 0; s < 32; s++) W.lens[288 + s] = 5;
                assign_codes(W.lens, 288, W.code);
                assign_codes(W.lens + 288, 32, W.code + 288);
            }
            sync_work();
        }
        parse<true>(text, n, W, o, lane);
        put(o, uni32(W.code[256]), uni32(W.lens[256]), lane);
        const uint32_t bytes = finish(o, lane);
        if (!o.fail && bytes == want) return bytes;
    }
    store_block(text, n, slot, lane);
    return stored;
}

// ---- BGZF framing: byte i of a member whose deflate stream is `payload` bytes long ---------------------------------------------------
static MCX_DEF_HD uint8_t member_byte(uint32_t i, const uint8_t *stream, uint32_t payload, uint32_t crc, uint32_t isize)
{
    if (i >= 18 && i < 18 + payload) return stream[i - 18];
    if (i < 18) {
        const uint32_t bsize = payload + kMemberExtra - 1;
        switch (i) {
        case 0: return 0x1f; case 1: return 0x8b; case 2: return 8; case 3: return 4; case 9: return 0xff; case 10: return 6;
        case 12: return 'B'; case 13: return 'C'; case 14: return 2; case 16: return (uint8_t)bsize; case 17: return (uint8_t)(bsize >> 8);
        default: return 0;
        }
    }
    const uint32_t k = i - 18 - payload; // CRC-32, ISIZE: little-endian
    return (uint8_t)((k < 4 ? crc : isize) >> (8 * (k & 3u)));
}
// a slot's size for blocks of `block` bytes of text: the stored form, whole words
static MCX_DEF_HD uint32_t slot_bytes_of(uint32_t block) { return (block + kStoredExtra + 3 + 15) / 16 * 16; }

} // namespace def
} // namespace mcx
#endif
