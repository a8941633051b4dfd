// mapcaller_amd/csrc/mcx_inflate.h — one raw deflate stream of known output size (a BGZF member: at most 64 KB of text), inflated and CRC-checked
// by one wavefront; for the device (k_inflate, mcx_inflate.hip) and, with one lane, for the host (tests/hostemu/inflate_check.cpp).
//
// RFC 1951 restated (stored, fixed and dynamic blocks, any number of them); the length / distance base tables and the shape of the header reader are
// those of this project's host restatement, mcx_pgz.h.  No code of zlib's.
//
// What is the same in every lane — the bit buffer, the positions in input and output, a table look-up's result — is kept uniform (uni32: readfirstlane on
// the device), so that the decode loop runs on the scalar unit and nothing diverges.  What a wavefront's lanes share the work of:
//   tables    a lane per symbol: its canonical code from the counts (ranks by ballot), its replicated entries of the root table
//   literals  up to eight gathered in a register, stored by as many lanes at once
//   matches   lane i writes dst[p + i] = dst[p - D + (i mod D)], i < L: right for overlapping copies, D = 1 included.  The source may be bytes the
//             wavefront stored a step earlier: a workgroup-scope fence orders them (the output is at most 64 KB and stays in L2)
//   CRC-32    a contiguous slice per lane (byte table), the partial values multiplied by x^(8 * bytes behind the slice) mod P and summed
// Tables per wavefront (Tables, 3.6 KB; LDS on the device): a 10-bit root table for literal / length codes and an 8-bit one for distance codes; a longer
// code is found by the canonical walk over the per-length counts and the symbols sorted by code — no sub-tables, a fixed footprint.
//
// Every loop is bounded and every access checked: input is read inside src[0 .. readable) only (readable >= src_len: what the caller's buffer holds from
// the member's first byte on; eight bytes of slack behind a member let every refill be one 64-bit load; what lies
// behind src_len is read as zeros and never consumed; where fewer than 8 bytes are readable the refill goes byte by byte), output is written inside dst[0 .. isize) only; a damaged member ends with a status.
#ifndef MCX_INFLATE_H
#define MCX_INFLATE_H
#include <stdint.h>
#include <string.h>
#include "../../include/mcx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MCX_INF_HD __host__ __device__ __forceinline__
#else
#define MCX_INF_HD inline
#endif

namespace mcx {
namespace inf {

#if defined(__HIP_DEVICE_COMPILE__)
enum : uint32_t { kLanes = 64 };
static MCX_INF_HD uint32_t uni32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
static MCX_INF_HD uint64_t ballot(bool p) { return __ballot(p); }
static MCX_INF_HD uint32_t popc64(uint64_t m) { return (uint32_t)__popcll(m); }
static MCX_INF_HD uint32_t xor_lanes(uint32_t x) { for (int s = 32; s; s >>= 1) x ^= (uint32_t)__shfl_xor((int)x, s, 64); return x; }
// what one lane stored to the tables is read by the others of its wavefront (no other wavefront shares them)
static MCX_INF_HD void sync_tables()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// what the wavefront's lanes stored to the output is read by other lanes of it
static MCX_INF_HD void sync_output()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
#else
enum : uint32_t { kLanes = 1 };
static MCX_INF_HD uint32_t uni32(uint32_t x) { return x; }
static MCX_INF_HD uint64_t ballot(bool p) { return p ? 1u : 0u; }
static MCX_INF_HD uint32_t popc64(uint64_t m) { uint32_t n = 0; for (; m; m &= m - 1) n++; return n; }
static MCX_INF_HD uint32_t xor_lanes(uint32_t x) { return x; }
static MCX_INF_HD void sync_tables() {}
static MCX_INF_HD void sync_output() {}
#endif
static MCX_INF_HD uint64_t uni64(uint64_t x) { return (uint64_t)uni32((uint32_t)x) | ((uint64_t)uni32((uint32_t)(x >> 32)) << 32); }

enum : uint32_t { kLitRootBits = 10, kDistRootBits = 8, kClRootBits = 7, kMaxIsize = 65536, kCrcPoly = 0xEDB88320u };

// an entry of a root table: symbol | code length << 12; 0: no code of at most the root's bits begins like this (a longer one, or none)
struct Tables {
    uint16_t lit_root[1u << kLitRootBits];
    uint16_t dist_root[1u << kDistRootBits]; // (the code-length code's 7-bit table while a dynamic header is read)
    uint16_t lit_sorted[288], dist_sorted[32];
    uint16_t lit_cnt[16], dist_cnt[16];
    uint8_t lens[288 + 32];
    uint8_t cl_lens[32];
};

struct Info { uint32_t max_lit_len, max_dist_len, blocks; }; // (host checks) the longest code of each kind a stream's headers declared

static MCX_INF_HD uint32_t rev16(uint32_t v, uint32_t bits) // the low `bits` bits of v, reversed
{
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
    v = ((v & 0x00FFu) << 8) | ((v >> 8) & 0x00FFu);
    return v >> (16 - bits);
}

// A canonical Huffman code from lens[0 .. n) (0: unused): root[0 .. 1 << root_bits), sorted[], cnt[1 .. 15].  Returns 0: a complete code, 1: a single code
// of length 1 (the one incomplete code zlib accepts), 2: no code at all, -1: over-subscribed or otherwise incomplete.  *longest: the longest code.
static MCX_INF_HD int build_code(const uint8_t *lens, uint32_t n, uint16_t *root, uint32_t root_bits, uint16_t *sorted, uint16_t *cnt, uint32_t lane, uint32_t *longest)
{
    uint32_t count[16], first[16], offs[16], run[16];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int l = 0; l < 16; l++) count[l] = run[l] = 0;
    for (uint32_t base = 0; base < n; base += kLanes) {
        const uint32_t s = base + lane, l = s < n ? lens[s] : 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int L = 1; L < 16; L++) count[L] += popc64(ballot(l == (uint32_t)L));
    }
    uint32_t used = 0, top = 0;
    int32_t left = 1;
    bool over = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int L = 1; L < 16; L++) {
        left = left * 2 - (int32_t)count[L];
        if (left < 0) over = true;
        if (left < 0) left = 0; // (no overflow of the running product; `over` is what counts)
        used += count[L];
        if (count[L]) top = (uint32_t)L;
    }
    *longest = top;
    for (uint32_t i = lane; i < (1u << root_bits); i += kLanes) root[i] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int L = 0; L < 16; L++) if ((uint32_t)L % kLanes == lane) cnt[L] = (uint16_t)(L ? count[L] : 0u);
    sync_tables();
    if (over) return -1;
    if (used == 0) return 2;
    int kind = 0;
    if (left > 0) { if (used == 1 && count[1] == 1) kind = 1; else return -1; }
    {
        uint32_t code = 0, at = 0;
        first[0] = offs[0] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int L = 1; L < 16; L++) { code = (code + (L > 1 ? count[L - 1] : 0u)) << 1; first[L] = code; offs[L] = at; at += count[L]; }
    }
    for (uint32_t base = 0; base < n; base += kLanes) {
        const uint32_t s = base + lane, l = s < n ? lens[s] : 0u;
        uint32_t code = 0, at = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int L = 1; L < 16; L++) {
            const uint64_t m = ballot(l == (uint32_t)L);
            if (l == (uint32_t)L) { const uint32_t r = run[L] + popc64(m & ((1ull << lane) - 1)); code = first[L] + r; at = offs[L] + r; }
            run[L] += popc64(m);
        }
        if (l) {
            sorted[at] = (uint16_t)s;
            if (l <= root_bits) {
                const uint16_t e = (uint16_t)(s | (l << 12));
                for (uint32_t i = rev16(code, l); i < (1u << root_bits); i += 1u << l) root[i] = e;
            }
        }
    }
    sync_tables();
    return kind;
}

// the bit reader: LSB first, 64 bits, refilled eight bytes at a time; bytes from src_len on read as zeros
struct Bits {
    const uint8_t *src;
    uint32_t src_len, readable, p;
    uint64_t buf;
    uint32_t cnt;
};
static MCX_INF_HD void bits_refill(Bits &b)
{
    uint64_t w = 0;
    if (b.p < b.src_len) {
        const uint32_t have = b.src_len - b.p;
        if (b.readable - b.p >= 8) {
            memcpy(&w, b.src + b.p, 8);
            w = uni64(w);
            if (have < 8) w &= (1ull << (8 * have)) - 1;
        } else { // (the last bytes of a buffer without slack)
            for (uint32_t i = 0; i < have && i < 8; i++) w |= (uint64_t)uni32(b.src[b.p + i]) << (8 * i);
        }
    }
    b.buf |= w << b.cnt;
    b.p += (63 - b.cnt) >> 3; // (as many whole bytes as fit are kept, the rest is fetched again next time; behind src_len the position only counts)
    b.cnt |= 56;
}
// the reader set at bit `bit` of src, anywhere in it (a stretch of an ordinary gzip stream begins at any bit: mcx_gz_dev.h)
static MCX_INF_HD void bits_start(Bits &b, const uint8_t *src, uint32_t src_len, uint32_t readable, uint64_t bit)
{
    b.src = src; b.src_len = src_len; b.readable = readable < src_len ? src_len : readable; b.p = (uint32_t)(bit >> 3); b.buf = 0; b.cnt = 0;
    bits_refill(b);
    b.buf >>= (uint32_t)(bit & 7u); b.cnt -= (uint32_t)(bit & 7u);
}
static MCX_INF_HD uint32_t bits_peek(const Bits &b, uint32_t n) { return (uint32_t)(b.buf & ((1ull << n) - 1)); }
static MCX_INF_HD void bits_drop(Bits &b, uint32_t n) { b.buf >>= n; b.cnt -= n; }
static MCX_INF_HD uint32_t bits_take(Bits &b, uint32_t n) { const uint32_t v = bits_peek(b, n); bits_drop(b, n); return v; }
static MCX_INF_HD uint64_t bits_pos(const Bits &b) { return (uint64_t)b.p * 8 - b.cnt; }                 // bits consumed
static MCX_INF_HD bool bits_over(const Bits &b) { return bits_pos(b) > (uint64_t)b.src_len * 8; }        // ... more than the member holds

// the next symbol of a code; -1: the bits are no code
static MCX_INF_HD int decode_sym(Bits &b, const uint16_t *root, uint32_t root_bits, const uint16_t *sorted, const uint16_t *cnt)
{
    const uint32_t e = uni32(root[bits_peek(b, root_bits)]);
    if (e) { bits_drop(b, e >> 12); return (int)(e & 0xFFFu); }
    // the canonical walk: one more bit per length, the code compared with that length's first code and count
    uint32_t code = 0, first = 0, index = 0;
    const uint32_t bits = bits_peek(b, 15);
    for (uint32_t len = 1; len <= 15; len++) {
        code |= (bits >> (len - 1)) & 1u;
        const uint32_t c = uni32(cnt[len]);
        if (code - first < c) { bits_drop(b, len); return (int)uni32(sorted[index + (code - first)]); }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    return -1;
}

// RFC 1951 3.2.5: length codes 257 + i (3 .. 258) and distance codes (1 .. 32768) with their extra bits, as arithmetic (mcx_pgz.h holds them as tables)
static MCX_INF_HD uint32_t len_base(uint32_t i) { return i < 8 ? 3 + i : i == 28 ? 258u : 3 + ((4 + (i & 3u)) << ((i - 4) >> 2)); }
static MCX_INF_HD uint32_t len_extra(uint32_t i) { return i < 8 || i == 28 ? 0u : (i - 4) >> 2; }
static MCX_INF_HD uint32_t dist_extra(uint32_t i) { return i < 4 ? 0u : (i - 2) >> 1; }
static MCX_INF_HD uint32_t dist_base(uint32_t i) { return i < 4 ? i + 1 : ((2u + (i & 1u)) << dist_extra(i)) + 1; }

// CRC-32 (reflected, polynomial 0xEDB88320): the byte table, products in GF(2)[x] mod P with x^0 at bit 31
static MCX_INF_HD uint32_t crc_table_entry(uint32_t i) { for (int k = 0; k < 8; k++) i = (i >> 1) ^ (kCrcPoly & (0u - (i & 1u))); return i; }
static MCX_INF_HD uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) { p ^= b & (0u - ((a >> (31 - i)) & 1u)); b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u))); }
    return p;
}
static MCX_INF_HD uint32_t gf_x8n(uint32_t n) // x^(8 n) mod P
{
    uint32_t r = 0x80000000u, sq = 0x00800000u;
    for (; n; n >>= 1) { if (n & 1u) r = gf_mul(r, sq); sq = gf_mul(sq, sq); }
    return r;
}
// of dst[0 .. n): 64 contiguous slices, a lane each, combined
static MCX_INF_HD uint32_t crc_of(const uint8_t *dst, uint32_t n, const uint32_t *crc_tab, uint32_t lane)
{
    const uint32_t slice = (n + 63) / 64;
    uint32_t acc = 0;
    for (uint32_t k = lane; k < 64; k += kLanes) {
        const uint32_t lo = k * slice < n ? k * slice : n, hi = lo + slice < n ? lo + slice : n;
        uint32_t c = k == 0 ? 0xFFFFFFFFu : 0u;
        for (uint32_t i = lo; i < hi; i++) c = crc_tab[(c ^ dst[i]) & 0xFFu] ^ (c >> 8);
        acc ^= gf_mul(c, gf_x8n(n - hi));
    }
    return uni32(xor_lanes(acc)) ^ 0xFFFFFFFFu;
}

// the header of a dynamic block (RFC 1951 3.2.7) behind BFINAL / BTYPE: both codes built; 0 or a status
static MCX_INF_HD uint32_t read_dynamic(Bits &b, Tables &t, uint32_t lane, bool &no_dist, Info *info)
{
    bits_refill(b);
    const uint32_t hlit = bits_take(b, 5) + 257, hdist = bits_take(b, 5) + 1, hclen = bits_take(b, 4) + 4;
    if (bits_over(b)) return MCX_INFLATE_INPUT;
    if (hlit > 286 || hdist > 30) return MCX_INFLATE_DAMAGED;
    for (uint32_t i = lane; i < 32; i += kLanes) t.cl_lens[i] = 0;
    sync_tables();
    for (uint32_t i = 0; i < hclen; i++) {
        // (RFC 1951: 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 — five bits each, packed)
        const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
        const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
        const uint32_t at = (uint32_t)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31u);
        bits_refill(b);
        const uint32_t v = bits_take(b, 3);
        if (lane == 0) t.cl_lens[at] = (uint8_t)v;
    }
    if (bits_over(b)) return MCX_INFLATE_INPUT;
    sync_tables();
    uint32_t longest;
    if (build_code(t.cl_lens, 19, t.dist_root, kClRootBits, t.dist_sorted, t.dist_cnt, lane, &longest) != 0) return MCX_INFLATE_DAMAGED;
    const uint32_t total = hlit + hdist;
    uint32_t n = 0, prev = 0;
    while (n < total) {
        bits_refill(b);
        const uint64_t left = (uint64_t)b.src_len * 8 > bits_pos(b) ? (uint64_t)b.src_len * 8 - bits_pos(b) : 0;
        const int s = decode_sym(b, t.dist_root, kClRootBits, t.dist_sorted, t.dist_cnt);
        if (s < 0) return left < 7 ? MCX_INFLATE_INPUT : MCX_INFLATE_DAMAGED;
        uint32_t rep = 1, v = (uint32_t)s;
        if (s == 16) { if (n == 0) return MCX_INFLATE_DAMAGED; v = prev; rep = 3 + bits_take(b, 2); }
        else if (s == 17) { v = 0; rep = 3 + bits_take(b, 3); }
        else if (s == 18) { v = 0; rep = 11 + bits_take(b, 7); }
        if (bits_over(b)) return MCX_INFLATE_INPUT;
        if (n + rep > total) return MCX_INFLATE_DAMAGED;
        for (uint32_t i = lane; i < rep; i += kLanes) t.lens[n + i] = (uint8_t)v;
        n += rep; prev = v;
    }
    sync_tables();
    if (uni32(t.lens[256]) == 0) return MCX_INFLATE_DAMAGED; // (no end-of-block code)
    uint32_t ll, dl;
    const int lk = build_code(t.lens, hlit, t.lit_root, kLitRootBits, t.lit_sorted, t.lit_cnt, lane, &ll);
    if (lk != 0 && lk != 1) return MCX_INFLATE_DAMAGED;
    const int dk = build_code(t.lens + hlit, hdist, t.dist_root, kDistRootBits, t.dist_sorted, t.dist_cnt, lane, &dl);
    if (dk < 0) return MCX_INFLATE_DAMAGED;
    no_dist = dk == 2;
    if (info) { if (ll > info->max_lit_len) info->max_lit_len = ll; if (dl > info->max_dist_len) info->max_dist_len = dl; }
    return 0;
}

static MCX_INF_HD void fixed_codes(Tables &t, uint32_t lane)
{
    for (uint32_t i = lane; i < 288; i += kLanes) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (uint32_t i = lane; i < 32; i += kLanes) t.lens[288 + i] = 5; // (codes 30 and 31 never occur in a valid stream: refused where they are decoded)
    sync_tables();
    uint32_t longest;
    build_code(t.lens, 288, t.lit_root, kLitRootBits, t.lit_sorted, t.lit_cnt, lane, &longest);
    build_code(t.lens + 288, 32, t.dist_root, kDistRootBits, t.dist_sorted, t.dist_cnt, lane, &longest);
}

// the literals gathered so far go to dst[out - n_lit .. out)
static MCX_INF_HD void flush_literals(uint8_t *dst, uint32_t out, uint64_t lits, uint32_t n_lit, uint32_t lane)
{
    for (uint32_t i = lane; i < n_lit; i += kLanes) dst[out - n_lit + i] = (uint8_t)(lits >> (8 * i));
}

// One member: src[0 .. src_len) -> dst[0 .. isize), its CRC-32 compared with `crc`; readable >= src_len: the bytes that may be read from src on.  Called by every lane of a wavefront with the same arguments (on
// the host: by the one lane 0).  crc_tab: the 256-entry byte table (crc_table_entry).  Returns an mcx_inflate_status, the same in every lane.
static MCX_INF_HD uint32_t inflate_member(const uint8_t *src, uint32_t src_len, uint32_t readable, uint8_t *dst, uint32_t isize, uint32_t crc, Tables &t, const uint32_t *crc_tab, uint32_t lane, Info *info)
{
    if (isize > kMaxIsize) return MCX_INFLATE_LENGTH;
    Bits b;
    b.src = src; b.src_len = src_len; b.readable = readable < src_len ? src_len : readable; b.p = 0; b.buf = 0; b.cnt = 0;
    uint32_t out = 0, n_lit = 0, codes = 0; // codes: what the tables hold — 0 nothing, 1 the fixed codes, 2 a dynamic block's
    uint64_t lits = 0;
    bool no_dist = false;
    // every step below consumes a bit or writes a byte, and both are limited: the guard is never what ends a valid member
    uint64_t guard = (uint64_t)src_len * 8 + isize + 64;
    for (;;) {
        bits_refill(b);
        const uint32_t bfinal = bits_take(b, 1), btype = bits_take(b, 2);
        if (bits_over(b)) return MCX_INFLATE_INPUT;
        if (info) info->blocks++;
        if (btype == 3) return MCX_INFLATE_DAMAGED;
        if (btype == 0) {
            bits_drop(b, b.cnt & 7u); // to the byte boundary (cnt is congruent to the bits left of the current byte)
            bits_refill(b);
            const uint32_t len = bits_take(b, 16), nlen = bits_take(b, 16);
            if (bits_over(b)) return MCX_INFLATE_INPUT;
            if ((len ^ nlen) != 0xFFFFu) return MCX_INFLATE_DAMAGED;
            const uint32_t at = b.p - (b.cnt >> 3); // (whole bytes are left in the buffer)
            if ((uint64_t)at + len > src_len) return MCX_INFLATE_INPUT;
            if (len > isize - out) return MCX_INFLATE_LENGTH;
            flush_literals(dst, out, lits, n_lit, lane); n_lit = 0; lits = 0;
            for (uint32_t i = lane; i < len; i += kLanes) dst[out + i] = src[at + i];
            out += len;
            b.p = at + len; b.buf = 0; b.cnt = 0;
        } else {
            if (btype == 1) { if (codes != 1) fixed_codes(t, lane); codes = 1; no_dist = false; }
            else {
                codes = 0;
                if (const uint32_t st = read_dynamic(b, t, lane, no_dist, info)) return st;
                codes = 2;
            }
            for (;;) {
                if (guard-- == 0) return MCX_INFLATE_DAMAGED;
                bits_refill(b); // >= 56 bits: a literal / length code (15) + length extra (5) + distance code (15) + distance extra (13) = 48
                const uint64_t left = (uint64_t)src_len * 8 > bits_pos(b) ? (uint64_t)src_len * 8 - bits_pos(b) : 0;
                const int s = decode_sym(b, t.lit_root, kLitRootBits, t.lit_sorted, t.lit_cnt);
                if (s < 0) return left < 15 ? MCX_INFLATE_INPUT : MCX_INFLATE_DAMAGED;
                if (s < 256) {
                    if (bits_over(b)) return MCX_INFLATE_INPUT;
                    if (out >= isize) return MCX_INFLATE_LENGTH;
                    lits |= (uint64_t)(uint32_t)s << (8 * n_lit);
                    n_lit++; out++;
                    if (n_lit == 8) { flush_literals(dst, out, lits, n_lit, lane); n_lit = 0; lits = 0; }
                    continue;
                }
                if (s == 256) { if (bits_over(b)) return MCX_INFLATE_INPUT; break; }
                const uint32_t li = (uint32_t)s - 257;
                if (li >= 29) return bits_over(b) ? MCX_INFLATE_INPUT : MCX_INFLATE_DAMAGED;
                const uint32_t len = len_base(li) + bits_take(b, len_extra(li));
                const uint64_t dleft = (uint64_t)src_len * 8 > bits_pos(b) ? (uint64_t)src_len * 8 - bits_pos(b) : 0;
                const int ds = no_dist ? -1 : decode_sym(b, t.dist_root, kDistRootBits, t.dist_sorted, t.dist_cnt);
                if (ds < 0) return dleft < 15 ? MCX_INFLATE_INPUT : MCX_INFLATE_DAMAGED;
                if (ds >= 30) return bits_over(b) ? MCX_INFLATE_INPUT : MCX_INFLATE_DAMAGED;
                const uint32_t dist = dist_base((uint32_t)ds) + bits_take(b, dist_extra((uint32_t)ds));
                if (bits_over(b)) return MCX_INFLATE_INPUT;
                if (dist > out) return MCX_INFLATE_DAMAGED; // (before the start of the member's text)
                if (len > isize - out) return MCX_INFLATE_LENGTH;
                flush_literals(dst, out, lits, n_lit, lane); n_lit = 0; lits = 0;
                sync_output();
                const uint8_t *from = dst + out - dist;
                for (uint32_t i = lane; i < len; i += kLanes) dst[out + i] = from[i < dist ? i : i % dist];
                out += len;
            }
        }
        if (bfinal) break; // (what follows the final block inside src_len is ignored, as zlib's inflate(Z_FINISH) ignores it)
    }
    flush_literals(dst, out, lits, n_lit, lane);
    if (out != isize) return MCX_INFLATE_LENGTH;
    sync_output();
    return crc_of(dst, isize, crc_tab, lane) == crc ? MCX_INFLATE_OK : MCX_INFLATE_CRC;
}

} // namespace inf
} // namespace mcx
#endif
