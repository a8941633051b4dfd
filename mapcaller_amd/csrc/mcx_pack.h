// mapcaller_amd/csrc/mcx_pack.h — ASCII reads -> the packed form of mcx_fm.h's pack_read(), 16 bases at a time.
//
// The arithmetic of k_pack_reads (mcx_pipeline.hip) as host-and-device code, so that a host program can run it over a buffer
// of exactly the batch's size (tests/hostemu/pack_check.cpp, pack4_check.cpp).  A read of 16 bytes or more is read 16 bytes at a
// time from byte addresses of its own and never outside its own bytes; a shorter one through the ALIGNED 16-byte words of the
// buffer (`base16`: the batch in HBM, a copy on the host) that hold a byte of it, and no other word.
#ifndef MCX_PACK_H
#define MCX_PACK_H
#include "mcx_fm.h"

namespace mcx {

// bytes b .. b+3 of the eight bytes lo (first), hi
static inline MCX_HD uint32_t pack_alignbyte(uint32_t hi, uint32_t lo, unsigned b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, b);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (b & 3)));
#endif
}

// the 16 bytes from byte A of base16 on, of which the first n (1..16) are wanted: the aligned word that holds byte A, and the
// next one only where a wanted byte lies in it (the other bytes of the result are unspecified)
static inline MCX_HD U4 load16_span(const U4 *base16, uint64_t A, int n)
{
    const U4 *q = base16 + (A >> 4);
    const U4 lo = q[0];
    const unsigned sh = (unsigned)(A & 15);
    if (sh == 0) return lo;
    U4 hi; hi.x = hi.y = hi.z = hi.w = 0;
    if ((int)sh + n > 16) hi = q[1];
    const unsigned qd = sh >> 2, b = sh & 3;
    uint32_t s0, s1, s2, s3, s4;
    switch (qd) {
    case 0: s0 = lo.x; s1 = lo.y; s2 = lo.z; s3 = lo.w; s4 = hi.x; break;
    case 1: s0 = lo.y; s1 = lo.z; s2 = lo.w; s3 = hi.x; s4 = hi.y; break;
    case 2: s0 = lo.z; s1 = lo.w; s2 = hi.x; s3 = hi.y; s4 = hi.z; break;
    default: s0 = lo.w; s1 = hi.x; s2 = hi.y; s3 = hi.z; s4 = hi.w; break;
    }
    U4 r;
    r.x = pack_alignbyte(s1, s0, b); r.y = pack_alignbyte(s2, s1, b);
    r.z = pack_alignbyte(s3, s2, b); r.w = pack_alignbyte(s4, s3, b);
    return r;
}

// bytes of the eight bytes lo (bytes 0-3), hi (bytes 4-7) picked by the four selector bytes of sel, each 0..7 (v_perm_b32)
static inline MCX_HD uint32_t pack_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; k++) r |= (uint32_t)((v >> (8 * ((sel >> (8 * k)) & 7u))) & 0xFFu) << (8 * k);
    return r;
#endif
}

// the 16 bytes from p on, p at any alignment (one global_load_dwordx4 on gfx950)
static inline MCX_HD U4 load16_bytes(const uint8_t *p)
{
    U4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// v, behind a fence for the optimiser: it would fold the two shift-and-ors of a gather below back into one 32-bit multiplication, which
// the vector unit issues at a quarter of their rate
static inline MCX_HD uint32_t pack_keep(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    return v;
}

// four ASCII bytes (first base in the low byte) -> 8 code bits (first base on top) and 4 N flags
// (first base on top); `comp`: complement the bases (mate 2).  nt4_code (mcx_fm.h) on four lanes of
// one register, by two byte-permute look-ups under the letter's low three bits: those are 1 for A, 3 for C, 4 for T and 7 for G in
// either case, so the first look-up fetches the letter they promise (0xFF elsewhere: no case-folded byte equals it) and the xor with
// the case-folded byte is zero exactly for a base; the second fetches the code, or its complement.  The four codes and the four
// flags are gathered by a multiplication each (x 0x40100401 and x 0x08040201, written as two shift-and-ors: the partial products
// lie on disjoint bits), which also puts the first base on top.
// (lower, kOdd only: 4 flags likewise for bytes with bit 5 set — a lower-case letter where the byte is a base at all)
template <bool kOdd>
static inline MCX_HD void pack4(uint32_t w, bool comp, uint32_t &codes, uint32_t &flags, uint32_t &lower)
{
    const uint32_t c = w & 0xDFDFDFDFu, k = w & 0x07070707u;
    const uint32_t x = c ^ pack_perm(0x47FFFF54u, 0x43FF41FFu, k);                          // G . . T | C . A .
    const uint32_t n = ((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) >> 7) & 0x01010101u;        // 0x01 where the byte is no base
    const uint32_t code = pack_perm(comp ? 0x01000000u : 0x02000003u, comp ? 0x02000300u : 0x01000000u, k) & ~(n * 3u);
    uint32_t y = pack_keep(code | (code << 10)); y |= y << 20;
    uint32_t f = pack_keep(n | (n << 9)); f |= f << 18;
    codes = y >> 24;
    flags = f >> 24;
    if (kOdd) {
        const uint32_t b = (w >> 5) & 0x01010101u;
        uint32_t l = pack_keep(b | (b << 9)); l |= l << 18;
        lower = l >> 24;
    } else lower = 0;
}

// the 16 bytes of a span as loaded (its n wanted bytes, pad = 16 - n others: at_end — the wanted ones are the last n of the vector as packed, that is after
// mate 2's reversal; otherwise the first n) -> code word, N flags and odd flags of pack16_span
template <bool kOdd>
static inline MCX_HD void pack16_vec(U4 v, int flipped, int pad, bool at_end, uint32_t &codes, uint32_t &flags, uint32_t &odd)
{
    if (flipped) { // byte order reversed: the span's last byte first
        const U4 t = v;
        v.x = __builtin_bswap32(t.w); v.y = __builtin_bswap32(t.z); v.z = __builtin_bswap32(t.y); v.w = __builtin_bswap32(t.x);
    }
    uint32_t c0, f0, c1, f1, c2, f2, c3, f3, l0, l1, l2, l3;
    pack4<kOdd>(v.x, flipped != 0, c0, f0, l0); pack4<kOdd>(v.y, flipped != 0, c1, f1, l1); pack4<kOdd>(v.z, flipped != 0, c2, f2, l2); pack4<kOdd>(v.w, flipped != 0, c3, f3, l3);
    uint32_t c = (c0 << 24) | (c1 << 16) | (c2 << 8) | c3, f = (f0 << 12) | (f1 << 8) | (f2 << 4) | f3, o = kOdd ? f | (l0 << 12) | (l1 << 8) | (l2 << 4) | l3 : 0u;
    if (at_end) { c <<= 2 * pad; f = ((f << pad) & 0xFFFFu) | ((1u << pad) - 1u); o = (o << pad) & 0xFFFFu; } // (pad 0: a whole span)
    else { c &= ~0u << (2 * pad); o &= ~0u << pad; f = (f | ((1u << pad) - 1u)) & 0xFFFFu; }
    codes = c; flags = f; odd = o & 0xFFFFu;
}

// where in a read of 16 bytes or more the 16 bytes under bases i0 .. i0+n-1 (n in 1..16) are fetched: a whole span at its own first byte, the read's last
// bases (n < 16) in the 16 bytes that end with them (forward) or begin with them (mate 2: the read's first bytes) — never a byte outside the read; the n
// wanted bytes then lie at the end of the vector as packed
static inline MCX_HD int pack_span_at(int rlen, int flipped, int i0, int n)
{
    return flipped ? rlen - i0 - n : i0 - (16 - n);
}

// 16 oriented bases i0 .. i0+15 of a read of rlen bytes that starts at byte A0 of base16 -> (code word, MSB first; 16 N flags,
// bit 15 = base i0); bases past the read end give code 0 and flag 1; odd (kOdd; 0 without): 16 flags likewise for bytes of the read
// that are not an upper-case A C G T (what the -vcf bookkeeping asks of a read: mcx_profile.h), 0 past the read end.
// A read of 16 bytes or more is fetched 16 bytes at a time from byte addresses of its own (pack_span_at), so that one path serves every
// span of such a read, whole or not.  A shorter read goes through load16_span.
template <bool kOdd = true>
static inline MCX_HD void pack16_span(const U4 *base16, uint64_t A0, int rlen, int flipped, int i0, uint32_t &codes, uint32_t &flags, uint32_t &odd)
{
    int n = rlen - i0; if (n > 16) n = 16;
    codes = 0; flags = 0xFFFFu; odd = 0;
    if (n <= 0) return;
    if (rlen >= 16) pack16_vec<kOdd>(load16_bytes((const uint8_t *)base16 + A0 + (uint64_t)pack_span_at(rlen, flipped, i0, n)), flipped, 16 - n, true, codes, flags, odd);
    else // the span of the file's bytes under these bases: forward [i0, i0+n); mate 2 (reverse-complemented) [rlen-i0-n, rlen-i0) backwards
        pack16_vec<kOdd>(load16_span(base16, A0 + (uint64_t)(flipped ? rlen - i0 - n : i0), n), flipped, 16 - n, flipped != 0, codes, flags, odd);
}

// the two words of a row that depend on the read's length alone: the zero word behind the codes, the all-ones word behind the masks
static inline MCX_HD void pack_row_ends(int rlen, uint32_t *row)
{
    const int nc = (rlen + 15) >> 4, nmw = (rlen + 31) >> 5;
    row[nc] = 0u;
    row[nc + 1 + nmw] = 0xFFFFFFFFu;
}

// bases 32 m .. 32 m + 31 of a read (m < (rlen + 31) / 32) into its row: two code words (one where the read ends in the first)
// and mask word m.  has_n: flags of bases inside the read; odd: as pack16_span's, of both halves
template <bool kOdd = true>
static inline MCX_HD void pack_unit32(const U4 *base16, uint64_t A0, int rlen, int flipped, int m, uint32_t *row, uint32_t &has_n, uint32_t &odd)
{
    const int nc = (rlen + 15) >> 4;
    uint32_t c0, f0, c1, f1, o0, o1;
    if (rlen >= 16) { // both spans' bytes are asked for before either is packed (a part without a second span fetches the first one's again)
        const uint8_t *p = (const uint8_t *)base16 + A0;
        const int i0 = 32 * m, left1 = rlen - i0 - 16, n0 = left1 >= 0 ? 16 : rlen - i0, n1 = left1 > 16 ? 16 : left1;
        const U4 v0 = load16_bytes(p + pack_span_at(rlen, flipped, i0, n0));
        const U4 v1 = load16_bytes(p + (n1 > 0 ? pack_span_at(rlen, flipped, i0 + 16, n1) : pack_span_at(rlen, flipped, i0, n0)));
        pack16_vec<kOdd>(v0, flipped, 16 - n0, true, c0, f0, o0);
        pack16_vec<kOdd>(v1, flipped, n1 > 0 ? 16 - n1 : 0, true, c1, f1, o1);
        if (n1 <= 0) { c1 = 0; f1 = 0xFFFFu; o1 = 0; }
    } else {
        pack16_span<kOdd>(base16, A0, rlen, flipped, 32 * m, c0, f0, o0);
        pack16_span<kOdd>(base16, A0, rlen, flipped, 32 * m + 16, c1, f1, o1);
    }
    row[2 * m] = c0;
    if (2 * m + 1 < nc) row[2 * m + 1] = c1;
    row[nc + 1 + m] = (f0 << 16) | f1;
    const int left = rlen - 32 * m; // bases of this mask word inside the read (bit 31 = the first)
    has_n = ((f0 << 16) | f1) & (left >= 32 ? ~0u : ~(0xFFFFFFFFu >> left));
    odd = o0 | o1;
}

} // namespace mcx
#endif
