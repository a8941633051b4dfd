// mapcaller_amd/csrc/mcx_pack.h — ASCII reads -> the packed form of mcx_fm.h's pack_read(), 16 bases at a time.
//
// The arithmetic of k_pack_reads (mcx_pipeline.hip) as host-and-device code, so that a host program can run it over a buffer
// of exactly the batch's size (tests/hostemu/pack_check.cpp).  Everything here reads the bytes through ALIGNED 16-byte words
// of a buffer (`base16`: the batch in HBM, a copy on the host) and touches a word only when it
// holds a byte of the span it was asked for.
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

// four ASCII bytes (first base in the low byte) -> 8 code bits (first base on top) and 4 N flags
// (first base on top); `comp`: complement the bases (mate 2).  nt4_code (mcx_fm.h) on four lanes of
// one register: fold case, A/C/G/T membership by zero-byte tests, (c >> 1) & 3 hashes A0 C1 T2 G3.
// (lower: 4 flags likewise for bytes with bit 5 set — a lower-case letter where the byte is a base at all)
static inline MCX_HD void pack4(uint32_t w, bool comp, uint32_t &codes, uint32_t &flags, uint32_t &lower)
{
    const uint32_t c = w & 0xDFDFDFDFu;
#define MCX_ZERO_BYTES(t) (~((((t) & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | (t) | 0x7F7F7F7Fu)) // 0x80 where a byte is 0
    const uint32_t member = (MCX_ZERO_BYTES(c ^ 0x41414141u) | MCX_ZERO_BYTES(c ^ 0x43434343u) | MCX_ZERO_BYTES(c ^ 0x47474747u) | MCX_ZERO_BYTES(c ^ 0x54545454u)) >> 7; // 0x01 per base
#undef MCX_ZERO_BYTES
    const uint32_t h = (c >> 1) & 0x03030303u;
    uint32_t code = h ^ ((h >> 1) & 0x01010101u);
    if (comp) code ^= 0x03030303u;
    code &= member * 3u;
    const uint32_t y = __builtin_bswap32(code), n = __builtin_bswap32(member ^ 0x01010101u);
    codes = (y | (y >> 6) | (y >> 12) | (y >> 18)) & 0xFFu;
    flags = (n | (n >> 7) | (n >> 14) | (n >> 21)) & 0xFu;
    const uint32_t l = __builtin_bswap32((w >> 5) & 0x01010101u);
    lower = (l | (l >> 7) | (l >> 14) | (l >> 21)) & 0xFu;
}

// 16 oriented bases i0 .. i0+15 of a read of rlen bytes that starts at byte A0 of base16 -> (code word, MSB first; 16 N flags,
// bit 15 = base i0); bases past the read end give code 0 and flag 1; odd: 16 flags likewise for bytes of the read that are not
// an upper-case A C G T (what the -vcf bookkeeping asks of a read: mcx_profile.h), 0 past the read end
static inline MCX_HD void pack16_span(const U4 *base16, uint64_t A0, int rlen, int flipped, int i0, uint32_t &codes, uint32_t &flags, uint32_t &odd)
{
    int n = rlen - i0; if (n > 16) n = 16;
    codes = 0; flags = 0xFFFFu; odd = 0;
    if (n <= 0) return;
    // the span of the file's bytes under these bases: forward [i0, i0+n); mate 2 (reverse-complemented) [rlen-i0-n, rlen-i0) backwards
    const int a0 = flipped ? rlen - i0 - n : i0;
    U4 v = load16_span(base16, A0 + (uint64_t)a0, n);
    if (flipped) { // byte order reversed: the span's last byte first
        const U4 t = v;
        v.x = __builtin_bswap32(t.w); v.y = __builtin_bswap32(t.z); v.z = __builtin_bswap32(t.y); v.w = __builtin_bswap32(t.x);
    }
    uint32_t c0, f0, c1, f1, c2, f2, c3, f3, l0, l1, l2, l3;
    pack4(v.x, flipped != 0, c0, f0, l0); pack4(v.y, flipped != 0, c1, f1, l1); pack4(v.z, flipped != 0, c2, f2, l2); pack4(v.w, flipped != 0, c3, f3, l3);
    uint32_t c = (c0 << 24) | (c1 << 16) | (c2 << 8) | c3, f = (f0 << 12) | (f1 << 8) | (f2 << 4) | f3, o = f | (l0 << 12) | (l1 << 8) | (l2 << 4) | l3;
    if (n < 16) {
        const int pad = 16 - n;
        if (flipped) { c <<= 2 * pad; f = (f << pad) & 0xFFFFu; o = (o << pad) & 0xFFFFu; } // the n bytes sat at the end of the reversed vector
        else { c &= ~0u << (2 * pad); o &= ~0u << pad; }
        f |= (1u << pad) - 1u;
        if (!flipped) f &= 0xFFFFu;
    }
    codes = c; flags = f; odd = o & 0xFFFFu;
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
static inline MCX_HD void pack_unit32(const U4 *base16, uint64_t A0, int rlen, int flipped, int m, uint32_t *row, uint32_t &has_n, uint32_t &odd)
{
    const int nc = (rlen + 15) >> 4;
    uint32_t c0, f0, c1, f1, o0, o1;
    pack16_span(base16, A0, rlen, flipped, 32 * m, c0, f0, o0);
    pack16_span(base16, A0, rlen, flipped, 32 * m + 16, c1, f1, o1);
    row[2 * m] = c0;
    if (2 * m + 1 < nc) row[2 * m + 1] = c1;
    row[nc + 1 + m] = (f0 << 16) | f1;
    const int left = rlen - 32 * m; // bases of this mask word inside the read (bit 31 = the first)
    has_n = ((f0 << 16) | f1) & (left >= 32 ? ~0u : ~(0xFFFFFFFFu >> left));
    odd = o0 | o1;
}

} // namespace mcx
#endif
