// mapcaller_amd/csrc/mcx_bam.h — one read's BAM record(s) from its record, for the device and (tests/hostemu) for the host.
//
// The reference's -bam hands every SAM line it would print to htslib 1.5's sam_parse1 and writes what comes back with sam_write1 (src/ReadMapping.cpp:548-606;
// the parser: src/htslib/sam.c:940-1100, the binning: hts.h hts_reg2bin).  The line is mcx_sam.h's, so the record is a function of the same mcx_aln and read —
// restated here without the detour through text, all little-endian, never aligned:
//   block_size (the bytes behind it)  refID  pos  | l_read_name  mapq  bin(16) | n_cigar_op(16)  flag(16) | l_seq  next_refID  next_pos  tlen      36 bytes
//   QNAME NUL   CIGAR words   SEQ, two bases a byte   QUAL   tags
//   mapped (chr >= 0):  refID chr, pos - 1, mapq and flag as they are, the pool's words (len << 4 | op: BAM's own), NM AS XS
//   unmapped:           refID -1, pos -1, mapq 0, flag | 4, no CIGAR, AS 0, XS 0 (the line says "*\t0\t0\t*")
//   bin: the UCSC bin of [pos0, pos0 + reference length), the M/D/N/=/X lengths summed; an unmapped line's length is 1 (bin 4680)
//   mate: has_mate and mate_pos >= 1: refID again, mate_pos - 1, tlen; else -1, -1, 0
//   SEQ: byte k of the line's SEQ (sam_seq_byte: reversal, complement, twice-complement applied) as its 4-bit code, the first of a byte in the high nibble
//   QUAL: byte k of the line's QUAL (sam_qual_byte) - 33; 0xff throughout where the line's QUAL is '*' — no qualities, or a quality line that is that one byte
//   tags: 2 letters, a type, the value — the smallest integer type that holds it, unsigned for values >= 0 (C S I), signed below (c s i)
// A line sam_parse1 rejects makes no record: a QNAME of 252 bytes or more ("query name too long"), a QUAL that is not '*' and whose printed length
// (sam_qual_len) is not rlen ("SEQ and QUAL are of different length").  That a mapped line's CIGAR takes rlen bases of the read is the pipeline's
// invariant, not tested here.  No padding NULs behind QNAME: htslib pads in memory only.
// The pieces (bam_fixed_put, bam_tags_*, bam_nibble, bam_qual_out) are what k_bam_write (mcx_bam.hip) spreads over a wavefront; bam_one_len / bam_one_put put
// them together for one lane: the length kernel and the host.
#ifndef MCX_BAM_H
#define MCX_BAM_H
#include "mcx_sam.h"

namespace mcx {

enum { kBamFixed = 36, kBamMaxName = 251 }; // block_size and the 32 bytes of the core; the longest QNAME htslib takes

// the 4-bit code of a SEQ byte: its place in "=ACMGRSVTWYHKDBN" whatever its case, 1 2 4 8 for the digits 0 1 2 3, 15 for anything else
static inline MCX_HD uint8_t bam_nibble(uint8_t c)
{
    if (c == '=') return 0;
    if (c >= '0' && c <= '3') return (uint8_t)(1u << (c - '0'));
    switch (c | 0x20) { // (only letters reach a case: no other byte comes to lie in 'a'..'z')
    case 'a': return 1;  case 'c': return 2;  case 'm': return 3;  case 'g': return 4;  case 'r': return 5;
    case 's': return 6;  case 'v': return 7;  case 't': return 8;  case 'w': return 9;  case 'y': return 10;
    case 'h': return 11; case 'k': return 12; case 'd': return 13; case 'b': return 14;
    default: return 15;
    }
}

// the UCSC bin of [beg, end), 0-based: 14-bit windows at the finest of 5 levels below the root, each level 8 times as wide
static inline MCX_HD uint16_t bam_bin(int64_t beg, int64_t end)
{
    --end;
    int64_t first = 4681; // ((1 << 15) - 1) / 7: the finest level's first bin
    int shift = 14;
    for (int level = 5; level > 0; level--) {
        if ((beg >> shift) == (end >> shift)) return (uint16_t)(first + (beg >> shift));
        shift += 3;
        first -= (int64_t)1 << (3 * (level - 1));
    }
    return 0;
}
// reference bases a CIGAR spans: M D N = X
static inline MCX_HD int64_t bam_ref_len(const uint32_t *cigar, int n)
{
    int64_t len = 0;
    for (int k = 0; k < n; k++) {
        const uint32_t op = cigar[k] & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) len += cigar[k] >> 4;
    }
    return len;
}

static inline MCX_HD uint8_t *bam_le16(uint8_t *o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); return o + 2; }
static inline MCX_HD uint8_t *bam_le32(uint8_t *o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); o[3] = (uint8_t)(v >> 24); return o + 4; }

// an integer tag: 3 bytes and its value's 1, 2 or 4
static inline MCX_HD uint32_t bam_tag_len(int32_t v) { return v >= 0 ? (v <= 255 ? 4u : v <= 65535 ? 5u : 7u) : (v >= -128 ? 4u : v >= -32768 ? 5u : 7u); }
static inline MCX_HD uint8_t *bam_tag_put(uint8_t *o, char a, char b, int32_t v)
{
    *o++ = (uint8_t)a; *o++ = (uint8_t)b;
    if (v >= 0) {
        if (v <= 255) { *o++ = 'C'; *o++ = (uint8_t)v; return o; }
        if (v <= 65535) { *o++ = 'S'; return bam_le16(o, (uint32_t)v); }
        *o++ = 'I';
        return bam_le32(o, (uint32_t)v);
    }
    if (v >= -128) { *o++ = 'c'; *o++ = (uint8_t)v; return o; }
    if (v >= -32768) { *o++ = 's'; return bam_le16(o, (uint32_t)v); }
    *o++ = 'i';
    return bam_le32(o, (uint32_t)v);
}
static inline MCX_HD uint32_t bam_tags_len(const mcx_aln &rec)
{
    return rec.chr < 0 ? 8u : bam_tag_len(rec.nm) + bam_tag_len(rec.as) + bam_tag_len(rec.xs);
}
static inline MCX_HD uint8_t *bam_tags_put(const mcx_aln &rec, uint8_t *o)
{
    if (rec.chr < 0) { o = bam_tag_put(o, 'A', 'S', 0); return bam_tag_put(o, 'X', 'S', 0); }
    o = bam_tag_put(o, 'N', 'M', rec.nm); o = bam_tag_put(o, 'A', 'S', rec.as);
    return bam_tag_put(o, 'X', 'S', rec.xs);
}

// CIGAR operations of the record: an unmapped line has none
static inline MCX_HD uint32_t bam_n_cigar(const mcx_aln &rec) { return rec.chr < 0 || rec.n_cigar < 0 ? 0u : (uint32_t)rec.n_cigar; }

// what a line's QUAL comes to: '*' (0xff throughout), or its bytes; ql = sam_qual_len
static inline MCX_HD bool bam_qual_star(const SamRead &d, const SamTurn &t, uint32_t ql) { return !d.qual || (ql == 1 && sam_qual_byte(d, t, 0) == '*'); }
static inline MCX_HD bool bam_keep_ql(const SamRead &d, const SamTurn &t, uint32_t ql) { return d.name_len <= (uint32_t)kBamMaxName && (bam_qual_star(d, t, ql) || ql == d.rlen); }
static inline MCX_HD bool bam_keep(const SamRead &d, const mcx_aln &rec)
{
    const SamTurn t = sam_turn(d, rec);
    return bam_keep_ql(d, t, sam_qual_len(d, t));
}

// where the pieces of a kept record lie, from its first byte
struct BamLayout { uint32_t cigar_at, seq_at, qual_at, tags_at, total; };
// the tags behind XS (SamTail; include/mcx.h at mcx_sam_tags): 'M' 'D' 'Z' the pool's string NUL; 'M' 'C' 'Z' the mate's CIGAR as text NUL, MQ as bam_tag_put makes it;
// 'R' 'G' 'Z' the ID NUL
static inline MCX_HD uint32_t bam_md_len(uint32_t md_len) { return md_len ? 4 + md_len : 0; }
static inline MCX_HD uint32_t bam_mc_len(const SamTail &t) { return t.mc_n ? 4 + sam_cigar_len(t.mc, t.mc_n) + bam_tag_len(t.mq) : 0; }
static inline MCX_HD uint32_t bam_rg_len(uint32_t rg_len) { return rg_len ? 4 + rg_len : 0; }
static inline MCX_HD uint32_t bam_tail_len(const SamTail &t) { return bam_md_len(t.md_len) + bam_mc_len(t) + bam_rg_len(t.rg_len); }
static inline MCX_HD uint8_t *bam_mc_put(uint8_t *o, const SamTail &t) // (mc_n > 0)
{
    *o++ = 'M'; *o++ = 'C'; *o++ = 'Z';
    o = sam_cigar_put(o, t.mc, t.mc_n);
    *o++ = 0;
    return bam_tag_put(o, 'M', 'Q', t.mq);
}
static inline MCX_HD uint8_t *bam_tail_put(uint8_t *o, const SamTail &t)
{
    if (t.md_len) {
        *o++ = 'M'; *o++ = 'D'; *o++ = 'Z';
        for (uint32_t k = 0; k < t.md_len; k++) *o++ = t.md[k];
        *o++ = 0;
    }
    if (t.mc_n) o = bam_mc_put(o, t);
    if (t.rg_len) {
        *o++ = 'R'; *o++ = 'G'; *o++ = 'Z';
        for (uint32_t k = 0; k < t.rg_len; k++) *o++ = t.rg[k];
        *o++ = 0;
    }
    return o;
}
static inline MCX_HD BamLayout bam_layout(const SamRead &d, const mcx_aln &rec, const SamTail &tail)
{
    BamLayout l;
    l.cigar_at = (uint32_t)kBamFixed + d.name_len + 1;
    l.seq_at = l.cigar_at + 4 * bam_n_cigar(rec);
    l.qual_at = l.seq_at + (d.rlen + 1) / 2;
    l.tags_at = l.qual_at + d.rlen;
    l.total = l.tags_at + bam_tags_len(rec) + bam_tail_len(tail);
    return l;
}

// the 36 bytes ahead of QNAME
static inline MCX_HD void bam_fixed_put(const SamRead &d, const mcx_aln &rec, const uint32_t *cigar, uint32_t total, uint8_t *o)
{
    const bool mapped = rec.chr >= 0;
    const uint32_t nc = bam_n_cigar(rec);
    const int64_t pos0 = mapped ? rec.pos - 1 : -1;
    const bool mate = mapped && rec.has_mate && rec.mate_pos >= 1;
    o = bam_le32(o, total - 4);
    o = bam_le32(o, (uint32_t)(mapped ? rec.chr : -1));
    o = bam_le32(o, (uint32_t)pos0);
    *o++ = (uint8_t)(d.name_len + 1);
    *o++ = (uint8_t)(mapped ? rec.mapq : 0);
    o = bam_le16(o, bam_bin(pos0, pos0 + (mapped && nc ? bam_ref_len(cigar, (int)nc) : 1)));
    o = bam_le16(o, nc);
    o = bam_le16(o, (uint32_t)(mapped ? rec.flag : rec.flag | 4));
    o = bam_le32(o, d.rlen);
    o = bam_le32(o, (uint32_t)(mate ? rec.chr : -1));
    o = bam_le32(o, (uint32_t)(mate ? rec.mate_pos - 1 : -1));
    bam_le32(o, (uint32_t)(mate ? rec.tlen : 0));
}
static inline MCX_HD uint8_t bam_cigar_byte(const uint32_t *cigar, uint32_t k) { return (uint8_t)(cigar[k >> 2] >> (8 * (k & 3u))); } // byte k of the words
static inline MCX_HD uint8_t bam_seq_out(const SamRead &d, const SamTurn &t, uint32_t k) // byte k of the packed SEQ: bases 2k and 2k + 1
{
    const uint8_t hi = bam_nibble(sam_seq_byte(d, t, 2 * k));
    return (uint8_t)(hi << 4 | (2 * k + 1 < d.rlen ? bam_nibble(sam_seq_byte(d, t, 2 * k + 1)) : 0));
}
static inline MCX_HD uint8_t bam_qual_out(const SamRead &d, const SamTurn &t, bool star, uint32_t k) { return star ? (uint8_t)0xff : (uint8_t)(sam_qual_byte(d, t, k) - 33); }

// one line's record: its bytes (0: the line is dropped); the same written at o (returns the end)
static inline MCX_HD uint64_t bam_one_len(const SamRead &d, const mcx_aln &rec, const SamTail &tail)
{
    return bam_keep(d, rec) ? bam_layout(d, rec, tail).total : 0;
}
static inline MCX_HD uint8_t *bam_one_put(const SamRead &d, const mcx_aln &rec, const uint32_t *cigar, uint8_t *o, const SamTail &tail)
{
    const SamTurn t = sam_turn(d, rec);
    const uint32_t ql = sam_qual_len(d, t);
    if (!bam_keep_ql(d, t, ql)) return o;
    const bool star = bam_qual_star(d, t, ql);
    const BamLayout l = bam_layout(d, rec, tail);
    bam_fixed_put(d, rec, cigar, l.total, o);
    for (uint32_t k = 0; k < d.name_len; k++) o[kBamFixed + k] = d.name[k];
    o[kBamFixed + d.name_len] = 0;
    for (uint32_t k = l.cigar_at; k < l.seq_at; k++) o[k] = bam_cigar_byte(cigar, k - l.cigar_at);
    for (uint32_t k = l.seq_at; k < l.qual_at; k++) o[k] = bam_seq_out(d, t, k - l.seq_at);
    for (uint32_t k = 0; k < d.rlen; k++) o[l.qual_at + k] = bam_qual_out(d, t, star, k);
    return bam_tail_put(bam_tags_put(rec, o + l.tags_at), tail);
}

// read r's record(s): the record of unique mode, then its extras' with the same name, bases and quality; *dropped: the lines among them that made none
static inline MCX_HD uint64_t bam_rec_len(const mcx_sam_in &in, uint32_t r, uint32_t *dropped, const mcx_sam_tags &tg = mcx_sam_tags())
{
    const SamRead d = sam_read_of(in, r);
    const mcx_aln rec = in.aln[r];
    uint64_t n = bam_one_len(d, rec, sam_tail_of(in, tg, r, r, rec, false));
    uint32_t none = n ? 0u : 1u, lo, hi;
    sam_extras_of(in, r, lo, hi);
    for (uint32_t i = lo; i < hi; i++) { const mcx_aln x = in.x_recs[i]; const uint64_t m = bam_one_len(d, x, sam_tail_of(in, tg, in.n_reads + i, r, x, true)); n += m; none += m ? 0u : 1u; }
    *dropped = none;
    return n;
}
static inline MCX_HD uint64_t bam_rec_put(const mcx_sam_in &in, uint32_t r, uint8_t *out, const mcx_sam_tags &tg = mcx_sam_tags())
{
    const SamRead d = sam_read_of(in, r);
    const mcx_aln rec = in.aln[r];
    uint8_t *o = bam_one_put(d, rec, in.cigar + (uint32_t)rec.cigar_off, out, sam_tail_of(in, tg, r, r, rec, false));
    uint32_t lo, hi;
    sam_extras_of(in, r, lo, hi);
    for (uint32_t i = lo; i < hi; i++) { const mcx_aln x = in.x_recs[i]; o = bam_one_put(d, x, in.x_cigar + (uint32_t)x.cigar_off, o, sam_tail_of(in, tg, in.n_reads + i, r, x, true)); }
    return (uint64_t)(o - out);
}

} // namespace mcx
#endif
