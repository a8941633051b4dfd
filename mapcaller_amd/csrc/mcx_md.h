// mapcaller_amd/csrc/mcx_md.h — one line's MD:Z string from its record, the read and the genome, for the device and (tests/hostemu) for the host.
//
// What `samtools calmd` writes (include/mcx.h says it in full): the line's CIGAR is walked over its printed SEQ (sam_seq_byte) against the forward genome from
// chr_fwd[chr] + pos - 1.  u counts matching columns.  An M / = / X column that matches (bam_nibble of the SEQ byte equals the reference letter's and is not 15)
// adds to u; one that does not writes u, the reference letter, and u = 0.  A D operation writes u, '^', its reference letters, and u = 0.  I and S take read
// bases, N takes reference bases, H and P take nothing; none of them writes or ends a run.  The final u is always written.
// The reference letter is "ACGT"[the pac's two bits], or — inside a hole of the index's .amb file — the hole's own letter in upper case; outside the genome 'N'.
// The pieces (md_pac_code, md_letter, md_matches, md_span, md_holes_of, md_digits, md_put_num) are what k_md (mcx_md.hip) spreads over a wavefront; md_one_len /
// md_one_put put them together for one lane: the host, and what the kernels are held against.
#ifndef MCX_MD_H
#define MCX_MD_H
#include "mcx_bam.h"

namespace mcx {

// the genome as MD sees it: the 2-bit forward text, its length, the contigs' starts, and the ambiguity holes sorted by offset (none: n_holes = 0, never touched)
struct MdRef {
    const uint8_t *pac;
    int64_t G;
    const int64_t *chr_fwd;
    const int64_t *hole_off; const int32_t *hole_len; const uint8_t *hole_letter; uint32_t n_holes;
};

static inline MCX_HD uint32_t md_pac_code(const uint8_t *pac, int64_t g) { return (pac[g >> 2] >> ((~(uint32_t)g & 3u) << 1)) & 3u; } // MSB first
static inline MCX_HD uint32_t md_byte_code(uint8_t byte, int64_t g) { return ((uint32_t)byte >> ((~(uint32_t)g & 3u) << 1)) & 3u; }    // ... of a byte already fetched
static inline MCX_HD uint8_t md_upper(uint8_t c) { return c >= 'a' && c <= 'z' ? (uint8_t)(c - 32) : c; }

// the holes that overlap [g0, g1): [lo, hi) of the table, by one binary search for the first hole that ends behind g0
static inline MCX_HD void md_holes_of(const MdRef &ref, int64_t g0, int64_t g1, uint32_t &lo, uint32_t &hi)
{
    lo = hi = 0;
    if (ref.n_holes == 0) return;
    uint32_t a = 0, b = ref.n_holes;
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (ref.hole_off[m] + ref.hole_len[m] <= g0) a = m + 1; else b = m;
    }
    lo = hi = a;
    while (hi < ref.n_holes && ref.hole_off[hi] < g1) hi++;
}
// the letter of the hole among [lo, hi) that holds g; 0: none does
static inline MCX_HD uint8_t md_hole_letter(const MdRef &ref, uint32_t lo, uint32_t hi, int64_t g)
{
    for (uint32_t h = lo; h < hi; h++)
        if (g >= ref.hole_off[h] && g < ref.hole_off[h] + ref.hole_len[h]) return md_upper(ref.hole_letter[h]);
    return 0;
}
// the reference letter at g: code is the pac's two bits there (not looked at outside the genome or inside a hole)
static inline MCX_HD uint8_t md_letter_of(const MdRef &ref, uint32_t lo, uint32_t hi, int64_t g, uint32_t code)
{
    if (g < 0 || g >= ref.G) return 'N';
    if (lo < hi) { const uint8_t h = md_hole_letter(ref, lo, hi, g); if (h) return h; }
    return (uint8_t)"ACGT"[code & 3u];
}
static inline MCX_HD uint8_t md_letter(const MdRef &ref, uint32_t lo, uint32_t hi, int64_t g)
{
    return md_letter_of(ref, lo, hi, g, g >= 0 && g < ref.G ? md_pac_code(ref.pac, g) : 0u);
}
// the column classifier: does this SEQ byte match this reference letter
static inline MCX_HD bool md_matches(uint8_t seq, uint8_t letter)
{
    const uint8_t a = bam_nibble(seq);
    return a != 15 && a == bam_nibble(letter);
}
// SEQ byte k of the line; a CIGAR that takes more bases than the read has meets 'N' there
static inline MCX_HD uint8_t md_seq(const SamRead &d, const SamTurn &t, uint32_t k) { return k < d.rlen ? sam_seq_byte(d, t, k) : (uint8_t)'N'; }

// what an operation takes: bit 0 read bases, bit 1 reference bases, bit 2 its reference bases are columns of MD (M = X: compared; D: deleted)
static inline MCX_HD uint32_t md_op_takes(uint32_t op)
{
    switch (op) {
    case 0: case 7: case 8: return 7u; // M = X
    case 1: case 4: return 1u;          // I S
    case 2: return 6u;                  // D
    case 3: return 2u;                  // N
    default: return 0u;                 // H P and what BAM does not define
    }
}
// does the line get a tag at all
static inline MCX_HD bool md_has(const mcx_aln &rec) { return rec.chr >= 0 && rec.n_cigar > 0; }
static inline MCX_HD int64_t md_g0(const MdRef &ref, const mcx_aln &rec) { return ref.chr_fwd[rec.chr] + rec.pos - 1; }
// reference bases the CIGAR spans (N included)
static inline MCX_HD int64_t md_span(const uint32_t *cigar, int n)
{
    int64_t len = 0;
    for (int k = 0; k < n; k++) if (md_op_takes(cigar[k] & 15u) & 2u) len += cigar[k] >> 4;
    return len;
}

static inline MCX_HD uint32_t md_digits(uint32_t v) { uint32_t n = 1; while (v >= 10) { v /= 10; n++; } return n; }
static inline MCX_HD uint8_t *md_put_num(uint8_t *o, uint32_t v)
{
    const uint32_t n = md_digits(v);
    for (uint32_t k = n; k-- > 0;) { o[k] = (uint8_t)('0' + v % 10); v /= 10; }
    return o + n;
}

// one line's string by one lane: written at o when o is not null; returns its bytes (0: no tag)
static inline MCX_HD uint32_t md_one_walk(const MdRef &ref, const SamRead &d, const mcx_aln &rec, const uint32_t *cigar, uint8_t *o)
{
    if (!md_has(rec)) return 0;
    const SamTurn t = sam_turn(d, rec);
    const int64_t g0 = md_g0(ref, rec);
    uint32_t lo, hi;
    md_holes_of(ref, g0, g0 + md_span(cigar, rec.n_cigar), lo, hi);
    uint32_t n = 0, u = 0, y = 0;
    int64_t x = g0;
    for (int k = 0; k < rec.n_cigar; k++) {
        const uint32_t len = cigar[k] >> 4, takes = md_op_takes(cigar[k] & 15u);
        if (takes == 7u) {
            for (uint32_t j = 0; j < len; j++) {
                const uint8_t letter = md_letter(ref, lo, hi, x + j);
                if (md_matches(md_seq(d, t, y + j), letter)) { u++; continue; }
                if (o) { uint8_t *e = md_put_num(o + n, u); *e = letter; }
                n += md_digits(u) + 1; u = 0;
            }
        } else if (takes == 6u) {
            if (o) { uint8_t *e = md_put_num(o + n, u); *e++ = '^'; for (uint32_t j = 0; j < len; j++) e[j] = md_letter(ref, lo, hi, x + j); }
            n += md_digits(u) + 1 + len; u = 0;
        }
        if (takes & 1u) y += len;
        if (takes & 2u) x += len;
    }
    if (o) md_put_num(o + n, u);
    return n + md_digits(u);
}
static inline MCX_HD uint32_t md_one_len(const MdRef &ref, const SamRead &d, const mcx_aln &rec, const uint32_t *cigar) { return md_one_walk(ref, d, rec, cigar, nullptr); }
static inline MCX_HD uint8_t *md_one_put(const MdRef &ref, const SamRead &d, const mcx_aln &rec, const uint32_t *cigar, uint8_t *o) { return o + md_one_walk(ref, d, rec, cigar, o); }

// line e of a batch — e < n_reads: read e's own record; else the -m extra e - n_reads — as (read, record, CIGAR)
static inline MCX_HD uint32_t md_n_lines(const mcx_sam_in &in, uint32_t n_extras) { return in.n_reads + n_extras; }
static inline MCX_HD void md_line_of(const mcx_sam_in &in, uint32_t e, uint32_t &r, mcx_aln &rec, const uint32_t *&cigar)
{
    if (e < in.n_reads) { r = e; rec = in.aln[e]; cigar = in.cigar + (uint32_t)rec.cigar_off; return; }
    const uint32_t i = e - in.n_reads;
    uint32_t a = 0, b = in.n_reads; // the last read whose extras begin at or before i (reads without extras in between share the value: take the last)
    while (a < b) {
        const uint32_t m = a + ((b - a) >> 1);
        if (in.x_index[m + 1] <= i) a = m + 1; else b = m;
    }
    r = a < in.n_reads ? a : in.n_reads - 1;
    rec = in.x_recs[i]; cigar = in.x_cigar + (uint32_t)rec.cigar_off;
}

} // namespace mcx
#endif
