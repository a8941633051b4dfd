// mapcaller_amd/csrc/mcx_sam.h — one read's SAM line(s) from its record, for the device and (tests/hostemu) for the host.
//
// GenerateSingleSamStream / GeneratePairedSamStream (reference src/SamReport.cpp:324-488) restated from sam_line(), sam_record()
// and comp_char() of mcx_batch.h, which every golden SAM pins to the reference byte for byte:
//   QNAME \t FLAG \t  then  "*\t0\t0\t*\t*\t0\t0\t"  for an unmapped read, or
//                           RNAME \t POS \t MAPQ \t CIGAR  and  "\t=\t" PNEXT \t TLEN \t  (has_mate)  |  "\t*\t0\t0\t"
//   SEQ \t QUAL  then  "\tNM:i:" nm "\tAS:i:" as "\tXS:i:" xs "\n"  |  "\tAS:i:0\tXS:i:0\n"  (unmapped)
// SEQ: the reference reverse-complements mate 2 in place before mapping (ReadMapping.cpp:451) and prints that string for
// forward-strand hits and unmapped reads, its reverse complement otherwise — flipped = mate 2, again = mapped && !fwd; one of the
// two: reverse complement (anything but ACGTacgt gives N); both: complemented twice in forward order (upper case, N for the rest).
// QUAL: rlen bytes, NUL from where the reference stopped taking the quality line (GetData.cpp:51-52: strncpy); printed with %s —
// forward up to the first NUL, reversed from the last byte backwards up to the first NUL (empty when the line was short).
// The pieces (sam_head_*, sam_tags_*, sam_seq_byte, sam_qual_len) are what k_sam_write (mcx_sam.hip) spreads over a wavefront;
// sam_line_len / sam_line_put put them together for one lane: the length kernel, the lines too long for the LDS staging, the host.
#ifndef MCX_SAM_H
#define MCX_SAM_H
#include "mcx_types.h"
#include "../../include/mcx.h"

namespace mcx {

struct SamContigs { const char *text; const uint32_t *off; }; // the contigs' names back to back; name i is text[off[i] .. off[i + 1])

// what of read r does not depend on the record
struct SamRead {
    const uint8_t *name, *seq, *qual; // qual null: '*'
    uint32_t name_len, rlen;
    bool flipped;                     // mapped as the second read of a pair
};
static inline MCX_HD SamRead sam_read_of(const mcx_sam_in &in, uint32_t r)
{
    SamRead d;
    d.name = in.names + in.name_off[r]; d.name_len = in.name_off[r + 1] - in.name_off[r];
    d.seq = in.bases + in.off[r]; d.rlen = in.off[r + 1] - in.off[r];
    d.qual = in.qual ? in.qual + in.off[r] : nullptr;
    d.flipped = in.paired && (r & 1u);
    return d;
}

static inline MCX_HD uint8_t sam_comp(uint8_t c) // GetComplementaryBase, tools.cpp:3-18
{
    switch (c) {
    case 'A': case 'a': return 'T';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    case 'T': case 't': return 'A';
    default: return 'N';
    }
}

static inline MCX_HD uint32_t sam_num_len(int64_t v)
{
    uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
    uint32_t n = v < 0 ? 2u : 1u;
    while (u >= 10) { u /= 10; n++; }
    return n;
}
static inline MCX_HD uint8_t *sam_num(uint8_t *o, int64_t v)
{
    const uint32_t n = sam_num_len(v);
    uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
    for (uint32_t k = n; k-- > (v < 0 ? 1u : 0u);) { o[k] = (uint8_t)('0' + u % 10); u /= 10; }
    if (v < 0) o[0] = '-';
    return o + n;
}
static inline MCX_HD uint8_t *sam_lit(uint8_t *o, const char *s) { while (*s) *o++ = (uint8_t)*s++; return o; }

// a CIGAR as column 6 prints it (and MC:Z: the mate's, through the same code)
static inline MCX_HD uint32_t sam_cigar_len(const uint32_t *cigar, int n)
{
    uint32_t len = 0;
    for (int k = 0; k < n; k++) len += sam_num_len((int64_t)(cigar[k] >> 4)) + 1;
    return len;
}
static inline MCX_HD uint8_t *sam_cigar_put(uint8_t *o, const uint32_t *cigar, int n)
{
    for (int k = 0; k < n; k++) {
        const uint32_t w = cigar[k];
        o = sam_num(o, (int64_t)(w >> 4)); *o++ = (uint8_t)"MIDNSHP="[w & 7];
    }
    return o;
}

// the fields between QNAME and SEQ, with the tabs around them
static inline MCX_HD uint32_t sam_head_len(const mcx_aln &rec, const uint32_t *cigar, const SamContigs &cn)
{
    uint32_t n = 1 + sam_num_len(rec.flag) + 1;
    if (rec.chr < 0) return n + 14;
    n += cn.off[rec.chr + 1] - cn.off[rec.chr] + 1 + sam_num_len(rec.pos) + 1 + sam_num_len(rec.mapq) + 1;
    n += sam_cigar_len(cigar, rec.n_cigar);
    return n + (rec.has_mate ? 3 + sam_num_len(rec.mate_pos) + 1 + sam_num_len(rec.tlen) + 1 : 7);
}
static inline MCX_HD uint8_t *sam_head_put(const mcx_aln &rec, const uint32_t *cigar, const SamContigs &cn, uint8_t *o)
{
    *o++ = '\t'; o = sam_num(o, rec.flag); *o++ = '\t';
    if (rec.chr < 0) return sam_lit(o, "*\t0\t0\t*\t*\t0\t0\t");
    for (uint32_t k = cn.off[rec.chr]; k < cn.off[rec.chr + 1]; k++) *o++ = (uint8_t)cn.text[k];
    *o++ = '\t'; o = sam_num(o, rec.pos); *o++ = '\t'; o = sam_num(o, rec.mapq); *o++ = '\t';
    o = sam_cigar_put(o, cigar, rec.n_cigar);
    if (!rec.has_mate) return sam_lit(o, "\t*\t0\t0\t");
    o = sam_lit(o, "\t=\t"); o = sam_num(o, rec.mate_pos); *o++ = '\t'; o = sam_num(o, rec.tlen); *o++ = '\t';
    return o;
}

static inline MCX_HD uint32_t sam_tags_len(const mcx_aln &rec)
{
    return rec.chr < 0 ? 15u : 6 + sam_num_len(rec.nm) + 6 + sam_num_len(rec.as) + 6 + sam_num_len(rec.xs) + 1;
}
static inline MCX_HD uint8_t *sam_tags_put(const mcx_aln &rec, uint8_t *o)
{
    if (rec.chr < 0) return sam_lit(o, "\tAS:i:0\tXS:i:0\n");
    o = sam_lit(o, "\tNM:i:"); o = sam_num(o, rec.nm); o = sam_lit(o, "\tAS:i:"); o = sam_num(o, rec.as); o = sam_lit(o, "\tXS:i:"); o = sam_num(o, rec.xs);
    *o++ = '\n';
    return o;
}

// how SEQ and QUAL of a line are turned
struct SamTurn { bool reverse, twice, qual_forward; };
static inline MCX_HD SamTurn sam_turn(const SamRead &d, const mcx_aln &rec)
{
    const bool again = rec.chr >= 0 && rec.fwd == 0; // a second reverse complement for the output
    SamTurn t;
    t.reverse = d.flipped != again; t.twice = d.flipped && again; t.qual_forward = d.flipped == again;
    return t;
}
static inline MCX_HD uint8_t sam_seq_byte(const SamRead &d, const SamTurn &t, uint32_t k) // byte k of SEQ
{
    if (t.reverse) return sam_comp(d.seq[d.rlen - 1 - k]);
    return t.twice ? sam_comp(sam_comp(d.seq[k])) : d.seq[k];
}
static inline MCX_HD uint32_t sam_qual_len(const SamRead &d, const SamTurn &t) // bytes of QUAL
{
    if (!d.qual) return 1;
    uint32_t n = 0;
    if (t.qual_forward) while (n < d.rlen && d.qual[n]) n++;
    else while (n < d.rlen && d.qual[d.rlen - 1 - n]) n++;
    return n;
}
static inline MCX_HD uint8_t sam_qual_byte(const SamRead &d, const SamTurn &t, uint32_t k) // byte k of QUAL, k < sam_qual_len
{
    return !d.qual ? (uint8_t)'*' : t.qual_forward ? d.qual[k] : d.qual[d.rlen - 1 - k];
}

// A line's MD string in the batch's pool (mcx_md.h makes it; include/mcx.h: entry r is read r's own record, n_reads + i the -m extra i): its bytes, 0 without
// a pool or a tag.
static inline MCX_HD uint32_t sam_md_of(const mcx_sam_in &in, uint32_t entry, const uint8_t *&md)
{
    md = nullptr;
    if (!in.md || !in.md_off) return 0;
    md = in.md + in.md_off[entry];
    return in.md_off[entry + 1] - in.md_off[entry];
}

// What a line carries behind XS, in this order (include/mcx.h at mcx_sam_tags): "\tMD:Z:" and the pool's string, copied; "\tMC:Z:" the mate's CIGAR and "\tMQ:i:" its
// MAPQ; "\tRG:Z:" the read group's ID.  The first of them goes over the newline sam_tags_put ended the line with, a newline ends the last.
struct SamTail {
    const uint8_t *md; uint32_t md_len;   // 0: no MD
    const uint32_t *mc; int32_t mc_n, mq; // the mate's CIGAR words and MAPQ; mc_n 0: neither MC nor MQ
    const uint8_t *rg; uint32_t rg_len;   // 0: no RG
};
// read r's own line (extra = false; entry = r) or its -m extra (entry = n_reads + i).  The mate of read r of a batch mapped as pairs is r ^ 1: its record is
// fetched once, here, and only with mate_tags on.  Both tags iff the mate's record is mapped and the line's own FLAG has 0x8 clear; never on an extra.
static inline MCX_HD SamTail sam_tail_of(const mcx_sam_in &in, const mcx_sam_tags &tg, uint32_t entry, uint32_t r, const mcx_aln &own, bool extra)
{
    SamTail t;
    t.md_len = sam_md_of(in, entry, t.md);
    t.mc = nullptr; t.mc_n = 0; t.mq = 0;
    if (tg.mate_tags && in.paired && !extra && (r ^ 1u) < in.n_reads && !(own.flag & 8)) {
        const mcx_aln m = in.aln[r ^ 1u];
        if (m.chr >= 0 && m.n_cigar > 0) { t.mc = in.cigar + (uint32_t)m.cigar_off; t.mc_n = m.n_cigar; t.mq = m.mapq; }
    }
    t.rg = tg.rg_len ? tg.rg : nullptr; t.rg_len = t.rg ? tg.rg_len : 0;
    return t;
}
static inline MCX_HD uint32_t sam_md_len(uint32_t md_len) { return md_len ? 6 + md_len : 0; }
static inline MCX_HD uint32_t sam_mc_len(const SamTail &t) { return t.mc_n ? 6 + sam_cigar_len(t.mc, t.mc_n) + 6 + sam_num_len(t.mq) : 0; }
static inline MCX_HD uint32_t sam_rg_len(uint32_t rg_len) { return rg_len ? 6 + rg_len : 0; }
static inline MCX_HD uint32_t sam_tail_len(const SamTail &t) { return sam_md_len(t.md_len) + sam_mc_len(t) + sam_rg_len(t.rg_len); }
static inline MCX_HD uint8_t *sam_md_lit(uint8_t *o) { return sam_lit(o, "\tMD:Z:"); }
static inline MCX_HD uint8_t *sam_rg_lit(uint8_t *o) { return sam_lit(o, "\tRG:Z:"); }
static inline MCX_HD uint8_t *sam_mc_put(uint8_t *o, const SamTail &t) // "\tMC:Z:" CIGAR "\tMQ:i:" MAPQ (mc_n > 0)
{
    o = sam_cigar_put(sam_lit(o, "\tMC:Z:"), t.mc, t.mc_n);
    return sam_num(sam_lit(o, "\tMQ:i:"), t.mq);
}
static inline MCX_HD uint8_t *sam_tail_put(uint8_t *o, const SamTail &t) // o: behind the line's newline
{
    if (!sam_tail_len(t)) return o;
    o--;
    if (t.md_len) { o = sam_md_lit(o); for (uint32_t k = 0; k < t.md_len; k++) *o++ = t.md[k]; }
    if (t.mc_n) o = sam_mc_put(o, t);
    if (t.rg_len) { o = sam_rg_lit(o); for (uint32_t k = 0; k < t.rg_len; k++) *o++ = t.rg[k]; }
    *o++ = '\n';
    return o;
}

// one line: its bytes; the same written at o (returns the end)
static inline MCX_HD uint64_t sam_one_len(const SamRead &d, const mcx_aln &rec, const uint32_t *cigar, const SamContigs &cn, const SamTail &tail)
{
    return (uint64_t)d.name_len + sam_head_len(rec, cigar, cn) + d.rlen + 1 + sam_qual_len(d, sam_turn(d, rec)) + sam_tags_len(rec) + sam_tail_len(tail);
}
static inline MCX_HD uint8_t *sam_one_put(const SamRead &d, const mcx_aln &rec, const uint32_t *cigar, const SamContigs &cn, uint8_t *o, const SamTail &tail)
{
    for (uint32_t k = 0; k < d.name_len; k++) *o++ = d.name[k];
    o = sam_head_put(rec, cigar, cn, o);
    const SamTurn t = sam_turn(d, rec);
    for (uint32_t k = 0; k < d.rlen; k++) *o++ = sam_seq_byte(d, t, k);
    *o++ = '\t';
    const uint32_t ql = sam_qual_len(d, t);
    for (uint32_t k = 0; k < ql; k++) *o++ = sam_qual_byte(d, t, k);
    return sam_tail_put(sam_tags_put(rec, o), tail);
}

// -m: read r's extra lines (SamReport.cpp:364-488: every further candidate with the best score), none without x_index
static inline MCX_HD void sam_extras_of(const mcx_sam_in &in, uint32_t r, uint32_t &lo, uint32_t &hi)
{
    lo = hi = 0;
    if (in.x_index) { lo = in.x_index[r]; hi = in.x_index[r + 1]; }
}

// read r's line(s): the record of unique mode, then its extras with the same name, bases and quality
static inline MCX_HD uint64_t sam_line_len(const mcx_sam_in &in, const SamContigs &cn, uint32_t r, const mcx_sam_tags &tg = mcx_sam_tags())
{
    const SamRead d = sam_read_of(in, r);
    const mcx_aln rec = in.aln[r];
    uint64_t n = sam_one_len(d, rec, in.cigar + (uint32_t)rec.cigar_off, cn, sam_tail_of(in, tg, r, r, rec, false));
    uint32_t lo, hi;
    sam_extras_of(in, r, lo, hi);
    for (uint32_t i = lo; i < hi; i++) { const mcx_aln x = in.x_recs[i]; n += sam_one_len(d, x, in.x_cigar + (uint32_t)x.cigar_off, cn, sam_tail_of(in, tg, in.n_reads + i, r, x, true)); }
    return n;
}
static inline MCX_HD uint64_t sam_line_put(const mcx_sam_in &in, const SamContigs &cn, uint32_t r, uint8_t *out, const mcx_sam_tags &tg = mcx_sam_tags())
{
    const SamRead d = sam_read_of(in, r);
    const mcx_aln rec = in.aln[r];
    uint8_t *o = sam_one_put(d, rec, in.cigar + (uint32_t)rec.cigar_off, cn, out, sam_tail_of(in, tg, r, r, rec, false));
    uint32_t lo, hi;
    sam_extras_of(in, r, lo, hi);
    for (uint32_t i = lo; i < hi; i++) { const mcx_aln x = in.x_recs[i]; o = sam_one_put(d, x, in.x_cigar + (uint32_t)x.cigar_off, cn, o, sam_tail_of(in, tg, in.n_reads + i, r, x, true)); }
    return (uint64_t)(o - out);
}

} // namespace mcx
#endif
