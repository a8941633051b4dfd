// mapcaller_amd/csrc/mcx_fastq.h — the reader's rules for FASTQ text (plain, and the .gz readers'), once, for the device (mcx_fastq.hip) and for the host
// (tests/hostemu/fastq_check.cpp).
//
// Restated from MappedFastq::parse and header_of of mcx_reader.h, which every golden SAM pins to the reference (GetNextEntry, GetData.cpp:32-55;
// IdentifyHeaderBegPos / IdentifyHeaderEndPos, :3-20), and from pack_word of the same file:
//   a line     what getline gives: up to and including '\n'; the text's last line may lack it
//   record k   lines 4k .. 4k+3 counted from the text's first byte, whatever they hold
//   name       header_of over the header line with its newline: [p1, p2), empty when p2 <= p1
//   rlen       length of the sequence line less one: the last byte goes whether or not it is a newline
//   quality    the '+' line is skipped; q_take = min(length of the quality line with its newline, rlen), 0 when the line is absent
//   stops      no header line (END); no sequence line or rlen == 0 (EMPTY: what ends the reference's input, GetData.cpp:91); rlen > max_read_len
//   rows       A 0, C 1, G 2, T 3, sixteen bases to a word, the first in the top bits; any other byte has code 0 and is listed
// THE GZ RULE (MCX_FASTQ_RULE_GZ), restated from Parser::line / Parser::entry of mcx_reader.h in gz_mode_ with FASTQ input (gzGetNextEntry: gzgets with a
// 1024-byte buffer, strlen semantics, GetData.cpp:101-128):
//   a piece    what gzgets(buffer, 1024) gives: at s, the bytes up to and including the first '\n' within text[s, s + 1023); without one, those 1023 bytes
//              when there are as many, else the rest of the text (unfinished, the text's last).  The next piece begins right behind: the pieces tile the
//              text as the lines do, a line of L bytes (newline included) in ceil(L / 1023) of them — so the piece table has the line table's form
//   C length   a piece's bytes before its first NUL (strlen), all of them when it has none
//   record k   pieces 4k .. 4k+3.  Header: C length 0 or a first byte other than '@' and '>' ends the input (EMPTY); the name is header_of over the C
//              length.  rlen = C length of the sequence piece less one (0 for 0); q_take = min(C length of the fourth piece, rlen), 0 when it is absent
//   stops      as under the plain rule, with pieces for lines
//   final == 0 a record is taken only when its four pieces are complete: each ends in '\n' or is 1023 bytes long
// FASTA (MCX_READS_FASTA), restated from Parser::entry of mcx_reader.h with FASTA input, which the golden SAMs pin to the reference (GetNextEntry,
// GetData.cpp:56-77; gzGetNextEntry, :101-128).  Lines and pieces are those above.
// PLAIN FASTA:
//   a header   line 0 of the text whatever it holds, and every later line whose first byte is '>'
//   record k   from its header to the next header or the text's end; the name is header_of over the header line
//   sequence   every non-header line less its last byte (newline or not), back to back: an empty line gives nothing, '\r' and a '>' behind a line's first
//              byte are bases, a NUL does not end a line (the host reader copies len - 1 bytes); rlen their sum, q_take = 0
//   stops      no header line (END); rlen == 0 — a header behind a header, a header last — (EMPTY); rlen > max_read_len (TOO_LONG)
//   final == 0 a record is taken only when a later header line has begun inside the text; an unfinished last record that holds more than max_read_len
//              bases already stops with TOO_LONG (a streaming caller makes progress or fails); consumed is the start of the first header line that
//              belongs to no taken record, so a text carried from there begins with a header and gives the same records
//   rec        seq: the first byte behind the header line; rlen the total — the bases are NOT contiguous in the text: take the bases / off group
//   tables     per line L its header flag and payload (fa_line); hn[], bo[] their exclusive sums over lines 0 .. n_lines (the last entry: the totals);
//              hl[k] the line of header k, hl[n_headers] = n_lines — a record's rlen is a difference of two sums
// GZ-RULE FASTA: the GZ rule with record k = pieces 2k, 2k + 1 and no quality (stride 2 for 4 below).
#ifndef MCX_FASTQ_H
#define MCX_FASTQ_H
#include "mcx_types.h"
#include "../../include/mcx.h"

namespace mcx {
namespace fq {

// header_of (mcx_reader.h): l[0 .. len) is the header line with its newline, len >= 1
static inline MCX_HD void header_of(const uint8_t *l, uint32_t len, uint32_t &p1, uint32_t &p2)
{
    const uint32_t lim = len > 100u ? 100u : len;
    p1 = len - 1; p2 = lim - 1;
    for (uint32_t i = 1; i < len; i++) if (l[i] != '>' && l[i] != '@') { p1 = i; break; }
    for (uint32_t i = 1; i < lim; i++) { const uint8_t c = l[i]; if (c <= ' ' || c == '/' || c >= 0x7f) { p2 = i; break; } }
}

// Line L of a text of `bytes` bytes with n_nl newlines, the starts of its lines 0 .. at least L + 1 in ls[] (ls[0] = 0, ls[i] = one past the i-th
// newline): where it begins and how long it is with its newline; false when the text has no such line.
static inline MCX_HD bool line_of(const uint32_t *ls, uint64_t n_nl, uint32_t bytes, uint64_t L, uint32_t &start, uint32_t &len)
{
    if (L > n_nl) return false;
    start = ls[L];
    if (start >= bytes) return false; // (only L == n_nl: the text ends with its last newline)
    len = (L < n_nl ? ls[L + 1] : bytes) - start;
    return true;
}

// Record k of the text: MCX_FASTQ_MORE and the record in rec when it is one to take, else why the text's records end before it.
// The caller has made sure that ls[] holds the starts of lines 0 .. 4k + 4 as far as the text has them.
static inline MCX_HD uint32_t record_of(const uint8_t *text, uint32_t bytes, const uint32_t *ls, uint64_t n_nl, uint32_t k, int32_t max_read_len, mcx_fastq_rec &rec)
{
    const uint64_t L = 4ull * k;
    uint32_t s, len;
    if (!line_of(ls, n_nl, bytes, L, s, len)) return MCX_FASTQ_END;
    uint32_t p1, p2;
    header_of(text + s, len, p1, p2);
    rec.name = s + p1; rec.name_len = p2 > p1 ? p2 - p1 : 0;
    if (!line_of(ls, n_nl, bytes, L + 1, s, len)) return MCX_FASTQ_EMPTY; // no sequence line
    rec.seq = s; rec.rlen = len - 1;
    uint32_t q, ql;
    if (!line_of(ls, n_nl, bytes, L + 3, q, ql)) { q = 0; ql = 0; }
    rec.qual = q; rec.q_take = ql < rec.rlen ? ql : rec.rlen;
    if (rec.rlen == 0) return MCX_FASTQ_EMPTY;
    if ((int64_t)rec.rlen > (int64_t)max_read_len) return MCX_FASTQ_TOO_LONG;
    return MCX_FASTQ_MORE;
}

// with final == 0: record k is taken only when its four lines all end in '\n' inside the text
static inline MCX_HD bool record_whole(uint64_t n_nl, uint32_t k) { return n_nl >= 4ull * k + 4; }

// ---- the GZ rule ----------------------------------------------------------------------------------------------
enum : uint32_t { kGzPiece = 1023 }; // gzgets(buffer, 1024)
// pieces of a line of len bytes (its newline included; the text's last line may lack one), and where piece j of the line that starts at s begins
static inline MCX_HD uint32_t gz_pieces_of(uint32_t len) { return (len + kGzPiece - 1) / kGzPiece; }
static inline MCX_HD uint32_t gz_piece_start(uint32_t s, uint32_t j) { return s + j * kGzPiece; }
// The lines that can hold pieces 0 .. 4 * eff_max: the text's, at most 4 * eff_max of them (every line holds a piece at least).  ls[] as line_of takes it.
static inline MCX_HD uint32_t gz_lines_counted(const uint32_t *ls, uint64_t n_nl, uint32_t bytes, uint32_t eff_max)
{
    const uint64_t cap = 4ull * eff_max;
    if (n_nl >= cap) return (uint32_t)cap;
    return (uint32_t)n_nl + (ls[n_nl] < bytes ? 1u : 0u); // (an unterminated last line counts)
}
// pieces of line L (0 from the counted lines on): what the exclusive sums po[] are taken of
static inline MCX_HD uint32_t gz_line_pieces(const uint32_t *ls, uint64_t n_nl, uint32_t bytes, uint32_t n_counted, uint32_t L)
{
    if (L >= n_counted) return 0;
    return gz_pieces_of((L < n_nl ? ls[L + 1] : bytes) - ls[L]);
}
// Entry q of the piece table, q <= 4 * eff_max: po[0 .. 4 * eff_max] the exclusive sums of gz_line_pieces, their last the number of pieces P.  Piece q < P
// lies in the line found by search over the sums; entry P is the end of the counted lines (where piece P begins, if the text has one); false behind it.
static inline MCX_HD bool gz_piece_entry(const uint32_t *ls, uint64_t n_nl, uint32_t bytes, const uint32_t *po, uint32_t eff_max, uint32_t n_counted, uint32_t q, uint32_t &start)
{
    const uint32_t n = 4u * eff_max, P = po[n];
    if (q > P) return false;
    if (q == P) { start = n_counted <= n_nl ? ls[n_counted] : bytes; return true; }
    uint32_t lo = 0, hi = n_counted; // the last line L < n_counted with po[L] <= q (po rises strictly over the counted lines)
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (po[mid] <= q) lo = mid; else hi = mid; }
    start = gz_piece_start(ls[lo], q - po[lo]);
    return true;
}
// pieces in the table ps[] (ps[that many]: the end of the last one), as the record functions take it in n_nl's place
static inline MCX_HD uint64_t gz_pieces_counted(const uint32_t *po, uint32_t eff_max) { const uint32_t n = 4u * eff_max; return po[n] < n ? po[n] : n; }
static inline MCX_HD uint32_t gz_c_len(const uint8_t *p, uint32_t len, bool any_nul)
{
    if (any_nul) for (uint32_t i = 0; i < len; i++) if (p[i] == 0) return i; // (a text without any NUL does not pay for the search)
    return len;
}
// record_of under the GZ rule: ps[] / n_p the piece table in the place of ls[] / n_nl; any_nul: the text holds a NUL somewhere
// stride: pieces to a record, 4 (FASTQ) or 2 (FASTA: no quality)
static inline MCX_HD uint32_t gz_record_of(const uint8_t *text, uint32_t bytes, const uint32_t *ps, uint64_t n_p, uint32_t k, int32_t max_read_len, bool any_nul, mcx_fastq_rec &rec, uint32_t stride = 4)
{
    const uint64_t L = (uint64_t)stride * k;
    uint32_t s, len;
    if (!line_of(ps, n_p, bytes, L, s, len)) return MCX_FASTQ_END;
    uint32_t cl = gz_c_len(text + s, len, any_nul);
    if (cl == 0 || (text[s] != '@' && text[s] != '>')) return MCX_FASTQ_EMPTY; // (entry() returns false: the input ends)
    uint32_t p1, p2;
    header_of(text + s, cl, p1, p2);
    rec.name = s + p1; rec.name_len = p2 > p1 ? p2 - p1 : 0;
    if (!line_of(ps, n_p, bytes, L + 1, s, len)) return MCX_FASTQ_EMPTY; // no sequence piece
    cl = gz_c_len(text + s, len, any_nul);
    rec.seq = s; rec.rlen = cl ? cl - 1 : 0;
    uint32_t q, ql;
    if (stride == 4 && line_of(ps, n_p, bytes, L + 3, q, ql)) ql = gz_c_len(text + q, ql, any_nul); else { q = 0; ql = 0; }
    rec.qual = q; rec.q_take = ql < rec.rlen ? ql : rec.rlen;
    if (rec.rlen == 0) return MCX_FASTQ_EMPTY;
    if ((int64_t)rec.rlen > (int64_t)max_read_len) return MCX_FASTQ_TOO_LONG;
    return MCX_FASTQ_MORE;
}
// with final == 0: record k is taken only when its four pieces are complete — the first three are when the fourth exists (an unfinished piece is the text's last)
static inline MCX_HD bool gz_record_whole(const uint8_t *text, uint32_t bytes, const uint32_t *ps, uint64_t n_p, uint32_t k, uint32_t stride = 4)
{
    uint32_t s, len;
    if (!line_of(ps, n_p, bytes, (uint64_t)stride * k + stride - 1, s, len)) return false;
    return len == kGzPiece || text[s + len - 1] == '\n';
}

// ---- plain FASTA ----------------------------------------------------------------------------------------------
// lines of the text: its newlines, and an unterminated last line; ls[] holds the starts of lines 0 .. n_nl
static inline MCX_HD uint32_t fa_n_lines(const uint32_t *ls, uint64_t n_nl, uint32_t bytes) { return (uint32_t)n_nl + (ls[n_nl] < bytes ? 1u : 0u); }
// line L: whether it is a header, and the bases it gives (0, 0 from n_lines on: what the exclusive sums are taken of)
static inline MCX_HD void fa_line(const uint8_t *text, uint32_t bytes, const uint32_t *ls, uint64_t n_nl, uint32_t n_lines, uint32_t L, uint32_t &hdr, uint32_t &pay)
{
    hdr = pay = 0;
    if (L >= n_lines) return;
    const uint32_t s = ls[L], len = (L < n_nl ? ls[L + 1] : bytes) - s;
    if (L == 0 || text[s] == '>') hdr = 1; else pay = len - 1;
}
// Record k: why the records end before it, or MCX_FASTQ_MORE — with `taken` when it is one to take (final == 0: not the text's last).  n_hdr = hn[n_lines].
static inline MCX_HD uint32_t fa_record_of(const uint8_t *text, uint32_t bytes, const uint32_t *ls, uint64_t n_nl, const uint32_t *bo, const uint32_t *hl, uint32_t n_hdr, uint32_t k,
                                           int32_t max_read_len, int32_t final, mcx_fastq_rec &rec, bool &taken)
{
    taken = false;
    if (k >= n_hdr) return final ? MCX_FASTQ_END : MCX_FASTQ_MORE;
    const uint32_t h = hl[k], s = ls[h], len = (h < n_nl ? ls[h + 1] : bytes) - s;
    uint32_t p1, p2;
    header_of(text + s, len, p1, p2);
    rec.name = s + p1; rec.name_len = p2 > p1 ? p2 - p1 : 0;
    rec.seq = s + len; rec.rlen = bo[hl[k + 1]] - bo[h]; rec.qual = 0; rec.q_take = 0;
    const bool too_long = (int64_t)rec.rlen > (int64_t)max_read_len;
    if (!final && k + 1 >= n_hdr) return too_long ? MCX_FASTQ_TOO_LONG : MCX_FASTQ_MORE; // (unfinished: more of it may follow)
    if (rec.rlen == 0) return MCX_FASTQ_EMPTY;
    if (too_long) return MCX_FASTQ_TOO_LONG;
    taken = true;
    return MCX_FASTQ_MORE;
}
// the first byte that belongs to none of the n records taken
static inline MCX_HD uint32_t fa_consumed(const uint32_t *ls, const uint32_t *hl, uint32_t n_hdr, uint32_t n, uint32_t bytes) { return n < n_hdr ? ls[hl[n]] : bytes; }

static inline MCX_HD uint32_t code_of(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; } // 4: not upper-case ACGT
static inline MCX_HD uint64_t odd_entry(uint32_t read, uint32_t pos, uint8_t c) { return ((uint64_t)read << 32) | ((uint64_t)pos << 8) | c; }
// bases [i, i + n) of seq, n <= 16, as one word of the row
static inline MCX_HD uint32_t pack_word(const uint8_t *seq, uint32_t i, uint32_t n)
{
    uint32_t w = 0;
    for (uint32_t j = 0; j < n; j++) w |= (code_of(seq[i + j]) & 3u) << (30 - 2 * j);
    return w;
}

} // namespace fq
} // namespace mcx
#endif
