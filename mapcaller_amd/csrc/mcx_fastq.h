// mapcaller_amd/csrc/mcx_fastq.h — the reader's rules for plain FASTQ text, once, for the device (mcx_fastq.hip) and for the host
// (tests/hostemu/fastq_check.cpp).
//
// Restated from MappedFastq::parse and header_of of mcx_files.cpp, which every golden SAM pins to the reference (GetNextEntry, GetData.cpp:32-55;
// IdentifyHeaderBegPos / IdentifyHeaderEndPos, :3-20), and from pack_word of the same file:
//   a line     what getline gives: up to and including '\n'; the text's last line may lack it
//   record k   lines 4k .. 4k+3 counted from the text's first byte, whatever they hold
//   name       header_of over the header line with its newline: [p1, p2), empty when p2 <= p1
//   rlen       length of the sequence line less one: the last byte goes whether or not it is a newline
//   quality    the '+' line is skipped; q_take = min(length of the quality line with its newline, rlen), 0 when the line is absent
//   stops      no header line (END); no sequence line or rlen == 0 (EMPTY: what ends the reference's input, GetData.cpp:91); rlen > max_read_len
//   rows       A 0, C 1, G 2, T 3, sixteen bases to a word, the first in the top bits; any other byte has code 0 and is listed
// PLAIN RULE ONLY: the .gz readers' lines (gzgets with a 1024-byte buffer, strlen semantics, GetData.cpp:101-128) and FASTA are not covered.
#ifndef MCX_FASTQ_H
#define MCX_FASTQ_H
#include "mcx_types.h"
#include "../../include/mcx.h"

namespace mcx {
namespace fq {

// header_of (mcx_files.cpp): l[0 .. len) is the header line with its newline, len >= 1
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
