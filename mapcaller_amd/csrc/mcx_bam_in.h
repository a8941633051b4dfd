// mapcaller_amd/csrc/mcx_bam_in.h — the rules for BAM records as read input (MCX_READS_BAM), once, for the device (mcx_bam_in.hip) and for the host
// (tests/hostemu/bam_in_check.cpp).  The text is what follows a BAM file's header: records back to back, each `block_size` (4 bytes) and that many bytes —
//   refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen (32 bytes), read_name (NUL-terminated), cigar, seq (4-bit), qual, tags.
// The yardstick is the FASTQ twin, the text `samtools fastq` would make of the file: every taken record gives the name, bases, qualities, row and odd bytes
// that mcx_fastq.h's plain rule gives of `@read_name\nSEQ\n+\nQUAL\n`.
//   rule P      a record at o is plausible when 32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size <= 2^28, l_read_name >= 1 with a NUL
//               as the name's last byte, l_seq >= 0, and -1 <= refID, next_refID < n_ref.  Every field is read only once its offset is known to lie in the text
//   the chain   from offset 0, o -> o + 4 + block_size.  At o == bytes the text ends on a boundary (kEnd); a record whose fixed part, name or end lies behind
//               the text's end runs past it (kPast) unless what can be read of it already fails P (kBad)
//   taken       flag & 0x900 == 0 (secondary and supplementary lines are skipped, as samtools fastq skips them)
//   of a taken record   name: header_of over '@' + read_name + '\n'; rlen = l_seq (0: EMPTY, > max_read_len: TOO_LONG); base i "=ACMGRSVTWYHKDBN"[nibble i], high
//               nibble first; quality min(q, 93) + 33, q_take = rlen, 0 when the first quality byte is 0xFF.  Flag 0x10: the read is given back as sequenced —
//               base i is the bit reversal (the complement, IUPAC codes included) of nibble rlen - 1 - i, quality i is byte rlen - 1 - i
//   mates       (mcx_fastq_parser_set_mates) taken records count in twos: the first with 0x1 and 0x40, the second with 0x1 and 0x80, their names equal (UNPAIRED)
#ifndef MCX_BAM_IN_H
#define MCX_BAM_IN_H
#include "mcx_types.h"
#include "../../include/mcx.h"

namespace mcx {
namespace bamin {

enum : uint32_t { kFixed = 36, kMaxBlock = 1u << 28, kSkipFlags = 0x900u };
enum : uint32_t { kOk = 0, kEnd = 1, kPast = 2, kBad = 3 }; // what lies at an offset of the chain

static inline MCX_HD uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline MCX_HD uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

struct Fixed { uint32_t block_size, l_read_name, n_cigar, flag, l_seq; };

// the record at o: kOk — P holds and the whole record lies inside text[0 .. bytes); r is filled whenever the fixed part could be read (kOk, and kPast / kBad behind it)
static inline MCX_HD uint32_t record_at(const uint8_t *text, uint64_t bytes, uint64_t o, int32_t n_ref, Fixed &r)
{
    r.block_size = r.l_read_name = r.n_cigar = r.flag = r.l_seq = 0;
    if (o >= bytes) return kEnd;
    if (o + kFixed > bytes) return kPast;
    const uint8_t *p = text + o;
    r.block_size = rd32(p); r.l_read_name = p[12]; r.n_cigar = rd16(p + 16); r.flag = rd16(p + 18); r.l_seq = rd32(p + 20);
    const int32_t ref = (int32_t)rd32(p + 4), next_ref = (int32_t)rd32(p + 24);
    if ((int32_t)r.l_seq < 0 || r.l_read_name < 1 || r.block_size > kMaxBlock) return kBad;
    const uint64_t least = 32ull + r.l_read_name + 4ull * r.n_cigar + ((uint64_t)r.l_seq + 1) / 2 + r.l_seq;
    if (least > r.block_size) return kBad;
    if (ref < -1 || ref >= n_ref || next_ref < -1 || next_ref >= n_ref) return kBad;
    const uint64_t nul = o + kFixed + r.l_read_name - 1; // (inside the record: least <= block_size)
    if (nul >= bytes) return kPast;
    if (text[nul] != 0) return kBad;
    if (o + 4 + r.block_size > bytes) return kPast;
    return kOk;
}
static inline MCX_HD uint64_t next_of(uint64_t o, const Fixed &r) { return o + 4 + r.block_size; }
static inline MCX_HD bool taken(const Fixed &r) { return (r.flag & kSkipFlags) == 0; }

// header_of (mcx_fastq.h) over the line '@' + name[0 .. l_read_name - 1) + '\n' without building it: [p1, p2) in that line, whose byte i >= 1 is name[i - 1]
static inline MCX_HD void name_span(const uint8_t *name, uint32_t l_read_name, uint32_t &p1, uint32_t &p2)
{
    const uint32_t len = l_read_name + 1, lim = len > 100u ? 100u : len;
    p1 = len - 1; p2 = lim - 1;
    for (uint32_t i = 1; i < len; i++) { const uint8_t c = i < l_read_name ? name[i - 1] : (uint8_t)'\n'; if (c != '>' && c != '@') { p1 = i; break; } }
    for (uint32_t i = 1; i < lim; i++) { const uint8_t c = i < l_read_name ? name[i - 1] : (uint8_t)'\n'; if (c <= ' ' || c == '/' || c >= 0x7f) { p2 = i; break; } }
}

// the taken record at o (record_at said kOk) as offsets into the text; MCX_FASTQ_MORE, or why the text's records end at it
static inline MCX_HD uint32_t rec_of(const uint8_t *text, uint64_t o, const Fixed &r, int32_t max_read_len, mcx_fastq_rec &rec)
{
    uint32_t p1, p2;
    name_span(text + o + kFixed, r.l_read_name, p1, p2);
    rec.name = (uint32_t)(o + kFixed + p1 - 1); rec.name_len = p2 > p1 ? p2 - p1 : 0;
    rec.seq = (uint32_t)(o + kFixed + r.l_read_name + 4u * r.n_cigar);
    rec.rlen = r.l_seq;
    rec.qual = rec.seq + (r.l_seq + 1) / 2;
    rec.q_take = 0;
    if (r.l_seq == 0) return MCX_FASTQ_EMPTY;
    if ((int64_t)r.l_seq > (int64_t)max_read_len) return MCX_FASTQ_TOO_LONG;
    rec.q_take = text[rec.qual] == 0xFF ? 0 : r.l_seq;
    return MCX_FASTQ_MORE;
}

// two taken records as mates: their flags, and their names after the name rule
static inline MCX_HD bool mates_ok(const uint8_t *text, const mcx_fastq_rec &a, uint32_t flag_a, const mcx_fastq_rec &b, uint32_t flag_b)
{
    if ((flag_a & 0x41u) != 0x41u || (flag_b & 0x81u) != 0x81u || a.name_len != b.name_len) return false;
    for (uint32_t i = 0; i < a.name_len; i++) if (text[a.name + i] != text[b.name + i]) return false;
    return true;
}

static inline MCX_HD uint32_t bitrev4(uint32_t n) { return ((n & 1u) << 3) | ((n & 2u) << 1) | ((n & 4u) >> 1) | ((n & 8u) >> 3); }
// the 4-bit code of base i of the read as sequenced
static inline MCX_HD uint32_t nibble_of(const uint8_t *seq, uint32_t rlen, bool reversed, uint32_t i)
{
    const uint32_t j = reversed ? rlen - 1 - i : i;
    const uint32_t n = (seq[j >> 1] >> ((~j & 1u) * 4u)) & 15u;
    return reversed ? bitrev4(n) : n;
}
static inline MCX_HD uint8_t letter_of(uint32_t nibble) { return (uint8_t)"=ACMGRSVTWYHKDBN"[nibble]; }
static inline MCX_HD bool odd_nibble(uint32_t n) { return n != 1u && n != 2u && n != 4u && n != 8u; }       // not A, C, G, T
static inline MCX_HD uint32_t code2_of(uint32_t n) { return n == 2u ? 1u : n == 4u ? 2u : n == 8u ? 3u : 0u; } // the row's 2-bit code; 0 for every other letter
static inline MCX_HD uint8_t qual_of(const uint8_t *qual, uint32_t rlen, bool reversed, uint32_t i)
{
    const uint8_t q = qual[reversed ? rlen - 1 - i : i];
    return (uint8_t)((q > 93 ? 93 : q) + 33);
}
// bases [i, i + n) of the read, n <= 16, as one word of the row: the first base in the top bits
static inline MCX_HD uint32_t row_word(const uint8_t *seq, uint32_t rlen, bool reversed, uint32_t i, uint32_t n)
{
    uint32_t w = 0;
    for (uint32_t j = 0; j < n; j++) w |= code2_of(nibble_of(seq, rlen, reversed, i + j)) << (30 - 2 * j);
    return w;
}

// The BAM file's header: magic, l_text, text, n_ref, and per reference l_name, name, l_ref.  0 and *records_at / *n_ref; 1: `bytes` holds too little; -1: no BAM
static inline int reads_header(const uint8_t *text, uint64_t bytes, uint64_t *records_at, int32_t *n_ref)
{
    const uint8_t magic[4] = {'B', 'A', 'M', 1};
    for (uint64_t i = 0; i < 4 && i < bytes; i++) if (text[i] != magic[i]) return -1;
    if (bytes < 8) return 1;
    const int32_t l_text = (int32_t)rd32(text + 4);
    if (l_text < 0) return -1;
    uint64_t o = 8ull + (uint32_t)l_text;
    if (o + 4 > bytes) return 1;
    const int32_t n = (int32_t)rd32(text + o);
    if (n < 0) return -1;
    o += 4;
    for (int32_t i = 0; i < n; i++) {
        if (o + 4 > bytes) return 1;
        const int32_t l_name = (int32_t)rd32(text + o);
        if (l_name < 1) return -1;
        o += 4ull + (uint32_t)l_name + 4; // the name and l_ref
        if (o > bytes) return 1;
    }
    *records_at = o; *n_ref = n;
    return 0;
}

} // namespace bamin
} // namespace mcx
#endif
