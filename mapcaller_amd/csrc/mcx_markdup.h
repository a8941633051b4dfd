// mapcaller_amd/csrc/mcx_markdup.h — what makes two reads duplicates of each other (-markdup), for the device (mcx_markdup.hip) and
// (tests/hostemu/markdup_check.cpp) for the host.
//
// Everything is read from a record's own bytes (mcx_bam.h's layout, little-endian, never aligned), counted from block_size:
//   refID at byte 4, pos at 8, l_read_name at 12, n_cigar_op at 16, the flag at 18-19, l_seq at 20; the name at 36, behind it the CIGAR words, SEQ
//   ((l_seq + 1) / 2 bytes) and QUAL (l_seq bytes).
//   end(record)   = (refID, u5, reverse): the unclipped 5' end.  Forward: u5 = pos - the lengths of the leading S and H operations.  Reverse: u5 = pos + reflen - 1
//                   + the lengths of the trailing S and H operations, reflen the sum over M, D, N, = and X.  u5 may be negative.
//   score(record) = the sum of the QUAL bytes that are 15 or more; 0xff (no quality) counts as 0.
//   packed end    = refID << 40 | (u5 + 2^38) << 1 | reverse: 24 | 39 | 1 bits, injective — and ordered like (refID, u5, reverse) — for 0 <= refID < 2^24 - 1 and
//                   |u5| < 2^38.  All-ones is no end (refID 2^24 - 1 is refused): it stands for "none".  Outside that range dup_pack says so; nothing is folded.
// A record of 2^23 bases or more is outside the range as well: two mates' scores are summed in 32 bits.
// The units, and which of them are duplicates, are mcx_markdup.hip's (the rule in words: include/mcx.h).
#ifndef MCX_MARKDUP_H
#define MCX_MARKDUP_H
#include <cstdint>
#include "mcx_bam_sort.h"

namespace mcx {

enum { kDupNone = 0, kDupFragment = 1, kDupPair = 2, kDupSecondMate = 4 }; // mcx_dup_unit.kind: bits 0-1 the kind; bit 2: the fragment is the pair's second read
enum { kDupRefLimit = (1 << 24) - 1, kDupSeqLimit = 1 << 23 };
const int64_t kDupU5Limit = 1ll << 38;
const uint64_t kDupNoEnd = ~0ull;

struct DupEnd { int32_t ref_id; int64_t u5; uint32_t reverse; };

// the bytes a record's fields take, from block_size on: false when len (4 + block_size) is shorter than its name, CIGAR, SEQ and QUAL
static inline MCX_SORT_HD bool dup_record_fits(const uint8_t *rec, uint64_t len)
{
    if (len < 36) return false;
    const uint64_t l_name = rec[12], n_cigar = (uint32_t)rec[16] | (uint32_t)rec[17] << 8, l_seq = bam_get32(rec + 20);
    return 36 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq <= len;
}
static inline MCX_SORT_HD uint32_t dup_flag(const uint8_t *rec) { return (uint32_t)rec[18] | (uint32_t)rec[19] << 8; }
static inline MCX_SORT_HD bool dup_placed(const uint8_t *rec) { return !(dup_flag(rec) & 4u); }
// where QUAL begins, counted from the record's first byte
static inline MCX_SORT_HD uint64_t dup_qual_at(const uint8_t *rec)
{
    const uint64_t l_name = rec[12], n_cigar = (uint32_t)rec[16] | (uint32_t)rec[17] << 8, l_seq = bam_get32(rec + 20);
    return 36 + l_name + 4 * n_cigar + (l_seq + 1) / 2;
}

// rec: a record that fits (dup_record_fits)
static inline MCX_SORT_HD DupEnd dup_end(const uint8_t *rec)
{
    const uint32_t l_name = rec[12], n_cigar = (uint32_t)rec[16] | (uint32_t)rec[17] << 8;
    const uint8_t *cg = rec + 36 + l_name;
    DupEnd e;
    e.ref_id = (int32_t)bam_get32(rec + 4);
    e.reverse = (dup_flag(rec) >> 4) & 1u;
    const int64_t pos = (int32_t)bam_get32(rec + 8);
    if (!e.reverse) {
        int64_t clip = 0;
        for (uint32_t k = 0; k < n_cigar; k++) {
            const uint32_t w = bam_get32(cg + 4 * k), op = w & 15u;
            if (op != 4 && op != 5) break; // S and H at the start
            clip += w >> 4;
        }
        e.u5 = pos - clip;
    } else {
        int64_t ref_len = 0, clip = 0; // clip: the S and H operations since the last operation of another kind
        for (uint32_t k = 0; k < n_cigar; k++) {
            const uint32_t w = bam_get32(cg + 4 * k), op = w & 15u;
            if (op == 4 || op == 5) { clip += w >> 4; continue; }
            clip = 0;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += w >> 4;
        }
        e.u5 = pos + ref_len - 1 + clip;
    }
    return e;
}

static inline MCX_SORT_HD uint32_t dup_score_byte(uint32_t q) { return q >= 15u && q != 0xffu ? q : 0u; }
// (the device sums the same bytes many lanes a record: mcx_markdup.hip)
static inline MCX_SORT_HD uint64_t dup_score(const uint8_t *rec)
{
    const uint8_t *q = rec + dup_qual_at(rec);
    const uint64_t l_seq = bam_get32(rec + 20);
    uint64_t s = 0;
    for (uint64_t k = 0; k < l_seq; k++) s += dup_score_byte(q[k]);
    return s;
}

// false: outside the range the packing holds apart
static inline MCX_SORT_HD bool dup_pack(const DupEnd &e, uint64_t *out)
{
    if (e.ref_id < 0 || e.ref_id >= (int32_t)kDupRefLimit || e.u5 <= -kDupU5Limit || e.u5 >= kDupU5Limit) return false;
    *out = (uint64_t)(uint32_t)e.ref_id << 40 | (uint64_t)(e.u5 + kDupU5Limit) << 1 | (uint64_t)e.reverse;
    return true;
}

} // namespace mcx
#endif
