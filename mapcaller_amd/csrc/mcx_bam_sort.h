// mapcaller_amd/csrc/mcx_bam_sort.h — the order of a coordinate-sorted BAM file (-sort), for the device and (tests/hostemu/sort_check.cpp) for the host.
//
// A record's key is read from the record's own bytes (mcx_bam.h's layout, all little-endian, never aligned), counted from block_size:
//   refID at byte 4, pos at byte 8, the flag at bytes 18-19 (bit 0x10: the reverse strand)
//   key = (uint32_t)refID << 32 | (uint32_t)(pos + 1) << 1 | reverse
// which is the comparison of samtools sort without -n: refID -1 is the largest (unmapped records last), and on one position forward comes before
// reverse.  Ties keep input order: the order of the reads in the file, and among one read's records under -m the order k_bam_write wrote them in.
#ifndef MCX_BAM_SORT_H
#define MCX_BAM_SORT_H
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MCX_SORT_HD __host__ __device__
#else
#define MCX_SORT_HD
#endif

namespace mcx {

enum { kBamMinBlock = 32 }; // the smallest block_size: the 32 bytes of the core behind it (a record of our own is never below 38 bytes)

static inline MCX_SORT_HD uint32_t bam_get32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

static inline MCX_SORT_HD uint64_t bam_sort_key_of(uint32_t ref_id, uint32_t pos, uint32_t flag)
{
    return (uint64_t)ref_id << 32 | (uint64_t)(uint32_t)((pos + 1u) << 1) | (uint64_t)((flag >> 4) & 1u);
}
// rec: the record's first byte (block_size); 20 bytes of it are read
static inline MCX_SORT_HD uint64_t bam_sort_key(const uint8_t *rec)
{
    return bam_sort_key_of(bam_get32(rec + 4), bam_get32(rec + 8), (uint32_t)rec[18] | (uint32_t)rec[19] << 8);
}

} // namespace mcx
#endif
