// tests/hostemu/md_check.cpp — the device's MD:Z strings (mapcaller_amd/csrc/mcx_md.h) and the formatters that append them (mcx_sam.h, mcx_bam.h) compiled for the
// host: tests/test_md_host.py holds them against a plain restatement of the definition, tests/test_md_device.py holds the kernels against them.  Built by the tests
// with their own compiler command (g++ -shared), not by this directory's Makefile.
#include "../../mapcaller_amd/csrc/mcx_md.h"

// The strings of every line of `in` (host pointers; n_extras = x_index[n_reads], 0 without extras) as the kernels make them: lengths first (md_off[n_reads + n_extras + 1],
// the last one the total), then the bytes at out[md_off[e] ..].  Returns the total, -1 if it does not fit cap, -(e + 2) if line e's string is not as long as its length said.
extern "C" int64_t md_check_strings(const mcx_sam_in *in, const uint8_t *pac, int64_t G, const int64_t *chr_fwd, const int64_t *hole_off, const int32_t *hole_len,
                                    const uint8_t *hole_letter, uint32_t n_holes, uint8_t *out, uint64_t cap, uint32_t *md_off)
{
    const mcx::MdRef ref = {pac, G, chr_fwd, hole_off, hole_len, hole_letter, n_holes};
    const uint32_t n_extras = in->x_index && in->n_reads ? in->x_index[in->n_reads] : 0;
    const uint32_t n = mcx::md_n_lines(*in, n_extras);
    uint64_t total = 0;
    for (uint32_t e = 0; e < n; e++) {
        uint32_t r; mcx_aln rec; const uint32_t *cigar;
        mcx::md_line_of(*in, e, r, rec, cigar);
        md_off[e] = (uint32_t)total;
        total += mcx::md_one_len(ref, mcx::sam_read_of(*in, r), rec, cigar);
    }
    md_off[n] = (uint32_t)total;
    if (total > cap) return -1;
    for (uint32_t e = 0; e < n; e++) {
        uint32_t r; mcx_aln rec; const uint32_t *cigar;
        mcx::md_line_of(*in, e, r, rec, cigar);
        if (mcx::md_one_put(ref, mcx::sam_read_of(*in, r), rec, cigar, out + md_off[e]) != out + md_off[e + 1]) return -(int64_t)e - 2;
    }
    return (int64_t)total;
}

// sam_check.cpp's sam_check_format and bam_check.cpp's record walk for an `in` that carries md / md_off: the text (the records) with the MD tags appended
extern "C" int64_t md_check_sam(const mcx_sam_in *in, const char *contig_text, const uint32_t *contig_off, uint8_t *out, uint64_t cap, uint64_t *line_off)
{
    const mcx::SamContigs cn = {contig_text, contig_off};
    uint64_t total = 0;
    for (uint32_t r = 0; r < in->n_reads; r++) { line_off[r] = total; total += mcx::sam_line_len(*in, cn, r); }
    line_off[in->n_reads] = total;
    if (total > cap) return -1;
    for (uint32_t r = 0; r < in->n_reads; r++)
        if (mcx::sam_line_put(*in, cn, r, out + line_off[r]) != line_off[r + 1] - line_off[r]) return -(int64_t)r - 2;
    return (int64_t)total;
}
extern "C" int64_t md_check_bam(const mcx_sam_in *in, uint8_t *out, uint64_t cap, uint64_t *rec_off)
{
    uint64_t total = 0;
    for (uint32_t r = 0; r < in->n_reads; r++) { uint32_t dropped; rec_off[r] = total; total += mcx::bam_rec_len(*in, r, &dropped); }
    rec_off[in->n_reads] = total;
    if (total > cap) return -1;
    for (uint32_t r = 0; r < in->n_reads; r++)
        if (mcx::bam_rec_put(*in, r, out + rec_off[r]) != rec_off[r + 1] - rec_off[r]) return -(int64_t)r - 2;
    return (int64_t)total;
}
