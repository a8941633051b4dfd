// tests/hostemu/tags_check.cpp — the formatters' read-group and mate tags (mapcaller_amd/csrc/mcx_sam.h, mcx_bam.h: SamTail) and the -rg argument's parser
// (mcx_tags.h) compiled for the host: tests/test_tags_host.py holds them against a plain restatement of the rule at mcx_sam_tags (include/mcx.h),
// tests/test_tags_device.py holds the kernels against them.  Built by the tests with their own compiler command (g++ -shared), not by this directory's Makefile.
#include <cstring>
#include "../../mapcaller_amd/csrc/mcx_bam.h"
#include "../../mapcaller_amd/csrc/mcx_tags.h"

// md_check.cpp's walks with a mcx_sam_tags beside `in` (null: both switches off).  Returns the total, -1 if it does not fit cap, -(r + 2) if read r's bytes are
// not as many as its length said.
extern "C" int64_t tags_check_sam(const mcx_sam_in *in, const mcx_sam_tags *tags, const char *contig_text, const uint32_t *contig_off, uint8_t *out, uint64_t cap, uint64_t *line_off)
{
    const mcx::SamContigs cn = {contig_text, contig_off};
    const mcx_sam_tags tg = tags ? *tags : mcx_sam_tags();
    uint64_t total = 0;
    for (uint32_t r = 0; r < in->n_reads; r++) { line_off[r] = total; total += mcx::sam_line_len(*in, cn, r, tg); }
    line_off[in->n_reads] = total;
    if (total > cap) return -1;
    for (uint32_t r = 0; r < in->n_reads; r++)
        if (mcx::sam_line_put(*in, cn, r, out + line_off[r], tg) != line_off[r + 1] - line_off[r]) return -(int64_t)r - 2;
    return (int64_t)total;
}
extern "C" int64_t tags_check_bam(const mcx_sam_in *in, const mcx_sam_tags *tags, uint8_t *out, uint64_t cap, uint64_t *rec_off)
{
    const mcx_sam_tags tg = tags ? *tags : mcx_sam_tags();
    uint64_t total = 0;
    for (uint32_t r = 0; r < in->n_reads; r++) { uint32_t dropped; rec_off[r] = total; total += mcx::bam_rec_len(*in, r, &dropped, tg); }
    rec_off[in->n_reads] = total;
    if (total > cap) return -1;
    for (uint32_t r = 0; r < in->n_reads; r++)
        if (mcx::bam_rec_put(*in, r, out + rec_off[r], tg) != rec_off[r + 1] - rec_off[r]) return -(int64_t)r - 2;
    return (int64_t)total;
}

// The -rg argument through the parser: the line (real TABs, no newline) into line[0 .. 4096], its ID into id[0 .. 255], both NUL-terminated; returns the line's
// length, or -1 with the reason in why[0 .. 255].
extern "C" int64_t tags_check_rg(const char *arg, char *line, char *id, char *why)
{
    std::string l, i, w;
    const bool ok = mcx::rg_parse(arg, l, i, w);
    line[0] = id[0] = why[0] = 0;
    if (!ok) { strncpy(why, w.c_str(), 255); why[255] = 0; return -1; }
    memcpy(line, l.c_str(), l.size() + 1);
    memcpy(id, i.c_str(), i.size() + 1);
    return (int64_t)l.size();
}
