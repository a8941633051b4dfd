// tests/hostemu/sam_check.cpp — the device's SAM formatter (mapcaller_amd/csrc/mcx_sam.h) compiled for the host: tests/test_sam_device.py
// holds it against the golden SAM files.  Built by the test with its own compiler command (g++ -shared), not by this directory's Makefile.
#include "../../mapcaller_amd/csrc/mcx_sam.h"

// The lines of every read of `in` (host pointers), as the kernels make them: lengths first (line_off[n_reads + 1], the last one the total), then the
// text at out[line_off[r] ..].  Returns the total, -1 if it does not fit cap, -(r + 2) if read r's text is not as long as its length said.
extern "C" int64_t sam_check_format(const mcx_sam_in *in, const char *contig_text, const uint32_t *contig_off, uint8_t *out, uint64_t cap, uint64_t *line_off)
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
