// tests/hostemu/bam_check.cpp — the device's BAM encoder (mapcaller_amd/csrc/mcx_bam.h) compiled for the host: tests/test_bam_host.py holds it against the
// golden SAM files and hand-assembled records, tests/test_bam_device.py holds the kernels against it.  Built by the test with its own compiler command
// (g++ -shared), not by this directory's Makefile.  With -DBAM_CHECK_MAIN it is a stand-alone program for a sanitizer build (see main below).
#include "../../mapcaller_amd/csrc/mcx_bam.h"

// The records of every read of `in` (host pointers), as the kernels make them: lengths first (rec_off[n_reads + 1], the last one the total; *n_dropped the
// lines that make no record), then the bytes at out[rec_off[r] ..].  Returns the total, -1 if it does not fit cap, -(r + 2) if read r's bytes are not as
// many as its length said.
extern "C" int64_t bam_check_format(const mcx_sam_in *in, uint8_t *out, uint64_t cap, uint64_t *rec_off, uint64_t *n_dropped)
{
    uint64_t total = 0, dropped = 0;
    for (uint32_t r = 0; r < in->n_reads; r++) {
        uint32_t none = 0;
        rec_off[r] = total;
        total += mcx::bam_rec_len(*in, r, &none);
        dropped += none;
    }
    rec_off[in->n_reads] = total;
    if (n_dropped) *n_dropped = dropped;
    if (total > cap) return -1;
    for (uint32_t r = 0; r < in->n_reads; r++)
        if (mcx::bam_rec_put(*in, r, out + rec_off[r]) != rec_off[r + 1] - rec_off[r]) return -(int64_t)r - 2;
    return (int64_t)total;
}
extern "C" uint32_t bam_check_bin(int64_t beg, int64_t end) { return mcx::bam_bin(beg, end); }
extern "C" uint32_t bam_check_nibble(uint32_t c) { return mcx::bam_nibble((uint8_t)c); }

#ifdef BAM_CHECK_MAIN
// A sanitizer's view of the encoder: reads one batch as tests/test_bam_host.py dumps it (dump_batch: a header of counts, then the arrays), sizes it, encodes it
// into a heap buffer of exactly the size, and writes the bytes to the second path.  Built with -fsanitize=address,undefined and run by hand; not a test.
#include <cstdio>
#include <cstdlib>
#include <vector>
static std::vector<uint8_t> take(FILE *f, uint64_t bytes)
{
    std::vector<uint8_t> v(bytes);
    if (bytes && fread(v.data(), 1, bytes, f) != bytes) { fprintf(stderr, "short file\n"); exit(2); }
    return v;
}
int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s batch.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[8]; // n_reads, paired, has_qual, bases bytes, name bytes, cigar words, extras, extra cigar words (extras == UINT64_MAX: no x_index)
    if (fread(h, 8, 8, f) != 8) return 2;
    const uint64_t n = h[0];
    const bool multi = h[6] != ~0ull;
    // (every array in a heap block of exactly its size: a read past an end is the sanitizer's to find)
    std::vector<uint8_t> off = take(f, (n + 1) * 4), name_off = take(f, (n + 1) * 4), bases = take(f, h[3]), qual = take(f, h[2] ? h[3] : 0), names = take(f, h[4]);
    std::vector<uint8_t> aln = take(f, n * sizeof(mcx_aln)), cigar = take(f, h[5] * 4);
    std::vector<uint8_t> x_index = take(f, multi ? (n + 1) * 4 : 0), x_recs = take(f, multi ? h[6] * sizeof(mcx_aln) : 0), x_cigar = take(f, multi ? h[7] * 4 : 0);
    fclose(f);
    mcx_sam_in in = {};
    in.bases = bases.data(); in.off = (const uint32_t *)off.data(); in.qual = h[2] ? qual.data() : nullptr;
    in.names = names.data(); in.name_off = (const uint32_t *)name_off.data();
    in.aln = (const mcx_aln *)aln.data(); in.cigar = (const uint32_t *)cigar.data();
    if (multi) { in.x_index = (const uint32_t *)x_index.data(); in.x_recs = (const mcx_aln *)x_recs.data(); in.x_cigar = (const uint32_t *)x_cigar.data(); }
    in.n_reads = (uint32_t)n; in.paired = (int32_t)h[1];
    std::vector<uint64_t> rec_off(n + 1);
    uint64_t dropped = 0;
    bam_check_format(&in, nullptr, 0, rec_off.data(), &dropped);
    std::vector<uint8_t> out(rec_off[n]);
    const int64_t got = bam_check_format(&in, out.data(), out.size(), rec_off.data(), &dropped);
    if (got != (int64_t)out.size()) { fprintf(stderr, "bam_check_format: %lld\n", (long long)got); return 1; }
    FILE *o = fopen(argv[2], "wb");
    if (!o || (out.size() && fwrite(out.data(), 1, out.size(), o) != out.size())) return 2;
    fclose(o);
    printf("%llu reads, %llu bytes, %llu lines dropped\n", (unsigned long long)n, (unsigned long long)out.size(), (unsigned long long)dropped);
    return 0;
}
#endif
