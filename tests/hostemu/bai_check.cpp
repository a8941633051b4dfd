// tests/hostemu/bai_check.cpp — -index's host half (mapcaller_amd/csrc/mcx_bai.h: the accumulator of the stretches, the finish, the writer) behind a few C entry
// points: tests/test_bai_host.py holds it against a restatement of htslib's rules written out in Python.  Built by the test with its own compiler command
// (g++ -shared), not by this directory's Makefile.  With -DBAI_CHECK_MAIN it is a stand-alone program for a sanitizer build (see main below).
#include "../../mapcaller_amd/csrc/mcx_bai.h"

static_assert(sizeof(mcx::bai::Run) == 24, "a stretch is 24 bytes: int32 ref_id, uint32 bin, uint64 u, uint32 n_mapped, uint32 n_unmapped");

extern "C" uint32_t bai_check_reg2bin(int64_t beg, int64_t end) { return mcx::bai::reg2bin(beg, end); }
extern "C" uint64_t bai_check_windows_of(int64_t contig_len) { return mcx::bai::windows_of(contig_len); }

// The index of n_calls run lists (call k has call_n[k] stretches; all calls' back to back in runs) pushed one after the other, finished with final_offset and
// the windows' table (lin_base: n_ref + 1 entries).  Returns the file's size and writes it to out when cap holds it; -1: a run list did not continue the
// order, -2: a stretch names a contig or a bin that does not exist.  stats: stretches (after joining), bins, linear entries, bytes.
extern "C" int64_t bai_check_build(uint32_t n_ref, uint32_t n_calls, const uint64_t *call_n, const mcx::bai::Run *runs, uint64_t final_offset, const uint64_t *lin, const uint64_t *lin_base,
                                   uint8_t *out, uint64_t cap, uint64_t stats[4])
{
    mcx::bai::Index ix;
    uint64_t at = 0;
    for (uint32_t k = 0; k < n_calls; k++) {
        if (!ix.push(runs + at, call_n[k])) return -1;
        at += call_n[k];
    }
    std::vector<uint8_t> bytes;
    mcx::bai::Stats st;
    if (!ix.finish(n_ref, final_offset, lin, lin_base, &bytes, &st)) return -2;
    if (stats) { stats[0] = st.stretches; stats[1] = st.bins; stats[2] = st.intervals; stats[3] = st.bytes; }
    if (bytes.size() <= cap && !bytes.empty()) memcpy(out, bytes.data(), bytes.size());
    return (int64_t)bytes.size();
}

#ifdef BAI_CHECK_MAIN
// A sanitizer's view of the same: reads the cases as tests/test_bai_host.py dumps them (dump_cases), every array in a heap block of exactly its size, and
// writes each case's result and bytes to the second path, where the test compares them with the library form's.  Built with -fsanitize=address,undefined and
// run by hand; the test builds it plainly.
#include <cstdio>
#include <cstdlib>
template <class T> static std::vector<T> take(FILE *f, uint64_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short file\n"); exit(2); }
    return v;
}
int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    const uint64_t n_cases = take<uint64_t>(f, 1)[0];
    uint64_t total = 0;
    for (uint64_t c = 0; c < n_cases; c++) {
        const std::vector<uint64_t> h = take<uint64_t>(f, 5); // contigs, calls, final_offset, stretches, windows
        const std::vector<uint64_t> call_n = take<uint64_t>(f, h[1]);
        const std::vector<mcx::bai::Run> runs = take<mcx::bai::Run>(f, h[3]);
        const std::vector<uint64_t> lin_base = take<uint64_t>(f, h[0] + 1), lin = take<uint64_t>(f, h[4]);
        uint64_t stats[4] = {0, 0, 0, 0};
        const int64_t need = bai_check_build((uint32_t)h[0], (uint32_t)h[1], call_n.data(), runs.data(), h[2], lin.data(), lin_base.data(), nullptr, 0, stats);
        std::vector<uint8_t> out(need > 0 ? (size_t)need : 0);
        const int64_t n = bai_check_build((uint32_t)h[0], (uint32_t)h[1], call_n.data(), runs.data(), h[2], lin.data(), lin_base.data(), out.data(), out.size(), stats);
        if (n != need) { fprintf(stderr, "case %llu: two calls, two sizes\n", (unsigned long long)c); return 1; }
        fwrite(&n, 8, 1, o);
        if (n > 0) fwrite(out.data(), 1, (size_t)n, o);
        total += n > 0 ? (uint64_t)n : 0;
    }
    fclose(f);
    if (fclose(o) != 0) return 2;
    printf("%llu cases, %llu bytes\n", (unsigned long long)n_cases, (unsigned long long)total);
    return 0;
}
#endif
