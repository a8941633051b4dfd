// tests/hostemu/markdup_check.cpp — -markdup's arithmetic (mapcaller_amd/csrc/mcx_markdup.h: a record's end, score and packed end) compiled for the host behind one C
// entry point: tests/test_markdup_host.py holds it against the rule written out in Python.  Built by the test with its own compiler command (g++ -shared), not
// by this directory's Makefile.  With -DMARKDUP_CHECK_MAIN it is a stand-alone program for a sanitizer build (see main below).
#include "../../mapcaller_amd/csrc/mcx_markdup.h"

// rec[0 .. len): one record from block_size on.  -1: len is not 4 + block_size, or the record is shorter than its name, CIGAR, SEQ and QUAL (nothing else is
// read then); else out = refID, u5, reverse, score, placed, packed end — and 1 when the end packs, 0 when it lies outside the packing's range (packed: all-ones)
extern "C" int markdup_check_record(const uint8_t *rec, uint64_t len, int64_t out[6])
{
    if (len < 36 || 4 + (uint64_t)mcx::bam_get32(rec) != len || !mcx::dup_record_fits(rec, len)) return -1;
    const mcx::DupEnd e = mcx::dup_end(rec);
    uint64_t packed = mcx::kDupNoEnd;
    const bool ok = mcx::bam_get32(rec + 20) < (uint32_t)mcx::kDupSeqLimit && mcx::dup_pack(e, &packed);
    if (!ok) packed = mcx::kDupNoEnd;
    out[0] = e.ref_id; out[1] = e.u5; out[2] = e.reverse; out[3] = (int64_t)mcx::dup_score(rec); out[4] = mcx::dup_placed(rec) ? 1 : 0; out[5] = (int64_t)packed;
    return ok ? 1 : 0;
}

#ifdef MARKDUP_CHECK_MAIN
// A sanitizer's view of the same: reads the records as tests/test_markdup_host.py dumps them (a count, then per record its length and bytes), every record in a
// heap block of exactly its size, and writes each record's result and six values to the second path, where the test compares them with the library form's.
// Built with -fsanitize=address,undefined and run by hand; the test builds it plainly.
#include <cstdio>
#include <cstdlib>
#include <vector>
int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s records.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint64_t n = 0;
    if (fread(&n, 8, 1, f) != 1) return 2;
    for (uint64_t k = 0; k < n; k++) {
        uint64_t len = 0;
        if (fread(&len, 8, 1, f) != 1) return 2;
        std::vector<uint8_t> rec((size_t)len);
        if (len && fread(rec.data(), 1, (size_t)len, f) != len) return 2;
        int64_t out[7] = {0, 0, 0, 0, 0, 0, 0};
        out[6] = markdup_check_record(rec.data(), len, out);
        fwrite(out, 8, 7, o);
    }
    fclose(f);
    if (fclose(o) != 0) return 2;
    printf("%llu records\n", (unsigned long long)n);
    return 0;
}
#endif
