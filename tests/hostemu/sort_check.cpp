// tests/hostemu/sort_check.cpp — -sort's order (mapcaller_amd/csrc/mcx_bam_sort.h) and the plan of its merge (mcx_sort_plan.h) compiled for the host:
// tests/test_bam_sort_host.py holds the key against the formula written out in Python and the plan against brute force.  Built by the test with its own
// compiler command (g++ -shared), not by this directory's Makefile.  With -DSORT_CHECK_MAIN it is a stand-alone program for a sanitizer build (see main below).
#include "../../mapcaller_amd/csrc/mcx_bam_sort.h"
#include "../../mapcaller_amd/csrc/mcx_sort_plan.h"

extern "C" uint64_t sort_check_key(const uint8_t *rec) { return mcx::bam_sort_key(rec); }

// The plan over n_runs runs given flat: run r has run_n[r] records (keys, lens: all runs' back to back) and run_nb[r] blocks, block_usize the bytes of the
// run's stream in each (all runs' back to back; a block's place in the file is made up here: the blocks of all runs one behind the other, each 26 bytes larger
// than its text).  out: 8 values a slice — chunk, run, r0, r1, b0, b1, k0, k1 — in chunk order; splitters: room for one less than the records.  Returns the
// number of slices, -1 when out is too small; *n_chunks the chunks.
extern "C" int64_t sort_check_plan(uint32_t n_runs, const uint64_t *run_n, const uint64_t *keys, const uint32_t *lens, const uint64_t *run_nb, const uint32_t *block_usize,
                                   uint64_t chunk_bytes, uint64_t *out, uint64_t cap_slices, uint64_t *n_chunks, uint64_t *splitters)
{
    using namespace mcx::sortplan;
    std::vector<Run> runs(n_runs);
    uint64_t at = 0, bat = 0, file_at = 0;
    for (uint32_t r = 0; r < n_runs; r++) {
        runs[r].keys.assign(keys + at, keys + at + run_n[r]);
        runs[r].lens.assign(lens + at, lens + at + run_n[r]);
        at += run_n[r];
        uint64_t u = 0;
        for (uint64_t k = 0; k < run_nb[r]; k++) {
            Block b; b.c_off = file_at; b.c_size = block_usize[bat + k] + 26; b.u_size = block_usize[bat + k]; b.u_off = u;
            runs[r].blocks.push_back(b);
            u += b.u_size; file_at += b.c_size;
        }
        bat += run_nb[r];
        runs[r].finish();
    }
    Plan plan;
    make_plan(runs, chunk_bytes, &plan);
    *n_chunks = plan.chunks.size();
    for (size_t k = 0; k < plan.splitters.size(); k++) splitters[k] = plan.splitters[k];
    uint64_t n = 0;
    for (size_t c = 0; c < plan.chunks.size(); c++)
        for (const Slice &s : plan.chunks[c].slices) {
            if (n >= cap_slices) return -1;
            uint64_t *o = out + 8 * n++;
            o[0] = c; o[1] = s.run; o[2] = s.r0; o[3] = s.r1; o[4] = s.b0; o[5] = s.b1; o[6] = s.k0; o[7] = s.k1;
        }
    return (int64_t)n;
}

#ifdef SORT_CHECK_MAIN
// A sanitizer's view of both: reads the cases as tests/test_bam_sort_host.py dumps them (dump_cases) — records for the key, then plan cases —, every array in a
// heap block of exactly its size, and writes the keys and the plans' slices to the second path, where the test compares them with the library form's.
// Built with -fsanitize=address,undefined and run by hand; the test builds it plainly.
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
    const uint64_t n_recs = take<uint64_t>(f, 1)[0];
    for (uint64_t i = 0; i < n_recs; i++) {
        const uint64_t len = take<uint64_t>(f, 1)[0];
        const std::vector<uint8_t> rec = take<uint8_t>(f, len); // (a record of exactly 20 bytes is enough for the key: a read past them is the sanitizer's to find)
        const uint64_t key = sort_check_key(rec.data());
        fwrite(&key, 8, 1, o);
    }
    const uint64_t n_cases = take<uint64_t>(f, 1)[0];
    uint64_t slices_total = 0;
    for (uint64_t c = 0; c < n_cases; c++) {
        const std::vector<uint64_t> h = take<uint64_t>(f, 4); // runs, chunk_bytes, records, blocks
        const std::vector<uint64_t> run_n = take<uint64_t>(f, h[0]), run_nb = take<uint64_t>(f, h[0]), keys = take<uint64_t>(f, h[2]);
        const std::vector<uint32_t> lens = take<uint32_t>(f, h[2]), usize = take<uint32_t>(f, h[3]);
        std::vector<uint64_t> out(8 * (h[2] + 1)), splitters(h[2] + 1);
        uint64_t n_chunks = 0;
        const int64_t n = sort_check_plan((uint32_t)h[0], run_n.data(), keys.data(), lens.data(), run_nb.data(), usize.data(), h[1], out.data(), h[2] + 1, &n_chunks, splitters.data());
        if (n < 0) { fprintf(stderr, "case %llu: more slices than records\n", (unsigned long long)c); return 1; }
        const uint64_t head[2] = {(uint64_t)n, n_chunks};
        fwrite(head, 8, 2, o);
        fwrite(out.data(), 8, 8 * (size_t)n, o);
        slices_total += (uint64_t)n;
    }
    fclose(f);
    if (fclose(o) != 0) return 2;
    printf("%llu keys, %llu plans, %llu slices\n", (unsigned long long)n_recs, (unsigned long long)n_cases, (unsigned long long)slices_total);
    return 0;
}
#endif
