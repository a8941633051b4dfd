// tests/hostemu/parser_check.cpp — TEST INFRASTRUCTURE: the product's two readers (mcx_reader.h) on the host, without a GPU: every record they hand out, as
// name <TAB> bases <TAB> qualities lines.  parser_dump: the sequential reader (Parser: .gz through the parallel inflater, BGZF, zlib's reader, FASTA with
// multi-line records).  mapped_dump: the mapped reader of plain FASTQ (MappedFastq: open, count, finish, parse) over a whole file.
// Linked against libmcx.so for the entry points the header refers to (the device inflater's); nothing of the mapping path runs.
#include "../../mapcaller_amd/csrc/mcx_reader.h"

using namespace mcx::files;

static void dump_rec(FILE *f, const char *base, const Rec &r, bool fastq)
{
    fwrite(base + r.name, 1, r.name_len, f); fputc('\t', f);
    fwrite(base + r.seq, 1, r.rlen, f); fputc('\t', f);
    if (fastq) fwrite(base + r.qual, 1, r.q_take, f);
    fputc('\n', f);
}

extern "C" long long parser_dump(const char *path, int max_len, int per_take, const char *out_path, char *err, int err_cap)
{
    Parser ps;
    std::string e;
    if (!ps.open(path, e)) { snprintf(err, (size_t)err_cap, "%s", e.c_str()); return -1; }
    FILE *f = fopen(out_path, "wb");
    if (!f) return -2;
    long long n = 0;
    for (bool more = true; more;) {
        View v;
        more = ps.take(v, (uint32_t)per_take, max_len);
        if (!v.error.empty()) { snprintf(err, (size_t)err_cap, "%s", v.error.c_str()); fclose(f); return -3; }
        for (const Rec &r : v.recs) { dump_rec(f, v.base, r, ps.fastq()); n++; }
    }
    fclose(f);
    return n;
}

// the whole file as the front end's mapped route sees it: a record needs its header and sequence lines, and the records end where parse() stops
extern "C" long long mapped_dump(const char *path, int max_len, int threads, const char *out_path, char *err, int err_cap)
{
    MappedFastq mf;
    std::string e;
    if (!mf.open(path, e)) { snprintf(err, (size_t)err_cap, "%s", e.c_str()); return -1; }
    Pool pool(threads);
    mf.count(0, mf.n_blocks(), pool);
    mf.finish();
    const uint64_t total = (mf.lines() + 2) / 4;
    std::vector<Rec> recs((size_t)total + 1);
    size_t n = 0;
    (void)mf.parse(0, total, max_len, recs.data(), n, e);
    if (!e.empty()) { snprintf(err, (size_t)err_cap, "%s", e.c_str()); return -3; }
    FILE *f = fopen(out_path, "wb");
    if (!f) return -2;
    for (size_t i = 0; i < n; i++) dump_rec(f, mf.data(), recs[i], true);
    fclose(f);
    return (long long)n;
}
