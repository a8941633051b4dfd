// tests/hostemu/bam_in_check.cpp — the parser's contract under MCX_READS_BAM on the host, one thread, built only from mapcaller_amd/csrc/mcx_bam_in.h: the rules
// the kernels of mcx_bam_in.hip compile, run as the sequential walk.  tests/test_bam_in_host.py builds it as a shared object (bam_in_check_parse: the call's
// arguments, host pointers; bam_in_check_header: mcx_bam_reads_header's) and, with -DBAM_IN_CHECK_MAIN, as a stand-alone program for
// -fsanitize=address,undefined: it reads a file of texts and parses each with final 0 and 1, with and without mates, and max_records 0 .. 3 and unbounded, from a
// heap copy of exactly the text's size into heap buffers of exactly the contract's sizes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mapcaller_amd/csrc/mcx_bam_in.h"
#include "../../mapcaller_amd/csrc/mcx_fastq.h"

using namespace mcx::bamin;

extern "C" int bam_in_check_header(const uint8_t *text, uint64_t bytes, uint64_t *records_at, int32_t *n_ref) { return reads_header(text, bytes, records_at, n_ref); }

extern "C" int bam_in_check_parse(const mcx_fastq_in *in, const mcx_fastq_out *out, int mates, mcx_fastq_info *info)
{
    memset(info, 0, sizeof *info);
    if (in->text[1] || in->bytes[0] >= (1ull << 32)) return MCX_ERR_ARG;
    if (out->rows && (int64_t)out->row_words * 16 < (int64_t)in->max_read_len) return MCX_ERR_ARG;
    const uint8_t *text = in->text[0];
    const uint64_t bytes = in->bytes[0];
    const uint32_t cap = mates ? in->max_records & ~1u : in->max_records;
    std::vector<mcx_fastq_rec> recs;
    std::vector<uint32_t> flags;
    uint64_t o = 0, consumed = 0;
    uint32_t stop = MCX_FASTQ_MORE;
    bool pending = false;
    mcx_fastq_rec first; uint32_t first_f = 0;
    memset(&first, 0, sizeof first);
    for (;;) {
        if (!pending && recs.size() >= cap) { stop = MCX_FASTQ_MORE; break; }
        Fixed r;
        const uint32_t st = record_at(text, bytes, o, in->n_ref, r);
        if (st == kEnd) { stop = pending ? (in->final ? MCX_FASTQ_UNPAIRED : MCX_FASTQ_MORE) : MCX_FASTQ_END; break; }
        if (st == kPast) { stop = in->final ? MCX_FASTQ_DAMAGED : MCX_FASTQ_MORE; break; }
        if (st == kBad) { stop = MCX_FASTQ_DAMAGED; break; }
        if (!taken(r)) { o = next_of(o, r); if (!pending) consumed = o; continue; }
        mcx_fastq_rec rec;
        const uint32_t why = rec_of(text, o, r, in->max_read_len, rec);
        if (why != MCX_FASTQ_MORE) { stop = why; break; }
        if (!mates) { recs.push_back(rec); flags.push_back(r.flag); o = next_of(o, r); consumed = o; continue; }
        if (!pending) { first = rec; first_f = r.flag; pending = true; o = next_of(o, r); continue; }
        if (!mates_ok(text, first, first_f, rec, r.flag)) { stop = MCX_FASTQ_UNPAIRED; break; }
        recs.push_back(first); flags.push_back(first_f); recs.push_back(rec); flags.push_back(r.flag);
        pending = false; o = next_of(o, r); consumed = o;
    }
    const uint32_t n = (uint32_t)recs.size();
    info->n_records[0] = n; info->stop[0] = stop; info->consumed[0] = consumed; info->n_reads = n;
    if (out->recs[0]) for (uint32_t i = 0; i < n; i++) out->recs[0][i] = recs[i];
    for (uint32_t r = 0; r < n; r++) {
        const mcx_fastq_rec &c = recs[r];
        const bool rev = (flags[r] & 0x10u) != 0;
        info->n_bases += c.rlen; info->n_name_bytes += c.name_len;
        if (c.rlen > info->longest) info->longest = c.rlen;
        for (uint32_t i = 0; i < c.rlen; i++) info->n_odd += odd_nibble(nibble_of(text + c.seq, c.rlen, rev, i));
    }
    int rc = 0;
    if (out->bases) {
        if (out->bases_cap < info->n_bases + 32) rc = MCX_ERR_CAPACITY;
        else {
            uint32_t at = 0;
            for (uint32_t r = 0; r < n; r++) {
                const mcx_fastq_rec &c = recs[r];
                const bool rev = (flags[r] & 0x10u) != 0;
                out->off[r] = at;
                for (uint32_t i = 0; i < c.rlen; i++) out->bases[at + i] = letter_of(nibble_of(text + c.seq, c.rlen, rev, i));
                if (out->qual) for (uint32_t i = 0; i < c.rlen; i++) out->qual[at + i] = c.q_take ? qual_of(text + c.qual, c.rlen, rev, i) : (uint8_t)0;
                at += c.rlen;
            }
            out->off[n] = at;
        }
    }
    if (out->names) {
        if (out->names_cap < info->n_name_bytes) rc = MCX_ERR_CAPACITY;
        else {
            uint32_t at = 0;
            for (uint32_t r = 0; r < n; r++) {
                out->name_off[r] = at;
                memcpy(out->names + at, text + recs[r].name, recs[r].name_len);
                at += recs[r].name_len;
            }
            out->name_off[n] = at;
        }
    }
    if (out->rows) {
        if (out->odd_cap < info->n_odd) rc = MCX_ERR_CAPACITY;
        else {
            uint32_t n_odd = 0;
            for (uint32_t r = 0; r < n; r++) {
                const mcx_fastq_rec &c = recs[r];
                const bool rev = (flags[r] & 0x10u) != 0;
                uint32_t *row = out->rows + (size_t)r * out->row_words;
                uint32_t k = 0;
                for (uint32_t i = 0; i < c.rlen; i += 16, k++) row[k] = row_word(text + c.seq, c.rlen, rev, i, c.rlen - i < 16 ? c.rlen - i : 16);
                for (; k < out->row_words; k++) row[k] = 0;
                for (uint32_t i = 0; i < c.rlen; i++) {
                    const uint32_t nb = nibble_of(text + c.seq, c.rlen, rev, i);
                    if (odd_nibble(nb)) out->odd[n_odd++] = mcx::fq::odd_entry(r, i, letter_of(nb));
                }
                out->len[r] = c.rlen;
            }
        }
    }
    return rc;
}

#ifdef BAM_IN_CHECK_MAIN
// file: cases of { u32 kind (0: records, 1: a header), u32 max_read_len, i32 n_ref, u32 pad, u64 bytes, the bytes }
namespace {
int fail(const char *what, size_t c) { fprintf(stderr, "bam_in_check: case %zu: %s\n", c, what); return 1; }

int run_case(size_t c, const uint8_t *t0, uint64_t b0, int32_t max_len, int32_t n_ref)
{
    uint8_t *a = (uint8_t *)malloc(b0 ? b0 : 1); // (a heap copy of exactly the text's size: a read one byte outside it is reported)
    memcpy(a, t0, b0);
    const uint32_t bounds[] = {0, 1, 2, 3, (uint32_t)(b0 / 37 + 1)};
    int bad = 0;
    for (int mates = 0; mates < 2 && !bad; mates++)
        for (int fin = 0; fin < 2 && !bad; fin++)
            for (uint32_t mr : bounds) {
                mcx_fastq_in in; memset(&in, 0, sizeof in);
                in.text[0] = a; in.bytes[0] = b0; in.max_records = mr; in.max_read_len = max_len; in.final = fin; in.n_ref = n_ref;
                mcx_fastq_out none; memset(&none, 0, sizeof none);
                mcx_fastq_info need;
                if (bam_in_check_parse(&in, &none, mates, &need)) { bad = fail("the sizing call failed", c); break; }
                const uint32_t n = need.n_reads, rw = (uint32_t)((max_len + 15) / 16);
                mcx_fastq_out o; memset(&o, 0, sizeof o);
                o.recs[0] = (mcx_fastq_rec *)malloc((size_t)need.n_records[0] * sizeof(mcx_fastq_rec) + 1);
                o.bases_cap = need.n_bases + 32; o.names_cap = need.n_name_bytes; o.odd_cap = need.n_odd; o.row_words = rw;
                o.bases = (uint8_t *)malloc(o.bases_cap); o.qual = (uint8_t *)malloc(o.bases_cap); o.off = (uint32_t *)malloc((size_t)(n + 1) * 4);
                o.names = (uint8_t *)malloc(o.names_cap + 1); o.name_off = (uint32_t *)malloc((size_t)(n + 1) * 4);
                o.rows = (uint32_t *)malloc((size_t)n * rw * 4 + 1); o.len = (uint32_t *)malloc((size_t)n * 4 + 1); o.odd = (uint64_t *)malloc((size_t)o.odd_cap * 8 + 1);
                mcx_fastq_info info;
                if (bam_in_check_parse(&in, &o, mates, &info)) bad = fail("the call failed with buffers of the sizes it asked for", c);
                else if (memcmp(&info, &need, sizeof info)) bad = fail("two calls disagree", c);
                else if (o.off[n] != info.n_bases || o.name_off[n] != info.n_name_bytes) bad = fail("the last offset is not the total", c);
                else if (info.n_records[0] > mr || info.consumed[0] > b0 || (mates && (info.n_records[0] & 1))) bad = fail("counts out of range", c);
                void *p[] = {o.recs[0], o.bases, o.qual, o.off, o.names, o.name_off, o.rows, o.len, o.odd};
                for (void *q : p) free(q);
                if (bad) break;
            }
    free(a);
    return bad;
}

int run_header(size_t c, const uint8_t *t0, uint64_t b0)
{
    for (uint64_t cut = 0; cut <= b0; cut += (b0 > 4096 && cut > 64 && cut + 64 < b0 ? 997 : 1)) { // (every byte of a small header; of a large one its ends and a stride)
        uint8_t *a = (uint8_t *)malloc(cut ? cut : 1);
        memcpy(a, t0, cut);
        uint64_t at = 0; int32_t n_ref = 0;
        const int rc = reads_header(a, cut, &at, &n_ref);
        free(a);
        if (rc == 0 && at > cut) return fail("a header's end behind the bytes given", c);
    }
    return 0;
}
} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: bam_in_check cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "bam_in_check: cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + n);
    fclose(f);
    size_t at = 0, c = 0;
    while (at < d.size()) {
        if (d.size() - at < 24) return fail("a cut case header", c);
        uint32_t kind, max_len; int32_t n_ref; uint64_t b;
        memcpy(&kind, &d[at], 4); memcpy(&max_len, &d[at + 4], 4); memcpy(&n_ref, &d[at + 8], 4); memcpy(&b, &d[at + 16], 8);
        at += 24;
        if (kind > 1 || b > d.size() - at) return fail("a damaged case header", c);
        if (kind == 0 ? run_case(c, d.data() + at, b, (int32_t)max_len, n_ref) : run_header(c, d.data() + at, b)) return 1;
        at += b; c++;
    }
    return 0;
}
#endif
