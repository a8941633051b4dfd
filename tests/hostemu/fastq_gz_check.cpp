// tests/hostemu/fastq_gz_check.cpp — mcx_fastq_parse's contract under the GZ rule (MCX_FASTQ_RULE_GZ) on the host, one thread, built only from
// mapcaller_amd/csrc/mcx_fastq.h: the steps the kernels of mcx_fastq.hip take — line starts, pieces per line, their exclusive sums, the piece table by a search
// per entry, the records over that table — run in sequence.  tests/test_bgzf_resident.py builds it as a shared object (fastq_gz_check_parse: the call's
// arguments, host pointers) and, with -DFASTQ_GZ_CHECK_MAIN, as a stand-alone program for -fsanitize=address,undefined: it reads a file of texts and parses
// each with final 0 and 1 and max_records 0 .. 3 and unbounded, into heap buffers of exactly the contract's sizes (tests/hostemu/fastq_check.cpp's driver).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mapcaller_amd/csrc/mcx_fastq.h"

using namespace mcx::fq;

extern "C" int fastq_gz_check_parse(const mcx_fastq_in *in, const mcx_fastq_out *out, mcx_fastq_info *info)
{
    memset(info, 0, sizeof *info);
    const int nt = in->text[1] ? 2 : 1;
    for (int t = 0; t < nt; t++) if (in->bytes[t] >= (1ull << 32)) return MCX_ERR_ARG;
    if (out->rows && (int64_t)out->row_words * 16 < (int64_t)in->max_read_len) return MCX_ERR_ARG;
    std::vector<mcx_fastq_rec> recs[2];
    for (int t = 0; t < nt; t++) {
        const uint8_t *text = in->text[t];
        const uint32_t bytes = (uint32_t)in->bytes[t];
        const uint32_t eff_max = (uint32_t)(in->max_records < (uint64_t)bytes / 3 + 1 ? in->max_records : (uint64_t)bytes / 3 + 1); // (as the device bounds its tables)
        std::vector<uint32_t> ls(1, 0u);
        bool any_nul = false;
        for (uint32_t i = 0; i < bytes; i++) { if (text[i] == '\n') ls.push_back(i + 1); any_nul |= text[i] == 0; }
        const uint64_t n_nl = ls.size() - 1;
        // the piece table, of exactly the 4 * eff_max + 1 entries the device keeps (heap: a read or write outside them is reported)
        const uint32_t n_tab = 4u * eff_max + 1;
        const uint32_t n_counted = gz_lines_counted(ls.data(), n_nl, bytes, eff_max);
        std::vector<uint32_t> pc(n_tab), po(n_tab), ps(n_tab, 0xFFFFFFFFu);
        for (uint32_t L = 0; L < n_tab; L++) pc[L] = gz_line_pieces(ls.data(), n_nl, bytes, n_counted, L);
        for (uint32_t L = 0, sum = 0; L < n_tab; L++) { po[L] = sum; sum += pc[L]; }
        for (uint32_t q = 0; q < n_tab; q++) { uint32_t s; if (gz_piece_entry(ls.data(), n_nl, bytes, po.data(), eff_max, n_counted, q, s)) ps[q] = s; }
        const uint64_t n_p = gz_pieces_counted(po.data(), eff_max);
        uint32_t n = 0, stop = MCX_FASTQ_MORE;
        for (; n < eff_max; n++) {
            if (!in->final && !gz_record_whole(text, bytes, ps.data(), n_p, n)) break;
            mcx_fastq_rec rec;
            memset(&rec, 0, sizeof rec);
            stop = gz_record_of(text, bytes, ps.data(), n_p, n, in->max_read_len, any_nul, rec);
            if (stop != MCX_FASTQ_MORE) break;
            recs[t].push_back(rec);
        }
        info->n_records[t] = n; info->stop[t] = stop;
        info->consumed[t] = 4ull * n <= n_p ? ps[4ull * n] : bytes;
        if (out->recs[t]) for (uint32_t i = 0; i < n; i++) out->recs[t][i] = recs[t][i];
    }
    const uint32_t n_reads = nt == 2 ? 2 * (info->n_records[0] < info->n_records[1] ? info->n_records[0] : info->n_records[1]) : info->n_records[0];
    info->n_reads = n_reads;
    auto rec_of = [&](uint32_t r) -> const mcx_fastq_rec & { return nt == 2 ? recs[r & 1][r >> 1] : recs[0][r]; };
    auto text_of = [&](uint32_t r) { return in->text[nt == 2 ? (r & 1) : 0]; };
    for (uint32_t r = 0; r < n_reads; r++) {
        const mcx_fastq_rec &c = rec_of(r);
        info->n_bases += c.rlen; info->n_name_bytes += c.name_len;
        if (c.rlen > info->longest) info->longest = c.rlen;
        for (uint32_t i = 0; i < c.rlen; i++) info->n_odd += code_of(text_of(r)[c.seq + i]) > 3;
    }
    int rc = 0;
    if (out->bases) {
        if (out->bases_cap < info->n_bases + 32) rc = MCX_ERR_CAPACITY;
        else {
            uint32_t at = 0;
            for (uint32_t r = 0; r < n_reads; r++) {
                const mcx_fastq_rec &c = rec_of(r);
                out->off[r] = at;
                memcpy(out->bases + at, text_of(r) + c.seq, c.rlen);
                if (out->qual) { memcpy(out->qual + at, text_of(r) + c.qual, c.q_take); memset(out->qual + at + c.q_take, 0, c.rlen - c.q_take); }
                at += c.rlen;
            }
            out->off[n_reads] = at;
        }
    }
    if (out->names) {
        if (out->names_cap < info->n_name_bytes) rc = MCX_ERR_CAPACITY;
        else {
            uint32_t at = 0;
            for (uint32_t r = 0; r < n_reads; r++) {
                const mcx_fastq_rec &c = rec_of(r);
                out->name_off[r] = at;
                memcpy(out->names + at, text_of(r) + c.name, c.name_len);
                at += c.name_len;
            }
            out->name_off[n_reads] = at;
        }
    }
    if (out->rows) {
        if (out->odd_cap < info->n_odd) rc = MCX_ERR_CAPACITY;
        else {
            uint32_t n_odd = 0;
            for (uint32_t r = 0; r < n_reads; r++) {
                const mcx_fastq_rec &c = rec_of(r);
                const uint8_t *seq = text_of(r) + c.seq;
                uint32_t *row = out->rows + (size_t)r * out->row_words;
                uint32_t k = 0;
                for (uint32_t i = 0; i < c.rlen; i += 16, k++) row[k] = pack_word(seq, i, c.rlen - i < 16 ? c.rlen - i : 16);
                for (; k < out->row_words; k++) row[k] = 0;
                for (uint32_t i = 0; i < c.rlen; i++) if (code_of(seq[i]) > 3) out->odd[n_odd++] = odd_entry(r, i, seq[i]);
                out->len[r] = c.rlen;
            }
        }
    }
    return rc;
}

#ifdef FASTQ_GZ_CHECK_MAIN
// file: cases of { u32 n_texts, u32 max_read_len, u64 bytes[2], text 0, text 1 }
namespace {
int fail(const char *what, size_t c) { fprintf(stderr, "fastq_gz_check: case %zu: %s\n", c, what); return 1; }

int run_case(size_t c, const uint8_t *t0, uint64_t b0, const uint8_t *t1, uint64_t b1, int nt, int32_t max_len)
{
    // (heap copies of exactly the texts' sizes: a read one byte outside them is reported)
    uint8_t *a = (uint8_t *)malloc(b0 ? b0 : 1), *b = (uint8_t *)malloc(b1 ? b1 : 1);
    memcpy(a, t0, b0); memcpy(b, t1, b1);
    const uint32_t bounds[] = {0, 1, 2, 3, (uint32_t)((b0 > b1 ? b0 : b1) / 3 + 1)};
    int bad = 0;
    for (int fin = 0; fin < 2 && !bad; fin++)
        for (uint32_t mr : bounds) {
            mcx_fastq_in in; memset(&in, 0, sizeof in);
            in.text[0] = a; in.bytes[0] = b0;
            if (nt == 2) { in.text[1] = b; in.bytes[1] = b1; }
            in.max_records = mr; in.max_read_len = max_len; in.final = fin;
            mcx_fastq_out none; memset(&none, 0, sizeof none);
            mcx_fastq_info need;
            if (fastq_gz_check_parse(&in, &none, &need)) { bad = fail("the sizing call failed", c); break; }
            const uint32_t n = need.n_reads, rw = (uint32_t)((max_len + 15) / 16);
            mcx_fastq_out o; memset(&o, 0, sizeof o);
            for (int t = 0; t < nt; t++) o.recs[t] = (mcx_fastq_rec *)malloc((size_t)need.n_records[t] * sizeof(mcx_fastq_rec));
            o.bases_cap = need.n_bases + 32; o.names_cap = need.n_name_bytes; o.odd_cap = need.n_odd; o.row_words = rw;
            o.bases = (uint8_t *)malloc(o.bases_cap); o.qual = (uint8_t *)malloc(o.bases_cap); o.off = (uint32_t *)malloc((size_t)(n + 1) * 4);
            o.names = (uint8_t *)malloc(o.names_cap); o.name_off = (uint32_t *)malloc((size_t)(n + 1) * 4);
            o.rows = (uint32_t *)malloc((size_t)n * rw * 4); o.len = (uint32_t *)malloc((size_t)n * 4); o.odd = (uint64_t *)malloc((size_t)o.odd_cap * 8);
            mcx_fastq_info info;
            if (fastq_gz_check_parse(&in, &o, &info)) bad = fail("the call failed with buffers of the sizes it asked for", c);
            else if (memcmp(&info, &need, sizeof info)) bad = fail("two calls disagree", c);
            else if (o.off[n] != info.n_bases || o.name_off[n] != info.n_name_bytes) bad = fail("the last offset is not the total", c);
            else if (info.n_records[0] > mr || info.consumed[0] > b0 || info.consumed[1] > b1) bad = fail("counts out of range", c);
            else if (o.odd_cap) { mcx_fastq_out s = o; s.odd_cap--; if (fastq_gz_check_parse(&in, &s, &info) != MCX_ERR_CAPACITY) bad = fail("a short odd list was not refused", c); }
            void *p[] = {o.recs[0], o.recs[1], o.bases, o.qual, o.off, o.names, o.name_off, o.rows, o.len, o.odd};
            for (void *q : p) free(q);
            if (bad) break;
        }
    free(a); free(b);
    return bad;
}
} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: fastq_gz_check cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "fastq_gz_check: cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + n);
    fclose(f);
    size_t at = 0, c = 0;
    while (at < d.size()) {
        if (d.size() - at < 24) return fail("a cut header", c);
        uint32_t nt, max_len; uint64_t b[2];
        memcpy(&nt, &d[at], 4); memcpy(&max_len, &d[at + 4], 4); memcpy(b, &d[at + 8], 16);
        at += 24;
        if ((nt != 1 && nt != 2) || b[0] > d.size() - at || b[1] > d.size() - at - b[0]) return fail("a damaged header", c);
        if (run_case(c, d.data() + at, b[0], d.data() + at + b[0], b[1], (int)nt, (int32_t)max_len)) return 1;
        at += b[0] + b[1]; c++;
    }
    return 0;
}
#endif
