// tests/hostemu/fasta_check.cpp — mcx_fastq_parse's contract for FASTA text (MCX_READS_FASTA) under both rules on the host, one thread, built only from
// mapcaller_amd/csrc/mcx_fastq.h: the steps the kernels of mcx_fastq.hip take — line starts, per line its header flag and payload, their exclusive sums, the
// headers' lines, the records over those tables, the bases gathered line by line (plain rule); the piece table and the records two pieces apiece (GZ rule) —
// run in sequence.  tests/test_fasta_device.py builds it as a shared object (fasta_check_parse: the call's arguments, host pointers, and the rule) and, with
// -DFASTA_CHECK_MAIN, as a stand-alone program for -fsanitize=address,undefined: it reads a file of texts and parses each under both rules with final 0 and 1
// and max_records 0 .. 3 and unbounded, into heap buffers of exactly the contract's sizes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mapcaller_amd/csrc/mcx_fastq.h"

using namespace mcx::fq;

extern "C" int fasta_check_parse(const mcx_fastq_in *in, const mcx_fastq_out *out, mcx_fastq_info *info, int rule)
{
    memset(info, 0, sizeof *info);
    const int nt = in->text[1] ? 2 : 1;
    for (int t = 0; t < nt; t++) if (in->bytes[t] >= (1ull << 32)) return MCX_ERR_ARG;
    if (out->rows && (int64_t)out->row_words * 16 < (int64_t)in->max_read_len) return MCX_ERR_ARG;
    if (rule != MCX_FASTQ_RULE_PLAIN && rule != MCX_FASTQ_RULE_GZ) return MCX_ERR_ARG;
    std::vector<mcx_fastq_rec> recs[2];
    std::vector<std::vector<uint8_t>> seqs[2]; // a record's bases back to back, as the gather leaves them
    for (int t = 0; t < nt; t++) {
        const uint8_t *text = in->text[t];
        const uint32_t bytes = (uint32_t)in->bytes[t];
        const uint32_t eff_max = (uint32_t)(in->max_records < (uint64_t)bytes / 3 + 1 ? in->max_records : (uint64_t)bytes / 3 + 1); // (as the device bounds its tables)
        std::vector<uint32_t> ls(1, 0u);
        bool any_nul = false;
        for (uint32_t i = 0; i < bytes; i++) { if (text[i] == '\n') ls.push_back(i + 1); any_nul |= text[i] == 0; }
        const uint64_t n_nl = ls.size() - 1;
        uint32_t n = 0, stop = MCX_FASTQ_MORE;
        if (rule == MCX_FASTQ_RULE_PLAIN) {
            // tables of exactly the n_nl + 2 entries the device keeps (heap: a read or write outside them is reported)
            const uint32_t n_tab = (uint32_t)n_nl + 2, n_lines = fa_n_lines(ls.data(), n_nl, bytes);
            std::vector<uint32_t> fh(n_tab), fp(n_tab), hn(n_tab), bo(n_tab), hl(n_tab, 0xFFFFFFFFu);
            for (uint32_t L = 0; L < n_tab; L++) fa_line(text, bytes, ls.data(), n_nl, n_lines, L, fh[L], fp[L]);
            for (uint32_t L = 0, a = 0, b = 0; L < n_tab; L++) { hn[L] = a; bo[L] = b; a += fh[L]; b += fp[L]; }
            for (uint32_t L = 0; L <= n_lines; L++) if (L == n_lines || fh[L]) hl[hn[L]] = L;
            const uint32_t n_hdr = hn[n_lines];
            for (; n < eff_max; n++) {
                mcx_fastq_rec rec;
                memset(&rec, 0, sizeof rec);
                bool taken;
                stop = fa_record_of(text, bytes, ls.data(), n_nl, bo.data(), hl.data(), n_hdr, n, in->max_read_len, in->final, rec, taken);
                if (!taken) break;
                recs[t].push_back(rec);
                std::vector<uint8_t> seq(rec.rlen);
                for (uint32_t L = hl[n] + 1; L < hl[n + 1]; L++) // k_fa_gather
                    for (uint32_t i = 0; i < bo[L + 1] - bo[L]; i++) seq[bo[L] - bo[hl[n]] + i] = text[ls[L] + i];
                seqs[t].push_back(seq);
            }
            info->consumed[t] = fa_consumed(ls.data(), hl.data(), n_hdr, n, bytes);
        } else {
            const uint32_t n_tab = 4u * eff_max + 1;
            const uint32_t n_counted = gz_lines_counted(ls.data(), n_nl, bytes, eff_max);
            std::vector<uint32_t> pc(n_tab), po(n_tab), ps(n_tab, 0xFFFFFFFFu);
            for (uint32_t L = 0; L < n_tab; L++) pc[L] = gz_line_pieces(ls.data(), n_nl, bytes, n_counted, L);
            for (uint32_t L = 0, sum = 0; L < n_tab; L++) { po[L] = sum; sum += pc[L]; }
            for (uint32_t q = 0; q < n_tab; q++) { uint32_t s; if (gz_piece_entry(ls.data(), n_nl, bytes, po.data(), eff_max, n_counted, q, s)) ps[q] = s; }
            const uint64_t n_p = gz_pieces_counted(po.data(), eff_max);
            for (; n < eff_max; n++) {
                if (!in->final && !gz_record_whole(text, bytes, ps.data(), n_p, n, 2)) break;
                mcx_fastq_rec rec;
                memset(&rec, 0, sizeof rec);
                stop = gz_record_of(text, bytes, ps.data(), n_p, n, in->max_read_len, any_nul, rec, 2);
                if (stop != MCX_FASTQ_MORE) break;
                recs[t].push_back(rec);
                seqs[t].push_back(std::vector<uint8_t>(text + rec.seq, text + rec.seq + rec.rlen));
            }
            if (n == eff_max) stop = MCX_FASTQ_MORE;
            info->consumed[t] = 2ull * n <= n_p ? ps[2ull * n] : bytes;
        }
        if (n == eff_max) stop = MCX_FASTQ_MORE;
        info->n_records[t] = n; info->stop[t] = stop;
        if (out->recs[t]) for (uint32_t i = 0; i < n; i++) out->recs[t][i] = recs[t][i];
    }
    const uint32_t n_reads = nt == 2 ? 2 * (info->n_records[0] < info->n_records[1] ? info->n_records[0] : info->n_records[1]) : info->n_records[0];
    info->n_reads = n_reads;
    auto rec_of = [&](uint32_t r) -> const mcx_fastq_rec & { return nt == 2 ? recs[r & 1][r >> 1] : recs[0][r]; };
    auto seq_of = [&](uint32_t r) -> const uint8_t * { return nt == 2 ? seqs[r & 1][r >> 1].data() : seqs[0][r].data(); };
    auto text_of = [&](uint32_t r) { return in->text[nt == 2 ? (r & 1) : 0]; };
    for (uint32_t r = 0; r < n_reads; r++) {
        const mcx_fastq_rec &c = rec_of(r);
        info->n_bases += c.rlen; info->n_name_bytes += c.name_len;
        if (c.rlen > info->longest) info->longest = c.rlen;
        for (uint32_t i = 0; i < c.rlen; i++) info->n_odd += code_of(seq_of(r)[i]) > 3;
    }
    int rc = 0;
    if (out->bases) {
        if (out->bases_cap < info->n_bases + 32) rc = MCX_ERR_CAPACITY;
        else {
            uint32_t at = 0;
            for (uint32_t r = 0; r < n_reads; r++) {
                const mcx_fastq_rec &c = rec_of(r);
                out->off[r] = at;
                if (c.rlen) memcpy(out->bases + at, seq_of(r), c.rlen);
                if (out->qual) memset(out->qual + at, 0, c.rlen); // (no quality: q_take = 0)
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
                if (c.name_len) memcpy(out->names + at, text_of(r) + c.name, c.name_len);
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
                const uint8_t *seq = seq_of(r);
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

#ifdef FASTA_CHECK_MAIN
// file: cases of { u32 n_texts, u32 max_read_len, u64 bytes[2], text 0, text 1 }
namespace {
int fail(const char *what, size_t c) { fprintf(stderr, "fasta_check: case %zu: %s\n", c, what); return 1; }

int run_case(size_t c, const uint8_t *t0, uint64_t b0, const uint8_t *t1, uint64_t b1, int nt, int32_t max_len)
{
    // (heap copies of exactly the texts' sizes: a read one byte outside them is reported)
    uint8_t *a = (uint8_t *)malloc(b0 ? b0 : 1), *b = (uint8_t *)malloc(b1 ? b1 : 1);
    memcpy(a, t0, b0); memcpy(b, t1, b1);
    const uint32_t bounds[] = {0, 1, 2, 3, (uint32_t)((b0 > b1 ? b0 : b1) / 3 + 1)};
    int bad = 0;
    for (int rule = 0; rule < 2 && !bad; rule++)
    for (int fin = 0; fin < 2 && !bad; fin++)
        for (uint32_t mr : bounds) {
            mcx_fastq_in in; memset(&in, 0, sizeof in);
            in.text[0] = a; in.bytes[0] = b0;
            if (nt == 2) { in.text[1] = b; in.bytes[1] = b1; }
            in.max_records = mr; in.max_read_len = max_len; in.final = fin;
            mcx_fastq_out none; memset(&none, 0, sizeof none);
            mcx_fastq_info need;
            if (fasta_check_parse(&in, &none, &need, rule)) { bad = fail("the sizing call failed", c); break; }
            const uint32_t n = need.n_reads, rw = (uint32_t)((max_len + 15) / 16);
            mcx_fastq_out o; memset(&o, 0, sizeof o);
            for (int t = 0; t < nt; t++) o.recs[t] = (mcx_fastq_rec *)malloc((size_t)need.n_records[t] * sizeof(mcx_fastq_rec));
            o.bases_cap = need.n_bases + 32; o.names_cap = need.n_name_bytes; o.odd_cap = need.n_odd; o.row_words = rw;
            o.bases = (uint8_t *)malloc(o.bases_cap); o.qual = (uint8_t *)malloc(o.bases_cap); o.off = (uint32_t *)malloc((size_t)(n + 1) * 4);
            o.names = (uint8_t *)malloc(o.names_cap ? o.names_cap : 1); o.name_off = (uint32_t *)malloc((size_t)(n + 1) * 4);
            o.rows = (uint32_t *)malloc((size_t)n * rw * 4 + 4); o.len = (uint32_t *)malloc((size_t)n * 4 + 4); o.odd = (uint64_t *)malloc((size_t)o.odd_cap * 8 + 8);
            mcx_fastq_info info;
            if (fasta_check_parse(&in, &o, &info, rule)) bad = fail("the call failed with buffers of the sizes it asked for", c);
            else if (memcmp(&info, &need, sizeof info)) bad = fail("two calls disagree", c);
            else if (o.off[n] != info.n_bases || o.name_off[n] != info.n_name_bytes) bad = fail("the last offset is not the total", c);
            else if (info.n_records[0] > mr || info.consumed[0] > b0 || info.consumed[1] > b1) bad = fail("counts out of range", c);
            else if (o.odd_cap) { mcx_fastq_out s = o; s.odd_cap--; if (fasta_check_parse(&in, &s, &info, rule) != MCX_ERR_CAPACITY) bad = fail("a short odd list was not refused", c); }
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
    if (argc < 2) { fprintf(stderr, "usage: fasta_check cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "fasta_check: cannot open %s\n", argv[1]); return 2; }
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
