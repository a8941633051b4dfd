// mapcaller_amd/csrc/mcx_batch.h — the file front end's batch object (what one batch of reads carries from the reader through the device to the writer,
// with its page-locked buffers) and the host formatter over it: SAM text as GeneratePairedSamStream / GenerateSingleSamStream make it.
#pragma once
#include "mcx_reader.h"
#include "mcx_sam.h"

namespace mcx { namespace files {

// ---- SAM text (GeneratePairedSamStream / GenerateSingleSamStream, SamReport.cpp:324-488) --------------------
inline char comp_char(char c) // GetComplementaryBase, tools.cpp:3-18
{
    switch (c) {
    case 'A': case 'a': return 'T';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    case 'T': case 't': return 'A';
    default: return 'N';
    }
}

struct Text { // writer over a buffer sized beforehand from an upper bound
    std::vector<char> b;
    char *w = nullptr;
    void start(size_t bound) { if (b.size() < bound) b.resize(bound); w = b.data(); }
    size_t size() const { return w ? (size_t)(w - b.data()) : 0; }
    void put(const char *p, size_t n) { memcpy(w, p, n); w += n; }
    void put(char c) { *w++ = c; }
    void lit(const char *s) { put(s, strlen(s)); }
    void num(long long v)
    {
        char t[24]; int n = 0;
        unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
        do { t[n++] = (char)('0' + u % 10); u /= 10; } while (u);
        if (v < 0) t[n++] = '-';
        while (n) *w++ = t[--n];
    }
};

// ---- a batch on its way through the stages -------------------------------------------------------------
struct Batch {
    View in[2];
    uint32_t n = 0;          // reads
    uint64_t number = 0;     // position of the batch in the input stream
    bool two_files = false, fastq = true, last = false;
    std::string error;
    // what crosses the device boundary, in page-locked memory (allocated once per batch object): 2-bit rows, lengths and the
    // bytes that are not ACGT on the way in; records and CIGAR words on the way out
    uint32_t *rows = nullptr, *lens = nullptr; uint64_t *odd = nullptr; mcx_aln32 *recs = nullptr; uint32_t *cig = nullptr; // (the records as they cross PCIe: 32 bytes each)
    size_t cap_reads = 0, cap_rows = 0, cap_odd = 0;
    uint32_t row_words = 0, n_odd[2] = {0, 0};
    std::vector<uint8_t> is_mate2;   // mapped as the second read of a pair
    uint32_t n_pair_reads = 0;       // reads [0, n_pair_reads) are mapped as pairs, the rest one by one: two parts, two CIGAR pools
    std::vector<Text> slices;        // the batch's SAM text
    uint64_t sam_bytes = 0;
    // -m: each part's extra lines, arrived with its records (mcx_stream_collect -> mcx_stream_multi): those of the part's read r are
    // recs[index[r] .. index[r + 1]), their cigar_off into cig
    struct Extras { std::vector<uint32_t> index, cig; std::vector<mcx_aln> recs; } mx[2];
    bool has_mx = false;
    // -md without device_sam: each part's MD strings, copied out behind its mapping (mcx_md_part_host): those of the part's read r at off[r], of its extra i at
    // off[part's reads + i] (the layout of mcx_md_dev)
    struct Md { std::vector<uint8_t> bytes; std::vector<uint32_t> off; } md[2];
    bool has_md = false;
    // -rg / -mc for the host formatter: the read group's ID (the run's; null: none) and whether the pairs' lines get MC and MQ
    const std::string *rg = nullptr;
    bool mate_tags = false;
    std::deque<bool> parts_out; // the parts on their way out, oldest first (true: the single-read part)
    // device_sam: the names and NUL-padded qualities of the batch's two parts on their way to the device (page-locked; a part's names back to back with
    // offsets that start at 0: the pairs' are sam_name_off[0 .. n_pair_reads], the single reads' sam_name_off[n_pair_reads + 1 .. n + 1]), and the text that came back
    uint8_t *sam_names = nullptr, *sam_qual = nullptr, *dev_text = nullptr; uint32_t *sam_name_off = nullptr;
    uint64_t cap_sam_names = 0, cap_sam_qual = 0, cap_sam_off = 0, dev_text_cap = 0, dev_bytes = 0;
    uint64_t sam_part_names[2] = {0, 0}, sam_part_qual[2] = {0, 0};
    std::vector<uint64_t> sam_qual_at;
    // the resident route (-gpu_inflate -gpu_parse on BGZF FASTQ): the batch's rows, lengths, odd bytes, names and qualities lie in device buffers that belong
    // to this object (made and grown by mcx_resident_next); `rb` says where.  `in[]` then holds counts only.
    mcx_resident_bufs *res = nullptr;
    mcx_resident_batch rb;
    bool resident = false;
    int error_rc = 0; // the code that goes with `error` where it is not the reader's own (a device that ran out of room: MCX_ERR_DEVICE)
    // an object from the spare queue becomes batch `number` of the input: no reads yet; every buffer keeps its capacity
    void reset(bool two, bool fq, uint64_t num)
    {
        two_files = two; fastq = fq; n = 0; last = false; error.clear(); number = num;
        in[0].clear(); in[1].clear(); n_odd[0] = n_odd[1] = 0; n_pair_reads = 0;
        resident = false; error_rc = 0;
    }
    // the code that goes with `error`
    int error_code() const { return error_rc ? error_rc : error.find("max_read_len") != std::string::npos ? MCX_ERR_UNSUPPORTED : MCX_ERR_IO; }
    bool reserve_sam(uint64_t reads, uint64_t names, uint64_t qual)
    {
        if (reads + 2 > cap_sam_off) { mcx_pinned_free(sam_name_off); cap_sam_off = reads + 2; sam_name_off = (uint32_t *)mcx_pinned_alloc(cap_sam_off * sizeof(uint32_t)); }
        if (names > cap_sam_names) { mcx_pinned_free(sam_names); cap_sam_names = names + names / 8 + 4096; sam_names = (uint8_t *)mcx_pinned_alloc(cap_sam_names); }
        if (qual > cap_sam_qual) { mcx_pinned_free(sam_qual); cap_sam_qual = qual + qual / 8 + 4096; sam_qual = (uint8_t *)mcx_pinned_alloc(cap_sam_qual); }
        return sam_name_off && (sam_names || !names) && (sam_qual || !qual);
    }
    bool reserve(size_t reads, size_t words_per_read)
    {
        if (reads > cap_reads) {
            mcx_pinned_free(lens); mcx_pinned_free(recs); mcx_pinned_free(cig);
            cap_reads = reads;
            lens = (uint32_t *)mcx_pinned_alloc((reads + 1) * sizeof(uint32_t));
            recs = (mcx_aln32 *)mcx_pinned_alloc(reads * sizeof(mcx_aln32));
            cig = (uint32_t *)mcx_pinned_alloc((MCX_CIGAR_POOL_WORDS(reads) + MCX_CIGAR_SLACK) * sizeof(uint32_t)); // (two pools: the pairs', the single reads')
        }
        if (reads * words_per_read > cap_rows) { mcx_pinned_free(rows); cap_rows = reads * words_per_read; rows = (uint32_t *)mcx_pinned_alloc(cap_rows * sizeof(uint32_t)); }
        return lens && recs && cig && rows;
    }
    bool reserve_odd(size_t n)
    {
        if (n > cap_odd) { mcx_pinned_free(odd); cap_odd = n + n / 2 + 1024; odd = (uint64_t *)mcx_pinned_alloc(cap_odd * sizeof(uint64_t)); }
        return odd != nullptr;
    }
    ~Batch() { mcx_resident_bufs_free(res); mcx_pinned_free(rows); mcx_pinned_free(lens); mcx_pinned_free(odd); mcx_pinned_free(recs); mcx_pinned_free(cig); mcx_pinned_free(sam_names); mcx_pinned_free(sam_qual); mcx_pinned_free(sam_name_off); mcx_pinned_free(dev_text); }
    // read r of the batch -> (file, index in that file's records)
    const Rec &rec(uint32_t r, const char *&base) const
    {
        const int f = two_files ? (int)(r & 1) : 0;
        base = in[f].base;
        return in[f].recs[two_files ? r >> 1 : r];
    }
    int n_parts() const { return n == 0 ? 0 : (n_pair_reads ? 1 : 0) + (n_pair_reads < n ? 1 : 0); }
};

// bytes one SAM line can take at most
inline size_t sam_bound(const HostIndex &ix, size_t name_len, size_t rlen, int chr, int n_cigar)
{
    return name_len + 2 * rlen + (chr >= 0 ? ix.chr_name[chr].size() : 1) + 11 * (size_t)(n_cigar > 0 ? n_cigar : 0) + 160;
}

// one SAM line of read r: `rec` with its operations at `cigar`
// (tail: what the line carries behind XS — MD, MC and MQ, RG — written by mcx_sam.h's sam_tail_put: the bytes of the device formatter)
inline void sam_line(const HostIndex &ix, const Batch &bt, uint32_t r, const mcx_aln &rec, const uint32_t *cigar, Text &o, const SamTail &tail)
{
    const char *base;
    const Rec &e = bt.rec(r, base);
    const char *seq = base + e.seq;
    const int rlen = (int)e.rlen;
    const char *qual = bt.fastq ? base + e.qual : nullptr;
    o.put(base + e.name, e.name_len);
    const bool mapped = rec.chr >= 0;
    // The reference reverse-complements mate 2 in place before mapping (ReadMapping.cpp:451) and prints
    // that string for forward-strand hits and unmapped reads, its reverse complement otherwise.
    const bool flipped = bt.is_mate2[r] != 0;
    const bool again = mapped && rec.fwd == 0; // a second reverse complement for the output
    o.put('\t'); o.num(rec.flag); o.put('\t');
    if (!mapped) o.lit("*\t0\t0\t*\t*\t0\t0\t");
    else {
        const std::string &cn = ix.chr_name[rec.chr];
        o.put(cn.data(), cn.size()); o.put('\t'); o.num(rec.pos); o.put('\t'); o.num(rec.mapq); o.put('\t');
        o.w = (char *)sam_cigar_put((uint8_t *)o.w, cigar, rec.n_cigar); // (column 6 and the mate's MC:Z through one code)
        if (rec.has_mate) { o.lit("\t=\t"); o.num(rec.mate_pos); o.put('\t'); o.num(rec.tlen); o.put('\t'); }
        else o.lit("\t*\t0\t0\t");
    }
    if (!flipped && !again) o.put(seq, (size_t)rlen);
    else if (flipped != again) { char *w = o.w; for (int k = rlen - 1; k >= 0; k--) *w++ = comp_char(seq[k]); o.w = w; }
    else { char *w = o.w; for (int k = 0; k < rlen; k++) *w++ = comp_char(comp_char(seq[k])); o.w = w; } // complemented twice: upper case, N for anything else
    o.put('\t');
    if (!qual) o.put('*');
    else {
        // the quality string as the reference holds it: q_take bytes of the line, NUL from there to the read's length (strncpy);
        // printed with %s — and its reversed copy, when the line was short, begins with that NUL
        const size_t ql = strnlen(qual, (size_t)e.q_take);
        if (flipped == again) o.put(qual, ql);
        else if (e.q_take == e.rlen) { char *w = o.w; for (int k = rlen - 1; k >= 0 && qual[k] != '\0'; k--) *w++ = qual[k]; o.w = w; }
    }
    if (!mapped) o.lit("\tAS:i:0\tXS:i:0\n");
    else { o.lit("\tNM:i:"); o.num(rec.nm); o.lit("\tAS:i:"); o.num(rec.as); o.lit("\tXS:i:"); o.num(rec.xs); o.put('\n'); }
    o.w = (char *)sam_tail_put((uint8_t *)o.w, tail);
}

// what line `rec` of read r carries behind XS: its MD string (none without -md), the read group, and — for read r's own record in the pairs' part — its mate's
// CIGAR and MAPQ by the rule at mcx_sam_tags.  The mate is read r ^ 1: a pair's mates are always in the same part of a batch (the pairs' part is reads
// [0, n_pair_reads), an even number, with its own CIGAR pool), so r ^ 1 < n_pair_reads whenever r is.
inline SamTail host_tail(const Batch &bt, uint32_t r, const mcx_aln &rec, bool extra, const uint8_t *md, uint32_t md_len)
{
    SamTail t;
    t.md = md; t.md_len = md_len;
    t.mc = nullptr; t.mc_n = 0; t.mq = 0;
    if (bt.mate_tags && !extra && r < bt.n_pair_reads && (r ^ 1u) < bt.n_pair_reads && !(rec.flag & 8)) {
        mcx_aln m;
        mcx_aln_unpack(&bt.recs[r ^ 1u], &m);
        if (m.chr >= 0 && m.n_cigar > 0) { t.mc = bt.cig + (size_t)(uint32_t)m.cigar_off; t.mc_n = m.n_cigar; t.mq = m.mapq; }
    }
    t.rg = bt.rg && !bt.rg->empty() ? (const uint8_t *)bt.rg->data() : nullptr;
    t.rg_len = t.rg ? (uint32_t)bt.rg->size() : 0;
    return t;
}

// -md: the string of entry k of a part's pool (none without -md, or for a line without a tag)
inline uint32_t md_entry(const Batch &bt, int part, size_t k, const uint8_t *&md)
{
    md = nullptr;
    const Batch::Md &m = bt.md[part];
    if (!bt.has_md || k + 1 >= m.off.size()) return 0;
    md = m.bytes.data() + m.off[k];
    return m.off[k + 1] - m.off[k];
}

// -m: read r's extra lines (none without -m) — where they lie in its part's extras
inline void extra_range(const Batch &bt, uint32_t r, const Batch::Extras *&x, uint32_t &lo, uint32_t &hi)
{
    const int part = r < bt.n_pair_reads ? 0 : 1;
    const uint32_t k = part ? r - bt.n_pair_reads : r;
    x = &bt.mx[part];
    lo = hi = 0;
    if (bt.has_mx && (size_t)k + 1 < x->index.size()) { lo = x->index[k]; hi = x->index[k + 1]; }
}

// read r's line(s): the record of unique mode, then (-m) every further candidate with the best score (SamReport.cpp:364-488)
inline void sam_record(const HostIndex &ix, const Batch &bt, uint32_t r, Text &o)
{
    mcx_aln rec;
    mcx_aln_unpack(&bt.recs[r], &rec);
    // the batch's CIGAR pool (the single-read part of a batch has one of its own behind the pairs'), cigar_off = the read's place in it
    const uint32_t *cigar = bt.cig + (r < bt.n_pair_reads ? 0 : MCX_CIGAR_POOL_WORDS(bt.n_pair_reads)) + (size_t)(uint32_t)rec.cigar_off;
    const int part = r < bt.n_pair_reads ? 0 : 1;
    const uint32_t part_reads = part ? bt.n - bt.n_pair_reads : bt.n_pair_reads;
    const uint8_t *md;
    uint32_t ml = md_entry(bt, part, part ? r - bt.n_pair_reads : r, md);
    sam_line(ix, bt, r, rec, cigar, o, host_tail(bt, r, rec, false, md, ml));
    const Batch::Extras *x; uint32_t lo, hi;
    extra_range(bt, r, x, lo, hi);
    for (uint32_t i = lo; i < hi; i++) { ml = md_entry(bt, part, (size_t)part_reads + i, md); sam_line(ix, bt, r, x->recs[i], x->cig.data() + (uint32_t)x->recs[i].cigar_off, o, host_tail(bt, r, x->recs[i], true, md, ml)); }
}

// bytes read r's line(s) can take at most
inline size_t sam_bound_read(const HostIndex &ix, const Batch &bt, uint32_t r, size_t name_len, size_t rlen)
{
    size_t b = sam_bound(ix, name_len, rlen, bt.recs[r].chr == 0xFFFFu ? -1 : (int)bt.recs[r].chr, bt.recs[r].n_cigar);
    const Batch::Extras *x; uint32_t lo, hi;
    extra_range(bt, r, x, lo, hi);
    for (uint32_t i = lo; i < hi; i++) b += sam_bound(ix, name_len, rlen, x->recs[i].chr, x->recs[i].n_cigar);
    if (bt.has_md) { // the lines' MD tags
        const int part = r < bt.n_pair_reads ? 0 : 1;
        const uint32_t part_reads = part ? bt.n - bt.n_pair_reads : bt.n_pair_reads;
        const uint8_t *md;
        b += 6 + md_entry(bt, part, part ? r - bt.n_pair_reads : r, md);
        for (uint32_t i = lo; i < hi; i++) b += 6 + md_entry(bt, part, (size_t)part_reads + i, md);
    }
    const size_t lines = 1 + (hi - lo);
    if (bt.rg) b += lines * (6 + bt.rg->size()); // the lines' RG tags
    if (bt.mate_tags && r < bt.n_pair_reads && (r ^ 1u) < bt.n_pair_reads) b += 6 + 11 * (size_t)bt.recs[r ^ 1u].n_cigar + 6 + 11; // MC: the mate's operations; MQ
    return b;
}

}} // namespace mcx::files
