// tests/hostemu/simple_io.h — TEST HARNESS: a deliberately plain, single-threaded second
// implementation of what the product does in its file front end (mcx_reader.h, mcx_batch.h) (reading FASTA/FASTQ(.gz) like
// GetData.cpp, SAM text like SamReport.cpp) and of the avgDist replay the product runs on the
// device (k_chunk_sums / k_check_est).  The harness maps with the product's device headers and
// writes SAM through these, so the two implementations check each other against the golden files.
#ifndef HOSTEMU_SIMPLE_IO_H
#define HOSTEMU_SIMPLE_IO_H
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <zlib.h>

#include "../../mapcaller_amd/csrc/mcx_types.h"
#include "../../mapcaller_amd/csrc/mcx_host.h"

namespace mcx {

struct HostRead {
    std::string name, seq, qual;
};

class ReadFile {
public:
    bool open(const std::string &path, std::string &err);
    bool next(HostRead &r); // false at end of file
    void close();
    bool fastq() const { return fastq_; }
    ~ReadFile() { close(); }
private:
    bool line(std::string &s);
    void *gz_ = nullptr;
    bool fastq_ = true;
    std::string pending_;
    bool have_pending_ = false;
};

// one SAM line for a read (no trailing newline); rec/cigar as produced by the mapping stages
void sam_line(const HostIndex &ix, const HostRead &rd, bool mate2_flipped, bool fastq, const struct AlnRec &rec,
              const uint32_t *cigar, std::string &out);

// Replay of the reference's insert-size feedback over one batch (ReadMapping.cpp:462, :538-539):
// avgDist is re-estimated after every chunk of 100 pairs once more than 1000 proper pairs were
// seen, and the next chunk pairs its mates with EstiDistance = (int)(avgDist*1.5).  Each pair
// reports the interval of estimates that leaves its result unchanged; the pairs whose chunk
// estimate falls outside it are returned in redo/redo_est (to be re-run with the exact value).
// avg = {avgDist, iTotalPairedNum, TotalPairedDistance, reads seen}; avg_out gets the state
// after the batch (valid once redo comes back empty).
struct PairOut;
void avg_replay(const struct PairOut *po, uint32_t n_pairs, const int64_t avg[4], std::vector<uint32_t> &redo,
                std::vector<int32_t> &redo_est, int64_t avg_out[4]);


// ---------------------------------------------------------------------------------------------
inline bool ReadFile::open(const std::string &path, std::string &err)
{
    gzFile g = gzopen(path.c_str(), "rb");
    if (!g) { err = "cannot open " + path; return false; }
    gzbuffer(g, 1 << 20);
    gz_ = g;
    int c = gzgetc(g);
    fastq_ = (c == '@'); // CheckReadFormat, GetData.cpp:22-31
    if (c != -1) gzungetc(c, g);
    have_pending_ = false;
    return true;
}

inline void ReadFile::close()
{
    if (gz_) gzclose((gzFile)gz_);
    gz_ = nullptr;
}

inline bool ReadFile::line(std::string &s)
{
    if (have_pending_) { s.swap(pending_); have_pending_ = false; return true; }
    s.clear();
    char buf[4096];
    for (;;) {
        if (!gzgets((gzFile)gz_, buf, sizeof buf)) return !s.empty();
        s += buf;
        if (!s.empty() && s.back() == '\n') return true;
    }
}

// IdentifyHeaderBegPos / IdentifyHeaderEndPos, GetData.cpp:3-20
static std::string header_of(const std::string &l)
{
    const int len = (int)l.size();
    int p1 = len - 1, lim = len > 100 ? 100 : len, p2 = lim - 1;
    for (int i = 1; i < len; i++) if (l[i] != '>' && l[i] != '@') { p1 = i; break; }
    for (int i = 1; i < lim; i++) if (l[i] == ' ' || l[i] == '/' || !isprint((unsigned char)l[i])) { p2 = i; break; }
    return p2 > p1 ? l.substr(p1, p2 - p1) : std::string();
}

inline bool ReadFile::next(HostRead &r)
{
    std::string l;
    r.name.clear(); r.seq.clear(); r.qual.clear();
    if (!line(l)) return false;
    r.name = header_of(l);
    if (fastq_) {
        if (!line(l)) return false;
        const size_t n = l.size(); // the last byte of the line is dropped (GetData.cpp:48-53)
        r.seq = l.substr(0, n ? n - 1 : 0);
        std::string plus, q;
        line(plus); line(q);
        q.resize(n, '\0');
        r.qual = q.substr(0, n ? n - 1 : 0);
    } else {
        for (;;) {
            if (!line(l)) break;
            if (l[0] == '>') { pending_ = l; have_pending_ = true; break; }
            if (!l.empty()) l.resize(l.size() - 1);
            r.seq += l;
        }
    }
    return !r.seq.empty();
}

// ---------------------------------------------------------------------------------------------
// avgDist feedback
// ---------------------------------------------------------------------------------------------
inline void avg_replay(const PairOut *po, uint32_t n_pairs, const int64_t avg[4], std::vector<uint32_t> &redo,
                std::vector<int32_t> &redo_est, int64_t avg_out[4])
{
    redo.clear(); redo_est.clear();
    const uint32_t chunk = kReadChunkSize / 2;
    int64_t tp = avg[1], td = avg[2];
    uint32_t cur = (uint32_t)avg[0];
    for (uint32_t p0 = 0; p0 < n_pairs; p0 += chunk) {
        const int32_t e = (int32_t)(cur * 1.5);
        const uint32_t p1 = n_pairs < p0 + chunk ? n_pairs : p0 + chunk;
        for (uint32_t p = p0; p < p1; p++) {
            const PairOut &o = po[p];
            const bool ok = (o.flags & kRescueUsedEst) ? o.est == e : (e >= o.est_lo && e <= o.est_hi);
            if (!ok) { redo.push_back(p); redo_est.push_back(e); }
            if (o.pair_ok) { tp++; td += o.pair_dist; }
        }
        if (tp > 1000) cur = (uint32_t)(int)(1. * td / tp + .5);
    }
    avg_out[0] = cur; avg_out[1] = tp; avg_out[2] = td; avg_out[3] = avg[3];
}

// ---------------------------------------------------------------------------------------------
// SAM text
// ---------------------------------------------------------------------------------------------
static inline char comp_char(char c) // GetComplementaryBase, tools.cpp:3-18
{
    switch (c) {
    case 'A': case 'a': return 'T';
    case 'C': case 'c': return 'G';
    case 'G': case 'g': return 'C';
    case 'T': case 't': return 'A';
    default: return 'N';
    }
}

static void revcomp(const std::string &in, std::string &out)
{
    out.resize(in.size());
    for (size_t i = 0, n = in.size(); i < n; i++) out[i] = comp_char(in[n - 1 - i]);
}


inline void sam_line(const HostIndex &ix, const HostRead &rd, bool mate2_flipped, bool fastq, const AlnRec &rec,
              const uint32_t *cigar, std::string &out)
{
    // The reference reverse-complements mate 2 in place before mapping (ReadMapping.cpp:451) and
    // prints that string for forward-strand hits, its reverse complement otherwise.
    std::string cur_seq, cur_qual, tmp;
    if (mate2_flipped) { revcomp(rd.seq, cur_seq); cur_qual.assign(rd.qual.rbegin(), rd.qual.rend()); }
    else { cur_seq = rd.seq; cur_qual = rd.qual; }
    char num[128];
    out = rd.name;
    const bool mapped = rec.chr >= 0;
    if (!mapped) {
        snprintf(num, sizeof num, "\t%d\t*\t0\t0\t*\t*\t0\t0\t", rec.flag);
        out += num; out += cur_seq; out += '\t'; out += fastq ? cur_qual : std::string("*");
        out += "\tAS:i:0\tXS:i:0";
        return;
    }
    snprintf(num, sizeof num, "\t%d\t", rec.flag); out += num;
    out += ix.chr_name[rec.chr];
    snprintf(num, sizeof num, "\t%lld\t%d\t", (long long)rec.pos, rec.mapq); out += num;
    static const char opc[8] = {'M', 'I', 'D', 'N', 'S', 'H', 'P', '='};
    for (int i = 0; i < rec.n_cigar; i++) { snprintf(num, sizeof num, "%u%c", cigar[i] >> 4, opc[cigar[i] & 7]); out += num; }
    if (rec.has_mate) { snprintf(num, sizeof num, "\t=\t%lld\t%d\t", (long long)rec.mate_pos, rec.tlen); out += num; }
    else out += "\t*\t0\t0\t";
    if (rec.fwd) { out += cur_seq; out += '\t'; out += fastq ? cur_qual : std::string("*"); }
    else {
        revcomp(cur_seq, tmp); out += tmp; out += '\t';
        if (fastq) { tmp.assign(cur_qual.rbegin(), cur_qual.rend()); out += tmp; } else out += '*';
    }
    snprintf(num, sizeof num, "\tNM:i:%d\tAS:i:%d\tXS:i:%d", rec.nm, rec.as, rec.xs); out += num;
}


} // namespace mcx
#endif
