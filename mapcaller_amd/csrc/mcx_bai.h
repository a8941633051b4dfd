// mapcaller_amd/csrc/mcx_bai.h — the .bai of a coordinate-sorted BAM file (-index), the host's half: plain C++, no HIP (tests/hostemu/bai_check.cpp compiles it
// with g++).  The device (mcx_bai.hip) reads every record once and leaves two things: a list of stretches — maximal runs of records with one (refID, bin), each
// with the virtual offset of its first record and its counts — and a table of the 16 kb windows' smallest offsets.  Everything an index holds follows from those
// two by the rules of htslib's hts_idx_push / hts_idx_finish (format BAI: min_shift 14, 5 levels, 37449 bins, the pseudo-bin 37450):
//   chunks    a stretch is the chunk [its u, the next stretch's u) of its bin, the last one's end is the EOF block's offset << 16
//   meta      per contig with records, bin 37450: (u of its first stretch, u of the first stretch behind it or the EOF offset), (mapped, unmapped)
//   linear    n_intv = the highest touched window + 1; untouched entries take the entry before them, leading ones the contig's first offset
//   finish    from level 5 up to 1, a bin whose chunks span less than 0x10000 bytes of the file ((last.v >> 16) - (first.u >> 16)) moves into its parent where
//             that exists; every list is in offset order; neighbours with prev.v >> 16 >= next.u >> 16 are joined
// htslib writes a contig's bins in the order of its hash table; here they go ascending by number, so the file is a function of the BAM file alone.
// Host memory: 24 bytes a stretch (Index::runs), not a byte per record.
#ifndef MCX_BAI_H
#define MCX_BAI_H
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

namespace mcx {
namespace bai {

enum { kMinShift = 14, kLevels = 5, kBins = 37449, kMetaBin = 37450, kNoCoorBin = 4680 }; // (4680: what reg2bin makes of a record without a contig, [-1, 0))
const uint64_t kUntouched = ~0ull;   // a window no record has touched
const uint64_t kMarkerDist = 0x10000; // a bin below this span of file offsets is not worth a seek of its own

// the smallest bin that holds [beg, end), end > beg (the SAM specification's reg2bin)
static inline uint32_t reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}
static inline uint32_t bin_first(uint32_t level) { return ((1u << (3 * level)) - 1) / 7; }
static inline uint32_t bin_parent(uint32_t bin) { return (bin - 1) >> 3; }

// a stretch as the device writes it (mcx_bai_run of include/mcx.h)
struct Run { int32_t ref_id; uint32_t bin; uint64_t u; uint32_t n_mapped, n_unmapped; };
typedef std::pair<uint64_t, uint64_t> Chunk; // [u, v)

struct Stats { uint64_t stretches = 0, bins = 0, intervals = 0, bytes = 0; };

struct Index {
    std::vector<Run> runs; // the stretches of all calls so far, in file order; a call's first joined to the one before it when (refID, bin) agree

    // the run list of the next call.  false — and nothing taken — when it does not continue the file's order: a contig below the last one, or one behind records
    // without a contig
    bool push(const Run *r, uint64_t n)
    {
        if (n == 0) return true;
        int32_t last = runs.empty() ? 0 : runs.back().ref_id;
        for (uint64_t k = 0; k < n; k++) {
            const int32_t t = r[k].ref_id < 0 ? -1 : r[k].ref_id;
            const bool first = runs.empty() && k == 0;
            if (!first && (last < 0 ? t >= 0 : (t >= 0 && t < last))) return false;
            last = t;
        }
        uint64_t k = 0;
        if (!runs.empty() && same(runs.back(), r[0])) { runs.back().n_mapped += r[0].n_mapped; runs.back().n_unmapped += r[0].n_unmapped; k = 1; }
        for (; k < n; k++) { runs.push_back(r[k]); if (runs.back().ref_id < 0) { runs.back().ref_id = -1; runs.back().bin = kNoCoorBin; } }
        return true;
    }
    static bool same(const Run &a, const Run &b) { return (a.ref_id < 0 && b.ref_id < 0) || (a.ref_id == b.ref_id && a.bin == b.bin); }

    // The file's bytes.  final_offset: the EOF block's place << 16.  lin / lin_base: the windows' table over all contigs, contig t's entries at
    // lin[lin_base[t] .. lin_base[t + 1]), kUntouched where no mapped record lies.  false: a stretch names a contig or a bin that does not exist.
    bool finish(uint32_t n_ref, uint64_t final_offset, const uint64_t *lin, const uint64_t *lin_base, std::vector<uint8_t> *out, Stats *stats) const
    {
        out->clear();
        put(out, "BAI\1", 4);
        put32(out, n_ref);
        Stats st;
        st.stretches = runs.size();
        uint64_t n_no_coor = 0;
        size_t k = 0;
        for (uint32_t t = 0; t < n_ref; t++) {
            size_t e = k;
            while (e < runs.size() && runs[e].ref_id == (int32_t)t) e++;
            std::map<uint32_t, std::vector<Chunk>> bins;
            uint64_t off_beg = 0;
            if (e > k) {
                uint64_t n_mapped = 0, n_unmapped = 0;
                for (size_t j = k; j < e; j++) {
                    if (runs[j].bin >= (uint32_t)kBins) return false;
                    bins[runs[j].bin].push_back(Chunk(runs[j].u, j + 1 < runs.size() ? runs[j + 1].u : final_offset));
                    n_mapped += runs[j].n_mapped; n_unmapped += runs[j].n_unmapped;
                }
                off_beg = runs[k].u;
                compress(bins);
                std::vector<Chunk> &meta = bins[kMetaBin];
                meta.push_back(Chunk(off_beg, e < runs.size() ? runs[e].u : final_offset));
                meta.push_back(Chunk(n_mapped, n_unmapped));
            }
            put32(out, (uint32_t)bins.size());
            for (const auto &b : bins) {
                put32(out, b.first);
                put32(out, (uint32_t)b.second.size());
                for (const Chunk &c : b.second) { put64(out, c.first); put64(out, c.second); }
            }
            st.bins += bins.size();
            // the linear index: up to the highest touched window, filled forward
            const uint64_t *w = lin + lin_base[t];
            uint64_t n_intv = lin_base[t + 1] - lin_base[t];
            while (n_intv > 0 && w[n_intv - 1] == kUntouched) n_intv--;
            put32(out, (uint32_t)n_intv);
            uint64_t prev = off_beg;
            for (uint64_t i = 0; i < n_intv; i++) { if (w[i] != kUntouched) prev = w[i]; put64(out, prev); }
            st.intervals += n_intv;
            k = e;
        }
        for (; k < runs.size(); k++) {
            if (runs[k].ref_id >= 0) return false; // (a contig the header does not have)
            n_no_coor += (uint64_t)runs[k].n_mapped + runs[k].n_unmapped;
        }
        put64(out, n_no_coor);
        st.bytes = out->size();
        if (stats) *stats = st;
        return true;
    }

    // compress_binning: the small bins into their parents, level by level, then the neighbours joined
    static void compress(std::map<uint32_t, std::vector<Chunk>> &bins)
    {
        for (uint32_t l = kLevels; l > 0; l--) {
            const uint32_t lo = bin_first(l), hi = bin_first(l + 1);
            for (auto it = bins.lower_bound(lo); it != bins.end() && it->first < hi;) {
                std::vector<Chunk> &p = it->second;
                std::sort(p.begin(), p.end()); // (a list that received children is no longer in offset order)
                auto parent = bins.find(bin_parent(it->first));
                if ((p.back().second >> 16) - (p.front().first >> 16) < kMarkerDist && parent != bins.end()) {
                    parent->second.insert(parent->second.end(), p.begin(), p.end());
                    it = bins.erase(it);
                } else ++it;
            }
        }
        for (auto &b : bins) {
            std::vector<Chunk> &p = b.second;
            std::sort(p.begin(), p.end());
            size_t m = 0;
            for (size_t l = 1; l < p.size(); l++) {
                if (p[m].second >> 16 >= p[l].first >> 16) { if (p[m].second < p[l].second) p[m].second = p[l].second; }
                else p[++m] = p[l];
            }
            p.resize(m + 1);
        }
    }

    static void put(std::vector<uint8_t> *o, const void *p, size_t n) { o->insert(o->end(), (const uint8_t *)p, (const uint8_t *)p + n); }
    static void put32(std::vector<uint8_t> *o, uint32_t v) { uint8_t b[4]; for (int k = 0; k < 4; k++) b[k] = (uint8_t)(v >> (8 * k)); put(o, b, 4); }
    static void put64(std::vector<uint8_t> *o, uint64_t v) { uint8_t b[8]; for (int k = 0; k < 8; k++) b[k] = (uint8_t)(v >> (8 * k)); put(o, b, 8); }
};

// the table's layout: contig t has ceil(len / 16384) windows and one more, so that a record that ends on the contig's last base — or, soft-clipped, a little
// behind it — still has its window
static inline uint64_t windows_of(int64_t contig_len) { return (uint64_t)((contig_len > 0 ? contig_len : 0) >> kMinShift) + 2; }

} // namespace bai
} // namespace mcx
#endif
