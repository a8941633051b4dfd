// mapcaller_amd/csrc/mcx_sort_plan.h — the plan of -sort's external merge (mcx_files.cpp); host only, no HIP in it (tests/hostemu/sort_check.cpp holds it
// against brute force).
//
// What there is: sorted runs.  Of each the host keeps the records' keys (ascending, ties in input order) and lengths, and the table of the BGZF blocks its
// records were written in: where a block lies in the temporary file, its size, and which bytes of the run's uncompressed stream it holds.
// What the plan makes of them: chunks, by key.  Splitter keys are chosen from every S-th key of every run, weighted with the bytes between the samples, so
// that a chunk comes to about `chunk_bytes` of records; chunk k holds the records with splitter[k-1] <= key < splitter[k], found by lower_bound in each run.
// Equal keys therefore never straddle chunks (a pile-up on one key makes a large chunk, never a split one), a chunk's records in a run are one contiguous
// slice, and the chunks sorted one by one — the slices taken in run order, stably — are the global stable sort.  Nothing of the result depends on
// chunk_bytes or S; they decide only how much is in HBM at a time.
#ifndef MCX_SORT_PLAN_H
#define MCX_SORT_PLAN_H
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace mcx {
namespace sortplan {

struct Block { uint64_t c_off; uint32_t c_size; uint32_t u_size; uint64_t u_off; }; // a BGZF block: place and size in the file; bytes of the run's stream [u_off, u_off + u_size)

struct Run {
    std::vector<uint64_t> keys;  // ascending
    std::vector<uint32_t> lens;  // 4 + block_size of each record
    std::vector<Block> blocks;   // in stream order, u_off contiguous from 0
    uint64_t bytes = 0;          // of records
    // the stream offset of every kStep-th record (byte_at sums at most kStep lengths on top)
    enum { kStep = 1024 };
    std::vector<uint64_t> cum;
    void finish()
    {
        cum.clear();
        uint64_t at = 0;
        for (size_t i = 0; i < lens.size(); i++) { if (i % kStep == 0) cum.push_back(at); at += lens[i]; }
        bytes = at;
    }
    uint64_t byte_at(uint64_t i) const // where record i starts in the run's stream (i == n: its end)
    {
        if (i >= lens.size()) return bytes;
        uint64_t at = cum[(size_t)(i / kStep)];
        for (uint64_t k = i / kStep * kStep; k < i; k++) at += lens[(size_t)k];
        return at;
    }
};

struct Slice {
    uint32_t run;
    uint64_t r0, r1;   // records [r0, r1) of the run
    uint64_t b0, b1;   // bytes [b0, b1) of the run's stream
    uint64_t k0, k1;   // blocks [k0, k1) of the run cover them: k0 the block that holds byte b0, k1 - 1 the one that holds byte b1 - 1
};
struct Chunk { std::vector<Slice> slices; uint64_t records = 0, bytes = 0; }; // the slices in run order; none is empty

struct Plan {
    std::vector<uint64_t> splitters; // strictly ascending; chunks.size() == splitters.size() + 1
    std::vector<Chunk> chunks;
    uint64_t sample_step = 0;
};

// every S-th key: S from the records a chunk takes and the number of runs — a splitter is off by at most S records a run
static inline uint64_t sample_step(const std::vector<Run> &runs, uint64_t chunk_bytes)
{
    uint64_t n = 0, bytes = 0, live = 0;
    for (const Run &r : runs) { n += r.keys.size(); bytes += r.bytes; live += r.keys.empty() ? 0 : 1; }
    if (n == 0) return 1;
    const uint64_t avg = std::max<uint64_t>(1, bytes / n), per_chunk = std::max<uint64_t>(1, chunk_bytes / avg);
    return std::min<uint64_t>(4096, std::max<uint64_t>(1, per_chunk / (2 * std::max<uint64_t>(1, live))));
}

static inline void make_plan(const std::vector<Run> &runs, uint64_t chunk_bytes, Plan *plan)
{
    plan->splitters.clear(); plan->chunks.clear();
    const uint64_t S = sample_step(runs, chunk_bytes);
    plan->sample_step = S;
    // the samples: a key, and the bytes of the records from it to the next sample of its run
    std::vector<std::pair<uint64_t, uint64_t>> samples;
    for (const Run &r : runs)
        for (uint64_t i = 0; i < r.keys.size(); i += S) samples.push_back(std::make_pair(r.keys[(size_t)i], r.byte_at(std::min<uint64_t>(i + S, r.keys.size())) - r.byte_at(i)));
    std::sort(samples.begin(), samples.end());
    uint64_t acc = 0, prev = 0;
    for (size_t k = 0; k < samples.size(); k++) {
        if (k && acc >= chunk_bytes && samples[k].first > prev) { plan->splitters.push_back(samples[k].first); acc = 0; }
        acc += samples[k].second;
        prev = samples[k].first;
    }
    const size_t n_chunks = plan->splitters.size() + 1;
    plan->chunks.resize(n_chunks);
    for (size_t ri = 0; ri < runs.size(); ri++) {
        const Run &r = runs[ri];
        uint64_t lo = 0;
        for (size_t k = 0; k < n_chunks; k++) {
            const uint64_t hi = k + 1 < n_chunks ? (uint64_t)(std::lower_bound(r.keys.begin() + (std::ptrdiff_t)lo, r.keys.end(), plan->splitters[k]) - r.keys.begin()) : (uint64_t)r.keys.size();
            if (hi > lo) {
                Slice s;
                s.run = (uint32_t)ri; s.r0 = lo; s.r1 = hi; s.b0 = r.byte_at(lo); s.b1 = r.byte_at(hi);
                // the block that holds byte b: the last one whose u_off is <= b (blocks of no bytes hold none and are passed over)
                auto holds = [&r](uint64_t b) {
                    size_t a = 0, z = r.blocks.size();
                    while (z - a > 1) { const size_t m = (a + z) / 2; if (r.blocks[m].u_off <= b) a = m; else z = m; }
                    return (uint64_t)a;
                };
                s.k0 = holds(s.b0); s.k1 = holds(s.b1 - 1) + 1;
                Chunk &c = plan->chunks[k];
                c.slices.push_back(s); c.records += hi - lo; c.bytes += s.b1 - s.b0;
            }
            lo = hi;
        }
    }
}

} // namespace sortplan
} // namespace mcx
#endif
