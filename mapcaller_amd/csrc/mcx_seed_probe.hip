// mapcaller_amd/csrc/mcx_seed_probe.hip — mcx_seed_walk_batch: the seeding walk of mcx_fm.h by itself, on reads the caller hands
// over, so that a test can hold it against a plain suffix array seed by seed.
//
// The kernel is k_seed's phase loop (mcx_pipeline.hip) without its queue: one read per lane, packed with pack_read into a stretch
// of global scratch of the lane's own (k_seed keeps the words in LDS), then seed_next_start / seed_begin / seed_fm with the
// caller's budget of FM steps per turn / seed_compare_wide / seed_take until the read has no further search.  Whatever the index
// holds is used as k_seed uses it: jump table, rank records, pair records, the full suffix array.  Without the full suffix array
// the rows seed_take leaves are resolved here with fm_sa, as k_sa does.  No arithmetic is restated here.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mcx.h"
#include "mcx_fm.h"
#include "mcx_internal.h"

using namespace mcx;

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

static_assert(sizeof(mcx_seed_hit) == sizeof(Hit), "mcx_seed_hit is mcx_types.h's Hit");

namespace {

__global__ void __launch_bounds__(64) k_seed_probe(IndexView ix, const uint8_t *seqs, const uint32_t *off, uint32_t n, int fm_budget, uint32_t cap,
                                                   uint32_t *scratch, uint32_t words_per_read, int32_t *n_hits, Hit *hits)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ReadRef rd; rd.ascii = seqs + off[i]; rd.rlen = (int)(off[i + 1] - off[i]); rd.flipped = 0;
    const int rlen = rd.rlen;
    PackedRead pk; pk.w = scratch + (uint64_t)i * words_per_read; pk.stride = 1; pk.n_code = 0; // (packed_words(rlen) <= words_per_read: the host sized it)
    pack_read(rd, pk);
    Hit *mine = hits + (uint64_t)i * cap;
    int nh = 0, p = 0;
    int64_t ext = 0, blocks = 0;
    uint32_t nm = 0;
    SeedWalk walk; walk.phase = 0;
    bool have = seed_next_start(pk, rlen, p, nm);
    while (have) {
        if (walk.phase == 0) seed_begin(ix, pk, rlen, nm, p, walk);
        if (walk.phase == 1) seed_fm(ix, pk, rlen, p, walk, blocks, fm_budget);
        if (walk.phase == 2) seed_compare_wide(ix, pk, rlen, p, walk, 1 << 30);
        if (walk.phase == 3) {
            seed_take(ix, p, walk, mine, (int)cap, nh, ext);
            have = seed_next_start(pk, rlen, p, nm);
        }
    }
    if (!ix.sa_full) { // the hits that are still rows (k_sa); the others carry their text position under the flag
        const int keep = nh < (int)cap ? nh : (int)cap;
        for (int k = 0; k < keep; k++) {
            if (mine[k].len & kHitResolved) { mine[k].len &= ~kHitResolved; continue; }
            int lf = 0;
            mine[k].gPos = (int64_t)fm_sa(ix, (uint64_t)mine[k].gPos, lf);
        }
    }
    n_hits[i] = nh;
}

struct DevBufs { // everything the call holds in HBM, released when it returns (whichever way)
    std::vector<void *> all;
    ~DevBufs() { for (void *p : all) (void)hipFree(p); }
    template <class T> bool take(T **p, size_t count)
    {
        void *v = nullptr;
        if (hipMalloc(&v, std::max<size_t>(count * sizeof(T), 16)) != hipSuccess) { (void)hipGetLastError(); return false; }
        all.push_back(v);
        *p = (T *)v;
        return true;
    }
};

} // namespace

extern "C" int mcx_seed_walk_batch(mcx_ctx *c, const uint8_t *seqs, const uint32_t *seq_off, uint32_t n, int fm_budget, uint32_t cap, int32_t *n_hits,
                                   mcx_seed_hit *hits)
{
    if (!c || !seqs || !seq_off || !n_hits || (cap && !hits)) return mcx_set_error(MCX_ERR_ARG, "mcx_seed_walk_batch: null argument");
    if (fm_budget < 1) return mcx_set_error(MCX_ERR_ARG, "mcx_seed_walk_batch: fm_budget must be at least 1");
    if (cap > (1u << 20)) return mcx_set_error(MCX_ERR_ARG, "mcx_seed_walk_batch: cap above 2^20");
    if (n == 0) return 0;
    uint32_t longest = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (seq_off[i + 1] < seq_off[i]) return mcx_set_error(MCX_ERR_ARG, "mcx_seed_walk_batch: offsets do not ascend");
        longest = std::max(longest, seq_off[i + 1] - seq_off[i]);
    }
    if (longest > (1u << 20)) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_seed_walk_batch: a read longer than 2^20 bases");
    const uint32_t words = (uint32_t)packed_words((int)longest);
    const size_t nb = seq_off[n];
    HIP_TRY(hipSetDevice(mcx_ctx_index(c)->device));
    hipStream_t s = (hipStream_t)mcx_ctx_stream(c);
    DevBufs d;
    uint8_t *d_seq = nullptr; uint32_t *d_off = nullptr, *d_scratch = nullptr; int32_t *d_n = nullptr; Hit *d_hits = nullptr;
    if (!d.take(&d_seq, nb + 32) /* (the packer fetches whole aligned 16-byte chunks) */ || !d.take(&d_off, (size_t)n + 1) || !d.take(&d_scratch, (size_t)n * words) ||
        !d.take(&d_n, n) || !d.take(&d_hits, (size_t)n * cap))
        return mcx_set_error(MCX_ERR_DEVICE, "mcx_seed_walk_batch: out of device memory");
    HIP_TRY(hipMemsetAsync(d_seq, 'N', nb + 32, s));
    HIP_TRY(hipMemcpyAsync(d_seq, seqs, nb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_off, seq_off, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_n, 0, (size_t)n * 4, s));
    HIP_TRY(hipMemsetAsync(d_hits, 0, std::max<size_t>((size_t)n * cap * sizeof(Hit), 16), s));
    k_seed_probe<<<(n + 63) / 64, 64, 0, s>>>(mcx_ctx_index(c)->view, d_seq, d_off, n, fm_budget, cap, d_scratch, words, d_n, d_hits);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(n_hits, d_n, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (cap) HIP_TRY(hipMemcpyAsync(hits, d_hits, (size_t)n * cap * sizeof(Hit), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}
