// mapcaller_amd/csrc/mcx_profile.hip — the -vcf bookkeeping of a finished batch (UpdateProfile / UpdateMultiHitCount): the
// kernels over the per-read detail records that k_simple and k_finish wrote (mcx_profile.h holds their device functions and
// types), the duplicate check's key sort, the tally and event archives, and the mcx_profile_* / mcx_ctx_create_fit ABI.
// Reached through that ABI and through profile_keys / _queue / _collect / _foreign / _accumulate, archive_append and
// sort_reserve (mcx_ctx.h), which the batch ABI of mcx_pipeline.hip calls.
#include "mcx_ctx.h"
#include <hipcub/hipcub.hpp>

namespace mcx {

// pass 1: break points, clip gate, and the (start position, read) key of every read that reaches
// the duplicate check (AlignmentProfile.cpp:53-77); n_valid counts them (the others get ~0 and sort last)
__global__ void k_prof_keys(const uint8_t *detail, DetailLayout dl, ReadBatch rb, IndexView ix, ProfView pv, SparseSink sink,
                            uint64_t *keys, uint32_t *n_valid)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t key = ~0ull;
    if (r < rb.n_reads) {
        const uint8_t *rec = detail + (uint64_t)r * dl.stride;
        const DetailHdr &d = *(const DetailHdr *)rec;
        if (d.type == 1) {
            const Frag *f = (const Frag *)(rec + sizeof(DetailHdr)) + d.frag0;
            const Frag &a = f[0], &b = f[d.n_frags - 1];
            const int rlen = (int)(rb.off[r + 1] - rb.off[r]);
            bool go = true;
            if (a.rLen == 0 && a.gLen == 0) {
                if (a.rPos > 20) { SparseRec s; s.pos = a.gPos < ix.G ? a.gPos : ix.G2 - 1 - a.gPos; s.type = 'B'; s.len = 0; sparse_put(sink, s); }
                if (a.rPos > pv.max_clip) go = false;
            }
            if (go && b.rLen == 0 && b.gLen == 0) {
                if (rlen - b.rPos > 20) { SparseRec s; s.pos = b.gPos < ix.G ? b.gPos : ix.G2 - 1 - b.gPos; s.type = 'B'; s.len = 0; sparse_put(sink, s); }
                if (rlen - b.rPos > pv.max_clip) go = false;
            }
            if (go) {
                const int64_t g = d.fwd ? a.gPos : ix.G2 - (a.gPos + a.gLen);
                key = ((uint64_t)g << 32) | r;
            }
        }
        keys[r] = key;
    }
    const uint64_t m = __ballot(key != ~0ull);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_valid, (uint32_t)__popcll(m));
}

// pass 2 (keys sorted by (start position, read number in input order), the reads of every shard of the
// round among them): a read is admitted when fewer than max_dup reads were admitted at its start position
// before it — earlier rounds (readCount plane) plus earlier reads of this round.  Only the reads
// [own_lo, own_lo + n_own) are this shard's: their flags are written.
// (n_dev: the number of keys where the host has not looked at it — a batch's bookkeeping queued behind its mapping; the grid then covers the batch's reads)
__global__ void k_prof_admit(const uint64_t *keys, uint64_t n, ProfView pv, uint8_t *admit, uint32_t own_lo, uint32_t n_own, const uint32_t *n_dev = nullptr)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n_dev) n = *n_dev;
    if (j >= n) return;
    const uint64_t key = keys[j];
    const uint32_t idx = (uint32_t)key - own_lo;
    if (idx >= n_own) return;
    const uint64_t g = key >> 32;
    int rank = 0;
    for (int k = 1; k <= pv.max_dup && (uint64_t)k <= j; k++) { if ((keys[j - k] >> 32) == g) rank++; else break; }
    const uint32_t before = pv.pl.h(kPlReadCount)[g];
    admit[idx] = (uint8_t)((admit[idx] & 2) | ((before + (uint32_t)rank < (uint32_t)pv.max_dup) ? 1 : 0)); // (bit 1: k_pack_reads')
}

// pass 2b (after every flag is out): the first key of each start position adds the round's admissions to
// readCount — the count of the whole run, the same on every shard (`readCount < iMaxDuplicate` then ++, :76-77)
__global__ void k_prof_count(const uint64_t *keys, uint64_t n, ProfView pv, const uint32_t *n_dev = nullptr)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n_dev) n = *n_dev;
    if (j >= n) return;
    const uint64_t g = keys[j] >> 32;
    if (j > 0 && (keys[j - 1] >> 32) == g) return;
    uint32_t run = 1;
    while (run < (uint32_t)pv.max_dup && j + run < n && (keys[j + run] >> 32) == g) run++;
    uint16_t *cnt = &pv.pl.h(kPlReadCount)[g]; // (a 16-bit store: the neighbouring position's half of the word is another thread's)
    const uint32_t v = (uint32_t)*cnt + run;
    *cnt = (uint16_t)(v < (uint32_t)pv.max_dup ? v : (uint32_t)pv.max_dup);
}

// (the reads in the order of their sorted start keys instead — the lanes of a wavefront then add to neighbouring stretches of the planes —
//  was measured in round 5: 30.38 against 30.46 ms per batch; the kernel is bound by the lines its atomics open, ~24 G line fills and
//  write-backs a second, wherever they lie)
__global__ void __launch_bounds__(256) k_prof_accum(const uint8_t *detail, DetailLayout dl, ReadBatch rb, IndexView ix, ProfView pv,
                                                    SparseSink sink, const uint8_t *admit, int paired, ColList cols)
{
    __shared__ SparseRec s_buf[4][96];
    __shared__ uint32_t s_cnt[4];
    WaveSparse ws; ws.buf = s_buf[threadIdx.x >> 6]; ws.cnt = &s_cnt[threadIdx.x >> 6]; ws.cap = 96;
    if ((threadIdx.x & 63) == 0) *ws.cnt = 0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    prof_read(detail, dl, rb, ix, pv, sink, ws, admit, paired, cols, r);
    wave_sparse_flush(ws, sink);
}

// pass 3b: the listed fragments, one per group of sixteen lanes
__global__ void __launch_bounds__(256) k_prof_cols(const uint8_t *detail, DetailLayout dl, ReadBatch rb, IndexView ix, ProfView pv,
                                                   SparseSink sink, ColList cols)
{
    __shared__ SparseRec s_buf[4][64];
    __shared__ uint32_t s_cnt[4];
    WaveSparse ws; ws.buf = s_buf[threadIdx.x >> 6]; ws.cnt = &s_cnt[threadIdx.x >> 6]; ws.cap = 64;
    if ((threadIdx.x & 63) == 0) *ws.cnt = 0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
    const uint32_t n = *cols.n < cols.cap ? *cols.n : cols.cap;
    const uint32_t group = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, n_groups = (gridDim.x * blockDim.x) >> 4;
    const int me = threadIdx.x & 15, grp_shift = threadIdx.x & 48;
    const uint32_t first = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 4; // (the wavefront's first group: its lanes leave the loop together)
    for (uint32_t k0 = first; k0 < n; k0 += n_groups) {
        const uint32_t k = k0 + (group - first);
        if (k < n) {
            const ColItem it = cols.items[k];
            ReadRef rd;
            rd.ascii = rb.bases + it.off; rd.rlen = it.rlen; rd.flipped = (it.flags & 2) ? 1 : 0;
            prof_walk<16>(rd, it.f, (it.flags & 1) != 0, detail + (uint64_t)it.read * dl.stride + dl.off_ops, ix, pv, sink, ws, me, grp_shift);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
        if (*ws.cnt >= ws.cap / 2) wave_sparse_flush(ws, sink);
    }
    wave_sparse_flush(ws, sink);
}

// mcx_profile_settle, before the scans: the words of a 16-bit difference plane back to two differences modulo 2^16 (mcx_planes.h)
__global__ void __launch_bounds__(256) k_prof_decode(uint32_t *words, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t w = words[i];
        if (w) words[i] = planes_decode(w);
    }
}

// mcx_profile_settle, after the scans: the exact-seed coverage joins the plane of the reference's base
__global__ void __launch_bounds__(256) k_prof_fold(IndexView ix, ProfView pv)
{
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pv.G; p += (int64_t)gridDim.x * blockDim.x) {
        const uint16_t m = pv.match[p];
        if (m) pv.pl.h(ref_code(ix, p))[p] += m; // (a 16-bit read-modify-write of the thread's own position)
    }
}

// field widths of MappingRecord_t, applied once all contributions are in (and, on several GPUs,
// after the all-reduce): 12-bit saturation, 16-bit wrap, duplicate cap
__global__ void k_prof_finalize(PlanesView pl, int max_dup)
{
    const int k = blockIdx.y; // one plane per grid row: no division per element (the strand planes are 16-bit words already: nothing to do)
    if (k == kPlMulti) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pl.G; i += (int64_t)gridDim.x * blockDim.x) { const uint32_t v = pl.multi[i]; if (v > 4095u) pl.multi[i] = 4095u; }
        return;
    }
    if (k > kPlReadCount) return;
    const uint16_t top = (uint16_t)(k == kPlReadCount ? max_dup : 4095);
    // two positions per thread: a word of the plane at a time
    uint32_t *w = (uint32_t *)pl.h(k);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pl.stride / 2; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t v = w[i];
        const uint32_t lo = v & 0xFFFFu, hi = v >> 16;
        if (lo > top || hi > top) w[i] = (lo < top ? lo : top) | ((hi < top ? hi : top) << 16);
    }
}

} // namespace mcx

__global__ void k_zero_but(uint32_t *cnt, int n, int keep_a, int keep_b)
{
    for (int k = threadIdx.x; k < n; k += blockDim.x) if (k != keep_a && k != keep_b) cnt[k] = 0;
}

// ---------------------------------------------------------------------------------------------
// -vcf bookkeeping: UpdateProfile / UpdateMultiHitCount for a finished batch (mcx_profile.h)
// ---------------------------------------------------------------------------------------------
// discordant-pair events, ReadMapping.cpp:486-521: kept as seen ('E' records: pos = the pair's number in the input stream,
// len = kind, seq = g1, g2, dist) — the reference's second branch pushes its DiscordPair variable whatever the previous
// discordant pair left in it, so they are resolved in input order once the run is over
// (mcx_disc_resolve: mcx_profile_sparse for one shard, mcx_call_variants for several)
__global__ void k_prof_disc(const uint8_t *detail, DetailLayout dl, uint32_t n_pairs, int64_t first_pair, SparseRec *out, uint32_t *n, uint32_t cap)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const DetailHdr &d = *(const DetailHdr *)(detail + (uint64_t)(2 * p) * dl.stride);
    if (d.disc_kind == 0) return;
    const uint32_t at = atomicAdd(n, 1u);
    if (at >= cap) return;
    SparseRec e;
    uint64_t *w = (uint64_t *)&e;
    for (int k = 0; k < (int)(sizeof(SparseRec) / 8); k++) w[k] = 0;
    e.pos = first_pair + p; e.type = 'E'; e.len = (uint8_t)d.disc_kind;
    const int64_t v[3] = {d.disc_g1, d.disc_g2, d.disc_dist};
    memcpy(e.seq, v, sizeof v);
    out[at] = e;
}

extern "C" int mcx_profile_attach(mcx_ctx *c, uint32_t *d_planes, int max_dup, int max_clip)
{
    static_assert(sizeof(mcx_sparse_rec) == sizeof(SparseRec), "mcx_sparse_rec and SparseRec must have one layout");
    if (!c || !d_planes) return mcx_set_error(MCX_ERR_ARG, "mcx_profile_attach: null argument");
    if (c->idx->view.G >= (int64_t)1 << 32) return mcx_set_error(MCX_ERR_UNSUPPORTED, "the alignment profile takes genomes below 2^32 bases");
    HIP_TRY(hipSetDevice(c->idx->device));
    if (c->later.pending) { (void)hipStreamSynchronize(c->later.stream); c->later.pending = false; } // (a profile that is given up with a batch's bookkeeping on its way)
    c->prof_planes = d_planes;
    c->prof_max_dup = (max_dup <= 0 || max_dup > 15) ? 15 : max_dup; // main.cpp:240-244, :323
    c->prof_max_clip = max_clip;
    if (!c->d_detail) {
        c->dlay = make_detail_layout(c->rlen_max);
        int rc;
        if ((rc = dmalloc(&c->d_detail, (size_t)c->dlay.stride * c->max_reads))) return rc;
        if ((rc = dmalloc(&c->d_admit, c->max_reads + 4))) return rc;
        c->prof_items_cap = (uint32_t)std::min<uint64_t>((uint64_t)c->max_reads * 4 + 1024, 0x7fffffffu);
        if ((rc = dmalloc(&c->d_prof_items, c->prof_items_cap))) return rc;
        if ((rc = sort_reserve(c, c->max_reads))) return rc;
        c->sparse_cap = (uint32_t)std::min<uint64_t>(c->max_reads * 2 + 4096, 0x7fffffffu);
        if ((rc = dmalloc(&c->d_sparse, c->sparse_cap))) return rc;
        HIP_TRY(hipHostMalloc((void **)&c->h_sparse_pin, (size_t)c->sparse_pin_recs * sizeof(SparseRec)));
    }
    c->h_sparse.clear(); c->h_events.clear(); c->n_tally = 0; c->arch.n = c->arch_ev.n = 0;
    c->arch.host = &c->h_sparse; c->arch_ev.host = &c->h_events;
    if (!c->arch.d) { // room for the first batches' records now, not in the middle of the first batch
        const uint64_t first = std::min<uint64_t>(std::max<uint64_t>(c->sparse_cap, (uint64_t)1 << 20), (uint64_t)1 << 22);
        if (hipMalloc((void **)&c->arch.d, first * sizeof(SparseRec)) == hipSuccess) c->arch.cap = first; else { (void)hipGetLastError(); c->arch.d = nullptr; }
    }
    const size_t match_n = (size_t)planes_stride(c->idx->view.G);
    if (!c->d_prof_match) {
        int rc = dmalloc(&c->d_prof_match, match_n);
        if (rc && c->later.have) { // the device has filled up since the second set was taken: it goes back, the bookkeeping runs inside the batches' calls from here on
            auto &L = c->later;
            (void)hipGetLastError();
            (void)hipStreamSynchronize(L.stream); (void)hipStreamSynchronize(L.keep_stream);
            for (void **q : {(void **)&L.d_detail_alt, (void **)&L.d_admit_alt, (void **)&L.d_keep_bases, (void **)&L.d_keep_off, (void **)&L.d_keep_bases_alt, (void **)&L.d_keep_off_alt, (void **)&L.d_ev}) if (*q) { (void)hipFree(*q); *q = nullptr; }
            L.have = false;
            if (c->kn.timing) fprintf(stderr, "[mcx profile] the second set of detail records goes back: the device has no room for the coverage plane beside it\n");
            rc = dmalloc(&c->d_prof_match, match_n);
        }
        if (rc) return rc;
    }
    HIP_TRY(hipMemsetAsync(c->d_prof_match, 0, match_n * sizeof(uint16_t), c->t0.stream));
    if (!c->kn.no_prof_overlap && !c->later.have && !c->later.tried) { // a second set of what a batch's mapping writes for the bookkeeping, if HBM has the room (without it: the bookkeeping inside the call, as before)
        auto &L = c->later;
        L.tried = true;
        L.ev_cap = (uint32_t)std::min<uint64_t>(c->max_reads / 2 + 4096, 0x7fffffffu);
        // (a stream of the lowest priority: queues of a priority of their own in the runtime — a stream of the default priority may share a hardware queue with the
        //  context's main stream, and then the bookkeeping runs before the next batch's kernels, not under them — and the mapping goes first where both want the chip)
        int prio_low = 0, prio_high = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
        size_t hbm_free = 0, hbm_all = 0;
        (void)hipMemGetInfo(&hbm_free, &hbm_all);
        const size_t second_set = (size_t)c->dlay.stride * c->max_reads + 2 * (c->max_bases + 4 * c->max_reads) + (size_t)L.ev_cap * sizeof(SparseRec);
        // (what is left afterwards has to hold the record archive's growth and the caller's own buffers: four gigabytes at least)
        bool ok = hbm_free > second_set + ((size_t)4 << 30) && hipMalloc((void **)&L.d_detail_alt, (size_t)c->dlay.stride * c->max_reads) == hipSuccess && hipMalloc((void **)&L.d_admit_alt, c->max_reads + 4) == hipSuccess &&
                  hipMalloc((void **)&L.d_keep_bases, c->max_bases + 64) == hipSuccess && hipMalloc((void **)&L.d_keep_off, (c->max_reads + 1) * sizeof(uint32_t)) == hipSuccess &&
                  hipMalloc((void **)&L.d_keep_bases_alt, c->max_bases + 64) == hipSuccess && hipMalloc((void **)&L.d_keep_off_alt, (c->max_reads + 1) * sizeof(uint32_t)) == hipSuccess &&
                  hipMalloc((void **)&L.d_cnt, CNT_N * sizeof(uint32_t)) == hipSuccess && hipMalloc((void **)&L.d_ev, (size_t)L.ev_cap * sizeof(SparseRec)) == hipSuccess &&
                  hipHostMalloc((void **)&L.h_cnt, CNT_N * sizeof(uint32_t)) == hipSuccess &&
                  hipStreamCreateWithPriority(&L.stream, hipStreamNonBlocking, prio_low) == hipSuccess && hipStreamCreateWithPriority(&L.keep_stream, hipStreamNonBlocking, prio_low) == hipSuccess;
        for (hipEvent_t *e : {&L.go, &L.done, &L.kept, &L.begun}) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            for (void **q : {(void **)&L.d_detail_alt, (void **)&L.d_admit_alt, (void **)&L.d_keep_bases, (void **)&L.d_keep_off, (void **)&L.d_keep_bases_alt, (void **)&L.d_keep_off_alt, (void **)&L.d_cnt, (void **)&L.d_ev}) if (*q) { (void)hipFree(*q); *q = nullptr; }
            if (c->kn.timing) fprintf(stderr, "[mcx profile] no room in HBM for a second set of detail records: a batch's bookkeeping runs inside its call\n");
        }
        L.have = ok;
    }
    c->prof_settled = false; c->prof_broken = false;
    return 0;
}

// A context — and, for a -vcf run, the planes and the bookkeeping's buffers — sized to what the device has left (the -vcf leg at 3.1 Gbp left
// 5.4 GB of 309, and a larger genome met a bare hipMalloc failure in the middle of its first batch).  Everything the run will take is taken HERE: the context,
// tier 0's pair records (otherwise the first batch's), the planes, the detail records.  When that does not fit with kFitMargin to spare — the record
// archive's growth, the caller's own batches, the stream slots — the run is degraded in a fixed order, each step said on stderr in one line:
//   1. the index gives its pair records back (mcx_index_trim: the seeding walk takes one base per step, 24.8 GB at 3.1 Gbp);
//   2. max_batch_reads is halved, again and again (down to 128 K reads);
// (a second set of detail records, which lets a batch's bookkeeping run under the next batch, is only ever taken when there is room: mcx_profile_attach).
// MCX_HBM_CAP_GB=n (tests): the run may take n GB, whatever the device has free.
constexpr size_t kFitMargin = (size_t)4 << 30;
extern "C" int mcx_ctx_create_fit(mcx_index *ix, const mcx_opts *opts, int with_profile, int paired, int max_dup, int max_clip, mcx_ctx **out, uint32_t **planes, mcx_fit *fit)
{
    if (!ix || !out || (with_profile && !planes)) return mcx_set_error(MCX_ERR_ARG, "mcx_ctx_create_fit: null argument");
    mcx_opts o;
    if (opts) o = *opts; else mcx_opts_default(&o);
    mcx_fit f; memset(&f, 0, sizeof f);
    size_t cap = 0; // MCX_HBM_CAP_GB=n (tests): the run may take n GB of the device, whatever is free
    if (const char *e = getenv("MCX_HBM_CAP_GB")) cap = (size_t)(atof(e) * (double)((size_t)1 << 30));
    HIP_TRY(hipSetDevice(ix->device));
    for (;;) {
        mcx_ctx *c = nullptr;
        uint32_t *pl = nullptr;
        size_t free0 = 0, hbm_free = 0, hbm_all = 0;
        (void)hipMemGetInfo(&free0, &hbm_all);
        int rc = mcx_ctx_create(ix, &o, &c);
        if (rc == 0) rc = reserve_tier0(c, paired, (uint64_t)o.max_batch_reads);
        if (rc == 0 && with_profile) {
            rc = mcx_planes_alloc(ix, &pl);
            if (rc == 0) rc = mcx_profile_attach(c, pl, max_dup, max_clip);
        }
        (void)hipMemGetInfo(&hbm_free, &hbm_all);
        const size_t took = free0 > hbm_free ? free0 - hbm_free : 0;
        if (cap) hbm_free = std::min(hbm_free, cap > took ? cap - took : 0);
        const bool fits = rc == 0 && hbm_free >= kFitMargin;
        if (fits) {
            f.max_batch_reads = o.max_batch_reads; f.hbm_free_bytes = (int64_t)hbm_free; f.hbm_taken_bytes = (int64_t)took; f.single_detail_set = with_profile && !c->later.have;
            if (fit) *fit = f;
            *out = c;
            if (planes) *planes = pl;
            return 0;
        }
        const std::string why = rc ? std::string(mcx_last_error()) : std::to_string((double)hbm_free / 1e9).substr(0, 5) + " GB of HBM would be left";
        (void)hipGetLastError(); // (an allocation that failed is no error of the run)
        if (pl) mcx_planes_free(pl);
        if (c) mcx_ctx_free(c);
        if (rc && rc != MCX_ERR_DEVICE) return rc; // (not a matter of room)
        if (ix->d_rank2) {
            if ((rc = mcx_index_trim(ix, 1))) return rc;
            f.pair_records_trimmed = 1;
            fprintf(stderr, "[mcx fit] %s with batches of %lld reads: the index gives its pair records back (the seeding walk takes one base per step)\n", why.c_str(), (long long)o.max_batch_reads);
            continue;
        }
        if (o.max_batch_reads > ((int64_t)1 << 17)) {
            o.max_batch_reads = std::max<int64_t>((int64_t)1 << 17, (o.max_batch_reads / 2 + 199) / 200 * 200); // (whole 200-read chunks: a caller that cuts its run into batches of this size keeps the chunk boundaries)
            f.batch_halvings++;
            fprintf(stderr, "[mcx fit] %s: batches of %lld reads instead\n", why.c_str(), (long long)o.max_batch_reads);
            continue;
        }
        return mcx_set_error(MCX_ERR_DEVICE, "mcx_ctx_create_fit: the device has no room for this run even with batches of " + std::to_string((long long)o.max_batch_reads) + " reads and without the pair records (" + why + ")");
    }
}

// key buffers and radix-sort scratch for n keys (grown on demand: a round's keys of all shards can outnumber a batch)
int sort_reserve(mcx_ctx *c, uint64_t n)
{
    if (n <= c->keys_cap) return 0;
    for (int k = 0; k < 2; k++) { if (c->d_keys[k]) (void)hipFree(c->d_keys[k]); c->d_keys[k] = nullptr; }
    if (c->d_sort_tmp) { (void)hipFree(c->d_sort_tmp); c->d_sort_tmp = nullptr; }
    c->keys_cap = 0;
    int rc;
    for (int k = 0; k < 2; k++) if ((rc = dmalloc(&c->d_keys[k], n))) return rc;
    hipcub::DoubleBuffer<uint64_t> dk(c->d_keys[0], c->d_keys[1]);
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, c->sort_tmp_bytes, dk, (int64_t)n, 0, 64));
    HIP_TRY(hipMalloc(&c->d_sort_tmp, c->sort_tmp_bytes + 256));
    c->keys_cap = n;
    return 0;
}

// What the host has to do about a queued batch's bookkeeping once it is through: overflow checks, the records into the archives.
int profile_collect(mcx_ctx *c)
{
    auto &L = c->later;
    if (!L.pending) return 0;
    L.pending = false;
    HIP_TRY(hipEventSynchronize(L.done));
    const uint32_t n_sp = L.h_cnt[CNT_TASKS], n_ev = L.h_cnt[CNT_RESCUE];
    if (n_sp > c->sparse_cap || n_ev > L.ev_cap) return mcx_set_error(MCX_ERR_CAPACITY, "profile: sparse record list overflow");
    if (L.h_cnt[CNT_UNSUP]) return mcx_set_error(MCX_ERR_UNSUPPORTED, "an insertion or deletion of more than 255 bases in an alignment: its string does not fit a tally record");
    if (int rc = archive_append(c, c->arch, c->d_sparse, n_sp, L.stream)) return rc;
    if (int rc = archive_append(c, c->arch_ev, L.d_ev, n_ev, L.stream)) return rc;
    HIP_TRY(hipStreamSynchronize(L.stream)); // (the archives are read on the context's stream; the lists are the next batch's to fill)
    if (c->kn.timing) fprintf(stderr, "[mcx profile] %u tally records, %u events, %u listed fragments (queued behind the batch; looked at %.2f ms later)\n", n_sp, n_ev, L.h_cnt[CNT_RTASK],
                              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - L.t_queued).count());
    return 0;
}

// One shard: the whole bookkeeping of the batch just mapped — keys, sort, admission, accumulation — queued on the bookkeeping's stream; nothing of it is
// waited for here.  The number of keys stays on the device (k_prof_admit / k_prof_count take it from there), the break-point records' count stays where
// k_prof_keys left it.  The next batch's mapping writes the other set of detail records and flag bytes.
int profile_queue(mcx_ctx *c)
{
    if (c->prof_settled) return mcx_set_error(MCX_ERR_ARG, "the profile has been settled (mcx_profile_settle / _finalize): attach it again before mapping more reads");
    if (int rc = profile_collect(c)) return rc; // (the batch before this one: through long ago, it ran under this batch's kernels)
    auto &L = c->later;
    BatchRun &br = c->run;
    hipStream_t ps = L.stream;
    const IndexView &ix = c->idx->view;
    ProfView pv; pv.pl = planes_view(c->prof_planes, ix.G); pv.match = c->d_prof_match; pv.G = ix.G; pv.max_dup = c->prof_max_dup; pv.max_clip = c->prof_max_clip;
    SparseSink sink; sink.recs = c->d_sparse; sink.n = L.d_cnt + CNT_TASKS; sink.cap = c->sparse_cap; sink.refused = L.d_cnt + CNT_UNSUP;
    const uint32_t n = br.rb.n_reads;
    ReadBatch rb; rb.bases = L.d_keep_bases; rb.off = L.d_keep_off; rb.n_reads = n;
    HIP_TRY(hipEventSynchronize(L.kept)); // (the caller's buffer is the caller's again: the copy was made beside the batch's first kernels)
    HIP_TRY(hipEventRecord(L.go, c->t0.stream));
    HIP_TRY(hipStreamWaitEvent(ps, L.go, 0));
    HIP_TRY(hipMemsetAsync(L.d_cnt, 0, CNT_N * sizeof(uint32_t), ps));
    k_prof_keys<<<(n + 255) / 256, 256, 0, ps>>>(c->d_detail, c->dlay, rb, ix, pv, sink, c->d_keys[0], L.d_cnt + CNT_OV);
    hipcub::DoubleBuffer<uint64_t> dk(c->d_keys[0], c->d_keys[1]);
    size_t tb = c->sort_tmp_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(c->d_sort_tmp, tb, dk, (int64_t)n, 0, 64, ps));
    const uint64_t *d_keys = dk.Current(); // (the keys of the reads that do not reach the duplicate check are ~0 and sort behind the others)
    // the counters of the second half start at zero, but for the two the first half hands over: the keys' number, the break-point records'
    static_assert(CNT_OV < CNT_N && CNT_TASKS < CNT_N, "counter indices");
    k_zero_but<<<1, 64, 0, ps>>>(L.d_cnt, CNT_N, CNT_OV, CNT_TASKS);
    k_prof_admit<<<(n + 255) / 256, 256, 0, ps>>>(d_keys, 0, pv, c->d_admit, 0u, n, L.d_cnt + CNT_OV);
    k_prof_count<<<(n + 255) / 256, 256, 0, ps>>>(d_keys, 0, pv, L.d_cnt + CNT_OV);
    ColList cols; cols.items = c->d_prof_items; cols.n = L.d_cnt + CNT_RTASK; cols.cap = c->prof_items_cap;
    // (a smaller grid for the two — 512 to 4096 workgroups, the batch walked in strides — changes nothing: 28.8-29.3 ms per batch either way; what the bookkeeping
    //  and the mapping beside it share is the memory system's rate of scattered line transfers, not the CUs)
    k_prof_accum<<<(n + 255) / 256, 256, 0, ps>>>(c->d_detail, c->dlay, rb, ix, pv, sink, c->d_admit, br.paired, cols);
    k_prof_cols<<<4096, 256, 0, ps>>>(c->d_detail, c->dlay, rb, ix, pv, sink, cols);
    if (br.paired) k_prof_disc<<<(n / 2 + 255) / 256, 256, 0, ps>>>(c->d_detail, c->dlay, n / 2, br.read_base / 2, L.d_ev, L.d_cnt + CNT_RESCUE, L.ev_cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(L.h_cnt, L.d_cnt, CNT_N * sizeof(uint32_t), hipMemcpyDeviceToHost, ps));
    HIP_TRY(hipEventRecord(L.done, ps));
    L.pending = true; L.t_queued = std::chrono::steady_clock::now();
    std::swap(c->d_detail, L.d_detail_alt); std::swap(c->d_admit, L.d_admit_alt); // the next batch's mapping writes the other set,
    std::swap(L.d_keep_bases, L.d_keep_bases_alt); std::swap(L.d_keep_off, L.d_keep_off_alt); // its reads are kept in the other copy
    return 0;
}

// break points, clip gate, and the sorted (start position, read) keys of the reads that reach the duplicate check
int profile_keys(mcx_ctx *c)
{
    BatchRun &br = c->run;
    hipStream_t s = c->t0.stream;
    const IndexView &ix = c->idx->view;
    ProfView pv; pv.pl = planes_view(c->prof_planes, ix.G); pv.match = c->d_prof_match; pv.G = ix.G; pv.max_dup = c->prof_max_dup; pv.max_clip = c->prof_max_clip;
    SparseSink sink; sink.recs = c->d_sparse; sink.n = c->t0.d_cnt + CNT_TASKS; sink.cap = c->sparse_cap; sink.refused = c->t0.d_cnt + CNT_UNSUP;
    const uint32_t n = br.rb.n_reads;
    HIP_TRY(hipMemsetAsync(c->t0.d_cnt, 0, CNT_N * sizeof(uint32_t), s));
    k_prof_keys<<<(n + 255) / 256, 256, 0, s>>>(c->d_detail, c->dlay, br.rb, ix, pv, sink, c->d_keys[0], c->t0.d_cnt + CNT_OV);
    hipcub::DoubleBuffer<uint64_t> dk(c->d_keys[0], c->d_keys[1]);
    size_t tb = c->sort_tmp_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(c->d_sort_tmp, tb, dk, (int64_t)n, 0, 64, s));
    HIP_TRY(hipMemcpyAsync(c->t0.h_cnt, c->t0.d_cnt, CNT_N * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    br.d_sorted_keys = dk.Current();
    br.n_keys = c->t0.h_cnt[CNT_OV];       // the keys of the other reads are ~0 and sort behind them
    br.n_sparse_keys = c->t0.h_cnt[CNT_TASKS]; // break-point records so far; the accumulation appends behind them
    return 0;
}

// the keys of a round this shard has no reads in: only the run's readCount moves
int profile_foreign(mcx_ctx *c, const uint64_t *h_all, uint64_t n_all)
{
    if (n_all == 0) return 0;
    hipStream_t s = c->t0.stream;
    ProfView pv; pv.pl = planes_view(c->prof_planes, c->idx->view.G); pv.match = c->d_prof_match; pv.G = c->idx->view.G; pv.max_dup = c->prof_max_dup; pv.max_clip = c->prof_max_clip;
    int rc = sort_reserve(c, n_all);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_keys[0], h_all, n_all * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    hipcub::DoubleBuffer<uint64_t> dk(c->d_keys[0], c->d_keys[1]);
    size_t tb = c->sort_tmp_bytes;
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(c->d_sort_tmp, tb, dk, (int64_t)n_all, 0, 64, s));
    k_prof_count<<<(unsigned)((n_all + 255) / 256), 256, 0, s>>>(dk.Current(), n_all, pv);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// the archived records leave HBM: through the two halves of a page-locked bounce buffer (a copy from HBM straight into
// pageable memory runs at ~1 GB/s), the next piece in flight while this one is copied out
static int archive_flush(mcx_ctx *c, mcx_ctx::Archive &a)
{
    if (a.n == 0) return 0;
    hipStream_t s = c->t0.stream;
    std::vector<mcx_sparse_rec> &host = *a.host;
    const bool tallies = &a == &c->arch;
    if (tallies) host.resize(c->n_tally); // (what the last mcx_profile_sparse* call appended for its caller goes again)
    host.reserve(host.size() + a.n); // (no resize: that would be one thread zeroing fresh pages before the copy touches them again)
    const uint64_t half = c->sparse_pin_recs / 2;
    const uint64_t n_piece = (a.n + half - 1) / half;
    auto start = [&](uint64_t k) -> hipError_t {
        const uint64_t lo = k * half, m = std::min<uint64_t>(half, a.n - lo);
        return hipMemcpyAsync(c->h_sparse_pin + (k & 1) * half, a.d + lo, m * sizeof(SparseRec), hipMemcpyDeviceToHost, s);
    };
    HIP_TRY(start(0));
    for (uint64_t k = 0; k < n_piece; k++) {
        HIP_TRY(hipStreamSynchronize(s));
        if (k + 1 < n_piece) HIP_TRY(start(k + 1));
        const uint64_t lo = k * half, m = std::min<uint64_t>(half, a.n - lo);
        const mcx_sparse_rec *piece = (const mcx_sparse_rec *)(c->h_sparse_pin + (k & 1) * half);
        host.insert(host.end(), piece, piece + m);
    }
    a.n = 0;
    if (tallies) c->n_tally = host.size();
    return 0;
}

static int sparse_flush(mcx_ctx *c)
{
    if (int rc = profile_collect(c)) return rc;
    c->h_sparse.resize(c->n_tally);
    if (int rc = archive_flush(c, c->arch)) return rc;
    return archive_flush(c, c->arch_ev);
}

// n records at d_src join an archive (on the stream); an archive that cannot grow any more goes to the host first
int archive_append(mcx_ctx *c, mcx_ctx::Archive &a, const SparseRec *d_src, uint64_t n, hipStream_t on)
{
    if (n == 0) return 0;
    hipStream_t s = on ? on : c->t0.stream;
    if (a.n + n > a.cap) {
        const uint64_t want = std::max<uint64_t>({2 * a.cap, a.n + n, &a == &c->arch ? (uint64_t)1 << 22 : (uint64_t)1 << 18});
        SparseRec *grown = nullptr;
        if (want <= c->arch_limit && hipMalloc((void **)&grown, want * sizeof(SparseRec)) == hipSuccess) {
            if (a.n) HIP_TRY(hipMemcpyAsync(grown, a.d, a.n * sizeof(SparseRec), hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (a.d) (void)hipFree(a.d);
            a.d = grown; a.cap = want;
        } else {
            (void)hipGetLastError();
            if (c->kn.timing) fprintf(stderr, "[mcx profile] no room in HBM for a larger record archive (%llu records wanted): what it holds goes to the host now, batch by batch from here on\n", (unsigned long long)want);
            int rc = archive_flush(c, a); // no room for a larger archive: what it holds goes to the host now
            if (rc) return rc;
            if (n > a.cap) {
                if (a.d) (void)hipFree(a.d);
                a.d = nullptr; a.cap = 0;
                HIP_TRY(hipMalloc((void **)&a.d, (size_t)n * sizeof(SparseRec)));
                a.cap = n;
            }
        }
    }
    HIP_TRY(hipMemcpyAsync(a.d + a.n, d_src, (size_t)n * sizeof(SparseRec), hipMemcpyDeviceToDevice, s));
    a.n += n;
    return 0;
}

// admission over `all` keys (null: the batch's own, already sorted on the device), then the accumulation of the own reads
int profile_accumulate(mcx_ctx *c, const uint64_t *h_all, uint64_t n_all, uint32_t slot_stride, uint32_t own_slot)
{
    if (c->prof_settled) return mcx_set_error(MCX_ERR_ARG, "the profile has been settled (mcx_profile_settle / _finalize): attach it again before mapping more reads");
    BatchRun &br = c->run;
    hipStream_t s = c->t0.stream;
    const IndexView &ix = c->idx->view;
    ProfView pv; pv.pl = planes_view(c->prof_planes, ix.G); pv.match = c->d_prof_match; pv.G = ix.G; pv.max_dup = c->prof_max_dup; pv.max_clip = c->prof_max_clip;
    SparseSink sink; sink.recs = c->d_sparse; sink.n = c->t0.d_cnt + CNT_TASKS; sink.cap = c->sparse_cap; sink.refused = c->t0.d_cnt + CNT_UNSUP;
    const uint32_t n = br.rb.n_reads;
    const int paired = br.paired;
    const uint64_t *d_keys = br.d_sorted_keys;
    uint64_t nk = br.n_keys;
    uint32_t own_lo = 0;
    if (h_all) {
        int rc = sort_reserve(c, std::max<uint64_t>(n_all, 1)); // (invalidates br.d_sorted_keys: the own keys are part of h_all)
        if (rc) return rc;
        if (n_all) HIP_TRY(hipMemcpyAsync(c->d_keys[0], h_all, n_all * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        hipcub::DoubleBuffer<uint64_t> dk(c->d_keys[0], c->d_keys[1]);
        size_t tb = c->sort_tmp_bytes;
        if (n_all) HIP_TRY(hipcub::DeviceRadixSort::SortKeys(c->d_sort_tmp, tb, dk, (int64_t)n_all, 0, 64, s));
        d_keys = dk.Current(); nk = n_all; own_lo = own_slot * slot_stride;
    }
    HIP_TRY(hipMemsetAsync(c->t0.d_cnt, 0, CNT_N * sizeof(uint32_t), s));
    HIP_TRY(hipMemcpyAsync(c->t0.d_cnt + CNT_TASKS, &br.n_sparse_keys, sizeof(uint32_t), hipMemcpyHostToDevice, s)); // (pageable source: copied before the call returns)
    if (nk) {
        k_prof_admit<<<(unsigned)((nk + 255) / 256), 256, 0, s>>>(d_keys, nk, pv, c->d_admit, own_lo, n);
        k_prof_count<<<(unsigned)((nk + 255) / 256), 256, 0, s>>>(d_keys, nk, pv);
    }
    ColList cols; cols.items = c->d_prof_items; cols.n = c->t0.d_cnt + CNT_RTASK; cols.cap = c->prof_items_cap;
    k_prof_accum<<<(n + 255) / 256, 256, 0, s>>>(c->d_detail, c->dlay, br.rb, ix, pv, sink, c->d_admit, paired, cols); // (bit 1 of a flag byte: k_pack_reads')
    k_prof_cols<<<4096, 256, 0, s>>>(c->d_detail, c->dlay, br.rb, ix, pv, sink, cols);
    SparseRec *d_ev = (SparseRec *)c->t0.d_tasks; // the SA task list is idle now
    const uint32_t ev_cap = (uint32_t)std::min<uint64_t>((uint64_t)c->t0.task_cap * sizeof(uint2) / sizeof(SparseRec), 0x7fffffffu);
    if (paired) k_prof_disc<<<(n / 2 + 255) / 256, 256, 0, s>>>(c->d_detail, c->dlay, n / 2, br.read_base / 2, d_ev, c->t0.d_cnt + CNT_RESCUE, ev_cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->t0.h_cnt, c->t0.d_cnt, CNT_N * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t n_sp = c->t0.h_cnt[CNT_TASKS], n_ev = c->t0.h_cnt[CNT_RESCUE];
    if (n_sp > c->sparse_cap || n_ev > ev_cap) return mcx_set_error(MCX_ERR_CAPACITY, "profile: sparse record list overflow");
    if (c->t0.h_cnt[CNT_UNSUP]) return mcx_set_error(MCX_ERR_UNSUPPORTED, "an insertion or deletion of more than 255 bases in an alignment: its string does not fit a tally record");
    // the records stay in HBM until somebody asks for them (mcx_profile_sparse*)
    const auto t_app = std::chrono::steady_clock::now();
    if (int rc = archive_append(c, c->arch, c->d_sparse, n_sp)) return rc;
    const int rc_ev = archive_append(c, c->arch_ev, d_ev, n_ev);
    if (c->kn.timing) fprintf(stderr, "[mcx profile] %u tally records, %u events, %u listed fragments; archives %.2f ms\n", n_sp, n_ev, c->t0.h_cnt[CNT_RTASK],
                                      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_app).count());
    return rc_ev;
}

// the planes kept as differences become counts (mcx_profile.h): once per run, after its last batch
extern "C" int mcx_profile_settle(mcx_ctx *c)
{
    if (!c) return mcx_set_error(MCX_ERR_ARG, "mcx_profile_settle: null argument");
    if (c->prof_broken) return mcx_set_error(MCX_ERR_DEVICE, "an earlier mcx_profile_settle failed half way: the planes are neither differences nor counts; attach the profile again");
    if (!c->prof_planes || c->prof_settled) return 0;
    HIP_TRY(hipSetDevice(c->idx->device));
    if (int rc = profile_collect(c)) return rc; // (the last batch's bookkeeping)
    hipStream_t s = c->t0.stream;
    const IndexView &ix = c->idx->view;
    const size_t G = (size_t)ix.G;
    const PlanesView pl = planes_view(c->prof_planes, ix.G);
    size_t tb = 0, tb16 = 0;
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tb, pl.multi, pl.multi, G, s));
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, tb16, c->d_prof_match, c->d_prof_match, G, s));
    tb = std::max(tb, tb16);
    void *tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, tb + 256)); // (nothing touched yet: a retry is safe)
    hipError_t e = hipcub::DeviceScan::InclusiveSum(tmp, tb, pl.multi, pl.multi, G, s);
    // the 16-bit difference planes: their words back to two differences each (mcx_planes.h), then the scan modulo 2^16
    uint16_t *diffs[5] = {pl.h(kPlF1), pl.h(kPlR2), pl.h(kPlF2), pl.h(kPlR1), c->d_prof_match};
    for (int k = 0; k < 5 && e == hipSuccess; k++) {
        k_prof_decode<<<8192, 256, 0, s>>>((uint32_t *)diffs[k], pl.stride / 2);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipcub::DeviceScan::InclusiveSum(tmp, tb, diffs[k], diffs[k], G, s);
    }
    if (e == hipSuccess) {
        ProfView pv; pv.pl = pl; pv.match = c->d_prof_match; pv.G = ix.G; pv.max_dup = c->prof_max_dup; pv.max_clip = c->prof_max_clip;
        k_prof_fold<<<8192, 256, 0, s>>>(ix, pv);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(tmp);
    if (e != hipSuccess) { c->prof_broken = c->prof_settled = true; HIP_TRY(e); } // (a second settle must not scan the scanned planes again)
    (void)hipFree(c->d_prof_match); c->d_prof_match = nullptr; // (6 GB at 3.1 Gbp: the variant caller's scans want the room)
    c->prof_settled = true;
    return 0;
}

extern "C" int mcx_profile_finalize(mcx_ctx *c, uint32_t *d_planes)
{
    if (!c || !d_planes) return mcx_set_error(MCX_ERR_ARG, "mcx_profile_finalize: null argument");
    HIP_TRY(hipSetDevice(c->idx->device));
    if (d_planes == c->prof_planes) { if (int rc = mcx_profile_settle(c)) return rc; }
    k_prof_finalize<<<dim3(4096, kPlanes), 256, 0, c->t0.stream>>>(planes_view(d_planes, c->idx->view.G), c->prof_max_dup);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->t0.stream));
    return 0;
}

extern "C" int mcx_profile_sparse(mcx_ctx *c, const mcx_sparse_rec **recs, uint64_t *n)
{
    if (!c || !recs || !n) return mcx_set_error(MCX_ERR_ARG, "mcx_profile_sparse: null argument");
    HIP_TRY(hipSetDevice(c->idx->device));
    if (int rc = sparse_flush(c)) return rc;
    mcx_disc_resolve(c->h_events.data(), c->h_events.size(), c->idx->view.G, c->h_sparse); // (appended behind the tallies: no second copy of them)
    *recs = c->h_sparse.data(); *n = c->h_sparse.size();
    return 0;
}

extern "C" int mcx_profile_sparse_shard(mcx_ctx *c, const mcx_sparse_rec **recs, uint64_t *n)
{
    if (!c || !recs || !n) return mcx_set_error(MCX_ERR_ARG, "mcx_profile_sparse_shard: null argument");
    HIP_TRY(hipSetDevice(c->idx->device));
    if (int rc = sparse_flush(c)) return rc;
    c->h_sparse.insert(c->h_sparse.end(), c->h_events.begin(), c->h_events.end());
    *recs = c->h_sparse.data(); *n = c->h_sparse.size();
    return 0;
}

