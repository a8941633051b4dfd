// mapcaller_amd/csrc/mcx_stream.hip — batches from host memory, three in flight (copy in | kernels | copy out), each in a slot of
// the context: the bulk copies, the 2-bit rows of mcx_stream_submit_packed back to bytes (k_unpack_reads, k_apply_odd,
// k_neutralize), the 32-byte records and the -m extras on their way out (k_pack_recs, slot_multi_*), and the mcx_stream_* ABI.
// Reached through that ABI alone; it calls mcx_map_batch_dev and pack_reads() (mcx_pipeline.hip).
#include "mcx_ctx.h"
#include <hipcub/hipcub.hpp>

// ---------------------------------------------------------------------------------------------
// batches from host memory with the copies overlapped with the kernels
// ---------------------------------------------------------------------------------------------
// Bulk copies across the device boundary: the DMA engines by default (52 GB/s each way on the test box, and they leave the
// CUs to the kernels).  MCX_STREAM_KERNEL_COPY=1 moves them with a kernel instead (page-locked host memory is mapped into
// the device's address space) — measured slower next to the mapping kernels (82 ms instead of 70 ms per 8 M-read batch), kept for
// boxes whose DMA queues are the bottleneck.
__global__ void __launch_bounds__(256) k_copy16(const U4 *__restrict__ src, U4 *__restrict__ dst, uint64_t n16)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

static int bulk_copy(mcx_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s)
{
    if (bytes == 0) return 0;
    // (MCX_STREAM_KERNEL_COPY: this library's own copy kernel over the mapped host memory instead of the runtime's copies — round 5 tried it for the way out
    //  alone, on grids of 16 / 48 / 128 workgroups, next to the mapping kernels: 23.7 / 26.1 / 27.2 ms per step against the runtime's 20.6)
    static const char *mode = getenv("MCX_STREAM_KERNEL_COPY"); // ("in" / "out": one direction alone)
    static const int blocks = getenv("MCX_COPY_BLOCKS") ? atoi(getenv("MCX_COPY_BLOCKS")) : 512;
    const bool use_dma = mode == nullptr || (!strcmp(mode, "in") && kind != hipMemcpyHostToDevice) || (!strcmp(mode, "out") && kind != hipMemcpyDeviceToHost);
    const size_t n16 = bytes / 16;
    bool mapped = false; // is the host side page-locked memory the device can address?
    {
        hipPointerAttribute_t a;
        const void *host = kind == hipMemcpyHostToDevice ? src : dst;
        if (hipPointerGetAttributes(&a, host) == hipSuccess) mapped = a.type == hipMemoryTypeHost;
        else (void)hipGetLastError();
    }
    if (use_dma || !mapped || n16 == 0 || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15)) { HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, s)); return 0; }
    k_copy16<<<blocks, 256, 0, s>>>((const U4 *)src, (U4 *)dst, (uint64_t)n16);
    HIP_TRY(hipGetLastError());
    if (bytes & 15) HIP_TRY(hipMemcpyAsync((uint8_t *)dst + n16 * 16, (const uint8_t *)src + n16 * 16, bytes & 15, kind, s));
    (void)c;
    return 0;
}

static mcx_ctx::Slot *oldest_slot(mcx_ctx *c, int state)
{
    mcx_ctx::Slot *best = nullptr;
    for (auto &sl : c->slot) if (sl.state == state && (!best || sl.seq < best->seq)) best = &sl;
    return best;
}

// a free slot, its HBM allocated on first use
static int stream_slot(mcx_ctx *c, mcx_ctx::Slot **out)
{
    mcx_ctx::Slot *sl = oldest_slot(c, 0);
    if (!sl) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_submit: three batches are in flight (collect one first)");
    int rc;
    if (!c->h2d_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&c->h2d_stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&c->d2h_stream, hipStreamNonBlocking));
    }
    if (!sl->d_bases) {
        if ((rc = dmalloc(&sl->d_bases, c->max_bases + 16 * c->max_reads + 64))) return rc; // (+16 per read: packed rows end on a word)
        if ((rc = dmalloc(&sl->d_off, c->max_reads + 1))) return rc;
        if ((rc = dmalloc(&sl->d_recs, c->max_reads))) return rc;
        if ((rc = dmalloc(&sl->d_cig, MCX_CIGAR_POOL_WORDS(c->max_reads)))) return rc;
        HIP_TRY(hipEventCreateWithFlags(&sl->in_ready, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&sl->mapped, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&sl->out_done, hipEventDisableTiming));
    }
    *out = sl;
    return 0;
}

// 2-bit rows -> the ASCII bytes of the batch: one thread per sixteen bases (the letters ACGT; k_apply_odd puts back every other byte)
// (the lengths are the caller's: one beyond its row or the context's longest read — lim —, or a sum beyond the slot — max_bases —, is flagged in
//  *err and nothing is written for it; mcx_stream_next refuses the batch.  Round 4 walked the lengths on the host before the copy: a
//  millisecond per 8 M reads with the GPU idle.)
__global__ void __launch_bounds__(256) k_unpack_reads(const uint32_t *codes, uint32_t row_words, const uint32_t *off, uint32_t n_reads, uint8_t *bases,
                                                      uint64_t max_bases, uint32_t lim, uint32_t *err)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t r = (uint32_t)(t / row_words), k = (uint32_t)(t % row_words);
    if (r >= n_reads) return;
    const uint32_t o = off[r], rlen = off[r + 1] - o;
    if (rlen > lim || off[r + 1] < o) { if (k == 0) atomicOr(err, 1u); return; }
    if ((uint64_t)o + rlen > max_bases) { if (k == 0) atomicOr(err, 2u); return; }
    if (16 * k >= rlen) return;
    const uint32_t w = codes[(uint64_t)r * row_words + k];
    uint32_t q[4]; // sixteen letters, four to a word, the first in the low byte
#pragma unroll
    for (int g = 0; g < 4; g++) {
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t c = (w >> (30 - 2 * (4 * g + i))) & 3u;
            v |= (uint32_t)((0x54474341u >> (8 * c)) & 0xFFu) << (8 * i); // "ACGT"
        }
        q[g] = v;
    }
    uint8_t *dst = bases + o + 16 * k;
    const uint32_t nb = rlen - 16 * k < 16 ? rlen - 16 * k : 16;
    const uintptr_t a = (uintptr_t)dst;
    if (nb == 16 && (a & 3) == 0) { uint32_t *d4 = (uint32_t *)dst; d4[0] = q[0]; d4[1] = q[1]; d4[2] = q[2]; d4[3] = q[3]; }
    else if (nb == 16 && (a & 1) == 0) { uint16_t *d2 = (uint16_t *)dst; for (int i = 0; i < 8; i++) d2[i] = (uint16_t)(q[i >> 1] >> (16 * (i & 1))); }
    else for (uint32_t i = 0; i < nb; i++) dst[i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));
}

__global__ void k_apply_odd(const uint64_t *odd, uint32_t n_odd, const uint32_t *off, uint32_t n_reads, uint8_t *bases, uint64_t max_bases)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_odd) return;
    const uint64_t e = odd[i];
    const uint32_t r = (uint32_t)(e >> 32), pos = (uint32_t)(e >> 8) & 0xFFFFFFu;
    if (r < n_reads && off[r + 1] >= off[r] && pos < off[r + 1] - off[r] && (uint64_t)off[r] + pos < max_bases) bases[off[r] + pos] = (uint8_t)e;
}

// a batch whose lengths k_unpack_reads refused maps nothing: every read becomes empty, so that no kernel behind this one meets a length it was not sized
// for — the host hears of it when it next looks (mcx_stream_map), not before the batch's first kernel: no wait at the start of a step
__global__ void __launch_bounds__(256) k_neutralize(uint32_t *off, uint32_t n_reads, const uint32_t *err)
{
    if (*err == 0) return;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r <= n_reads; r += gridDim.x * blockDim.x) off[r] = 0;
}

// 2-bit rows into a free slot and back to bytes there.  kind: where the caller's arrays lie — host memory (mcx_stream_submit_packed: over the device boundary,
// counted in bytes_in) or the context's device (mcx_stream_submit_dev: device-to-device copies on the same copy-in stream, not counted)
static int submit_rows(mcx_ctx *c, const uint32_t *codes, uint32_t row_words, const uint32_t *len, uint32_t n_reads, const uint64_t *odd, uint32_t n_odd, hipMemcpyKind kind,
                       const char *who)
{
    if (!c || !codes || !len || n_reads == 0 || row_words == 0 || (n_odd && !odd)) return mcx_set_error(MCX_ERR_ARG, std::string(who) + ": bad argument");
    if (n_reads > c->max_reads) return mcx_set_error(MCX_ERR_ARG, "batch larger than max_batch_reads");
    const uint32_t row_max = (uint32_t)(c->rlen_max + 15) / 16;
    if (row_words > row_max) return mcx_set_error(MCX_ERR_UNSUPPORTED, std::string(who) + ": rows are longer than max_read_len");
    HIP_TRY(hipSetDevice(c->idx->device));
    mcx_ctx::Slot *sl = nullptr;
    int rc = stream_slot(c, &sl);
    if (rc) return rc;
    hipStream_t s = c->h2d_stream;
    if (!sl->d_codes) {
        if ((rc = dmalloc(&sl->d_codes, c->max_reads * (uint64_t)row_max))) return rc;
        if ((rc = dmalloc(&sl->d_len, c->max_reads + 1))) return rc;
        if ((rc = dmalloc(&sl->d_err, 1))) return rc;
        HIP_TRY(hipHostMalloc((void **)&sl->h_err, sizeof(uint32_t)));
        *sl->h_err = 0;
    }
    if (n_odd > sl->odd_cap) {
        if (sl->d_odd) { HIP_TRY(hipStreamSynchronize(s)); (void)hipFree(sl->d_odd); sl->d_odd = nullptr; }
        sl->odd_cap = std::max<uint32_t>(n_odd + n_odd / 2, 1u << 16);
        if ((rc = dmalloc(&sl->d_odd, sl->odd_cap))) return rc;
    }
    if (!c->d_scan_tmp) {
        size_t need = 0;
        HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, need, sl->d_len, sl->d_off + 1, (int)c->max_reads, s));
        c->scan_tmp_bytes = need + 256;
        HIP_TRY(hipMalloc(&c->d_scan_tmp, c->scan_tmp_bytes));
    }
    if ((rc = bulk_copy(c, sl->d_codes, codes, (size_t)n_reads * row_words * 4, kind, s))) return rc;
    if ((rc = bulk_copy(c, sl->d_len, len, (size_t)n_reads * 4, kind, s))) return rc;
    if (n_odd && (rc = bulk_copy(c, sl->d_odd, odd, (size_t)n_odd * 8, kind, s))) return rc;
    HIP_TRY(hipMemsetAsync(sl->d_off, 0, 4, s));
    size_t tmp = c->scan_tmp_bytes;
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(c->d_scan_tmp, tmp, sl->d_len, sl->d_off + 1, (int)n_reads, s));
    const uint64_t threads = (uint64_t)n_reads * row_words;
    HIP_TRY(hipMemsetAsync(sl->d_err, 0, 4, s));
    k_unpack_reads<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(sl->d_codes, row_words, sl->d_off, n_reads, sl->d_bases, c->max_bases,
                                                                   std::min<uint32_t>(row_words * 16u, (uint32_t)c->rlen_max), sl->d_err);
    if (n_odd) k_apply_odd<<<(n_odd + 255) / 256, 256, 0, s>>>(sl->d_odd, n_odd, sl->d_off, n_reads, sl->d_bases, c->max_bases);
    k_neutralize<<<256, 256, 0, s>>>(sl->d_off, n_reads, sl->d_err);
    HIP_TRY(hipGetLastError());
    sl->lens_checked = true;
    // the batch's 2-bit form for the kernels, made here — behind its copy in, under the batch before it — instead of at the start of its own step (0.76 ms of
    // the step per 8 M reads).  Mated or not is a guess (what the last batch was); a wrong one, or a profile attached meanwhile, and the step packs as before.
    sl->prepacked = false;
    if (!c->prof_planes && !c->kn.no_prepack) {
        if (!sl->d_prepack) {
            if ((rc = dmalloc(&sl->d_prepack, c->max_reads * (uint64_t)c->wpad))) return rc;
            if ((rc = dmalloc(&sl->d_any_n, 1))) return rc;
        }
        ReadBatch rb; rb.bases = sl->d_bases; rb.off = sl->d_off; rb.n_reads = n_reads;
        const int tpr = (c->rlen_max + 31) / 32 + 1;
        HIP_TRY(hipMemsetAsync(sl->d_any_n, 0, 4, s));
        pack_reads(rb, c->last_paired, c->wpad, tpr, sl->d_prepack, sl->d_any_n, nullptr, s);
        HIP_TRY(hipGetLastError());
        sl->prepacked = true; sl->pre_paired = c->last_paired;
    }
    HIP_TRY(hipEventRecord(sl->in_ready, s));
    sl->n_reads = n_reads; sl->state = 1; sl->seq = ++c->stream_seq;
    if (kind == hipMemcpyHostToDevice) c->stream_bytes_in += (uint64_t)n_reads * row_words * 4 + (uint64_t)n_reads * 4 + (uint64_t)n_odd * 8;
    return 0;
}

extern "C" int mcx_stream_submit_packed(mcx_ctx *c, const uint32_t *codes, uint32_t row_words, const uint32_t *len, uint32_t n_reads, const uint64_t *odd,
                                        uint32_t n_odd)
{
    return submit_rows(c, codes, row_words, len, n_reads, odd, n_odd, hipMemcpyHostToDevice, "mcx_stream_submit_packed");
}

extern "C" int mcx_stream_submit_dev(mcx_ctx *c, const uint32_t *d_codes, uint32_t row_words, const uint32_t *d_len, uint32_t n_reads, const uint64_t *d_odd,
                                     uint32_t n_odd)
{
    return submit_rows(c, d_codes, row_words, d_len, n_reads, d_odd, n_odd, hipMemcpyDeviceToDevice, "mcx_stream_submit_dev");
}

extern "C" int mcx_stream_submit(mcx_ctx *c, const uint8_t *bases, const uint32_t *off, uint32_t n_reads)
{
    if (!c || !bases || !off || n_reads == 0) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_submit: bad argument");
    if (n_reads > c->max_reads) return mcx_set_error(MCX_ERR_ARG, "batch larger than max_batch_reads");
    if (off[n_reads] > c->max_bases) return mcx_set_error(MCX_ERR_ARG, "batch holds more bases than max_batch_reads * max_read_len");
    HIP_TRY(hipSetDevice(c->idx->device));
    mcx_ctx::Slot *sl = nullptr;
    int rc = stream_slot(c, &sl);
    if (rc) return rc;
    if (sl->d_err) HIP_TRY(hipMemsetAsync(sl->d_err, 0, 4, c->h2d_stream)); // (the slot once took 2-bit rows: nothing of that batch's verdict is this one's)
    sl->lens_checked = false; sl->prepacked = false;
    if ((rc = bulk_copy(c, sl->d_bases, bases, off[n_reads], hipMemcpyHostToDevice, c->h2d_stream))) return rc;
    if ((rc = bulk_copy(c, sl->d_off, off, (size_t)(n_reads + 1) * 4, hipMemcpyHostToDevice, c->h2d_stream))) return rc;
    HIP_TRY(hipEventRecord(sl->in_ready, c->h2d_stream));
    sl->n_reads = n_reads; sl->state = 1; sl->seq = ++c->stream_seq;
    c->stream_bytes_in += (uint64_t)off[n_reads] + (uint64_t)(n_reads + 1) * 4;
    return 0;
}

// the oldest submitted batch, in HBM once the context's stream gets there
extern "C" int mcx_stream_next(mcx_ctx *c, const uint8_t **d_bases, const uint32_t **d_off, uint32_t *n_reads, mcx_aln **d_aln, uint32_t **d_cigar)
{
    if (c) c->mx.ready = false; // (-m: the extras in the context are of a batch before this one)
    if (!c || !d_bases || !d_off || !d_aln || !d_cigar) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_next: null argument");
    HIP_TRY(hipSetDevice(c->idx->device));
    if (oldest_slot(c, 2)) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_next: the previous batch was not handed back (mcx_stream_mapped)");
    mcx_ctx::Slot *sl = oldest_slot(c, 1);
    if (!sl) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_next: nothing submitted");
    HIP_TRY(hipStreamWaitEvent(c->t0.stream, sl->in_ready, 0));
    c->lens_checked = sl->lens_checked; // (for the mcx_batch_begin that follows: no need to look for an over-long read, nor to wait for the answer)
    c->lens_checked_off = sl->d_off; c->lens_checked_bases = sl->d_bases;
    c->pre = mcx_ctx::PrePacked();
    if (sl->prepacked) { c->pre.packed = sl->d_prepack; c->pre.bases = sl->d_bases; c->pre.paired = sl->pre_paired; c->pre.any_n = sl->d_any_n; }
    sl->state = 2;
    *d_bases = sl->d_bases; *d_off = sl->d_off; *d_aln = (mcx_aln *)sl->d_recs; *d_cigar = sl->d_cig;
    if (n_reads) *n_reads = sl->n_reads;
    return 0;
}

__global__ void __launch_bounds__(256) k_pack_recs(const AlnRec *recs, uint32_t n, mcx_aln32 *out);

// (-m) the batch's extras, in read order in the context's buffers until its next batch begins, go into the slot's own on the
// mapping stream (packed to mcx_aln32 like the records) — behind its `mapped` event their copy out joins the records'
static int slot_multi_pack(mcx_ctx *c, mcx_ctx::Slot *sl)
{
    auto &o = sl->mx;
    const auto &m = c->mx;
    o.have = m.on && m.ready && m.n_reads == sl->n_reads;
    if (!o.have) { o.n_reads = o.n_recs = o.n_words = 0; return 0; }
    int rc;
    if (!o.d_index && (rc = dmalloc(&o.d_index, c->max_reads + 1))) return rc;
    if (m.n_recs > o.rec_cap) {
        if (o.d_recs) (void)hipFree(o.d_recs);
        o.d_recs = nullptr; o.rec_cap = 0;
        if ((rc = dmalloc(&o.d_recs, (size_t)m.n_recs + m.n_recs / 2 + 1024))) return rc;
        o.rec_cap = m.n_recs + m.n_recs / 2 + 1024;
    }
    if (m.n_words > o.word_cap) {
        if (o.d_cig) (void)hipFree(o.d_cig);
        o.d_cig = nullptr; o.word_cap = 0;
        if ((rc = dmalloc(&o.d_cig, (size_t)m.n_words + m.n_words / 2 + 4096))) return rc;
        o.word_cap = m.n_words + m.n_words / 2 + 4096;
    }
    o.n_reads = m.n_reads; o.n_recs = m.n_recs; o.n_words = m.n_words;
    HIP_TRY(hipMemcpyAsync(o.d_index, m.d_index, ((size_t)o.n_reads + 1) * 4, hipMemcpyDeviceToDevice, c->t0.stream));
    if (o.n_words) HIP_TRY(hipMemcpyAsync(o.d_cig, m.d_out_cig, (size_t)o.n_words * 4, hipMemcpyDeviceToDevice, c->t0.stream));
    if (o.n_recs) k_pack_recs<<<(o.n_recs + 255) / 256, 256, 0, c->t0.stream>>>(m.d_out, o.n_recs, o.d_recs);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ... and their copy to the slot's page-locked buffers on the copy-out stream (counted in bytes_out)
static int slot_multi_out(mcx_ctx *c, mcx_ctx::Slot *sl)
{
    auto &o = sl->mx;
    if (!o.have) return 0;
    if (!o.h_index) { o.h_index = (uint32_t *)mcx_pinned_alloc((c->max_reads + 1) * 4); if (!o.h_index) return mcx_set_error(MCX_ERR_DEVICE, "cannot allocate pinned host memory"); }
    if (o.n_recs > o.h_rec_cap) {
        mcx_pinned_free(o.h_recs); o.h_rec_cap = o.rec_cap;
        if (!(o.h_recs = (mcx_aln32 *)mcx_pinned_alloc((size_t)o.h_rec_cap * sizeof(mcx_aln32)))) { o.h_rec_cap = 0; return mcx_set_error(MCX_ERR_DEVICE, "cannot allocate pinned host memory"); }
    }
    if (o.n_words > o.h_word_cap) {
        mcx_pinned_free(o.h_cig); o.h_word_cap = o.word_cap;
        if (!(o.h_cig = (uint32_t *)mcx_pinned_alloc((size_t)o.h_word_cap * 4))) { o.h_word_cap = 0; return mcx_set_error(MCX_ERR_DEVICE, "cannot allocate pinned host memory"); }
    }
    const size_t b_index = ((size_t)o.n_reads + 1) * 4, b_recs = (size_t)o.n_recs * sizeof(mcx_aln32), b_cig = (size_t)o.n_words * 4;
    HIP_TRY(hipMemcpyAsync(o.h_index, o.d_index, b_index, hipMemcpyDeviceToHost, c->d2h_stream));
    if (b_recs) HIP_TRY(hipMemcpyAsync(o.h_recs, o.d_recs, b_recs, hipMemcpyDeviceToHost, c->d2h_stream));
    if (b_cig) HIP_TRY(hipMemcpyAsync(o.h_cig, o.d_cig, b_cig, hipMemcpyDeviceToHost, c->d2h_stream));
    c->stream_bytes_out += b_index + b_recs + b_cig;
    return 0;
}

extern "C" int mcx_stream_multi(mcx_ctx *c, const uint32_t **index, const mcx_aln32 **recs, const uint32_t **cigar, uint32_t *n_reads, uint32_t *n_recs, uint32_t *n_words)
{
    if (!c) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_multi: null argument");
    if (!c->mx.on) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_multi: -m is off (mcx_ctx_set_multi)");
    const mcx_ctx::Slot *sl = c->collected;
    const bool have = sl && sl->mx.have;
    if (index) *index = have ? sl->mx.h_index : nullptr;
    if (recs) *recs = have ? sl->mx.h_recs : nullptr;
    if (cigar) *cigar = have ? sl->mx.h_cig : nullptr;
    if (n_reads) *n_reads = have ? sl->mx.n_reads : 0;
    if (n_recs) *n_recs = have ? sl->mx.n_recs : 0;
    if (n_words) *n_words = have ? sl->mx.n_words : 0;
    return 0;
}

// the batch mcx_stream_next gave out is mapped: its results start their way to host memory
extern "C" int mcx_stream_mapped(mcx_ctx *c, mcx_aln *aln, uint32_t *cigar)
{
    if (!c || !aln || !cigar) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_mapped: null argument");
    HIP_TRY(hipSetDevice(c->idx->device));
    mcx_ctx::Slot *sl = oldest_slot(c, 2);
    if (!sl) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_mapped: no batch is being mapped");
    int rc;
    if ((rc = slot_multi_pack(c, sl))) return rc;
    HIP_TRY(hipEventRecord(sl->mapped, c->t0.stream));
    HIP_TRY(hipStreamWaitEvent(c->d2h_stream, sl->mapped, 0));
    const size_t rec_bytes = (size_t)sl->n_reads * sizeof(AlnRec), cig_bytes = (size_t)c->run.cig_words * 4; // (the pool's used words only)
    if ((rc = slot_multi_out(c, sl))) return rc;
    if ((rc = bulk_copy(c, aln, sl->d_recs, rec_bytes, hipMemcpyDeviceToHost, c->d2h_stream))) return rc;
    if ((rc = bulk_copy(c, cigar, sl->d_cig, cig_bytes, hipMemcpyDeviceToHost, c->d2h_stream))) return rc;
    if (sl->lens_checked) HIP_TRY(hipMemcpyAsync(sl->h_err, sl->d_err, 4, hipMemcpyDeviceToHost, c->d2h_stream)); // what k_unpack_reads thought of the caller's lengths: mcx_stream_collect reads it
    HIP_TRY(hipEventRecord(sl->out_done, c->d2h_stream));
    sl->state = 3;
    c->stream_bytes_out += rec_bytes + cig_bytes;
    return 0;
}

// the records of a mapped batch in 32 bytes each (mcx_aln32, include/mcx.h) for their way to the host
__global__ void __launch_bounds__(256) k_pack_recs(const AlnRec *recs, uint32_t n, mcx_aln32 *out)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const AlnRec a = recs[r];
    mcx_aln32 o;
    o.pos_lo = (uint32_t)a.pos; o.pos_hi = (uint8_t)((uint64_t)a.pos >> 32); o.mate_lo = (uint32_t)a.mate_pos; o.mate_hi = (uint8_t)((uint64_t)a.mate_pos >> 32);
    o.mapq = (uint8_t)a.mapq; o.bits = (uint8_t)((a.fwd ? 1 : 0) | (a.has_mate ? 2 : 0)); o.tlen = a.tlen; o.flag = (uint16_t)a.flag;
    o.chr = a.chr < 0 ? (uint16_t)0xFFFFu : (uint16_t)a.chr; o.nm = (int16_t)a.nm; o.as = (int16_t)a.as; o.xs = (int16_t)a.xs;
    o.n_cigar = (uint16_t)a.n_cigar; o.cigar_off = (uint32_t)a.pad[0];
    ((U4 *)out)[2 * (uint64_t)r] = ((const U4 *)&o)[0]; ((U4 *)out)[2 * (uint64_t)r + 1] = ((const U4 *)&o)[1];
}

extern "C" int mcx_stream_mapped32(mcx_ctx *c, mcx_aln32 *aln, uint32_t *cigar)
{
    static_assert(sizeof(mcx_aln32) == 32, "mcx_aln32 is two 16-byte words");
    if (!c || !aln || !cigar) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_mapped32: null argument");
    HIP_TRY(hipSetDevice(c->idx->device));
    mcx_ctx::Slot *sl = oldest_slot(c, 2);
    if (!sl) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_mapped32: no batch is being mapped");
    if (c->idx->view.n_chr >= 0xFFFF || (c->idx->view.G2 >> 40)) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_stream_mapped32: more than 65534 contigs or positions beyond 2^40 (use mcx_stream_mapped)");
    int rc;
    if (!sl->d_recs32 && (rc = dmalloc(&sl->d_recs32, c->max_reads))) return rc;
    k_pack_recs<<<(sl->n_reads + 255) / 256, 256, 0, c->t0.stream>>>(sl->d_recs, sl->n_reads, sl->d_recs32); // (a read's operations are at most MCX_CIGAR_STRIDE x the pool's slack: far below 2^16)
    HIP_TRY(hipGetLastError());
    if ((rc = slot_multi_pack(c, sl))) return rc;
    HIP_TRY(hipEventRecord(sl->mapped, c->t0.stream));
    HIP_TRY(hipStreamWaitEvent(c->d2h_stream, sl->mapped, 0));
    const size_t rec_bytes = (size_t)sl->n_reads * sizeof(mcx_aln32), cig_bytes = (size_t)c->run.cig_words * 4; // (the pool's used words only)
    if ((rc = slot_multi_out(c, sl))) return rc;
    if ((rc = bulk_copy(c, aln, sl->d_recs32, rec_bytes, hipMemcpyDeviceToHost, c->d2h_stream))) return rc;
    if ((rc = bulk_copy(c, cigar, sl->d_cig, cig_bytes, hipMemcpyDeviceToHost, c->d2h_stream))) return rc;
    if (sl->lens_checked) HIP_TRY(hipMemcpyAsync(sl->h_err, sl->d_err, 4, hipMemcpyDeviceToHost, c->d2h_stream));
    HIP_TRY(hipEventRecord(sl->out_done, c->d2h_stream));
    sl->state = 3;
    c->stream_bytes_out += rec_bytes + cig_bytes;
    return 0;
}

static int stream_map(mcx_ctx *c, int paired, int64_t avg[4], mcx_aln *aln, mcx_aln32 *aln32, uint32_t *cigar, mcx_stats *stats);
extern "C" int mcx_stream_map32(mcx_ctx *c, int paired, int64_t avg[4], mcx_aln32 *aln, uint32_t *cigar, mcx_stats *stats) { return stream_map(c, paired, avg, nullptr, aln, cigar, stats); }
extern "C" int mcx_stream_map(mcx_ctx *c, int paired, int64_t avg[4], mcx_aln *aln, uint32_t *cigar, mcx_stats *stats) { return stream_map(c, paired, avg, aln, nullptr, cigar, stats); }
static int stream_map(mcx_ctx *c, int paired, int64_t avg[4], mcx_aln *aln, mcx_aln32 *aln32, uint32_t *cigar, mcx_stats *stats)
{
    const uint8_t *d_bases; const uint32_t *d_off; mcx_aln *d_aln; uint32_t *d_cig; uint32_t n = 0;
    int rc = mcx_stream_next(c, &d_bases, &d_off, &n, &d_aln, &d_cig);
    if (rc) return rc;
    rc = mcx_map_batch_dev(c, d_bases, d_off, n, paired, avg, d_aln, d_cig, stats);
    mcx_ctx::Slot *sl = oldest_slot(c, 2);
    if (rc == 0 && sl->lens_checked) { // what k_unpack_reads thought of the caller's lengths (a refused batch was mapped as empty reads)
        uint32_t err = 0;
        HIP_TRY(hipMemcpy(&err, sl->d_err, 4, hipMemcpyDeviceToHost));
        if (err) rc = mcx_set_error(MCX_ERR_ARG, (err & 1u) ? "mcx_stream_submit_packed: a read is longer than its row / max_read_len" : "batch holds more bases than max_batch_reads * max_read_len");
    }
    if (rc) { sl->state = 0; return rc; }
    return aln32 ? mcx_stream_mapped32(c, aln32, cigar) : mcx_stream_mapped(c, aln, cigar);
}

extern "C" int mcx_stream_collect(mcx_ctx *c, uint64_t *bytes_in, uint64_t *bytes_out)
{
    if (!c) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_collect: null argument");
    HIP_TRY(hipSetDevice(c->idx->device));
    mcx_ctx::Slot *sl = oldest_slot(c, 3);
    if (!sl) return mcx_set_error(MCX_ERR_ARG, "mcx_stream_collect: no mapped batch is on its way out");
    HIP_TRY(hipEventSynchronize(sl->out_done));
    sl->state = 0;
    c->collected = sl;
    if (bytes_in) *bytes_in = c->stream_bytes_in;
    if (bytes_out) *bytes_out = c->stream_bytes_out;
    if (sl->lens_checked && sl->h_err && *sl->h_err) { // the two-half form (mcx_stream_next + mcx_map_batch_dev / mcx_batch_* + mcx_stream_mapped): the refusal arrives with the records
        const uint32_t err = *sl->h_err;
        *sl->h_err = 0;
        return mcx_set_error(MCX_ERR_ARG, (err & 1u) ? "mcx_stream_submit_packed: a read is longer than its row / max_read_len (the batch was mapped as empty reads)"
                                            : "mcx_stream_submit_packed: the batch holds more bases than max_batch_reads * max_read_len (it was mapped as empty reads)");
    }
    return 0;
}

