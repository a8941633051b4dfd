// mapcaller_amd/csrc/mcx_deflate.hip — text compressed to BGZF blocks on the device (mcx_deflater_create / _free / _set_block, mcx_bgzf_bound, mcx_bgzf_deflate_dev,
// mcx_bgzf_deflate, mcx_bgzf_eof; the file front end's -bgzf goes through mcx_bgzf_deflate_dev from mcx_sam.hip).
//
// The twin of mcx_inflate.hip.  The text is worked through in launches of a fixed amount (kLaunchText), so the scratch is bounded:
//   k_deflate   one wavefront per block of text (mcx_deflate.h's deflate_block): two blocks to a workgroup, each with a Work of its own in LDS (14.3 KB) and the
//               CRC-32 byte table shared — 29.5 KB a workgroup, five workgroups (ten wavefronts) to a CU's 160 KB.  The raw deflate stream goes to the block's
//               slot in the scratch, its size and the text's CRC-32 to the block's Meta
//   k_places    one workgroup: the prefix sum of the member sizes behind the bytes the earlier launches of the call made (a running total in HBM: no launch waits
//               for the host)
//   k_gather    a workgroup per block: header, stream, CRC-32 and ISIZE to their final place in the caller's buffer — complete, contiguous BGZF blocks in text order
// The object owns a non-blocking stream, the scratch (made on first use, sized by the text it has seen: at most kLaunchText and its slots) and, for the host
// form, page-locked staging and its twins in HBM.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/mcx.h"
#include "mcx_deflate.h"
#include "mcx_internal.h"

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace {

enum { kDefWaves = 2 };                                   // wavefronts (blocks of text) per workgroup
const uint64_t kLaunchText = 128ull << 20;                // bytes of text one launch takes at most ...
const uint64_t kLaunchBlocks = 65536;                     // ... and blocks (small block sizes)

struct Meta { uint32_t payload, crc; uint64_t at; };      // a block's stream bytes, its text's CRC-32, and where its member begins in the output

__global__ void __launch_bounds__(64 * kDefWaves) k_deflate(const uint8_t *__restrict__ text, uint64_t text_bytes, uint32_t block, uint32_t n_blocks, uint8_t *__restrict__ slots,
                                                            uint32_t slot_bytes, Meta *__restrict__ meta)
{
    __shared__ mcx::def::Work work[kDefWaves];
    __shared__ uint32_t crc_tab[256];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) crc_tab[i] = mcx::inf::crc_table_entry(i);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = mcx::inf::uni32(threadIdx.x >> 6);
    const uint32_t i = blockIdx.x * kDefWaves + w;
    if (i >= n_blocks) return; // (the whole wavefront; nothing below waits for another one)
    const uint64_t at = (uint64_t)i * block;
    const uint32_t n = (uint32_t)(text_bytes - at < block ? text_bytes - at : block); // (the host made n_blocks = ceil(text_bytes / block): n >= 1)
    uint32_t crc = 0;
    const uint32_t payload = mcx::def::deflate_block(text + at, n, slots + (uint64_t)i * slot_bytes, slot_bytes, work[w], crc_tab, lane, &crc);
    if (lane == 0) { meta[i].payload = payload; meta[i].crc = crc; }
}

// meta[i].at = *total + the sizes of the members before i; *total += all of them.  block_at (may be null): the same places, kept for the whole call —
// entry i of this launch's part, and behind the launch's last block the new total (the next launch begins there and writes the same value)
__global__ void __launch_bounds__(1024) k_places(Meta *__restrict__ meta, uint32_t n_blocks, uint64_t *__restrict__ total, uint64_t *__restrict__ block_at)
{
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x, per = (n_blocks + 1023) / 1024;
    const uint32_t lo = t * per < n_blocks ? t * per : n_blocks, hi = lo + per < n_blocks ? lo + per : n_blocks;
    uint64_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += meta[i].payload + mcx::def::kMemberExtra;
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) { // (an inclusive scan of the 1024 partial sums)
        const uint64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t at = *total + part[t] - sum;
    for (uint32_t i = lo; i < hi; i++) { meta[i].at = at; if (block_at) block_at[i] = at; at += meta[i].payload + mcx::def::kMemberExtra; }
    __syncthreads(); // (every thread has read *total)
    if (t == 1023) { if (block_at) block_at[n_blocks] = at; *total += part[1023]; }
}

__global__ void __launch_bounds__(256) k_gather(const uint8_t *__restrict__ slots, uint32_t slot_bytes, const Meta *__restrict__ meta, uint32_t n_blocks, uint32_t block, uint64_t text_bytes,
                                                uint8_t *__restrict__ out, uint64_t out_cap)
{
    const uint32_t i = blockIdx.x;
    if (i >= n_blocks) return;
    const Meta m = meta[i];
    const uint64_t text_at = (uint64_t)i * block;
    const uint32_t isize = (uint32_t)(text_bytes - text_at < block ? text_bytes - text_at : block);
    const uint32_t payload = m.payload < slot_bytes ? m.payload : slot_bytes, member = payload + mcx::def::kMemberExtra;
    if (m.at > out_cap || member > out_cap - m.at) return; // (the host checked out_cap against mcx_bgzf_bound: never)
    const uint8_t *stream = slots + (uint64_t)i * slot_bytes;
    uint8_t *dst = out + m.at;
    for (uint32_t k = threadIdx.x; k < member; k += blockDim.x) dst[k] = mcx::def::member_byte(k, stream, payload, m.crc, isize);
}

} // namespace

struct mcx_deflater {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t block = mcx::def::kMaxBlock;
    uint64_t max_text = 0;                                 // per launch of the host form
    uint8_t *d_slots = nullptr; uint64_t cap_slots = 0;    // the scratch: a slot per block of a launch
    Meta *d_meta = nullptr; uint64_t cap_meta = 0;
    uint64_t *d_block_at = nullptr; uint64_t cap_block_at = 0, n_block_at = 0; // where the blocks of the last mcx_bgzf_deflate_dev begin, over all its launches
    uint64_t *d_total = nullptr, *h_total = nullptr;
    uint8_t *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr; uint64_t cap_in = 0, cap_out = 0; // the host form's staging
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms = 0;
};

namespace {

uint64_t blocks_of(uint64_t text_bytes, uint32_t block) { return (text_bytes + block - 1) / block; }

int grow_dev(mcx_deflater *f, void **p, uint64_t *cap, uint64_t want, const char *what)
{
    if (want <= *cap) return 0;
    if (*p) { (void)hipStreamSynchronize(f->stream); (void)hipFree(*p); *p = nullptr; *cap = 0; }
    if (hipMalloc(p, want) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return mcx_set_error(MCX_ERR_DEVICE, std::string("mcx_bgzf_deflate: no room in HBM for ") + what); }
    *cap = want;
    return 0;
}

// the launches of one call: text in HBM to blocks in HBM, *f->d_total the bytes made; nothing is waited for.  keep_places: the blocks' places stay in
// f->d_block_at for mcx_bgzf_deflate_blocks (d_meta is a launch's and overwritten by the next)
int queue(mcx_deflater *f, const uint8_t *d_text, uint64_t text_bytes, uint8_t *d_out, uint64_t out_cap, bool keep_places)
{
    const uint32_t block = f->block, slot_bytes = mcx::def::slot_bytes_of(block);
    const uint64_t per_launch = std::max<uint64_t>(1, std::min<uint64_t>(kLaunchText / block, kLaunchBlocks));
    const uint64_t most = std::min<uint64_t>(per_launch, blocks_of(text_bytes, block));
    if (int rc = grow_dev(f, (void **)&f->d_slots, &f->cap_slots, most * slot_bytes, "the blocks' slots")) return rc;
    uint64_t meta_bytes = f->cap_meta * sizeof(Meta);
    if (int rc = grow_dev(f, (void **)&f->d_meta, &meta_bytes, most * sizeof(Meta), "the blocks' sizes")) return rc;
    f->cap_meta = meta_bytes / sizeof(Meta);
    if (keep_places) {
        f->n_block_at = 0;
        uint64_t at_bytes = f->cap_block_at * 8;
        if (int rc = grow_dev(f, (void **)&f->d_block_at, &at_bytes, (blocks_of(text_bytes, block) + 1) * 8, "the blocks' places")) { f->cap_block_at = 0; return rc; }
        f->cap_block_at = at_bytes / 8;
        f->n_block_at = blocks_of(text_bytes, block);
    }
    HIP_TRY(hipMemsetAsync(f->d_total, 0, 8, f->stream));
    for (uint64_t at = 0; at < text_bytes; at += per_launch * block) {
        const uint64_t bytes = std::min<uint64_t>(text_bytes - at, per_launch * block);
        const uint32_t n = (uint32_t)blocks_of(bytes, block);
        k_deflate<<<(n + kDefWaves - 1) / kDefWaves, 64 * kDefWaves, 0, f->stream>>>(d_text + at, bytes, block, n, f->d_slots, slot_bytes, f->d_meta);
        k_places<<<1, 1024, 0, f->stream>>>(f->d_meta, n, f->d_total, keep_places ? f->d_block_at + at / block : nullptr);
        k_gather<<<n, 256, 0, f->stream>>>(f->d_slots, slot_bytes, f->d_meta, n, block, bytes, d_out, out_cap);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

} // namespace

extern "C" void mcx_deflater_free(mcx_deflater *f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    void *d[] = {f->d_slots, f->d_meta, f->d_block_at, f->d_total, f->d_in, f->d_out};
    for (void *p : d) if (p) (void)hipFree(p);
    mcx_pinned_free(f->h_total); mcx_pinned_free(f->h_in); mcx_pinned_free(f->h_out);
    for (hipEvent_t e : f->ev) if (e) (void)hipEventDestroy(e);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

extern "C" int mcx_deflater_create(int device, uint64_t max_text_bytes, mcx_deflater **out)
{
    if (!out) return mcx_set_error(MCX_ERR_ARG, "mcx_deflater_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { (void)hipGetLastError(); return mcx_set_error(MCX_ERR_DEVICE, "mcx_deflater_create: no such device"); }
    HIP_TRY(hipSetDevice(device));
    mcx_deflater *f = new mcx_deflater();
    f->device = device;
    f->max_text = max_text_bytes ? max_text_bytes : 8ull << 20;
    int rc = 0;
    if (hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess) rc = MCX_ERR_DEVICE;
    for (hipEvent_t &e : f->ev) if (rc == 0 && hipEventCreate(&e) != hipSuccess) rc = MCX_ERR_DEVICE;
    if (rc == 0 && hipMalloc((void **)&f->d_total, 8) != hipSuccess) rc = MCX_ERR_DEVICE;
    if (rc == 0 && !(f->h_total = (uint64_t *)mcx_pinned_alloc(8))) rc = MCX_ERR_DEVICE;
    if (rc) { (void)hipGetLastError(); mcx_deflater_free(f); return mcx_set_error(MCX_ERR_DEVICE, "mcx_deflater_create: cannot set the object up on the device"); }
    *out = f;
    return 0;
}

extern "C" int mcx_deflater_set_block(mcx_deflater *f, uint32_t text_bytes)
{
    if (!f) return mcx_set_error(MCX_ERR_ARG, "mcx_deflater_set_block: null argument");
    if (text_bytes < 1 || text_bytes > mcx::def::kMaxBlock) return mcx_set_error(MCX_ERR_ARG, "mcx_deflater_set_block: a BGZF block takes 1 to 65280 bytes of text");
    f->block = text_bytes;
    return 0;
}

extern "C" uint64_t mcx_bgzf_bound(uint64_t text_bytes, uint32_t block_text_bytes)
{
    const uint32_t block = block_text_bytes >= 1 && block_text_bytes <= mcx::def::kMaxBlock ? block_text_bytes : (uint32_t)mcx::def::kMaxBlock;
    return text_bytes + blocks_of(text_bytes, block) * (mcx::def::kMemberExtra + mcx::def::kStoredExtra); // (every block stored)
}

extern "C" int mcx_bgzf_eof(uint8_t out[28])
{
    if (!out) return mcx_set_error(MCX_ERR_ARG, "mcx_bgzf_eof: null argument");
    const uint8_t empty[2] = {3, 0}; // (a fixed block that holds the end-of-block code alone: what bgzip ends a file with)
    for (uint32_t i = 0; i < 28; i++) out[i] = mcx::def::member_byte(i, empty, 2, 0, 0);
    return 0;
}

extern "C" int mcx_bgzf_deflate_dev(mcx_deflater *f, const uint8_t *d_text, uint64_t text_bytes, uint8_t *d_out, uint64_t out_cap, uint64_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!f || !n_out) return mcx_set_error(MCX_ERR_ARG, "mcx_bgzf_deflate_dev: null argument");
    f->n_block_at = 0;
    if (text_bytes == 0) return 0;
    if (!d_text || !d_out) return mcx_set_error(MCX_ERR_ARG, "mcx_bgzf_deflate_dev: null argument");
    if (out_cap < mcx_bgzf_bound(text_bytes, f->block))
        return mcx_set_error(MCX_ERR_CAPACITY, "mcx_bgzf_deflate_dev: the blocks of " + std::to_string(text_bytes) + " bytes of text can take " + std::to_string(mcx_bgzf_bound(text_bytes, f->block)) + " bytes");
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(hipEventRecord(f->ev[0], f->stream));
    if (int rc = queue(f, d_text, text_bytes, d_out, out_cap, true)) return rc;
    HIP_TRY(hipEventRecord(f->ev[1], f->stream));
    HIP_TRY(hipMemcpyAsync(f->h_total, f->d_total, 8, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    HIP_TRY(hipEventElapsedTime(&f->last_ms, f->ev[0], f->ev[1]));
    *n_out = *f->h_total;
    return 0;
}

extern "C" int mcx_bgzf_deflate_blocks(mcx_deflater *f, const uint64_t **d_block_at, uint64_t *n_blocks)
{
    if (!f || !d_block_at || !n_blocks) return mcx_set_error(MCX_ERR_ARG, "mcx_bgzf_deflate_blocks: null argument");
    *n_blocks = f->n_block_at;
    *d_block_at = f->n_block_at ? f->d_block_at : nullptr;
    return 0;
}

// the last mcx_bgzf_deflate_dev's kernels in ms, by events on the deflater's stream (scripts/deflate_rate.py)
extern "C" int mcx_bgzf_deflate_last_ms(mcx_deflater *f, float *ms)
{
    if (!f || !ms) return mcx_set_error(MCX_ERR_ARG, "mcx_bgzf_deflate_last_ms: null argument");
    *ms = f->last_ms;
    return 0;
}

extern "C" int mcx_bgzf_deflate(mcx_deflater *f, const uint8_t *text, uint64_t text_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!f || !n_out) return mcx_set_error(MCX_ERR_ARG, "mcx_bgzf_deflate: null argument");
    if (text_bytes == 0) return 0;
    if (!text || !out) return mcx_set_error(MCX_ERR_ARG, "mcx_bgzf_deflate: null argument");
    if (out_cap < mcx_bgzf_bound(text_bytes, f->block))
        return mcx_set_error(MCX_ERR_CAPACITY, "mcx_bgzf_deflate: the blocks of " + std::to_string(text_bytes) + " bytes of text can take " + std::to_string(mcx_bgzf_bound(text_bytes, f->block)) + " bytes");
    HIP_TRY(hipSetDevice(f->device));
    // a launch of the host form: whole blocks, max_text bytes at most (one block at least)
    const uint64_t step = std::max<uint64_t>(1, f->max_text / f->block) * f->block, first = std::min(step, text_bytes), bound = mcx_bgzf_bound(first, f->block);
    if (first > f->cap_in || bound > f->cap_out) {
        (void)hipStreamSynchronize(f->stream);
        mcx_pinned_free(f->h_in); mcx_pinned_free(f->h_out); f->h_in = f->h_out = nullptr;
        if (f->d_in) (void)hipFree(f->d_in);
        if (f->d_out) (void)hipFree(f->d_out);
        f->d_in = f->d_out = nullptr; f->cap_in = f->cap_out = 0;
        f->h_in = (uint8_t *)mcx_pinned_alloc(first); f->h_out = (uint8_t *)mcx_pinned_alloc(bound);
        if (!f->h_in || !f->h_out || hipMalloc((void **)&f->d_in, first) != hipSuccess || hipMalloc((void **)&f->d_out, bound) != hipSuccess) {
            (void)hipGetLastError();
            return mcx_set_error(MCX_ERR_DEVICE, "mcx_bgzf_deflate: no room for the staging buffers (host or HBM)");
        }
        f->cap_in = first; f->cap_out = bound;
    }
    uint64_t made = 0;
    for (uint64_t at = 0; at < text_bytes; at += step) {
        const uint64_t bytes = std::min(step, text_bytes - at);
        memcpy(f->h_in, text + at, bytes);
        HIP_TRY(hipMemcpyAsync(f->d_in, f->h_in, bytes, hipMemcpyHostToDevice, f->stream));
        if (int rc = queue(f, f->d_in, bytes, f->d_out, f->cap_out, false)) return rc;
        HIP_TRY(hipMemcpyAsync(f->h_total, f->d_total, 8, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        const uint64_t got = *f->h_total;
        if (got > f->cap_out || got > out_cap - made) return mcx_set_error(MCX_ERR_DEVICE, "mcx_bgzf_deflate: the blocks are larger than their bound");
        HIP_TRY(hipMemcpyAsync(f->h_out, f->d_out, got, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        memcpy(out + made, f->h_out, got);
        made += got;
    }
    *n_out = made;
    return 0;
}
