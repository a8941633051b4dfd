// mapcaller_amd/csrc/mcx_gz_dev.hip — ordinary gzip streams inflated on the device (mcx_gunzipper_create / _free / _reset, mcx_gunzip_round_dev,
// mcx_gunzip_text_dev, mcx_gz_inflate_dev; the resident route's ordinary .gz files go through mcx_gz_file_*).
//
// Replaces, for ordinary .gz input, pgz::Reader's host threads (mcx_pgz.h); the method and every device function are mcx_gz_dev.h's.
//   k_gz_search    a wavefront per stretch but the first: its block start (find_start), or 0
//   k_gz_inflate   a wavefront per stretch with a start: its symbols behind its prefix in the arena, its record (inflate_stretch)
//   k_gz_windows   ONE workgroup: the chain's windows in sequence, the two in hand in LDS, each written out for the text pass; the last is the next round's
//   k_gz_text      a wavefront per piece of 32 K symbols: bytes at their final offsets, the piece's CRC-32
// Four wavefronts to a workgroup with tables of their own in LDS, as k_inflate has it; what the host needs back is written by one lane with ordinary stores.
// Between inflate and windows the host walks the chain (a few thousand records, one small copy).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/mcx.h"
#include "mcx_gz_dev.h"
#include "mcx_internal.h"

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace {

using namespace mcx::gzd;
enum { kGzWaves = 4, kWinThreads = 512 };

__global__ void __launch_bounds__(64 * kGzWaves) k_gz_search(const uint8_t *__restrict__ src, Geo g, uint64_t *__restrict__ starts)
{
    __shared__ mcx::inf::Tables tabs[kGzWaves];
    const uint32_t lane = threadIdx.x & 63u, w = mcx::inf::uni32(threadIdx.x >> 6);
    const uint32_t i = blockIdx.x * kGzWaves + w;
    if (i >= g.n) return; // (the whole wavefront; nothing below waits for another one)
    uint64_t at = g.start_bit;
    if (i > 0) at = find_start(src, g.src_len, g.readable, (uint64_t)i * g.stretch * 8, (uint64_t)(i + 1) * g.stretch * 8, tabs[w], lane);
    if (lane == 0) starts[i] = at;
}

__global__ void __launch_bounds__(64 * kGzWaves) k_gz_inflate(const uint8_t *__restrict__ src, Geo g, const uint64_t *__restrict__ starts, const uint8_t *__restrict__ win, uint16_t *arena, Rec *__restrict__ recs)
{
    __shared__ mcx::inf::Tables tabs[kGzWaves];
    const uint32_t lane = threadIdx.x & 63u, w = mcx::inf::uni32(threadIdx.x >> 6);
    const uint32_t i = blockIdx.x * kGzWaves + w;
    if (i >= g.n) return;
    const uint64_t from = mcx::inf::uni64(starts[i]);
    if (i > 0 && from == 0) { // no start: the stretch takes no part in the round
        if (lane == 0) { Rec r; r.start_bit = 0; r.stop_bit = 0; r.how = kNone; r.n_syms = 0; recs[i] = r; }
        return;
    }
    inflate_stretch(src, g, i, from, starts, win, arena + (uint64_t)i * g.stride, tabs[w], lane, recs + i);
}

// last_at[k]: where in the arena the kWin symbols begin that end at chain stretch k's end.  win: the window before the round, and behind it on return;
// wins[k * kWin ..): the window before chain stretch k.
__global__ void __launch_bounds__(kWinThreads) k_gz_windows(const uint16_t *__restrict__ arena, const uint64_t *__restrict__ last_at, uint32_t n_chain, uint8_t *win, uint8_t *__restrict__ wins)
{
    __shared__ uint8_t wa[kWin], wb[kWin];
    for (uint32_t j = threadIdx.x; j < kWin; j += kWinThreads) wa[j] = win[j];
    __syncthreads();
    uint8_t *w = wa, *nw = wb;
    for (uint32_t k = 0; k < n_chain; k++) {
        for (uint32_t j = threadIdx.x; j < kWin; j += kWinThreads) wins[(uint64_t)k * kWin + j] = w[j];
        window_step(arena + last_at[k], w, nw, threadIdx.x, kWinThreads);
        __syncthreads();
        uint8_t *t = w; w = nw; nw = t;
    }
    for (uint32_t j = threadIdx.x; j < kWin; j += kWinThreads) win[j] = w[j];
}

__global__ void __launch_bounds__(64 * kGzWaves) k_gz_text(const uint16_t *__restrict__ arena, const Piece *__restrict__ pieces, uint32_t n, const uint8_t *__restrict__ wins, uint8_t *dst, uint32_t *__restrict__ crc)
{
    __shared__ uint32_t crc_tab[256];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) crc_tab[i] = mcx::inf::crc_table_entry(i);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = mcx::inf::uni32(threadIdx.x >> 6);
    const uint32_t i = blockIdx.x * kGzWaves + w;
    if (i >= n) return;
    const Piece p = pieces[i];
    const uint64_t sym_at = mcx::inf::uni64(p.sym_at), dst_at = mcx::inf::uni64(p.dst_at);
    const uint32_t len = mcx::inf::uni32(p.n), win = mcx::inf::uni32(p.win);
    const uint32_t c = text_piece(arena + sym_at, len, wins + (uint64_t)win * kWin, dst + dst_at, crc_tab, lane);
    if (lane == 0) crc[i] = c;
}

} // namespace

struct mcx_gunzipper {
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t stretch = 0, arena_symbols = 0;
    uint32_t max_n = 0, cur_n = 0;
    uint16_t *d_arena = nullptr;
    uint64_t *d_starts = nullptr, *d_last = nullptr, *h_last = nullptr;
    Rec *d_recs = nullptr, *h_recs = nullptr;
    uint8_t *d_win = nullptr, *d_wins = nullptr;
    Piece *d_pieces = nullptr, *h_pieces = nullptr;
    uint32_t *d_crc = nullptr, *h_crc = nullptr;
    uint64_t max_pieces = 0;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    Geo g;
    Chain chain;
    uint32_t win_have = 0;
    int src_is_end = 0;
    bool begun = false;
    uint64_t hbm = 0; // bytes of HBM the object took
};

extern "C" void mcx_gunzipper_free(mcx_gunzipper *z)
{
    if (!z) return;
    (void)hipSetDevice(z->device);
    if (z->stream) (void)hipStreamSynchronize(z->stream);
    void *d[] = {z->d_arena, z->d_starts, z->d_last, z->d_recs, z->d_win, z->d_wins, z->d_pieces, z->d_crc};
    for (void *p : d) if (p) (void)hipFree(p);
    mcx_pinned_free(z->h_last); mcx_pinned_free(z->h_recs); mcx_pinned_free(z->h_pieces); mcx_pinned_free(z->h_crc);
    for (hipEvent_t e : z->ev) if (e) (void)hipEventDestroy(e);
    if (z->stream) (void)hipStreamDestroy(z->stream);
    delete z;
}

extern "C" int mcx_gunzipper_create(int device, uint64_t stretch_bytes, uint32_t max_stretches, uint64_t arena_symbols, mcx_gunzipper **out)
{
    if (!out) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzipper_create: null argument");
    *out = nullptr;
    if (stretch_bytes && stretch_bytes < 4096) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzipper_create: a stretch has at least 4096 bytes");
    const uint64_t stretch = stretch_bytes ? stretch_bytes : 65536;
    const uint32_t max_n = max_stretches ? max_stretches : 2048;
    if (stretch > (1ull << 24) || max_n > (1u << 16) || stretch * ((uint64_t)max_n + 1) > 0x7FFF0000ull) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzipper_create: a round may not hold 2 GB of compressed bytes");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { (void)hipGetLastError(); return mcx_set_error(MCX_ERR_DEVICE, "mcx_gunzipper_create: no such device"); }
    HIP_TRY(hipSetDevice(device));
    mcx_gunzipper *z = new mcx_gunzipper();
    z->device = device; z->stretch = stretch; z->max_n = z->cur_n = max_n;
    z->arena_symbols = arena_symbols ? arena_symbols : 8 * stretch * max_n;
    z->max_pieces = z->arena_symbols / kPiece + max_n + 1;
    memset(&z->g, 0, sizeof z->g);
    const uint64_t arena_bytes = arena_total(z->arena_symbols, max_n) * 2;
    bool ok = hipStreamCreateWithFlags(&z->stream, hipStreamNonBlocking) == hipSuccess;
    for (hipEvent_t &e : z->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && hipMalloc((void **)&z->d_arena, arena_bytes) == hipSuccess && hipMalloc((void **)&z->d_starts, (size_t)max_n * 8) == hipSuccess &&
         hipMalloc((void **)&z->d_last, (size_t)max_n * 8) == hipSuccess && hipMalloc((void **)&z->d_recs, (size_t)max_n * sizeof(Rec)) == hipSuccess &&
         hipMalloc((void **)&z->d_win, kWin) == hipSuccess && hipMalloc((void **)&z->d_wins, (size_t)max_n * kWin) == hipSuccess &&
         hipMalloc((void **)&z->d_pieces, z->max_pieces * sizeof(Piece)) == hipSuccess && hipMalloc((void **)&z->d_crc, z->max_pieces * 4) == hipSuccess;
    if (ok) {
        z->h_last = (uint64_t *)mcx_pinned_alloc((size_t)max_n * 8); z->h_recs = (Rec *)mcx_pinned_alloc((size_t)max_n * sizeof(Rec));
        z->h_pieces = (Piece *)mcx_pinned_alloc(z->max_pieces * sizeof(Piece)); z->h_crc = (uint32_t *)mcx_pinned_alloc(z->max_pieces * 4);
        ok = z->h_last && z->h_recs && z->h_pieces && z->h_crc && hipMemsetAsync(z->d_win, 0, kWin, z->stream) == hipSuccess && hipStreamSynchronize(z->stream) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        mcx_gunzipper_free(z);
        return mcx_set_error(MCX_ERR_DEVICE, "mcx_gunzipper_create: no room for the symbol arena (" + std::to_string(arena_bytes >> 20) + " MB of HBM) and its staging");
    }
    z->hbm = arena_bytes + (uint64_t)max_n * (kWin + 16 + sizeof(Rec)) + kWin + z->max_pieces * (sizeof(Piece) + 4);
    if (getenv("MCX_ALLOC_LOG")) fprintf(stderr, "[mcx alloc] %8.3f GB gunzipper: %u stretches of %llu bytes a round, 2 bytes a symbol of %llu, prefixes and windows\n", (double)z->hbm / 1e9, max_n, (unsigned long long)stretch, (unsigned long long)z->arena_symbols);
    *out = z;
    return 0;
}

extern "C" void mcx_gunzipper_reset(mcx_gunzipper *z)
{
    if (!z) return;
    (void)hipSetDevice(z->device);
    (void)hipMemsetAsync(z->d_win, 0, kWin, z->stream);
    (void)hipStreamSynchronize(z->stream);
    z->win_have = 0; z->cur_n = z->max_n; z->begun = false;
    z->chain.at.clear(); z->chain.pieces.clear(); z->chain.off.assign(1, 0);
}

// mcx_gunzip_round_dev in two halves: begin queues the search, the inflate and the copy of the records and returns at once — the caller stages the next
// round's bytes meanwhile —, end waits, walks the chain and runs the windows
int mcx_gunzip_round_begin(mcx_gunzipper *z, const uint8_t *d_src, uint64_t src_bytes, uint32_t start_bit, int src_is_end)
{
    if (!z || !d_src) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzip_round_dev: null argument");
    if (start_bit > 7 || src_bytes == 0 || src_bytes > 0x7FFFFFF0ull) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzip_round_dev: start_bit is 0 .. 7, src_bytes 1 .. 2 GB");
    if (z->begun) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzip_round_dev: a round is under way");
    HIP_TRY(hipSetDevice(z->device));
    z->g = plan_round(src_bytes, start_bit, z->stretch, z->cur_n, z->arena_symbols, z->win_have);
    z->src_is_end = src_is_end;
    const Geo &g = z->g;
    const uint32_t blocks = (g.n + kGzWaves - 1) / kGzWaves;
    HIP_TRY(hipEventRecord(z->ev[0], z->stream));
    k_gz_search<<<blocks, 64 * kGzWaves, 0, z->stream>>>(d_src, g, z->d_starts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(z->ev[1], z->stream));
    k_gz_inflate<<<blocks, 64 * kGzWaves, 0, z->stream>>>(d_src, g, z->d_starts, z->d_win, z->d_arena, z->d_recs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(z->ev[2], z->stream));
    HIP_TRY(hipMemcpyAsync(z->h_recs, z->d_recs, (size_t)g.n * sizeof(Rec), hipMemcpyDeviceToHost, z->stream));
    z->begun = true;
    return 0;
}

int mcx_gunzip_round_end(mcx_gunzipper *z, mcx_gz_round *info)
{
    if (!z || !info) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzip_round_dev: null argument");
    if (!z->begun) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzip_round_dev: no round is under way");
    z->begun = false;
    memset(info, 0, sizeof *info);
    HIP_TRY(hipSetDevice(z->device));
    HIP_TRY(hipStreamSynchronize(z->stream));
    const Geo &g = z->g;
    walk(g, z->h_recs, z->src_is_end, z->chain, info);
    z->cur_n = next_stretches(g.n, z->max_n, z->chain.room_hit);
    HIP_TRY(hipEventElapsedTime(&info->ms[0], z->ev[0], z->ev[1]));
    HIP_TRY(hipEventElapsedTime(&info->ms[1], z->ev[1], z->ev[2]));
    const uint32_t nc = (uint32_t)z->chain.at.size();
    if (nc) {
        if (z->chain.pieces.size() > z->max_pieces) return mcx_set_error(MCX_ERR_DEVICE, "mcx_gunzip_round_dev: more pieces than the arena can hold");
        for (uint32_t k = 0; k < nc; k++) z->h_last[k] = (uint64_t)z->chain.at[k] * g.stride + z->h_recs[z->chain.at[k]].n_syms;
        HIP_TRY(hipMemcpyAsync(z->d_last, z->h_last, (size_t)nc * 8, hipMemcpyHostToDevice, z->stream));
        HIP_TRY(hipEventRecord(z->ev[3], z->stream));
        k_gz_windows<<<1, kWinThreads, 0, z->stream>>>(z->d_arena, z->d_last, nc, z->d_win, z->d_wins);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(z->ev[4], z->stream));
        HIP_TRY(hipStreamSynchronize(z->stream));
        HIP_TRY(hipEventElapsedTime(&info->ms[2], z->ev[3], z->ev[4]));
        z->win_have = (uint32_t)std::min<uint64_t>((uint64_t)z->win_have + info->text_bytes, kWin);
    }
    if (info->status == MCX_GZ_CAPACITY)
        (void)mcx_set_error(MCX_ERR_CAPACITY, "mcx_gunzip_round_dev: one stretch of " + std::to_string(z->stretch) + " compressed bytes makes more than the arena's " + std::to_string(z->arena_symbols) + " symbols: create the gunzipper with more arena_symbols");
    return 0;
}

extern "C" int mcx_gunzip_round_dev(mcx_gunzipper *z, const uint8_t *d_src, uint64_t src_bytes, uint32_t start_bit, int src_is_end, mcx_gz_round *info)
{
    if (!info) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzip_round_dev: null argument");
    if (int rc = mcx_gunzip_round_begin(z, d_src, src_bytes, start_bit, src_is_end)) return rc;
    return mcx_gunzip_round_end(z, info);
}

extern "C" int mcx_gunzip_text_dev(mcx_gunzipper *z, uint8_t *d_dst, uint64_t dst_cap, mcx_gz_round *info)
{
    if (!z || !info) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzip_text_dev: null argument");
    if (z->begun) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzip_text_dev: a round is under way");
    if (info->text_bytes != z->chain.off.back()) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzip_text_dev: info is not the last round's");
    info->crc32 = 0; info->ms[3] = 0;
    const uint32_t np = (uint32_t)z->chain.pieces.size();
    if (np == 0) return 0;
    if (!d_dst) return mcx_set_error(MCX_ERR_ARG, "mcx_gunzip_text_dev: null argument");
    if (dst_cap < info->text_bytes) return mcx_set_error(MCX_ERR_CAPACITY, "mcx_gunzip_text_dev: the round's text is " + std::to_string(info->text_bytes) + " bytes, dst_cap " + std::to_string(dst_cap));
    HIP_TRY(hipSetDevice(z->device));
    memcpy(z->h_pieces, z->chain.pieces.data(), (size_t)np * sizeof(Piece));
    HIP_TRY(hipMemcpyAsync(z->d_pieces, z->h_pieces, (size_t)np * sizeof(Piece), hipMemcpyHostToDevice, z->stream));
    HIP_TRY(hipEventRecord(z->ev[5], z->stream));
    k_gz_text<<<(np + kGzWaves - 1) / kGzWaves, 64 * kGzWaves, 0, z->stream>>>(z->d_arena, z->d_pieces, np, z->d_wins, d_dst, z->d_crc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(z->ev[6], z->stream));
    HIP_TRY(hipMemcpyAsync(z->h_crc, z->d_crc, (size_t)np * 4, hipMemcpyDeviceToHost, z->stream));
    HIP_TRY(hipStreamSynchronize(z->stream));
    HIP_TRY(hipEventElapsedTime(&info->ms[3], z->ev[5], z->ev[6]));
    info->crc32 = combine(z->chain, z->h_crc);
    return 0;
}

// ---- a file: the one walker (mcx_gz_dev.h's Reader) over an engine that stages a round's bytes through page-locked memory ----
namespace {

struct Staged { // a set of staging buffers: file bytes [from, from + bytes) lie at d[0 .. bytes), 8 zero bytes behind them
    uint8_t *h = nullptr, *d = nullptr;
    uint64_t cap = 0, bytes = 0;
    const uint8_t *from = nullptr;
    hipEvent_t ready = nullptr;
};

struct Engine {
    mcx_gunzipper *z = nullptr;
    hipStream_t copy = nullptr;
    Staged set[2];
    int cur = 0;
    uint64_t rounds = 0, staged_hits = 0; // rounds begun; those whose bytes stage() had brought already

    int fill(Staged &s, const uint8_t *src, uint64_t bytes, hipStream_t on)
    {
        if (bytes + 8 > s.cap) {
            (void)hipStreamSynchronize(copy);
            mcx_pinned_free(s.h); if (s.d) (void)hipFree(s.d);
            s.h = nullptr; s.d = nullptr; s.cap = 0;
            const uint64_t cap = bytes + bytes / 8 + 4096;
            s.h = (uint8_t *)mcx_pinned_alloc(cap);
            if (!s.h || hipMalloc((void **)&s.d, cap) != hipSuccess) { (void)hipGetLastError(); mcx_pinned_free(s.h); s.h = nullptr; s.d = nullptr; return mcx_set_error(MCX_ERR_DEVICE, "-gpu_gz: no room for a round's compressed bytes (" + std::to_string(cap >> 20) + " MB, host and HBM)"); }
            s.cap = cap;
            if (getenv("MCX_ALLOC_LOG")) fprintf(stderr, "[mcx alloc] %8.3f GB gunzipper: a round's compressed bytes (one of two staging twins)\n", (double)cap / 1e9);
        }
        memcpy(s.h, src, bytes);
        memset(s.h + bytes, 0, 8);
        s.from = src; s.bytes = bytes;
        HIP_TRY(hipMemcpyAsync(s.d, s.h, bytes + 8, hipMemcpyHostToDevice, on));
        HIP_TRY(hipEventRecord(s.ready, on));
        return 0;
    }
    int begin(const uint8_t *src, uint64_t bytes, uint32_t start_bit, int is_end)
    {
        HIP_TRY(hipSetDevice(z->device));
        const Staged &o = set[cur ^ 1]; // what stage() brought while the last round ran
        rounds++;
        if (o.from && src >= o.from && src + bytes <= o.from + o.bytes) { cur ^= 1; staged_hits++; }
        else if (int rc = fill(set[cur], src, bytes, z->stream)) return rc;
        Staged &s = set[cur];
        HIP_TRY(hipStreamWaitEvent(z->stream, s.ready, 0));
        return mcx_gunzip_round_begin(z, s.d + (src - s.from), bytes, start_bit, is_end);
    }
    void stage(const uint8_t *src, uint64_t bytes)
    {
        Staged &s = set[cur ^ 1];
        s.from = nullptr;
        if (fill(s, src, bytes, copy) != 0) s.from = nullptr; // (the round then stages its bytes itself, and says what is wrong)
    }
    int end(mcx_gz_round *info) { return mcx_gunzip_round_end(z, info); }
    uint32_t stretches() const { return z->cur_n; }
    uint64_t stretch_bytes() const { return z->stretch; }
    void reset() { mcx_gunzipper_reset(z); }
};

} // namespace

struct mcx_gz_file {
    Engine e;
    Reader<Engine> *rd = nullptr;
    uint64_t delivered = 0;
};

void mcx_gz_file_free(mcx_gz_file *f)
{
    if (!f) return;
    delete f->rd;
    if (f->e.z) (void)hipSetDevice(f->e.z->device);
    if (f->e.copy) { (void)hipStreamSynchronize(f->e.copy); }
    if (f->e.z) mcx_gunzipper_free(f->e.z);
    for (Staged &s : f->e.set) { mcx_pinned_free(s.h); if (s.d) (void)hipFree(s.d); if (s.ready) (void)hipEventDestroy(s.ready); }
    if (f->e.copy) (void)hipStreamDestroy(f->e.copy);
    delete f;
}

// data[0 .. size): the whole file, which outlives the object.  *out stays null (and the call returns 0) when the file does not begin with a gzip header.
int mcx_gz_file_open(int device, const uint8_t *data, size_t size, uint64_t stretch_bytes, uint32_t round_stretches, mcx_gz_file **out)
{
    *out = nullptr;
    if (!gzip_header(data, size)) return 0;
    mcx_gz_file *f = new mcx_gz_file();
    int rc = mcx_gunzipper_create(device, stretch_bytes, round_stretches, 0, &f->e.z);
    if (rc == 0 && (hipStreamCreateWithFlags(&f->e.copy, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&f->e.set[0].ready, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&f->e.set[1].ready, hipEventDisableTiming) != hipSuccess)) { (void)hipGetLastError(); rc = mcx_set_error(MCX_ERR_DEVICE, "-gpu_gz: no stream on the device"); }
    if (rc) { mcx_gz_file_free(f); return rc; }
    f->rd = new Reader<Engine>(f->e, data, size);
    f->rd->open();
    *out = f;
    return 0;
}
// the next round: 1 — info->text_bytes of text wait to be fetched by mcx_gz_file_text (0 bytes is possible) —, 0 at the input's end, or an error
int mcx_gz_file_next(mcx_gz_file *f, mcx_gz_round *info) { return f->rd->next(info); }
// ... into d_dst; *counts: the text is part of the file's (false: the member's trailer does not match — the input ends here and nothing of the round is handed on)
int mcx_gz_file_text(mcx_gz_file *f, uint8_t *d_dst, uint64_t dst_cap, mcx_gz_round *info, bool *counts)
{
    *counts = false;
    if (int rc = mcx_gunzip_text_dev(f->e.z, d_dst, dst_cap, info)) return rc;
    *counts = f->rd->commit(info);
    if (*counts) f->delivered += info->text_bytes;
    return 0;
}
bool mcx_gz_file_failed(const mcx_gz_file *f) { return f->rd->failed(); }
uint64_t mcx_gz_file_delivered(const mcx_gz_file *f) { return f->delivered; }
void mcx_gz_file_staging(const mcx_gz_file *f, uint64_t *rounds, uint64_t *staged_hits) { *rounds = f->e.rounds; *staged_hits = f->e.staged_hits; }

static thread_local uint64_t last_staging[2] = {0, 0};
extern "C" void mcx_gz_inflate_dev_last(uint64_t stats[2]) { if (stats) { stats[0] = last_staging[0]; stats[1] = last_staging[1]; } }

extern "C" int64_t mcx_gz_inflate_dev(const char *path, int device, uint64_t stretch_bytes, uint32_t round_stretches, uint8_t *out, uint64_t cap, uint64_t *n_out)
{
    if (n_out) *n_out = 0;
    last_staging[0] = last_staging[1] = 0;
    if (!path) return -1;
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return -1;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 18) { close(fd); return -1; }
    void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return -1;
    mcx_gz_file *f = nullptr;
    int64_t ret = -1;
    uint8_t *d_text = nullptr;
    uint64_t d_cap = 0, total = 0;
    if (mcx_gz_file_open(device, (const uint8_t *)m, (size_t)st.st_size, stretch_bytes, round_stretches, &f) == 0 && f) {
        bool bad = false;
        for (;;) {
            mcx_gz_round info;
            const int r = mcx_gz_file_next(f, &info);
            if (r < 0) { bad = true; break; }
            if (r == 0) break;
            if (info.text_bytes > d_cap) {
                if (d_text) (void)hipFree(d_text);
                d_text = nullptr; d_cap = info.text_bytes + info.text_bytes / 4 + 4096;
                if (hipMalloc((void **)&d_text, d_cap) != hipSuccess) { (void)hipGetLastError(); d_text = nullptr; d_cap = 0; bad = true; break; }
            }
            bool counts = false;
            if (mcx_gz_file_text(f, d_text, d_cap, &info, &counts) != 0) { bad = true; break; }
            if (!counts) break;
            if (out && total < cap && info.text_bytes) {
                const uint64_t k = std::min<uint64_t>(info.text_bytes, cap - total);
                if (hipMemcpy(out + total, d_text, k, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); bad = true; break; }
            }
            total += info.text_bytes;
        }
        if (n_out) *n_out = total;
        ret = bad || mcx_gz_file_failed(f) ? -2 : (int64_t)total;
        mcx_gz_file_staging(f, &last_staging[0], &last_staging[1]);
    }
    if (d_text) (void)hipFree(d_text);
    mcx_gz_file_free(f);
    munmap(m, (size_t)st.st_size);
    return ret;
}
