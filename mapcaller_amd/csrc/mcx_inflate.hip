// mapcaller_amd/csrc/mcx_inflate.hip — BGZF members inflated on the device (mcx_inflater_create / _free, mcx_inflate_dev, mcx_inflate; the file front
// end's -gpu_inflate goes through mcx_inflate_begin / mcx_inflate_end).
//
// Replaces, for BGZF input, the zlib calls of the reader's thread pool (Parser::feed_bgzf, mcx_files.cpp): inflate + crc32 per member.
//   k_inflate   one wavefront per member (mcx_inflate.h's inflate_member): four members to a workgroup, each with tables of its own in LDS and the
//               CRC-32 byte table shared; the member's status word written by lane 0
// The object owns a non-blocking stream and two sets of staging buffers (page-locked on the host, their twins in HBM): while one set's members are on
// the device the next set is filled by the host.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcx.h"
#include "mcx_inflate.h"
#include "mcx_internal.h"

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace {

enum { kInfWaves = 4 }; // wavefronts (members) per workgroup

__global__ void __launch_bounds__(64 * kInfWaves) k_inflate(const uint8_t *__restrict__ src, uint64_t src_bytes, const mcx_deflate_member *__restrict__ members, uint32_t n,
                                                            uint8_t *dst, uint32_t *__restrict__ status)
{
    __shared__ mcx::inf::Tables tabs[kInfWaves];
    __shared__ uint32_t crc_tab[256];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) crc_tab[i] = mcx::inf::crc_table_entry(i);
    __syncthreads();
    // (the wavefront's number and its member are the same in every lane; said so, the decoder's state lives in scalar registers)
    const uint32_t lane = threadIdx.x & 63u, w = mcx::inf::uni32(threadIdx.x >> 6);
    const uint32_t i = blockIdx.x * kInfWaves + w;
    if (i >= n) return; // (the whole wavefront; nothing below waits for another one)
    const mcx_deflate_member m = members[i];
    const uint64_t src_off = mcx::inf::uni64(m.src_off), dst_off = mcx::inf::uni64(m.dst_off);
    const uint32_t src_len = mcx::inf::uni32(m.src_len), isize = mcx::inf::uni32(m.isize), crc = mcx::inf::uni32(m.crc32);
    const uint64_t rest = src_bytes - src_off; // (the host checked: the member lies inside src_bytes)
    const uint32_t readable = rest > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)rest;
    const uint32_t st = mcx::inf::inflate_member(src + src_off, src_len, readable, dst + dst_off, isize, crc, tabs[w], crc_tab, lane, nullptr);
    if (lane == 0) status[i] = st;
}

struct Set { // one set of staging buffers: what one launch of the host form takes
    uint8_t *h_src = nullptr, *h_dst = nullptr, *d_src = nullptr, *d_dst = nullptr;
    mcx_deflate_member *h_mem = nullptr, *d_mem = nullptr;
    uint32_t *h_status = nullptr, *d_status = nullptr;
    hipEvent_t done = nullptr;
    std::vector<uint64_t> dst_off; // where the caller wants each member's text
    uint32_t n = 0;
    uint64_t dst_bytes = 0;
    bool busy = false;
    bool to_dev = false; // the text went to the caller's buffer in HBM (mcx_inflate_begin_dev): none to hand out
};

} // namespace

struct mcx_inflater {
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t max_src = 0, max_dst = 0;
    uint32_t max_members = 0;
    bool text_bufs = true; // the sets hold buffers for the text (h_dst, d_dst); false: an inflater of the resident route, whose text stays in the caller's HBM
    Set set[2];
    uint32_t next = 0, oldest = 0; // the set the next mcx_inflate_begin fills; the one the next mcx_inflate_end waits for
    mcx_deflate_member *h_check = nullptr; uint32_t *h_check_status = nullptr; // mcx_inflate_dev: the caller's members and status words, looked at by the host
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms = 0; // the last launch of mcx_inflate_dev, by the events around it
};

namespace {

int launch(mcx_inflater *f, const uint8_t *d_src, uint64_t src_bytes, const mcx_deflate_member *d_mem, uint32_t n, uint8_t *d_dst, uint32_t *d_status)
{
    k_inflate<<<(n + kInfWaves - 1) / kInfWaves, 64 * kInfWaves, 0, f->stream>>>(d_src, src_bytes, d_mem, n, d_dst, d_status);
    HIP_TRY(hipGetLastError());
    return 0;
}

// what every member must satisfy before anything is launched
const char *member_fault(const mcx_deflate_member &m, uint64_t src_bytes, uint64_t dst_cap)
{
    if (m.isize > 65536) return "a member's isize is larger than 65536";
    if (m.src_off > src_bytes || m.src_len > src_bytes - m.src_off) return "a member lies outside src_bytes";
    if (m.dst_off > dst_cap || m.isize > dst_cap - m.dst_off) return "a member's text lies outside dst_cap";
    return nullptr;
}

} // namespace

extern "C" void mcx_inflater_free(mcx_inflater *f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    for (Set &s : f->set) {
        mcx_pinned_free(s.h_src); mcx_pinned_free(s.h_dst); mcx_pinned_free(s.h_mem); mcx_pinned_free(s.h_status);
        void *d[] = {s.d_src, s.d_dst, s.d_mem, s.d_status};
        for (void *p : d) if (p) (void)hipFree(p);
        if (s.done) (void)hipEventDestroy(s.done);
    }
    mcx_pinned_free(f->h_check); mcx_pinned_free(f->h_check_status);
    for (hipEvent_t e : f->ev) if (e) (void)hipEventDestroy(e);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

static int create(int device, uint64_t max_src_bytes, uint64_t max_dst_bytes, uint32_t max_members, bool text_bufs, mcx_inflater **out);
extern "C" int mcx_inflater_create(int device, uint64_t max_src_bytes, uint64_t max_dst_bytes, uint32_t max_members, mcx_inflater **out)
{
    return create(device, max_src_bytes, max_dst_bytes, max_members, true, out);
}
// an inflater whose launches leave their text in the caller's HBM (mcx_inflate_begin_dev): staging for the compressed bytes, the members and the status words only
int mcx_inflater_create_dev(int device, uint64_t max_src_bytes, uint32_t max_members, mcx_inflater **out)
{
    return create(device, max_src_bytes, 65536, max_members, false, out);
}
static int create(int device, uint64_t max_src_bytes, uint64_t max_dst_bytes, uint32_t max_members, bool text_bufs, mcx_inflater **out)
{
    if (!out) return mcx_set_error(MCX_ERR_ARG, "mcx_inflater_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { (void)hipGetLastError(); return mcx_set_error(MCX_ERR_DEVICE, "mcx_inflater_create: no such device"); }
    HIP_TRY(hipSetDevice(device));
    mcx_inflater *f = new mcx_inflater();
    f->device = device; f->text_bufs = text_bufs;
    // (a launch holds at least one member of the largest kind: 64 KB of text, and compressed bytes that did not shrink)
    f->max_dst = max_dst_bytes ? std::max<uint64_t>(max_dst_bytes, 65536) : (8ull << 20) + 65536;
    f->max_src = max_src_bytes ? std::max<uint64_t>(max_src_bytes, 65536 + 1024) : f->max_dst + f->max_dst / 64 + 4096;
    f->max_members = max_members ? max_members : 16384;
    int rc = 0;
    if (hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess) rc = MCX_ERR_DEVICE;
    for (hipEvent_t &e : f->ev) if (rc == 0 && hipEventCreate(&e) != hipSuccess) rc = MCX_ERR_DEVICE;
    for (Set &s : f->set) {
        if (rc) break;
        s.h_src = (uint8_t *)mcx_pinned_alloc(f->max_src + 8); s.h_dst = text_bufs ? (uint8_t *)mcx_pinned_alloc(f->max_dst) : nullptr;
        s.h_mem = (mcx_deflate_member *)mcx_pinned_alloc((size_t)f->max_members * sizeof(mcx_deflate_member));
        s.h_status = (uint32_t *)mcx_pinned_alloc((size_t)f->max_members * 4);
        if (!s.h_src || (text_bufs && !s.h_dst) || !s.h_mem || !s.h_status) { rc = MCX_ERR_DEVICE; break; }
        if (hipMalloc((void **)&s.d_src, f->max_src + 8) != hipSuccess || (text_bufs && hipMalloc((void **)&s.d_dst, f->max_dst) != hipSuccess) ||
            hipMalloc((void **)&s.d_mem, (size_t)f->max_members * sizeof(mcx_deflate_member)) != hipSuccess || hipMalloc((void **)&s.d_status, (size_t)f->max_members * 4) != hipSuccess ||
            hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) rc = MCX_ERR_DEVICE;
    }
    if (rc == 0) {
        f->h_check = (mcx_deflate_member *)mcx_pinned_alloc((size_t)f->max_members * sizeof(mcx_deflate_member));
        f->h_check_status = (uint32_t *)mcx_pinned_alloc((size_t)f->max_members * 4);
        if (!f->h_check || !f->h_check_status) rc = MCX_ERR_DEVICE;
    }
    if (rc) { (void)hipGetLastError(); mcx_inflater_free(f); return mcx_set_error(MCX_ERR_DEVICE, "mcx_inflater_create: no room for the staging buffers (host or HBM)"); }
    *out = f;
    return 0;
}

extern "C" int mcx_inflate_dev(mcx_inflater *f, const uint8_t *d_src, uint64_t src_bytes, const mcx_deflate_member *d_members, uint32_t n, uint8_t *d_dst, uint64_t dst_cap, uint32_t *d_status)
{
    if (!f) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate_dev: null argument");
    if (n == 0) return 0;
    if (!d_src || !d_members || !d_status || (!d_dst && dst_cap)) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate_dev: null argument");
    if (n > f->max_members) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate_dev: more members than the inflater was created for");
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(hipMemcpyAsync(f->h_check, d_members, (size_t)n * sizeof(mcx_deflate_member), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    for (uint32_t i = 0; i < n; i++)
        if (const char *why = member_fault(f->h_check[i], src_bytes, dst_cap)) return mcx_set_error(MCX_ERR_ARG, std::string("mcx_inflate_dev: ") + why);
    HIP_TRY(hipEventRecord(f->ev[0], f->stream));
    if (int rc = launch(f, d_src, src_bytes, d_members, n, d_dst, d_status)) return rc;
    HIP_TRY(hipEventRecord(f->ev[1], f->stream));
    HIP_TRY(hipMemcpyAsync(f->h_check_status, d_status, (size_t)n * 4, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    HIP_TRY(hipEventElapsedTime(&f->last_ms, f->ev[0], f->ev[1]));
    uint32_t bad = 0;
    for (uint32_t i = 0; i < n; i++) bad += f->h_check_status[i] != 0;
    if (bad) return mcx_set_error(MCX_ERR_IO, std::to_string(bad) + " of " + std::to_string(n) + " deflate members are damaged");
    return 0;
}

// the last mcx_inflate_dev's kernel in ms, by events on the inflater's stream (scripts/bgzf_rate.py)
extern "C" int mcx_inflate_last_ms(mcx_inflater *f, float *ms)
{
    if (!f || !ms) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate_last_ms: null argument");
    *ms = f->last_ms;
    return 0;
}

// the capacities of one launch through host buffers (what the file front end cuts its stretches by)
void mcx_inflater_caps(const mcx_inflater *f, uint64_t *max_src, uint64_t *max_dst, uint32_t *max_members)
{
    *max_src = f->max_src; *max_dst = f->max_dst; *max_members = f->max_members;
}

// The host form in two halves.  begin: the members' compressed bytes (src_off into src) are packed into the next set's page-locked buffer — with the 8
// bytes of slack behind them —, and copy in, kernel and copy out are queued on the stream; returns at once.  The members must fit one launch, and at most
// two begins may be outstanding.  end: waits for the oldest begin, hands each member's text to dst + its dst_off and its status word to status[] (may be
// null); 0, or MCX_ERR_IO when a member failed.
static int begin(mcx_inflater *f, const uint8_t *src, uint64_t src_bytes, const mcx_deflate_member *members, uint32_t n, uint8_t *d_dst, uint64_t dst_cap);
int mcx_inflate_begin(mcx_inflater *f, const uint8_t *src, uint64_t src_bytes, const mcx_deflate_member *members, uint32_t n, uint64_t dst_cap)
{
    if (!f->text_bufs) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate_begin: the inflater has no buffers for the text");
    return begin(f, src, src_bytes, members, n, nullptr, dst_cap);
}
// The same with the text left in HBM: member i's goes to d_dst[dst_off .. dst_off + isize), d_dst of dst_cap bytes on the inflater's device; any number of
// members up to a launch's, any sum of isize (several stretches in one launch).  mcx_inflate_end then hands out the status words alone (dst: null).
int mcx_inflate_begin_dev(mcx_inflater *f, const uint8_t *src, uint64_t src_bytes, const mcx_deflate_member *members, uint32_t n, uint8_t *d_dst, uint64_t dst_cap)
{
    if (!d_dst) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate_begin_dev: null argument");
    return begin(f, src, src_bytes, members, n, d_dst, dst_cap);
}
static int begin(mcx_inflater *f, const uint8_t *src, uint64_t src_bytes, const mcx_deflate_member *members, uint32_t n, uint8_t *d_dst, uint64_t dst_cap)
{
    Set &s = f->set[f->next];
    if (s.busy) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate_begin: two launches are outstanding already");
    if (n > f->max_members) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate_begin: more members than a launch holds");
    uint64_t so = 0, to = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (const char *why = member_fault(members[i], src_bytes, dst_cap)) return mcx_set_error(MCX_ERR_ARG, std::string("mcx_inflate: ") + why);
        so += members[i].src_len; to += members[i].isize;
    }
    if (so > f->max_src || (!d_dst && to > f->max_dst)) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate_begin: more bytes than a launch holds");
    HIP_TRY(hipSetDevice(f->device));
    s.dst_off.resize(n);
    so = to = 0;
    for (uint32_t i = 0; i < n; i++) {
        const mcx_deflate_member &m = members[i];
        memcpy(s.h_src + so, src + m.src_off, m.src_len);
        mcx_deflate_member &d = s.h_mem[i];
        d.src_off = so; d.dst_off = d_dst ? m.dst_off : to; d.src_len = m.src_len; d.isize = m.isize; d.crc32 = m.crc32; d.reserved = 0;
        s.dst_off[i] = m.dst_off;
        so += m.src_len; to += m.isize;
    }
    memset(s.h_src + so, 0, 8);
    s.n = n; s.dst_bytes = to; s.to_dev = d_dst != nullptr;
    if (n) {
        HIP_TRY(hipMemcpyAsync(s.d_src, s.h_src, so + 8, hipMemcpyHostToDevice, f->stream));
        HIP_TRY(hipMemcpyAsync(s.d_mem, s.h_mem, (size_t)n * sizeof(mcx_deflate_member), hipMemcpyHostToDevice, f->stream));
        if (int rc = launch(f, s.d_src, so + 8, s.d_mem, n, d_dst ? d_dst : s.d_dst, s.d_status)) return rc;
        if (to && !d_dst) HIP_TRY(hipMemcpyAsync(s.h_dst, s.d_dst, to, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(hipMemcpyAsync(s.h_status, s.d_status, (size_t)n * 4, hipMemcpyDeviceToHost, f->stream));
    }
    HIP_TRY(hipEventRecord(s.done, f->stream));
    s.busy = true;
    f->next ^= 1u;
    return 0;
}

int mcx_inflate_end(mcx_inflater *f, uint8_t *dst, uint32_t *status, uint32_t *n_bad)
{
    Set &s = f->set[f->oldest];
    if (n_bad) *n_bad = 0;
    if (!s.busy) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate_end: nothing is outstanding");
    s.busy = false;
    f->oldest ^= 1u;
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(hipEventSynchronize(s.done));
    uint32_t bad = 0;
    for (uint32_t i = 0; i < s.n && !s.to_dev;) { // members whose texts follow one another at the caller's too leave in one copy
        uint32_t j = i;
        uint64_t bytes = 0;
        do { bytes += s.h_mem[j].isize; j++; } while (j < s.n && s.dst_off[j] == s.dst_off[i] + bytes);
        if (bytes) memcpy(dst + s.dst_off[i], s.h_dst + s.h_mem[i].dst_off, bytes);
        i = j;
    }
    for (uint32_t i = 0; i < s.n; i++) { if (status) status[i] = s.h_status[i]; bad += s.h_status[i] != 0; }
    if (n_bad) *n_bad = bad;
    if (bad) return mcx_set_error(MCX_ERR_IO, std::to_string(bad) + " of " + std::to_string(s.n) + " deflate members are damaged");
    return 0;
}

extern "C" int mcx_inflate(mcx_inflater *f, const uint8_t *src, uint64_t src_bytes, const mcx_deflate_member *members, uint32_t n, uint8_t *dst, uint64_t dst_cap, uint32_t *status)
{
    if (!f) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate: null argument");
    if (n == 0) return 0;
    if (!src || !members || (!dst && dst_cap)) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate: null argument");
    if (f->set[0].busy || f->set[1].busy) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate: launches of mcx_inflate_begin are outstanding");
    for (uint32_t i = 0; i < n; i++) { // everything is checked before the first launch
        if (const char *why = member_fault(members[i], src_bytes, dst_cap)) return mcx_set_error(MCX_ERR_ARG, std::string("mcx_inflate: ") + why);
        if (members[i].src_len > f->max_src) return mcx_set_error(MCX_ERR_ARG, "mcx_inflate: a member is larger than the inflater's max_src_bytes");
    }
    // as many launches as the capacities require, the next one's bytes staged while this one's are on the device
    int rc = 0, io = 0;
    uint32_t begun = 0, ended = 0, first[2] = {0, 0};
    while (ended < n && rc == 0) {
        uint32_t outstanding = (f->set[0].busy ? 1u : 0u) + (f->set[1].busy ? 1u : 0u);
        if (begun < n && outstanding < 2) {
            uint32_t k = begun;
            uint64_t so = 0, to = 0;
            while (k < n && k - begun < f->max_members && so + members[k].src_len <= f->max_src && to + members[k].isize <= f->max_dst) { so += members[k].src_len; to += members[k].isize; k++; }
            first[f->next] = begun;
            rc = mcx_inflate_begin(f, src, src_bytes, members + begun, k - begun, dst_cap);
            begun = k;
            if (rc == 0 && begun < n && outstanding == 0) continue; // (a second launch behind the first before anything is waited for)
        }
        if (rc) break;
        Set &s = f->set[f->oldest];
        const uint32_t at = first[f->oldest], cnt = s.n;
        const int e = mcx_inflate_end(f, dst, status ? status + at : nullptr, nullptr);
        if (e == MCX_ERR_IO) io = e; else if (e) rc = e;
        ended = at + cnt;
    }
    if (rc) { // (leave nothing outstanding behind an error)
        (void)hipStreamSynchronize(f->stream);
        f->set[0].busy = f->set[1].busy = false; f->next = f->oldest = 0;
        return rc;
    }
    return io ? mcx_set_error(MCX_ERR_IO, "mcx_inflate: deflate members are damaged (see the status words)") : 0;
}
