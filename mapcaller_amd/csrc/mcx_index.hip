// mapcaller_amd/csrc/mcx_index.hip — the index in HBM: loaded from the reference's files or taken from arrays built on the device
// (mcx_index_build.hip), with what the seeding walk adds to it (derived .bwt blocks, full suffix array, jump table, rank and pair
// records), and the mcx_index_* ABI.  Reached through that ABI alone; it calls what mcx_build.h declares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
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

// Expands the sampled suffix array: the chain of LF steps that starts at a sampled row visits
// exactly the rows whose bwt_sa() walk ends at the next sampled row, with values one lower per
// step (SA[LF(k)] = SA[k] - 1).  One chain per lane, ~32 dependent block fetches each.
__global__ void k_expand_sa(IndexView ix, uint64_t n_sa, uint64_t *full)
{
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_sa) return;
    uint64_t k = j * (uint64_t)ix.sa_intv;
    uint64_t val = j == 0 ? ix.seq_len : ix.sa[j];
    full[k] = j == 0 ? ~0ull : val;
    const uint64_t mask = (uint64_t)ix.sa_intv - 1;
    for (;;) {
        k = fm_lf(ix, k);
        val -= 1;
        if ((k & mask) == 0) break;
        full[k] = val;
    }
}

// the derived form of the index blocks (mcx_fm.h fm_derive_block): one thread per block that holds symbols
__global__ void k_derive_bwt(uint32_t *bwt, uint64_t n_blocks)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_blocks) fm_derive_block(bwt + (i << 4));
}

static int derive_bwt(mcx_index *ix)
{
    const uint64_t n_blocks = (ix->host.seq_len + 127) / 128;
    k_derive_bwt<<<(unsigned)((n_blocks + 255) / 256), 256>>>((uint32_t *)ix->d_bwt, n_blocks);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

__global__ void k_build_ktab(IndexView ix, int K, U4 *tab)
{
    const uint64_t n = 1ull << (2 * K);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t x0, x1, x2;
        ktab_entry(ix, (uint32_t)i, K, x0, x1, x2);
        tab[i] = ktab_pack(x0, x1, x2);
    }
}

// the K-mer jump table of the seeding walk (mcx_fm.h): 16 bytes per K-mer, K from the text length
// (MCX_KTAB_K overrides it for experiments)
static int build_rank(mcx_index *ix);
static int build_ktab(mcx_index *ix)
{
    int K = ktab_k_for(ix->view.seq_len);
    if (const char *e = getenv("MCX_KTAB_K")) { const int k = atoi(e); if (k >= 4 && k <= 16) K = k; } // (16: 69 GB — one pair step fewer per search; no room for it beside the -vcf planes)
    const size_t bytes = (size_t)16 << (2 * K);
    hipError_t e = hipMalloc(&ix->d_ktab, bytes);
    if (e != hipSuccess) return mcx_set_error(MCX_ERR_DEVICE, std::string("hipMalloc(ktab): ") + hipGetErrorString(e));
    ix->view.ktab = nullptr; ix->view.ktab_k = K;
    k_build_ktab<<<8192, 256>>>(ix->view, K, (U4 *)ix->d_ktab);
    e = hipDeviceSynchronize();
    if (e != hipSuccess) return mcx_set_error(MCX_ERR_DEVICE, std::string("k_build_ktab: ") + hipGetErrorString(e));
    ix->view.ktab = (const uint32_t *)ix->d_ktab;
    ix->hbm_bytes += (int64_t)bytes;
    return build_rank(ix);
}

// the rank records of the seeding walk (mcx_fm.h RankChunk): one thread per .bwt block, four records per base
__global__ void k_build_rank(const uint32_t *bwt, uint64_t n_blocks, uint64_t n_chunks, RankChunk *rank, unsigned long long *cross)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_blocks) return;
    const uint32_t *blk = bwt + (i << 4);
    uint64_t before[4];
    for (int c = 0; c < 4; c++) before[c] = fm_plain_count((uint64_t)blk[2 * c] | ((uint64_t)blk[2 * c + 1] << 32));
    for (int q = 0; q < 4; q++) {
        const uint64_t chunk = 4 * i + q;
        if (chunk >= n_chunks) break;
        RankChunk out[4];
        uint64_t ne[4], ng[4];
        fm_rank_records(blk[8 + 2 * q], blk[9 + 2 * q], before, out, ne, ng);
        for (int b = 0; b < 4; b++) {
            rank[(uint64_t)b * n_chunks + chunk] = out[b];
            if (ne[b] >> 32) atomicMin(&cross[b], (unsigned long long)chunk);
            if (ng[b] >> 32) atomicMin(&cross[4 + b], (unsigned long long)chunk);
            before[b] += (uint64_t)__popc(out[b].eq);
        }
    }
}

static int build_rank(mcx_index *ix)
{
    if (!ix->view.sa_full || getenv("MCX_NO_RANK")) return 0; // (the walk then counts in the .bwt blocks: MCX_NO_RANK for experiments)
    // a record keeps its two running counts in 32 bits plus ONE crossing chunk per base and count (rank_cross): exact while no count
    // passes 2^32 twice, i.e. below 2^33 symbols.  Longer texts (genomes above ~4.29 Gbp) walk the .bwt blocks, which have no such limit.
    if (ix->host.seq_len >= ((uint64_t)1 << 33)) return 0;
    const uint64_t n_blocks = (ix->host.seq_len + 127) / 128, n_chunks = (ix->host.seq_len + 31) / 32;
    const size_t bytes = (size_t)4 * n_chunks * sizeof(RankChunk) + 64;
    unsigned long long *d_cross = nullptr, h_cross[8];
    for (auto &x : h_cross) x = ~0ull;
    hipError_t e = hipMalloc(&ix->d_rank, bytes);
    if (e != hipSuccess) return mcx_set_error(MCX_ERR_DEVICE, std::string("hipMalloc(rank records): ") + hipGetErrorString(e));
    HIP_TRY(hipMalloc((void **)&d_cross, sizeof h_cross));
    e = hipMemcpy(d_cross, h_cross, sizeof h_cross, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        k_build_rank<<<(unsigned)((n_blocks + 255) / 256), 256>>>((const uint32_t *)ix->d_bwt, n_blocks, n_chunks, (RankChunk *)ix->d_rank, d_cross);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(h_cross, d_cross, sizeof h_cross, hipMemcpyDeviceToHost);
    (void)hipFree(d_cross);
    if (e != hipSuccess) return mcx_set_error(MCX_ERR_DEVICE, std::string("rank records: ") + hipGetErrorString(e)); // (d_rank is the index's: mcx_index_free releases it)
    ix->view.rank = ix->d_rank; ix->view.rank_chunks = n_chunks;
    for (int k = 0; k < 8; k++) ix->view.rank_cross[k] = h_cross[k];
    ix->hbm_bytes += (int64_t)bytes;
    // the pair records on top (two bases per step): MCX_NO_RANK2 for experiments, MCX_RANK2_CHECK=n extends n random intervals both ways
    if (!ix->pair_records || getenv("MCX_NO_RANK2")) return 0;
    const char *chk = getenv("MCX_RANK2_CHECK");
    const int rc = mcx_build_pair_records(ix->view, &ix->d_rank2, &ix->d_rank2_c2, &ix->rank2_bytes, chk ? atoi(chk) : 0);
    if (rc && ix->pair_records == MCX_INDEX_PAIRS_IF_ROOM) {
        // nobody asked for the records by name (the CLI without -vcf takes them when there is room): a device that is too full for them
        // — several shards on it, a smaller part — keeps the one-base walk, which needs nothing more
        fprintf(stderr, "[mcx] the pair records do not fit this device (%s): the seeding walk takes one base per step\n", mcx_last_error());
        (void)hipGetLastError();
        mcx_set_error(0, "");
        ix->d_rank2 = ix->d_rank2_c2 = nullptr; ix->rank2_bytes = 0;
        ix->view.rank2 = nullptr; ix->view.rank2_c2 = nullptr;
        return 0;
    }
    if (rc) return rc;
    ix->hbm_bytes += ix->rank2_bytes;
    return 0;
}

static int upload(void **dst, const void *src, size_t bytes, size_t pad, int64_t &acc)
{
    HIP_TRY(hipMalloc(dst, bytes + pad));
    if (pad) HIP_TRY(hipMemset((uint8_t *)*dst + bytes, 0, pad));
    HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    acc += (int64_t)(bytes + pad);
    return 0;
}

static int index_to_device(mcx_index *ix, int full_sa)
{
    HostIndex &h = ix->host;
    int rc;
    if ((rc = upload(&ix->d_bwt, h.bwt.data(), h.bwt.size() * 4, 128, ix->hbm_bytes))) return rc;
    if ((rc = upload(&ix->d_sa, h.sa.data(), h.sa.size() * 8, 0, ix->hbm_bytes))) return rc;
    if ((rc = upload(&ix->d_pac, h.pac.data(), h.pac.size(), 16, ix->hbm_bytes))) return rc;
    if ((rc = upload(&ix->d_end_pos, h.end_pos.data(), h.end_pos.size() * 8, 0, ix->hbm_bytes))) return rc;
    if ((rc = upload(&ix->d_end_chr, h.end_chr.data(), h.end_chr.size() * 4, 0, ix->hbm_bytes))) return rc;
    if ((rc = upload(&ix->d_chr_fwd, h.chr_fwd.data(), h.chr_fwd.size() * 8, 0, ix->hbm_bytes))) return rc;
    if (!h.hole_off.empty()) { // the ambiguity holes, beside the index: not part of the view the mapping kernels are passed
        if ((rc = upload(&ix->d_hole_off, h.hole_off.data(), h.hole_off.size() * 8, 0, ix->hbm_bytes))) return rc;
        if ((rc = upload(&ix->d_hole_len, h.hole_len.data(), h.hole_len.size() * 4, 0, ix->hbm_bytes))) return rc;
        if ((rc = upload(&ix->d_hole_letter, h.hole_letter.data(), h.hole_letter.size(), 0, ix->hbm_bytes))) return rc;
    }
    IndexView &v = ix->view;
    v.bwt = (const uint32_t *)ix->d_bwt; v.sa = (const uint64_t *)ix->d_sa; v.sa_full = nullptr; v.ktab = nullptr; v.ktab_k = 0; v.rank = nullptr; v.rank_chunks = 0; for (auto &x : v.rank_cross) x = ~0ull; v.rank2 = nullptr; v.rank2_c2 = nullptr; v.rank2_lone = ~0ull; v.rank2_t0 = 0;
    v.pac = (const uint8_t *)ix->d_pac;
    v.end_pos = (const int64_t *)ix->d_end_pos; v.end_chr = (const int32_t *)ix->d_end_chr;
    v.chr_fwd = (const int64_t *)ix->d_chr_fwd;
    v.primary = h.primary; for (int i = 0; i < 5; i++) v.L2[i] = h.L2[i];
    v.seq_len = h.seq_len; v.G = h.G; v.G2 = 2 * h.G;
    v.n_ends = (int32_t)h.end_pos.size(); v.n_chr = (int32_t)h.chr_len.size(); v.sa_intv = h.sa_intv;
    if ((rc = derive_bwt(ix))) return rc;
    if (full_sa) {
        size_t bytes = (size_t)(h.seq_len + 1) * 8;
        HIP_TRY(hipMalloc(&ix->d_sa_full, bytes + 16)); // (+16: rows are fetched in pairs, seed_take)
        ix->hbm_bytes += (int64_t)bytes;
        uint64_t n_sa = h.sa.size();
        k_expand_sa<<<(unsigned)((n_sa + 255) / 256), 256>>>(v, n_sa, (uint64_t *)ix->d_sa_full);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        v.sa_full = (const uint64_t *)ix->d_sa_full;
    }
    return build_ktab(ix);
}

extern "C" int mcx_index_load(const char *prefix, int device, int full_sa, mcx_index **out)
{
    if (!prefix || !out) return mcx_set_error(MCX_ERR_ARG, "mcx_index_load: null argument");
    mcx_index *ix = new mcx_index();
    std::string err;
    if (!host_index_load(prefix, ix->host, err)) { delete ix; return mcx_set_error(MCX_ERR_IO, err); }
    ix->device = device;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { delete ix; return mcx_set_error(MCX_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e)); }
    ix->pair_records = full_sa >= 2 ? full_sa : 0;
    int rc = index_to_device(ix, full_sa);
    if (rc) { mcx_index_free(ix); return rc; }
    *out = ix;
    return 0;
}

__global__ void k_pack_pac(const uint8_t *codes, uint64_t G, uint8_t *pac)
{
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < G / 4 + 1; b += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t v = 0;
        for (int k = 0; k < 4; k++) { uint64_t i = b * 4 + k; v = (v << 2) | (i < G ? (codes[i] & 3u) : 0u); }
        pac[b] = (uint8_t)v;
    }
}

static int index_from_arrays(mcx_index *ix, const DevIndexArrays &arr, const uint8_t *d_codes, int64_t G);

extern "C" int mcx_index_from_codes(const uint8_t *d_codes, int32_t n_chr, const int32_t *chr_len, const char *const *chr_name,
                                    int device, int full_sa, mcx_index **out, double *build_seconds)
{
    if (!d_codes || !chr_len || n_chr <= 0 || !out) return mcx_set_error(MCX_ERR_ARG, "mcx_index_from_codes: bad argument");
    HIP_TRY(hipSetDevice(device));
    mcx_index *ix = new mcx_index();
    ix->device = device;
    HostIndex &h = ix->host;
    int64_t G = 0;
    for (int i = 0; i < n_chr; i++) {
        h.chr_len.push_back(chr_len[i]);
        h.chr_name.push_back(chr_name && chr_name[i] ? chr_name[i] : ("chr" + std::to_string(i + 1)));
        G += chr_len[i];
    }
    h.G = G;
    host_index_finish(h);
    DevIndexArrays arr;
    int rc = mcx_build_suffix_index(d_codes, (uint64_t)G, full_sa != 0, arr, build_seconds);
    if (rc) { delete ix; return rc; }
    ix->pair_records = full_sa >= 2 ? full_sa : 0;
    rc = index_from_arrays(ix, arr, d_codes, G);
    if (rc) { mcx_index_free(ix); return rc; }
    *out = ix;
    return 0;
}

static int index_from_arrays(mcx_index *ix, const DevIndexArrays &arr, const uint8_t *d_codes, int64_t G)
{
    HostIndex &h = ix->host;
    int rc;
    h.primary = arr.primary; for (int i = 0; i < 5; i++) h.L2[i] = arr.L2[i];
    h.seq_len = arr.seq_len; h.sa_intv = 32;
    ix->d_bwt = arr.bwt; ix->d_sa = arr.sa; ix->d_sa_full = arr.sa_full;
    ix->hbm_bytes = (int64_t)(arr.bwt_words * 4 + arr.n_sa * 8 + (arr.sa_full ? (arr.seq_len + 1) * 8 : 0));
    ix->n_bwt_words = arr.bwt_words; ix->n_sa = arr.n_sa;
    HIP_TRY(hipMalloc(&ix->d_pac, (size_t)G / 4 + 32));
    k_pack_pac<<<1024, 256>>>(d_codes, (uint64_t)G, (uint8_t *)ix->d_pac);
    HIP_TRY(hipGetLastError());
    int64_t acc = 0;
    if ((rc = upload(&ix->d_end_pos, h.end_pos.data(), h.end_pos.size() * 8, 0, acc))) return rc;
    if ((rc = upload(&ix->d_end_chr, h.end_chr.data(), h.end_chr.size() * 4, 0, acc))) return rc;
    if ((rc = upload(&ix->d_chr_fwd, h.chr_fwd.data(), h.chr_fwd.size() * 8, 0, acc))) return rc;
    ix->hbm_bytes += acc + G / 4 + 32;
    IndexView &v = ix->view;
    v.bwt = (const uint32_t *)ix->d_bwt; v.sa = (const uint64_t *)ix->d_sa; v.sa_full = (const uint64_t *)ix->d_sa_full; v.ktab = nullptr; v.ktab_k = 0; v.rank = nullptr; v.rank_chunks = 0; for (auto &x : v.rank_cross) x = ~0ull; v.rank2 = nullptr; v.rank2_c2 = nullptr; v.rank2_lone = ~0ull; v.rank2_t0 = 0;
    v.pac = (const uint8_t *)ix->d_pac;
    v.end_pos = (const int64_t *)ix->d_end_pos; v.end_chr = (const int32_t *)ix->d_end_chr; v.chr_fwd = (const int64_t *)ix->d_chr_fwd;
    v.primary = h.primary; for (int i = 0; i < 5; i++) v.L2[i] = h.L2[i];
    v.seq_len = h.seq_len; v.G = h.G; v.G2 = 2 * h.G;
    v.n_ends = (int32_t)h.end_pos.size(); v.n_chr = (int32_t)h.chr_len.size(); v.sa_intv = 32;
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = derive_bwt(ix))) return rc;
    return build_ktab(ix);
}

// writes <prefix>.bwt/.sa/.pac/.ann/.amb from an index built in HBM (no ambiguity holes: the
// codes it was built from had none)
extern "C" int mcx_index_save(const mcx_index *ix, const char *prefix)
{
    if (!ix || !prefix) return mcx_set_error(MCX_ERR_ARG, "mcx_index_save: null argument");
    if (!ix->n_bwt_words) return mcx_set_error(MCX_ERR_ARG, "mcx_index_save: only indexes built with mcx_index_from_codes can be saved");
    HIP_TRY(hipSetDevice(ix->device));
    const HostIndex &h = ix->host;
    std::string p(prefix);
    std::vector<uint32_t> words(ix->n_bwt_words);
    HIP_TRY(hipMemcpy(words.data(), ix->d_bwt, words.size() * 4, hipMemcpyDeviceToHost));
    { // the file holds the plain counts (the blocks in HBM carry sub-block counts in their top bits: fm_derive_block)
        const uint64_t n_blocks = (h.seq_len + 127) / 128;
        for (uint64_t i = 0; i < n_blocks && i * 16 + 8 <= words.size(); i++) for (int x = 0; x < 4; x++) words[i * 16 + 2 * x + 1] &= 0xFFu;
    }
    FILE *f = fopen((p + ".bwt").c_str(), "wb");
    if (!f) return mcx_set_error(MCX_ERR_IO, "cannot write " + p + ".bwt");
    fwrite(&h.primary, 8, 1, f); fwrite(h.L2 + 1, 8, 4, f); fwrite(words.data(), 4, words.size(), f); fclose(f);
    std::vector<uint64_t> sa(ix->n_sa);
    HIP_TRY(hipMemcpy(sa.data(), ix->d_sa, sa.size() * 8, hipMemcpyDeviceToHost));
    f = fopen((p + ".sa").c_str(), "wb");
    if (!f) return mcx_set_error(MCX_ERR_IO, "cannot write " + p + ".sa");
    const uint64_t intv = 32;
    fwrite(&h.primary, 8, 1, f); fwrite(h.L2 + 1, 8, 4, f); fwrite(&intv, 8, 1, f); fwrite(&h.seq_len, 8, 1, f);
    fwrite(sa.data() + 1, 8, sa.size() - 1, f); fclose(f);
    const uint64_t G = (uint64_t)h.G;
    std::vector<uint8_t> pac(G / 4 + 1);
    HIP_TRY(hipMemcpy(pac.data(), ix->d_pac, pac.size(), hipMemcpyDeviceToHost));
    f = fopen((p + ".pac").c_str(), "wb");
    if (!f) return mcx_set_error(MCX_ERR_IO, "cannot write " + p + ".pac");
    fwrite(pac.data(), 1, (G >> 2) + ((G & 3) == 0 ? 0 : 1), f);
    uint8_t ct = 0;
    if (G % 4 == 0) fwrite(&ct, 1, 1, f);
    ct = (uint8_t)(G % 4); fwrite(&ct, 1, 1, f); fclose(f);
    f = fopen((p + ".ann").c_str(), "w");
    if (!f) return mcx_set_error(MCX_ERR_IO, "cannot write " + p + ".ann");
    fprintf(f, "%lld %d %u\n", (long long)h.G, (int)h.chr_len.size(), 11u);
    for (size_t i = 0; i < h.chr_len.size(); i++)
        fprintf(f, "%d %s (null)\n%lld %d %d\n", 0, h.chr_name[i].c_str(), (long long)h.chr_fwd[i], h.chr_len[i], 0);
    fclose(f);
    f = fopen((p + ".amb").c_str(), "w");
    if (!f) return mcx_set_error(MCX_ERR_IO, "cannot write " + p + ".amb");
    fprintf(f, "%lld %d %u\n", (long long)h.G, (int)h.chr_len.size(), 0u);
    fclose(f);
    return 0;
}

extern "C" void mcx_index_free(mcx_index *ix)
{
    if (!ix) return;
    void *p[] = {ix->d_bwt, ix->d_sa, ix->d_sa_full, ix->d_pac, ix->d_end_pos, ix->d_end_chr, ix->d_chr_fwd, ix->d_ktab, ix->d_rank, ix->d_rank2, ix->d_rank2_c2, ix->d_hole_off, ix->d_hole_len, ix->d_hole_letter};
    for (void *q : p) if (q) (void)hipFree(q);
    // (a caller that frees the index before its contexts — allowed: a context that is only freed afterwards touches no device memory of the index — leaves
    //  the host object to the last mcx_ctx_free, which still counts itself out of it)
    ix->d_bwt = ix->d_sa = ix->d_sa_full = ix->d_pac = ix->d_end_pos = ix->d_end_chr = ix->d_chr_fwd = ix->d_ktab = ix->d_rank = ix->d_rank2 = ix->d_rank2_c2 = nullptr;
    ix->d_hole_off = ix->d_hole_len = ix->d_hole_letter = nullptr;
    if (ix->n_ctx.load() > 0) { ix->orphan.store(true); return; }
    delete ix;
}
// gives back what an index holds above `full_sa` (2 -> 1: the pair records).  Contexts made before keep their view of the index: close them first.
extern "C" int mcx_index_trim(mcx_index *ix, int full_sa)
{
    if (!ix) return mcx_set_error(MCX_ERR_ARG, "mcx_index_trim: null argument");
    if (full_sa < 1) return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_index_trim: only the pair records can be released (full_sa = 1)");
    if (full_sa >= 2 || !ix->d_rank2) return 0;
    // a context keeps pointers into what goes (the view it copies per pass, a batch under way): none may be alive
    if (ix->n_ctx.load() > 0) return mcx_set_error(MCX_ERR_ARG, "mcx_index_trim: " + std::to_string(ix->n_ctx.load()) + " context(s) of this index are still open; free them first");
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());
    (void)hipFree(ix->d_rank2); (void)hipFree(ix->d_rank2_c2);
    ix->d_rank2 = ix->d_rank2_c2 = nullptr;
    ix->view.rank2 = nullptr; ix->view.rank2_c2 = nullptr;
    ix->hbm_bytes -= ix->rank2_bytes; ix->rank2_bytes = 0;
    return 0;
}
extern "C" int64_t mcx_index_genome_size(const mcx_index *ix) { return ix->host.G; }
extern "C" int32_t mcx_index_n_chr(const mcx_index *ix) { return (int32_t)ix->host.chr_len.size(); }
extern "C" const char *mcx_index_chr_name(const mcx_index *ix, int32_t i) { return ix->host.chr_name[i].c_str(); }
extern "C" int32_t mcx_index_chr_len(const mcx_index *ix, int32_t i) { return ix->host.chr_len[i]; }
extern "C" int64_t mcx_index_hbm_bytes(const mcx_index *ix) { return ix->hbm_bytes; }

