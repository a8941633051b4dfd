// mapcaller_amd/csrc/mcx_sam_state.h — what a context keeps for its output formatters on the device (mcx_sam.hip: SAM text; mcx_bam.hip: BAM records), which take
// the same input and share the lengths, the scan's scratch and — in the file front end — the part's buffers.  Not part of the ABI; HIP translation units only.
#ifndef MCX_SAM_STATE_H
#define MCX_SAM_STATE_H
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <string>
#include <vector>
#include "mcx_internal.h"

namespace mcx {

// -sort (mcx_bam_sort.hip): the arrays of a call's records — source and destination offsets, keys, lengths and indexes, as found and in sorted order —, the
// groups' counts, hipcub's scratch, the sorted records, and for the merge's chunks the blocks read back, their members and their text
struct SortBufs {
    uint64_t *d_src_off = nullptr, *d_dst_off = nullptr, *d_key = nullptr, *d_key_s = nullptr; uint32_t *d_len = nullptr, *d_len_s = nullptr, *d_idx = nullptr, *d_idx_s = nullptr; uint64_t cap = 0;
    uint32_t *d_count = nullptr, *d_first = nullptr; uint64_t cap_groups = 0;
    void *d_tmp = nullptr; size_t tmp_bytes = 0;
    uint32_t *d_error = nullptr;
    uint8_t *d_sorted = nullptr, *d_src = nullptr, *d_inflated = nullptr; uint64_t cap_sorted = 0, cap_src = 0, cap_inflated = 0;
    mcx_deflate_member *d_members = nullptr; uint32_t *d_status = nullptr; uint64_t *d_slices = nullptr; uint64_t cap_members = 0, cap_status = 0, cap_slices = 0;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float ms[4] = {0, 0, 0, 0}; // the last call's index, sort, place, gather
    ~SortBufs()
    {
        void *p[] = {d_src_off, d_dst_off, d_key, d_key_s, d_len, d_len_s, d_idx, d_idx_s, d_count, d_first, d_tmp, d_error, d_sorted, d_src, d_inflated, d_members, d_status, d_slices};
        for (void *q : p) if (q) (void)hipFree(q);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

// -index (mcx_bai.hip): per record of a call its (refID, bin), virtual offset, end window (packed with the contig, and its running maximum), first window, head
// and mapped flags (and their running sums); per stretch its first record; hipcub's scratch
struct BaiBufs {
    uint64_t *d_tb = nullptr, *d_u = nullptr, *d_wpack = nullptr, *d_wmax = nullptr, *d_hm = nullptr, *d_hs = nullptr; uint32_t *d_w0 = nullptr, *d_start = nullptr; uint64_t cap = 0;
    void *d_tmp = nullptr; size_t tmp_bytes = 0;
    uint32_t *d_error = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float ms[3] = {0, 0, 0}; // the last call's records, stretches, windows
    ~BaiBufs()
    {
        void *p[] = {d_tb, d_u, d_wpack, d_wmax, d_hm, d_hs, d_w0, d_start, d_tmp, d_error};
        for (void *q : p) if (q) (void)hipFree(q);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

// -markdup (mcx_markdup.hip): a call's units before they are known to be whole (d_units; the front end's resolve: the whole run's, with their bytes in d_dup), a
// chunk's duplicate bytes (d_bits), and the resolve's tables: two key and two index arrays of two entries a unit, the heads' flags, hipcub's scratch
struct DupBufs {
    mcx_dup_unit *d_units = nullptr; uint64_t cap_units = 0;
    uint8_t *d_bits = nullptr, *d_dup = nullptr; uint64_t cap_bits = 0, cap_dup = 0;
    uint64_t *d_ka = nullptr, *d_kb = nullptr; uint32_t *d_ia = nullptr, *d_ib = nullptr, *d_flag = nullptr; uint64_t cap = 0;
    void *d_tmp = nullptr; size_t tmp_bytes = 0;
    uint32_t *d_error = nullptr; // [0] the error bits, [1] and [2] the groups the resolve counted among pairs and among fragments
    hipEvent_t ev[2] = {nullptr, nullptr};
    float ms[3] = {0, 0, 0}; // the last units, resolve and mark call
    uint64_t groups = 0;     // the last resolve's
    void drop_run() // what the front end's one resolve held: the run's units and their bytes
    {
        if (d_units) (void)hipFree(d_units);
        if (d_dup) (void)hipFree(d_dup);
        d_units = nullptr; d_dup = nullptr; cap_units = 0; cap_dup = 0;
    }
    void drop_tables()       // the resolve's arrays, which are as large as the whole run's units
    {
        void *p[] = {d_ka, d_kb, d_ia, d_ib, d_flag, d_tmp};
        for (void *q : p) if (q) (void)hipFree(q);
        d_ka = d_kb = nullptr; d_ia = d_ib = d_flag = nullptr; d_tmp = nullptr; cap = 0; tmp_bytes = 0;
    }
    ~DupBufs()
    {
        drop_tables();
        void *p[] = {d_units, d_bits, d_dup, d_error};
        for (void *q : p) if (q) (void)hipFree(q);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

// the contigs' names (once), the lengths and offsets of a batch, and — for the file front end — the names, qualities and text (or records) of a batch part in HBM
struct SamState {
    char *d_cn_text = nullptr; uint32_t *d_cn_off = nullptr;
    uint64_t *d_len = nullptr, *d_off = nullptr; uint64_t cap_reads = 0;
    void *d_tmp = nullptr; size_t tmp_bytes = 0;
    uint64_t *h_total = nullptr;            // page-locked: [0] the batch's bytes, [1] (BAM) the lines that made no record
    unsigned long long *d_dropped = nullptr; // (BAM) counted by the length kernel
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float ms[3] = {0, 0, 0}; // the last call's length kernel, scan, write kernel
    uint8_t *d_names = nullptr, *d_qual = nullptr, *d_text = nullptr, *d_bgzf = nullptr; uint32_t *d_name_off = nullptr; // (d_bgzf: -bgzf, the text's blocks)
    uint64_t cap_names = 0, cap_qual = 0, cap_text = 0, cap_name_off = 0, cap_bgzf = 0;
    uint8_t *d_md = nullptr; uint32_t *d_md_off = nullptr; uint64_t cap_md = 0, cap_md_off = 0; // -md (mcx_md.hip): a batch part's MD strings and their offsets
    bool want_md = false;                                                                        // the file front end's -md is on (mcx_md_set)
    float md_ms[3] = {0, 0, 0};                                                                 // the last mcx_md[_dev]'s length kernel, scan, write kernel
    uint8_t *d_rg = nullptr; mcx_sam_tags tags = mcx_sam_tags();                                // -rg / -mc (mcx_tags_set): the read group's ID in HBM and what the front end's formatter calls get
    SortBufs sort;
    BaiBufs bai;
    DupBufs dup;
    ~SamState()
    {
        void *p[] = {d_cn_text, d_cn_off, d_len, d_off, d_tmp, d_dropped, d_names, d_qual, d_text, d_name_off, d_bgzf, d_md, d_md_off, d_rg};
        for (void *q : p) if (q) (void)hipFree(q);
        if (h_total) (void)hipHostFree(h_total);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

static inline int sam_state_of(mcx_ctx *c, SamState **out)
{
    void **slot = mcx_ctx_sam_slot(c, [](void *p) { delete (SamState *)p; });
    if (!*slot) *slot = new SamState();
    SamState *st = (SamState *)*slot;
    if (!st->d_cn_text) { // the contigs' names go to the device once per context
        const HostIndex &hx = mcx_ctx_index(c)->host;
        std::string text;
        std::vector<uint32_t> off(1, 0);
        for (const std::string &s : hx.chr_name) { text += s; off.push_back((uint32_t)text.size()); }
        hipError_t e = hipMalloc((void **)&st->d_cn_off, off.size() * 4);
        if (e == hipSuccess) e = hipMalloc((void **)&st->d_dropped, 8);
        if (e == hipSuccess) e = hipMemcpy(st->d_cn_off, off.data(), off.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess && !st->h_total) e = hipHostMalloc((void **)&st->h_total, 16, hipHostMallocDefault);
        for (hipEvent_t &ev : st->ev) if (e == hipSuccess && !ev) e = hipEventCreate(&ev);
        char *d_text = nullptr;
        if (e == hipSuccess) e = hipMalloc((void **)&d_text, text.size() + 16);
        if (e == hipSuccess) e = hipMemcpy(d_text, text.data(), text.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (d_text) (void)hipFree(d_text);
            if (st->d_cn_off) (void)hipFree(st->d_cn_off);
            if (st->d_dropped) (void)hipFree(st->d_dropped);
            st->d_cn_off = nullptr; st->d_dropped = nullptr;
            return mcx_set_error(MCX_ERR_DEVICE, std::string("the formatter's buffers: ") + hipGetErrorString(e));
        }
        st->d_cn_text = d_text; // (set last: a half-made state is made again)
    }
    *out = st;
    return 0;
}

// mate_tags with -m extras: an extra is paired with another candidate of the mate than the one whose CIGAR the batch holds
static inline bool tags_ok(const mcx_sam_in *in, const mcx_sam_tags *tags) { return !(tags && tags->mate_tags && in->x_index); }
static constexpr const char *kTagsWithExtras = ": MC and MQ cannot be made for -m lines (mate_tags with x_index): an extra line is paired with another candidate of the mate";

template <class T> int sam_grow(T **p, uint64_t *cap, uint64_t need, const char *what)
{
    if (need <= *cap) return 0;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    const uint64_t want = need + need / 8 + 4096;
    if (hipMalloc((void **)p, want * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return mcx_set_error(MCX_ERR_DEVICE, std::string("no room in HBM for ") + what + " (" + std::to_string(want * sizeof(T) >> 20) + " MB): map with a smaller -batch");
    }
    *cap = want;
    return 0;
}

// room for the lengths, the offsets and the scan's scratch at n_reads + 1 entries
static inline int sam_scan_room(SamState *st, uint64_t entries, hipStream_t s)
{
    if (entries <= st->cap_reads) return 0;
    uint64_t cap_b = st->cap_reads;
    int rc;
    if ((rc = sam_grow(&st->d_len, &st->cap_reads, entries, "the lines' lengths"))) return rc;
    if ((rc = sam_grow(&st->d_off, &cap_b, entries, "the lines' offsets"))) return rc;
    size_t need = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, need, st->d_len, st->d_off, (int)st->cap_reads, s) != hipSuccess) return mcx_set_error(MCX_ERR_DEVICE, "the scan over the lines' lengths cannot be sized");
    if (need > st->tmp_bytes) {
        if (st->d_tmp) (void)hipFree(st->d_tmp);
        st->d_tmp = nullptr; st->tmp_bytes = 0;
        if (hipMalloc(&st->d_tmp, need) != hipSuccess) { (void)hipGetLastError(); return mcx_set_error(MCX_ERR_DEVICE, "no room in HBM for the scan over the lines' lengths"); }
        st->tmp_bytes = need;
    }
    return 0;
}

} // namespace mcx
#endif
