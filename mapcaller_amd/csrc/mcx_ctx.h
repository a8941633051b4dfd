// mapcaller_amd/csrc/mcx_ctx.h — the context of a mapping run and what the units of libmcx.so that work on it share
// (mcx_pipeline.hip, mcx_dp_stage.hip, mcx_stream.hip, mcx_profile.hip).  Not part of the ABI.
#ifndef MCX_CTX_H
#define MCX_CTX_H
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
#include "mcx_dp.h"
#include "mcx_dp_lane2.h"
#include "mcx_simple.h"
#include "mcx_profile.h"
#include "mcx_internal.h"

using namespace mcx;

// ---------------------------------------------------------------------------------------------
// errors (mcx_set_error: mcx_pipeline.hip), allocation
// ---------------------------------------------------------------------------------------------
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

// (MCX_TIMING) a host wait that took long says so
template <typename F>
static inline hipError_t timed_wait(bool on, const char *what, int line, F &&f)
{
    if (!on) return f();
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = f();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms > 15) fprintf(stderr, "[mcx] %.1f ms in %s (line %d)\n", ms, what, line);
    return e;
}
extern std::atomic<size_t> g_dmalloc_bytes; // (MCX_TIMING: what a context takes)
template <class T>
static int dmalloc(T **p, size_t n, int line = __builtin_LINE(), const char *file = __builtin_FILE())
{
    HIP_TRY(hipMalloc((void **)p, n * sizeof(T)));
    g_dmalloc_bytes += n * sizeof(T);
    static const bool log = getenv("MCX_ALLOC_LOG") != nullptr;
    if (log && n * sizeof(T) >= ((size_t)256 << 20)) fprintf(stderr, "[mcx alloc] %8.2f GB at %s:%d\n", (double)(n * sizeof(T)) / 1e9, file, line);
    return 0;
}

struct PairSel {             // which pairs a launch works on
    const uint32_t *ids;     // batch pair id per local index (null: identity)
    const int32_t *est;      // EstiDistance per local index
    uint32_t n;
};

static __device__ __forceinline__ uint32_t sel_pair(const PairSel &s, uint32_t local) { return s.ids ? s.ids[local] : local; }

// (counters that many wavefronts add to sit one per 256 bytes: their atomics then run in different L2 channels instead of queueing on one line)
constexpr int kCntPad = 64;
constexpr int kDpBuckets = 1024; // shapes the problems of a long DP list are dealt by (mcx_dp_stage.hip: k_dp_sort_*)

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
// The MCX_* switches of DESIGN §3 (none changes a result), read ONCE when a context is made: nothing in the launch path asks the
// environment.  What was measured slower and served no test is gone (the heavy pairs clustered first, one DP stream per list, the
// ungrouped wavefront DP, the narrow comparison windows of the seeding walk, mate rescue a workgroup per pair for every pair).
struct Knobs {
    bool timing = false, seed_one_base = false, dp_by_wave = false, dp_lane_always = false, late_reseed = false, no_work_order = false, no_simple = false,
         simple_no_dp = false, cluster_by_lane = false, rescue_in_line = false, build_by_lane = false, no_sums_cache = false, prof_by_column = false,
         tier1_hist = false, dp_hist = false, no_tier_overlap = false, no_late_overlap = false, no_prof_overlap = false, no_prepack = false, no_tier1_grow = false, cluster_in_line = false, cluster_split = false, cluster_mem = false;
    int seed_fm_budget = 6, build_wave_limit = 0x7fffffff;
    uint32_t order_min = 16384u;
};

struct Tier {
    Caps caps;
    Layout lay;
    uint8_t *state = nullptr;
    uint32_t max_pairs = 0;
    uint32_t grow_to = 0; // the large tier: how many pair records it may grow to when a batch's heavy pairs do not fit one pass (tier1_grow; 0 = fixed)
};

enum { CNT_TASKS = 0, CNT_RESCUE = 1 * kCntPad, CNT_JOB0 = 2 * kCntPad, CNT_JOB1 = 3 * kCntPad, CNT_JOB2 = 4 * kCntPad, CNT_JOB3 = 5 * kCntPad,
       CNT_JOB4 = 6 * kCntPad, CNT_JOB5 = 7 * kCntPad, CNT_OV = 8 * kCntPad, CNT_LF = 9 * kCntPad, CNT_CELLS = 10 * kCntPad, CNT_UNSUP = 11 * kCntPad,
       CNT_QUEUE = 12 * kCntPad, CNT_EARLY = 13 * kCntPad, CNT_LATE = 14 * kCntPad, CNT_RTASK = 15 * kCntPad, CNT_RPLAN = 16 * kCntPad, CNT_RESCUE_N = 17 * kCntPad, CNT_RSEED = 18 * kCntPad,
       CNT_SIMPLE = 19 * kCntPad, CNT_EARLY_HITS = 20 * kCntPad, CNT_SIMPLE_LATER = 21 * kCntPad, CNT_SIMPLE_JOBS = 22 * kCntPad, CNT_N = 23 * kCntPad,
       // behind the counters proper, cleared with them at the start of a pass (a memset in the middle of a pass was seen to sit 1.4 ms in its queue):
       CNT_ORDER = CNT_N, CNT_DP_SORT = CNT_ORDER + 16 * kCntPad, CNT_ALL = CNT_DP_SORT + 4 * kDpBuckets,
       CNT_COPY = CNT_ORDER + 6 * kCntPad }; // what a pass copies to the host: the counters proper and the order's six class counts (mcx_pass_last_shape)
constexpr uint32_t kLateRoom = 2048; // pairs of a pass that may run over after clustering and still go through the large tier beside it

// What a pass over a selection of pairs works with besides the pair records: stream, counters, work lists, DP scratch.
// The context holds three sets — tier 0's (t0), the large tier's (t1), the late pairs' (t2) —, so that the large tier can map the
// heavy pairs of a pass (listed while the pass clusters) on a stream of its own while the rest of the pass is still under way.
struct RescueTask; struct RescueRes; struct RescuePlan; // (mcx_pipeline.hip)
struct PassRes {
    hipStream_t stream = nullptr;
    uint32_t *d_cnt = nullptr, *h_cnt = nullptr;
    uint2 *d_tasks = nullptr; uint32_t task_cap = 0;
    DpJob *d_jobs[kDpClasses] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; uint32_t job_cap[kDpClasses] = {0, 0, 0, 0, 0, 0};
    uint32_t *d_rescue = nullptr; uint32_t rescue_cap = 0;
    uint32_t *d_kscratch = nullptr; // k_rescue's scratch (not owned: a third of the context's)
    RescueTask *d_rtasks = nullptr; RescueRes *d_rres = nullptr; Hit *d_rseeds = nullptr; RescuePlan *d_rplans = nullptr; uint32_t *d_rescue_n = nullptr; // mate rescue window by window
    uint32_t rtask_cap = 0, rseed_cap = 0;
    uint8_t *d_dp_scratch[3] = {nullptr, nullptr, nullptr}; uint64_t dp_stride[3] = {0, 0, 0}; uint32_t dp_blocks[3] = {0, 0, 0};
    uint32_t *d_dp_lane = nullptr; uint32_t dp_lane_blocks = 0; // k_dp_lane2's words for the three short lists (tiny | small | half), dp_lane_blocks wavefronts each
    uint32_t *d_dp_order[2] = {nullptr, nullptr}; // the two long lists by shape (k_dp_sort_*; their bucket counts and cursors: CNT_DP_SORT)
    hipStream_t dp_stream[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; hipEvent_t dp_fork = nullptr, dp_join[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // the heavy pairs' order and clustering on dp_stream[0] beside the straight-line path (tier 0's set only): the hits are final | pass H listed its classes | its clustering is done
    hipEvent_t ev_seeded = nullptr, ev_order_h = nullptr, ev_heavy = nullptr;
    uint32_t *d_ov = nullptr; uint32_t ov_cap = 0;
    uint32_t *d_sel_ids = nullptr; int32_t *d_est = nullptr;
    hipEvent_t ev[12] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

struct BatchRun { // the batch between mcx_batch_begin and mcx_batch_end
    bool open = false, sums_valid = false, keys_out = false;
    ReadBatch rb; int paired = 0;
    uint32_t n_pairs = 0, n_chunks = 0, longest = 0; // (longest read of the batch)
    AlnRec *recs = nullptr; uint32_t *cig = nullptr; // records [n_reads]; the batch's CIGAR pool
    uint32_t cig_cap = 0, cig_words = 0;             // its capacity (MCX_CIGAR_POOL_WORDS(n_reads)) and, once the batch is closed, the words taken
    int64_t read_base = 0, mapped = 0;
    unsigned long long hs[3] = {0, 0, 0};
    std::vector<uint32_t> ok, ds; // per chunk: proper pairs; summed distance, then summed read lengths
    const uint32_t *d_ok = nullptr, *d_ds = nullptr; // ... and where they lie on the device while sums_valid (the batch's tail keeps them in its own words, mcx_batch_sums in the per-read arrays)
    const uint64_t *d_sorted_keys = nullptr; uint64_t n_keys = 0; uint32_t n_sparse_keys = 0;
    std::chrono::steady_clock::time_point t0, t_begun; double ms_setup = 0; // (t_begun, ms_setup: MCX_TIMING)
    mcx_stats *stats = nullptr;
};

struct mcx_ctx {
    const mcx_index *idx = nullptr;
    bool counted = false; // (among idx->n_ctx)
    bool lens_checked = false; // the batch about to begin holds no read longer than max_read_len (mcx_stream_next says so for batches that came as 2-bit rows)
    const uint32_t *lens_checked_off = nullptr; const uint8_t *lens_checked_bases = nullptr; // ... said of THESE buffers (the slot's) and of no others
    // ... and is packed already (mcx_stream_submit_packed packed it behind its copy in, under the batch before it): where, from which bytes, mated or not, and its any-N word
    struct PrePacked { const uint32_t *packed = nullptr; const uint8_t *bases = nullptr; int paired = 0; const uint32_t *any_n = nullptr; } pre;
    int last_paired = 1;                 // what the last batch was mapped as: the guess a batch on its way in is packed under
    const uint32_t *packed_now = nullptr; // the 2-bit form the batch in flight is mapped from (d_packed, or a slot's)
    int wpad_now = 0;                     // ... and the words from one of its rows to the next: what the batch's longest read needs, wpad at the most (a slot's rows: wpad)
    Knobs kn;
    Params pm;
    mcx_opts opts;
    Tier tier[2];
    uint64_t max_reads = 0, max_bases = 0;
    int rlen_max = 256;
    PassRes t0;               // tier 0's set of pass resources; its stream is the context's (mcx_ctx_stream)
    uint32_t *d_kscratch = nullptr; // k_rescue's scratch for reads with N: a third per set of pass resources
    hipEvent_t ev_pack[2] = {nullptr, nullptr};
    uint32_t *d_read_ext = nullptr, *d_read_blocks = nullptr;
    uint32_t *d_packed = nullptr; int wpad = 0; // 2-bit form of the batch's reads: room for rows of wpad words, what a read of max_read_len takes (a batch's own stride: wpad_now)
    uint32_t *d_order = nullptr; // the pairs of a pass by weight (k_order_*; their class counts: CNT_ORDER)
    uint8_t *d_done = nullptr;                           // per pair of a pass: k_simple wrote its records (the per-pair kernels skip it)
    uint32_t *d_sl_pairs = nullptr, *d_sl_list = nullptr; // the straight-line pairs that wait for a small gapped extension (SimpleLater)
    SimpleJob *d_sl_jobs = nullptr; SimpleRes *d_sl_res = nullptr; uint32_t sl_cap = 0;
    PairOut *d_pout = nullptr, *d_pout_sel = nullptr; // per-pair outcome of the finish stage; a gathered selection of it
    uint8_t *d_mapq = nullptr; int mapq_rows = 0;
    // -vcf bookkeeping (mcx_profile.h): caller-owned counter planes, per-read alignment detail
    uint32_t *prof_planes = nullptr; int prof_max_dup = 5, prof_max_clip = 5;
    ColItem *d_prof_items = nullptr; uint32_t prof_items_cap = 0; // fragments whose columns k_prof_cols walks
    uint16_t *d_prof_match = nullptr; bool prof_settled = false, prof_broken = false; // (broken: a settle failed half way — some planes scanned, some not)
    // exact-seed coverage as differences (mcx_profile.h); freed by mcx_profile_settle
    uint8_t *d_detail = nullptr; DetailLayout dlay;
    // One shard: a batch's bookkeeping is queued behind its mapping on a stream of its own and runs under the NEXT batch's kernels.  What the
    // mapping writes for it exists twice (detail records, flag bytes: the sets change places when a batch's bookkeeping is queued), the batch's reads are kept
    // in a copy of the context's (the caller's buffer is the caller's again when the call returns), and the bookkeeping has counters and an event list of its own.
    struct ProfLater {
        bool have = false, tried = false, pending = false, kept_now = false; // the resources exist; a batch's bookkeeping is queued and the host has not looked at its counts; the batch in flight has its reads kept
        hipStream_t stream = nullptr, keep_stream = nullptr; hipEvent_t go = nullptr, done = nullptr, kept = nullptr, begun = nullptr;
        uint8_t *d_detail_alt = nullptr, *d_admit_alt = nullptr, *d_keep_bases = nullptr, *d_keep_bases_alt = nullptr; uint32_t *d_keep_off = nullptr, *d_keep_off_alt = nullptr;
        uint32_t *d_cnt = nullptr, *h_cnt = nullptr; SparseRec *d_ev = nullptr; uint32_t ev_cap = 0;
        std::chrono::steady_clock::time_point t_queued;
    } later;
    uint64_t *d_keys[2] = {nullptr, nullptr}; uint8_t *d_admit = nullptr; void *d_sort_tmp = nullptr; size_t sort_tmp_bytes = 0;
    SparseRec *d_sparse = nullptr; uint32_t sparse_cap = 0;
    struct Archive { SparseRec *d = nullptr; uint64_t n = 0, cap = 0; std::vector<mcx_sparse_rec> *host = nullptr; };
    Archive arch, arch_ev;                      // the tally records / discordant-pair events of the batches so far, still in HBM
    uint64_t arch_limit = (uint64_t)1 << 28;    // (at most 16 GB)
    SparseRec *h_sparse_pin = nullptr; uint32_t sparse_pin_recs = 1u << 18; // page-locked bounce buffer for their way to the host (16 MB)
    std::vector<mcx_sparse_rec> h_sparse, h_events; // tallies (followed by what the last mcx_profile_sparse* call appended for its caller: n_tally is where that starts); discordant-pair events ('E')
    size_t n_tally = 0;
    uint64_t keys_cap = 0;       // keys the sort buffers hold
    uint64_t *h_keys = nullptr; uint64_t h_keys_cap = 0; // pinned: the batch's keys for the exchange between shards
    // the tail of a whole-batch pass queued behind its kernels, before the host waits for them (mcx_map_batch_dev: queue_batch_tail) — the
    // seeding statistics, the per-chunk sums, the insert-size walk over them and the check of every pair's estimate, one copy back
    struct Tail {
        bool want = false, queued = false, ran = false; // asked for by the caller of this batch; queued by its pass and still standing; queued at all
        int64_t state0[3] = {1000, 0, 0};      // avgDist, pairs, distance sum before the batch
        uint32_t *d = nullptr;                 // device: [0..8) counters (n_redo, mapped), [8..8 + nc) the chunks' estimates
        uint32_t *h = nullptr; uint32_t cap = 0; // page-locked: counters[8] | flags[4] | statistics (3 x u64) | ok[nc] ds[nc] ls[nc] est[nc]
        hipEvent_t ev[2] = {nullptr, nullptr};
    } tail;
    uint32_t *d_batch_flags = nullptr; // [0] words taken in the batch's CIGAR pool, [1] longest read of the batch, [2] the pool ran over, [3] a read holds an N
    BatchRun run;
    PassRes t1;               // the large tier's own set; allocated when every suffix-array entry is resident
    bool overlap_tiers = false;
    bool dp_grown = false; // dp_scratch_grow() has had its one attempt
    uint32_t job2_seen = 0; // the longest 65-256-column DP list of a tier-0 pass so far
    volatile uint32_t *h_early = nullptr; uint32_t *d_early = nullptr; // page-locked words k_publish_early writes behind the clustering kernel: the host's view and the device's
    PassRes t2;               // a third set: the large tier's pass over the pairs that ran over after clustering (k_build's list)
    hipEvent_t ev_built = nullptr, ev_late_done = nullptr;
    bool overlap_late = false;
    hipEvent_t ev_clustered = nullptr;
    bool light_fit = false;       // light_pairs_fit(tier 0's capacities): asked once, where the capacities are made
    bool regs_fit = false;        // packed_hits_fit(the index's text length, max_read_len): k_cluster may keep a read's seeds in registers (asked once, where the context is made)
    bool aside_pays = true;       // the last large tier-0 pass had a straight-line path for the heavy pairs' clustering to hide behind (pass_finish: kAsideGatePairs)
    uint32_t last_shape[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // mcx_pass_last_shape: the last tier-0 pass
    // mcx_stream_*: three batches in flight (copy in | kernels | copy out), each in a slot of its own
    struct Slot {
        uint8_t *d_bases = nullptr; uint32_t *d_off = nullptr; AlnRec *d_recs = nullptr; uint32_t *d_cig = nullptr;
        mcx_aln32 *d_recs32 = nullptr; // the records in 32 bytes each for their way out (mcx_stream_mapped32)
        uint32_t *d_codes = nullptr, *d_len = nullptr, *d_err = nullptr; uint64_t *d_odd = nullptr; uint32_t odd_cap = 0; // mcx_stream_submit_packed: what arrives; restored to d_bases / d_off
        uint32_t n_reads = 0; int state = 0; uint64_t seq = 0; // 0 free, 1 copy in started, 2 handed to the kernels, 3 copy out started
        bool lens_checked = false; // the batch came as 2-bit rows: no read is longer than the context's slots (k_unpack_reads / k_neutralize saw to it)
        uint32_t *h_err = nullptr; // pinned: d_err's word on its way out with the batch's records (mcx_stream_mapped / _mapped32 -> mcx_stream_collect)
        uint32_t *d_prepack = nullptr, *d_any_n = nullptr; bool prepacked = false; int pre_paired = 0; // k_pack_reads' output made on the way in
        hipEvent_t in_ready = nullptr, mapped = nullptr, out_done = nullptr;
        // -m: the batch's extras on their way out with its records (slot_multi_out): in read order, the records as mcx_aln32
        struct Extras {
            bool have = false; uint32_t n_reads = 0, n_recs = 0, n_words = 0;
            uint32_t *d_index = nullptr, *d_cig = nullptr; mcx_aln32 *d_recs = nullptr; uint32_t rec_cap = 0, word_cap = 0;
            uint32_t *h_index = nullptr, *h_cig = nullptr; mcx_aln32 *h_recs = nullptr; uint32_t h_rec_cap = 0, h_word_cap = 0;
        } mx;
    } slot[3];
    const Slot *collected = nullptr; // the slot mcx_stream_collect handed over last (mcx_stream_multi)
    hipStream_t h2d_stream = nullptr, d2h_stream = nullptr;
    uint64_t stream_seq = 0, stream_bytes_in = 0, stream_bytes_out = 0;
    void *d_scan_tmp = nullptr; size_t scan_tmp_bytes = 0; // the prefix sum of the read lengths (mcx_stream_submit_packed)
    void *files_state = nullptr; void (*files_drop)(void *) = nullptr; // mcx_files.cpp's batch buffers (mcx_ctx_files_slot)
    void *sam_state = nullptr; void (*sam_drop)(void *) = nullptr;     // mcx_sam.hip's device buffers (mcx_ctx_sam_slot)
    // staging for the host-buffer entry point
    uint8_t *d_bases = nullptr; uint32_t *d_off = nullptr; AlnRec *d_recs = nullptr; uint32_t *d_cig = nullptr;
    // -m (mcx_ctx_set_multi): the extras pool k_finish<true> fills, and the last batch's extras in read order (multi_close)
    struct Multi {
        bool on = false, ready = false;
        uint32_t rec_cap = 0, word_cap = 0;            // the pool's
        AlnRec *d_pool = nullptr; uint32_t *d_pool_cig = nullptr; uint32_t *d_cnt = nullptr; uint4 *d_ref = nullptr;
        uint32_t *d_counts = nullptr;                  // records | words per read, [2][max_reads + 1], scanned into d_index | d_windex
        uint32_t *d_index = nullptr, *d_windex = nullptr;
        AlnRec *d_out = nullptr; uint32_t *d_out_cig = nullptr; uint32_t out_cap = 0, out_wcap = 0;
        void *d_tmp = nullptr; size_t tmp_bytes = 0;
        uint32_t n_reads = 0, n_recs = 0, n_words = 0;  // the last batch's
    } mx;
};

// ---------------------------------------------------------------------------------------------
// the host functions that cross a unit boundary
// ---------------------------------------------------------------------------------------------
// mcx_pipeline.hip
int reserve_tier0(mcx_ctx *c, int paired, uint64_t n_reads);
void pack_reads(const ReadBatch &rb, int paired, int wpad, int tpr, uint32_t *out, uint32_t *any_n, uint8_t *odd_flag, hipStream_t s);
// mcx_dp_stage.hip
int launch_dp(const Knobs &kn, const PassRes &R, const Ctx &cx, const JobSinks &sinks, const ReadBatch &rb, const PairSel &sel, int rlen_max);
uint64_t lane_short_words(int which);
uint64_t lane_stride_words(bool nw, int rows, int strips);
// mcx_profile.hip
int profile_keys(mcx_ctx *c);
int profile_queue(mcx_ctx *c);
int profile_collect(mcx_ctx *c);
int archive_append(mcx_ctx *c, mcx_ctx::Archive &a, const SparseRec *d_src, uint64_t n, hipStream_t on = nullptr);
int profile_foreign(mcx_ctx *c, const uint64_t *h_all, uint64_t n_all);
int sort_reserve(mcx_ctx *c, uint64_t n);
int profile_accumulate(mcx_ctx *c, const uint64_t *h_all, uint64_t n_all, uint32_t slot_stride, uint32_t own_slot);

#endif
