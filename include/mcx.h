/* include/mcx.h — C ABI of the MI355X seed-and-extend path (libmcx.so).
 *
 * MapCaller has no plugin/FFI interface: its seam is the set of extern C++ functions of
 * reference src/structure.h:223-292 that the mapping driver calls.  This header is the batch
 * C ABI that replaces them; each entry point names the reference interface it stands in for.
 * Plain pointers and sizes only — no C++ or torch types.  INTEGRATION.md shows the shims with
 * the reference's own signatures (BWT_Search, nw_alignment, ksw2_alignment) built on top.
 *
 * Conventions: functions return 0 on success and a negative mcx_status otherwise;
 * mcx_last_error() gives a message.  A context is bound to one GPU and one host thread.
 * Pointers named d_* are device (HBM) pointers, everything else is host memory.
 */
#ifndef MCX_H
#define MCX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcx_index mcx_index;
typedef struct mcx_ctx mcx_ctx;

enum mcx_status {
    MCX_OK = 0,
    MCX_ERR_IO = -1,        /* index or read file missing / truncated */
    MCX_ERR_ARG = -2,
    MCX_ERR_DEVICE = -3,    /* HIP runtime error (no GPU, out of memory, launch failure) */
    MCX_ERR_CAPACITY = -4,  /* a pair exceeded the hard capacities of the last tier */
    MCX_ERR_UNSUPPORTED = -5
};

const char *mcx_last_error(void);
int mcx_device_count(void);

/* ---- index ------------------------------------------------------------------------------
 * Replaces bwa_idx_load + RestoreReferenceInfo (reference src/bwt_index.cpp:150-258, called
 * from src/main.cpp:350-361): parses <prefix>.bwt/.sa/.pac/.ann/.amb (the byte-compatible BWA
 * files `MapCaller index` writes) and stages them in HBM.  full_sa != 0 additionally expands
 * the 1-in-32 sampled suffix array to every row on the GPU (bwt_sa then is one 8-byte gather) and
 * derives the seeding walk's jump table and rank records; full_sa = 2 adds the pair
 * records — BWT_Search's extension (src/bwt_search.cpp:128-151) two bases per step, 4 bytes per text
 * position (25 GB for a human genome): same searches, fewer fetches. */
#define MCX_INDEX_SAMPLED 0
#define MCX_INDEX_FULL 1
#define MCX_INDEX_PAIRS 2
#define MCX_INDEX_PAIRS_IF_ROOM 3 /* the pair records when the device has room for them; else MCX_INDEX_FULL with one line on stderr */
int mcx_index_load(const char *prefix, int device, int full_sa, mcx_index **out);
/* Gives back what the index holds above the level `full_sa` (MCX_INDEX_FULL: the pair records), e.g. before the
 * alignment profile's planes are attached.  Refused (MCX_ERR_ARG) while a context of the index is alive. */
int mcx_index_trim(mcx_index *, int full_sa);
/* Replaces bwa_idx_build (reference src/BWT_Index/bwtindex.c:77; `MapCaller index ref.fa prefix`,
 * src/main.cpp:199-207): builds BWT/occ/SA on the GPU from a FASTA file and writes the same
 * five files. */
int mcx_index_build(const char *fasta_path, const char *prefix, int device);
/* The same construction for a genome that already sits in HBM (one code 0..3 per byte, contigs
 * concatenated): builds the index in place, no files.  mcx_index_save writes the five files. */
int mcx_index_from_codes(const uint8_t *d_codes, int32_t n_chr, const int32_t *chr_len, const char *const *chr_name,
                         int device, int full_sa, mcx_index **out, double *build_seconds);
int mcx_index_save(const mcx_index *, const char *prefix);
/* Releases the index's HBM at once.  Contexts of the index that are still alive must not map any more; freeing them afterwards is allowed (the index's
 * host object stays until the last of them is gone). */
void mcx_index_free(mcx_index *);
int64_t mcx_index_genome_size(const mcx_index *);
int32_t mcx_index_n_chr(const mcx_index *);
const char *mcx_index_chr_name(const mcx_index *, int32_t i);
int32_t mcx_index_chr_len(const mcx_index *, int32_t i);
int64_t mcx_index_hbm_bytes(const mcx_index *);

/* ---- options: the reference's globals that steer the path (src/main.cpp:159-191) ---------- */
typedef struct mcx_opts {
    int32_t alg;             /* 0 = nw (default, NW_ALG main.cpp:166), 1 = ksw2 (-alg) */
    int32_t max_pos_diff;    /* MaxPosDiff, -indel, default 30 */
    float max_mismatch_rate; /* MaxMisMatchRate, -maxmm, default 0.05 */
    int32_t max_read_len;    /* longest read the context must hold (default 256) */
    int64_t max_batch_reads; /* reads per batch the context is sized for */
} mcx_opts;
void mcx_opts_default(mcx_opts *);

/* A context's HBM: what mcx_ctx_create takes (itemised on stderr with MCX_ALLOC_LOG=1), tier 0's pair records with the first batch, and — only while more
 * than 16 GB of the device stay free after it — two growths on demand, each said on stderr under MCX_ALLOC_LOG / MCX_TIMING: the large tier's pair records
 * when a batch sends it more pairs than one pass holds (3 KB per read of the batch to start with, 2-24 GB; up to 262144 pairs), and the scratch of the
 * 65-256-column DP list after a batch that fills it (4 GB -> at most 12 GB, once).  MCX_NO_TIER1_GROW=1 keeps both as created; a size asked for with
 * MCX_TIER1_GB is kept too.  Results do not depend on either (tests/test_gpu_parity.py: the SAM of a run that grows equals one that does not). */
int mcx_ctx_create(const mcx_index *, const mcx_opts *, mcx_ctx **out);
/* The same with everything the run will take from the device taken at once — the context, tier 0's pair records (otherwise allocated by the first batch),
 * and with_profile != 0: the counter planes (mcx_planes_alloc -> *planes; free with mcx_planes_free) and the bookkeeping's buffers (mcx_profile_attach with
 * max_dup / max_clip) — and, when that leaves less than 4 GB of HBM, degraded in a fixed order until it fits, each step said on stderr: the index gives its
 * pair records back (mcx_index_trim), then max_batch_reads is halved, repeatedly (whole 200-read chunks, down to 128 K reads).  *fit (may be NULL) says
 * what was done; the caller cuts its run into batches of fit->max_batch_reads.  paired: the run's batches are read pairs (half the pair records).
 * Replaces the reference's `new MappingRecord_t[GenomeSize]` (main.cpp:366-370), which has the host's memory to fall back on. */
typedef struct mcx_fit {
    int32_t pair_records_trimmed; /* 1: mcx_index_trim was applied */
    int32_t batch_halvings;       /* how often max_batch_reads was halved */
    int32_t single_detail_set;    /* 1: no second set of detail records — a batch's -vcf bookkeeping runs inside its call */
    int32_t pad;
    int64_t max_batch_reads;      /* what the context was made for */
    int64_t hbm_free_bytes;       /* free HBM with everything allocated */
    int64_t hbm_taken_bytes;      /* what the run's allocations took (context, pair records of tier 0, planes, bookkeeping) */
} mcx_fit;
int mcx_ctx_create_fit(mcx_index *, const mcx_opts *, int with_profile, int paired, int max_dup, int max_clip, mcx_ctx **out, uint32_t **planes, mcx_fit *fit);
void mcx_ctx_free(mcx_ctx *);

/* ---- per-call drop-ins ------------------------------------------------------------------
 * BWT_Search (reference src/bwt_search.cpp:121, declared src/structure.h:279; only caller
 * src/ReadMapping.cpp:138).  seqs: n concatenated code strings (0..4), seq_off[n+1]; each is
 * searched from start[i] to its end.  len/freq: n each; loc: n*50 (freq[i] entries used). */
int mcx_bwt_search_batch(mcx_ctx *, const uint8_t *seqs, const uint32_t *seq_off, const int32_t *start, uint32_t n,
                         int32_t *len, int32_t *freq, uint64_t *loc);
/* Test entry: the greedy seeding walk of one read (IdentifySimplePairs' loop, reference src/ReadMapping.cpp:133-150, before its
 * PosDiff filter) as the batch pipeline's seeding kernel runs it — the same device functions in the same phase loop, on whatever
 * the index holds (jump table, rank records, pair records, full or sampled suffix array) — for n reads in host memory.  seqs: the
 * reads' ASCII bases as mcx_map_batch takes them, concatenated, seq_off[n + 1]; no read is reverse-complemented.  fm_budget >= 1:
 * FM steps a search takes per turn of the loop (the pipeline's resumable shape; results do not depend on it).  hits: n * cap
 * records, read i's first min(n_hits[i], cap) at hits + i * cap in the order the walk finds them (a search's rows in suffix
 * order), gPos a text position in [0, 2G); n_hits[i] counts past cap, as the kernel's own counter does. */
typedef struct mcx_seed_hit { int64_t gPos; int32_t rPos; int32_t len; } mcx_seed_hit;
int mcx_seed_walk_batch(mcx_ctx *, const uint8_t *seqs, const uint32_t *seq_off, uint32_t n, int fm_budget, uint32_t cap,
                        int32_t *n_hits, mcx_seed_hit *hits);
/* nw_alignment / ksw2_alignment (reference src/nw_alignment.cpp:18, src/ksw2_alignment.cpp:250;
 * declared src/structure.h:289,292; called from src/ReadAlignment.cpp:186-187).  q = read
 * fragments, t = genome fragments (ASCII), concatenated with offset arrays of n+1 entries.
 * ops receives, for job i, ops_len[i] column codes 'M' (base/base), 'I' ('-' in the genome
 * string) and 'D' ('-' in the read string) at ops + (q_off[i] + t_off[i]); score[i] is
 * ez.score of ksw_extz2_sse for ksw2 and 2x the final s for nw. */
int mcx_extend_batch(mcx_ctx *, int alg, const uint8_t *q, const uint32_t *q_off, const uint8_t *t,
                     const uint32_t *t_off, uint32_t n, uint8_t *ops, int32_t *ops_len, int32_t *score);
/* The same problems through the forms the batch pipeline runs its long DP lists on, in the caller's order: form 1 = one problem per
 * lane (lane l of group g takes problem 64 g + l), form 2 = two per lane in 16-bit halves (problem 128 g + 2 l in the low half,
 * 128 g + 2 l + 1 in the high one); strip = 8 or 16 target columns per strip; blocks = wavefronts launched (0: one per group; fewer
 * than there are groups: a wavefront takes several groups one after the other in the same scratch).  alg: 0 nw, 1 ksw2.  ops, ops_len
 * as mcx_extend_batch; score[i] is 2x the final s for nw and 0 for ksw2; summaries: null, or room for n records of 64 bytes (the
 * pipeline's per-problem summary of the column string: csrc/mcx_types.h DpSummary, with cols_off = the two lengths' sum less
 * cols_len).  MCX_ERR_UNSUPPORTED for a target letter outside ACGT, a target longer than 256 bases (64 with strips of 8), a query longer
 * than 2048, an empty string, another form or strip. */
int mcx_extend_lanes(mcx_ctx *, int alg, int form, int strip, uint32_t blocks, const uint8_t *q, const uint32_t *q_off, const uint8_t *t,
                     const uint32_t *t_off, uint32_t n, uint8_t *ops, int32_t *ops_len, int32_t *score, void *summaries);

/* ---- the whole path -----------------------------------------------------------------------
 * One record per read: what GeneratePairedSamStream / GenerateSingleSamStream print
 * (reference src/SamReport.cpp:324-488) in the default unique mode. */
typedef struct mcx_aln {
    int64_t pos;       /* POS, 1-based; 0 = unmapped */
    int64_t mate_pos;  /* PNEXT */
    int32_t chr;       /* RNAME index, -1 = '*' */
    int32_t flag;      /* FLAG */
    int32_t mapq;      /* MAPQ */
    int32_t tlen;      /* TLEN */
    int32_t nm, as, xs;/* NM:i AS:i XS:i */
    int32_t n_cigar;   /* CIGAR operations: len << 4 | op, M=0 I=1 D=2 S=4 */
    int32_t fwd;       /* 0: SEQ/QUAL are printed reverse-complemented / reversed */
    int32_t has_mate;  /* RNEXT '=' */
    int32_t cigar_off; /* word offset of the read's first operation in the batch's CIGAR pool */
    int32_t pad;       /* 64-byte records */
} mcx_aln;

/* The same record in 32 bytes, for the way out of HBM (mcx_stream_map32 / mcx_stream_mapped32): at 64 bytes a read the copy of a
 * batch's records outlasts the part of the next batch's step in which the host has nothing to wait for, and every wait behind it takes
 * milliseconds (the device boundary).  Positions below 2^40, at most 65 535 contigs, reads of up to 1000 bases:
 * the path's own limits.  mcx_aln_unpack gives the 64-byte form back. */
typedef struct mcx_aln32 {
    uint32_t pos_lo, mate_lo;   /* POS, PNEXT: low 32 bits */
    uint8_t pos_hi, mate_hi;    /* ... bits 32-39 */
    uint8_t mapq;
    uint8_t bits;               /* 1: fwd, 2: has_mate */
    int32_t tlen;
    uint16_t flag;
    uint16_t chr;               /* 0xFFFF = '*' */
    int16_t nm, as, xs;
    uint16_t n_cigar;
    uint32_t cigar_off;
} mcx_aln32;
static inline void mcx_aln_unpack(const mcx_aln32 *p, mcx_aln *o)
{
    o->pos = (int64_t)p->pos_lo | ((int64_t)p->pos_hi << 32); o->mate_pos = (int64_t)p->mate_lo | ((int64_t)p->mate_hi << 32);
    o->chr = p->chr == 0xFFFFu ? -1 : (int32_t)p->chr; o->flag = p->flag; o->mapq = p->mapq; o->tlen = p->tlen;
    o->nm = p->nm; o->as = p->as; o->xs = p->xs; o->n_cigar = p->n_cigar; o->fwd = p->bits & 1; o->has_mate = (p->bits >> 1) & 1;
    o->cigar_off = (int32_t)p->cigar_off; o->pad = 0;
}

typedef struct mcx_stats {
    int64_t reads, mapped, pairs, pair_dist_sum;
    int64_t pair_len_sum;   /* ReadLengthSum: bases of the reads counted in `pairs` (ReadMapping.cpp:529-530) */
    int64_t fm_ext_steps;   /* E of SURVEY.md §8d: sum of BWT_Search lengths */
    int64_t fm_blocks;      /* index records the extension walk fetched: 16-byte rank records (64-byte .bwt blocks without the full suffix array) */
    int64_t sa_hits;        /* H: suffix-array hits resolved */
    int64_t dp_jobs, dp_cells;
    int64_t tier1_pairs;    /* pairs re-run with the large capacities */
    int64_t replayed_pairs; /* pairs re-run because the avgDist trajectory moved past their validity interval */
    int64_t halved_selections; /* times a selection of pairs was mapped in two halves because a work list ran over */
    int64_t simple_pairs;   /* pairs (reads, single-end) that went from their seeds to their records on the straight-line path (k_simple) */
    double ms_encode /* k_pack_reads */, ms_seed, ms_sa, ms_cluster /* the pass's stream from the order's end to the rescue fork: k_cluster (with the heavy pairs aside: the light pairs' launch and whatever wait for the heavy side is left) */, ms_rescue, ms_build, ms_dp, ms_finish, ms_total;
    double ms_simple;       /* the straight-line path: k_simple (collect), k_simple_dp, k_simple (replay) */
    double ms_order;        /* k_order_count + k_order_place */
} mcx_stats;

#define MCX_CIGAR_STRIDE 32 /* CIGAR words per read a batch's pool has room for on average ... */
#define MCX_CIGAR_SLACK 65536 /* ... plus this many: a batch of a few reads with long CIGARs (or re-run pairs, which take fresh words) still fits */
#define MCX_CIGAR_POOL_WORDS(n_reads) ((size_t)(n_reads) * MCX_CIGAR_STRIDE + MCX_CIGAR_SLACK) /* the capacity every d_cigar / cigar argument must have */

/* Replaces the body of ReadMapping() for one batch (reference src/ReadMapping.cpp:416-646):
 * seeding, clustering, pairing, rescue, extension, scoring, flags/MAPQ/CIGAR.  d_bases: ASCII
 * reads in HBM (16-byte aligned, readable up to 32 bytes past the last base: whole 16-byte words
 * are fetched), d_off: n_reads+1 byte offsets (device), paired: mates interleaved.
 * avg_state[4] carries the reference's running insert-size estimate across batches
 * {avgDist, iTotalPairedNum, TotalPairedDistance, reads seen} (ReadMapping.cpp:20-21,:538-539);
 * initialise with mcx_avg_init.  Results (device): d_aln[n_reads] and the batch's CIGAR pool d_cigar
 * (capacity MCX_CIGAR_POOL_WORDS(n_reads) words): the operations of read r are the n_cigar words from
 * d_cigar[d_aln[r].cigar_off] on.  The pool is filled by wavefronts in no particular order (offsets differ
 * from run to run, contents do not); mcx_cigar_words tells how many of its words the last batch took —
 * all a copy to the host has to move. */
void mcx_avg_init(int64_t avg_state[4]);
int mcx_map_batch_dev(mcx_ctx *, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired,
                      int64_t avg_state[4], mcx_aln *d_aln, uint32_t *d_cigar, mcx_stats *stats);
int mcx_cigar_words(mcx_ctx *, uint32_t *n_words);
/* same with host buffers (pinned staging inside) */
int mcx_map_batch(mcx_ctx *, const uint8_t *bases, const uint32_t *off, uint32_t n_reads, int paired,
                  int64_t avg_state[4], mcx_aln *aln, uint32_t *cigar, mcx_stats *stats);

/* -m (MapCaller's bUnique = false): a read whose best score is held by several candidates gets a SAM line for
 * each of them, in candidate order.  The first is the record above, as in unique mode; the others ("extras")
 * come apart from the fixed one-record-per-read output.  on: the mode for the context's following batches.
 * extra_cap: the initial capacity of the device's extras pool in lines (0: a default); a batch that needs
 * more makes the pool grow (MCX_ALLOC_LOG says so) and no line is ever dropped.  The profile (-vcf) does not
 * change.  A batch that maps single-end reads gives the later lines FLAG 0 or 16 by strand. */
int mcx_ctx_set_multi(mcx_ctx *, int on, uint32_t extra_cap);
/* The extras of the batch the last mapping call mapped (mcx_map_batch_dev / mcx_map_batch / mcx_stream_map*
 * / mcx_batch_end*), in HBM and in read order: the lines of read r are d_recs[d_index[r] .. d_index[r + 1])
 * (d_index has n_reads + 1 entries); a record's cigar_off points into d_cigar.  Valid until the next batch
 * of the context begins. */
int mcx_multi_lines(mcx_ctx *, const uint32_t **d_index, const mcx_aln **d_recs, const uint32_t **d_cigar, uint32_t *n_recs, uint32_t *n_words);
/* the same copied to host memory: index[n_reads + 1], recs[n_recs], cigar[n_words] (sizes from mcx_multi_lines) */
int mcx_multi_copy(mcx_ctx *, uint32_t *index, mcx_aln *recs, uint32_t *cigar);

/* ---- batches from host memory with the copies overlapped with the kernels -------------------------
 * The device boundary of the drop-in: reads arrive in (pinned) host memory, records leave to (pinned)
 * host memory.  Three batches are in flight, each in a slot of HBM of its own: one being copied in on a
 * copy stream, one under the kernels, one being copied out on another copy stream.
 *   mcx_stream_submit   starts the copy of a batch to HBM and returns at once
 *   mcx_stream_map      maps the oldest submitted batch (like mcx_map_batch_dev: the host thread drives
 *                       the kernels), then starts the copy of its records to aln / cigar
 *   mcx_stream_collect  waits until the oldest mapped batch has arrived in host memory
 * so the loop  submit(i+1); map(i); collect(i-1)  keeps PCIe busy in both directions under the kernels.
 * mcx_stream_next / mcx_stream_mapped are mcx_stream_map in two halves for callers that map the batch
 * in steps (mcx_batch_*): the first hands out the batch's place in HBM, the second starts the copy out.
 * bytes_in / bytes_out (may be NULL): bytes moved over the boundary so far. */
int mcx_stream_submit(mcx_ctx *, const uint8_t *bases, const uint32_t *off, uint32_t n_reads);
/* The same with the reads as a host parser packs them — a quarter of the bytes over PCIe: read r has len[r] bases, its 2-bit codes
 * (A 0, C 1, G 2, T 3; sixteen bases to a word, the first in the top bits) are the words codes[r * row_words ..]; every byte of
 * a read that is not one of the upper-case letters ACGT is listed in `odd` as (read << 32 | position << 8 | byte) and has
 * code 0 in the row.  The device restores the ASCII bytes exactly (mcx_stream_next hands out the same d_bases / d_off as after
 * mcx_stream_submit), so nothing downstream can tell the two apart.  row_words >= ceil(longest read / 16).
 * DEFERRED ERROR: the lengths are checked on the device by the kernel that restores the bytes (no wait at the start of the step).  A batch with a read longer
 * than its row / max_read_len, or with more bases than the slot holds, is mapped as n_reads EMPTY reads (every record unmapped) and refused after the fact with
 * MCX_ERR_ARG: by mcx_stream_map / mcx_stream_map32 when they return, and — for the two-half form mcx_stream_next + mcx_map_batch_dev / mcx_batch_* +
 * mcx_stream_mapped / _mapped32 — by the mcx_stream_collect that hands the batch's records over (the slot is released either way; its records are not results). */
int mcx_stream_submit_packed(mcx_ctx *, const uint32_t *codes, uint32_t row_words, const uint32_t *len, uint32_t n_reads, const uint64_t *odd,
                             uint32_t n_odd);
/* The same with the three arrays in HBM already, on the context's device — what mcx_fastq_parse_dev's rows / len / odd are: the copies into the slot are
 * device-to-device on the slot's copy-in stream, everything behind them (the bytes restored, the lengths checked, the deferred error, mcx_stream_next / _map /
 * _map32 / _collect, the -m extras) is mcx_stream_submit_packed's.  bytes_in does not count such a batch: nothing of it crossed the device boundary.
 * The call returns at once.  THE CALLER'S BUFFERS must hold their contents — written and complete when the call is made: the copies do not wait for any
 * stream of the caller's — until mcx_stream_next / mcx_stream_map / mcx_stream_map32 has handed the batch out. */
int mcx_stream_submit_dev(mcx_ctx *, const uint32_t *d_codes, uint32_t row_words, const uint32_t *d_len, uint32_t n_reads, const uint64_t *d_odd,
                          uint32_t n_odd);
/* One read's row for mcx_stream_submit_packed, the way the file front end makes it (host code, no device involved; sixteen bases at a time where the
 * CPU has BMI2): row[0 .. row_words) written, the read's bytes that are not upper-case ACGT appended to odd[*n_odd ..] as (read << 32 | position << 8 | byte)
 * while *n_odd < odd_cap.  Returns how many such bytes the read holds (more than were room for: the caller's list was too short). */
uint32_t mcx_pack_row(const uint8_t *seq, uint32_t rlen, uint32_t read, uint32_t *row, uint32_t row_words, uint64_t *odd, uint32_t odd_cap, uint32_t *n_odd);
/* The CPUs the host side counts on when it sizes its thread pools: the affinity mask, cut by the cgroup's CPU-time share (cpu.max / cfs_quota) — not the
 * machine's hardware threads; MCX_HOST_CPUS=n overrides. */
uint32_t mcx_host_cpus(void);
/* The file front end's reader for ordinary .gz input by itself (replaces gzGetNextChunk's gzgets, src/GetData.cpp:101-146, for plain gzip streams): the stream is
 * cut into stretches of stretch_bytes compressed bytes (0: 2 MB), block starts are searched for in them, `threads` stretches are inflated side by side and the
 * 32 KB windows between them filled in afterwards (mapcaller_amd/csrc/mcx_pgz.h).  The text goes to out[0 .. cap) as far as it fits (out may be NULL); returns
 * its whole length, -1 when the file cannot be read or is no gzip file, -2 when the stream is damaged (*n_out: the bytes delivered before that). */
int64_t mcx_gz_inflate(const char *path, int threads, uint64_t stretch_bytes, uint8_t *out, uint64_t cap, uint64_t *n_out);
int mcx_stream_map(mcx_ctx *, int paired, int64_t avg_state[4], mcx_aln *aln, uint32_t *cigar, mcx_stats *stats);
int mcx_stream_collect(mcx_ctx *, uint64_t *bytes_in, uint64_t *bytes_out);
/* -m (mcx_ctx_set_multi): the extras of the batch the last mcx_stream_collect handed over, which came to host memory with its
 * records (packed to mcx_aln32 on the device, counted in bytes_out): index[n_reads + 1], recs[n_recs] (cigar_off into cigar),
 * cigar[n_words], as mcx_multi_lines describes them.  The buffers are the slot's, page-locked, and hold until a batch is mapped in
 * that slot again (at the earliest by the second mcx_stream_map* / mcx_stream_mapped* call after the collect).  n_reads = 0: the
 * batch carried none. */
int mcx_stream_multi(mcx_ctx *, const uint32_t **index, const mcx_aln32 **recs, const uint32_t **cigar, uint32_t *n_reads, uint32_t *n_recs, uint32_t *n_words);
int mcx_stream_next(mcx_ctx *, const uint8_t **d_bases, const uint32_t **d_off, uint32_t *n_reads, mcx_aln **d_aln, uint32_t **d_cigar);
int mcx_stream_mapped(mcx_ctx *, mcx_aln *aln, uint32_t *cigar);
/* mcx_stream_map / mcx_stream_mapped with the records leaving HBM in 32 bytes each (packed on the device, half the bytes across PCIe) */
int mcx_stream_map32(mcx_ctx *, int paired, int64_t avg_state[4], mcx_aln32 *aln, uint32_t *cigar, mcx_stats *stats);
int mcx_stream_mapped32(mcx_ctx *, mcx_aln32 *aln, uint32_t *cigar);

/* ---- a batch in steps: runs whose batches are mapped by several GPUs ---------------------------
 * The reference re-estimates the insert size after every 200-read chunk (ReadMapping.cpp:462,
 * :538-539), one trajectory over the whole input stream.  mcx_map_batch* walks it within a batch;
 * when consecutive batches are mapped by different GPUs the trajectory has to be walked over all of
 * them, so the batch is exposed in steps and the caller exchanges the per-chunk sums between them:
 *   mcx_batch_begin   maps every pair with EstiDistance est0 (the best guess at hand)
 *   mcx_batch_sums    per chunk of 100 pairs: proper pairs, their summed distance and read lengths
 *                     (host arrays, valid until the next call on the context)
 *   mcx_batch_replay  est_chunk[k] = the EstiDistance the single-stream run uses for chunk k: pairs
 *                     whose outcome depends on the difference are mapped again; n_redone = how many.
 *                     Repeat sums -> replay until no shard re-ran a pair.
 *   mcx_batch_end     closes the batch (long-CIGAR pool, -vcf bookkeeping with local admission)
 * read_base = reads of the run that precede this batch in input order (orders the discordant-pair
 * events of mcx_profile_sparse across shards; must be even for paired batches). */
int mcx_batch_begin(mcx_ctx *, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired, int32_t est0,
                    int64_t read_base, mcx_aln *d_aln, uint32_t *d_cigar, mcx_stats *stats);
int mcx_batch_sums(mcx_ctx *, uint32_t *n_chunks, const uint32_t **pairs, const uint32_t **dist, const uint32_t **len);
int mcx_batch_replay(mcx_ctx *, const int32_t *est_chunk, uint32_t *n_redone, mcx_stats *stats);
int mcx_batch_end(mcx_ctx *, mcx_stats *stats);
/* The reference's walk itself (ReadMapping.cpp:538-539): state = {avgDist, iTotalPairedNum,
 * TotalPairedDistance}; fills est_chunk[0..n_chunks) with the EstiDistance each chunk is mapped
 * with and advances the state over the chunks. */
void mcx_avg_walk(int64_t state[3], const uint32_t *pairs, const uint32_t *dist, uint32_t n_chunks, int32_t *est_chunk);
/* The same feedback with nothing but TOTALS between the shards of a run (24 bytes a shard and round instead of its per-chunk
 * sums): the walk has a closed form — the estimate before a chunk is the round's starting one, or, once more than 1000 proper
 * pairs lie before the chunk, the rounded mean distance over everything before it — so a shard needs of the shards before
 * it (in input order) only how many proper pairs they held and at which summed distance.
 *   mcx_batch_totals  {proper pairs, summed distance} of the batch as it stands
 *   mcx_batch_check   state_before = {avgDist at the round's start, pairs and distance before this batch's first chunk (the
 *                     round's starting totals + those of the shards before this one)}; first_of_round: the batch is the
 *                     round's first (its first chunk takes avgDist as it is).  The chunks' estimates are made on the device,
 *                     the pairs whose estimate moved are listed and re-run (as mcx_batch_replay does); *n_redone.
 *   mcx_avg_advance   the state after a round: state += totals; avgDist follows when the round held a chunk at all
 * A round: begin, then { totals -> exchange -> check } until no shard re-ran a pair, then advance and end. */
int mcx_batch_totals(mcx_ctx *, int64_t totals[2]);
int mcx_batch_check(mcx_ctx *, const int64_t state_before[3], int first_of_round, uint32_t *n_redone, mcx_stats *stats);
void mcx_avg_advance(int64_t state[3], int64_t pairs, int64_t dist, int64_t n_chunks);

/* ---- exchange between the shards of one run (one shard = one GPU) --------------------------------
 * Collective: every shard calls allgather the same number of times; `bytes` is the same on every
 * shard; recv receives size * bytes in rank order.  Host memory.  mapcaller-mi355x -gpus N provides
 * one between its host threads, mapcaller_amd/run.py one over torch.distributed. */
typedef struct mcx_exchange {
    void *user;
    int32_t rank, size;
    int (*allgather)(void *user, const void *send, void *recv, uint64_t bytes);
} mcx_exchange;
/* An in-process exchange for `size` host threads of one process (one per GPU): mcx_exchange_local
 * fills size entries of out[] that share one rendezvous; mcx_exchange_local_free releases it. */
int mcx_exchange_local(int32_t size, mcx_exchange *out);
void mcx_exchange_local_free(mcx_exchange *first);

/* ---- -vcf bookkeeping -------------------------------------------------------------------------
 * Replaces UpdateProfile / UpdateMultiHitCount (reference src/AlignmentProfile.cpp:41-271, called
 * under ProfileLock from src/ReadMapping.cpp:562-573) and the discordant-site lists
 * (src/ReadMapping.cpp:486-521).  d_planes: caller-owned, zero-initialised device memory of
 * mcx_planes_bytes(GenomeSize) bytes (mcx_planes_alloc makes it) — MappingRecord_t
 * (src/structure.h:152-163) unpacked into one plane per counter, each in the width it needs, 22 bytes
 * per position: with stride = GenomeSize rounded up to 64, first multi_hit as u32 [stride], then
 * A C G T readCount F1 R2 F2 R1 as u16 [stride] each (mapcaller_amd/csrc/mcx_planes.h says why 16
 * bits are exact for those nine) — so that several GPUs can sum their arrays
 * with one all-reduce.  Once attached, every mcx_map_batch* call adds its reads.  While a run is
 * being mapped the strand and multi_hit planes (and a context-owned plane for exact-seed coverage)
 * hold DIFFERENCES (+1 where a read starts to cover, -1 behind its end): mcx_profile_settle turns
 * them into counts, once, after the run's last batch and BEFORE the planes are read or summed
 * across GPUs; after it the context takes no more reads until the profile is attached again.
 * mcx_profile_finalize applies the reference's field widths (12-bit saturation at 4095, 16-bit
 * wrap, duplicate cap) in place; call it once, after the last batch (and after the reduce).
 * mcx_profile_sparse returns the insert / delete / break-point tallies ('I','D','B': one record
 * per event, to be summed by (pos, seq)) and the inversion / translocation site records ('V','T':
 * pos = gPos, dist in the first 8 bytes of seq).  max_dup = iMaxDuplicate (-dup, default 5),
 * max_clip = MaxClipSize (-maxclip, default 5).
 * On one shard the bookkeeping of a batch — duplicate check, the planes' updates, the tallies — is QUEUED behind the batch
 * when its call returns and runs under the next batch's kernels (a second set of per-read detail records and a copy of the
 * batch's reads in the context: the caller's buffers are the caller's again on return); mcx_profile_settle / _finalize /
 * _sparse*, the next batch's end and mcx_ctx_free wait for it — the planes are not to be read before one of them, as before.
 * Errors of a batch's bookkeeping (a list that ran over) come back from the next of these calls.  Without room in HBM for
 * the second set, or with MCX_NO_PROF_OVERLAP=1, it runs inside the batch's call. */
typedef struct mcx_sparse_rec {
    int64_t pos;
    uint8_t type;
    uint8_t len;   /* 'I','D': length of the whole string (up to 255); a string longer than seq continues in the */
    char seq[54];  /* records that directly follow ('C': len = bytes held).  Keep a list's records in order.      */
} mcx_sparse_rec;
int mcx_profile_attach(mcx_ctx *, uint32_t *d_planes, int max_dup, int max_clip);
int mcx_profile_settle(mcx_ctx *);                       /* idempotent; implied by mcx_profile_finalize on the attached planes */
int mcx_profile_finalize(mcx_ctx *, uint32_t *d_planes);
int mcx_profile_sparse(mcx_ctx *, const mcx_sparse_rec **recs, uint64_t *n);
/* For a run spread over several shards: the same tallies, but the discordant-pair events as they
 * were seen ('E': pos = pair number in input order, len = branch of ReadMapping.cpp:486-521,
 * seq = g1, g2, dist) instead of 'V'/'T' — the reference's second branch reports whatever the
 * previous discordant pair of the *whole stream* left behind (ReadMapping.cpp:418, :499-505), so the
 * events of all shards are replayed in input order by mcx_call_variants, which takes both forms. */
int mcx_profile_sparse_shard(mcx_ctx *, const mcx_sparse_rec **recs, uint64_t *n);
/* Duplicate cap across shards (AlignmentProfile.cpp:76-77 admits the first max_dup uniquely mapped
 * reads per start position in input order).  Between mcx_batch_end_keys (instead of mcx_batch_end)
 * and mcx_batch_accumulate the caller gathers the keys of all shards of the round:
 *   mcx_batch_end_keys    closes the batch; keys (host, pinned) = (start position << 32 | read
 *                         index in the batch) of the reads that reach the duplicate check
 *   mcx_batch_accumulate  all_keys = the keys of every shard of the round with the index replaced
 *                         by (slot * slot_stride + index), slots in input order; own reads are those
 *                         of slot own_slot.  Admission is decided over all of them against the
 *                         readCount plane, which every shard keeps for the whole run (it is the same
 *                         on all shards and is NOT summed by the reduce); then the own reads are
 *                         accumulated. */
int mcx_batch_end_keys(mcx_ctx *, mcx_stats *stats, const uint64_t **keys, uint64_t *n_keys);
int mcx_batch_accumulate(mcx_ctx *, const uint64_t *all_keys, uint64_t n_all, uint32_t slot_stride, uint32_t own_slot);

/* Device storage for the ten planes of one genome (zero-initialised); free with mcx_planes_free.
 * mcx_planes_bytes: its size (22 bytes per position of the genome rounded up to 64 positions). */
int mcx_planes_alloc(const mcx_index *, uint32_t **d_planes);
void mcx_planes_free(uint32_t *d_planes);
uint64_t mcx_planes_bytes(int64_t genome_size);

/* ---- variant calling ---------------------------------------------------------------------------
 * Replaces VariantCalling() (reference src/VariantCalling.cpp:696-740; called from src/main.cpp:379
 * after Mapping()): block read depth (CalBlockReadDepth :105-121), the per-position scan for
 * SNVs / unmapped gaps / duplicated regions / gVCF and monomorphic records (IdentifyVariants
 * :549-680), indel calls from the insert / delete tallies (GetAreaIndFrequency :63-94), break-point
 * candidates and <INV>/<TNL> calls (:173-340), filters and the VCF text (:404-500).
 * The dense work runs on the GPU over the finalized planes; the sparse tallies are host maps.
 * d_planes: the array given to mcx_profile_attach, after mcx_profile_finalize (and, on several
 * GPUs, after the all-reduce).  recs: every record mcx_profile_sparse returned (all ranks, any
 * order).  paired_pairs / pair_dist_sum / pair_len_sum: totals of mcx_stats over the run
 * (iTotalPairedNum, TotalPairedDistance, ReadLengthSum; src/ReadMapping.cpp:782-790).
 * Options hold the reference's switches; mcx_vcf_defaults fills src/main.cpp:157-187's values. */
typedef struct mcx_vcf_opts {
    int32_t ploidy, min_allele_depth, min_cnv, min_gap, fragment_size; /* -ploidy -ad -min_cnv -min_gap -size */
    int32_t filter, gvcf, monomorphic, somatic;                        /* -filter -gvcf -monomorphic -somatic */
    int32_t max_dup, max_clip;                                         /* -dup -maxclip (used by mcx_profile_attach) */
    float freq_thr;                                                    /* FrequencyThr = 0.2 (no switch) */
    const char *sample_id, *ref_name, *cmdline;                        /* -id; ##reference= and ##command_line= texts */
} mcx_vcf_opts;
typedef struct mcx_vcf_stats {
    int64_t n_snv, n_ins, n_del, n_inv, n_tnl, n_records; /* VarNumVec (VariantCalling.cpp:730) + VCF body lines */
    int32_t avg_read_len, fragment_size;                  /* avgReadLength, FragmentSize used for the break points */
    double ms_depth, ms_scan, ms_total;                   /* k_vc_depth, k_vc_scan (device), whole call (wall) */
} mcx_vcf_stats;
void mcx_vcf_defaults(mcx_vcf_opts *);
int mcx_call_variants(const mcx_index *, const uint32_t *d_planes, const mcx_sparse_rec *recs, uint64_t n_recs,
                      int64_t paired_pairs, int64_t pair_dist_sum, int64_t pair_len_sum,
                      const mcx_vcf_opts *, const char *vcf_path, mcx_vcf_stats *stats);
/* Test entry: the dense half of mcx_call_variants by itself, so that its kernels can be held against a plain restatement on
 * planes made for the purpose.  No index: d_pac is the forward genome in device memory, four bases a byte as in the .pac file
 * ((genome_size + 3) / 4 bytes); d_planes as for mcx_call_variants.  Runs, in this order on one object, the scan (block depth,
 * per-position records, their (position, type) order), the column gather of pos[0 .. n_pos) and the coverage sums (mode 0) /
 * minima over covered positions (mode 1; ~0 if there is none) of ranges[0 .. n_ranges), each [beg, end] inclusive and clipped
 * to the genome.  *sites / *n_sites: the ordered records, in storage of the library's that the next call on any thread
 * replaces; columns, range_vals: the caller's, n_pos and n_ranges entries.  A position outside the genome gives a zero column.
 * Of opts, -ploidy -ad -somatic -monomorphic -gvcf and freq_thr are read (-gvcf is dropped beside -monomorphic as in
 * mcx_call_variants). */
typedef struct mcx_vc_site {  /* a call (type 0 SNV, 11 monomorphic) or a run boundary (100 .. 105: gap start / end, dup start / end, */
    int64_t pos;              /* normal start / end) at pos; alt: codes of the one or two ALT alleles, low nibble first, 0xF = none  */
    uint8_t type, geno, qscore, alt;
    uint16_t DP, AD_ref, AD_alt, pad;
    uint32_t pad2;
} mcx_vc_site;
typedef struct mcx_vc_column { uint32_t v[10]; int32_t depth; uint32_t ref; } mcx_vc_column; /* the ten counters, block depth, reference code */
typedef struct mcx_vc_range { int64_t beg, end; int32_t mode, pad; } mcx_vc_range;
int mcx_vc_dense_dev(int device, const uint8_t *d_pac, int64_t genome_size, const uint32_t *d_planes, const mcx_vcf_opts *,
                     const int64_t *pos, uint64_t n_pos, const mcx_vc_range *ranges, uint64_t n_ranges,
                     const mcx_vc_site **sites, uint64_t *n_sites, mcx_vc_column *columns, uint64_t *range_vals);

/* ---- SAM text ----------------------------------------------------------------------------------
 * Replaces GenerateSingleSamStream / GeneratePairedSamStream (reference src/SamReport.cpp:324-488) and the -m lines
 * (:364-488) for a whole batch: the text is made in HBM from what mcx_map_batch[_dev] was given and gave back.  Read r's
 * line(s) — its record's, then those of its extras x_recs[x_index[r] .. x_index[r + 1]) — follow one another in read order.
 * paired: the batch was mapped as pairs; SEQ/QUAL of every second read are then printed the way the reference prints mate 2,
 * which it reverse-complements before mapping (ReadMapping.cpp:451): as they are for a reverse-strand hit, turned otherwise,
 * bytes other than ACGTacgt as N whenever a complement is taken.  qual: read r's rlen bytes at off[r], the bytes of the quality
 * line the reference takes (the first min(line, rlen), GetData.cpp:51-52) with NUL behind them up to rlen: QUAL is printed up to
 * the first NUL, or — reversed — from the last byte backwards up to the first NUL (empty when the line was short). */
typedef struct mcx_sam_in {
    const uint8_t *bases; const uint32_t *off;        /* as given to mcx_map_batch[_dev]: n_reads + 1 offsets */
    const uint8_t *qual;                               /* NULL: '*'.  Else read r's rlen bytes at off[r], NUL-padded (see above) */
    const uint8_t *names; const uint32_t *name_off;    /* QNAMEs back to back; n_reads + 1 offsets */
    const mcx_aln *aln; const uint32_t *cigar;         /* the batch's records and CIGAR pool */
    const uint32_t *x_index; const mcx_aln *x_recs; const uint32_t *x_cigar; /* -m extras as mcx_multi_lines hands them out; NULL: none */
    uint32_t n_reads; int32_t paired;
    const uint8_t *md; const uint32_t *md_off;         /* the lines' MD strings as mcx_md[_dev] makes them (below); NULL: no MD:Z tag, the bytes of before */
} mcx_sam_in;
/* d_in: the struct in host memory, every pointer in it a device pointer.  d_text[0 .. cap) receives the text, d_line_off (device, may be
 * NULL) n_reads + 1 byte offsets of the reads' first lines, the last one the total; *n_bytes is always the exact size of the batch's
 * text.  cap smaller than that: nothing is written to d_text and the call returns MCX_ERR_CAPACITY — allocate and call again (a call
 * with cap = 0 asks for the size).  Runs on the context's stream and returns when the text is there. */
int mcx_sam_format_dev(mcx_ctx *, const mcx_sam_in *d_in, uint8_t *d_text, uint64_t cap, uint64_t *d_line_off, uint64_t *n_bytes);
/* same with host buffers (staged inside) */
int mcx_sam_format(mcx_ctx *, const mcx_sam_in *in, uint8_t *text, uint64_t cap, uint64_t *line_off, uint64_t *n_bytes);
/* OutputSamHeaders (reference src/ReadMapping.cpp:101-123): the @PG / @SQ lines the file front end writes ahead of the first
 * batch; *n_bytes their size, MCX_ERR_CAPACITY (nothing written) when cap is smaller. */
int mcx_sam_header(const mcx_index *, char *out, uint64_t cap, uint64_t *n_bytes);

/* ---- Read-group and mate tags ------------------------------------------------------------------------
 * What `samtools addreplacerg` and `samtools fixmate -m` add to a finished file — which the reference does not write —, made inside the formatters while a pair's
 * two records are neighbours in HBM.  Two independent switches (mapcaller-mi355x -rg, -mc); without them every byte is what it was.
 * The read-group line (mcx_rg_parse; bwa mem -R's form): the argument as given, every two-character sequence "\t" replaced by a TAB.  It must begin with "@RG" TAB;
 *   every further TAB-separated field is two characters of [A-Za-z][A-Za-z0-9], ':' and at least one byte; exactly one field is ID; no byte below 0x20 other than
 *   TAB and none 0x7f; the ID at most 255 bytes, the line at most 4096.  Anything else is MCX_ERR_ARG, the reason in mcx_last_error.
 * Header: the line, with a newline, is the last line of the header text, behind what mcx_sam_header writes (mcx_sam_header_rg, mcx_bam_header_rg: l_text grows by it).
 * RG:Z:<ID> goes on every line, mapped or not, the -m extras included.
 * MC:Z and MQ:i: read r of a batch mapped as pairs has the mate m = r ^ 1.  Both tags are written iff paired, m < n_reads, the mate's own record is mapped
 *   (chr >= 0 and n_cigar > 0) and the line's own FLAG has bit 0x8 clear — where the reference calls the mate unmapped an MC would contradict the flag (some lines have
 *   a mapped mate and 0x8 set all the same: they get neither).  An unmapped read whose mate is mapped gets both.  MC is the mate's CIGAR exactly as the mate's own line
 *   prints it in column 6 (the same code prints both), MQ the mate's mapq.  A batch of single reads gets neither.  FLAG, RNEXT, PNEXT and TLEN stay the reference's.
 *   An -m extra is paired with another candidate of the mate than the one whose CIGAR is held: mate_tags with a non-null x_index is MCX_ERR_UNSUPPORTED, nothing written.
 * Order: mapped lines NM AS XS [MD] [MC MQ] [RG]; unmapped lines AS XS [MC MQ] [RG].
 * BAM: 'M' 'C' 'Z' the string NUL; MQ as the smallest integer type that holds it ('C' for 0 .. 255); 'R' 'G' 'Z' the ID NUL; block_size grows by those bytes.
 * mcx_sam_tags travels beside mcx_sam_in (whose layout stays): rg the ID's bytes — a device pointer for the _dev calls, staged inside for the host forms —, NULL
 * or rg_len 0: no RG tag; mate_tags != 0: MC and MQ.  A NULL mcx_sam_tags is both off: mcx_sam_format[_dev] and mcx_bam_format[_dev] are these calls with NULL. */
typedef struct mcx_sam_tags { const uint8_t *rg; uint32_t rg_len; int32_t mate_tags; } mcx_sam_tags;
int mcx_sam_format_tags_dev(mcx_ctx *, const mcx_sam_in *d_in, const mcx_sam_tags *tags, uint8_t *d_text, uint64_t cap, uint64_t *d_line_off, uint64_t *n_bytes);
int mcx_sam_format_tags(mcx_ctx *, const mcx_sam_in *in, const mcx_sam_tags *tags, uint8_t *text, uint64_t cap, uint64_t *line_off, uint64_t *n_bytes);
int mcx_bam_format_tags_dev(mcx_ctx *, const mcx_sam_in *d_in, const mcx_sam_tags *tags, uint8_t *d_out, uint64_t cap, uint64_t *d_rec_off, uint64_t *n_bytes, uint64_t *n_dropped);
int mcx_bam_format_tags(mcx_ctx *, const mcx_sam_in *in, const mcx_sam_tags *tags, uint8_t *out, uint64_t cap, uint64_t *rec_off, uint64_t *n_bytes, uint64_t *n_dropped);
/* The -rg argument checked and taken apart: line[0 .. cap) receives the line with real TABs, no newline and no NUL, *line_len its size, *id_at / *id_len where
 * its ID lies in it (any of the four may be NULL).  MCX_ERR_ARG with the reason in words; MCX_ERR_CAPACITY (nothing written) when cap is smaller than the line. */
int mcx_rg_parse(const char *arg, char *line, uint64_t cap, uint64_t *line_len, uint32_t *id_at, uint32_t *id_len);
/* mcx_sam_header's bytes, and mcx_bam_header's (sorted != 0: mcx_bam_header_sorted's), with rg_line (NUL-terminated, real TABs, no newline: checked as by
 * mcx_rg_parse) as the last line of the text.  A NULL rg_line gives those calls' bytes. */
int mcx_sam_header_rg(const mcx_index *, const char *rg_line, char *out, uint64_t cap, uint64_t *n_bytes);
int mcx_bam_header_rg(const mcx_index *, const char *rg_line, int sorted, uint8_t *out, uint64_t cap, uint64_t *n_bytes);

/* ---- MD:Z strings ------------------------------------------------------------------------------------
 * The string that says, against the CIGAR, which reference bases a line mismatches or deletes — what `samtools calmd` writes, which the reference does not — made in
 * HBM from the mcx_sam_in the formatters take and the index's genome.  MD is defined for a mapped line (chr >= 0, n_cigar > 0) by walking its CIGAR over the
 * line's printed SEQ (the reversal, complement and twice-complement rules of mcx_sam_format_dev applied) against the forward reference from chr_fwd[chr] + pos - 1:
 *   M columns (and = and X)  a match extends the current run u; a mismatch writes u, then the reference letter, and sets u = 0 — two adjacent mismatches
 *                            give "..A0C..", a mismatch in the first column a leading "0"
 *   D                        writes u, '^', the deleted reference letters, and sets u = 0 ("^AC0T": a mismatch directly behind a deletion)
 *   I, S                     take read bases only and do not end a run; N skips reference bases without text; H and P do nothing
 *   the end                  the final u is always written: 150M without a mismatch gives "150"
 *   a column matches         iff the 4-bit BAM code of the SEQ byte (case ignored; 15 for anything outside "=ACMGRSVTWYHKDBN") equals the reference letter's and
 *                            is not 15: a read N never matches, not even a reference N
 *   the reference letter     "ACGT"[the two bits of the .pac], or, inside an ambiguity hole of the index's .amb file (lines of "offset length letter"), the
 *                            hole's own letter in upper case — not the random base the packer put into the .pac; 'N' outside the genome
 * Unmapped lines and lines without a CIGAR get no tag.  d_md[0 .. cap) receives the strings back to back, no NULs, no "MD:Z:"; d_md_off (device, may be NULL) has
 * n_reads + n_extras + 1 entries: read r's own record at [r], the -m extra i (the index into x_recs; n_extras = x_index[n_reads]) at [n_reads + i], the last one
 * the total; a zero-length entry means no tag.  *n_bytes is always exact; cap smaller than that: nothing is written to d_md, MCX_ERR_CAPACITY (cap = 0 asks for the
 * size).  More than 4 GiB of strings: MCX_ERR_UNSUPPORTED.  names, name_off and qual of d_in are not read.  On the context's stream, waited for.
 * A pool handed to the formatters through mcx_sam_in.md / md_off appends "\tMD:Z:" + the string behind XS:i of a SAM line, and 'M' 'D' 'Z', the string and a NUL
 * behind the XS tag of a BAM record (block_size grows by that); the strings are copied from the pool, never recomputed. */
int mcx_md_dev(mcx_ctx *, const mcx_sam_in *d_in, uint8_t *d_md, uint64_t cap, uint32_t *d_md_off, uint64_t *n_bytes);
/* same with host buffers (staged inside) */
int mcx_md(mcx_ctx *, const mcx_sam_in *in, uint8_t *md, uint64_t cap, uint32_t *md_off, uint64_t *n_bytes);
/* the last call's device times in ms: length kernel, scan, write kernel */
int mcx_md_last_ms(mcx_ctx *, float ms[3]);

/* ---- BAM records ---------------------------------------------------------------------------------
 * The same batch as uncompressed BAM records (the reference's -bam: every SAM line through htslib's sam_parse1 / sam_write1, src/ReadMapping.cpp:548-606),
 * made in HBM from the mcx_sam_in that mcx_sam_format_dev takes — the record of the line that call would print, field for field: refID / pos - 1 / mapq / bin
 * (UCSC binning, 14-bit minimum shift, 5 levels) / flag (| 4 unmapped), the pool's CIGAR words as they are, SEQ two bases a byte, QUAL - 33 (0xff: none), NM / AS / XS
 * as the smallest integer type that holds the value.  A line htslib's parser rejects makes no record and is counted: a QNAME of 252 bytes or more, a QUAL that is
 * not '*' and not as long as SEQ.  Read r's record(s) — its extras' behind its own — start at d_rec_off[r] (device, may be NULL; n_reads + 1 entries, the last one
 * the total); records are not aligned and say nothing of BGZF: mcx_bgzf_deflate_dev frames them.  *n_bytes is always the exact size, *n_dropped (may be NULL) the
 * lines left out; cap smaller than the size: nothing is written, MCX_ERR_CAPACITY (cap = 0 asks for the size).  On the context's stream, waited for. */
int mcx_bam_format_dev(mcx_ctx *, const mcx_sam_in *d_in, uint8_t *d_out, uint64_t cap, uint64_t *d_rec_off, uint64_t *n_bytes, uint64_t *n_dropped);
/* same with host buffers (staged inside) */
int mcx_bam_format(mcx_ctx *, const mcx_sam_in *in, uint8_t *out, uint64_t cap, uint64_t *rec_off, uint64_t *n_bytes, uint64_t *n_dropped);
/* The uncompressed BAM header: "BAM\1", l_text, mcx_sam_header's text, n_ref, and per contig l_name, the name with its NUL, l_ref.  *n_bytes its size,
 * MCX_ERR_CAPACITY (nothing written) when cap is smaller; MCX_ERR_UNSUPPORTED for a contig longer than 2^31 - 1, which BAM cannot say. */
int mcx_bam_header(const mcx_index *, uint8_t *out, uint64_t cap, uint64_t *n_bytes);
/* Records in HBM put into coordinate order (mapcaller-mi355x -sort).  A record's key is read from its own bytes — (uint32_t)refID << 32 | (uint32_t)(pos + 1) << 1 |
 * reverse (flag bit 0x10): samtools sort's comparison, refID -1 last, forward before reverse on one position —, the sort is stable: ties keep their order in d_recs.
 * d_recs[0 .. n_bytes) are whole records in n_groups groups, group g at d_grp_off[g] .. d_grp_off[g + 1] (mcx_bam_format_dev's d_rec_off: a read's records — none,
 * one, several); d_out receives the same n_bytes in key order, contiguous, d_keys / d_lens (may be NULL; room for n_bytes / 36 entries at most) each output
 * record's key and length (4 + block_size), *n_records their number.  The block_size chain is walked inside each group: offsets that do not ascend from 0 to
 * n_bytes, a block_size below 32 or a record that leaves its group return MCX_ERR_ARG, with nothing written to d_out and nothing read outside d_recs[0 .. n_bytes).
 * cap < n_bytes: MCX_ERR_CAPACITY; n_groups == 0: 0, nothing written.  Scratch (about 50 bytes a record) stays with the context.  On the context's stream, waited for. */
int mcx_bam_sort_dev(mcx_ctx *, const uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_grp_off, uint32_t n_groups, uint8_t *d_out, uint64_t cap,
                     uint64_t *d_keys, uint32_t *d_lens, uint64_t *n_records);
/* the last call's device times in ms: index (chain walk, scan, keys), sort, place (lengths gathered and summed), gather */
int mcx_bam_sort_last_ms(mcx_ctx *, float ms[4]);
/* (tests, measurements) the last tier-0 pass of the context: out[0..5] the pairs the order listed per weight class, heaviest first (all zero: the pass
   made no order); out[6] the pairs of the heavy classes' clustering launch, out[7] of the light classes'; out[8] 1 when the heavy pairs were listed and
   clustered on a side stream beside the straight-line path, 0 when one launch in line took all classes; out[9] the pairs that launch listed for the large tier */
int mcx_pass_last_shape(mcx_ctx *, uint32_t out[10]);
/* mcx_bam_header's bytes for a coordinate-sorted file: the text begins with "@HD\tVN:1.6\tSO:coordinate\n" */
int mcx_bam_header_sorted(const mcx_index *, uint8_t *out, uint64_t cap, uint64_t *n_bytes);
/* What a .bai is made of (mapcaller-mi355x -index), from one run of coordinate-sorted records in HBM that has just been deflated.  d_recs[0 .. n_bytes) are
 * n_records whole records, record i at d_rec_off[i] .. d_rec_off[i + 1] (device; n_records + 1 entries from 0 to n_bytes); they were cut into BGZF blocks of
 * block_text_bytes of text, block k of the n_blocks = ceil(n_bytes / block_text_bytes) written at byte d_block_coff[k] of the file (device; n_blocks + 1 entries,
 * the last one the byte behind them).  A record's virtual offset u is d_block_coff[offset / block] << 16 | offset % block; its interval is [pos, bam_endpos): pos +
 * the reference length of its CIGAR (M, D, N, = and X), pos + 1 when flag bit 4 is set or that length is 0; its bin is reg2bin of the interval (htslib's
 * hts_idx_push: min_shift 14, 5 levels; 4680 for a record without a contig).
 * d_runs[0 .. runs_cap) receives one entry per maximal stretch of records with one (ref_id, bin) — the first record's u, the records without and with flag bit 4 —,
 * all records with refID < 0 as one stretch (ref_id -1, bin 4680); *n_runs their number.  d_lin is the table of the 16 kb windows of all n_ref contigs, contig t's at
 * d_lin[d_lin_base[t] .. d_lin_base[t + 1]) (device; d_lin_base has n_ref + 1 entries), which the caller sets to all-ones once: every window that a record without
 * flag bit 4 on a contig touches (pos >> 14 .. (end - 1) >> 14) holds the smallest u seen so far, over consecutive calls on one table.
 * MCX_ERR_ARG, with nothing written to d_runs or d_lin and nothing read outside the inputs: offsets that do not ascend from 0 to n_bytes, a record that is not
 * 4 + its block_size long or shorter than its name and CIGAR, n_blocks that is not the number of blocks, a refID of n_ref or more, a position or end beyond 2^29 or
 * beyond the contig's windows, records whose (refID, pos) descend, a record on a contig behind one without.  runs_cap too small: MCX_ERR_CAPACITY, *n_runs says what
 * is needed, nothing written.  n_records == 0: 0, no stretches.  Scratch (52 bytes a record) stays with the context.  On the context's stream, waited for. */
typedef struct mcx_bai_run { int32_t ref_id; uint32_t bin; uint64_t u; uint32_t n_mapped, n_unmapped; } mcx_bai_run;
int mcx_bam_index_dev(mcx_ctx *, const uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_rec_off, uint32_t n_records, uint32_t block_text_bytes,
                      const uint64_t *d_block_coff, uint32_t n_blocks, uint64_t *d_lin, const uint64_t *d_lin_base, uint32_t n_ref,
                      mcx_bai_run *d_runs, uint64_t runs_cap, uint64_t *n_runs);
/* the last call's device times in ms: records (fields, CIGAR walk, offsets, order), stretches (flags, scans, the list), windows (running maximum, the table) */
int mcx_bam_index_last_ms(mcx_ctx *, float ms[3]);
/* Duplicate marking (mapcaller-mi355x -markdup), in three operations.  The rule (mcx_markdup.h holds its arithmetic for the device and the host):
 *   a read is a group of mcx_bam_format_dev's rec_off and its record the group's first; it is placed when it has a record and flag bit 4 is clear.
 *   end(record) = (refID, u5, reverse), u5 the unclipped 5' position: forward pos - leading S and H, reverse pos + reflen - 1 + trailing S and H (reflen over M, D, N,
 *   = and X); score(record) = the sum of the QUAL bytes that are 15 or more (0xff counts as 0).  A packed end is refID << 40 | (u5 + 2^38) << 1 | reverse, for
 *   0 <= refID < 2^24 - 1, |u5| < 2^38 and fewer than 2^23 bases; all-ones is no end.
 *   Units, numbered in input order.  Paired: reads 2i and 2i + 1 are unit i — both placed: a pair unit, its key the two ends in ascending order, its score the sum of
 *   both; one placed: a fragment unit, key its end, score its own; none placed: no unit (kind 0).  Single-end: read i is unit i, a fragment unit when placed.
 *   Among pair units with equal keys the one with the highest score stays, a tie going to the lowest number; the others are duplicates.  A fragment unit is a
 *   duplicate when a pair unit has one of its two ends equal to the fragment's end; otherwise, among fragments with equal ends, all but the best (as above) are.
 * mcx_bam_dup_units_dev: d_recs / n_bytes / d_grp_off / n_groups as for mcx_bam_sort_dev (paired: n_groups must be even); d_units receives *n_units = n_groups / 2
 * (paired) or n_groups entries.  kind: bits 0-1 are 0 none, 1 fragment, 2 pair; bit 2 is set when a paired input's fragment is the second read.  end1 is all-ones
 * for a fragment, both ends for none.  MCX_ERR_ARG, with nothing written and nothing read outside d_recs[0 .. n_bytes): offsets that do not ascend from 0 to n_bytes,
 * a block_size below 32, a record that leaves its group or is shorter than its name, CIGAR, SEQ and QUAL — and, said apart, a placed read outside the packing's range.
 * mcx_dup_resolve_dev: d_dup[u] = 1 when unit u is a duplicate, else 0, for all n_units (device, one byte a unit), by stable radix sorts: no result depends on
 * anything but the units and their order.  Scratch (56 bytes a unit and the sorts' own) stays with the context; when HBM does not hold it: MCX_ERR_CAPACITY, the
 * bytes needed in words, nothing written.  kind values other than the above: MCX_ERR_ARG.
 * mcx_bam_dup_mark_dev: sets flag bit 0x400 — bit 2 of byte 19, a byte store — in every record i (d_rec_off: n_records + 1 entries, device) with d_rec_dup[i] != 0
 * (device, one byte a record) and touches nothing else.  Offsets that descend, leave n_bytes or leave a record less than 20 bytes: MCX_ERR_ARG, nothing written.
 * All three run on the context's stream and are waited for. */
typedef struct mcx_dup_unit { uint64_t end0, end1; uint32_t score, kind; } mcx_dup_unit;
int mcx_bam_dup_units_dev(mcx_ctx *, const uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_grp_off, uint32_t n_groups, int paired, mcx_dup_unit *d_units, uint64_t *n_units);
int mcx_dup_resolve_dev(mcx_ctx *, const mcx_dup_unit *d_units, uint64_t n_units, uint8_t *d_dup);
int mcx_bam_dup_mark_dev(mcx_ctx *, uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_rec_off, uint32_t n_records, const uint8_t *d_rec_dup);
/* the device times in ms of the context's last call of each: units, resolve, mark */
int mcx_markdup_last_ms(mcx_ctx *, float ms[3]);

/* ---- BGZF input inflated on the device -------------------------------------------------------------
 * bgzip's container is a row of independent gzip members of at most 64 KB of text, each of which says how long it is ('BC' extra
 * field) and carries the CRC-32 and the length of its text.  An inflater takes the raw deflate streams of many members at once — a
 * wavefront per member: stored, fixed and dynamic blocks (RFC 1951), the CRC-32 taken on the device as well — and is an object of
 * its own, with a stream of its own (non-blocking): reader threads use one beside a context that maps.  One host thread per object.
 * A member: src[src_off .. src_off + src_len) -> dst[dst_off .. dst_off + isize), isize <= 65536, any alignment; behind the last
 * member's bytes src must be readable for 8 bytes more (src_bytes includes them).  status[i] is an mcx_inflate_status; a member
 * that fails writes nothing outside its own bytes of dst.  Bytes behind the final block inside src_len are ignored. */
enum mcx_inflate_status {
    MCX_INFLATE_OK = 0,
    MCX_INFLATE_DAMAGED = 1, /* no deflate stream: block type 3, LEN != ~NLEN, an invalid code or set of codes, a distance before the start */
    MCX_INFLATE_INPUT = 2,   /* the input ran out before the final block ended */
    MCX_INFLATE_LENGTH = 3,  /* the stream ends short of isize or runs past it */
    MCX_INFLATE_CRC = 4      /* the text is not the one the CRC-32 was taken of */
};
typedef struct mcx_inflater mcx_inflater;
typedef struct mcx_deflate_member {   /* 32 bytes */
    uint64_t src_off;  uint64_t dst_off;   /* any alignment */
    uint32_t src_len, isize, crc32, reserved;
} mcx_deflate_member;
/* Capacities of one launch through host buffers (mcx_inflate): compressed bytes, bytes of text, members; 0: defaults (8 MB of text). */
int  mcx_inflater_create(int device, uint64_t max_src_bytes, uint64_t max_dst_bytes, uint32_t max_members, mcx_inflater **out);
void mcx_inflater_free(mcx_inflater *);
/* device pointers; runs on the inflater's own stream and returns when the text is there; 0, or MCX_ERR_IO when any member failed (d_status says which).
 * MCX_ERR_ARG before any launch: a member outside src_bytes (its 8 bytes of slack included) or dst_cap, isize > 65536, n > max_members. */
int  mcx_inflate_dev(mcx_inflater *, const uint8_t *d_src, uint64_t src_bytes, const mcx_deflate_member *d_members, uint32_t n, uint8_t *d_dst, uint64_t dst_cap, uint32_t *d_status);
/* host buffers, staged through the object's page-locked buffers, in as many launches as its capacities require (no slack needed behind src) */
int  mcx_inflate(mcx_inflater *, const uint8_t *src, uint64_t src_bytes, const mcx_deflate_member *members, uint32_t n, uint8_t *dst, uint64_t dst_cap, uint32_t *status);
/* the BGZF reader by itself, the twin of mcx_gz_inflate: whole length of the text, -1 unreadable / first bytes are no BGZF member, -2 a damaged member (*n_out: bytes delivered before it) */
int64_t mcx_bgzf_inflate(const char *path, int device, uint8_t *out, uint64_t cap, uint64_t *n_out);

/* ---- ordinary gzip streams inflated on the device ---------------------------------------------------
 * A gzip member that is not BGZF is ONE deflate stream: a block starts at any bit, and a match reaches 32 KB back into text that is not there yet.  A
 * gunzipper does on the device what mcx_gz_inflate does with host threads (mcx_pgz.h's method; mcx_gz_dev.h, mcx_gz_dev.hip): the compressed bytes of a ROUND
 * are cut into stretches of stretch_bytes; a wavefront per stretch looks for a block start in its own bytes (dynamic block, complete codes, first symbols
 * decode to text); a wavefront per stretch with a start inflates from there into 16-bit symbols (below 256 a byte, 256 + p "byte p of the 32 KB before my
 * start") until it ends on a later stretch's start (or has passed 4 later stretches in which no start was found); the host walks the chain stretch 0 -> whichever stretch begins where the last one stopped (a false start
 * is never met and costs time only); one workgroup resolves the chain's 32 KB windows in sequence; all symbols become bytes in parallel, a CRC-32 per piece.
 * The call is in two halves so that the caller knows text_bytes before it makes room: mcx_gunzip_round_dev runs search, inflate, chain and windows and says where
 * the round ended; mcx_gunzip_text_dev writes the round's text to d_dst[0 .. text_bytes) and takes its CRC-32.  A round with text_bytes > 0 must be fetched before
 * the next round is run (the symbols lie in the object's arena).  The next round starts at end_bit: pass src + (end_bit >> 3) and start_bit = end_bit & 7.
 * The object keeps the last 32 KB of text as the next round's window; mcx_gunzipper_reset at the start of a member.  It knows nothing of gzip headers and
 * trailers: final = 1 says the member's final block ended at end_bit, and the caller compares CRC-32 (zlib's crc32_combine over the rounds) and ISIZE.
 * status: MCX_GZ_OK — text_bytes may still be 0: a stretch ran out of room in the arena (overflowed), the chain ends in front of it and the next round takes half
 * as many stretches (down to one, which has the whole arena; back to the full number after a round whose chain no overflow ended); call again.  MCX_GZ_MORE: only
 * with src_is_end = 0 — not even the first stretch reached a block end inside src_bytes: pass more bytes.  MCX_GZ_DAMAGED / MCX_GZ_INPUT / MCX_GZ_CAPACITY (one
 * stretch with the whole arena is out of room: mcx_last_error says so in words): the stream ends here, the calls return 0 and the status says why.
 * One host thread per object; a non-blocking stream of its own.  HBM: 2 bytes a symbol of the arena + 64 KB a stretch (the window prefixes) + 32 KB a stretch
 * (the resolved windows). */
enum mcx_gz_status { MCX_GZ_OK = 0, MCX_GZ_DAMAGED = 1, MCX_GZ_INPUT = 2 /* the stream ends inside a block */, MCX_GZ_CAPACITY = 3, MCX_GZ_MORE = 4 /* not the file's end: pass more bytes */ };
typedef struct mcx_gz_round {
    uint64_t end_bit;     /* where the next round starts, relative to src[0] */
    uint64_t text_bytes;  /* what mcx_gunzip_text_dev will write */
    uint32_t crc32;       /* of this round's text alone (valid after mcx_gunzip_text_dev) */
    uint32_t final;       /* 1: the member's final block ended the round at end_bit */
    uint32_t status;      /* mcx_gz_status */
    uint32_t stretches, starts, chain, overflowed; /* cut, found by the search, in the chain (stretch 0 included), out of room */
    float ms[4];          /* search, inflate, windows, text + CRC: events on the object's stream */
} mcx_gz_round;
typedef struct mcx_gunzipper mcx_gunzipper;
int  mcx_gunzipper_create(int device, uint64_t stretch_bytes /* 0: 64 KB; at least 4096 */, uint32_t max_stretches /* 0: 2048 */, uint64_t arena_symbols /* 0: 8 per compressed byte of a full round */, mcx_gunzipper **out);
void mcx_gunzipper_free(mcx_gunzipper *);
void mcx_gunzipper_reset(mcx_gunzipper *);  /* a new member begins: no window */
/* d_src[0 .. src_bytes) in HBM, readable 8 bytes further; start_bit 0..7; src_is_end: the bytes end with the file */
int  mcx_gunzip_round_dev(mcx_gunzipper *, const uint8_t *d_src, uint64_t src_bytes, uint32_t start_bit, int src_is_end, mcx_gz_round *info);
int  mcx_gunzip_text_dev(mcx_gunzipper *, uint8_t *d_dst, uint64_t dst_cap, mcx_gz_round *info);
/* the reader by itself, the twin of mcx_gz_inflate and mcx_bgzf_inflate: same return values (-1 no gzip file, -2 damaged, *n_out bytes delivered before).
 * Members are walked by their RFC 1952 headers, every trailer's CRC-32 and ISIZE are compared, concatenated members are followed and garbage behind a
 * complete member ends the input quietly; a round's bytes go to HBM through page-locked memory, the next round's while this one is on the device.
 * round_stretches 0: 2048. */
int64_t mcx_gz_inflate_dev(const char *path, int device, uint64_t stretch_bytes, uint32_t round_stretches, uint8_t *out, uint64_t cap, uint64_t *n_out);
/* of the calling thread's last mcx_gz_inflate_dev: rounds begun, and rounds whose compressed bytes were already in HBM when they began (staged while the round
 * before ran: every round but a member's first, unless a block is longer than the slack of four stretches) */
void mcx_gz_inflate_dev_last(uint64_t stats[2]);

/* ---- text compressed to BGZF on the device --------------------------------------------------------------
 * The way back: text that lies in HBM — the SAM text of mcx_sam_format_dev — becomes a row of BGZF blocks, each an independent gzip member of at most
 * 65 280 bytes of text (bgzip's cut; mcx_deflater_set_block: fewer), which samtools, bgzip -d, zcat and Python's gzip read.  A wavefront per block: LZ77
 * matches inside the block's own bytes (4 .. 258 bytes long, 1 .. 32 768 back), dynamic Huffman codes (RFC 1951 block type 2) — or the fixed codes, or the
 * bytes stored, whichever is smallest, so a block's deflate stream never exceeds its text + 5 bytes —, the CRC-32 taken on the device.  The same text and
 * block size give the same bytes on every run.  A deflater is an object of its own like an inflater: one device, a non-blocking stream of its own, scratch in
 * HBM made on first use (a slot per block of a launch; a launch takes at most 128 MB of text) and, for the host form, page-locked staging.  One host thread
 * per object.
 * A block: the 18-byte header 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 02 00, BSIZE = the block's size - 1; the deflate stream; CRC-32; ISIZE.
 * mcx_bgzf_deflate_dev writes complete, contiguous blocks in text order (every call starts a fresh block; no EOF block) to d_out and their bytes to *n_out;
 * text_bytes == 0 writes nothing.  out_cap < mcx_bgzf_bound(text_bytes, the block size): MCX_ERR_CAPACITY, nothing written.  Runs on the object's stream and
 * returns when the bytes are there. */
typedef struct mcx_deflater mcx_deflater;
int      mcx_deflater_create(int device, uint64_t max_text_bytes /* per launch through host buffers; 0: default (8 MB) */, mcx_deflater **out);
void     mcx_deflater_free(mcx_deflater *);
int      mcx_deflater_set_block(mcx_deflater *, uint32_t text_bytes);    /* 1..65280 per BGZF block, sticky; default 65280; else MCX_ERR_ARG */
uint64_t mcx_bgzf_bound(uint64_t text_bytes, uint32_t block_text_bytes); /* bytes the blocks of that much text can take at most (every block stored: text + 31 per block) */
int      mcx_bgzf_deflate_dev(mcx_deflater *, const uint8_t *d_text, uint64_t text_bytes, uint8_t *d_out, uint64_t out_cap, uint64_t *n_out);
/* where the blocks of the last mcx_bgzf_deflate_dev lie: *d_block_at a device array of the object's own, valid until its next call, with *n_blocks + 1 entries —
 * block k begins at byte (*d_block_at)[k] of d_out, the last entry is *n_out — over all launches of that call (mcx_bam_index_dev makes virtual offsets of them);
 * *n_blocks 0 and a null array after a call without text or before the first */
int      mcx_bgzf_deflate_blocks(mcx_deflater *, const uint64_t **d_block_at, uint64_t *n_blocks);
/* host buffers, staged through the object's page-locked buffers in as many launches as max_text_bytes requires: the same bytes */
int      mcx_bgzf_deflate(mcx_deflater *, const uint8_t *text, uint64_t text_bytes, uint8_t *out, uint64_t out_cap, uint64_t *n_out);
int      mcx_bgzf_eof(uint8_t out[28]);                                  /* the empty block that ends a BGZF file */

/* ---- FASTQ text parsed on the device ---------------------------------------------------------------
 * Replaces the host reader's parse and pack of plain FASTQ (MappedFastq::parse, header_of and mcx_pack_row; the reference's GetNextEntry,
 * GetData.cpp:3-20, :32-55) for text that lies in HBM already — what mcx_inflate_dev delivers — and produces exactly the arrays
 * mcx_map_batch_dev, mcx_sam_in and mcx_stream_submit_packed / mcx_stream_submit_dev take.  FASTQ (the default) or FASTA (mcx_fastq_parser_set_format, below),
 * under one of two rules (mcx_fastq_parser_set_rule).  THE PLAIN RULE, the default: a line is what getline gives (up to and including '\n', the text's last line possibly without one).
 * Record k of a text is its lines 4k .. 4k+3 counted from the text's first byte, whatever they hold: the name by the reference's header rule, rlen =
 * the sequence line's length less one (its last byte goes, newline or not), the '+' line skipped, q_take = min(quality line with its newline, rlen),
 * 0 when that line is absent.  A text's records end at the first of: max_records taken (MORE); with final == 0 a record whose four lines do not all
 * end in '\n' inside the text (MORE); no header line (END); no sequence line or rlen == 0, which is what ends the reference's input (EMPTY);
 * rlen > max_read_len (TOO_LONG).  The records before a stop count.
 * THE GZ RULE (MCX_FASTQ_RULE_GZ) is the .gz readers' (the reference's gzGetNextEntry, GetData.cpp:101-128: gzgets with a 1024-byte buffer, C strings): the text
 * is cut into PIECES from its first byte — the piece at s is the bytes up to and including the first '\n' within text[s, s + 1023); without one, those 1023 bytes
 * when there are as many, else the rest of the text (unfinished, the text's last) — and record k is pieces 4k .. 4k+3, each taken up to its first NUL (its C
 * length).  Header: C length 0 or a first byte other than '@' and '>' ends the input (EMPTY); the name by the header rule over the C length.  rlen = C length of
 * the sequence piece less one (0 for 0); q_take = min(C length of the fourth piece, rlen).  The stops are the plain rule's with pieces for lines; with final == 0
 * a record is taken only when its four pieces are complete (each ends in '\n' or is 1023 bytes long).  consumed[t] is always a piece start of its line, so a
 * caller that carries text[consumed ..) forward gets the same pieces again.  Texts without any NUL do not pay for the C lengths.
 * FASTA (MCX_READS_FASTA; the reference's GetNextEntry, GetData.cpp:56-77, and gzGetNextEntry, :101-128).  PLAIN RULE: line 0 of the text is a header whatever it
 * holds, and so is every later line whose first byte is '>'; record k runs from its header to the next header or the text's end.  The name is the header rule's;
 * the sequence is every non-header line less its last byte (newline or not) back to back — an empty line gives nothing, '\r' and a '>' inside a line are bases,
 * a NUL does not end a line —, rlen their sum, q_take = 0.  Stops: no header line (END), rlen == 0 (EMPTY: a header behind a header, a header last), rlen >
 * max_read_len (TOO_LONG), max_records taken (MORE).  With final == 0 a record is taken only when a later header line has begun inside the text (its sequence is
 * known to be complete); an unfinished last record that already holds more than max_read_len bases stops with TOO_LONG, so that a streaming caller makes progress
 * or fails; consumed[t] is the start of the first header line that belongs to no taken record: a text carried from there gives the same records.  A record's
 * seq is the offset of the first byte behind its header line and rlen the total: the bases are NOT contiguous in the text — take the bases / off group.  The
 * line table covers the whole text: scratch of about 24 bytes per line, grown on demand (MCX_ERR_DEVICE when HBM has no room), and one more wait inside the call.
 * GZ RULE: record k is pieces 2k and 2k + 1 — header and one sequence piece —, otherwise as above; with final == 0 a record is taken when both pieces are complete.
 * Under either rule there is no quality: the qual group, when given, is filled with NULs.
 * A parser is an object of its own like an inflater: one device, a non-blocking stream of its own, scratch in HBM (about 64 bytes per record of
 * max_records and 4 bytes per 4 KB of text) and page-locked staging for the host form, both growing on demand.  One host thread per object.
 *   n_records[t], stop[t]   records taken of text t and why no more (an mcx_fastq_stop)
 *   consumed[t]             offset of the first byte that belongs to no taken record: a streaming caller carries text[consumed ..) over
 *   n_reads                 n_records[0] for one text, 2 * min(n_records[0], n_records[1]) for two (read 2i is record i of text[0], read 2i+1
 *                           record i of text[1]); both counts are reported and a mismatch is the caller's to judge
 *   longest, n_bases, n_name_bytes, n_odd   over the n_reads reads: the longest rlen, the sums of rlen and name_len, the bytes that are not upper-case ACGT
 * Outputs, each group optional (NULL: not produced):
 *   recs[t]                 max_records records of text t's capacity; n_records[t] written; offsets into text t
 *   bases, off, qual        the layout of mcx_map_batch_dev / mcx_sam_in: the reads' bases back to back, n_reads + 1 offsets, and read r's rlen
 *                           quality bytes at off[r]: q_take bytes, then NUL.  bases and qual 16-byte aligned with room for bases_cap bytes each, off
 *                           for 2 * max_records + 1 words (max_records + 1 for one text); needs bases_cap >= n_bases + 32 (nothing is written behind
 *                           n_bases).  qual NULL: bases and off alone.  bases_cap = bytes[0] + bytes[1] + 32 always suffices.
 *   names, name_off         the names back to back (names_cap >= n_name_bytes) and n_reads + 1 offsets (capacity as off)
 *   rows, len, odd          the arguments of mcx_stream_submit_packed: row_words words per read (capacity 2 * max_records rows, max_records for one
 *                           text), the lengths, and the odd bytes in (read, position) order, the same bytes on every run (odd_cap >= n_odd entries)
 * MCX_ERR_ARG before any launch: a text of 4 GiB or more (the two of a pair together: off[] holds 32-bit offsets), rows with row_words < ceil(max_read_len / 16).  A bases_cap, names_cap or odd_cap that is too
 * small: MCX_ERR_CAPACITY, info filled with the sizes needed, nothing written to THAT group (the others are complete).  The call runs on the
 * parser's stream, waits once in the middle (the capacities are judged by the host) and returns when the results are there. */
typedef struct mcx_fastq_parser mcx_fastq_parser;
int  mcx_fastq_parser_create(int device, uint64_t max_text_bytes, uint32_t max_records, mcx_fastq_parser **out); /* 0: defaults; grows on demand */
void mcx_fastq_parser_free(mcx_fastq_parser *);
enum mcx_fastq_rule { MCX_FASTQ_RULE_PLAIN = 0, MCX_FASTQ_RULE_GZ = 1 };
int  mcx_fastq_parser_set_rule(mcx_fastq_parser *, int rule); /* the rule of the parser's following calls; MCX_ERR_ARG: no such rule */
enum mcx_reads_format { MCX_READS_FASTQ = 0, MCX_READS_FASTA = 1 };
enum mcx_reads_format_bam { MCX_READS_BAM = 2 }; /* a third format: BAM records (below, "BAM read input"), set with mcx_fastq_parser_set_reads */
int  mcx_fastq_parser_set_format(mcx_fastq_parser *, int format); /* what the parser's following calls take the text for (sticky, like the rule); MCX_ERR_ARG: no such format */

typedef struct mcx_fastq_rec { uint32_t name, name_len, seq, rlen, qual, q_take; } mcx_fastq_rec; /* 24 bytes; offsets into the record's own text */
enum mcx_fastq_stop { MCX_FASTQ_MORE = 0, MCX_FASTQ_END = 1, MCX_FASTQ_EMPTY = 2, MCX_FASTQ_TOO_LONG = 3 };
enum mcx_fastq_stop_bam { MCX_FASTQ_DAMAGED = 4, MCX_FASTQ_UNPAIRED = 5 }; /* two more stops, under MCX_READS_BAM alone */

typedef struct mcx_fastq_in {
    const uint8_t *text[2]; uint64_t bytes[2];  /* text[1] NULL: one file.  Two: read 2i is record i of text[0], read 2i+1 record i of text[1]; each < 4 GiB; any alignment */
    uint32_t max_records;                       /* per text */
    int32_t max_read_len;
    int32_t final;                              /* 0: more text follows, only records whose four lines all end in '\n' inside the text are taken */
    int32_t n_ref;                              /* MCX_READS_BAM alone: the n_ref of the file's header (mcx_bam_reads_header), which a record's refID is held against */
} mcx_fastq_in;
typedef struct mcx_fastq_out {                  /* any group may be NULL: not produced */
    mcx_fastq_rec *recs[2];
    uint8_t *bases; uint32_t *off; uint8_t *qual; uint64_t bases_cap;   /* the layout of mcx_map_batch_dev / mcx_sam_in: 16-byte aligned, bases_cap >= bases + 32 */
    uint8_t *names; uint32_t *name_off; uint64_t names_cap;
    uint32_t *rows; uint32_t row_words; uint32_t *len; uint64_t *odd; uint32_t odd_cap;  /* the arguments of mcx_stream_submit_packed */
} mcx_fastq_out;
typedef struct mcx_fastq_info { uint32_t n_records[2], stop[2]; uint64_t consumed[2]; uint32_t n_reads, longest, n_odd, pad; uint64_t n_bases, n_name_bytes; } mcx_fastq_info;

int mcx_fastq_parse_dev(mcx_fastq_parser *, const mcx_fastq_in *d_in, const mcx_fastq_out *d_out, mcx_fastq_info *info); /* structs in host memory, pointers in them device pointers */
int mcx_fastq_parse(mcx_fastq_parser *, const mcx_fastq_in *in, const mcx_fastq_out *out, mcx_fastq_info *info);         /* host buffers, staged inside */

/* ---- BAM read input (MCX_READS_BAM; mcx_bam_in.hip, the rules in mcx_bam_in.h) ----------------------------------------------------------------
 * The text is what follows a BAM file's header (mcx_bam_reads_header says where): records back to back, found by the chain o -> o + 4 + block_size from offset 0.
 * One text only (text[1] != NULL: MCX_ERR_ARG); the rule setting is ignored; mcx_fastq_in.n_ref is the header's.  A record is PLAUSIBLE when
 * 32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size <= 2^28, l_read_name >= 1 with a NUL as the name's last byte, l_seq >= 0 and
 * -1 <= refID, next_refID < n_ref.  The first record that is not stops the text with MCX_FASTQ_DAMAGED; one whose bytes run past the text with MCX_FASTQ_MORE
 * (final == 0) or MCX_FASTQ_DAMAGED (final == 1); a text that ends on a record boundary with MCX_FASTQ_END.  The records before a stop count.  TAKEN are the
 * records with flag & 0x900 == 0 (secondary and supplementary lines are skipped, as `samtools fastq` skips them), and of a taken record come what the plain rule
 * gives of its FASTQ twin `@read_name\nSEQ\n+\nQUAL\n`: the name by the header rule, rlen = l_seq (0: EMPTY; > max_read_len: TOO_LONG), the bases
 * "=ACMGRSVTWYHKDBN"[nibble], the qualities min(q, 93) + 33 (none, q_take = 0, when the first quality byte is 0xFF); with flag 0x10 the read as sequenced: bases
 * reversed and complemented (IUPAC codes included), qualities reversed.  mcx_fastq_rec holds offsets into the text: seq the first packed-base byte, qual the first
 * quality byte.  consumed[0] is a record boundary: skipped records in front of a stop count as consumed.
 * mcx_fastq_parser_set_mates(parser, 1) (sticky): taken records count in twos (max_records: its even part) — the first with 0x1 and 0x40, the second with 0x1 and
 * 0x80, their names equal after the header rule; the first two that are not stop the text with MCX_FASTQ_UNPAIRED, the pairs before count; a single taken record
 * at the end gives MORE (final == 0) or UNPAIRED (final == 1); consumed[0] lies behind the last taken pair and the skipped records that follow it.
 * The records are found in chunks of 64 KB (MCX_BAM_CHUNK=bytes, at least 256: a debug override no result depends on): a search for a plausible start per chunk, a
 * walk per chunk, a join on the device that walks again every chunk the chain does not arrive at where the search said, an exclusive sum and the write.
 * mcx_bam_reads_header: 0 with *records_at (the first record's offset) and *n_ref; 1 when `bytes` holds too little of the header; -1 when the bytes are no BAM.
 * mcx_bam_reads_last: of the parser's last call — records walked, taken, skipped for 0x900, the flag of the first taken record, chunks, chunks whose searched
 * start was not on the chain. */
int mcx_bam_reads_header(const uint8_t *text, uint64_t bytes, uint64_t *records_at, int32_t *n_ref);
int mcx_fastq_parser_set_reads(mcx_fastq_parser *, int format); /* mcx_fastq_parser_set_format for all three formats: MCX_READS_FASTQ, MCX_READS_FASTA, MCX_READS_BAM (set_format itself takes its two alone, as before) */
int mcx_fastq_parser_set_mates(mcx_fastq_parser *, int mates);
int mcx_bam_reads_last(mcx_fastq_parser *, uint64_t stats[6]);
int mcx_bam_reads_last_ms(mcx_fastq_parser *, float ms[4]); /* the last call's search, walk, join and unpack on the device, by events on the parser's stream */

/* ---- files: MapCaller -i <prefix> -f A [-f2 B] -alg nw|ksw2 -sam out (src/main.cpp:212-321) */
int mcx_map_files(mcx_ctx *, const char *fq1, const char *fq2, const char *sam_path, mcx_stats *stats);
/* The same with the remaining switches of the reference's file loop (src/ReadMapping.cpp:689-760):
 * interleaved_pairs = -p (one file holds both mates alternately), host_threads = -t (parser /
 * formatter threads on the host; 0 = pick), append_sam: a further library of the same run (no
 * header, append), avg_state: carries the insert-size estimate across libraries (NULL = fresh).
 * Sharding over several GPUs (one shard each — threads of one process or processes): the input stream
 * is cut into batches of the context's max_batch_reads, batch k belongs to shard k % shard_count; a
 * shard parses (plain FASTQ: touches) and maps only its batches, and writes their lines at their final
 * place in sam_path — the same path on every shard: shard 0 creates the file and writes the header,
 * the shards learn where their batches' text goes from one another (mcx_file_opts.exchange).  avg_state
 * must be the same on every shard when the run starts; it is again when it ends (avg_state[3] = reads
 * of the whole input).
 * device_sam (mapcaller-mi355x -gpu_sam): the names and NUL-padded qualities of a batch part follow its reads to HBM, the part's text is
 * made there from the records, the CIGAR pool and the -m extras still in the slot, and comes back as text for the one writer; the
 * pool of formatter threads has nothing to do.  Same bytes in the file; buffers of about 0.6 KB per read of a batch are taken only then.
 * device_inflate (mapcaller-mi355x -gpu_inflate): a read file that is BGZF is inflated by an mcx_inflater of its own on the context's device, a stretch of
 * 8 MB of text per call, the next stretch's bytes staged meanwhile; the reader's pool of inflate threads is not created.  Same reads, same end of
 * the input at a damaged member.  Ordinary .gz and plain files are read as before (ordinary .gz: see bit 2 below).
 * device_parse (mapcaller-mi355x -gpu_parse): where the input is plain FASTQ that the front end maps into memory, the byte range of each of this shard's batches goes
 * through page-locked staging to an mcx_fastq_parser of its own on the context's device — about 0.3 KB of HBM per read of a batch, taken after the context's —, and
 * records, 2-bit rows, lengths and odd bytes come back: the reader's threads only copy.  Same reads, same end of the input, same error texts.  Plain FASTA (a
 * regular file not named .gz whose first byte is not '@': one file, or two as pairs; not sharded, not -p) no longer goes through one sequential reader per
 * file: the reader thread hands the files' bytes to the parser in chunks (final = 0, text[consumed ..) carried on, more bytes when a chunk holds too few
 * records, final = 1 at the end) and a batch's bases, offsets, names and name offsets come back into the batch's own buffer, where the host formatter,
 * device_sam and -m find them as the sequential reader leaves them; rows, lengths and odd bytes enter the slot as above (route: MCX_ROUTE_PARSE).  .gz and BGZF
 * are read as before, and so is FASTA under -p or in a sharded run.
 * device_inflate AND device_parse, THE RESIDENT ROUTE: where every read file of the call is BGZF (named .gz) and all are FASTQ (first text byte '@') or all FASTA (any other: GZ-rule FASTA, no qualities) — one file, or two as pairs —,
 * the run is not sharded, -p is off and the SAM text — if any is made — is device_sam's, the reads stay in HBM from the compressed bytes to the records: the host
 * walks the members and stages the compressed bytes; an inflater per file takes several 8 MB stretches per launch and leaves their text in a buffer in HBM; one
 * mcx_fastq_parser under the GZ rule finds a batch's records in it (final = 0, text[consumed ..) carried to the next batch), packs rows, lengths and odd bytes
 * into device buffers that travel with the batch object, which enter the slot through mcx_stream_submit_dev; names and NUL-padded qualities reach the SAM
 * kernels from the same buffers.  Only the records, or the SAM text, come back.  Same reads, same end of the input (a damaged stretch, garbage behind a member,
 * a header that is none, an empty or too long read, file 2 shorter or longer), same error texts.  HBM, taken after the context's: see DESIGN §5b.  Any other
 * combination runs exactly as without the route; mcx_files_route says which stages ran on the device.
 * device_inflate is a bit set: bit 1 (MCX_INFLATE_BGZF) is all of the above.  Bit 2 (MCX_INFLATE_GZ; mapcaller-mi355x -gpu_gz) opens the resident route to read files that are
 * ORDINARY gzip streams (gzip, pigz, a sequencer's writer): with device_parse and the route's other conditions, a file named .gz that begins with a gzip header and is not
 * BGZF is inflated by an mcx_gunzipper of its own — a round of MCX_GZ_ROUND_STRETCHES stretches at a time, its bytes staged through page-locked memory while the round
 * before is on the device, the text left behind what the file's buffer in HBM holds — and parsed under the GZ rule like a BGZF file's.  The route applies per file: a BGZF
 * file needs bit 1, an ordinary one bit 2, and a pair may mix the two kinds (route: MCX_ROUTE_GZ in place of MCX_ROUTE_INFLATE).  The first round of each ordinary file is
 * run when the files are opened: where its chain holds fewer than half of its stretches, or it has fewer than two (not text, stored blocks only, blocks longer than a
 * stretch, a small file), the route does not apply to the call, which runs as without the switch.  Bit 2 without device_parse, in a sharded run, with -p or with the host
 * formatter runs exactly as without it: the host readers, no route bit.  A round whose stream is damaged, or whose trailer's CRC-32 or ISIZE does not match, hands on
 * nothing and ends the file's input there; the rounds before it count, one line on stderr names the file and the bytes of text delivered, and the call returns what the
 * host route returns (the end of a file's input is no error).  How many reads precede a damaged place depends on the round size, here as with the host reader's rounds:
 * the two routes deliver whole rounds, and theirs differ.  HBM per ordinary file, taken after the context's: 2 bytes a symbol of a round (8 symbols a compressed byte),
 * 96 KB a stretch, the staging twins of a round's compressed bytes, and the file's text (MCX_ALLOC_LOG=1 itemises it).
 * Debug overrides (no result depends on them): MCX_GZ_STRETCH=bytes (default 65536, at least 4096), MCX_GZ_ROUND_STRETCHES=n (default 512) — the tests put many stretches
 * and rounds into small files with them.
 * device_sam is a bit set: bit 1 (MCX_SAM_DEVICE) is the above, bit 2 (MCX_SAM_BGZF; mapcaller-mi355x -bgzf) writes the SAM file as BGZF and implies bit 1, because the text
 * has to be in HBM: every part's text is compressed where it lies by an mcx_deflater of the run's own (each part starts a fresh block) and only the blocks come back for
 * the one writer; the header goes out as blocks of its own, and the 28-byte EOF block ends the file.  A library appended with append_sam starts over the previous EOF
 * block, so a finished file has exactly one, at its end; on a stream (sam_path "-") every library ends with its own, which readers skip.  gzip -d of the file is, byte
 * for byte, the SAM file written without the bit, and the same input gives the same file on every run.  On every input route that device_sam works on, the resident
 * route and -m included; with shard_count > 1 the call returns MCX_ERR_UNSUPPORTED before anything is opened.  (route: MCX_ROUTE_BGZF.)
 * bit 4 (MCX_SAM_BAM; mapcaller-mi355x -bam) writes BAM instead and implies bits 1 and 2: the header is mcx_bam_header's bytes as BGZF blocks of their own, every part's
 * records are made by mcx_bam_format_dev's kernels into the buffer the deflater reads, and everything else is the BGZF path above (fresh block per part — a record may
 * straddle the blocks within a part —, EOF block, append_sam over the previous EOF block with no second header, stdout, MCX_BGZF_BLOCK, the resident route, -m, the
 * refusal of shard_count > 1).  gzip -d of the file is the uncompressed BAM stream htslib makes of the SAM lines; no index is written, nothing is sorted.  The lines
 * left out (mcx_bam_format_dev) are counted over the call and the total printed to stderr once, when it is not 0 (MCX_TIMING=1: beside the bgzf line, always).  (route: MCX_ROUTE_BAM.)
 * bit 8 (MCX_SAM_SORT; mapcaller-mi355x -sort; only with bit 4) makes the file a coordinate-sorted BAM (mcx_bam_sort_dev's order, stable from the first read to the
 * last: a function of the input alone, whatever the batch, block or chunk size).  Every part's records are sorted before they are compressed and go, as a run, to a
 * temporary file (sam_path + ".sort.tmp"; for "-": ${TMPDIR:-/tmp}/mcx_sort.<pid>.tmp), of the size of the unsorted file, removed when the call returns, however it
 * returns; the host keeps 12 bytes a record (key, length) and 24 bytes a block.  Behind the last batch the runs are cut by key into chunks of about 256 MB of
 * records (MCX_SORT_CHUNK=bytes: a debug switch) — equal keys never in two chunks —, and every chunk's slices are read back, inflated, sorted and compressed on the
 * device and written behind mcx_bam_header_sorted's header; a pile-up on one key makes a chunk that HBM must hold whole (MCX_ERR_CAPACITY when it does not).
 * MCX_ERR_UNSUPPORTED before anything is opened: the bit without bit 4, append_sam (a sorted file cannot be appended to), shard_count > 1.  (route: MCX_ROUTE_SORT.)
 * bit 16 (MCX_SAM_INDEX; mapcaller-mi355x -index; only with bit 8) writes sam_path + ".bai" as well, the index samtools index would make of the file (format BAI; the
 * same chunks, meta pairs and linear entries as htslib's hts_idx_push / hts_idx_finish, a contig's bins listed ascending — a function of the BAM file alone): after
 * each chunk of the merge is compressed, mcx_bam_index_dev reads its records, which still lie in HBM, against the places of the chunk's blocks in the file, and
 * the host keeps 24 bytes a stretch of records with one (contig, bin).  The index is written — under another name, then renamed — once the BAM file is complete
 * and closed, and removed when the call fails; the BAM file's bytes are those of a run without the bit.  MCX_ERR_UNSUPPORTED before anything is opened: the bit
 * without bit 8, sam_path "-" (no name to put the index beside), a contig longer than 2^29 (BAI cannot address it; CSI is not offered).  (route: MCX_ROUTE_INDEX.)
 * bit 32 (MCX_SAM_MARKDUP; mapcaller-mi355x -markdup; only with bit 8) sets flag bit 0x400 on every record that is a duplicate by the rule at mcx_bam_dup_units_dev;
 * the file's bytes after gzip -d are those of a run without the bit but for that flag bit, and a function of the input alone.  Before a part is sorted its units are
 * made from the records in read order (a pair's mates are neighbouring groups: a paired part with an odd number of reads is refused in words) and come back beside
 * the keys and lengths, with the group every sorted record came from; behind the last batch all units go to HBM once, mcx_dup_resolve_dev decides, and every
 * chunk of the merge marks its sorted records before they are compressed (-index reads marked records).  Host memory on top of -sort's 12 bytes a record: 4 bytes
 * a record and 24 bytes a unit (12 a record for pairs) until the resolve, 1 byte a record from there on.  There is no optical-duplicate distance, no library or
 * read-group distinction (-sort takes one library), and same-strand pairs are not told apart by which mate comes first.  One line on stderr says what was found.
 * MCX_ERR_UNSUPPORTED before anything is opened: the bit without bit 8; a context with -m (mcx_ctx_set_multi).  (route: MCX_ROUTE_MARKDUP.)
 * bit 64 (MCX_SAM_MD; mapcaller-mi355x -md) puts an MD:Z tag behind XS on every mapped line (mcx_md_dev's strings): behind a batch part's mapping its strings are
 * made in HBM from the part's reads, records, CIGAR pool and (-m) extras, which carry their own; with bit 1 they feed the device formatters where they lie (SAM
 * text, BGZF, BAM; -sort, -markdup and -index see only longer records), without it they come to the host with the part's records and the host formatter appends
 * them.  Without the bit every file is byte for byte what it was.  MCX_ERR_UNSUPPORTED before anything is opened: shard_count > 1.
 * bit 128 (MCX_SAM_MC; mapcaller-mi355x -mc) puts MC:Z and MQ:i on the lines of pairs, and read_group of mcx_map_files_rg (mapcaller-mi355x -rg) an @RG line into the
 * header and RG:Z on every line: the rule stands at mcx_sam_tags.  The ID goes to HBM once per run and the device formatters make the tags where they make the
 * line (SAM text, BGZF, BAM; -sort, -markdup and -index see only longer records); without bit 1 the host formatter writes the same bytes — a pair's mates are always
 * in the same part of a batch.  The header line is written on every route, also by the merge of a sorted file; an append_sam library gets the same group's tags and
 * no second header line.  MCX_ERR_UNSUPPORTED before anything is opened: either of them with shard_count > 1; bit 128 on a context with -m (mcx_ctx_set_multi);
 * read_group works with -m.  A read_group that mcx_rg_parse would refuse: MCX_ERR_ARG before anything is opened.
 * Debug override (no result depends on it): MCX_BGZF_BLOCK=n, the bytes of text per BGZF block (1 .. 65280, the default; the tests put many blocks into small files with it).
 * Debug override (no result depends on it): MCX_RESIDENT_LAUNCH_BYTES=n, the bytes of text one inflate launch of the resident route makes (default 128 MB: sixteen
 * stretches; smaller than a stretch: the stretch takes several launches — the tests put many launch and carry boundaries into small files with it). */
typedef struct mcx_file_opts {
    int32_t interleaved_pairs, host_threads, append_sam;
    int32_t device_sam; /* bits of mcx_sam_bits.  1: the SAM text is made on the device (mcx_sam_format_dev's kernels) instead of by host threads; 0: as before */
    int64_t *avg_state; /* int64_t[4], see mcx_avg_init */
    int32_t shard_rank, shard_count; /* 0, 0: the whole input */
    int32_t device_inflate; /* bits of mcx_inflate_bits.  1: BGZF input is inflated and CRC-checked on the device (mcx_inflate's kernel) instead of by a pool of host threads; 2: ordinary gzip streams take the resident route (with device_parse); 0: as before */
    int32_t device_parse; /* 1: plain FASTQ input is parsed and packed to 2-bit rows on the device (mcx_fastq_parse's kernels) instead of by the reader's pool of host threads; 0: as before */
    const mcx_exchange *exchange;    /* required when shard_count > 1: the shards walk ONE insert-size trajectory and
                                        decide the duplicate cap over ONE input order, so that SAM and profile equal the
                                        single-stream run's (rank/size must equal shard_rank/shard_count) */
} mcx_file_opts;
enum mcx_inflate_bits {
    MCX_INFLATE_BGZF = 1, /* mapcaller-mi355x -gpu_inflate: BGZF read files are inflated on the device */
    MCX_INFLATE_GZ = 2    /* mapcaller-mi355x -gpu_gz: ordinary gzip streams are, on the resident route (needs device_parse; alone it changes nothing) */
};
enum mcx_sam_bits {
    MCX_SAM_DEVICE = 1, /* the SAM text is made on the device */
    MCX_SAM_BGZF = 2,   /* ... and leaves it as BGZF blocks (implies MCX_SAM_DEVICE) */
    MCX_SAM_BAM = 4,    /* ... which hold BAM records instead of SAM text (implies both) */
    MCX_SAM_SORT = 8,   /* ... in coordinate order (only with MCX_SAM_BAM) */
    MCX_SAM_INDEX = 16, /* ... with its .bai written beside it (only with MCX_SAM_SORT) */
    MCX_SAM_MARKDUP = 32, /* ... and flag bit 0x400 on its duplicate records (only with MCX_SAM_SORT) */
    MCX_SAM_MD = 64,     /* an MD:Z tag on every mapped line, made on the device (mcx_md_dev); with any of the above, and with none: the host formatter appends it */
    MCX_SAM_MC = 128     /* MC:Z and MQ:i on the lines of pairs (the rule: mcx_sam_tags); with any of the above, and with none */
};
void mcx_file_opts_default(mcx_file_opts *);
int mcx_map_files_ex(mcx_ctx *, const char *fq1, const char *fq2, const mcx_file_opts *, const char *sam_path, mcx_stats *stats);
/* mcx_map_files_ex with a read group: read_group is the validated @RG line with real TABs and no newline (mcx_rg_parse's line, NUL-terminated); NULL: none, and
 * the call is mcx_map_files_ex.  (mcx_file_opts keeps its layout: the line travels beside it.) */
int mcx_map_files_rg(mcx_ctx *, const char *fq1, const char *fq2, const mcx_file_opts *, const char *read_group, const char *sam_path, mcx_stats *stats);
/* Which stages of the context's last mcx_map_files* call ran on the device, per read file (route[1] = 0 for one file): the opt-in switches that do not apply
 * to an input are ignored without a word, and the output is the same bytes by design.  MCX_TIMING=1 prints it. */
enum mcx_route {
    MCX_ROUTE_INFLATE = 1, /* the file's BGZF members were inflated on the device */
    MCX_ROUTE_PARSE = 2,   /* its records were found and packed on the device */
    MCX_ROUTE_ROWS = 4,    /* its batches entered their slots from HBM (mcx_stream_submit_dev): the resident route */
    MCX_ROUTE_SAM = 8,     /* the SAM text was made on the device */
    MCX_ROUTE_BGZF = 16,   /* ... and compressed to BGZF blocks there */
    MCX_ROUTE_BAM = 32,    /* ... as BAM records, not text */
    MCX_ROUTE_SORT = 64,   /* ... sorted by coordinate and merged on the device */
    MCX_ROUTE_INDEX = 128, /* ... and indexed there: the .bai is made of what the merge's chunks say of their records */
    MCX_ROUTE_MARKDUP = 256, /* ... their duplicates decided and flagged there */
    MCX_ROUTE_GZ = 512,    /* the file's gzip stream was inflated on the device */
    MCX_ROUTE_BAM_IN = 1024 /* the file is BAM: its records were found and unpacked on the device (beside INFLATE | PARSE | ROWS) */
};
int mcx_files_route(mcx_ctx *, uint32_t route[2]);
/* What the context's last mcx_map_files* call with MCX_SAM_SORT did: runs, chunks of the merge, slices, slices that start inside a BGZF block, bytes read back from
 * the temporary file, and how many of those were read twice (the blocks at slice borders).  All 0 after a sorted run that failed. */
int mcx_files_sort_stats(mcx_ctx *, uint64_t stats[6]);
/* What the context's last mcx_map_files* call with MCX_SAM_INDEX wrote: stretches (maximal runs of records with one contig and bin, after joining across the
 * merge's chunks), bins written (the pseudo-bins included), linear-index entries, and the .bai file's bytes.  All 0 after an indexed run that failed. */
int mcx_files_index_stats(mcx_ctx *, uint64_t stats[4]);
/* What the context's last mcx_map_files* call with MCX_SAM_MARKDUP found: pair units, duplicate pair units, fragment units, duplicate fragment units, groups (keys
 * that two or more pair units share, plus ends on which a fragment is a duplicate), and the microseconds the units, the resolve and the marks took.  All 0 after a run that failed. */
int mcx_files_markdup_stats(mcx_ctx *, uint64_t stats[6]);

#ifdef __cplusplus
}
#endif
#endif
