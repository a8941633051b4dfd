// mapcaller_amd/csrc/mcx_internal.h — what the translation units of libmcx.so share (not part of the ABI)
#ifndef MCX_INTERNAL_H
#define MCX_INTERNAL_H
#include "mcx_types.h"
#include "mcx_host.h"
#include "mcx_build.h"
#include "../../include/mcx.h"
#include "mcx_bai.h"
#include <atomic>
#include <vector>

struct mcx_index {
    mcx::IndexView view;
    mcx::HostIndex host;
    int device = 0;
    void *d_bwt = nullptr, *d_sa = nullptr, *d_sa_full = nullptr, *d_pac = nullptr;
    void *d_end_pos = nullptr, *d_end_chr = nullptr, *d_chr_fwd = nullptr, *d_ktab = nullptr, *d_rank = nullptr;
    void *d_hole_off = nullptr, *d_hole_len = nullptr, *d_hole_letter = nullptr; // the .amb file's ambiguity holes (host.hole_*), for the MD strings alone (mcx_md.hip); null: none
    void *d_rank2 = nullptr, *d_rank2_c2 = nullptr; // pair records (mcx_fm.h PairSlot): built when the index is made with full_sa = 2
    int64_t rank2_bytes = 0;
    int pair_records = 0;
    int64_t hbm_bytes = 0;
    uint64_t n_bwt_words = 0, n_sa = 0; // set for indexes built in HBM (mcx_index_from_codes)
    mutable std::atomic<int> n_ctx{0};  // contexts alive on this index (mcx_ctx_create / mcx_ctx_free): mcx_index_trim refuses while there are any
    mutable std::atomic<bool> orphan{false}; // mcx_index_free was called while contexts were alive: the last mcx_ctx_free deletes this object
};

// what the file front end (mcx_files.cpp) needs to know about a context
const mcx_index *mcx_ctx_index(const mcx_ctx *);
int mcx_ctx_max_read_len(const mcx_ctx *);
uint64_t mcx_ctx_max_reads(const mcx_ctx *);
// host buffers <-> the context's staging arrays in HBM, on the context's stream (stage_out waits for it)
int mcx_stage_in(mcx_ctx *, const uint8_t *bases, const uint32_t *off, uint32_t n_reads, const uint8_t **d_bases, const uint32_t **d_off,
                 mcx_aln **d_aln, uint32_t **d_cigar);
int mcx_stage_out(mcx_ctx *, uint32_t n_reads, mcx_aln *aln, uint32_t *cigar);
bool mcx_ctx_has_profile(const mcx_ctx *);
bool mcx_ctx_multi(const mcx_ctx *); // -m is on (mcx_ctx_set_multi)
// something the file front end keeps with the context from call to call (its page-locked batch buffers): *slot, freed with
// `drop` when the context goes
void **mcx_ctx_files_slot(mcx_ctx *, void (*drop)(void *));
// the same for mcx_sam.hip's device buffers, and the stream (a hipStream_t) the context's kernels run on
void **mcx_ctx_sam_slot(mcx_ctx *, void (*drop)(void *));
void *mcx_ctx_stream(mcx_ctx *);
// -bgzf: the run's deflater with its block size, and what it has done so far (text in, blocks out, seconds of the calling thread); bam (-bam): what goes in is
// not a part's SAM text but its BAM records (mcx_bam.hip), and dropped counts the lines that made none
// sort (-sort; null: none): the part's records are put into coordinate order before they are compressed (mcx_bam_sort.hip), and the sorted keys and lengths of
// the part — a run of the merge — arrive in the sink
// dup (-markdup; null: none): the run's units so far — the part's own from part_base on, made before it is sorted (mcx_markdup.hip) — and per sorted record of the
// part the group (read) it came from; behind the last batch the resolve's groups; device ms and seconds of the calling thread for units, resolve and marks
struct mcx_dup_sink {
    std::vector<mcx_dup_unit> units; uint64_t part_base = 0; int part_paired = 0;
    std::vector<uint32_t> grp;
    uint64_t groups = 0;
    float ms[3] = {0, 0, 0}; double seconds[3] = {0, 0, 0};
};
struct mcx_sort_sink { std::vector<uint64_t> keys; std::vector<uint32_t> lens; double run_seconds = 0; mcx_dup_sink *dup = nullptr; };
struct mcx_sam_bgzf { mcx_deflater *deflater; uint32_t block; uint64_t text_bytes, out_bytes; double seconds; int bam; uint64_t dropped; mcx_sort_sink *sort; };
// -gpu_sam (mcx_sam.hip): the text of one mapped part of a batch, from its slot in HBM to (*text)[at ..] in page-locked host memory; bgzf (null: none): the text is
// compressed in HBM first and its BGZF blocks arrive instead, *n_bytes their size
int mcx_sam_part(mcx_ctx *, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired, const uint8_t *names, const uint32_t *name_off,
                 const uint8_t *qual, uint64_t qual_bytes, const mcx_aln *d_aln, const uint32_t *d_cigar, uint8_t **text, uint64_t *text_cap, uint64_t at, uint64_t *n_bytes, mcx_sam_bgzf *bgzf);
// -bam (mcx_bam.hip): mcx_bam_format_dev for sam_part's input — the records of a part into d_out[0 .. cap), *n_bytes their exact size (MCX_ERR_CAPACITY, nothing
// written, when cap is smaller), *n_dropped the lines that made none; the context's device is current
int mcx_bam_part_dev(mcx_ctx *, const mcx_sam_in *d_in, const mcx_sam_tags *tags, uint8_t *d_out, uint64_t cap, uint64_t *n_bytes, uint64_t *n_dropped);
// -rg / -mc (mcx_sam.hip): the read group's ID goes to HBM once per run; the context's following mcx_sam_part[_dev] calls hand it, and the mate-tag switch, to their
// formatter.  (nullptr, 0, 0) at the end of the run: both off, the ID's bytes freed.
int mcx_tags_set(mcx_ctx *, const char *id, uint32_t id_len, int mate_tags);
// -md (mcx_md.hip).  set: the context's following mcx_sam_part[_dev] calls make their part's MD strings first and hand them to the formatter.  part_dev: the
// strings of `in`'s lines (n_extras: the context's extras of the part) into the formatter state's own pool, which in->md / in->md_off then point at.  part_host:
// the same for a part still in its slot whose text the host makes: the strings and their offsets (n_reads + extras + 1 entries) come back with the part.
void mcx_md_set(mcx_ctx *, int on);
bool mcx_md_wanted(mcx_ctx *);
int mcx_md_part_dev(mcx_ctx *, mcx_sam_in *in, uint32_t n_extras, uint64_t *n_bytes);
int mcx_md_part_host(mcx_ctx *, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired, const mcx_aln *d_aln, const uint32_t *d_cigar,
                     std::vector<uint8_t> *md, std::vector<uint32_t> *md_off);
// -sort (mcx_bam_sort.hip).  part: what mcx_bam_part_dev just made (n_reads groups, n_bytes) in key order in a buffer of the state's own, *d_sorted; keys and
// lengths into the sink.  chunk: one chunk of the merge, from the blocks read back from the temporary file to the blocks of the sorted file (see there).
int mcx_bam_sort_part(mcx_ctx *, uint32_t n_reads, uint64_t n_bytes, mcx_sort_sink *sink, const uint8_t **d_sorted);
int mcx_bam_sort_chunk(mcx_ctx *, mcx_inflater *, mcx_deflater *, uint32_t block, const uint8_t *src, uint64_t src_bytes, const mcx_deflate_member *members, uint32_t n_members,
                       uint64_t text_bytes, const uint32_t *lens, uint64_t n_records, const uint64_t *slice_first, const uint64_t *slice_base, uint32_t n_slices, uint64_t rec_bytes,
                       uint8_t **h_out, uint64_t *h_out_cap, uint64_t *n_out, double secs[4], struct mcx_bai_sink *bai, uint64_t file_at, mcx_dup_sink *dup, const uint8_t *dup_bytes);
// -markdup (mcx_markdup.hip).  part: the units of what mcx_bam_part_dev just made (n_reads groups in read order, n_bytes; paired: reads 2i and 2i + 1 are mates)
// behind the sink's units.  resolve: all of the sink's units to HBM, *dup one byte a unit back.  chunk: a sorted chunk of the merge (d_rec_off: n + 1 entries)
// gets its flag bits — h_dup[n] in the order the chunk's records came in, d_perm the sort's permutation.
int mcx_markdup_part(mcx_ctx *, uint32_t n_reads, uint64_t n_bytes, int paired, mcx_dup_sink *);
int mcx_markdup_resolve(mcx_ctx *, mcx_dup_sink *, std::vector<uint8_t> *dup);
int mcx_markdup_chunk(mcx_ctx *, mcx_dup_sink *, uint8_t *d_recs, const uint64_t *d_rec_off, uint32_t n, const uint8_t *h_dup, const uint32_t *d_perm);
// -index (mcx_bai.hip): the index of the file the merge writes.  begin: the windows' table of the context's contigs in HBM, all-ones.  chunk: the records just
// deflated (d_rec_off: n + 1 entries; the deflater still knows where their blocks lie) whose blocks will go to byte file_at of the file: their stretches join the
// accumulator, their windows the table.  end: the table comes back and the file's bytes are made, eof_at the byte the EOF block is written at.  The sink's
// device arrays go with mcx_bai_free.
struct mcx_bai_sink {
    mcx::bai::Index acc;
    std::vector<uint64_t> lin_base;                       // n_ref + 1: where each contig's windows begin in the table
    uint64_t *d_lin = nullptr, *d_lin_base = nullptr;
    mcx_bai_run *d_runs = nullptr; uint64_t cap_runs = 0;
    std::vector<mcx_bai_run> h_runs;
    mcx::bai::Stats stats;
    double seconds = 0;                                   // of the calling thread, all three
    float ms[3] = {0, 0, 0};                              // the device's, summed over the chunks: records, stretches, windows
};
int mcx_bai_begin(mcx_ctx *, mcx_bai_sink *);
int mcx_bai_chunk(mcx_ctx *, mcx_bai_sink *, const uint8_t *d_recs, uint64_t n_bytes, const uint64_t *d_rec_off, uint32_t n_records, uint32_t block, mcx_deflater *, uint64_t file_at);
int mcx_bai_end(mcx_ctx *, mcx_bai_sink *, uint64_t eof_at, std::vector<uint8_t> *bytes);
void mcx_bai_free(mcx_ctx *, mcx_bai_sink *);
// -gpu_inflate (mcx_inflate.hip): the host form of mcx_inflate in two halves, so that the reader stages a stretch's bytes while the stretch before is on
// the device — begin packs the members' bytes (src_off into src) into page-locked staging and queues copy in, kernel and copy out; end waits for the oldest
// begin and hands the text to dst + each member's dst_off (0, or MCX_ERR_IO when a member failed).  At most two begins outstanding; caps: what one holds.
int mcx_inflate_begin(mcx_inflater *, const uint8_t *src, uint64_t src_bytes, const mcx_deflate_member *members, uint32_t n, uint64_t dst_cap);
int mcx_inflate_end(mcx_inflater *, uint8_t *dst, uint32_t *status, uint32_t *n_bad);
void mcx_inflater_caps(const mcx_inflater *, uint64_t *max_src, uint64_t *max_dst, uint32_t *max_members);
// ... and for text that stays in HBM (the resident route): an inflater without buffers for the text, and a begin whose members' dst_off point into d_dst, a buffer
// of dst_cap bytes on the inflater's device — any sum of isize, so several stretches go in one launch; mcx_inflate_end (dst: null) hands out the status words
int mcx_inflater_create_dev(int device, uint64_t max_src_bytes, uint32_t max_members, mcx_inflater **out);
int mcx_inflate_begin_dev(mcx_inflater *, const uint8_t *src, uint64_t src_bytes, const mcx_deflate_member *members, uint32_t n, uint8_t *d_dst, uint64_t dst_cap);
// mcx_sam_part for names, name offsets and NUL-padded qualities in HBM (mcx_fastq_parse_dev's outputs): nothing is copied in
int mcx_sam_part_dev(mcx_ctx *, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n_reads, int paired, const uint8_t *d_names, const uint32_t *d_name_off,
                     const uint8_t *d_qual, const mcx_aln *d_aln, const uint32_t *d_cigar, uint8_t **text, uint64_t *text_cap, uint64_t at, uint64_t *n_bytes, mcx_sam_bgzf *bgzf);
// mcx_fastq_parse_dev in two halves: the caller sizes its buffers from *info in between
int mcx_fastq_dev_sizes(mcx_fastq_parser *, const mcx_fastq_in *in, mcx_fastq_info *info);
int mcx_fastq_dev_out(mcx_fastq_parser *, const mcx_fastq_out *out, const mcx_fastq_info *info);
// MCX_READS_BAM (mcx_bam_in.hip): the two passes of a parser whose format is BAM, on the parser's stream (a hipStream_t) — *state is made by the first sizes call
// and freed with the parser; last: mcx_bam_reads_last's counters and the stages' ms (either may be null; a null state gives zeros)
struct mcx_bam_in;
int mcx_bam_in_sizes(mcx_bam_in **state, void *stream, const mcx_fastq_in *in, int mates, mcx_fastq_info *info, const char *who);
int mcx_bam_in_out(mcx_bam_in *, void *stream, const mcx_fastq_out *out, const mcx_fastq_info *info, const char *who);
void mcx_bam_in_last(const mcx_bam_in *, uint64_t stats[6], float ms[4]);
uint32_t mcx_bam_in_grown(const mcx_bam_in *);
void mcx_bam_in_free(mcx_bam_in *);
// -gpu_parse (mcx_fastq.hip): the host form of mcx_fastq_parse in three steps — stage hands out the parser's page-locked staging for two texts of these sizes
// (the reader's pool copies the batch's byte ranges into it); staged_sizes sends them to HBM and parses: *info says how many reads, odd bytes, how long the longest;
// staged_out brings the groups of `out` (HOST pointers, page-locked ones without a further copy) back — rows with row_words 0 come ceil(longest / 16) words wide.
int mcx_fastq_stage(mcx_fastq_parser *, const uint64_t bytes[2], uint8_t *h[2]);
int mcx_fastq_staged_sizes(mcx_fastq_parser *, const uint64_t bytes[2], int two, uint32_t max_records, int32_t max_read_len, int32_t final, mcx_fastq_info *info);
int mcx_fastq_staged_out(mcx_fastq_parser *, const mcx_fastq_out *out, const mcx_fastq_info *info);
// (the file front end's readers) a BGZF member at p (n bytes left in the file): its whole size and the length of its extra field; 0 if it is not one
static inline size_t mcx_bgzf_member_at(const uint8_t *p, size_t n, size_t &xlen)
{
    if (n < 28 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
    xlen = (size_t)p[10] | ((size_t)p[11] << 8);
    if (12 + xlen + 8 > n) return 0;
    for (size_t o = 12; o + 4 <= 12 + xlen;) { // the subfields of the extra field: SI1 SI2 SLEN(2) data
        const size_t slen = (size_t)p[o + 2] | ((size_t)p[o + 3] << 8);
        if (p[o] == 'B' && p[o + 1] == 'C' && slen == 2 && o + 6 <= 12 + xlen) {
            const size_t size = ((size_t)p[o + 4] | ((size_t)p[o + 5] << 8)) + 1;
            return (size >= 12 + xlen + 8 && size <= n) ? size : 0;
        }
        o += 4 + slen;
    }
    return 0;
}
// The resident route (mcx_resident.hip; -gpu_inflate / -gpu_gz with -gpu_parse): one or two read files whose text never leaves HBM.  kinds: mcx_file_opts.device_inflate's bits — a BGZF file
// needs MCX_INFLATE_BGZF, an ordinary gzip stream MCX_INFLATE_GZ (and a first round whose chain holds at least half of its stretches).  open: *out stays null (and
// the call returns 0) when a file is no BGZF file named .gz, has no text, or the files are not all FASTQ (first text byte '@') or all FASTA — the route does not apply.  next: the next batch of up to
// per_file records a file — more members inflated as needed, the records found under the GZ rule, rows / lengths / odd bytes (and, want_sam, names, their
// offsets and NUL-padded qualities) written to *bufs, device buffers that belong to the caller's batch object (made on first use, grown on demand, freed with
// mcx_resident_bufs_free).  One host thread per object.
struct mcx_resident;
struct mcx_resident_bufs;
struct mcx_resident_batch {
    uint32_t n_records[2];     // records each file gave: per_file, or fewer where its records ended (then `last`)
    bool last[2];
    char too_long[2][128];     // the name of the read that ended a file because it is longer than max_read_len (has_too_long); whole: header_of ends a name within the header's first 100 bytes
    bool has_too_long[2];
    uint32_t n_reads;          // reads in the buffers: n_records[0], or 2 * n_records[0] mate by mate — 0 when file 2 gave fewer than file 1 or a read is too long
    const uint32_t *rows, *len; const uint64_t *odd; uint32_t row_words, n_odd, longest; // mcx_stream_submit_dev's arguments
    const uint8_t *names, *qual; const uint32_t *name_off;                              // mcx_sam_part_dev's (qual null: FASTA)
    uint64_t n_bases, n_name_bytes;                                                     // (plain) what mcx_resident_host_out's bases and names groups hold
};
int mcx_resident_open(int device, const char *const paths[2], int n_files, uint32_t kinds, bool bam, mcx_resident **out);
// bam (the one file is BGZF and its text begins "BAM\1", whatever its name): the header is walked behind the first launch, the records are found and unpacked under
// MCX_READS_BAM, and the first taken record's flag 0x1 says whether next hands out pairs (bam_paired: an even number of records a batch, mate by mate) or single
// reads.  A file that cannot be read so is an error, not a fallback.  next: mates that are not neighbours fail with MCX_ERR_ARG; a damaged record ends the input
// with one line on stderr.
bool mcx_resident_bam(const mcx_resident *);
bool mcx_resident_bam_paired(const mcx_resident *);
// MCX_ROUTE_INFLATE or MCX_ROUTE_GZ: how file f's text came to be in HBM
uint32_t mcx_resident_inflate_bit(const mcx_resident *, int f);
// The same object over plain FASTA files (-gpu_parse): the files' bytes go to HBM a launch at a time, the records are plain-rule FASTA's, and next leaves the
// batch on the device (bufs: unused): host_out brings the groups of `out` (HOST pointers; rows with row_words 0 come ceil(longest / 16) words wide) back, any
// number of times until the next batch is asked for.  fasta: the files are FASTA (either open).
int mcx_resident_open_plain(int device, const char *const paths[2], int n_files, mcx_resident **out);
int mcx_resident_host_out(mcx_resident *, const mcx_fastq_out *out);
bool mcx_resident_fasta(const mcx_resident *);
void mcx_resident_close(mcx_resident *);
int mcx_resident_next(mcx_resident *, mcx_resident_bufs **bufs, uint32_t per_file, int32_t max_read_len, bool want_sam, mcx_resident_batch *out);
void mcx_resident_bufs_free(mcx_resident_bufs *);
// -gpu_gz (mcx_gz_dev.hip): mcx_gunzip_round_dev in two halves — begin queues the search, the inflate and the copy of the stretches' records and returns at once, end
// waits, walks the chain and runs the windows — and an ordinary .gz file as a whole: the one walker of members, trailers and staging (mcx_gz_dev.h's Reader), for
// mcx_gz_inflate_dev and the resident route.  open: data[0 .. size) is the whole file and outlives the object; *out stays null (the call returns 0) when it does
// not begin with a gzip header.  next: 1 — a round whose info->text_bytes of text (0 is possible) mcx_gz_file_text fetches into d_dst —, 0 at the input's end
// (failed: where the stream is damaged), or an error.  text: *counts false — the member's trailer does not match: nothing of the round is handed on, the input ends.
struct mcx_gz_file;
int mcx_gunzip_round_begin(mcx_gunzipper *, const uint8_t *d_src, uint64_t src_bytes, uint32_t start_bit, int src_is_end);
int mcx_gunzip_round_end(mcx_gunzipper *, mcx_gz_round *info);
int mcx_gz_file_open(int device, const uint8_t *data, size_t size, uint64_t stretch_bytes, uint32_t round_stretches, mcx_gz_file **out);
int mcx_gz_file_next(mcx_gz_file *, mcx_gz_round *info);
int mcx_gz_file_text(mcx_gz_file *, uint8_t *d_dst, uint64_t dst_cap, mcx_gz_round *info, bool *counts);
bool mcx_gz_file_failed(const mcx_gz_file *);
uint64_t mcx_gz_file_delivered(const mcx_gz_file *);
void mcx_gz_file_staging(const mcx_gz_file *, uint64_t *rounds, uint64_t *staged_hits); // rounds begun, and those whose bytes the prefetch had staged
void mcx_gz_file_free(mcx_gz_file *);
void *mcx_pinned_alloc(size_t bytes); // page-locked host memory (null on failure); mcx_pinned_free accepts null
void mcx_pinned_free(void *);

#endif
