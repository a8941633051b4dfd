// mapcaller_amd/csrc/mcx_files.cpp — files in, SAM text out, around the batch API (host only): the run itself and the C entry points.
// Its parts: mcx_pool.h (host threads, queues), mcx_reader.h (the readers), mcx_batch.h (the batch object, the host formatter), mcx_shards.h (several shards).
//
// Replaces the reading and writing halves of the reference's ReadMapping() loop: GetNextChunk /
// gzGetNextChunk (src/GetData.cpp:85-140) and Generate{Paired,Single}SamStream + fprintf
// (src/SamReport.cpp:324-488, src/ReadMapping.cpp:536-546).  The reference does both per 200-read
// chunk under locks; at GPU mapping rates they are the wall, so here
//   * a plain FASTQ file is mapped into memory and indexed by line count (a record is four lines from
//     the start of the file, whatever the lines hold — GetData.cpp:45-55), in parallel; a batch is then
//     parsed by a pool of host threads, each from the first byte of its own stretch of records, with
//     the reads' names, bases and qualities left where they lie in the file (the SAM formatter reads
//     them there) and the bases packed to 2 bits on the way (a quarter of the bytes cross PCIe); a
//     shard of a several-GPU run touches only the bytes of its own batches;
//   * .gz files and FASTA go through one sequential reader per file (zlib / multi-line records) — except BGZF input with -gpu_inflate -gpu_parse, whose text
//     stays in HBM from the compressed bytes on (the resident route, mcx_resident.hip): the reader thread then only asks for the next batch, the mapper
//     submits it from HBM (mcx_stream_submit_dev) and the SAM kernels take names and qualities where the parser left them; and except plain FASTA with
//     -gpu_parse, whose bytes go to HBM in chunks and whose records, bases, names, rows and odd bytes come back from the device parser;
//   * batches flow through parse | copy in, map, copy out (three device slots: the copies of one
//     batch under the kernels of its neighbours) | format + write;
//   * SAM lines are formatted by a second pool into per-slice buffers and written with positioned
//     writes, every slice at its final place in the file — by every shard into the one output file:
//     the shards tell each other their batches' sizes with the rounds' other messages.
//   * with -sort (only -bam) every part's records are sorted on the device before they are compressed and go as a run to a temporary file, of which the
//     host keeps keys, lengths and block tables; behind the last batch merge() cuts the runs by key into chunks (mcx_sort_plan.h) and reads back, inflates,
//     sorts, deflates and writes each of them — every step one bulk operation (mcx_bam_sort.hip).
// Text semantics follow the reference byte for byte: header trimming (GetData.cpp:3-20), the last
// byte of a FASTQ sequence line dropped (:48-53), multi-line FASTA for plain files (:56-77), the
// 1024-byte line buffer, the '@'/'>' check and single-line FASTA of the .gz reader (:101-128), an
// odd tail chunk of interleaved input mapped as single reads (ReadMapping.cpp:442).
//
// A run is a Run object: open_input() chooses one of four input routes, open_output() sets the SAM file up, then three threads (read_loop, format_loop,
// write_loop) work beside the calling thread's map_loop(), batch objects going round between them through four queues.
#include <sys/file.h>

#include "mcx_tags.h"
#include "mcx_batch.h"
#include "mcx_shards.h"
#include "mcx_sort_plan.h"

using namespace mcx;
using namespace mcx::files;

extern "C" void mcx_file_opts_default(mcx_file_opts *o) { memset(o, 0, sizeof *o); }

// what the file front end keeps with a context from call to call: its batch objects (page-locked and device buffers: slow to get), and which stages of the
// last call ran on the device
namespace {
typedef std::unique_ptr<Batch> BatchPtr;
struct Kept { std::vector<BatchPtr> objects; uint32_t route[2] = {0, 0}; uint64_t sort_stats[6] = {0, 0, 0, 0, 0, 0}; uint64_t index_stats[4] = {0, 0, 0, 0}; uint64_t markdup_stats[6] = {0, 0, 0, 0, 0, 0}; };
Kept *kept_of(mcx_ctx *c)
{
    void **slot = mcx_ctx_files_slot(c, [](void *p) { delete (Kept *)p; });
    if (!*slot) *slot = new Kept();
    return (Kept *)*slot;
}
} // namespace

extern "C" int mcx_files_route(mcx_ctx *c, uint32_t route[2])
{
    if (!c || !route) return mcx_set_error(MCX_ERR_ARG, "mcx_files_route: null argument");
    const Kept *k = kept_of(c);
    route[0] = k->route[0]; route[1] = k->route[1];
    return 0;
}

extern "C" int mcx_files_sort_stats(mcx_ctx *c, uint64_t stats[6])
{
    if (!c || !stats) return mcx_set_error(MCX_ERR_ARG, "mcx_files_sort_stats: null argument");
    memcpy(stats, kept_of(c)->sort_stats, sizeof kept_of(c)->sort_stats);
    return 0;
}

extern "C" int mcx_files_index_stats(mcx_ctx *c, uint64_t stats[4])
{
    if (!c || !stats) return mcx_set_error(MCX_ERR_ARG, "mcx_files_index_stats: null argument");
    memcpy(stats, kept_of(c)->index_stats, sizeof kept_of(c)->index_stats);
    return 0;
}

extern "C" int mcx_files_markdup_stats(mcx_ctx *c, uint64_t stats[6])
{
    if (!c || !stats) return mcx_set_error(MCX_ERR_ARG, "mcx_files_markdup_stats: null argument");
    memcpy(stats, kept_of(c)->markdup_stats, sizeof kept_of(c)->markdup_stats);
    return 0;
}

extern "C" uint32_t mcx_pack_row(const uint8_t *seq, uint32_t rlen, uint32_t read, uint32_t *row, uint32_t row_words, uint64_t *odd, uint32_t odd_cap, uint32_t *n_odd)
{
    std::vector<uint64_t> o;
    pack_row(seq, rlen, read, row, row_words, o);
    for (uint64_t v : o) if (odd && n_odd && *n_odd < odd_cap) odd[(*n_odd)++] = v;
    return (uint32_t)o.size();
}

extern "C" uint32_t mcx_host_cpus(void) { return mcx_usable_cpus(); }

extern "C" int mcx_exchange_local(int32_t size, mcx_exchange *out)
{
    if (size < 1 || !out) return mcx_set_error(MCX_ERR_ARG, "mcx_exchange_local: bad argument");
    Rendezvous *rv = new Rendezvous();
    rv->size = size; rv->ptr.assign((size_t)size, nullptr);
    LocalPeer *peers = new LocalPeer[(size_t)size];
    for (int r = 0; r < size; r++) {
        peers[r].rv = rv; peers[r].rank = r;
        out[r].user = &peers[r]; out[r].rank = r; out[r].size = size; out[r].allgather = local_allgather;
    }
    return 0;
}

extern "C" void mcx_exchange_local_free(mcx_exchange *first)
{
    if (!first || !first->user) return;
    LocalPeer *peers = (LocalPeer *)first->user; // (rank 0's entry is the head of the array)
    delete peers[0].rv;
    delete[] peers;
    first->user = nullptr;
}

namespace {

// a plain FASTQ file: it is mapped and indexed; anything else goes through a sequential reader
bool plain_fastq(const char *path)
{
    const std::string p(path);
    if (p.size() > 3 && p.compare(p.size() - 3, 3, ".gz") == 0) return false;
    if (getenv("MCX_SERIAL_PARSER")) return false; // (tests: the sequential reader on plain files)
    struct stat st;
    if (stat(path, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size == 0) return false;
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const int ch = fgetc(f);
    fclose(f);
    return ch == '@'; // CheckReadFormat, GetData.cpp:22-31
}
// a plain FASTA file: not named .gz, a regular file that is not empty, its first byte anything but '@'
bool plain_fasta(const char *path)
{
    const std::string p(path);
    if (p.size() > 3 && p.compare(p.size() - 3, 3, ".gz") == 0) return false;
    if (getenv("MCX_SERIAL_PARSER")) return false; // (tests: the sequential reader)
    struct stat st;
    if (stat(path, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size == 0) return false;
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const int ch = fgetc(f);
    fclose(f);
    return ch != EOF && ch != '@';
}

// a BAM file: BGZF whose text begins "BAM\1", whatever its name — the first member that holds text is inflated here to see
bool bam_file(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    std::vector<uint8_t> head((size_t)1 << 17);
    head.resize(fread(head.data(), 1, head.size(), f));
    fclose(f);
    for (size_t o = 0; o < head.size();) {
        size_t xlen = 0;
        const size_t size = mcx_bgzf_member_at(head.data() + o, head.size() - o, xlen);
        if (!size) return false;
        const uint8_t *p = head.data() + o;
        const uint32_t isize = (uint32_t)p[size - 4] | ((uint32_t)p[size - 3] << 8) | ((uint32_t)p[size - 2] << 16) | ((uint32_t)p[size - 1] << 24);
        if (isize == 0) { o += size; continue; } // (an empty member in front)
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return false;
        uint8_t magic[4] = {0, 0, 0, 0};
        zs.next_in = const_cast<uint8_t *>(p + 12 + xlen); zs.avail_in = (uInt)(size - 12 - xlen - 8);
        zs.next_out = magic; zs.avail_out = sizeof magic;
        (void)inflate(&zs, Z_SYNC_FLUSH);
        const bool is = zs.avail_out == 0 && memcmp(magic, "BAM\1", 4) == 0;
        inflateEnd(&zs);
        return is;
    }
    return false;
}

// all n bytes at p: behind what was written before (stream), or at byte `at` of the file
bool write_all(int fd, const char *p, size_t n, uint64_t at, bool stream)
{
    for (size_t done = 0; done < n;) {
        const ssize_t w = stream ? write(fd, p + done, n - done) : pwrite(fd, p + done, n - done, (off_t)(at + done));
        if (w <= 0) return false;
        done += (size_t)w;
    }
    return true;
}

// seconds of a run: busy per stage and waiting, and wall seconds since `begin` (MCX_TIMING=1 prints them)
struct Timing {
    Tick begin = now();
    double w_open = 0, w_first_parsed = 0, w_reader = 0, w_mapped = 0, w_first_mapped = 0;
    double parse = 0, map = 0, format = 0, write = 0, p_lines = 0, p_pack = 0, p_wait = 0, p_push = 0, m_take = 0, m_collect = 0, f_push = 0, m_in = 0, m_dev = 0, m_out = 0, m_submit = 0, m_sam = 0;
    std::vector<double> each_dev; // mcx_map_batch_dev, batch by batch
    double wall() const { return secs(begin, now()); }
};

// where a run's reads come from, chosen once (open_input)
enum Route {
    kResident,   // BGZF (-gpu_inflate) or ordinary .gz (-gpu_gz) FASTQ or FASTA with -gpu_parse: inflated, cut and packed in HBM (mcx_resident.hip)
    kFastaDev,   // plain FASTA with -gpu_parse: the files' bytes go to HBM in chunks, a batch's records, bases, names, rows and odd bytes come back
    kMappedDev,  // plain FASTQ, mapped; -gpu_parse: a batch's text is parsed and packed on the device
    kMapped,     // plain FASTQ, mapped, parsed and packed by the pool
    kSequential  // .gz, FASTA: one Parser per file
};

struct Run {
    // ---- what the run was asked for ---------------------------------------------------------------------------------
    mcx_ctx *const c;
    const char *const fq1, *const fq2, *const sam_path;
    const mcx_file_opts opt;
    mcx_stats *const stats;
    const mcx_index *const idx;
    const HostIndex &hix;
    const int max_len;
    Kept *const kept;
    const int nf;               // input files
    const bool two;
    bool paired; // (a BAM file: its first taken record's flag decides, open_input)
    bool bam_in = false; // fq1 is a BAM file: the resident route under MCX_READS_BAM, or an error
    const uint64_t shard_count, shard_rank;
    const bool sharded;
    const uint64_t batch_reads;
    const uint32_t per_file;    // reads a batch takes from each file
    // (two pools of this size — parse + pack, format — beside the mapper's and the writer's threads: three quarters of the CPUs the process may use each;
    //  the pools take turns more than they overlap.  On the bench box's 16-CPU share: 6 / 8 / 12 / 16 / 24 / 64 threads a pool -> 10.6 / 10.9 / 13.2 / 12.2 / 10.9 / 10.2 M reads/s to SAM.
    //  The shards of a run share the host: each takes its part.)
    const int threads;
    const bool wants_sam;
    const bool dev_sam;         // the text is made on the device (mcx_sam.hip); without a SAM file there is none to make
    const bool bgzf;            // ... and compressed there: the file is BGZF (mcx_deflate.hip)
    const bool bam;             // ... of BAM records, not text (mcx_bam.hip)
    const bool sort;            // ... in coordinate order: sorted runs to a temporary file, merged behind the last batch (mcx_bam_sort.hip, mcx_sort_plan.h)
    const bool index;           // ... with its .bai beside it, made of what the merge's chunks say of their records (mcx_bai.hip, mcx_bai.h)
    const bool markdup;         // ... and flag bit 0x400 on its duplicates: units per part, one resolve behind the last batch, marks in the merge (mcx_markdup.hip)
    Timing t;
    Shards sh;
    Pool pool;                  // parse + pack
    Pool fpool;                 // format + write (threads of its own: the two stages overlap)

    // ---- the input ------------------------------------------------------------------------------------------------------
    Route route = kSequential;
    uint32_t route_bits[2] = {0, 0}; // what mcx_files_route will say of each file
    MappedFastq mf[2];
    Parser ps[2];
    struct FqFree { void operator()(mcx_fastq_parser *q) const { mcx_fastq_parser_free(q); } };
    std::unique_ptr<mcx_fastq_parser, FqFree> fq_parser; // -gpu_parse on plain FASTQ
    struct PinnedRecs { mcx_fastq_rec *p[2] = {nullptr, nullptr}; mcx_fastq_rec *&operator[](int f) { return p[f]; } ~PinnedRecs() { mcx_pinned_free(p[0]); mcx_pinned_free(p[1]); } } fq_recs; // a batch's records as the device hands them out
    struct ResFree { void operator()(mcx_resident *r) const { mcx_resident_close(r); } };
    std::unique_ptr<mcx_resident, ResFree> resident; // -gpu_inflate -gpu_parse on BGZF FASTQ: the reads stay in HBM (mcx_resident.hip)
    bool fastq = true;
    uint64_t total_recs[2] = {0, 0}; // (mapped) records of each file
    mcx_fastq_info fq_info;          // (the reader's) what the device parser said of the batch in hand; zero on the other routes

    // ---- the output: one file, every batch's text at its final place -----------------------------------------------------
    int sam_fd = -1;
    bool sam_stream = false; // stdout: written front to back
    uint64_t sam_base = 0;   // where the first batch's text goes
    std::atomic<int> write_rc{0};
    struct DefFree { void operator()(mcx_deflater *d) const { mcx_deflater_free(d); } };
    std::unique_ptr<mcx_deflater, DefFree> deflater; // -bgzf: the header's blocks (the opening thread), then every part's (the mapper's thread)
    mcx_sam_bgzf zs = {nullptr, 65280, 0, 0, 0};
    // -sort: while the batches are mapped sam_fd is the temporary file of the runs; the file asked for waits in out_fd for the merge
    int out_fd = -1;
    bool out_stream = false;
    std::string tmp_path;
    mcx_sort_sink sink;                // the keys and lengths of the part just made (the mapper's thread)
    std::vector<sortplan::Run> runs;   // ... kept per run, with its blocks
    uint64_t tmp_at = 0;               // where the batch in the mapper's hands will lie in the temporary file
    double sort_secs[5] = {0, 0, 0, 0, 0}; // the merge: read, copy in, inflate, sort, deflate + copy out
    double merge_seconds = 0;
    // -index: the stretches and windows of the merge's chunks, and — once the EOF block is written — the bytes of <sam_path>.bai, which close_output writes
    mcx_bai_sink bai;
    std::vector<uint8_t> bai_bytes;
    // -markdup: the run's units (the mapper's thread), and per run of the merge the group every sorted record came from — 4 bytes a record — with the number of
    // the part's first unit; behind the resolve one byte a record instead: does it get the flag bit
    mcx_dup_sink dsink;
    struct DupRun { std::vector<uint32_t> grp; uint64_t base = 0; int paired = 0; std::vector<uint8_t> bits; };
    std::vector<DupRun> dup_runs;
    double dup_host_seconds = 0;
    uint64_t indexed_records = 0;
    ~Run() { drop_tmp(); }
    uint8_t bgzf_eof[28];
    std::deque<BatchPtr> waiting; // (the writer's; sharded) formatted, their place in the file not known yet

    // ---- between the stages -----------------------------------------------------------------------------------------------
    // batch objects circulate: their buffers (page-locked: slow to get) are allocated once and stay with the context from call to call
    // (one shard holds at most eleven at a time: two per queue between the stages, three on the device, one each in the reader's, the
    //  formatter's and the writer's hands; shards wait two rounds for the places of their text: sixteen.  At -batch 2 M reads an object
    //  pins ~0.5 GB of host memory — 6 GB a shard —, which is the host-memory bill of a run: see INTEGRATION.md)
    const int n_objects;
    Queue<BatchPtr> parsed, mapped, formatted, spare;
    std::atomic<bool> abort{false};
    Places places;

    // ---- the mapper's state ---------------------------------------------------------------------------------------------------
    int rc = 0;
    int64_t local_avg[4];
    int64_t *avg = nullptr;
    const bool profile, multi;
    int in_flight = 0;             // parts submitted and not collected yet
    std::deque<BatchPtr> leaving;  // mapped, their last part on its way out (oldest first), with the number of parts each still waits for
    std::deque<int> leaving_parts;
    bool input_done = false, dead = false, ended = false; // dead: a shard failed and every shard knows; ended: the input ended in an earlier batch
    uint64_t rounds_done = 0;
    uint64_t place_next = 0;
    std::deque<std::pair<uint64_t, bool>> rounds_unplaced; // (sharded) rounds mapped whose text sizes have not been exchanged; did this shard hold a batch of the round?
    BatchPtr cur, nxt;             // the batch being mapped and the one behind it (already on its way in)
    bool cur_in = false, nxt_in = false;
    // the part of `cur` that is on the device, and how many of its parts are on their way out
    const uint8_t *d_bases = nullptr; const uint32_t *d_off = nullptr; mcx_aln *d_aln = nullptr; uint32_t *d_cig = nullptr; uint32_t n_dev = 0;
    int parts_out = 0;
    bool host_md = false; // -md without device_sam: every mapped part's MD strings come to the host for the formatter's threads (part_md)
    // -rg / -mc: the validated @RG line (real TABs, no newline; empty: none) for the header of every route, its ID, and — for the host formatter — the mate-tag switch
    std::string rg_line, rg_id;
    bool host_mate_tags = false;
    const char *rg_or_null() const { return rg_line.empty() ? nullptr : rg_line.c_str(); }

    Run(mcx_ctx *ctx, const char *f1, const char *f2, const mcx_file_opts &o, const char *sam, mcx_stats *st)
        : c(ctx), fq1(f1), fq2(f2), sam_path(sam), opt(o), stats(st), idx(mcx_ctx_index(ctx)), hix(idx->host), max_len(mcx_ctx_max_read_len(ctx)), kept(kept_of(ctx)),
          nf(f2 && f2[0] ? 2 : 1), two(nf == 2), paired(two || o.interleaved_pairs),
          shard_count(o.shard_count > 1 ? (uint64_t)o.shard_count : 1), shard_rank(shard_count > 1 ? (uint64_t)o.shard_rank : 0), sharded(shard_count > 1),
          batch_reads(std::max<uint64_t>(kReadChunkSize, mcx_ctx_max_reads(ctx) / kReadChunkSize * kReadChunkSize)), per_file((uint32_t)(two ? batch_reads / 2 : batch_reads)),
          threads(o.host_threads > 0 ? o.host_threads : (int)std::min<unsigned>(64, std::max<unsigned>(1, mcx_usable_cpus() * 3 / 4 / (unsigned)shard_count))),
          wants_sam(sam && sam[0]), dev_sam(o.device_sam != 0 && wants_sam), bgzf((o.device_sam & MCX_SAM_BGZF) != 0 && wants_sam), bam((o.device_sam & MCX_SAM_BAM) != 0 && bgzf), sort((o.device_sam & MCX_SAM_SORT) != 0 && bam), index((o.device_sam & MCX_SAM_INDEX) != 0 && sort), markdup((o.device_sam & MCX_SAM_MARKDUP) != 0 && sort), pool(threads), fpool(threads),
          n_objects(sharded ? 16 : 12), parsed(2), mapped(2), formatted(2), spare((size_t)n_objects),
          profile(mcx_ctx_has_profile(ctx)), multi(mcx_ctx_multi(ctx))
    {
        kept->route[0] = kept->route[1] = 0;
        sh.x = opt.exchange; sh.slot_stride = (uint32_t)batch_reads; sh.cap_chunks = (uint32_t)(batch_reads / kReadChunkSize + 2);
        memset(&fq_info, 0, sizeof fq_info);
    }
    bool mapped_input() const { return route == kMappedDev || route == kMapped; }

    // ---- the input: the resident route, mapped and indexed (plain FASTQ), or a sequential reader per file --------------------------
    // (from here on a sharded run's shards leave together: whatever fails on one is told to the others)
    int open_input()
    {
        const bool plain = plain_fastq(fq1) && (!two || plain_fastq(fq2));
        if (!plain && (opt.device_inflate & (MCX_INFLATE_BGZF | MCX_INFLATE_GZ)) && opt.device_parse && !sharded && !opt.interleaved_pairs && (!wants_sam || opt.device_sam)) {
            const char *paths[2] = {fq1, two ? fq2 : nullptr};
            mcx_resident *r = nullptr;
            if (int e = mcx_resident_open(idx->device, paths, nf, (uint32_t)opt.device_inflate, bam_in, &r)) return e;
            resident.reset(r); // (null: a file is of a kind device_inflate has no bit for, the search cannot cut it, or the files differ in format — the route does not apply and the files are read as without it)
        }
        if (bam_in) { // (mcx_map_files_rg has set the switches the route needs: there is no other reader of BAM)
            if (!resident) return mcx_set_error(MCX_ERR_IO, std::string(fq1) + ": cannot be read as a BAM file");
            paired = mcx_resident_bam_paired(resident.get());
        }
        if (!plain && !resident && opt.device_parse && !sharded && !opt.interleaved_pairs && plain_fasta(fq1) && (!two || plain_fasta(fq2))) {
            const char *paths[2] = {fq1, two ? fq2 : nullptr};
            mcx_resident *r = nullptr;
            if (int e = mcx_resident_open_plain(idx->device, paths, nf, &r)) return e;
            resident.reset(r);
            if (resident) route = kFastaDev;
        }
        if (resident) fastq = !mcx_resident_fasta(resident.get());
        if (route != kFastaDev) route = resident ? kResident : !plain ? kSequential : opt.device_parse ? kMappedDev : kMapped;
        if (mapped_input()) { if (int e = open_mapped()) return e; }
        else if (route == kSequential) { if (int e = open_sequential()) return e; } // (the resident route has opened its files itself)
        const uint32_t sam_bit = (dev_sam ? (uint32_t)MCX_ROUTE_SAM : 0u) | (bgzf ? (uint32_t)MCX_ROUTE_BGZF : 0u) | (bam ? (uint32_t)MCX_ROUTE_BAM : 0u) | (sort ? (uint32_t)MCX_ROUTE_SORT : 0u) | (index ? (uint32_t)MCX_ROUTE_INDEX : 0u) | (markdup ? (uint32_t)MCX_ROUTE_MARKDUP : 0u);
        for (int f = 0; f < nf; f++)
            route_bits[f] = sam_bit | (bam_in ? (uint32_t)MCX_ROUTE_BAM_IN : 0u) | (route == kResident ? mcx_resident_inflate_bit(resident.get(), f) | (uint32_t)(MCX_ROUTE_PARSE | MCX_ROUTE_ROWS)
                                                          : (ps[f].device_inflated() ? (uint32_t)MCX_ROUTE_INFLATE : 0u) | (route == kMappedDev || route == kFastaDev ? (uint32_t)MCX_ROUTE_PARSE : 0u));
        return 0;
    }
    int open_mapped()
    {
        int e = 0;
        std::string err;
        for (int f = 0; f < nf && e == 0; f++) if (!mf[f].open(f ? fq2 : fq1, err)) e = mcx_set_error(MCX_ERR_IO, err);
        if (sharded && (e = sh.agree(e))) return e;
        if (e) return e;
        for (int f = 0; f < nf; f++) {
            // the line counts: every shard counts a share of the blocks, then they tell one another
            const size_t nb = mf[f].n_blocks();
            const size_t b0 = nb * shard_rank / shard_count, b1 = nb * (shard_rank + 1) / shard_count;
            mf[f].count(b0, b1, pool);
            if (sharded) {
                const size_t most = (nb + shard_count - 1) / shard_count + 1;
                std::vector<uint32_t> mine(most, 0);
                memcpy(mine.data(), mf[f].counts() + b0, (b1 - b0) * sizeof(uint32_t));
                if (int e2 = sh.gather(mine.data(), most * sizeof(uint32_t))) return e2;
                for (uint64_t r = 0; r < shard_count; r++) {
                    const size_t r0 = nb * r / shard_count, r1 = nb * (r + 1) / shard_count;
                    memcpy(mf[f].counts() + r0, sh.recv.data() + (size_t)r * most * sizeof(uint32_t), (r1 - r0) * sizeof(uint32_t));
                }
            }
            mf[f].finish();
            total_recs[f] = (mf[f].lines() + 2) / 4; // a record needs its header and sequence lines
        }
        // -gpu_parse: this shard's batches are parsed and packed by an mcx_fastq_parser of its own on the context's device (its HBM is taken after the context's)
        if (route == kMappedDev) {
            mcx_fastq_parser *q = nullptr;
            const uint64_t per = per_file;
            if (mcx_fastq_parser_create(idx->device, (uint64_t)std::min<uint64_t>(mf[0].bytes(), per * 200 + 65536), (uint32_t)std::min<uint64_t>(per, 0xFFFFFFFFu), &q) != 0)
                e = mcx_set_error(MCX_ERR_DEVICE, std::string("-gpu_parse: ") + mcx_last_error());
            fq_parser.reset(q);
            for (int f = 0; f < nf && e == 0; f++)
                if (!(fq_recs[f] = (mcx_fastq_rec *)mcx_pinned_alloc((size_t)std::max<uint64_t>(per, 1) * sizeof(mcx_fastq_rec)))) e = mcx_set_error(MCX_ERR_DEVICE, "-gpu_parse: cannot allocate pinned host memory");
            if (sharded && (e = sh.agree(e))) return e;
            if (e) return e;
        }
        return 0;
    }
    int open_sequential()
    {
        int e = 0;
        std::string err;
        const int inflate_device = (opt.device_inflate & MCX_INFLATE_BGZF) ? idx->device : -1; // -gpu_inflate: BGZF files are inflated on the context's device
        if (!ps[0].open(fq1, err, inflate_device)) e = mcx_set_error(MCX_ERR_IO, err);
        if (e == 0 && two && !ps[1].open(fq2, err, inflate_device)) e = mcx_set_error(MCX_ERR_IO, err);
        if (e == 0 && two && ps[0].fastq() != ps[1].fastq()) e = mcx_set_error(MCX_ERR_IO, std::string(fq1) + " and " + fq2 + " are with different format");
        if (sharded && (e = sh.agree(e))) return e;
        if (e) return e;
        fastq = ps[0].fastq();
        return 0;
    }

    // ---- the output ------------------------------------------------------------------------------------------------------------
    int open_output()
    {
        if (!wants_sam) return 0;
        int e = 0;
        if (bgzf) { // -bgzf: a deflater of the run's own on the context's device
            mcx_deflater *d = nullptr;
            if (mcx_deflater_create(idx->device, 1u << 20, &d) != 0) return mcx_set_error(MCX_ERR_DEVICE, std::string("-bgzf: ") + mcx_last_error());
            deflater.reset(d);
            zs.deflater = d; zs.block = 65280; zs.bam = bam ? 1 : 0;
            if (const char *env = getenv("MCX_BGZF_BLOCK")) { // (debug override: the bytes of text per block)
                const long v = atol(env);
                if (v >= 1 && v <= 65280) zs.block = (uint32_t)v;
            }
            if (int e2 = mcx_deflater_set_block(d, zs.block)) return e2;
            mcx_bgzf_eof(bgzf_eof);
        }
        if (strcmp(sam_path, "-") == 0) {
            if (sharded) e = mcx_set_error(MCX_ERR_ARG, "a sharded run cannot write its SAM to stdout");
            sam_fd = 1; sam_stream = true;
        } else {
            // shard 0 creates (or empties) the file; the others open it once that has happened
            if (shard_rank == 0) {
                sam_fd = ::open(sam_path, O_RDWR | O_CREAT | (opt.append_sam ? 0 : O_TRUNC), 0644);
                if (sam_fd < 0) e = mcx_set_error(MCX_ERR_IO, std::string("cannot write ") + sam_path);
            }
            if (sharded && (e = sh.agree(e))) { if (sam_fd >= 0) close(sam_fd); return e; }
            if (shard_rank != 0) {
                sam_fd = ::open(sam_path, O_RDWR, 0644);
                if (sam_fd < 0) e = mcx_set_error(MCX_ERR_IO, std::string("cannot write ") + sam_path);
            }
            struct stat st;
            if (e == 0 && opt.append_sam && fstat(sam_fd, &st) == 0) sam_base = (uint64_t)st.st_size;
            // (-bgzf) a further library starts over the EOF block of the one before: a finished file has one, at its end
            uint8_t tail[28];
            if (e == 0 && bgzf && opt.append_sam && sam_base >= 28 && pread(sam_fd, tail, 28, (off_t)(sam_base - 28)) == 28 && memcmp(tail, bgzf_eof, 28) == 0) sam_base -= 28;
        }
        if (e == 0 && sort) { // the runs go to a temporary file, without a header; the file asked for is written by the merge
            out_fd = sam_fd; out_stream = sam_stream;
            if (out_stream) { const char *dir = getenv("TMPDIR"); tmp_path = std::string(dir && dir[0] ? dir : "/tmp") + "/mcx_sort." + std::to_string((long long)getpid()) + ".tmp"; }
            else tmp_path = std::string(sam_path) + ".sort.tmp";
            sam_fd = ::open(tmp_path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0600);
            sam_stream = false; sam_base = 0;
            zs.sort = &sink;
            if (markdup) sink.dup = &dsink;
            if (sam_fd < 0) {
                e = mcx_set_error(MCX_ERR_IO, "-sort: cannot write the temporary file " + tmp_path);
                tmp_path.clear();
                sam_fd = out_fd; sam_stream = out_stream; out_fd = -1;
            }
        }
        if (e == 0 && !opt.append_sam && !sort) {
            std::string hdr;
            if (bam) { // -bam: the binary header, text and contigs
                uint64_t n = 0;
                (void)mcx_bam_header_rg(idx, rg_or_null(), 0, nullptr, 0, &n);
                hdr.resize((size_t)n);
                if (n == 0 || mcx_bam_header_rg(idx, rg_or_null(), 0, (uint8_t *)&hdr[0], n, &n) != 0) e = mcx_set_error(MCX_ERR_UNSUPPORTED, std::string("-bam: ") + mcx_last_error());
            } else {
                sam_header(hix, hdr);
                if (!rg_line.empty()) hdr += rg_line + "\n"; // (-rg: the last line of the header text)
            }
            if (bgzf && e == 0) { // the header as BGZF blocks of its own
                std::string blocks((size_t)mcx_bgzf_bound(hdr.size(), zs.block), '\0');
                uint64_t made = 0;
                const auto t0 = now();
                e = mcx_bgzf_deflate(zs.deflater, (const uint8_t *)hdr.data(), hdr.size(), (uint8_t *)&blocks[0], blocks.size(), &made);
                zs.text_bytes += hdr.size(); zs.out_bytes += made; zs.seconds += secs(t0, now());
                blocks.resize((size_t)made);
                hdr.swap(blocks);
            }
            if (e == 0 && shard_rank == 0) {
                const ssize_t w = sam_stream ? write(sam_fd, hdr.data(), hdr.size()) : pwrite(sam_fd, hdr.data(), hdr.size(), 0);
                if (w != (ssize_t)hdr.size()) e = mcx_set_error(MCX_ERR_IO, std::string("cannot write ") + sam_path);
            }
            sam_base = hdr.size();
        }
        if (sharded) e = sh.agree(e);
        if (e) { if (sam_fd >= 0 && !sam_stream) close(sam_fd); return e; }
        return 0;
    }
    // both ends are open: the route is the context's to report, the batch objects come out of its keeping
    void begin()
    {
        for (int f = 0; f < nf; f++) kept->route[f] = route_bits[f];
        mcx_avg_init(local_avg);
        avg = opt.avg_state ? opt.avg_state : local_avg;
        place_next = sam_base;
        t.w_open = t.wall();
        for (int k = 0; k < n_objects; k++) {
            if (!kept->objects.empty()) { spare.push(std::move(kept->objects.back())); kept->objects.pop_back(); }
            else spare.push(BatchPtr(new Batch));
        }
    }
    // (the batch objects go back to the context with their buffers; the device buffers of the resident route only for a run that took it — HBM that a context
    //  which has gone back to another route would hold for nothing)
    void keep_objects()
    {
        auto keep = [&](BatchPtr &b) { if (route != kResident && b->res) { mcx_resident_bufs_free(b->res); b->res = nullptr; } kept->objects.push_back(std::move(b)); };
        BatchPtr b;
        while (spare.try_pop(b)) keep(b);
        while (parsed.try_pop(b)) keep(b);
        while (mapped.try_pop(b)) keep(b);
    }
    int close_output()
    {
        if (sam_fd >= 0 && !sam_stream) { if (close(sam_fd) != 0 && write_rc.load() == 0) write_rc.store(MCX_ERR_IO); }
        if (rc == 0 && write_rc.load()) rc = mcx_set_error(MCX_ERR_IO, std::string("cannot write ") + (sam_path ? sam_path : ""));
        if (index) write_index();
        return rc;
    }
    // -index: the BAM file is complete and closed — its index goes beside it, whole (written under another name and renamed) or not at all; after a run that
    // failed, an index an earlier run left there would describe another file: it goes
    void write_index()
    {
        const std::string path = std::string(sam_path) + ".bai", part = path + ".tmp";
        memset(kept->index_stats, 0, sizeof kept->index_stats);
        if (rc == 0) {
            const int fd = ::open(part.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            bool ok = fd >= 0 && write_all(fd, (const char *)bai_bytes.data(), bai_bytes.size(), 0, false);
            if (fd >= 0 && close(fd) != 0) ok = false;
            if (ok && rename(part.c_str(), path.c_str()) != 0) ok = false;
            if (!ok) { unlink(part.c_str()); rc = mcx_set_error(MCX_ERR_IO, "-index: cannot write " + path); }
        }
        if (rc) { unlink(path.c_str()); return; }
        kept->index_stats[0] = bai.stats.stretches; kept->index_stats[1] = bai.stats.bins; kept->index_stats[2] = bai.stats.intervals; kept->index_stats[3] = bai.stats.bytes;
    }

    // ---- stage 1: parse + pack ---------------------------------------------------------------------------------------
    void read_loop()
    {
        bool done = false;
        uint64_t number = 0;
        while (!done) {
            const bool mine = number % shard_count == shard_rank;
            if (mapped_input() && !mine && (number + 1) * (uint64_t)per_file < total_recs[0]) { number++; continue; } // another shard's batch: not a byte of it is touched
            const Tick tw = now();
            BatchPtr b = spare.pop();
            const Tick t0 = now();
            t.p_wait += secs(tw, t0);
            b->reset(two, fastq, number);
            memset(&fq_info, 0, sizeof fq_info);
            switch (route) {
            case kResident: fill_resident(*b); break;
            case kFastaDev: fill_fasta_dev(*b); break;
            case kMappedDev: fill_mapped_dev(*b, number, mine); break;
            case kMapped: fill_mapped(*b, number, mine); break;
            case kSequential: fill_sequential(*b); break;
            }
            t.p_lines += secs(t0, now());
            done = settle(*b, mine);
            // batches are dealt to the shards in turn; another shard's batch is dropped — unless it carries the end of the input
            // or an error, which every shard must see (the sequential reader has to walk the stream to get past it)
            number++;
            if (!mine && !done) { spare.push(std::move(b)); continue; }
            if (!mine && b->error.empty()) b->n = 0;
            const Tick tp = now();
            if (b->n && b->error.empty()) {
                pack(*b);
                if (dev_sam && b->error.empty() && !b->resident) stage_sam_names(*b); // (the resident route: names and qualities are in HBM already)
            }
            if (!b->error.empty()) done = true;
            b->last = done;
            t.p_pack += secs(tp, now());
            t.parse += secs(t0, now());
            if (t.w_first_parsed == 0) t.w_first_parsed = t.wall();
            const Tick tq = now();
            parsed.push(std::move(b));
            t.p_push += secs(tq, now());
        }
        t.w_reader = t.wall();
    }
    // what every route's batch goes through: the mates' counts, the files' errors; true: this batch is the last
    bool settle(Batch &b, bool mine)
    {
        if (two) {
            // the reference stops at the first empty read of file 1 and takes whatever file 2 holds (GetData.cpp:91-93)
            if (mine || !mapped_input()) {
                if (b.in[1].n() < b.in[0].n()) b.error = std::string(fq2) + " holds fewer reads than " + fq1;
                if (b.in[1].n() > b.in[0].n()) b.in[1].recs.resize(b.in[0].n());
                b.n = 2 * b.in[0].n();
            }
        } else b.n = b.in[0].n();
        bool done = b.in[0].last;
        for (int f = 0; f < 2; f++) if (!b.in[f].error.empty()) b.error = b.in[f].error;
        if (!b.error.empty() || abort.load()) done = true;
        return done;
    }
    // the resident route: the batch is counted, cut and packed in HBM; the views hold the files' counts and ends, as Parser::take leaves them
    void fill_resident(Batch &b)
    {
        b.resident = true;
        if ((b.error_rc = mcx_resident_next(resident.get(), &b.res, per_file, max_len, dev_sam, &b.rb)) != 0) { b.in[0].error = mcx_last_error(); return; }
        for (int f = 0; f < nf; f++) {
            View &v = b.in[f];
            if (!v.recs.resize(b.rb.n_records[f])) { v.error = "out of memory for the batch's read records"; continue; } // (counted, never read)
            v.last = b.rb.last[f];
            if (b.rb.has_too_long[f]) v.error = "read " + std::string(b.rb.too_long[f]) + " is longer than max_read_len";
        }
    }
    // plain FASTA with -gpu_parse: the batch is counted and cut in HBM as on the resident route; its bases and names come back into the first view's own buffer
    // (bases, then names) with the offsets as records, which is how Parser::take leaves a batch: the host formatter, device_sam and -m find them there
    void fill_fasta_dev(Batch &b)
    {
        if ((b.error_rc = mcx_resident_next(resident.get(), &b.res, per_file, max_len, false, &b.rb)) != 0) { b.in[0].error = std::string("-gpu_parse: ") + mcx_last_error(); return; }
        const uint32_t n = b.rb.n_reads;
        std::vector<uint32_t> off((size_t)n + 1), noff((size_t)n + 1);
        std::vector<char> &own = b.in[0].own;
        own.resize((size_t)(b.rb.n_bases + b.rb.n_name_bytes) + 32);
        if (n) {
            mcx_fastq_out o;
            memset(&o, 0, sizeof o);
            o.bases = (uint8_t *)own.data(); o.off = off.data(); o.bases_cap = b.rb.n_bases + 32;
            o.names = (uint8_t *)own.data() + b.rb.n_bases; o.name_off = noff.data(); o.names_cap = b.rb.n_name_bytes; // (behind the bases: copied after them)
            if ((b.error_rc = mcx_resident_host_out(resident.get(), &o)) != 0) { b.in[0].error = std::string("-gpu_parse: ") + mcx_last_error(); return; }
        }
        for (int f = 0; f < nf; f++) {
            View &v = b.in[f];
            v.base = own.data();
            if (!v.recs.resize(b.rb.n_records[f])) { v.error = "out of memory for the batch's read records"; continue; }
            v.last = b.rb.last[f];
            if (b.rb.has_too_long[f]) v.error = "read " + std::string(b.rb.too_long[f]) + " is longer than max_read_len";
            Rec *dst = v.recs.data();
            for (uint32_t r = (uint32_t)f; r < n; r += (uint32_t)nf) { // (records behind the batch's reads — a file ahead of the other, a batch that is not mapped — are counted, never read)
                Rec rec; memset(&rec, 0, sizeof rec);
                rec.name = (size_t)b.rb.n_bases + noff[r]; rec.name_len = noff[r + 1] - noff[r]; rec.seq = off[r]; rec.rlen = off[r + 1] - off[r];
                dst[r / (uint32_t)nf] = rec;
            }
        }
    }
    void fill_sequential(Batch &b)
    {
        if (two) {
            std::thread t2([&] { ps[1].take(b.in[1], per_file, max_len); });
            ps[0].take(b.in[0], per_file, max_len);
            t2.join();
        } else ps[0].take(b.in[0], per_file, max_len);
    }
    // (mapped) the records of batch `number`: [r0, r1[f]) of file f, cnt[f] of them
    struct Span { uint64_t r0, r1[2], cnt[2]; };
    Span span_of(uint64_t number) const
    {
        Span s = {number * per_file, {0, 0}, {0, 0}};
        for (int f = 0; f < nf; f++) {
            s.r1[f] = std::min<uint64_t>(s.r0 + per_file, total_recs[f]);
            s.cnt[f] = s.r1[f] > s.r0 ? s.r1[f] - s.r0 : 0;
        }
        return s;
    }
    // file f ends with this batch: its records stopped early, or there are no more behind them
    bool ends_with(const Span &s, int f, bool stopped) const { return stopped || s.cnt[f] < per_file || s.r1[f] >= total_recs[f]; }
    // the records of both files in one pass of the pool, every share written where it belongs
    void fill_mapped(Batch &b, uint64_t number, bool mine)
    {
        for (int f = 0; f < nf; f++) b.in[f].base = mf[f].data();
        if (!mine) { for (int f = 0; f < nf; f++) b.in[f].last = true; return; } // (the input ends inside another shard's batch: an empty batch carries the news)
        const Span s = span_of(number);
        int parts[2] = {0, 0};
        for (int f = 0; f < nf; f++) {
            View &v = b.in[f];
            parts[f] = pool.slices(s.cnt[f], 2048);
            v.recs.resize((size_t)s.cnt[f]);
            if (v.recs.size() != s.cnt[f]) { v.error = "out of memory"; parts[f] = 0; }
        }
        const int all = parts[0] + parts[1];
        std::vector<size_t> got((size_t)std::max(all, 1), 0);
        std::vector<std::string> perr((size_t)std::max(all, 1));
        std::vector<uint8_t> ok((size_t)std::max(all, 1), 1);
        if (all) pool.run(all, [&](int k2) {
            const int f = k2 < parts[0] ? 0 : 1, k = f ? k2 - parts[0] : k2;
            const uint64_t a = s.cnt[f] * (uint64_t)k / (uint64_t)parts[f], z = s.cnt[f] * (uint64_t)(k + 1) / (uint64_t)parts[f];
            ok[(size_t)k2] = mf[f].parse(s.r0 + a, s.r0 + z, max_len, b.in[f].recs.data() + a, got[(size_t)k2], perr[(size_t)k2]) ? 1 : 0;
        });
        for (int f = 0; f < nf; f++) {
            if (!parts[f]) continue;
            View &v = b.in[f];
            bool stopped = false;
            for (int k = 0; k < parts[f] && !stopped; k++) {
                const size_t k2 = (size_t)(f ? parts[0] + k : k);
                if (!ok[k2]) { // the records end inside this share: those before the stop count, nothing behind them
                    stopped = true;
                    if (!perr[k2].empty()) v.error = perr[k2];
                    v.recs.resize((size_t)(s.cnt[f] * (uint64_t)k / (uint64_t)parts[f]) + got[k2]);
                }
            }
            v.last = ends_with(s, f, stopped);
        }
    }
    // The byte ranges of records [r0, r1) of each file — from the line index, as above — go to the parser's page-locked staging through the pool and are
    // parsed as whole texts (final): the same records, the same stops as MappedFastq::parse gives.
    void fill_mapped_dev(Batch &b, uint64_t number, bool mine)
    {
        if (!mine) return fill_mapped(b, number, false);
        const Span s = span_of(number);
        uint64_t bytes[2] = {0, 0};
        size_t p0[2] = {0, 0};
        for (int f = 0; f < nf; f++) {
            b.in[f].base = mf[f].data();
            if (s.cnt[f]) { p0[f] = mf[f].line_start(4 * s.r0); bytes[f] = mf[f].line_start(4 * s.r1[f]) - p0[f]; }
        }
        std::string perr;
        uint8_t *h[2] = {nullptr, nullptr};
        if (bytes[0] + bytes[1]) {
            if (mcx_fastq_stage(fq_parser.get(), bytes, h) != 0) perr = std::string("-gpu_parse: ") + mcx_last_error();
            else {
                const uint64_t piece = 1u << 20, n0 = (bytes[0] + piece - 1) / piece, n1 = (bytes[1] + piece - 1) / piece;
                pool.run((int)(n0 + n1), [&](int k) {
                    const int f = (uint64_t)k < n0 ? 0 : 1;
                    const uint64_t at = ((uint64_t)k - (f ? n0 : 0)) * piece;
                    memcpy(h[f] + at, mf[f].data() + p0[f] + at, (size_t)std::min<uint64_t>(piece, bytes[f] - at));
                });
                mcx_fastq_out recs_only;
                memset(&recs_only, 0, sizeof recs_only);
                recs_only.recs[0] = fq_recs[0]; recs_only.recs[1] = two ? fq_recs[1] : nullptr;
                if (mcx_fastq_staged_sizes(fq_parser.get(), bytes, two ? 1 : 0, (uint32_t)std::max(s.cnt[0], s.cnt[1]), max_len, 1, &fq_info) != 0 ||
                    mcx_fastq_staged_out(fq_parser.get(), &recs_only, &fq_info) != 0) perr = std::string("-gpu_parse: ") + mcx_last_error();
            }
        }
        for (int f = 0; f < nf; f++) {
            View &v = b.in[f];
            if (!perr.empty()) { v.error = perr; continue; }
            const uint64_t got = std::min<uint64_t>(fq_info.n_records[f], s.cnt[f]);
            const bool stopped = got < s.cnt[f];
            if (!v.recs.resize((size_t)got)) { v.error = "out of memory"; continue; }
            const mcx_fastq_rec *src = fq_recs[f];
            Rec *dst = v.recs.data();
            const uint64_t at = p0[f];
            pool.for_range(got, 4096, [&](int, uint64_t lo, uint64_t hi) { // the offsets rebased to the mapped file: the formatter and -gpu_sam's gather read names and qualities where they lie
                for (uint64_t i = lo; i < hi; i++) {
                    const mcx_fastq_rec &e = src[i];
                    Rec rec; memset(&rec, 0, sizeof rec);
                    rec.name = at + e.name; rec.name_len = e.name_len; rec.seq = at + e.seq; rec.rlen = e.rlen;
                    rec.qual = e.qual ? at + e.qual : 0; rec.q_take = e.q_take; // (no quality line: offset 0, nothing taken, as the host reader has it)
                    dst[i] = rec;
                }
            });
            if (stopped && fq_info.stop[f] == MCX_FASTQ_TOO_LONG) { // the name of the read that is too long, by the host's header rule at the first byte that was not taken
                const char *l = mf[f].data() + at + fq_info.consumed[f];
                const char *e = find_nl(l, mf[f].data() + mf[f].bytes());
                const size_t len = e ? (size_t)(e - l) + 1 : (size_t)(mf[f].data() + mf[f].bytes() - l);
                int q1, q2;
                header_of(l, (int)len, q1, q2);
                v.error = "read " + std::string(l + q1, q2 > q1 ? (size_t)(q2 - q1) : 0) + " is longer than max_read_len";
            }
            v.last = ends_with(s, f, stopped);
        }
    }

    // 2-bit rows of this shard's reads, the bytes that are not ACGT beside them
    void pack(Batch &b)
    {
        const uint32_t n = b.n;
        uint32_t npr = paired ? n : 0; // reads mapped as pairs; the odd tail of an interleaved file is mapped read by read
        if (paired && (n & 1)) npr = n / kReadChunkSize * kReadChunkSize;
        b.n_pair_reads = npr;
        uint32_t longest = b.resident || route == kFastaDev ? b.rb.longest : fq_info.longest;
        if (route == kMapped || route == kSequential) {
            std::vector<uint32_t> most((size_t)pool.slices(n, 4096), 0);
            pool.for_range(n, 4096, [&](int k, uint64_t lo, uint64_t hi) {
                uint32_t m = 0;
                for (uint32_t r = (uint32_t)lo; r < (uint32_t)hi; r++) { const char *base; m = std::max(m, b.rec(r, base).rlen); }
                most[(size_t)k] = m;
            });
            for (uint32_t m : most) longest = std::max(longest, m);
        }
        b.row_words = (longest + 15) / 16;
        if (!b.reserve(std::max<size_t>(n, batch_reads), b.resident ? 1 : std::max<size_t>(b.row_words, ((size_t)max_len + 15) / 16))) b.error = "cannot allocate pinned host memory";
        else switch (route) {
        case kResident: pack_resident(b); break;
        case kFastaDev: pack_fasta_dev(b); break;
        case kMappedDev: pack_mapped_dev(b); break;
        case kMapped: case kSequential: pack_host(b); break;
        }
        b.is_mate2.assign(n, 0);
        for (uint32_t r = 1; r < npr; r += 2) b.is_mate2[r] = 1;
    }
    // rows, lengths and odd bytes are in the batch's device buffers; the odd list is split at the pair / single part boundary as below — here one
    // of the two parts is the whole batch (two files: pairs; one: single reads, numbered from 0 as they are)
    void pack_resident(Batch &b)
    {
        if (b.rb.n_reads != b.n) b.error = "-gpu_parse: the device packed " + std::to_string(b.rb.n_reads) + " reads, the reader counted " + std::to_string(b.n);
        b.row_words = b.rb.row_words;
        b.n_odd[0] = b.n_pair_reads ? b.rb.n_odd : 0; b.n_odd[1] = b.n_pair_reads ? 0 : b.rb.n_odd;
    }
    // rows, lengths and the sorted list of odd bytes straight into the batch's page-locked buffers; the list is split at the first read of the
    // single-read part, whose reads are numbered from 0 like a batch of its own
    void pack_mapped_dev(Batch &b)
    {
        const uint32_t npr = b.n_pair_reads;
        mcx_fastq_out o;
        memset(&o, 0, sizeof o);
        if (fq_info.n_reads != b.n) b.error = "-gpu_parse: the device counted " + std::to_string(fq_info.n_reads) + " reads, the reader " + std::to_string(b.n);
        else if (fq_info.n_odd && !b.reserve_odd(fq_info.n_odd)) b.error = "cannot allocate pinned host memory";
        else {
            o.rows = b.rows; o.row_words = 0; o.len = b.lens; o.odd = b.odd; o.odd_cap = fq_info.n_odd;
            if (mcx_fastq_staged_out(fq_parser.get(), &o, &fq_info) != 0) b.error = std::string("-gpu_parse: ") + mcx_last_error();
            else {
                const uint64_t *cut = std::lower_bound(b.odd, b.odd + fq_info.n_odd, (uint64_t)npr << 32);
                b.n_odd[0] = (uint32_t)(cut - b.odd); b.n_odd[1] = fq_info.n_odd - b.n_odd[0];
                for (uint64_t *w = b.odd + b.n_odd[0]; w < b.odd + fq_info.n_odd; w++) *w -= (uint64_t)npr << 32;
            }
        }
    }
    // plain FASTA with -gpu_parse: as pack_mapped_dev, from the batch the resident object holds on the device
    void pack_fasta_dev(Batch &b)
    {
        const uint32_t npr = b.n_pair_reads, n_odd = b.rb.n_odd;
        mcx_fastq_out o;
        memset(&o, 0, sizeof o);
        if (b.rb.n_reads != b.n) b.error = "-gpu_parse: the device counted " + std::to_string(b.rb.n_reads) + " reads, the reader " + std::to_string(b.n);
        else if (n_odd && !b.reserve_odd(n_odd)) b.error = "cannot allocate pinned host memory";
        else {
            o.rows = b.rows; o.row_words = 0; o.len = b.lens; o.odd = b.odd; o.odd_cap = n_odd;
            if (mcx_resident_host_out(resident.get(), &o) != 0) b.error = std::string("-gpu_parse: ") + mcx_last_error();
            else {
                const uint64_t *cut = std::lower_bound(b.odd, b.odd + n_odd, (uint64_t)npr << 32);
                b.n_odd[0] = (uint32_t)(cut - b.odd); b.n_odd[1] = n_odd - b.n_odd[0];
                for (uint64_t *w = b.odd + b.n_odd[0]; w < b.odd + n_odd; w++) *w -= (uint64_t)npr << 32;
            }
        }
    }
    void pack_host(Batch &b)
    {
        const uint32_t n = b.n, npr = b.n_pair_reads;
        std::vector<uint64_t> all_odd[2];
        for (int part = 0; part < 2; part++) { // (a part's reads are numbered from 0: it is a batch of its own on the device)
            const uint32_t first = part ? npr : 0, cnt = part ? n - npr : npr;
            if (!cnt) continue;
            std::vector<std::vector<uint64_t>> odd((size_t)pool.slices(cnt, 4096));
            pool.for_range(cnt, 4096, [&](int k, uint64_t lo, uint64_t hi) {
                for (uint32_t r = first + (uint32_t)lo; r < first + (uint32_t)hi; r++) {
                    const char *base;
                    const Rec &e = b.rec(r, base);
                    b.lens[r] = e.rlen;
                    pack_row((const uint8_t *)base + e.seq, e.rlen, r - first, b.rows + (size_t)r * b.row_words, b.row_words, odd[(size_t)k]);
                }
            });
            for (auto &o : odd) all_odd[part].insert(all_odd[part].end(), o.begin(), o.end());
        }
        const size_t total = all_odd[0].size() + all_odd[1].size();
        if (total && !b.reserve_odd(total)) b.error = "cannot allocate pinned host memory";
        else if (total) {
            memcpy(b.odd, all_odd[0].data(), all_odd[0].size() * 8);
            memcpy(b.odd + all_odd[0].size(), all_odd[1].data(), all_odd[1].size() * 8);
        }
        b.n_odd[0] = (uint32_t)all_odd[0].size(); b.n_odd[1] = (uint32_t)all_odd[1].size();
    }
    // device_sam: names and qualities as mcx_sam_in takes them, a part's qualities where the device's offsets (the running sum of the lengths) put its reads
    void stage_sam_names(Batch &b)
    {
        const uint32_t n = b.n, npr = b.n_pair_reads;
        uint64_t names = 0, quals[2] = {0, 0};
        for (uint32_t r = 0; r < n; r++) { const char *base; names += b.rec(r, base).name_len; }
        b.sam_qual_at.resize(n);
        if (!b.reserve_sam(n, names, 0)) b.error = "cannot allocate pinned host memory";
        else {
            uint32_t *no = b.sam_name_off;
            for (uint32_t r = 0; r < n; r++) {
                const uint32_t part = r >= npr ? 1u : 0u;
                const char *base;
                const Rec &e = b.rec(r, base);
                if (r == 0 || r == npr) no[r + part] = 0;
                no[r + part + 1] = no[r + part] + e.name_len;
                b.sam_qual_at[r] = quals[part]; quals[part] += e.rlen;
            }
            b.sam_part_names[0] = npr ? no[npr] : 0; b.sam_part_names[1] = npr < n ? no[n + 1] : 0;
            b.sam_part_qual[0] = quals[0]; b.sam_part_qual[1] = quals[1];
            if (!b.reserve_sam(n, names, b.fastq ? quals[0] + quals[1] : 0)) b.error = "cannot allocate pinned host memory";
        }
        if (!b.error.empty()) return;
        pool.for_range(n, 4096, [&](int, uint64_t lo, uint64_t hi) {
            for (uint32_t r = (uint32_t)lo; r < (uint32_t)hi; r++) {
                const uint32_t part = r >= npr ? 1u : 0u;
                const char *base;
                const Rec &e = b.rec(r, base);
                memcpy(b.sam_names + (part ? b.sam_part_names[0] : 0) + b.sam_name_off[r + part], base + e.name, e.name_len);
                if (b.fastq) {
                    uint8_t *q = b.sam_qual + (part ? b.sam_part_qual[0] : 0) + b.sam_qual_at[r];
                    memcpy(q, base + e.qual, e.q_take);
                    memset(q + e.q_take, 0, e.rlen - e.q_take); // (what strncpy leaves behind a short quality line)
                }
            }
        });
    }

    // ---- stage 3: format + write -------------------------------------------------------------------------------------
    // (the text of batch i + 1 is made while batch i's is written)
    void format_loop()
    {
        bool stop = false;
        while (!stop) {
            BatchPtr b = mapped.pop();
            if (b->last) stop = true;
            b->sam_bytes = 0;
            if (dev_sam) { if (b->n && write_rc == 0) b->sam_bytes = b->dev_bytes; } // (made in HBM behind the batch's kernels: nothing to do here)
            else if (sam_fd >= 0 && b->n && write_rc == 0) {
                const Tick t0 = now();
                b->slices.resize((size_t)fpool.slices(b->n, 2048));
                fpool.for_range(b->n, 2048, [&](int k, uint64_t lo, uint64_t hi) {
                    Text &o = b->slices[(size_t)k];
                    size_t bound = 0;
                    for (uint32_t r = (uint32_t)lo; r < (uint32_t)hi; r++) {
                        const char *base;
                        const Rec &e = b->rec(r, base);
                        bound += sam_bound_read(hix, *b, r, e.name_len, e.rlen);
                    }
                    o.start(bound);
                    for (uint32_t r = (uint32_t)lo; r < (uint32_t)hi; r++) sam_record(hix, *b, r, o);
                });
                for (const Text &o : b->slices) b->sam_bytes += o.size();
                t.format += secs(t0, now());
            } else for (Text &o : b->slices) o.w = nullptr; // (no text of this batch; the buffers stay with the object)
            if (sharded && b->number % shard_count == shard_rank) places.put_size(b->number, b->sam_bytes); // (the other shards wait for the sizes of a round)
            const Tick tq = now();
            formatted.push(std::move(b));
            t.f_push += secs(tq, now());
        }
    }
    void write_loop()
    {
        uint64_t next_place = sam_base; // one shard: the batches follow one another
        bool stop = false;
        while (!stop) {
            BatchPtr b;
            if (waiting.empty()) b = formatted.pop();
            else if (!formatted.try_pop(b)) { flush_waiting(false); std::this_thread::sleep_for(std::chrono::microseconds(100)); continue; }
            if (b->last) stop = true;
            if (!sharded) { // its place is behind the batch before it
                if (sam_fd >= 0) write_out(*b, next_place);
                next_place += b->sam_bytes;
                spare.push(std::move(b));
            } else {
                // (a batch that carries nothing of this shard's — the news of the input's end — has no round of its own to be placed in)
                if (b->number % shard_count == shard_rank) waiting.push_back(std::move(b));
                else spare.push(std::move(b));
                flush_waiting(false);
            }
        }
        flush_waiting(true); // the places of the last rounds' text arrive with the closing exchanges
        if (bgzf && !sort && sam_fd >= 0 && write_rc == 0 && !write_all(sam_fd, (const char *)bgzf_eof, 28, next_place, sam_stream)) write_rc = MCX_ERR_IO; // (-bgzf is never sharded; -sort: the merge ends the file)
    }
    void flush_waiting(bool block) // batches whose place has arrived go out, oldest first
    {
        while (!waiting.empty()) {
            uint64_t at = 0;
            if (!places.wait_place(waiting.front()->number, at, block)) {
                if (!places.has_failed()) return; // not yet
                waiting.front()->sam_bytes = 0;   // the run has failed: nothing more is written
            }
            write_out(*waiting.front(), at);
            spare.push(std::move(waiting.front()));
            waiting.pop_front();
        }
    }
    void write_out(Batch &b, uint64_t at)
    {
        const Tick t1 = now();
        if (dev_sam) { // the batch's text is one piece, as it came from the device
            if (write_rc == 0 && !write_all(sam_fd, (const char *)b.dev_text, b.sam_bytes, at, sam_stream)) write_rc = MCX_ERR_IO;
        } else if (sam_stream) { for (Text &o : b.slices) if (o.size() && !write_all(sam_fd, o.b.data(), o.size(), 0, true)) write_rc = MCX_ERR_IO; }
        else if (b.sam_bytes) {
            std::vector<uint64_t> off(b.slices.size() + 1, at);
            for (size_t k = 0; k < b.slices.size(); k++) off[k + 1] = off[k] + b.slices[k].size();
            // Positioned writes, every slice at its final place, from this one thread: writers of one growing file queue up
            // behind its lock and get in each other's way (tools/ubench_filewrite.cpp on the bench box's tmpfs, a gigabyte of source text:
            // one thread 5.7 GB/s, two to sixteen 3.4-5.1; into pages that exist already 8.8 GB/s — but laying them out ahead of the
            // writer with fallocate(KEEP_SIZE) from a thread of its own, 128 MB at a time, made runs slower as often as faster, 1.17 / 1.59 s
            // against 1.31 / 1.28 for 6 GB of text: the two take the file's lock in turns; memcpy into a mapping of a sparse file 3.5-4.5 GB/s).
            // MCX_SAM_MMAP=1 keeps the mapping path for file systems where it pays; the file then grows under a lock of its
            // own and never shrinks: the other shards write further on.
            if (!(getenv("MCX_SAM_MMAP") && write_mapped(b, at, off)))
                for (size_t k = 0; k < b.slices.size() && write_rc == 0; k++)
                    if (!write_all(sam_fd, b.slices[k].b.data(), b.slices[k].size(), off[k], false)) write_rc = MCX_ERR_IO;
        }
        t.write += secs(t1, now());
    }
    bool write_mapped(Batch &b, uint64_t at, const std::vector<uint64_t> &off) // false: no mapping to be had
    {
        const uint64_t end = at + b.sam_bytes, page = (uint64_t)sysconf(_SC_PAGESIZE), a0 = at & ~(page - 1);
        struct stat st;
        bool ok = flock(sam_fd, LOCK_EX) == 0;
        if (ok) { ok = fstat(sam_fd, &st) == 0 && ((uint64_t)st.st_size >= end || ftruncate(sam_fd, (off_t)end) == 0); (void)flock(sam_fd, LOCK_UN); }
        char *m = ok ? (char *)mmap(nullptr, (size_t)(end - a0), PROT_READ | PROT_WRITE, MAP_SHARED, sam_fd, (off_t)a0) : (char *)MAP_FAILED;
        if (m == (char *)MAP_FAILED) return false;
        for (size_t k = 0; k < b.slices.size(); k++) { const Text &o = b.slices[k]; if (o.size()) memcpy(m + (off[k] - a0), o.b.data(), o.size()); } // (the pool belongs to the formatter)
        (void)munmap(m, (size_t)(end - a0));
        return true;
    }

    // ---- stage 2 (the calling thread): copy in | map | copy out, three parts of batches on the device at a time ------------------
    int place_round(uint64_t round, bool own) // the shards' batches of a round find their places in the file
    {
        uint64_t mine = 0;
        if (own && !places.wait_size(round * shard_count + shard_rank, mine)) mine = 0;
        if (int e = sh.gather(&mine, sizeof mine)) return e;
        uint64_t at = place_next;
        for (uint64_t r = 0; r < shard_count; r++) {
            uint64_t v; memcpy(&v, sh.recv.data() + (size_t)r * sizeof v, sizeof v);
            if (r == shard_rank && own) places.put_place(round * shard_count + shard_rank, at);
            at += v;
        }
        place_next = at;
        return 0;
    }
    int collect_oldest() // the oldest mapped part has arrived in host memory
    {
        const Tick tq = now();
        const int e = mcx_stream_collect(c, nullptr, nullptr);
        if (!leaving.empty() && !leaving.front()->parts_out.empty()) { // (-m) the part's extras came with it
            Batch *b = leaving.front().get();
            const bool second = b->parts_out.front();
            b->parts_out.pop_front();
            Batch::Extras &x = b->mx[second ? 1 : 0];
            x.index.clear(); x.recs.clear(); x.cig.clear();
            const uint32_t *ix = nullptr, *cg = nullptr; const mcx_aln32 *rs = nullptr; uint32_t nr = 0, nl = 0, nw = 0;
            if (e == 0 && multi && mcx_stream_multi(c, &ix, &rs, &cg, &nr, &nl, &nw) == 0 && nr) {
                x.index.assign(ix, ix + nr + 1); x.cig.assign(cg, cg + nw); x.recs.resize(nl);
                for (uint32_t i = 0; i < nl; i++) mcx_aln_unpack(&rs[i], &x.recs[i]);
            }
        }
        t.m_collect += secs(tq, now());
        in_flight--;
        if (!leaving.empty() && --leaving_parts.front() == 0) { mapped.push(std::move(leaving.front())); leaving.pop_front(); leaving_parts.pop_front(); }
        return e;
    }
    void collect_until(size_t left) { while (leaving.size() > left) { const int e = collect_oldest(); if (e && rc == 0) rc = e; } }
    int submit(Batch *p)
    {
        const uint32_t n = p->n, npr = p->n_pair_reads;
        int e = 0;
        if (p->resident) { // the arrays lie in HBM: device-to-device into the slot (one part: npr is 0 or n)
            e = mcx_stream_submit_dev(c, p->rb.rows, p->rb.row_words, p->rb.len, n, p->rb.n_odd ? p->rb.odd : nullptr, p->rb.n_odd);
            if (e == 0) in_flight++;
            return e;
        }
        if (npr) { e = mcx_stream_submit_packed(c, p->rows, p->row_words, p->lens, npr, p->odd, p->n_odd[0]); if (e) return e; in_flight++; }
        if (npr < n) {
            e = mcx_stream_submit_packed(c, p->rows + (size_t)npr * p->row_words, p->row_words, p->lens + npr, n - npr, p->odd ? p->odd + p->n_odd[0] : nullptr, p->n_odd[1]);
            if (e) return e;
            in_flight++;
        }
        return 0;
    }
    void take_next(bool block) // a parsed batch, its copy to the device started when there is room
    {
        if (nxt || input_done) return;
        BatchPtr b;
        const Tick tq = now();
        if (block) b = parsed.pop(); else if (!parsed.try_pop(b)) return;
        t.m_take += secs(tq, now());
        if (b->last) input_done = true;
        if (rc == 0 && !b->error.empty()) rc = mcx_set_error(b->error_code(), b->error);
        if (rc || ended) b->n = 0;
        nxt = std::move(b); nxt_in = false;
    }
    void try_submit_next()
    {
        if (!nxt || nxt_in || rc) return;
        if (nxt->n == 0) { nxt_in = true; return; }
        if (in_flight + nxt->n_parts() > 3) return;
        const Tick tq = now();
        const int e = submit(nxt.get());
        t.m_submit += secs(tq, now());
        if (e) rc = e; else nxt_in = true;
    }
    // the next part of `cur` that was copied in: where it lies on the device
    bool part_in()
    {
        const Tick tq = now();
        const int e = mcx_stream_next(c, &d_bases, &d_off, &n_dev, &d_aln, &d_cig);
        t.m_in += secs(tq, now());
        if (e && rc == 0) rc = e;
        return e == 0;
    }
    void part_out(Batch *p, bool second)
    {
        const Tick tq = now();
        const int e = second ? mcx_stream_mapped32(c, p->recs + p->n_pair_reads, p->cig + MCX_CIGAR_POOL_WORDS(p->n_pair_reads)) : mcx_stream_mapped32(c, p->recs, p->cig);
        t.m_out += secs(tq, now());
        if (e && rc == 0) rc = e;
        if (e == 0) { parts_out++; p->parts_out.push_back(second); }
    }
    void part_text(Batch *p, bool second, uint32_t cnt) // device_sam: the mapped part's text, made where its records lie and brought to the batch's page-locked buffer
    {
        if (!dev_sam || rc || !cnt) return;
        const Tick tq = now();
        const uint32_t npr = p->n_pair_reads;
        uint64_t got = 0;
        const int e = p->resident ? mcx_sam_part_dev(c, d_bases, d_off, cnt, second ? 0 : 1, p->rb.names, p->rb.name_off, p->fastq ? p->rb.qual : nullptr, d_aln, d_cig, &p->dev_text, &p->dev_text_cap, p->dev_bytes, &got, bgzf ? &zs : nullptr) :
                      mcx_sam_part(c, d_bases, d_off, cnt, second ? 0 : 1, p->sam_names + (second ? p->sam_part_names[0] : 0), p->sam_name_off + (second ? npr + 1 : 0),
                                   p->fastq ? p->sam_qual + (second ? p->sam_part_qual[0] : 0) : nullptr, p->sam_part_qual[second ? 1 : 0], d_aln, d_cig,
                                   &p->dev_text, &p->dev_text_cap, p->dev_bytes, &got, bgzf ? &zs : nullptr);
        if (e) rc = e;
        else {
            if (sort && !note_run(p->dev_text + p->dev_bytes, got, tmp_at + p->dev_bytes)) rc = mcx_set_error(MCX_ERR_DEVICE, "-sort: the part's blocks do not walk as BGZF");
            p->dev_bytes += got;
        }
        t.m_sam += secs(tq, now());
    }
    void part_md(Batch *p, bool second, uint32_t cnt) // -md for the host formatter: the mapped part's MD strings, made where its records lie
    {
        if (!host_md || rc || !cnt) return;
        const Tick tq = now();
        Batch::Md &m = p->md[second ? 1 : 0];
        if (const int e = mcx_md_part_host(c, d_bases, d_off, cnt, second ? 0 : 1, d_aln, d_cig, &m.bytes, &m.off)) rc = e;
        t.m_sam += secs(tq, now());
    }
    // one shard: the batch's parts are mapped as they are
    void map_alone(Batch *p, uint32_t n_pr, uint32_t n_sg)
    {
        if (n_pr && part_in()) { const Tick tq = now(); if (rc == 0) rc = mcx_map_batch_dev(c, d_bases, d_off, n_pr, 1, avg, d_aln, d_cig, stats); t.m_dev += secs(tq, now()); t.each_dev.push_back(secs(tq, now())); part_md(p, false, n_pr); part_text(p, false, n_pr); part_out(p, false); }
        if (n_sg && part_in()) { if (rc == 0) rc = mcx_map_batch_dev(c, d_bases, d_off, n_sg, 0, avg, d_aln, d_cig, stats); part_md(p, true, n_sg); part_text(p, true, n_sg); part_out(p, true); }
    }
    // one round of a sharded run (mcx_shards.h): what every shard holds, the paired parts, the single reads, the places of an earlier round's text
    void map_round(Batch *p, uint32_t n_pr, uint32_t n_sg)
    {
        rounds_done = p->number / shard_count + 1;
        Shards::Head h = {rc, rc ? 0u : n_pr, rc ? 0u : n_sg, p->last ? 1u : 0u};
        int e = sh.gather(&h, sizeof h);
        bool any_pair = false, any_single = false;
        uint64_t before = 0, round_total = 0;
        uint32_t my_pr = rc ? 0u : n_pr, my_sg = rc ? 0u : n_sg;
        if (e) rc = e;
        else {
            // the input ends with the first batch of the round that says so: the batches behind it do not exist
            int cut = sh.x->size;
            for (int r = 0; r < sh.x->size; r++) { Shards::Head o; memcpy(&o, sh.recv.data() + (size_t)r * sizeof o, sizeof o); if (o.last && r < cut) cut = r; }
            for (int r = 0; r < sh.x->size; r++) {
                Shards::Head o; memcpy(&o, sh.recv.data() + (size_t)r * sizeof o, sizeof o);
                if (o.rc && rc == 0) rc = mcx_set_error(o.rc, "shard " + std::to_string(r) + " failed");
                if (r > cut) { o.n_pair = o.n_single = 0; if (r == sh.x->rank) my_pr = my_sg = 0; }
                any_pair |= o.n_pair != 0; any_single |= o.n_single != 0;
                if (r < sh.x->rank) before += (uint64_t)o.n_pair + o.n_single;
                round_total += (uint64_t)o.n_pair + o.n_single;
            }
            if (cut < sh.x->size) { ended = true; abort.store(true); }
        }
        if (rc) my_pr = my_sg = 0;
        const int64_t round_base = avg[3];
        // (a part that was copied in but does not count any more — the input ended in a batch before this one — still leaves the device)
        const bool in1 = n_pr && part_in();
        if (rc == 0 && any_pair) rc = sh.pairs(c, d_bases, d_off, in1 ? my_pr : 0u, round_base + (int64_t)before, avg, profile, d_aln, d_cig, stats);
        if (in1) { part_text(p, false, my_pr); part_out(p, false); }
        const bool in2 = n_sg && part_in();
        if (rc == 0 && any_single) rc = sh.singles(c, d_bases, d_off, in2 ? my_sg : 0u, round_base + (int64_t)before + my_pr, profile, d_aln, d_cig, stats);
        if (in2) { part_text(p, true, my_sg); part_out(p, true); }
        if (my_pr == 0 && my_sg == 0) p->n = 0; // (nothing of this batch counts)
        avg[3] = round_base + (int64_t)round_total;
        if (rc) dead = true;
        // the text of an earlier round finds its place (two rounds later every formatter has long been through it)
        rounds_unplaced.push_back(std::make_pair(p->number / shard_count, p->number % shard_count == shard_rank));
        while (rounds_unplaced.size() > 2 && !dead) { const int e3 = place_round(rounds_unplaced.front().first, rounds_unplaced.front().second); rounds_unplaced.pop_front(); if (e3) { rc = e3; dead = true; } }
    }
    void map_loop()
    {
        for (;;) {
            if (!cur) {
                if (!nxt) { if (input_done) break; take_next(true); }
                while (nxt && !nxt_in && rc == 0) { try_submit_next(); if (!nxt_in && rc == 0) { const int e = collect_oldest(); if (e) rc = e; } }
                cur = std::move(nxt); cur_in = nxt_in; nxt_in = false;
                if (rc) { cur->n = 0; abort.store(true); }
            }
            // the batch behind it: parsed already?  then its copy in runs under this one's kernels
            take_next(false);
            try_submit_next();
            Batch *p = cur.get();
            const Tick t1 = now();
            // what of the batch is on the device (copied in, or on its way); after a failure it leaves the device unmapped
            const uint32_t n_pr = cur_in ? p->n_pair_reads : 0u, n_sg = cur_in ? p->n - p->n_pair_reads : 0u;
            parts_out = 0;
            d_bases = nullptr; d_off = nullptr; d_aln = nullptr; d_cig = nullptr; n_dev = 0;
            p->has_mx = multi;
            p->has_md = host_md;
            p->rg = rg_id.empty() ? nullptr : &rg_id; p->mate_tags = host_mate_tags;
            for (Batch::Md &m : p->md) { m.bytes.clear(); m.off.clear(); }
            for (Batch::Extras &x : p->mx) { x.index.clear(); x.recs.clear(); x.cig.clear(); }
            p->parts_out.clear();
            p->dev_bytes = 0;
            if (!sharded) map_alone(p, n_pr, n_sg);
            else if (!dead && !ended && p->number / shard_count >= rounds_done) map_round(p, n_pr, n_sg);
            else {
                // (sharded, after the end of the input or a failure: what is on the device leaves it unmapped)
                if (n_pr && part_in()) part_out(p, false);
                if (n_sg && part_in()) part_out(p, true);
                p->n = 0;
            }
            if (p->n) t.map += secs(t1, now());
            if (t.w_first_mapped == 0) t.w_first_mapped = t.wall();
            if (rc) { p->n = 0; abort.store(true); places.fail(); }
            if (sort) tmp_at += p->n ? p->dev_bytes : 0; // (the writer puts the batches one behind the other, those that count)
            if (parts_out == 0) { // nothing on its way out: the batch goes on as it is, behind the ones that are
                collect_until(0);
                mapped.push(std::move(cur));
            } else { leaving.push_back(std::move(cur)); leaving_parts.push_back(parts_out); }
            cur.reset(); cur_in = false;
            collect_until(1); // at most one batch's parts on their way out behind the one mapped next
        }
        collect_until(0);
        // (sharded) the places of the last rounds' text
        while (sharded && !rounds_unplaced.empty()) {
            if (!dead) { const int e = place_round(rounds_unplaced.front().first, rounds_unplaced.front().second); if (e) { if (rc == 0) rc = e; dead = true; places.fail(); } }
            rounds_unplaced.pop_front();
        }
        if (rc) places.fail();
        t.w_mapped = t.wall();
    }


    // ---- -sort: the runs, and the merge behind the last batch ---------------------------------------------------------------
    // a part has come back as `bytes` of BGZF blocks that will lie at byte `at` of the temporary file: its keys and lengths (the sink) and its block table
    bool note_run(const uint8_t *blocks, uint64_t bytes, uint64_t at)
    {
        if (sink.keys.empty()) return true;
        runs.emplace_back();
        sortplan::Run &r = runs.back();
        r.keys.swap(sink.keys); r.lens.swap(sink.lens);
        if (markdup) {
            dup_runs.emplace_back();
            DupRun &d = dup_runs.back();
            d.grp.swap(dsink.grp); d.base = dsink.part_base; d.paired = dsink.part_paired;
            if (d.grp.size() != r.lens.size()) return false;
        }
        uint64_t u = 0;
        for (uint64_t o = 0; o < bytes;) { // BSIZE at byte 16 of a block of ours, ISIZE in its last four
            if (bytes - o < 26 || blocks[o] != 0x1f || blocks[o + 1] != 0x8b || blocks[o + 12] != 'B' || blocks[o + 13] != 'C') return false;
            const uint32_t size = ((uint32_t)blocks[o + 16] | (uint32_t)blocks[o + 17] << 8) + 1;
            if (size < 26 || size > bytes - o) return false;
            const uint8_t *q = blocks + o + size - 4;
            const uint32_t isize = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
            sortplan::Block b; b.c_off = at + o; b.c_size = size; b.u_size = isize; b.u_off = u;
            r.blocks.push_back(b);
            u += isize; o += size;
        }
        r.finish();
        return r.bytes == u;
    }
    void drop_tmp() // the temporary file goes, however the run ends; the file asked for is sam_fd again
    {
        if (tmp_path.empty()) return;
        if (sam_fd >= 0) close(sam_fd);
        unlink(tmp_path.c_str());
        tmp_path.clear();
        sam_fd = out_fd; sam_stream = out_stream; out_fd = -1;
    }
    // every step of a chunk is one bulk operation: pread of the covering blocks, one inflate over all of them, the sort core, the deflater, one write
    int merge()
    {
        const Tick t_begin = now();
        if (markdup) if (const int e = resolve_duplicates()) return e;
        uint64_t chunk_bytes = 256ull << 20;
        if (const char *env = getenv("MCX_SORT_CHUNK")) { const long long v = atoll(env); if (v >= 1) chunk_bytes = (uint64_t)v; } // (debug override)
        sortplan::Plan plan;
        sortplan::make_plan(runs, chunk_bytes, &plan);
        for (sortplan::Run &r : runs) std::vector<uint64_t>().swap(r.keys); // (the plan is made: 8 of the 12 bytes a record go)
        uint64_t *ss = kept->sort_stats;
        ss[0] = runs.size(); ss[1] = plan.chunks.size();
        const int tmp_fd = sam_fd;
        const int fd = out_fd; const bool stream = out_stream;
        uint64_t place = 0;
        int e = 0;
        // the header, blocks of its own
        {
            uint64_t n = 0;
            (void)mcx_bam_header_rg(idx, rg_or_null(), 1, nullptr, 0, &n);
            std::string hdr((size_t)n, '\0');
            if (n == 0 || mcx_bam_header_rg(idx, rg_or_null(), 1, (uint8_t *)&hdr[0], n, &n) != 0) return mcx_set_error(MCX_ERR_UNSUPPORTED, std::string("-bam: ") + mcx_last_error());
            std::string blocks((size_t)mcx_bgzf_bound(hdr.size(), zs.block), '\0');
            uint64_t made = 0;
            if ((e = mcx_bgzf_deflate(zs.deflater, (const uint8_t *)hdr.data(), hdr.size(), (uint8_t *)&blocks[0], blocks.size(), &made))) return e;
            if (!write_all(fd, blocks.data(), (size_t)made, place, stream)) return mcx_set_error(MCX_ERR_IO, std::string("cannot write ") + sam_path);
            place += made;
        }
        if (index && (e = mcx_bai_begin(c, &bai))) { mcx_bai_free(c, &bai); return e; }
        mcx_inflater *inf = nullptr;
        if (mcx_inflater_create_dev(idx->device, 0, 1u << 16, &inf) != 0) { if (index) mcx_bai_free(c, &bai); return mcx_set_error(MCX_ERR_DEVICE, std::string("-sort: ") + mcx_last_error()); }
        uint8_t *h_src = nullptr, *h_out = nullptr;
        uint64_t h_src_cap = 0, h_out_cap = 0;
        std::vector<mcx_deflate_member> members;
        std::vector<uint32_t> lens;
        std::vector<uint8_t> bits;
        std::vector<uint64_t> first, base;
        for (size_t k = 0; k < plan.chunks.size() && e == 0; k++) {
            const sortplan::Chunk &ch = plan.chunks[k];
            if (ch.records == 0) continue;
            uint64_t src_bytes = 0;
            for (const sortplan::Slice &sl : ch.slices) { const sortplan::Run &r = runs[sl.run]; src_bytes += r.blocks[sl.k1 - 1].c_off + r.blocks[sl.k1 - 1].c_size - r.blocks[sl.k0].c_off; }
            if (src_bytes + 8 > h_src_cap) {
                mcx_pinned_free(h_src);
                h_src_cap = src_bytes + src_bytes / 8 + 4096;
                if (!(h_src = (uint8_t *)mcx_pinned_alloc(h_src_cap))) { h_src_cap = 0; e = mcx_set_error(MCX_ERR_DEVICE, "-sort: cannot allocate pinned host memory for a chunk's blocks"); break; }
            }
            members.clear(); lens.clear(); bits.clear(); first.clear(); base.clear();
            uint64_t so = 0, to = 0;
            const Tick t0 = now();
            for (const sortplan::Slice &sl : ch.slices) {
                const sortplan::Run &r = runs[sl.run];
                const uint64_t c0 = r.blocks[sl.k0].c_off, cn = r.blocks[sl.k1 - 1].c_off + r.blocks[sl.k1 - 1].c_size - c0;
                for (uint64_t done = 0; done < cn && e == 0;) {
                    const ssize_t got = pread(tmp_fd, h_src + so + done, (size_t)(cn - done), (off_t)(c0 + done));
                    if (got <= 0) e = mcx_set_error(MCX_ERR_IO, "-sort: cannot read the temporary file " + tmp_path); else done += (uint64_t)got;
                }
                if (e) break;
                first.push_back(lens.size());
                base.push_back(to + (sl.b0 - r.blocks[sl.k0].u_off));
                lens.insert(lens.end(), r.lens.begin() + (ptrdiff_t)sl.r0, r.lens.begin() + (ptrdiff_t)sl.r1);
                if (markdup) bits.insert(bits.end(), dup_runs[sl.run].bits.begin() + (ptrdiff_t)sl.r0, dup_runs[sl.run].bits.begin() + (ptrdiff_t)sl.r1);
                for (uint64_t j = sl.k0; j < sl.k1; j++) {
                    const sortplan::Block &b = r.blocks[j];
                    if (b.u_size) {
                        const uint8_t *q = h_src + so + (b.c_off - c0) + b.c_size - 8;
                        mcx_deflate_member m; memset(&m, 0, sizeof m);
                        m.src_off = so + (b.c_off - c0) + 18; m.src_len = b.c_size - 26; m.dst_off = to; m.isize = b.u_size;
                        m.crc32 = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
                        members.push_back(m);
                    }
                    to += b.u_size;
                }
                ss[2]++; ss[4] += cn;
                if (sl.b0 != r.blocks[sl.k0].u_off) { ss[3]++; ss[5] += r.blocks[sl.k0].c_size; } // (the slice before it in the run has read this block too)
                so += cn;
            }
            if (e) break;
            sort_secs[0] += secs(t0, now());
            memset(h_src + so, 0, 8);
            uint64_t made = 0;
            e = mcx_bam_sort_chunk(c, inf, zs.deflater, zs.block, h_src, so + 8, members.data(), (uint32_t)members.size(), to, lens.data(), lens.size(), first.data(), base.data(), (uint32_t)first.size(),
                                   ch.bytes, &h_out, &h_out_cap, &made, sort_secs + 1, index ? &bai : nullptr, place, markdup ? &dsink : nullptr, bits.data());
            if (e) break;
            indexed_records += lens.size();
            const Tick t1 = now();
            if (!write_all(fd, (const char *)h_out, (size_t)made, place, stream)) e = mcx_set_error(MCX_ERR_IO, std::string("cannot write ") + sam_path);
            t.write += secs(t1, now());
            place += made;
        }
        if (e == 0 && !write_all(fd, (const char *)bgzf_eof, 28, place, stream)) e = mcx_set_error(MCX_ERR_IO, std::string("cannot write ") + sam_path);
        if (index) { // the EOF block's place ends the last chunk of the index
            if (e == 0) e = mcx_bai_end(c, &bai, place, &bai_bytes);
            mcx_bai_free(c, &bai);
        }
        mcx_pinned_free(h_src); mcx_pinned_free(h_out);
        mcx_inflater_free(inf);
        merge_seconds = secs(t_begin, now());
        return e;
    }
    // -markdup, behind the last batch and ahead of the plan: the run's units are resolved on the device once, and every run's groups become its records' bytes —
    // a pair unit's verdict goes to both reads, a fragment unit's to the read that is placed, never to a mate without a place
    int resolve_duplicates()
    {
        std::vector<uint8_t> dup;
        if (const int e = mcx_markdup_resolve(c, &dsink, &dup)) return e;
        const Tick t0 = now();
        const std::vector<mcx_dup_unit> &units = dsink.units;
        uint64_t *ms = kept->markdup_stats;
        // per unit, which of its reads take the verdict: bit 0 the first (or only) read, bit 1 the second — the loop over the records then reads a byte, not a unit
        std::vector<uint8_t> takes(units.size());
        for (size_t u = 0; u < units.size(); u++) {
            const uint32_t kind = units[u].kind & 3u, second = (units[u].kind >> 2) & 1u;
            if (kind == 2) { ms[0]++; ms[1] += dup[u]; } else if (kind == 1) { ms[2]++; ms[3] += dup[u]; }
            takes[u] = !dup[u] ? 0 : kind == 2 ? 3 : kind == 1 ? (second ? 2 : 1) : 0;
        }
        ms[4] = dsink.groups;
        if (dup_runs.size() != runs.size()) return mcx_set_error(MCX_ERR_DEVICE, "-markdup: the runs and their groups do not match");
        for (DupRun &d : dup_runs) {
            d.bits.resize(d.grp.size());
            const uint32_t shift = d.paired ? 1 : 0;
            for (size_t i = 0; i < d.grp.size(); i++) {
                const uint32_t g = d.grp[i];
                const uint64_t u = d.base + (g >> shift);
                if (u >= takes.size()) return mcx_set_error(MCX_ERR_DEVICE, "-markdup: a record's group has no unit");
                d.bits[i] = (uint8_t)((takes[u] >> (g & shift)) & 1u);
            }
            std::vector<uint32_t>().swap(d.grp);
        }
        std::vector<mcx_dup_unit>().swap(dsink.units); // (the units go: from here on a byte a record)
        dup_host_seconds += secs(t0, now());
        return 0;
    }
    // behind the threads: the merge when all went well, and the end of the temporary file whatever happened
    void finish_sort()
    {
        if (!sort) return;
        memset(kept->sort_stats, 0, sizeof kept->sort_stats);
        memset(kept->markdup_stats, 0, sizeof kept->markdup_stats);
        if (rc == 0 && write_rc.load() == 0 && out_fd >= 0) rc = merge();
        if (markdup) {
            uint64_t *ms = kept->markdup_stats;
            if (rc) memset(ms, 0, sizeof kept->markdup_stats);
            else {
                ms[5] = (uint64_t)((dsink.seconds[0] + dsink.seconds[1] + dsink.seconds[2] + dup_host_seconds) * 1e6);
                fprintf(stderr, "markdup: %llu of %llu pairs and %llu of %llu single reads are duplicates, in %llu groups\n", (unsigned long long)ms[1], (unsigned long long)ms[0],
                        (unsigned long long)ms[3], (unsigned long long)ms[2], (unsigned long long)ms[4]);
            }
        }
        drop_tmp();
    }

    // -bam: the lines htslib's parser would have rejected made no record; said once a call, when there are any
    void report_dropped() const
    {
        if (bam && zs.dropped) fprintf(stderr, "Warning! %llu SAM lines made no BAM record (a read name of 252 bytes or more, or a quality line shorter than its read)\n", (unsigned long long)zs.dropped);
    }
    void report_timing() const
    {
        if (!getenv("MCX_TIMING")) return;
        std::string e;
        for (size_t k = 0; k < t.each_dev.size() && k < 24; k++) e += " " + std::to_string((int)(t.each_dev[k] * 1e4) / 10.0).substr(0, 5);
        fprintf(stderr, "[mcx_map_files] mcx_map_batch_dev, ms per batch:%s\n", e.c_str());
        fprintf(stderr, "[mcx_map_files] on the device (1 inflate, 2 parse, 4 rows from HBM, 8 SAM text, 16 BGZF blocks, 32 BAM records, 512 gunzip, 1024 BAM input): file 1 %u, file 2 %u%s\n", kept->route[0], kept->route[1], route == kResident ? " — the resident route" : "");
        if (dev_sam) fprintf(stderr, "[mcx_map_files] device_sam: names + qualities in, text made and brought back %.3f s of the mapper's time\n", t.m_sam);
        if (bgzf) fprintf(stderr, "[mcx_map_files] bgzf: %llu bytes of text -> %llu bytes of blocks (%u bytes of text a block), the deflater took %.3f s of them\n",
                          (unsigned long long)zs.text_bytes, (unsigned long long)zs.out_bytes, zs.block, zs.seconds);
        if (bam) fprintf(stderr, "[mcx_map_files] bam: the text above is BAM records; %llu lines made none\n", (unsigned long long)zs.dropped);
        if (sort) fprintf(stderr, "[mcx_map_files] sort: %llu runs (%.3f s of the mapper's time), %llu chunks of %llu slices (%llu start inside a block); the merge %.3f s: read %.3f, copy in %.3f, inflate %.3f, sort %.3f, deflate + copy out %.3f; %llu bytes read back, %llu of them twice\n",
                          (unsigned long long)kept->sort_stats[0], sink.run_seconds, (unsigned long long)kept->sort_stats[1], (unsigned long long)kept->sort_stats[2], (unsigned long long)kept->sort_stats[3], merge_seconds,
                          sort_secs[0], sort_secs[1], sort_secs[2], sort_secs[3], sort_secs[4], (unsigned long long)kept->sort_stats[4], (unsigned long long)kept->sort_stats[5]);
        if (index) fprintf(stderr, "[mcx_map_files] index: %llu records in %llu stretches, %llu bins and %llu linear entries written, %llu bytes; %.3f s of the merge (on the device: records %.3f, stretches %.3f, windows %.3f ms)\n",
                           (unsigned long long)indexed_records, (unsigned long long)bai.stats.stretches, (unsigned long long)bai.stats.bins, (unsigned long long)bai.stats.intervals, (unsigned long long)bai.stats.bytes,
                           bai.seconds, bai.ms[0], bai.ms[1], bai.ms[2]);
        if (markdup) fprintf(stderr, "[mcx_map_files] markdup: %llu pair units (%llu duplicates), %llu fragment units (%llu duplicates), %llu groups; units %.3f s of the mapper's time (on the device %.3f ms), resolve %.3f s (on the device %.3f ms) and %.3f s on the host, marks %.3f s of the merge's sort (on the device %.3f ms)\n",
                             (unsigned long long)kept->markdup_stats[0], (unsigned long long)kept->markdup_stats[1], (unsigned long long)kept->markdup_stats[2], (unsigned long long)kept->markdup_stats[3], (unsigned long long)kept->markdup_stats[4],
                             dsink.seconds[0], dsink.ms[0], dsink.seconds[1], dsink.ms[1], dup_host_seconds, dsink.seconds[2], dsink.ms[2]);
        fprintf(stderr, "[mcx_map_files] busy seconds: parse + pack %.3f (lines %.3f, rows %.3f; waited for a free batch %.3f) | map %.3f | format %.3f write %.3f  (%d + %d host threads, %s input)\n",
                t.parse, t.p_lines, t.p_pack, t.p_wait, t.map, t.format, t.write, threads, threads, mapped_input() ? "mapped" : "sequential");
        fprintf(stderr, "[mcx_map_files] waits: reader for room behind it %.3f | mapper for a parsed batch %.3f, for copies out %.3f | formatter for the writer %.3f || mapper's calls: submit %.3f, next %.3f, map_batch_dev %.3f, mapped %.3f\n", t.p_push, t.m_take, t.m_collect, t.f_push, t.m_submit, t.m_in, t.m_dev, t.m_out);
        fprintf(stderr, "[mcx_map_files] wall seconds: input opened and indexed %.3f | first batch parsed %.3f, mapped %.3f | last batch parsed %.3f, mapped %.3f | all written %.3f\n",
                t.w_open, t.w_first_parsed, t.w_first_mapped, t.w_reader, t.w_mapped, t.wall());
    }
};
} // namespace

extern "C" int mcx_map_files_ex(mcx_ctx *c, const char *fq1, const char *fq2, const mcx_file_opts *fo, const char *sam_path, mcx_stats *stats)
{
    return mcx_map_files_rg(c, fq1, fq2, fo, nullptr, sam_path, stats);
}

extern "C" int mcx_map_files_rg(mcx_ctx *c, const char *fq1, const char *fq2, const mcx_file_opts *fo, const char *read_group, const char *sam_path, mcx_stats *stats)
{
    if (!c || !fq1) return mcx_set_error(MCX_ERR_ARG, "mcx_map_files: null argument");
    mcx_file_opts opt;
    mcx_file_opts_default(&opt);
    if (fo) opt = *fo;
    if (opt.device_sam & MCX_SAM_BAM) opt.device_sam |= MCX_SAM_DEVICE | MCX_SAM_BGZF; // (BAM records are made on the device and framed as BGZF)
    // BAM read input: refused where it cannot be read, before anything is opened for writing; else it implies the resident route and the device formatter for this call
    const bool bam_in = bam_file(fq1);
    if (fq2 && fq2[0] && (bam_in || bam_file(fq2)))
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: a BAM read file holds both mates: it is given alone as the first file (-f reads.bam), not with or as a second file");
    if (bam_in && opt.shard_count > 1)
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: a sharded run does not read BAM input (-f reads.bam with -gpus N / -devices): map on one GPU");
    if (bam_in) {
        opt.device_inflate |= MCX_INFLATE_BGZF; opt.device_parse = 1; opt.interleaved_pairs = 0; // (the records' flags say whether they are pairs)
        if (sam_path && sam_path[0]) opt.device_sam |= MCX_SAM_DEVICE;
    }
    if (opt.shard_count > 1 && (!opt.exchange || !opt.exchange->allgather || opt.exchange->size != opt.shard_count || opt.exchange->rank != opt.shard_rank))
        return mcx_set_error(MCX_ERR_ARG, "mcx_map_files_ex: a sharded run needs mcx_file_opts.exchange with the shard's rank and count");
    if ((opt.device_sam & MCX_SAM_SORT) && !(opt.device_sam & MCX_SAM_BAM))
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: -sort puts BAM records into coordinate order and needs -bam (MCX_SAM_SORT without MCX_SAM_BAM); SAM text is not sorted");
    if ((opt.device_sam & MCX_SAM_SORT) && opt.append_sam)
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: a sorted file cannot be appended to (-sort with append_sam): map the libraries in one run, or merge the sorted files");
    if ((opt.device_sam & MCX_SAM_SORT) && opt.shard_count > 1)
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: a sharded run cannot write a sorted BAM file (-sort with -gpus N / -devices): map on one GPU");
    if ((opt.device_sam & MCX_SAM_INDEX) && !(opt.device_sam & MCX_SAM_SORT))
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: -index writes the .bai of a coordinate-sorted BAM file and needs -sort (MCX_SAM_INDEX without MCX_SAM_SORT); an unsorted file has no index");
    if ((opt.device_sam & MCX_SAM_MARKDUP) && !(opt.device_sam & MCX_SAM_SORT))
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: -markdup flags the duplicates of a coordinate-sorted BAM file and needs -sort (MCX_SAM_MARKDUP without MCX_SAM_SORT)");
    if ((opt.device_sam & MCX_SAM_MARKDUP) && mcx_ctx_multi(c))
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: -markdup takes one record a read: it cannot be combined with -m (a line for every equal-best alignment)");
    if ((opt.device_sam & MCX_SAM_INDEX) && sam_path && strcmp(sam_path, "-") == 0)
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: -index writes <file>.bai beside the BAM file: a file that goes to stdout has no name to put it beside");
    if (opt.device_sam & MCX_SAM_INDEX)
        for (int32_t len : mcx_ctx_index(c)->host.chr_len)
            if ((int64_t)len > (1ll << 29))
                return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: -index: a contig is longer than 2^29 bases, which a .bai cannot address (a .csi could: not offered)");
    if (opt.shard_count > 1 && (opt.device_sam & MCX_SAM_BGZF))
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: a sharded run cannot write its SAM file as BGZF or as BAM (-bgzf / -bam with -gpus N / -devices): map on one GPU, or without them");
    if (opt.shard_count > 1 && (opt.device_sam & MCX_SAM_MD))
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: a sharded run does not make MD tags (-md with -gpus N / -devices): map on one GPU, or without -md");
    // -rg / -mc: refused where they cannot be made, before anything is opened
    std::string rg_line, rg_id;
    if (read_group) {
        std::string why;
        if (!mcx::rg_parse(read_group, rg_line, rg_id, why)) return mcx_set_error(MCX_ERR_ARG, "mcx_map_files_rg: " + why);
        if (rg_line != read_group) return mcx_set_error(MCX_ERR_ARG, "mcx_map_files_rg: the read-group line must hold real TABs (mcx_rg_parse's line)");
    }
    if (opt.shard_count > 1 && (read_group || (opt.device_sam & MCX_SAM_MC)))
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: a sharded run does not make read-group or mate tags (-rg / -mc with -gpus N / -devices): map on one GPU, or without them");
    if ((opt.device_sam & MCX_SAM_MC) && mcx_ctx_multi(c))
        return mcx_set_error(MCX_ERR_UNSUPPORTED, "mcx_map_files_ex: -mc cannot be combined with -m: an extra line is paired with another candidate of the mate than the one whose CIGAR is held");
    // ... and, like -md, no output routes of their own: the bit comes off, and the context's device formatter calls are told (until the run is over)
    const bool with_out = sam_path && sam_path[0];
    const bool with_mc = (opt.device_sam & MCX_SAM_MC) != 0 && with_out;
    opt.device_sam &= ~(int32_t)MCX_SAM_MC;
    if (!with_out) { rg_line.clear(); rg_id.clear(); }
    // -md is no output route of its own: the bit comes off, and where the text is made on the device the context's formatter calls are told (until the run is over)
    const bool with_md = (opt.device_sam & MCX_SAM_MD) != 0 && sam_path && sam_path[0];
    opt.device_sam &= ~(int32_t)MCX_SAM_MD;
    struct MdSwitch { mcx_ctx *c; bool on; MdSwitch(mcx_ctx *ctx, bool o) : c(ctx), on(o) { if (on) mcx_md_set(c, 1); } ~MdSwitch() { if (on) mcx_md_set(c, 0); } } md_switch(c, with_md && opt.device_sam != 0);
    struct TagSwitch {
        mcx_ctx *c; bool on; int rc = 0;
        TagSwitch(mcx_ctx *ctx, bool o, const std::string &id, bool mc) : c(ctx), on(o) { if (on) rc = mcx_tags_set(c, id.data(), (uint32_t)id.size(), mc); }
        ~TagSwitch() { if (on) (void)mcx_tags_set(c, nullptr, 0, 0); }
    } tag_switch(c, (with_mc || !rg_id.empty()) && opt.device_sam != 0, rg_id, with_mc);
    if (tag_switch.rc) return tag_switch.rc;
    Run run(c, fq1, fq2, opt, sam_path, stats);
    run.bam_in = bam_in;
    run.host_md = with_md && opt.device_sam == 0;
    run.rg_line = rg_line;
    if (opt.device_sam == 0) { run.rg_id = rg_id; run.host_mate_tags = with_mc; }
    if (int e = run.open_input()) return e;
    if (int e = run.open_output()) return e;
    run.begin();
    std::thread reader([&] { run.read_loop(); });
    std::thread writer([&] { run.write_loop(); });
    std::thread formatter([&] { run.format_loop(); });
    run.map_loop();
    formatter.join();
    writer.join();
    reader.join();
    run.finish_sort();
    run.keep_objects();
    run.report_dropped();
    run.report_timing();
    return run.close_output();
}

extern "C" int mcx_map_files(mcx_ctx *c, const char *fq1, const char *fq2, const char *sam_path, mcx_stats *stats)
{
    return mcx_map_files_ex(c, fq1, fq2, nullptr, sam_path, stats);
}

// The file front end's parallel inflater on a file by itself (tests, scripts/gz_rate.py): the text of `path` into out[0 .. cap) as far as it fits; returns the
// text's whole length, -1 when the file cannot be mapped or is no gzip file, -2 when the stream is damaged (*n_out: what was delivered before that).
extern "C" int64_t mcx_gz_inflate(const char *path, int threads, uint64_t stretch_bytes, uint8_t *out, uint64_t cap, uint64_t *n_out)
{
    if (n_out) *n_out = 0;
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return -1;
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < 18) { close(fd); return -1; }
    void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return -1;
    int64_t total = 0;
    {
        Pool pool(std::max(1, threads));
        mcx::pgz::Reader rd;
        mcx::pgz::Text text;
        if (!rd.open((const uint8_t *)m, (size_t)st.st_size, pool.size(), stretch_bytes ? (size_t)stretch_bytes : (size_t)2 << 20, [&](int n, const std::function<void(int)> &f) { pool.run(n, f); })) total = -1;
        while (total >= 0 && rd.next(text)) {
            if (out && (uint64_t)total < cap) memcpy(out + total, text.data(), (size_t)std::min<uint64_t>(text.size(), cap - (uint64_t)total));
            total += (int64_t)text.size();
        }
        if (n_out) *n_out = (uint64_t)std::max<int64_t>(total, 0);
        if (rd.failed()) total = total < 0 ? -1 : -2;
    }
    munmap(m, (size_t)st.st_size);
    return total;
}

// The BGZF reader by itself (tests, scripts/bgzf_rate.py): the members of `path` inflated on `device`, a stretch of up to 8 MB of text per call of mcx_inflate;
// the text goes to out[0 .. cap) as far as it fits.  Returns the text's whole length (what is no member ends the input, as in the file front end), -1 when the
// file cannot be mapped or does not begin with a BGZF member, -2 when a member is damaged (*n_out: the bytes delivered before its stretch).
extern "C" int64_t mcx_bgzf_inflate(const char *path, int device, uint8_t *out, uint64_t cap, uint64_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!path) return -1;
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return -1;
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 28) { close(fd); return -1; }
    const size_t size = (size_t)st.st_size;
    void *mm = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (mm == MAP_FAILED) return -1;
    const uint8_t *map = (const uint8_t *)mm;
    size_t xlen = 0;
    mcx_inflater *inf = nullptr;
    if (!bgzf_member_at(map, size, xlen) || mcx_inflater_create(device, 0, 0, 0, &inf) != 0) { munmap(mm, size); return -1; }
    const uint64_t stretch = 8u << 20;
    std::vector<mcx_deflate_member> members;
    std::vector<uint8_t> text;
    int64_t total = 0;
    bool bad = false;
    for (size_t o = 0; o < size && !bad;) {
        members.clear();
        uint64_t bytes = 0;
        bool last = false;
        while (o < size) {
            const uint8_t *p = map + o;
            const size_t msize = bgzf_member_at(p, size - o, xlen);
            if (!msize) { last = true; break; }
            const uint32_t isize = (uint32_t)p[msize - 4] | ((uint32_t)p[msize - 3] << 8) | ((uint32_t)p[msize - 2] << 16) | ((uint32_t)p[msize - 1] << 24);
            const uint32_t crc = (uint32_t)p[msize - 8] | ((uint32_t)p[msize - 7] << 8) | ((uint32_t)p[msize - 6] << 16) | ((uint32_t)p[msize - 5] << 24);
            if (isize > 65536) { last = true; break; }
            if (bytes + isize > stretch) break;
            if (isize) {
                mcx_deflate_member m; memset(&m, 0, sizeof m);
                m.src_off = o + 12 + xlen; m.dst_off = bytes; m.src_len = (uint32_t)(msize - 12 - xlen - 8); m.isize = isize; m.crc32 = crc;
                members.push_back(m);
            }
            bytes += isize; o += msize;
        }
        if (bytes) {
            const bool fits = out && (uint64_t)total + bytes <= cap;
            if (!fits) text.resize(bytes);
            uint8_t *dst = fits ? out + total : text.data();
            if (mcx_inflate(inf, map, size, members.data(), (uint32_t)members.size(), dst, bytes, nullptr) != 0) bad = true;
            else {
                if (!fits && out && (uint64_t)total < cap) memcpy(out + total, dst, (size_t)(cap - (uint64_t)total));
                total += (int64_t)bytes;
            }
        }
        if (last) break;
    }
    if (n_out) *n_out = (uint64_t)total;
    mcx_inflater_free(inf);
    munmap(mm, size);
    return bad ? -2 : total;
}
