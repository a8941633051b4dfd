// mapcaller_amd/csrc/mcx_resident.hip — the file front end's resident route (-gpu_inflate -gpu_parse on BGZF FASTQ; -gpu_gz -gpu_parse on ordinary .gz): read files whose text stays in HBM from
// the compressed bytes to the batch's 2-bit rows (mcx_resident_open / _next / _close, mcx_resident_bufs_free; reached from mcx_files.cpp's reader thread alone).
//
// Replaces, for such files, Parser::feed_bgzf + Parser::entry + pack_row of mcx_files.cpp — whose rules it keeps: the members are walked into stretches of at
// most 8 MB of text exactly as feed_bgzf walks them, a stretch with a damaged member is not handed on and ends the input, what is no member ends it too; the
// records are the GZ rule's (mcx_fastq.h).  It launches no kernel of its own: per file an inflater without text buffers (mcx_inflate_begin_dev: several stretches
// per launch, the text left in the file's buffer in HBM), one mcx_fastq_parser under the GZ rule for both files, and device-to-device copies on a stream of its own
// that carry text[consumed ..) in front of the next text when the buffer's end is reached.
//   a batch   per file: count the records in what the buffer holds (final = 0 while members follow); fewer than wanted and the file goes on: one more launch,
//             count again.  Then one call for both files over text[0 .. consumed) with final = 1 — the same pieces, so the same records — that writes rows,
//             lengths and odd bytes (and names, their offsets and NUL-padded qualities for the SAM kernels) into the batch object's device buffers.
// FASTA: BGZF files whose text does not begin with '@' go the same way under GZ-rule FASTA (records of two pieces, no qualities: the SAM kernels get none).
// PLAIN FASTA under -gpu_parse alone (mcx_resident_open_plain): the same object over plain files — `more` sends the next bytes of the mapped file to HBM instead
// of inflating members, the parser runs under plain-rule FASTA, and the batch's arrays come back to host buffers (mcx_resident_host_out): the counting, the carry
// and the ends of the input are this file's for both.
// ORDINARY .gz under -gpu_gz -gpu_parse: a third kind of File — `more` runs one round of the file's gzip stream through mcx_gz_file_next / _text (mcx_gz_dev.hip: members,
// trailers and staging are that file's), making room between the two halves, and the text lands behind `have`; the parser runs under the GZ rule as for BGZF.  The
// first round is run by mcx_resident_open: a chain of fewer than half of its stretches, and the route does not apply to the call.
// BAM (one BGZF file whose text begins "BAM\1", whatever its name): the walker, the staging, the launches, the carry and ensure_room are the BGZF file's.  Behind the
// first launch the header is walked on the host (mcx_bam_reads_header over the text's first bytes, more launches while it asks for them) and `start` moves to the
// first record; the parser runs under MCX_READS_BAM (mcx_bam_in.hip), and the first taken record's flag decides the library: 0x1 set — pairs, the parser counts
// mates and a batch takes an even number of records —, else single reads.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/mcx.h"
#include "mcx_fastq.h"
#include "mcx_bam_in.h"
#include "mcx_internal.h"
// (mcx_gz_file_*: an ordinary .gz file's rounds, mcx_gz_dev.hip)

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mcx_set_error(MCX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace {

enum : uint64_t { kStretch = 8ull << 20 }; // the host route's stretch (Parser::kBlockBytes): what a damaged member takes with it

struct DBuf { void *p = nullptr; uint64_t cap = 0; };

// room for `need` bytes; what the buffer held is gone
int dgrow(DBuf &b, uint64_t need, const char *what)
{
    if (need <= b.cap) return 0;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    const uint64_t cap = need + need / 8 + 4096;
    if (hipMalloc(&b.p, cap) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return mcx_set_error(MCX_ERR_DEVICE, std::string("-gpu_inflate -gpu_parse: no room in HBM for ") + what + " (" + std::to_string(cap >> 20) + " MB): map with a smaller -batch");
    }
    b.cap = cap;
    static const bool log = getenv("MCX_ALLOC_LOG") != nullptr;
    if (log) fprintf(stderr, "[mcx alloc] %8.3f GB resident route: %s\n", (double)cap / 1e9, what);
    return 0;
}

struct File {
    const uint8_t *map = nullptr; size_t size = 0;
    size_t o = 0;            // the walk's place in the file
    bool walk_end = false;   // no member follows: the file's end, something that is no member, or a damaged stretch
    bool eof = false;        // ... and everything before that is in the text
    bool plain = false;      // a plain file: its bytes are the text
    mcx_gz_file *gz = nullptr; // an ordinary gzip stream (-gpu_gz): its rounds go through a gunzipper of the file's own (mcx_gz_dev.hip)
    uint32_t gz_rounds = 0;  // ... rounds run so far
    bool gz_taken = false;   // ... the route applies to the call (mcx_resident_open has returned the object)
    bool gz_uncut = false;   // ... its first round's chain holds fewer than half of its stretches: the route does not apply
    std::string path;
    uint64_t ask = 0;        // (plain) bytes the next `more` should bring, when more than a launch: what the batch in hand still lacks, by its records so far
    mcx_inflater *inf = nullptr;
    DBuf text[2]; int cur = 0;       // the file's text in HBM: text[cur][start .. have) is not consumed yet
    uint64_t start = 0, have = 0;
    std::vector<mcx_deflate_member> members; // of the stretches of one call of more()
    std::vector<uint32_t> stretch_of, status;
    std::vector<uint64_t> stretch_at;        // where each of those stretches begins in the call's text; the last entry: its end
};

} // namespace

struct mcx_resident {
    int device = 0, n_files = 0;
    hipStream_t stream = nullptr;
    File f[2];
    mcx_fastq_parser *parser = nullptr;
    DBuf bases, off;         // outputs of the parser that nobody reads (the qualities come in a group with them)
    uint64_t launch_bytes = 0, max_src = 0;
    uint32_t max_members = 0;
    bool fixed_launch = false;         // MCX_RESIDENT_LAUNCH_BYTES is set: every launch is that long
    bool fasta = false, plain = false; // FASTA text (no qualities); plain files (the results go back to the host)
    bool bam = false, bam_paired = false, bam_damaged_said = false; // a BAM file; its first taken record has flag 0x1: pairs; the line about its damage is out
    int32_t n_ref = 0;                 // ... the n_ref of its header
    uint64_t delivered = 0;            // ... reads handed out so far
    mcx_fastq_info all;                // (plain) the last batch's combined call, for mcx_resident_host_out
};
struct mcx_resident_bufs {
    int device = 0;
    DBuf rows, len, odd, qual, names, name_off;
};

namespace {

// room for `need` more bytes behind the text: what is not consumed moves to the front of the file's other buffer (device to device), which grows if it must
int ensure_room(mcx_resident *R, File &f, uint64_t need)
{
    if (f.have + need <= f.text[f.cur].cap) return 0;
    const uint64_t live = f.have - f.start;
    DBuf &to = f.text[f.cur ^ 1];
    if (int rc = dgrow(to, live + need + 64, "a read file's text")) return rc;
    if (live) {
        HIP_TRY(hipMemcpyAsync(to.p, (const uint8_t *)f.text[f.cur].p + f.start, live, hipMemcpyDeviceToDevice, R->stream));
        HIP_TRY(hipStreamSynchronize(R->stream));
    }
    f.cur ^= 1; f.start = 0; f.have = live;
    return 0;
}

// More text behind what the file's buffer holds: the next stretches — as many whole ones as a launch takes, one at least — inflated, checked, and handed on
// up to the first stretch with a damaged member.  Either the text grows or the file is at its end.
int more(mcx_resident *R, File &f)
{
    if (f.walk_end) { f.eof = true; return 0; }
    if (f.gz) { // the next round(s) of the gzip stream: the text grows behind `have`, or the stream is at its end
        for (;;) {
            mcx_gz_round info;
            const int r = mcx_gz_file_next(f.gz, &info);
            if (r < 0) return r;
            bool counts = false;
            if (r > 0) {
                if (f.gz_rounds++ == 0 && (info.stretches < 2 || info.chain * 2 < info.stretches)) { f.gz_uncut = true; f.walk_end = f.eof = true; return 0; }
                if (int rc = ensure_room(R, f, info.text_bytes + 64)) return rc;
                if (int rc = mcx_gz_file_text(f.gz, (uint8_t *)f.text[f.cur].p + f.have, f.text[f.cur].cap - f.have, &info, &counts)) return rc;
            }
            if (!counts) { // the input's end, or a round that is not handed on: a damaged stream, a trailer that does not match
                if (mcx_gz_file_failed(f.gz) && f.gz_taken) // (while the files are opened the route is not taken yet: a first round that fails leaves the call, and the word, to the host reader)
                    fprintf(stderr, "[mcx_map_files] -gpu_gz: %s: the gzip stream is damaged or ends early; the file's input ends behind %llu bytes of text\n", f.path.c_str(), (unsigned long long)mcx_gz_file_delivered(f.gz));
                f.walk_end = f.eof = true;
                return 0;
            }
            f.have += info.text_bytes;
            if (info.text_bytes) return 0;
        }
    }
    if (f.plain) { // the next bytes of the file, as they are
        const uint64_t n = std::min<uint64_t>(std::max(R->launch_bytes, f.ask), f.size - f.o);
        if (n) {
            if (int rc = ensure_room(R, f, n)) return rc;
            HIP_TRY(hipMemcpyAsync((uint8_t *)f.text[f.cur].p + f.have, f.map + f.o, n, hipMemcpyHostToDevice, R->stream));
            HIP_TRY(hipStreamSynchronize(R->stream));
            f.have += n; f.o += n;
        }
        f.walk_end = f.eof = f.o >= f.size;
        return 0;
    }
    f.members.clear(); f.stretch_of.clear(); f.stretch_at.assign(1, 0);
    uint64_t total = 0;
    while (!f.walk_end) {
        uint64_t st = 0; // one stretch, as Parser::feed_bgzf's walk cuts it
        bool last = false;
        while (f.o < f.size) {
            size_t xlen = 0;
            const uint8_t *p = f.map + f.o;
            const size_t size = mcx_bgzf_member_at(p, f.size - f.o, xlen);
            if (!size) { last = true; break; }
            const uint32_t isize = (uint32_t)p[size - 4] | ((uint32_t)p[size - 3] << 8) | ((uint32_t)p[size - 2] << 16) | ((uint32_t)p[size - 1] << 24);
            const uint32_t crc = (uint32_t)p[size - 8] | ((uint32_t)p[size - 7] << 8) | ((uint32_t)p[size - 6] << 16) | ((uint32_t)p[size - 5] << 24);
            if (isize > 65536) { last = true; break; }
            if (st + isize > kStretch) break;
            if (isize) { // (not the empty member that ends a BGZF file)
                mcx_deflate_member m; memset(&m, 0, sizeof m);
                m.src_off = f.o + 12 + xlen; m.dst_off = total + st; m.src_len = (uint32_t)(size - 12 - xlen - 8); m.isize = isize; m.crc32 = crc;
                f.members.push_back(m);
                f.stretch_of.push_back((uint32_t)f.stretch_at.size() - 1);
            }
            st += isize; f.o += size;
        }
        if (last || f.o >= f.size) f.walk_end = true; // (what follows is not a BGZF member: the input ends there, as it does where gzread gives up)
        if (st) { total += st; f.stretch_at.push_back(total); } // (else: empty members in the middle of a file)
        if (total && total + kStretch > R->launch_bytes) break;
    }
    if (total == 0) { f.eof = true; return 0; }
    if (int rc = ensure_room(R, f, total)) return rc;
    const size_t n = f.members.size();
    for (mcx_deflate_member &m : f.members) m.dst_off += f.have;
    f.status.assign(n, 0);
    uint8_t *dst = (uint8_t *)f.text[f.cur].p;
    const uint64_t cap = f.text[f.cur].cap;
    std::deque<std::pair<size_t, size_t>> flying; // launches on the device: their members [first, second)
    size_t at = 0, bad_from = n;
    int rc = 0;
    while ((at < n && bad_from == n) || !flying.empty()) {
        if (at < n && bad_from == n && flying.size() < 2) { // (the next launch's bytes are staged while this one's are on the device)
            size_t k = at;
            uint64_t so = 0, to = 0;
            while (k < n && k - at < R->max_members && so + f.members[k].src_len <= R->max_src && (k == at || to + f.members[k].isize <= R->launch_bytes)) { so += f.members[k].src_len; to += f.members[k].isize; k++; }
            if (k == at || mcx_inflate_begin_dev(f.inf, f.map, f.size, f.members.data() + at, (uint32_t)(k - at), dst, cap) != 0) {
                fprintf(stderr, "[mcx_map_files] -gpu_inflate: %s\n", k == at ? "a member larger than a launch holds" : mcx_last_error());
                bad_from = at; // (the input ends here)
                continue;
            }
            flying.push_back(std::make_pair(at, k));
            at = k;
            continue;
        }
        const std::pair<size_t, size_t> l = flying.front();
        flying.pop_front();
        const int e = mcx_inflate_end(f.inf, nullptr, f.status.data() + l.first, nullptr);
        if (e && e != MCX_ERR_IO && rc == 0) rc = e;
    }
    if (rc) return rc;
    for (size_t i = 0; i < n && i < bad_from; i++) if (f.status[i]) { bad_from = i; break; }
    uint64_t good = total;
    if (bad_from < n) { good = f.stretch_at[f.stretch_of[bad_from]]; f.walk_end = true; } // (a damaged stretch is not handed on; the stretches before it count)
    f.have += good;
    f.eof = f.walk_end;
    return 0;
}

int count(mcx_resident *R, const File &f, uint32_t max_records, int32_t max_read_len, mcx_fastq_info *info)
{
    mcx_fastq_in in;
    memset(&in, 0, sizeof in);
    in.bytes[0] = f.have - f.start;
    in.text[0] = in.bytes[0] ? (const uint8_t *)f.text[f.cur].p + f.start : nullptr;
    in.max_records = max_records; in.max_read_len = max_read_len; in.final = f.eof ? 1 : 0; in.n_ref = R->n_ref;
    return mcx_fastq_dev_sizes(R->parser, &in, info);
}

enum : uint64_t { kBamHeaderMost = 256ull << 20 };

// BAM: the header behind the first launch — the text's first bytes on the host, more launches while they hold too little of it; `start` moves to the first record
int bam_header(mcx_resident *R, File &f)
{
    std::vector<uint8_t> h;
    for (uint64_t want = 65536;;) {
        const uint64_t live = f.have - f.start, n = std::min(live, want);
        h.resize(n);
        if (n) HIP_TRY(hipMemcpy(h.data(), (const uint8_t *)f.text[f.cur].p + f.start, n, hipMemcpyDeviceToHost));
        uint64_t at = 0;
        int32_t n_ref = 0;
        const int rc = mcx_bam_reads_header(h.data(), n, &at, &n_ref);
        if (rc == 0) { f.start += at; R->n_ref = n_ref; return 0; }
        if (rc < 0) return mcx_set_error(MCX_ERR_IO, f.path + ": the BAM header is damaged");
        if (n < live) { want = live; continue; } // (more of it is in HBM already)
        if (live > kBamHeaderMost) return mcx_set_error(MCX_ERR_UNSUPPORTED, f.path + ": a BAM header of more than 256 MB is not read");
        if (f.eof) return mcx_set_error(MCX_ERR_IO, f.path + ": the BAM header is cut short");
        if (int e = more(R, f)) return e;
        want = f.have - f.start;
    }
}

// BAM: pairs or single reads — the flag of the first taken record, from as many launches as it takes to reach one
int bam_library(mcx_resident *R, File &f)
{
    for (;;) {
        mcx_fastq_info info;
        if (int rc = count(R, f, 1, 0x7FFFFFFF, &info)) return rc;
        uint64_t st[6];
        if (int rc = mcx_bam_reads_last(R->parser, st)) return rc;
        if (st[1]) { R->bam_paired = (st[3] & 1u) != 0; return 0; }
        if (f.eof || info.stop[0] != MCX_FASTQ_MORE) return 0; // no taken record at all: nothing will be mapped
        if (int rc = more(R, f)) return rc;
    }
}

} // namespace

void mcx_resident_close(mcx_resident *R)
{
    if (!R) return;
    (void)hipSetDevice(R->device);
    if (R->parser) mcx_fastq_parser_free(R->parser);
    for (File &f : R->f) {
        if (f.inf) mcx_inflater_free(f.inf); // (waits for what is still on the device)
        if (f.gz) mcx_gz_file_free(f.gz);
        for (DBuf &b : f.text) if (b.p) (void)hipFree(b.p);
        if (f.map) munmap((void *)f.map, f.size);
    }
    if (R->bases.p) (void)hipFree(R->bases.p);
    if (R->off.p) (void)hipFree(R->off.p);
    if (R->stream) (void)hipStreamDestroy(R->stream);
    delete R;
}

void mcx_resident_bufs_free(mcx_resident_bufs *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    DBuf *all[] = {&b->rows, &b->len, &b->odd, &b->qual, &b->names, &b->name_off};
    for (DBuf *d : all) if (d->p) (void)hipFree(d->p);
    delete b;
}

uint32_t mcx_resident_inflate_bit(const mcx_resident *R, int f) { return R->f[f].gz ? (uint32_t)MCX_ROUTE_GZ : (uint32_t)MCX_ROUTE_INFLATE; }

bool mcx_resident_bam(const mcx_resident *R) { return R->bam; }
bool mcx_resident_bam_paired(const mcx_resident *R) { return R->bam_paired; }

int mcx_resident_open(int device, const char *const paths[2], int n_files, uint32_t kinds, bool bam, mcx_resident **out)
{
    *out = nullptr;
    mcx_resident *R = new mcx_resident();
    R->device = device; R->n_files = n_files; R->bam = bam;
    bool applies = true, is_gz[2] = {false, false};
    for (int i = 0; i < n_files && applies; i++) {
        const std::string path(paths[i]);
        File &f = R->f[i];
        applies = bam || (path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0); // (the .gz readers' rule goes with the name, ReadMapping.cpp:709; a BAM file is one whatever its name)
        const int fd = applies ? ::open(paths[i], O_RDONLY) : -1;
        if (fd < 0) { applies = false; break; }
        struct stat st;
        applies = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size >= 28;
        if (applies) {
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) applies = false; else { f.map = (const uint8_t *)m; f.size = (size_t)st.st_size; }
        }
        close(fd);
        size_t xlen = 0;
        if (!applies) break;
        f.path = path;
        is_gz[i] = mcx_bgzf_member_at(f.map, f.size, xlen) == 0; // not BGZF: an ordinary gzip stream, or nothing of the kind (mcx_gz_file_open says which)
        applies = (kinds & (is_gz[i] ? MCX_INFLATE_GZ : MCX_INFLATE_BGZF)) != 0;
    }
    if (!applies) { mcx_resident_close(R); return 0; }
    const char *env = getenv("MCX_RESIDENT_LAUNCH_BYTES");
    R->launch_bytes = env && atoll(env) > 0 ? (uint64_t)atoll(env) : (128ull << 20);
    R->max_src = std::max<uint64_t>(R->launch_bytes / 2, 65536 + 1024) + 4096; // (text that does not shrink to half takes more launches)
    R->max_members = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(R->launch_bytes / 1024, 64), 1u << 18);
    int rc = 0;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&R->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); rc = mcx_set_error(MCX_ERR_DEVICE, "-gpu_inflate -gpu_parse: no stream on the context's device"); }
    const char *gz_s = getenv("MCX_GZ_STRETCH"), *gz_n = getenv("MCX_GZ_ROUND_STRETCHES");
    for (int i = 0; i < n_files && rc == 0 && applies; i++) {
        if (!is_gz[i]) { rc = mcx_inflater_create_dev(device, R->max_src, R->max_members, &R->f[i].inf); continue; }
        rc = mcx_gz_file_open(device, R->f[i].map, R->f[i].size, gz_s && atoll(gz_s) > 0 ? (uint64_t)atoll(gz_s) : 0, gz_n && atoll(gz_n) > 0 ? (uint32_t)atoll(gz_n) : 512, &R->f[i].gz);
        if (rc == 0 && !R->f[i].gz) applies = false; // (no gzip header)
    }
    if (rc == 0) rc = mcx_fastq_parser_create(device, 0, 0, &R->parser);
    if (rc == 0) rc = mcx_fastq_parser_set_rule(R->parser, MCX_FASTQ_RULE_GZ);
    // What the host reader judges FASTQ or FASTA by is the first byte of the first stretch it is handed ('@': FASTQ, CheckReadFormat, GetData.cpp:22-31): a first
    // stretch that is damaged hands it none.  The same here, from HBM; a file without text, and files of two formats, are left to that reader.
    bool fastq[2] = {true, true};
    for (int i = 0; i < n_files && rc == 0 && applies; i++) {
        File &f = R->f[i];
        while (rc == 0 && f.have == 0 && !f.eof) rc = more(R, f);
        uint8_t first = 0;
        if (rc == 0 && f.have && hipMemcpy(&first, f.text[f.cur].p, 1, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); rc = mcx_set_error(MCX_ERR_DEVICE, "-gpu_inflate -gpu_parse: copy from the device failed"); }
        applies = f.have != 0 && !f.gz_uncut;
        fastq[i] = first == '@' || bam;
    }
    if (n_files == 2 && fastq[0] != fastq[1]) applies = false;
    R->fasta = !fastq[0];
    if (rc == 0 && applies && R->fasta) rc = mcx_fastq_parser_set_format(R->parser, MCX_READS_FASTA);
    if (rc == 0 && bam) {
        if (!applies || n_files != 1 || R->f[0].gz) rc = mcx_set_error(MCX_ERR_IO, std::string(paths[0]) + ": the BAM file holds no text that can be inflated");
        if (rc == 0) rc = bam_header(R, R->f[0]);
        if (rc == 0) rc = mcx_fastq_parser_set_reads(R->parser, MCX_READS_BAM);
        if (rc == 0) rc = bam_library(R, R->f[0]);
        if (rc == 0 && R->bam_paired) rc = mcx_fastq_parser_set_mates(R->parser, 1);
    }
    if (rc || !applies) { mcx_resident_close(R); return rc; }
    for (File &f : R->f) f.gz_taken = true;
    *out = R;
    return 0;
}

// plain FASTA files (-gpu_parse): *out stays null when a file cannot be mapped — the caller's reader then says why
int mcx_resident_open_plain(int device, const char *const paths[2], int n_files, mcx_resident **out)
{
    *out = nullptr;
    mcx_resident *R = new mcx_resident();
    R->device = device; R->n_files = n_files; R->fasta = R->plain = true;
    bool applies = true;
    for (int i = 0; i < n_files && applies; i++) {
        File &f = R->f[i];
        f.plain = true;
        const int fd = ::open(paths[i], O_RDONLY);
        if (fd < 0) { applies = false; break; }
        struct stat st;
        applies = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0;
        if (applies) {
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) applies = false; else { f.map = (const uint8_t *)m; f.size = (size_t)st.st_size; }
        }
        close(fd);
    }
    if (!applies) { mcx_resident_close(R); return 0; }
    const char *env = getenv("MCX_RESIDENT_LAUNCH_BYTES");
    R->launch_bytes = env && atoll(env) > 0 ? (uint64_t)atoll(env) : (1ull << 20); // bytes of a file that go to HBM at a time, at least (every count walks all the text in hand: a batch asks for what it lacks)
    R->fixed_launch = env && atoll(env) > 0;
    int rc = 0;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&R->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); rc = mcx_set_error(MCX_ERR_DEVICE, "-gpu_parse: no stream on the context's device"); }
    if (rc == 0) rc = mcx_fastq_parser_create(device, 0, 0, &R->parser);
    if (rc == 0) rc = mcx_fastq_parser_set_format(R->parser, MCX_READS_FASTA);
    if (rc) { mcx_resident_close(R); return rc; }
    *out = R;
    return 0;
}

bool mcx_resident_fasta(const mcx_resident *R) { return R->fasta; }

// (plain) groups of the last batch into HOST buffers (mcx_fastq_staged_out: row_words 0 gives rows ceil(longest / 16) words wide)
int mcx_resident_host_out(mcx_resident *R, const mcx_fastq_out *out)
{
    return mcx_fastq_staged_out(R->parser, out, &R->all);
}

int mcx_resident_next(mcx_resident *R, mcx_resident_bufs **bufs, uint32_t per_file, int32_t max_read_len, bool want_sam, mcx_resident_batch *out)
{
    memset(out, 0, sizeof *out);
    HIP_TRY(hipSetDevice(R->device));
    const int nf = R->n_files;
    mcx_fastq_info info[2];
    for (int i = 0; i < nf; i++) {
        File &f = R->f[i];
        for (;;) {
            if (int rc = count(R, f, per_file, max_read_len, &info[i])) return rc;
            if (info[i].n_records[0] >= per_file || f.eof || info[i].stop[0] != MCX_FASTQ_MORE) break; // (a stop inside whole records stands whatever follows)
            // (plain: every count walks the whole text in hand, so the next bytes are as many as the batch still lacks, judged by its records so far)
            const uint64_t got = info[i].n_records[0], in_hand = f.have - f.start;
            f.ask = f.plain && !R->fixed_launch ? (got ? (uint64_t)((double)info[i].consumed[0] / (double)got * 1.05 * (double)(per_file - got)) + 65536 : 2 * in_hand) : 0;
            if (int rc = more(R, f)) return rc;
        }
        out->n_records[i] = info[i].n_records[0];
        out->last[i] = info[i].n_records[0] < per_file;
        if (R->bam && info[i].stop[0] == MCX_FASTQ_UNPAIRED)
            return mcx_set_error(MCX_ERR_ARG, f.path + ": the BAM file's mates are not neighbours (behind " + std::to_string(R->delivered + info[i].n_records[0]) +
                                                  " reads): collate it or sort it by name first (samtools collate, samtools sort -n)");
        if (R->bam && info[i].stop[0] == MCX_FASTQ_DAMAGED && !R->bam_damaged_said) {
            R->bam_damaged_said = true;
            fprintf(stderr, "[mcx_map_files] %s: a damaged BAM record, or one cut short; the file's input ends behind %llu reads\n", f.path.c_str(), (unsigned long long)(R->delivered + info[i].n_records[0]));
        }
        if (R->bam && out->last[i] && info[i].stop[0] == MCX_FASTQ_TOO_LONG) { // its name, from the record at the first byte that was not taken
            uint8_t head[mcx::bamin::kFixed + 256];
            const uint64_t at = f.start + info[i].consumed[0];
            const uint32_t len = (uint32_t)std::min<uint64_t>(sizeof head, f.have - at);
            HIP_TRY(hipMemcpy(head, (const uint8_t *)f.text[f.cur].p + at, len, hipMemcpyDeviceToHost));
            const uint32_t lrn = len > mcx::bamin::kFixed ? std::min<uint32_t>(head[12], len - mcx::bamin::kFixed) : 0;
            uint32_t p1 = 1, p2 = 1;
            if (lrn) mcx::bamin::name_span(head + mcx::bamin::kFixed, lrn, p1, p2);
            const uint32_t name_len = p2 > p1 ? std::min<uint32_t>(p2 - p1, sizeof out->too_long[i] - 1) : 0;
            memcpy(out->too_long[i], head + mcx::bamin::kFixed + p1 - 1, name_len);
            out->too_long[i][name_len] = 0;
            out->has_too_long[i] = true;
        } else
        if (out->last[i] && info[i].stop[0] == MCX_FASTQ_TOO_LONG) { // its name, from the header piece at the first byte that was not taken
            uint8_t piece[mcx::fq::kGzPiece];
            const uint64_t at = f.start + info[i].consumed[0];
            uint32_t len = (uint32_t)std::min<uint64_t>(mcx::fq::kGzPiece, f.have - at);
            HIP_TRY(hipMemcpy(piece, (const uint8_t *)f.text[f.cur].p + at, len, hipMemcpyDeviceToHost));
            if (const void *nl = memchr(piece, '\n', len)) len = (uint32_t)((const uint8_t *)nl - piece) + 1;
            if (!R->plain) len = (uint32_t)strnlen((const char *)piece, len); // (a plain line is not a C string; its name ends within the first 100 bytes either way)
            uint32_t p1 = 0, p2 = 0;
            if (len) mcx::fq::header_of(piece, len, p1, p2);
            const uint32_t name_len = p2 > p1 ? std::min<uint32_t>(p2 - p1, sizeof out->too_long[i] - 1) : 0;
            memcpy(out->too_long[i], piece + p1, name_len);
            out->too_long[i][name_len] = 0;
            out->has_too_long[i] = true;
        }
    }
    const bool too_long = out->has_too_long[0] || out->has_too_long[1];
    const uint32_t n_take = out->n_records[0];
    if (too_long || n_take == 0 || (nf == 2 && out->n_records[1] < n_take)) return 0; // (nothing of such a batch is mapped: the caller ends the run, or the input)
    // where the n_take records of each file end: a file that holds more of them keeps the rest for the next batch
    uint64_t consumed[2] = {0, 0};
    for (int i = 0; i < nf; i++) {
        consumed[i] = info[i].consumed[0];
        if (info[i].n_records[0] == n_take) continue;
        mcx_fastq_info fewer;
        if (int rc = count(R, R->f[i], n_take, max_read_len, &fewer)) return rc;
        if (fewer.n_records[0] != n_take) return mcx_set_error(MCX_ERR_DEVICE, "-gpu_parse: two counts of one text disagree");
        consumed[i] = fewer.consumed[0];
    }
    // the batch: both files' text up to there as whole texts (final) — the same pieces, so the same records, read 2i from file 1 and read 2i + 1 from file 2
    mcx_fastq_in in;
    memset(&in, 0, sizeof in);
    for (int i = 0; i < nf; i++) { const File &f = R->f[i]; in.text[i] = (const uint8_t *)f.text[f.cur].p + f.start; in.bytes[i] = consumed[i]; }
    in.max_records = n_take; in.max_read_len = max_read_len; in.final = 1; in.n_ref = R->n_ref;
    mcx_fastq_info all;
    if (int rc = mcx_fastq_dev_sizes(R->parser, &in, &all)) return rc;
    const uint32_t n = (uint32_t)nf * n_take;
    if (all.n_reads != n) return mcx_set_error(MCX_ERR_DEVICE, "-gpu_parse: the device counted " + std::to_string(all.n_reads) + " reads where " + std::to_string(n) + " were counted before");
    if (R->plain) { // the caller fetches what it needs into host buffers: the text stays where it is until the next batch is asked for
        R->all = all;
        for (int i = 0; i < nf; i++) R->f[i].start += consumed[i];
        out->n_reads = n; out->n_odd = all.n_odd; out->longest = all.longest; out->n_bases = all.n_bases; out->n_name_bytes = all.n_name_bytes;
        return 0;
    }
    if (!*bufs) { *bufs = new mcx_resident_bufs(); (*bufs)->device = R->device; }
    mcx_resident_bufs &b = **bufs;
    const uint32_t row_words = ((uint32_t)max_read_len + 15) / 16;
    int rc;
    if ((rc = dgrow(b.rows, (uint64_t)n * row_words * 4 + 16, "a batch's 2-bit rows")) || (rc = dgrow(b.len, (uint64_t)n * 4 + 16, "a batch's read lengths")) ||
        (rc = dgrow(b.odd, (uint64_t)all.n_odd * 8 + 16, "a batch's bytes that are not ACGT"))) return rc;
    mcx_fastq_out o;
    memset(&o, 0, sizeof o);
    o.rows = (uint32_t *)b.rows.p; o.row_words = row_words; o.len = (uint32_t *)b.len.p; o.odd = (uint64_t *)b.odd.p; o.odd_cap = all.n_odd;
    if (want_sam) {
        if ((rc = dgrow(b.names, all.n_name_bytes + 16, "a batch's read names")) || (rc = dgrow(b.name_off, ((uint64_t)n + 1) * 4, "a batch's name offsets"))) return rc;
        if (!R->fasta) { // (FASTA: no qualities — the SAM kernels write '*' for a null pointer)
            if ((rc = dgrow(R->bases, all.n_bases + 48, "the parser's bases")) || (rc = dgrow(R->off, ((uint64_t)n + 1) * 4, "the parser's offsets")) || (rc = dgrow(b.qual, all.n_bases + 48, "a batch's qualities"))) return rc;
            o.bases = (uint8_t *)R->bases.p; o.off = (uint32_t *)R->off.p; o.qual = (uint8_t *)b.qual.p; o.bases_cap = all.n_bases + 32;
        }
        o.names = (uint8_t *)b.names.p; o.name_off = (uint32_t *)b.name_off.p; o.names_cap = all.n_name_bytes;
    }
    if ((rc = mcx_fastq_dev_out(R->parser, &o, &all))) return rc;
    for (int i = 0; i < nf; i++) R->f[i].start += consumed[i];
    R->delivered += n;
    out->n_reads = n; out->rows = o.rows; out->len = o.len; out->odd = o.odd; out->row_words = row_words; out->n_odd = all.n_odd; out->longest = all.longest;
    out->names = o.names; out->qual = o.qual; out->name_off = o.name_off;
    return 0;
}
