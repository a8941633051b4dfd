// mapcaller_amd/csrc/mcx_reader.h — the file front end's input side (host only): a read as the formatter needs it (Rec, View), the header and line rules,
// the 2-bit packer, and the two readers: MappedFastq (a plain FASTQ file in memory, indexed by line count, parsed by a pool from any record on) and Parser
// (the sequential reader: .gz through the parallel inflater, BGZF on the host or the device, zlib's one thread, FASTA with multi-line records).
// Text semantics follow the reference byte for byte: see mcx_files.cpp.
#pragma once
#include <cstdio>
#include <cstring>
#include <string>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include <immintrin.h>
#include "mcx_pool.h"
#include "mcx_pgz.h"
#include "mcx_internal.h"
#include "mcx_cpus.h"

namespace mcx { namespace files {

// ---- input -------------------------------------------------------------------------------------------
// One read as the formatter needs it: where its name, bases and qualities lie (offsets from View::base — the mapped file,
// or the batch's own copy for .gz / FASTA input).
struct Rec {
    uint64_t name, seq, qual;
    uint32_t rlen, q_take;  // q_take: bytes of the quality line that count (min(line, rlen), GetData.cpp:51-52; printed up to a NUL)
    uint32_t name_len;
};
// the records of a View: plain memory that is not cleared when it is handed out (a batch object's 40 MB of them would be written twice)
class RecBuf {
public:
    RecBuf() {}
    RecBuf(const RecBuf &) = delete;
    RecBuf &operator=(const RecBuf &) = delete;
    ~RecBuf() { free(p_); }
    size_t size() const { return n_; }
    void clear() { n_ = 0; }
    bool reserve(size_t n) { if (n > cap_) { Rec *q = (Rec *)realloc(p_, n * sizeof(Rec)); if (!q) return false; p_ = q; cap_ = n; } return true; }
    bool resize(size_t n) { if (!reserve(n)) return false; n_ = n; return true; } // (new entries are the caller's to write)
    bool push_back(const Rec &r) { if (n_ == cap_ && !reserve(cap_ ? cap_ * 2 : 4096)) return false; p_[n_++] = r; return true; } // false: out of memory — the caller says so (a record dropped in silence would shift mate 1 against mate 2)
    Rec &operator[](size_t i) { return p_[i]; }
    const Rec &operator[](size_t i) const { return p_[i]; }
    Rec *data() { return p_; }
    const Rec *begin() const { return p_; }
    const Rec *end() const { return p_ + n_; }
private:
    Rec *p_ = nullptr; size_t n_ = 0, cap_ = 0;
};
struct View { // the reads of one file for one batch
    const char *base = nullptr;
    RecBuf recs;
    std::vector<char> own;  // .gz / FASTA: the batch's copy of names, bases, qualities
    bool last = false;      // the file ended (or delivered an empty read) after these
    std::string error;
    uint32_t n() const { return (uint32_t)recs.size(); }
    void clear() { recs.clear(); own.clear(); last = false; error.clear(); base = nullptr; }
};

// IdentifyHeaderBegPos / IdentifyHeaderEndPos, GetData.cpp:3-20
inline void header_of(const char *l, int len, int &p1, int &p2)
{
    const int lim = len > 100 ? 100 : len;
    p1 = len - 1; p2 = lim - 1;
    for (int i = 1; i < len; i++) if (l[i] != '>' && l[i] != '@') { p1 = i; break; }
    for (int i = 1; i < lim; i++) { const unsigned char c = (unsigned char)l[i]; if (c <= ' ' || c == '/' || c >= 0x7f) { p2 = i; break; } } // (' ', '/', or not printable: isprint in the C locale is 0x20..0x7e)
}

// 2-bit row for mcx_stream_submit_packed: sixteen bases to a word, the first on top; bytes that are not ACGT are listed
inline uint32_t pack_word(const uint8_t *seq, uint32_t i, uint32_t n, uint32_t read, std::vector<uint64_t> &odd) // bases [i, i + n), n <= 16
{
    static const struct Lut { uint8_t v[256]; Lut() { memset(v, 4, sizeof v); v['A'] = 0; v['C'] = 1; v['G'] = 2; v['T'] = 3; } } lut;
    uint32_t w = 0, bad = 0;
    for (uint32_t j = 0; j < n; j++) { const uint32_t c = lut.v[seq[i + j]]; bad |= c; w |= (c & 3u) << (30 - 2 * j); }
    if (bad & 4u) {
        w = 0;
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t c = lut.v[seq[i + j]];
            if (c > 3) odd.push_back(((uint64_t)read << 32) | ((uint64_t)(i + j) << 8) | seq[i + j]);
            else w |= c << (30 - 2 * j);
        }
    }
    return w;
}
inline void pack_row_plain(const uint8_t *seq, uint32_t rlen, uint32_t read, uint32_t *row, uint32_t row_words, std::vector<uint64_t> &odd)
{
    uint32_t k = 0;
    for (uint32_t i = 0; i < rlen; i += 16, k++) row[k] = pack_word(seq, i, rlen - i < 16 ? rlen - i : 16, read, odd);
    for (; k < row_words; k++) row[k] = 0;
}
// the same sixteen bases at a time: of A C G T, ((c >> 1) ^ (c >> 2)) & 3 is the code; the two-bit fields gathered by pext
__attribute__((target("sse2,bmi2"))) inline void pack_row_bmi2(const uint8_t *seq, uint32_t rlen, uint32_t read, uint32_t *row, uint32_t row_words, std::vector<uint64_t> &odd)
{
    const __m128i cA = _mm_set1_epi8('A'), cC = _mm_set1_epi8('C'), cG = _mm_set1_epi8('G'), cT = _mm_set1_epi8('T'), three = _mm_set1_epi8(3);
    uint32_t k = 0, i = 0;
    for (; i + 16 <= rlen; i += 16, k++) {
        const __m128i c = _mm_loadu_si128((const __m128i *)(seq + i));
        const __m128i known = _mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(c, cA), _mm_cmpeq_epi8(c, cC)), _mm_or_si128(_mm_cmpeq_epi8(c, cG), _mm_cmpeq_epi8(c, cT)));
        if (_mm_movemask_epi8(known) != 0xFFFF) { row[k] = pack_word(seq, i, 16, read, odd); continue; }
        const __m128i code = _mm_and_si128(_mm_xor_si128(_mm_srli_epi16(c, 1), _mm_srli_epi16(c, 2)), three); // (what the 16-bit shifts carry across bytes lands above bit 1)
        const uint64_t lo = (uint64_t)_mm_cvtsi128_si64(code), hi = (uint64_t)_mm_cvtsi128_si64(_mm_unpackhi_epi64(code, code));
        row[k] = ((uint32_t)_pext_u64(__builtin_bswap64(lo), 0x0303030303030303ull) << 16) | (uint32_t)_pext_u64(__builtin_bswap64(hi), 0x0303030303030303ull);
    }
    if (i < rlen) { row[k++] = pack_word(seq, i, rlen - i, read, odd); }
    for (; k < row_words; k++) row[k] = 0;
}
inline void pack_row(const uint8_t *seq, uint32_t rlen, uint32_t read, uint32_t *row, uint32_t row_words, std::vector<uint64_t> &odd)
{
    static const bool wide = __builtin_cpu_supports("bmi2") && !getenv("MCX_PLAIN_PACK");
    if (wide) pack_row_bmi2(seq, rlen, read, row, row_words, odd); else pack_row_plain(seq, rlen, read, row, row_words, odd);
}

// the next '\n' in [p, e), or nullptr: FASTQ lines are a few bytes to a few hundred, so sixteen bytes at a time from the first byte on (memchr's set-up costs more than the search)
inline const char *find_nl(const char *p, const char *e)
{
    const __m128i nl = _mm_set1_epi8('\n');
    while (p + 16 <= e) {
        const int m = _mm_movemask_epi8(_mm_cmpeq_epi8(_mm_loadu_si128((const __m128i *)p), nl));
        if (m) return p + __builtin_ctz((unsigned)m);
        p += 16;
    }
    for (; p < e; p++) if (*p == '\n') return p;
    return nullptr;
}

// A plain FASTQ file in memory, with the line count ahead of every 64 KB of it: record r begins at line 4 r.
class MappedFastq {
public:
    ~MappedFastq() { if (map_ && size_) munmap((void *)map_, size_); if (fd_ >= 0) close(fd_); }
    bool open(const std::string &path, std::string &err)
    {
        fd_ = ::open(path.c_str(), O_RDONLY);
        if (fd_ < 0) { err = "cannot open " + path; return false; }
        struct stat st;
        if (fstat(fd_, &st) != 0 || !S_ISREG(st.st_mode)) { err = "cannot map " + path; return false; }
        size_ = (size_t)st.st_size;
        if (size_) {
            map_ = (const char *)mmap(nullptr, size_, PROT_READ, MAP_SHARED, fd_, 0);
            if (map_ == MAP_FAILED) { map_ = nullptr; err = "cannot map " + path; return false; }
            (void)madvise((void *)map_, size_, MADV_WILLNEED);
        }
        n_blocks_ = (size_ + kBlock - 1) / kBlock;
        cnt_.assign(n_blocks_ + 1, 0);
        return true;
    }
    const char *data() const { return map_; }
    size_t bytes() const { return size_; }
    size_t n_blocks() const { return n_blocks_; }
    // newlines of blocks [b0, b1) (the shards of a run count a share each and tell one another)
    void count(size_t b0, size_t b1, Pool &pool)
    {
        const size_t n = b1 > b0 ? b1 - b0 : 0;
        const int parts = (int)std::min<size_t>(n, (size_t)pool.size() * 4);
        pool.run(parts, [&](int k) {
            for (size_t b = b0 + n * (size_t)k / (size_t)parts; b < b0 + n * (size_t)(k + 1) / (size_t)parts; b++) {
                const char *p = map_ + b * kBlock, *e = map_ + std::min(size_, (b + 1) * kBlock);
                uint32_t c = 0;
                while (p < e) { const char *q = (const char *)memchr(p, '\n', (size_t)(e - p)); if (!q) break; c++; p = q + 1; }
                cnt_[b] = c;
            }
        });
    }
    uint32_t *counts() { return cnt_.data(); }
    void finish() // prefix sums; lines of the file (an unterminated last line counts, like getline's)
    {
        pre_.assign(n_blocks_ + 1, 0);
        for (size_t b = 0; b < n_blocks_; b++) pre_[b + 1] = pre_[b] + cnt_[b];
        lines_ = pre_[n_blocks_] + ((size_ && map_[size_ - 1] != '\n') ? 1 : 0);
    }
    uint64_t lines() const { return lines_; }
    // byte at which line L begins (the file's size when it has no such line)
    size_t line_start(uint64_t L) const
    {
        if (L == 0) return 0;
        size_t lo = 0, hi = n_blocks_; // the block that holds the L-th newline
        while (lo < hi) { const size_t mid = (lo + hi) / 2; if (pre_[mid + 1] < L) lo = mid + 1; else hi = mid; }
        if (lo >= n_blocks_) return size_;
        uint64_t need = L - pre_[lo];
        const char *p = map_ + lo * kBlock, *e = map_ + std::min(size_, (lo + 1) * kBlock);
        while (need) { const char *q = (const char *)memchr(p, '\n', (size_t)(e - p)); if (!q) return size_; p = q + 1; need--; }
        return (size_t)(p - map_);
    }
    // Records [r0, r1) into out[0 ..), their number in n_out; stops like GetNextEntry at a missing sequence line or an empty read (false then).
    bool parse(uint64_t r0, uint64_t r1, int max_len, Rec *out, size_t &n_out, std::string &err) const
    {
        n_out = 0;
        size_t p = line_start(4 * r0);
        auto line = [&](const char *&l, size_t &len) { // the next line with its '\n' (getline); false at the end of the file
            if (p >= size_) return false;
            l = map_ + p;
            const char *e = find_nl(l, map_ + size_);
            len = e ? (size_t)(e - l) + 1 : size_ - p;
            p += len;
            return true;
        };
        for (uint64_t r = r0; r < r1; r++) {
            const char *l; size_t len;
            if (!line(l, len)) return false;
            int p1, p2;
            header_of(l, (int)len, p1, p2);
            Rec rec; memset(&rec, 0, sizeof rec);
            rec.name = (uint64_t)(l - map_) + (uint64_t)p1; rec.name_len = p2 > p1 ? (uint32_t)(p2 - p1) : 0;
            if (!line(l, len)) return false; // no sequence line
            rec.seq = (uint64_t)(l - map_); rec.rlen = len ? (uint32_t)(len - 1) : 0; // the last byte of the line is dropped (GetData.cpp:48-53)
            const char *q; size_t ql;
            (void)line(q, ql);              // the '+' line
            if (!line(q, ql)) { ql = 0; q = map_; }
            rec.qual = (uint64_t)(q - map_); rec.q_take = (uint32_t)std::min<size_t>(ql, rec.rlen);
            if (rec.rlen == 0) return false; // `.rlen == 0` ends the input (GetData.cpp:91)
            if ((int)rec.rlen > max_len) { err = "read " + std::string(map_ + rec.name, rec.name_len) + " is longer than max_read_len"; return false; }
            out[n_out++] = rec;
        }
        return true;
    }
private:
    enum : size_t { kBlock = 64u << 10 };
    int fd_ = -1;
    const char *map_ = nullptr;
    size_t size_ = 0, n_blocks_ = 0;
    std::vector<uint32_t> cnt_;
    std::vector<uint64_t> pre_;
    uint64_t lines_ = 0;
};

// a BGZF member at p (n bytes left in the file): its whole size and the length of its extra field; 0 if it is not one
inline size_t bgzf_member_at(const uint8_t *p, size_t n, size_t &xlen) { return mcx_bgzf_member_at(p, n, xlen); }

// The sequential reader: .gz through zlib, FASTA (multi-line records).
class Parser {
public:
    // inflate_device >= 0: a BGZF file is inflated on that device (mcx_inflate.hip) instead of by a pool of host threads; any other input is read as before
    bool open(const std::string &path, std::string &err, int inflate_device = -1)
    {
        gz_mode_ = path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0; // ReadMapping.cpp:709
        for (int k = 0; k < 4; k++) { std::unique_ptr<Block> b(new Block); b->d.resize(kHead + kBlockBytes); free_.push(std::move(b)); } // (one with the feeder, one with the splitter, two on their way)
        if (gz_mode_ && map_bgzf(path)) {
            // BGZF (bgzip, samtools): a gzip file made of independent members of at most 64 KB, each saying how long it is — the
            // members of a stretch are inflated side by side by a few threads — or, with -gpu_inflate, by a wavefront each on the device
            if (inflate_device >= 0 && mcx_inflater_create(inflate_device, 0, 0, 0, &inflater_) != 0) { err = std::string("-gpu_inflate: ") + mcx_last_error(); return false; }
            feeder_ = std::thread([this] { feed_bgzf(); });
        } else if (gz_mode_ && !getenv("MCX_GZ_SERIAL") && map_gz(path)) {
            // an ordinary gzip stream (what real FASTQ comes as): no entry points, so block starts are searched for and the stretches between them
            // inflated side by side against windows that are filled in afterwards (mcx_pgz.h) — zlib's one thread gives 0.5 GB/s of text per file
            feeder_ = std::thread([this] { feed_pgz(); });
        } else {
            gz_ = gzopen(path.c_str(), "rb");
            if (!gz_) { err = "cannot open " + path; return false; }
            gzbuffer(gz_, 1 << 20);
            // reading (and inflating) runs ahead of the line splitter on a thread of its own
            feeder_ = std::thread([this] {
                for (;;) {
                    std::unique_ptr<Block> b = free_.pop();
                    int got = stop_.load() ? 0 : gzread(gz_, b->text(), (unsigned)kBlockBytes);
                    b->n = got > 0 ? (size_t)got : 0;
                    b->look_for_nul();
                    const bool end = b->n == 0;
                    ready_.push(std::move(b));
                    if (end) break;
                }
            });
        }
        fill();
        fastq_ = end_ > pos_ && *pos_ == '@'; // CheckReadFormat, GetData.cpp:22-31
        return true;
    }
    ~Parser()
    {
        if (feeder_.joinable()) {
            stop_.store(true);
            if (cur_) { free_.push(std::move(cur_)); pos_ = end_ = nullptr; } // (the feeder may be waiting for a block to fill)
            while (!eof_) { std::unique_ptr<Block> b = ready_.pop(); if (b->n == 0) eof_ = true; else free_.push(std::move(b)); }
            feeder_.join();
        }
        if (gz_) gzclose(gz_);
        if (inflater_) mcx_inflater_free(inflater_); // (waits for what is still on the device: it reads the staging buffers, not the file)
        if (map_) munmap((void *)map_, map_size_);
    }
    bool fastq() const { return fastq_; }
    bool device_inflated() const { return inflater_ != nullptr; } // -gpu_inflate applied: the file is BGZF

    // appends up to `want` reads (copied into v.own); false once the input is exhausted (View::last set)
    bool take(View &v, uint32_t want, int max_len)
    {
        bool more = true;
        if (v.own.capacity() < (size_t)want * 64) v.own.reserve((size_t)want * (size_t)(own_per_rec_ + 16)); // (what the last batch's records took: no growth by doubling, no copies)
        const size_t own0 = v.own.size();
        uint32_t got = 0;
        for (uint32_t i = 0; i < want && more; i++) { if (!entry(v, max_len)) { v.last = true; more = false; } else got++; }
        if (got) own_per_rec_ = (v.own.size() - own0) / got + 1;
        v.base = v.own.data();
        return more;
    }

private:
    // A block of text on its way from the feeder to the line splitter: kBlockBytes of it behind kHead bytes of room, into which the splitter moves what the
    // block before left unfinished (a line's beginning, a record's first lines) — the lines are then cut where the feeder put them.  (Until round 6 every block
    // was copied once more, into the splitter's own buffer, and searched for a NUL there: both on the one thread per file that the .gz rate hangs on.)
    enum : size_t { kBlockBytes = 8u << 20, kHead = 64u << 10 };
    struct Block {
        std::vector<char> d; size_t n = 0; bool nul = false;
        char *text() { return d.data() + kHead; }
        void look_for_nul() { nul = n && memchr(text(), 0, n) != nullptr; } // (gzgets' lines are C strings: a NUL cuts one short — looked for per block, by the feeder)
    };
    gzFile gz_ = nullptr;
    bool gz_mode_ = false, fastq_ = true, eof_ = false, has_nul_ = false;
    size_t own_per_rec_ = 340; // bytes of names, bases and qualities a record of the last batch took
    std::unique_ptr<Block> cur_;             // the block the splitter is in
    const char *pos_ = nullptr, *end_ = nullptr; // what is left of it (with the carried-over bytes in front)
    std::vector<char> long_;                 // a line or record tail longer than kHead (a FASTA line of megabytes): block and tail put together here
    Queue<std::unique_ptr<Block>> ready_{4}, free_{4};
    std::thread feeder_;
    std::atomic<bool> stop_{false};
    const uint8_t *map_ = nullptr; // a BGZF file, mapped
    mcx_inflater *inflater_ = nullptr; // -gpu_inflate: the file's members are inflated on the device
    size_t map_size_ = 0;

    static size_t bgzf_member(const uint8_t *p, size_t n, size_t &xlen) { return bgzf_member_at(p, n, xlen); }
    bool map_bgzf(const std::string &path)
    {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        bool ok = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size >= 28;
        if (ok) {
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            ok = m != MAP_FAILED;
            if (ok) {
                size_t xlen = 0;
                if (bgzf_member((const uint8_t *)m, (size_t)st.st_size, xlen)) { map_ = (const uint8_t *)m; map_size_ = (size_t)st.st_size; }
                else { munmap(m, (size_t)st.st_size); ok = false; }
            }
        }
        close(fd);
        return ok;
    }
    bool map_gz(const std::string &path)
    {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        bool ok = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size >= 18;
        if (ok) {
            void *m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            ok = m != MAP_FAILED;
            if (ok) {
                if (pgz::gzip_header((const uint8_t *)m, (size_t)st.st_size)) { map_ = (const uint8_t *)m; map_size_ = (size_t)st.st_size; }
                else { munmap(m, (size_t)st.st_size); ok = false; } // (not a gzip file after all: zlib's reader passes such bytes through, as the reference's does)
            }
        }
        close(fd);
        return ok;
    }
    void feed_pgz()
    {
        Pool pool((int)std::max(2u, std::min(12u, mcx_usable_cpus() * 3 / 8)));
        pgz::Reader rd;
        pgz::Text text[2];
        bool have = rd.open(map_, map_size_, pool.size(), (size_t)2 << 20, [&](int n, const std::function<void(int)> &f) { pool.run(n, f); }) && rd.next(text[0]);
        for (int cur = 0; have && !stop_.load(); cur ^= 1) {
            // the next round is inflated while this round's text goes into the blocks (the pool stood still meanwhile: a tenth of the reader's time)
            bool more = false;
            std::thread ahead([&] { more = rd.next(text[cur ^ 1]); });
            const pgz::Text &t = text[cur];
            for (size_t o = 0; o < t.size() && !stop_.load();) {
                std::unique_ptr<Block> b = free_.pop();
                const size_t m = std::min<size_t>(t.size() - o, kBlockBytes);
                memcpy(b->text(), t.data() + o, m);
                b->n = m; o += m;
                b->look_for_nul();
                ready_.push(std::move(b));
            }
            ahead.join();
            have = more;
        }
        std::unique_ptr<Block> b = free_.pop(); // the end of the input (a damaged stream ends it where it stops making sense, as gzread's error does)
        b->n = 0;
        ready_.push(std::move(b));
    }
    void feed_bgzf()
    {
        struct Task { const uint8_t *src; uint32_t clen, isize, crc; size_t dst; };
        std::vector<Task> tasks;
        size_t o = 0;
        bool last = false; // what follows is not a BGZF member: the input ends there, as it does where gzread gives up
        auto walk = [&](size_t &total) { // as many members as a block of the pipe holds
            tasks.clear();
            total = 0;
            while (o < map_size_) {
                size_t xlen = 0;
                const uint8_t *p = map_ + o;
                const size_t size = bgzf_member(p, map_size_ - o, xlen);
                if (!size) { last = true; break; }
                const uint32_t isize = (uint32_t)p[size - 4] | ((uint32_t)p[size - 3] << 8) | ((uint32_t)p[size - 2] << 16) | ((uint32_t)p[size - 1] << 24);
                const uint32_t crc = (uint32_t)p[size - 8] | ((uint32_t)p[size - 7] << 8) | ((uint32_t)p[size - 6] << 16) | ((uint32_t)p[size - 5] << 24);
                if (isize > 65536) { last = true; break; }
                if (total + isize > kBlockBytes) break;
                Task t; t.src = p + 12 + xlen; t.clen = (uint32_t)(size - 12 - xlen - 8); t.isize = isize; t.crc = crc; t.dst = total;
                tasks.push_back(t);
                total += isize; o += size;
            }
        };
        if (inflater_) { feed_bgzf_device(walk, tasks, o, last); return; }
        Pool pool((int)std::max(2u, std::min(8u, mcx_usable_cpus() / 2)));
        std::atomic<int> bad(0);
        while (o < map_size_ && !stop_.load() && !bad.load() && !last) {
            std::unique_ptr<Block> b = free_.pop();
            size_t total = 0;
            walk(total);
            char *out = b->text();
            pool.run((int)tasks.size(), [&](int k) {
                const Task &t = tasks[(size_t)k];
                if (t.isize == 0) return; // (the empty member that ends a BGZF file)
                z_stream zs; memset(&zs, 0, sizeof zs);
                if (inflateInit2(&zs, -15) != Z_OK) { bad.store(1); return; }
                zs.next_in = const_cast<Bytef *>(t.src); zs.avail_in = t.clen;
                zs.next_out = (Bytef *)(out + t.dst); zs.avail_out = t.isize;
                const int rc = inflate(&zs, Z_FINISH);
                const bool ok = rc == Z_STREAM_END && zs.total_out == t.isize;
                inflateEnd(&zs);
                if (!ok || crc32(crc32(0L, Z_NULL, 0), (const Bytef *)(out + t.dst), t.isize) != t.crc) bad.store(1);
            });
            if (bad.load()) total = 0; // (a damaged stretch is not handed on)
            if (total == 0 && !bad.load() && !last && o < map_size_) { free_.push(std::move(b)); continue; } // (empty members in the middle of a file)
            b->n = total;
            b->look_for_nul();
            const bool end = total == 0;
            ready_.push(std::move(b));
            if (end) return;
        }
        std::unique_ptr<Block> b = free_.pop(); // the end of the input
        b->n = 0;
        ready_.push(std::move(b));
    }
    // The same stretches with the zlib calls replaced: a stretch's compressed bytes go to the inflater's page-locked staging and on to the device (one launch;
    // more only when a stretch holds more members or bytes than a launch does), its text comes back into the block.  The next stretch is walked and staged while
    // this one is on the device.  A stretch with a member that failed is not handed on and the input ends there: the host path's consequence.
    template <class Walk, class Tasks> void feed_bgzf_device(Walk &walk, Tasks &tasks, size_t &o, bool &last)
    {
        uint64_t max_src = 0, max_dst = 0; uint32_t max_members = 0;
        mcx_inflater_caps(inflater_, &max_src, &max_dst, &max_members);
        struct Launch { size_t total; bool closes; }; // a launch on the device: its stretch's bytes of text, and whether it is the stretch's last
        std::deque<Launch> flying;
        std::vector<mcx_deflate_member> members;
        std::unique_ptr<Block> b; // the block of the stretch whose launches are being collected
        bool bad = false;
        auto collect = [&]() -> bool { // the oldest launch; false: the input has ended
            if (!b) b = free_.pop();
            if (mcx_inflate_end(inflater_, (uint8_t *)b->text(), nullptr, nullptr) != 0) bad = true;
            const Launch l = flying.front();
            flying.pop_front();
            if (!l.closes) return true;
            const size_t total = bad ? 0 : l.total; // (a damaged stretch is not handed on)
            b->n = total;
            b->look_for_nul();
            ready_.push(std::move(b));
            return total != 0;
        };
        while (o < map_size_ && !stop_.load() && !last) {
            size_t total = 0;
            walk(total);
            if (total == 0) { if (!last && o < map_size_) continue; break; } // (empty members in the middle of a file; else the end)
            members.clear();
            for (const auto &t : tasks) {
                if (t.isize == 0) continue; // (the empty member that ends a BGZF file)
                mcx_deflate_member m; memset(&m, 0, sizeof m);
                m.src_off = (uint64_t)(t.src - map_); m.dst_off = t.dst; m.src_len = t.clen; m.isize = t.isize; m.crc32 = t.crc;
                members.push_back(m);
            }
            for (size_t at = 0; at < members.size();) {
                size_t k = at;
                uint64_t so = 0, to = 0;
                while (k < members.size() && k - at < max_members && so + members[k].src_len <= max_src && to + members[k].isize <= max_dst) { so += members[k].src_len; to += members[k].isize; k++; }
                while (flying.size() >= 2) if (!collect()) return;
                if (k == at || mcx_inflate_begin(inflater_, map_, map_size_, members.data() + at, (uint32_t)(k - at), kBlockBytes) != 0) {
                    fprintf(stderr, "[mcx_map_files] -gpu_inflate: %s\n", k == at ? "a member larger than a launch holds" : mcx_last_error());
                    while (!flying.empty()) if (!collect()) return;
                    last = true; // (the input ends here)
                    break;
                }
                flying.push_back(Launch{total, k == members.size()});
                at = k;
            }
            while (flying.size() > 1) if (!collect()) return; // (one launch stays on the device while the next stretch is walked and staged)
        }
        while (!flying.empty()) if (!collect()) return;
        if (!b) b = free_.pop(); // the end of the input
        b->n = 0;
        ready_.push(std::move(b));
    }

    void fill() // one more block of input behind what is left of this one
    {
        if (eof_) return;
        std::unique_ptr<Block> b = ready_.pop();
        if (b->n == 0) { eof_ = true; free_.push(std::move(b)); return; } // (what is left stays where it is: pos_ .. end_)
        const size_t left = (size_t)(end_ - pos_);
        if (b->nul) has_nul_ = true;
        if (left <= kHead) {
            if (left) memcpy(b->text() - left, pos_, left);
            pos_ = b->text() - left; end_ = b->text() + b->n;
            if (cur_) free_.push(std::move(cur_));
            cur_ = std::move(b);
            long_.clear();
        } else { // (rare: more left over than a block has room for in front)
            std::vector<char> both(left + b->n);
            memcpy(both.data(), pos_, left);
            memcpy(both.data() + left, b->text(), b->n);
            long_.swap(both);
            pos_ = long_.data(); end_ = long_.data() + long_.size();
            if (cur_) free_.push(std::move(cur_));
            free_.push(std::move(b));
        }
    }

    // next line including its '\n' (getline); the .gz reader's gzgets(buffer, 1024) cuts at 1023 bytes
    bool line(const char *&p, size_t &len, bool consume = true)
    {
        for (;;) {
            const size_t avail = (size_t)(end_ - pos_);
            const size_t lim = gz_mode_ ? std::min<size_t>(avail, 1023) : avail;
            const char *nl = lim ? find_nl(pos_, pos_ + lim) : nullptr; // (lines of tens to hundreds of bytes: memchr's set-up costs more than the search)
            if (nl) { p = pos_; len = (size_t)(nl - p) + 1; break; }
            if (gz_mode_ && avail >= 1023) { p = pos_; len = 1023; break; }
            if (eof_) { if (avail == 0) return false; p = pos_; len = avail; break; }
            fill();
        }
        if (consume) pos_ += len;
        return true;
    }

    bool entry(View &v, int max_len)
    {
        const char *p; size_t len;
        if (!line(p, len)) return false;
        if (gz_mode_) { // gzGetNextEntry :101-128 (strlen semantics: a line is a C string)
            if (has_nul_) len = strnlen(p, len);
            if (len == 0 || (p[0] != '@' && p[0] != '>')) return false;
        }
        int p1, p2;
        header_of(p, (int)len, p1, p2);
        std::vector<char> &o = v.own;
        const size_t name_at = o.size();
        if (p2 > p1) o.insert(o.end(), p + p1, p + p2);
        Rec rec; memset(&rec, 0, sizeof rec);
        rec.name = name_at; rec.name_len = (uint32_t)(o.size() - name_at);
        const size_t seq_at = o.size();
        size_t rlen = 0;
        if (fastq_ || gz_mode_) {
            if (!line(p, len)) { o.resize(name_at); return false; }
            if (gz_mode_ && has_nul_) len = strnlen(p, len);
            rlen = len ? len - 1 : 0; // the last byte of the line is dropped (GetData.cpp:48-53, :113)
            o.insert(o.end(), p, p + rlen);
            if (fastq_) {
                const char *q; size_t ql;
                line(q, ql);
                if (!line(q, ql)) ql = 0;
                if (gz_mode_ && has_nul_) ql = strnlen(q, ql);
                const size_t take = std::min(ql, rlen);
                rec.qual = o.size(); rec.q_take = (uint32_t)take;
                o.insert(o.end(), q, q + take);
            }
        } else { // plain FASTA: every line up to the next header (GetData.cpp:56-77)
            while (line(p, len, false)) {
                if (p[0] == '>') break;
                pos_ += len;
                o.insert(o.end(), p, p + len - 1);
            }
            rlen = o.size() - seq_at;
        }
        rec.seq = seq_at; rec.rlen = (uint32_t)rlen;
        if (rlen == 0) { o.resize(name_at); return false; } // `.rlen == 0` ends the input (GetData.cpp:91)
        if ((int)rlen > max_len) { v.error = "read " + std::string(o.data() + name_at, rec.name_len) + " is longer than max_read_len"; return false; }
        if (!v.recs.push_back(rec)) { v.error = "out of memory for the batch's read records"; o.resize(name_at); return false; }
        return true;
    }
};

}} // namespace mcx::files
