// mapcaller_amd/csrc/mcx_gz_dev.h — an ordinary gzip stream (one deflate stream, not BGZF's row of members) inflated by many wavefronts; for the device
// (mcx_gz_dev.hip's kernels) and, with one lane, for the host (tests/hostemu/gz_dev_check.cpp).
//
// mcx_pgz.h's method (Kerbiriou & Chikhi 2019, restated there) with a wavefront where it has a thread, on mcx_inflate.h's decoder — its Tables, build_code,
// read_dynamic, decode_sym, Bits and uniform-value discipline, none of them copied.  The compressed bytes of a ROUND are cut into n stretches of `stretch` bytes:
//   find_start        every stretch but the first looks for a block start in its own byte range.  The lanes test 64 candidate bits at a time with pgz::find_start's
//                     cheap filter (BFINAL 0, BTYPE 2, HLIT / HDIST <= 29, the code-length code fills its code space exactly); the survivors are taken in bit order,
//                     one at a time by the whole wavefront: read_dynamic in full (complete codes, an end-of-block code), then the block's first kProbeSyms symbols
//                     must be text (printable ASCII, TAB, CR, LF) with valid matches, and the block may not end before kProbeMin bytes.  The first that passes is
//                     the stretch's start, the same whatever the number of lanes.  A false start costs time only (below).
//   inflate_stretch   from a start (stretch 0: the round's known start bit) into 16-bit symbols: below 256 a byte, 256 + p "byte p of the 32 KB before my start".
//                     They are written behind a prefix of kWin symbols — those placeholders, or for stretch 0 the real window —, so a match copies symbols like
//                     any others: lane i writes o[p + i] = o[p - D + (i mod D)].  It stops at a block end (kBoundary) whose bit is the start of a later stretch,
//                     or lies at or beyond the round's end, or has the ranges of kPassed later stretches behind it in which no start was found (a round over
//                     bytes in which no start is found stays short and still makes progress; a passed stretch with a false start costs its own time only); at the final block (kFinal); or with kError / kInput / kRoom.
//   walk              (host) the chain: stretch 0, then whichever stretch begins exactly where the last one stopped.  A false start is never met: a true stretch
//                     stops on true block ends only; its output is dropped and the stretch before it has simply run on.
//   window_step       along the chain, a stretch's last kWin symbols resolved against the window before it: a serial chain, all threads inside a step.
//   text_piece        a piece of a chain stretch's symbols -> bytes at their final offset, resolved against the window before that stretch, and the piece's CRC-32
//                     (crc_of); the host combines the pieces with zlib's crc32_combine.
// Every loop is bounded and every access checked: input is read inside src[0 .. readable) only (what lies behind src_len reads as zeros and is never consumed:
// a reader that has consumed it has stopped with kInput), symbols are written inside the stretch's own region [0, kWin + room) only, a guard counter ends a stretch
// that decodes rubbish, and nothing waits for another wavefront.
// The host side of a round — its geometry (plan_round), the chain (walk), the pieces and how many stretches the next round takes (next_stretches) — is here too, so that
// the object (mcx_gz_dev.hip) and the host build make the same rounds; and so is the one walker of a FILE (Reader: RFC 1952 headers, trailers, concatenated members,
// garbage behind a member, staging of the next round's bytes), modelled on pgz::Reader, whose rules it keeps.
#ifndef MCX_GZ_DEV_H
#define MCX_GZ_DEV_H
#include "mcx_inflate.h"

namespace mcx {
namespace gzd {

using inf::kLanes;

enum : uint32_t { kWin = 32768, kGuardSyms = 64, kPassed = 4, kProbeSyms = 256, kProbeMin = 64, kPiece = 32768, kMaxRoom = 0xFFFF0000u };
enum Stop : uint32_t { kNone = 0 /* no start: takes no part */, kBoundary = 1, kFinal = 2, kError = 3, kInput = 4, kRoom = 5 };

// what a stretch records
struct Rec { uint64_t start_bit, stop_bit; uint32_t how, n_syms; };
// a round's geometry, the same for every stretch
struct Geo {
    uint64_t stretch, round_end_bit, stride; // bytes a stretch; the round's end; symbols between two stretches' regions (kWin + room + kGuardSyms)
    uint32_t n, src_len, readable, room;     // stretches; the round's bytes, and how many may be read; symbols a stretch may write behind its prefix
    uint32_t start_bit, win_have;            // stretch 0's start; bytes of text the member has before it (at most kWin)
};
// a piece of the text pass
struct Piece { uint64_t sym_at, dst_at; uint32_t n, win; }; // symbols arena[sym_at .. sym_at + n) -> dst[dst_at ..) against window `win` of the chain

static MCX_INF_HD bool is_text(uint32_t s) { return (s >= 32 && s < 127) || s == '\n' || s == '\r' || s == '\t'; }

// a candidate's dynamic header in full, then its first symbols as text
static MCX_INF_HD bool probe(const uint8_t *src, uint32_t src_len, uint32_t readable, uint64_t bit, inf::Tables &t, uint32_t lane)
{
    inf::Bits b;
    inf::bits_start(b, src, src_len, readable, bit + 3);
    bool no_dist = false;
    if (inf::read_dynamic(b, t, lane, no_dist, nullptr)) return false;
    uint32_t n = 0;
    for (uint32_t k = 0; k < kProbeSyms; k++) {
        inf::bits_refill(b);
        const int s = inf::decode_sym(b, t.lit_root, inf::kLitRootBits, t.lit_sorted, t.lit_cnt);
        if (s < 0) return false;
        if (s < 256) { if (!is_text((uint32_t)s)) return false; n++; continue; }
        if (s == 256) return !inf::bits_over(b) && n >= kProbeMin; // (a block of a few bytes in the middle of a stream: not something a compressor writes)
        const uint32_t li = (uint32_t)s - 257;
        if (li >= 29 || no_dist) return false;
        n += inf::len_base(li) + inf::bits_take(b, inf::len_extra(li));
        const int ds = inf::decode_sym(b, t.dist_root, inf::kDistRootBits, t.dist_sorted, t.dist_cnt);
        if (ds < 0 || ds >= 30) return false;
        inf::bits_drop(b, inf::dist_extra((uint32_t)ds));
    }
    return !inf::bits_over(b);
}

// a block start in bits [lo, hi) of src: the first candidate that passes (0: none).  Called by every lane of a wavefront with the same arguments.
static MCX_INF_HD uint64_t find_start(const uint8_t *src, uint32_t src_len, uint32_t readable, uint64_t lo, uint64_t hi, inf::Tables &t, uint32_t lane)
{
    for (uint64_t base = lo; base < hi; base += kLanes) {
        const uint64_t bit = base + lane, byte = bit >> 3;
        bool pass = false;
        if (bit < hi && byte + 24 < src_len) { // (16 bytes are looked at here; a start so close to the end of the bytes has no block behind it)
            uint64_t w; memcpy(&w, src + byte, 8);
            w >>= (bit & 7);
            if ((w & 7u) == 4u) { // BFINAL 0, BTYPE 2
                const uint32_t hlit = (uint32_t)(w >> 3) & 31u, hdist = (uint32_t)(w >> 8) & 31u, hclen = ((uint32_t)(w >> 13) & 15u) + 4u;
                if (hlit <= 29u && hdist <= 29u) {
                    uint64_t x = w >> 17; // 57 - (bit & 7) >= 50 bits left: sixteen lengths; the last three come from the next bytes
                    if (hclen > 13) { uint64_t y; memcpy(&y, src + byte + 8, 8); x |= y << (47 - (bit & 7)); }
                    uint32_t space = 0;
                    for (uint32_t i = 0; i < 19; i++) { const uint32_t l = (uint32_t)(x >> (3 * i)) & 7u; if (i < hclen && l) space += 128u >> l; }
                    pass = space == 128u;
                }
            }
        }
        uint64_t m = inf::ballot(pass);
        while (m) {
            const uint32_t k = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            if (probe(src, src_len, readable, base + k, t, lane)) return base + k;
        }
    }
    return 0;
}

// the literals gathered so far go to o[out - n_lit .. out)
static MCX_INF_HD void flush_syms(uint16_t *o, uint32_t out, uint64_t lits, uint32_t n_lit, uint32_t lane)
{
    for (uint32_t i = lane; i < n_lit; i += kLanes) o[out - n_lit + i] = (uint16_t)((lits >> (8 * i)) & 0xFFu);
}

// Stretch i of the round from bit `from` into region[0 .. kWin + g.room): the prefix, then its symbols.  starts[j]: stretch j's start (0: none), j < g.n.
// win: (stretch 0) the kWin bytes of text before the round, zeros in front where the member has fewer.  Called by every lane of a wavefront with the same
// arguments; *rec is written by lane 0.
static MCX_INF_HD void inflate_stretch(const uint8_t *src, const Geo &g, uint32_t i, uint64_t from, const uint64_t *starts, const uint8_t *win, uint16_t *region, inf::Tables &t, uint32_t lane, Rec *rec)
{
    for (uint32_t j = lane; j < kWin; j += kLanes) region[j] = i == 0 ? (uint16_t)win[j] : (uint16_t)(256 + j);
    inf::sync_output();
    uint16_t *o = region + kWin;
    const uint32_t room = g.room, src_len = g.src_len;
    const uint32_t reach = i == 0 ? g.win_have : kWin; // how far before the stretch a match may begin
    inf::Bits b;
    inf::bits_start(b, src, src_len, g.readable, from);
    uint32_t out = 0, n_lit = 0, codes = 0, how = kError, good = 0, passed = i, none = 0; // passed: the last stretch whose range lies behind the last block end; none: how many of them found no start
    uint64_t lits = 0, stop_bit = from;
    bool no_dist = false;
    // every step below consumes a bit or writes a symbol, and both are limited: the guard is never what ends a valid stretch
    uint64_t guard = ((uint64_t)src_len * 8 > from ? (uint64_t)src_len * 8 - from : 0) + room + 64;
    for (;;) {
        inf::bits_refill(b);
        const uint32_t bfinal = inf::bits_take(b, 1), btype = inf::bits_take(b, 2);
        if (inf::bits_over(b)) { how = kInput; break; }
        if (btype == 3) break;
        if (btype == 0) {
            inf::bits_drop(b, b.cnt & 7u);
            inf::bits_refill(b);
            const uint32_t len = inf::bits_take(b, 16), nlen = inf::bits_take(b, 16);
            if (inf::bits_over(b)) { how = kInput; break; }
            if ((len ^ nlen) != 0xFFFFu) break;
            const uint32_t at = b.p - (b.cnt >> 3);
            if ((uint64_t)at + len > src_len) { how = kInput; break; }
            if (len > room - out) { how = kRoom; break; }
            if (guard < len + 1) break;
            guard -= len + 1;
            flush_syms(o, out, lits, n_lit, lane); n_lit = 0; lits = 0;
            for (uint32_t k = lane; k < len; k += kLanes) o[out + k] = src[at + k];
            out += len;
            inf::bits_start(b, src, src_len, g.readable, (uint64_t)(at + len) * 8);
        } else {
            if (btype == 1) { if (codes != 1) inf::fixed_codes(t, lane); codes = 1; no_dist = false; }
            else {
                codes = 0;
                if (const uint32_t st = inf::read_dynamic(b, t, lane, no_dist, nullptr)) { how = st == MCX_INFLATE_INPUT ? (uint32_t)kInput : (uint32_t)kError; break; }
                codes = 2;
            }
            bool eob = false;
            for (;;) {
                if (guard-- == 0) break;
                inf::bits_refill(b);
                const int s = inf::decode_sym(b, t.lit_root, inf::kLitRootBits, t.lit_sorted, t.lit_cnt);
                if (inf::bits_over(b)) { how = kInput; break; }
                if (s < 0) break;
                if (s < 256) {
                    if (out >= room) { how = kRoom; break; }
                    lits |= (uint64_t)(uint32_t)s << (8 * n_lit);
                    n_lit++; out++;
                    if (n_lit == 8) { flush_syms(o, out, lits, n_lit, lane); n_lit = 0; lits = 0; }
                    continue;
                }
                if (s == 256) { eob = true; break; }
                const uint32_t li = (uint32_t)s - 257;
                if (li >= 29 || no_dist) break;
                const uint32_t len = inf::len_base(li) + inf::bits_take(b, inf::len_extra(li));
                const int ds = inf::decode_sym(b, t.dist_root, inf::kDistRootBits, t.dist_sorted, t.dist_cnt);
                if (inf::bits_over(b)) { how = kInput; break; }
                if (ds < 0 || ds >= 30) break;
                const uint32_t dist = inf::dist_base((uint32_t)ds) + inf::bits_take(b, inf::dist_extra((uint32_t)ds));
                if (inf::bits_over(b)) { how = kInput; break; }
                if (dist > out && dist - out > reach) break; // (before the start of the member's text; dist <= kWin: inside the prefix at worst)
                if (len > room - out) { how = kRoom; break; }
                flush_syms(o, out, lits, n_lit, lane); n_lit = 0; lits = 0;
                inf::sync_output();
                const uint16_t *fr = o + out - dist; // (pointer arithmetic inside the region: out - dist >= -kWin)
                for (uint32_t k = lane; k < len; k += kLanes) o[out + k] = fr[k < dist ? k : k % dist];
                out += len;
            }
            if (!eob) break;
        }
        // a block's end
        flush_syms(o, out, lits, n_lit, lane); n_lit = 0; lits = 0;
        const uint64_t e = inf::bits_pos(b);
        stop_bit = e; good = out;
        if (bfinal) { how = kFinal; break; }
        if (e >= g.round_end_bit) { how = kBoundary; break; }
        const uint64_t j = (e >> 3) / g.stretch; // the stretch whose range holds e
        if (j > i && j < g.n && inf::uni64(starts[j]) == e) { how = kBoundary; break; }
        for (; passed + 1 < j && passed + 1 < g.n; passed++) none += inf::uni64(starts[passed + 1]) == 0; // stretches i + 1 .. j - 1 lie behind e
        if (none >= kPassed) { how = kBoundary; break; }
    }
    if (lane == 0) { rec->start_bit = from; rec->stop_bit = stop_bit; rec->how = how; rec->n_syms = good; }
}

// one step of the window chain: last[0 .. kWin) — the kWin symbols that end at a stretch's end, reaching into its prefix when it is shorter — against the window w
// before the stretch give the window nw behind it.  Thread tid of nthreads; the caller puts a barrier between two steps.
static MCX_INF_HD void window_step(const uint16_t *last, const uint8_t *w, uint8_t *nw, uint32_t tid, uint32_t nthreads)
{
    for (uint32_t j = tid; j < kWin; j += nthreads) { const uint32_t s = last[j]; nw[j] = (uint8_t)(s < 256 ? s : w[(s - 256) & (kWin - 1)]); }
}

// a piece of the text: sym[0 .. n) -> dst[0 .. n) against window w (kWin bytes); returns the piece's CRC-32.  Every lane of a wavefront, the same arguments.
static MCX_INF_HD uint32_t text_piece(const uint16_t *sym, uint32_t n, const uint8_t *w, uint8_t *dst, const uint32_t *crc_tab, uint32_t lane)
{
    for (uint32_t j = lane; j < n; j += kLanes) { const uint32_t s = sym[j]; dst[j] = (uint8_t)(s < 256 ? s : w[(s - 256) & (kWin - 1)]); }
    inf::sync_output();
    return inf::crc_of(dst, n, crc_tab, lane);
}

} // namespace gzd
} // namespace mcx

// ---- the host side of a round, and of a file ----
#include <zlib.h>
#include <algorithm>
#include <vector>

namespace mcx {
namespace gzd {

// the geometry of a round over src_bytes from start_bit (0 .. 7) with at most cur_n stretches: no stretch begins beyond the bytes' end
static inline Geo plan_round(uint64_t src_bytes, uint32_t start_bit, uint64_t stretch, uint32_t cur_n, uint64_t arena_symbols, uint32_t win_have)
{
    Geo g;
    memset(&g, 0, sizeof g);
    const uint64_t n = std::min<uint64_t>(std::max<uint32_t>(cur_n, 1), src_bytes / stretch + 1);
    g.stretch = stretch; g.n = (uint32_t)n; g.round_end_bit = n * stretch * 8;
    g.src_len = (uint32_t)std::min<uint64_t>(src_bytes, 0x7FFFFFF0u); g.readable = g.src_len + 8;
    g.room = (uint32_t)std::min<uint64_t>(arena_symbols / n, kMaxRoom);
    g.stride = (uint64_t)kWin + g.room + kGuardSyms;
    g.start_bit = start_bit; g.win_have = win_have;
    return g;
}
// symbols the arena must hold for rounds of up to max_n stretches: the prefixes and guards beside arena_symbols
static inline uint64_t arena_total(uint64_t arena_symbols, uint32_t max_n) { return arena_symbols + (uint64_t)max_n * (kWin + kGuardSyms) + kGuardSyms; }

struct Chain {
    std::vector<uint32_t> at;     // the stretches of the chain
    std::vector<Piece> pieces;    // of the text pass
    std::vector<uint64_t> off = std::vector<uint64_t>(1, 0); // where each chain stretch's text begins in the round's; the last entry: text_bytes
    bool room_hit = false;        // a stretch out of room ended the chain
};

// The chain of a round from its stretches' records, and the round's figures (all but crc32 and ms).  A stretch with kError / kInput / kRoom ends the chain in
// front of it: the next round starts at its start bit, where it is stretch 0 and says what is wrong with the stream.
static inline void walk(const Geo &g, const Rec *recs, int src_is_end, Chain &c, mcx_gz_round *info)
{
    c.at.clear(); c.pieces.clear(); c.off.assign(1, 0); c.room_hit = false;
    info->end_bit = g.start_bit; info->text_bytes = 0; info->crc32 = 0; info->final = 0; info->status = MCX_GZ_OK;
    info->stretches = g.n; info->starts = 0; info->chain = 0; info->overflowed = 0;
    for (uint32_t i = 0; i < g.n; i++) { info->starts += i > 0 && recs[i].how != kNone; info->overflowed += recs[i].how == kRoom; }
    uint32_t cur = 0;
    uint64_t at = g.start_bit;
    for (;;) {
        const Rec &r = recs[cur];
        if (r.how != kBoundary && r.how != kFinal) {
            if (r.how == kRoom) c.room_hit = true;
            if (c.at.empty()) info->status = r.how == kRoom ? (g.n == 1 ? MCX_GZ_CAPACITY : MCX_GZ_OK) : r.how == kInput ? (src_is_end ? MCX_GZ_INPUT : MCX_GZ_MORE) : MCX_GZ_DAMAGED;
            break;
        }
        c.at.push_back(cur);
        c.off.push_back(c.off.back() + r.n_syms);
        at = r.stop_bit;
        if (r.how == kFinal) { info->final = 1; break; }
        const uint64_t j = (at >> 3) / g.stretch;
        if (j > cur && j < g.n && recs[j].how != kNone && recs[j].start_bit == at) cur = (uint32_t)j; else break;
    }
    info->end_bit = at; info->text_bytes = c.off.back(); info->chain = (uint32_t)c.at.size();
    for (size_t k = 0; k < c.at.size(); k++) {
        const uint32_t n = recs[c.at[k]].n_syms;
        for (uint32_t p = 0; p < n; p += kPiece) {
            Piece pc;
            pc.sym_at = (uint64_t)c.at[k] * g.stride + kWin + p; pc.dst_at = c.off[k] + p; pc.n = std::min<uint32_t>(kPiece, n - p); pc.win = (uint32_t)k;
            c.pieces.push_back(pc);
        }
    }
}
// stretches of the next round: half as many after a round whose chain a stretch out of room ended, the full number again after any other
static inline uint32_t next_stretches(uint32_t this_n, uint32_t max_n, bool room_hit) { return room_hit ? std::max<uint32_t>(this_n / 2, 1) : max_n; }
// the round's CRC-32 from its pieces'
static inline uint32_t combine(const Chain &c, const uint32_t *piece_crc)
{
    uint32_t crc = (uint32_t)crc32(0L, Z_NULL, 0);
    for (size_t k = 0; k < c.pieces.size(); k++) crc = (uint32_t)crc32_combine(crc, piece_crc[k], (z_off_t)c.pieces[k].n);
    return crc;
}

// A gzip member's header at p (RFC 1952): its length, 0 if it is not one (pgz::gzip_header's rule)
static inline size_t gzip_header(const uint8_t *p, size_t n)
{
    if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || (p[3] & 0xE0)) return 0;
    size_t o = 10;
    const int flg = p[3];
    if (flg & 4) { if (o + 2 > n) return 0; o += 2 + ((size_t)p[o] | ((size_t)p[o + 1] << 8)); }
    if (flg & 8) { while (o < n && p[o]) o++; o++; }
    if (flg & 16) { while (o < n && p[o]) o++; o++; }
    if (flg & 2) o += 2;
    return o < n ? o : 0;
}

// The walker of a file over an engine E that runs rounds on HOST bytes (the object behind page-locked staging; the host build directly):
//   int  begin(const uint8_t *src, uint64_t bytes, uint32_t start_bit, int is_end)   the round's search and inflate are under way
//   void stage(const uint8_t *src, uint64_t bytes)                                   bytes the next round will probably ask for (may do nothing)
//   int  end(mcx_gz_round *)                                                         the round's figures (0, or an error of the engine's own)
//   uint32_t stretches() / uint64_t stretch_bytes() / void reset()
// A round:  next() — > 0: a round with info.text_bytes of text (0 is possible), which the caller fetches with the engine's text call into room it has made and
// then hands to commit() — true: the text counts; false: the trailer does not match, nothing of the round is handed on.  next() == 0: the input's end (failed():
// where the stream is damaged); < 0: the engine's error.  pgz::Reader's rules: a file that does not begin with a header fails; what is no header behind a complete
// member ends the input quietly; members follow one another.
template <class E>
class Reader {
public:
    Reader(E &e, const uint8_t *data, size_t size) : e_(e), d_(data), size_(size) {}
    bool open() { return next_member(0); }
    bool failed() const { return failed_; }
    uint32_t status() const { return status_; } // of the round that failed
    int next(mcx_gz_round *info)
    {
        for (;;) {
            if (done_) return 0;
            const size_t at = (size_t)(bit_ >> 3);
            const uint64_t avail = size_ - at, n = e_.stretches(), S = e_.stretch_bytes();
            const uint64_t want = (n + 1) * S + extra_, bytes = std::min(avail, want);
            const int is_end = bytes == avail;
            if (int rc = e_.begin(d_ + at, bytes, (uint32_t)(bit_ & 7), is_end)) return rc < 0 ? rc : -1;
            if (!is_end) { const uint64_t ahead = std::min<uint64_t>(n * S, avail); e_.stage(d_ + at + ahead, std::min(avail - ahead, want + 4 * S + extra_)); } // (slack: a round ends on the first block end at or BEYOND its last stretch, so the next begins a block's rest further on and asks for `want` bytes from there)
            if (int rc = e_.end(info)) return rc < 0 ? rc : -1;
            if (info->status == MCX_GZ_MORE) { extra_ = std::max<uint64_t>(extra_ * 2, 4 * S); continue; }
            if (info->status != MCX_GZ_OK) { done_ = failed_ = true; status_ = info->status; return 0; }
            base_ = at;
            return 1;
        }
    }
    bool commit(const mcx_gz_round *info)
    {
        crc_ = (uint32_t)crc32_combine(crc_, info->crc32, (z_off_t)info->text_bytes);
        total_ += info->text_bytes;
        bit_ = (uint64_t)base_ * 8 + info->end_bit;
        if (info->final) { // trailer: CRC-32 and ISIZE (RFC 1952 2.3.1), then perhaps another member
            const size_t tb = (size_t)((bit_ + 7) >> 3);
            if (tb + 8 > size_) { done_ = failed_ = true; status_ = MCX_GZ_INPUT; return false; }
            const uint32_t want_crc = (uint32_t)d_[tb] | ((uint32_t)d_[tb + 1] << 8) | ((uint32_t)d_[tb + 2] << 16) | ((uint32_t)d_[tb + 3] << 24);
            const uint32_t want_len = (uint32_t)d_[tb + 4] | ((uint32_t)d_[tb + 5] << 8) | ((uint32_t)d_[tb + 6] << 16) | ((uint32_t)d_[tb + 7] << 24);
            if (want_crc != crc_ || want_len != (uint32_t)total_) { done_ = failed_ = true; status_ = MCX_GZ_DAMAGED; return false; }
            next_member(tb + 8); // (the text of this round still counts)
        }
        return true;
    }

private:
    E &e_;
    const uint8_t *d_; size_t size_;
    uint64_t bit_ = 0;        // the next block's bit, from the file's first byte
    size_t base_ = 0;         // the byte the last round's bits count from
    uint64_t extra_ = 0;      // bytes beyond a round's stretches that are passed on (more after MCX_GZ_MORE: a block longer than that)
    uint32_t crc_ = 0; uint64_t total_ = 0; // of this member so far
    uint32_t status_ = 0;
    bool done_ = false, failed_ = false;

    bool next_member(size_t at)
    {
        if (at >= size_) { done_ = true; return at == size_ && at > 0; }
        const size_t h = gzip_header(d_ + at, size_ - at);
        if (!h) { done_ = true; failed_ = at == 0; return false; } // (trailing garbage behind a complete member ends the input quietly, as gzread has it)
        bit_ = (uint64_t)(at + h) * 8; crc_ = (uint32_t)crc32(0L, Z_NULL, 0); total_ = 0;
        e_.reset();
        return true;
    }
};

} // namespace gzd
} // namespace mcx
#endif
