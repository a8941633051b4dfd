// tests/hostemu/gz_dev_check.cpp — the device's gunzipper (mapcaller_amd/csrc/mcx_gz_dev.h) compiled for the host with one lane: tests/test_gz_dev_host.py holds
// it against zlib's output, and tests/test_gz_device.py holds the kernels against it, round by round.  Built by the tests with their own compiler commands, not
// by this directory's Makefile: as a shared library (g++ -shared), and as a stand-alone program (-DGZ_DEV_CHECK_MAIN, with -fsanitize=address,undefined) that
// reads a file of vectors, runs every one of them and then seeded corruptions of them.
//
// The object below is mcx_gunzipper with loops where that has kernels: the same geometry, chain, pieces and halving (the header's host side), the arena laid out
// the same way — with guard symbols in front of the first region and in the gap behind every region, and guard bytes round the text, which must stay as they were.
#include "../../mapcaller_amd/csrc/mcx_gz_dev.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mcx::gzd;

namespace {
const uint32_t *crc_table()
{
    static uint32_t tab[256];
    static bool made = false;
    if (!made) { for (uint32_t i = 0; i < 256; i++) tab[i] = mcx::inf::crc_table_entry(i); made = true; }
    return tab;
}
enum : uint16_t { kGuardSym = 0xA5C3 };
enum : uint8_t { kGuardByte = 0x5A };
} // namespace

struct gzc {
    uint64_t stretch = 0, arena_symbols = 0;
    uint32_t max_n = 0, cur_n = 0, win_have = 0;
    uint16_t *arena = nullptr; // arena_total symbols: kGuardSyms in front, then the regions
    std::vector<uint64_t> starts;
    std::vector<Rec> recs;
    std::vector<uint8_t> win, wins;
    std::vector<uint32_t> piece_crc;
    uint8_t *src = nullptr; // the round's bytes in a buffer of exactly src_bytes + 8
    Geo g;
    Chain chain;
    int src_is_end = 0;
    bool begun = false;
    uint32_t guard_faults = 0;
    mcx::inf::Tables t;

    uint16_t *region(uint32_t i) const { return arena + kGuardSyms + (uint64_t)i * g.stride; }
    void set_guards()
    {
        for (uint32_t k = 0; k < kGuardSyms; k++) arena[k] = kGuardSym;
        for (uint32_t i = 0; i < g.n; i++) for (uint32_t k = 0; k < kGuardSyms; k++) region(i)[(uint64_t)kWin + g.room + k] = kGuardSym;
    }
    void check_guards()
    {
        for (uint32_t k = 0; k < kGuardSyms; k++) guard_faults += arena[k] != kGuardSym;
        for (uint32_t i = 0; i < g.n; i++) for (uint32_t k = 0; k < kGuardSyms; k++) guard_faults += region(i)[(uint64_t)kWin + g.room + k] != kGuardSym;
    }
};

extern "C" gzc *gzc_create(uint64_t stretch_bytes, uint32_t max_stretches, uint64_t arena_symbols)
{
    if (stretch_bytes && stretch_bytes < 4096) return nullptr;
    gzc *z = new gzc();
    z->stretch = stretch_bytes ? stretch_bytes : 65536;
    z->max_n = z->cur_n = max_stretches ? max_stretches : 2048;
    z->arena_symbols = arena_symbols ? arena_symbols : 8 * z->stretch * z->max_n;
    z->arena = (uint16_t *)malloc(arena_total(z->arena_symbols, z->max_n) * 2);
    if (!z->arena) { delete z; return nullptr; }
    z->starts.resize(z->max_n); z->recs.resize(z->max_n);
    z->win.assign(kWin, 0); z->wins.resize((size_t)z->max_n * kWin);
    memset(&z->g, 0, sizeof z->g);
    return z;
}
extern "C" void gzc_free(gzc *z) { if (z) { free(z->arena); free(z->src); delete z; } }
extern "C" void gzc_reset(gzc *z)
{
    z->win.assign(kWin, 0); z->win_have = 0; z->cur_n = z->max_n; z->begun = false;
    z->chain.at.clear(); z->chain.pieces.clear(); z->chain.off.assign(1, 0);
}
extern "C" uint32_t gzc_guard_faults(const gzc *z) { return z->guard_faults; }

// mcx_gunzip_round_dev.  src is copied into a buffer of exactly src_bytes + 8 (the contract's slack), so that a sanitizer sees any byte read outside it.
extern "C" int gzc_round(gzc *z, const uint8_t *src, uint64_t src_bytes, uint32_t start_bit, int src_is_end, mcx_gz_round *info)
{
    if (!z || !src || !info || start_bit > 7 || src_bytes == 0 || src_bytes > 0x7FFFFFF0ull) return MCX_ERR_ARG;
    memset(info, 0, sizeof *info);
    free(z->src);
    z->src = (uint8_t *)malloc(src_bytes + 8);
    memcpy(z->src, src, src_bytes);
    memset(z->src + src_bytes, 0xFF, 8); // (what lies behind the bytes is never consumed, whatever it is)
    z->g = plan_round(src_bytes, start_bit, z->stretch, z->cur_n, z->arena_symbols, z->win_have);
    const Geo &g = z->g;
    z->set_guards();
    z->starts[0] = start_bit;
    for (uint32_t i = 1; i < g.n; i++) z->starts[i] = find_start(z->src, g.src_len, g.readable, (uint64_t)i * g.stretch * 8, (uint64_t)(i + 1) * g.stretch * 8, z->t, 0);
    for (uint32_t i = 0; i < g.n; i++) {
        if (i > 0 && z->starts[i] == 0) { Rec r; r.start_bit = 0; r.stop_bit = 0; r.how = kNone; r.n_syms = 0; z->recs[i] = r; continue; }
        inflate_stretch(z->src, g, i, z->starts[i], z->starts.data(), z->win.data(), z->region(i), z->t, 0, &z->recs[i]);
    }
    walk(g, z->recs.data(), src_is_end, z->chain, info);
    z->cur_n = next_stretches(g.n, z->max_n, z->chain.room_hit);
    const uint32_t nc = (uint32_t)z->chain.at.size();
    std::vector<uint8_t> nw(kWin);
    for (uint32_t k = 0; k < nc; k++) {
        memcpy(z->wins.data() + (size_t)k * kWin, z->win.data(), kWin);
        window_step(z->region(z->chain.at[k]) + z->recs[z->chain.at[k]].n_syms, z->win.data(), nw.data(), 0, 1);
        z->win.swap(nw);
    }
    if (nc) z->win_have = (uint32_t)std::min<uint64_t>((uint64_t)z->win_have + info->text_bytes, kWin);
    z->check_guards();
    return 0;
}

// mcx_gunzip_text_dev.  The text is made in a buffer of exactly text_bytes between guard bytes, then handed to dst.
extern "C" int gzc_text(gzc *z, uint8_t *dst, uint64_t dst_cap, mcx_gz_round *info)
{
    if (!z || !info || info->text_bytes != z->chain.off.back()) return MCX_ERR_ARG;
    info->crc32 = 0;
    const size_t np = z->chain.pieces.size();
    if (np == 0) return 0;
    if (!dst) return MCX_ERR_ARG;
    if (dst_cap < info->text_bytes) return MCX_ERR_CAPACITY;
    uint8_t *buf = (uint8_t *)malloc(info->text_bytes + 128);
    memset(buf, kGuardByte, 64); memset(buf + 64 + info->text_bytes, kGuardByte, 64);
    z->piece_crc.resize(np);
    for (size_t k = 0; k < np; k++) {
        const Piece &p = z->chain.pieces[k];
        z->piece_crc[k] = text_piece(z->arena + kGuardSyms + p.sym_at, p.n, z->wins.data() + (size_t)p.win * kWin, buf + 64 + p.dst_at, crc_table(), 0);
    }
    for (int k = 0; k < 64; k++) z->guard_faults += (buf[k] != kGuardByte) + (buf[64 + info->text_bytes + k] != kGuardByte);
    z->check_guards();
    memcpy(dst, buf + 64, info->text_bytes);
    free(buf);
    info->crc32 = combine(z->chain, z->piece_crc.data());
    return 0;
}

// the last round's chain: its stretches and their start bits into idx[] / start_bit[] (as many as fit cap); returns how many it has
extern "C" uint32_t gzc_chain(const gzc *z, uint32_t *idx, uint64_t *start_bit, uint32_t cap)
{
    for (uint32_t k = 0; k < z->chain.at.size() && k < cap; k++) { idx[k] = z->chain.at[k]; start_bit[k] = z->recs[z->chain.at[k]].start_bit; }
    return (uint32_t)z->chain.at.size();
}
// every stretch's record of the last round: start bit, stop bit, how, symbols
extern "C" uint32_t gzc_records(const gzc *z, uint64_t *start_bit, uint64_t *stop_bit, uint32_t *how, uint32_t *n_syms, uint32_t cap)
{
    for (uint32_t i = 0; i < z->g.n && i < cap; i++) { start_bit[i] = z->recs[i].how == kNone ? 0 : z->recs[i].start_bit; stop_bit[i] = z->recs[i].stop_bit; how[i] = z->recs[i].how; n_syms[i] = z->recs[i].n_syms; }
    return z->g.n;
}

namespace {
struct HostEngine { // mcx_gz_dev.h's Reader over the object above: nothing to stage
    gzc *z;
    const uint8_t *src = nullptr; uint64_t bytes = 0; uint32_t start_bit = 0; int is_end = 0;
    const uint8_t *staged = nullptr; uint64_t staged_bytes = 0, rounds = 0, staged_hits = 0; // what stage() was last asked for; rounds begun, and those that lay inside it
    int begin(const uint8_t *s, uint64_t n, uint32_t bit, int end_)
    {
        src = s; bytes = n; start_bit = bit; is_end = end_;
        rounds++;
        if (staged && s >= staged && s + n <= staged + staged_bytes) staged_hits++;
        staged = nullptr;
        return 0;
    }
    void stage(const uint8_t *s, uint64_t n) { staged = s; staged_bytes = n; }
    int end(mcx_gz_round *info) { return gzc_round(z, src, bytes, start_bit, is_end, info); }
    uint32_t stretches() const { return z->cur_n; }
    uint64_t stretch_bytes() const { return z->stretch; }
    void reset() { gzc_reset(z); }
};
} // namespace

// mcx_gz_inflate_dev over a file in memory: the text's whole length, -1 no gzip file, -2 damaged (*n_out: bytes delivered before; *status: the mcx_gz_status of
// the round that failed; *rounds / *overflowed: rounds run, and rounds in which a stretch ran out of room; *guard_faults: guards that did not stay as they were)
extern "C" int64_t gzc_file(const uint8_t *data, uint64_t size, uint64_t stretch_bytes, uint32_t round_stretches, uint64_t arena_symbols, uint8_t *out, uint64_t cap, uint64_t *n_out, uint32_t *status, uint32_t *rounds,
                            uint32_t *overflowed, uint32_t *guard_faults)
{
    if (n_out) *n_out = 0;
    if (status) *status = 0;
    if (rounds) *rounds = 0;
    if (overflowed) *overflowed = 0;
    if (guard_faults) *guard_faults = 0;
    if (size < 18 || !gzip_header(data, size)) return -1;
    gzc *z = gzc_create(stretch_bytes, round_stretches, arena_symbols);
    if (!z) return -1;
    HostEngine e{z};
    Reader<HostEngine> rd(e, data, size);
    rd.open();
    uint64_t total = 0;
    std::vector<uint8_t> text;
    for (;;) {
        mcx_gz_round info;
        if (rd.next(&info) <= 0) break;
        if (rounds) (*rounds)++;
        if (overflowed && info.overflowed) (*overflowed)++;
        text.resize(info.text_bytes + 1);
        if (gzc_text(z, text.data(), info.text_bytes, &info) != 0) break;
        if (!rd.commit(&info)) break;
        if (out && total < cap) memcpy(out + total, text.data(), (size_t)std::min<uint64_t>(info.text_bytes, cap - total));
        total += info.text_bytes;
    }
    if (n_out) *n_out = total;
    if (status) *status = rd.status();
    if (guard_faults) *guard_faults = z->guard_faults;
    const bool failed = rd.failed();
    gzc_free(z);
    return failed ? -2 : (int64_t)total;
}

// the walker's staging by itself: over a file, how many rounds it begins and how many of them ask for bytes that lie inside what it had staged the round before
extern "C" void gzc_file_staging(const uint8_t *data, uint64_t size, uint64_t stretch_bytes, uint32_t round_stretches, uint64_t *rounds, uint64_t *staged_hits)
{
    *rounds = *staged_hits = 0;
    if (size < 18 || !gzip_header(data, size)) return;
    gzc *z = gzc_create(stretch_bytes, round_stretches, 0);
    if (!z) return;
    HostEngine e{z};
    Reader<HostEngine> rd(e, data, size);
    rd.open();
    std::vector<uint8_t> text;
    for (;;) {
        mcx_gz_round info;
        if (rd.next(&info) <= 0) break;
        text.resize(info.text_bytes + 1);
        if (gzc_text(z, text.data(), info.text_bytes, &info) != 0 || !rd.commit(&info)) break;
    }
    *rounds = e.rounds; *staged_hits = e.staged_hits;
    gzc_free(z);
}

#ifdef GZ_DEV_CHECK_MAIN
// The file: u32 n, then per vector  u32 file_len, expect, text_len, stretch, round_stretches, corrupt;  file_len bytes (the .gz file);  text_len bytes (its text).
// expect: 0 the whole text; 1 damaged (-2) and what was delivered is the text's beginning; 2 no gzip file (-1); 3 damaged (-2), whatever was delivered before
// the damage was found (a flipped byte may decode to other text for a while; only the member's CRC-32 would tell).
// Then argv[2] seeded corruptions of the vectors with corrupt != 0, in turn: a single bit flipped, or the file cut short.  Whatever comes out, no byte is read or
// written outside the buffers (the sanitizer's part) and no guard changes; a file that is still accepted whole gives the vector's text, a cut file its beginning.
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

struct Vec { uint32_t expect, stretch, round_stretches, corrupt; std::vector<uint8_t> file, text; };

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: gz_dev_check <vector file> [corruptions]\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t n_corrupt = argc > 2 ? (uint32_t)atoi(argv[2]) : 0;
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    std::vector<Vec> vecs(n);
    int bad = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t h[6];
        if (fread(h, 4, 6, f) != 6) { fprintf(stderr, "short file\n"); return 2; }
        Vec &v = vecs[i];
        v.expect = h[1]; v.stretch = h[3]; v.round_stretches = h[4]; v.corrupt = h[5];
        v.file.resize(h[0]); v.text.resize(h[2]);
        if (h[0] && fread(v.file.data(), 1, h[0], f) != h[0]) return 2;
        if (h[2] && fread(v.text.data(), 1, h[2], f) != h[2]) return 2;
        // (exact buffers: the sanitizer sees any byte outside them)
        uint8_t *in = (uint8_t *)malloc(v.file.size() ? v.file.size() : 1), *out = (uint8_t *)malloc(v.text.size() ? v.text.size() : 1);
        memcpy(in, v.file.data(), v.file.size());
        uint64_t got = 0; uint32_t status = 0, rounds = 0, over = 0, faults = 0;
        const int64_t r = gzc_file(in, v.file.size(), v.stretch, v.round_stretches, 0, out, v.text.size(), &got, &status, &rounds, &over, &faults);
        const uint64_t k = std::min<uint64_t>(got, v.text.size());
        const bool prefix = got <= v.text.size() && memcmp(out, v.text.data(), k) == 0;
        const bool ok = faults == 0 && (v.expect == 0 ? r == (int64_t)v.text.size() && prefix : v.expect == 1 ? r == -2 && prefix : v.expect == 3 ? r == -2 : r == -1);
        if (!ok) { printf("# vector %u: returned %lld, delivered %llu, status %u, guard faults %u, expected %u\n", i, (long long)r, (unsigned long long)got, status, faults, v.expect); bad++; }
        printf("%u %lld %llu %u %u %u\n", i, (long long)r, (unsigned long long)got, status, rounds, over);
        free(in); free(out);
    }
    fclose(f);
    std::vector<uint32_t> pool;
    for (uint32_t i = 0; i < n; i++) if (vecs[i].corrupt && vecs[i].expect == 0 && vecs[i].file.size() > 32) pool.push_back(i);
    uint32_t accepted = 0, refused = 0;
    for (uint32_t c = 0; c < n_corrupt && !pool.empty(); c++) {
        const Vec &v = vecs[pool[c % pool.size()]];
        const bool cut = (rng() & 3) == 0;
        const size_t len = cut ? (size_t)(rng() % v.file.size()) : v.file.size();
        uint8_t *in = (uint8_t *)malloc(len ? len : 1), *out = (uint8_t *)malloc(v.text.size() ? v.text.size() : 1);
        memcpy(in, v.file.data(), len);
        if (!cut) { const uint64_t bit = rng() % ((uint64_t)len * 8); in[bit >> 3] ^= (uint8_t)(1u << (bit & 7)); }
        uint64_t got = 0; uint32_t status = 0, rounds = 0, over = 0, faults = 0;
        const int64_t r = gzc_file(in, len, v.stretch, v.round_stretches, 0, out, v.text.size(), &got, &status, &rounds, &over, &faults);
        const uint64_t k = std::min<uint64_t>(got, v.text.size());
        bool ok = faults == 0;
        if (r >= 0 && !cut) ok = ok && r == (int64_t)v.text.size() && memcmp(out, v.text.data(), v.text.size()) == 0; // (a flip the stream does not depend on: the header's time, name, ...)
        if (cut) ok = ok && got <= v.text.size() && memcmp(out, v.text.data(), k) == 0;                                 // (what comes before the cut is the text's beginning)
        if (!ok) { printf("# corruption %u (%s): returned %lld, delivered %llu, guard faults %u\n", c, cut ? "cut" : "flip", (long long)r, (unsigned long long)got, faults); bad++; }
        if (r >= 0) accepted++; else refused++;
        free(in); free(out);
    }
    printf("corruptions: %u accepted, %u refused\n", accepted, refused);
    return bad ? 1 : 0;
}
#endif
