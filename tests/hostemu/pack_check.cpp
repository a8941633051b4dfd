// tests/hostemu/pack_check.cpp — the read packer's body (mapcaller_amd/csrc/mcx_pack.h) on the host, part by part the way k_pack_reads
// (mcx_pipeline.hip) walks a batch, against pack_read() (mcx_fm.h).
//
// The batch's bytes lie in a buffer of exactly the batch's size; a part reads its read through the aligned 16-byte words that hold a byte
// of the READ (stricter than the kernel's rule, which allows every word that holds a byte of the batch), copied to a buffer of exactly
// that many words, and the rows lie in a buffer of exactly the batch's rows, so that under -fsanitize=address a load or store outside any
// of them stops the program.  Compared: words [0, packed_words(rlen)) of every row,
// the batch's any-N word and every read's odd flag; rows of reads that do not fit the stride must stay untouched.
//
//   pack_check            runs every case; exit status 0 when all agree
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mapcaller_amd/csrc/mcx_pack.h"

using namespace mcx;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 24);
}

static const int kLens[16] = {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 149, 150, 151, 255, 256, 1000};
static const char kOdd[] = "NnacgtRYKMSWBDHVrykmswbdhvUu.-*";

struct Batch {
    std::vector<uint32_t> off;
    uint8_t *bytes = nullptr;   // exactly off.back() bytes
    uint8_t *padded = nullptr;  // the same bytes with room behind them, for pack_read()'s 16-byte cursor
    int longest = 0;
    ~Batch() { free(bytes); free(padded); }
};

// reads of the lengths of kLens[0 .. n_lens), mixed; a third clean, a third with odd bytes at the first and last byte and on both sides of
// every 16-base boundary (every 32-base one among them), a third with odd bytes anywhere
static void make_batch(Batch &b, uint32_t n_reads, int n_lens)
{
    b.off.assign(1, 0u);
    for (uint32_t r = 0; r < n_reads; r++) {
        const int len = kLens[(r * 7u + r / 16u) % (uint32_t)n_lens];
        b.off.push_back(b.off.back() + (uint32_t)len);
        if (len > b.longest) b.longest = len;
    }
    const uint32_t total = b.off.back();
    b.bytes = (uint8_t *)malloc(total);
    b.padded = (uint8_t *)aligned_alloc(16, ((size_t)total + 64 + 15) & ~(size_t)15);
    const size_t n_odd = sizeof kOdd - 1;
    for (uint32_t r = 0; r < n_reads; r++) {
        uint8_t *p = b.bytes + b.off[r];
        const int len = (int)(b.off[r + 1] - b.off[r]), kind = (int)(r % 3u);
        for (int i = 0; i < len; i++) {
            p[i] = (uint8_t)"ACGT"[rnd() & 3];
            if (kind == 2 && rnd() % 20 == 0) p[i] = (uint8_t)kOdd[rnd() % n_odd];
            // (both orientations: mate 2's boundaries count from the read's end)
            const bool edge = i == 0 || i == len - 1 || (i & 15) == 0 || (i & 15) == 15 || ((len - 1 - i) & 15) == 0 || ((len - 1 - i) & 15) == 15;
            if (kind == 1 && edge && rnd() % 2 == 0) p[i] = (uint8_t)kOdd[rnd() % n_odd];
        }
    }
    memcpy(b.padded, b.bytes, total);
    memset(b.padded + total, 'N', 64);
}

static int g_bad = 0;
static void bad(const char *what, uint32_t r, int k, uint32_t got, uint32_t want)
{
    if (g_bad++ < 20) fprintf(stderr, "  %s: read %u word %d: got %08x, want %08x\n", what, r, k, got, want);
}

// the batch through the packer with rows of wpad words and tpr parts per read
static void run_case(const Batch &b, int paired, int wpad, int tpr, const char *name)
{
    const uint32_t n_reads = (uint32_t)b.off.size() - 1;
    const uint32_t kFill = 0xDEADBEEFu;
    uint32_t *out = (uint32_t *)aligned_alloc(16, (size_t)n_reads * wpad * 4);
    for (size_t i = 0; i < (size_t)n_reads * wpad; i++) out[i] = kFill;
    std::vector<uint8_t> odd(n_reads, 0);
    uint32_t any_n = 0;
    const int before = g_bad;

    // a read staged: the aligned 16-byte words that hold bytes [a, e) of the batch, nothing else
    auto stage = [&](uint32_t a, uint32_t e, uint32_t &lo) -> U4 * {
        lo = a & ~15u;
        const uint32_t n16 = e > a ? (((e + 15u) & ~15u) - lo) >> 4 : 0u;
        if (n16 == 0) return nullptr;
        U4 *s = (U4 *)aligned_alloc(16, (size_t)n16 * 16);
        for (uint32_t i = 0; i < n16 * 16; i++) ((uint8_t *)s)[i] = (uint8_t)rnd(); // (what lies around the span is anything)
        memcpy((uint8_t *)s + (a - lo), b.bytes + a, e - a);
        return s;
    };
    auto part = [&](uint32_t r, int m) { // pack_read_part
        const uint32_t a = b.off[r];
        const int rlen = (int)(b.off[r + 1] - a), flipped = (paired && (r & 1)) ? 1 : 0, nmw = (rlen + 31) >> 5;
        if (packed_words(rlen) > wpad) return;
        uint32_t *o = out + (size_t)r * wpad;
        if (m < nmw) {
            uint32_t lo, has_n, od;
            U4 *s = stage(a, a + (uint32_t)rlen, lo);
            pack_unit32(s, a - lo, rlen, flipped, m, o, has_n, od);
            free(s);
            if (od) odd[r] |= 2;
            if (has_n) any_n |= 1;
        } else if (m == nmw) pack_row_ends(rlen, o);
    };

    for (uint32_t r = 0; r < n_reads; r++) for (int m = 0; m < tpr; m++) part(r, m); // k_pack_reads: a thread per part

    // what pack_read() makes of the same reads
    uint32_t want_any = 0;
    std::vector<uint32_t> ref((size_t)packed_words(b.longest) + 4);
    for (uint32_t r = 0; r < n_reads; r++) {
        const int rlen = (int)(b.off[r + 1] - b.off[r]);
        const uint32_t *o = out + (size_t)r * wpad;
        bool is_odd = false;
        for (int i = 0; i < rlen; i++) {
            const uint8_t ch = b.bytes[b.off[r] + i];
            if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') is_odd = true;
            if (nt4_code(ch) > 3 && packed_words(rlen) <= wpad) want_any = 1;
        }
        if (packed_words(rlen) > wpad) { // left out: nothing of its row may have been written
            for (int k = 0; k < wpad; k++) if (o[k] != kFill) bad("a row that was to be left out", r, k, o[k], kFill);
            if (odd[r]) bad("odd flag of a read left out", r, 0, odd[r], 0);
            continue;
        }
        ReadRef rd; rd.ascii = b.padded + b.off[r]; rd.rlen = rlen; rd.flipped = (paired && (r & 1)) ? 1 : 0;
        PackedRead pk; pk.w = ref.data(); pk.stride = 1; pk.n_code = 0;
        pack_read(rd, pk);
        for (int k = 0; k < packed_words(rlen); k++) if (o[k] != ref[k]) bad(name, r, k, o[k], ref[k]);
        if ((odd[r] != 0) != is_odd) bad("odd flag", r, 0, odd[r], is_odd ? 2u : 0u);
    }
    if (any_n != want_any) bad("any_n", 0, 0, any_n, want_any);
    free(out);
    printf("%-44s reads %5u paired %d wpad %3d tpr %2d: %s\n", name, n_reads, paired, wpad, tpr, g_bad == before ? "ok" : "MISMATCH");
}

static int stride_for(int len) { return (packed_words(len) + 3) & ~3; }

int main()
{
    const uint32_t sizes[3] = {2, 254, 4098};
    for (int n_lens = 15; n_lens <= 16; n_lens++) // without and with the read of 1000 bases
        for (uint32_t n : sizes) {
            Batch b;
            make_batch(b, n, n_lens);
            if (n >= 254) { // the reads start at every residue mod 16
                unsigned seen = 0;
                for (uint32_t r = 0; r < n; r++) seen |= 1u << (b.off[r] & 15);
                if (seen != 0xFFFFu) { fprintf(stderr, "read offsets miss a residue mod 16 (%04x)\n", seen); g_bad++; }
            }
            const int ctx_max = n_lens == 16 ? 1500 : 1000; // a context that allows more than the batch's longest read
            for (int paired = 0; paired <= 1; paired++) {
                run_case(b, paired, stride_for(b.longest), (b.longest + 31) / 32 + 1, "stride of the batch's longest read");
                run_case(b, paired, stride_for(ctx_max), (b.longest + 31) / 32 + 1, "stride of the context's maximum");
                run_case(b, paired, stride_for(ctx_max), (ctx_max + 31) / 32 + 1, "stride and parts of the context's maximum");
            }
            if (n_lens == 16) // rows for 256 bases: the reads of 1000 are left out
                run_case(b, 1, stride_for(256), (256 + 31) / 32 + 1, "reads longer than the rows");
        }
    { // reads of one length, the benchmark's shape
        Batch b;
        b.off.assign(1, 0u);
        for (uint32_t r = 0; r < 1000; r++) b.off.push_back(b.off.back() + 150u);
        b.longest = 150;
        b.bytes = (uint8_t *)malloc(b.off.back());
        b.padded = (uint8_t *)aligned_alloc(16, ((size_t)b.off.back() + 64 + 15) & ~(size_t)15);
        for (uint32_t i = 0; i < b.off.back(); i++) b.bytes[i] = (uint8_t)"ACGT"[rnd() & 3];
        memcpy(b.padded, b.bytes, b.off.back()); memset(b.padded + b.off.back(), 'N', 64);
        run_case(b, 1, stride_for(150), (150 + 31) / 32 + 1, "150 bases, rows of 20 words");
        run_case(b, 1, stride_for(256), (150 + 31) / 32 + 1, "150 bases, rows of 28 words");
    }
    if (g_bad) { fprintf(stderr, "pack_check: %d mismatches\n", g_bad); return 1; }
    printf("pack_check: all cases agree\n");
    return 0;
}
