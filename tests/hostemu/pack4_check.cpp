// tests/hostemu/pack4_check.cpp — the read packer's arithmetic (mapcaller_amd/csrc/mcx_pack.h) on the host, piece by piece:
//
//   pack4        every byte value 0..255 at each of the four byte positions of a word, the other three bytes drawn from "ACGTacgtNn" and from
//                random bytes, both strands, with and without the odd flags: codes, N flags and lower-case flags against nt4_code() (mcx_fm.h)
//                and "bit 5 set", byte by byte
//   pack16_span  reads of 16 to 83 bytes that start at every byte offset 0..15 of a 16-byte word, both strands, every span of theirs (whole
//                ones and the last, partial one), each read seen through a buffer of exactly the aligned 16-byte words that hold its bytes, so
//                that under -fsanitize=address a load outside them stops the program: the code word and the flags against pack_read()'s
//
//   pack4_check           runs every case; exit status 0 when all agree
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mapcaller_amd/csrc/mcx_pack.h"

using namespace mcx;

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 24);
}

static int g_bad = 0;

// what four bytes (first base in the low byte) must give, from nt4_code() alone
static void want4(uint32_t w, bool comp, uint32_t &codes, uint32_t &flags, uint32_t &lower)
{
    codes = flags = lower = 0;
    for (int j = 0; j < 4; j++) {
        const uint8_t b = (uint8_t)(w >> (8 * j));
        const int c = nt4_code(b);
        const uint32_t code = c > 3 ? 0u : (uint32_t)(comp ? 3 - c : c);
        codes |= code << (6 - 2 * j);
        flags |= (c > 3 ? 1u : 0u) << (3 - j);
        lower |= (uint32_t)((b >> 5) & 1) << (3 - j);
    }
}

static void check4(uint32_t w)
{
    for (int comp = 0; comp <= 1; comp++) {
        uint32_t wc, wf, wl, c, f, l;
        want4(w, comp != 0, wc, wf, wl);
        pack4<true>(w, comp != 0, c, f, l);
        if (c != wc || f != wf || l != wl) {
            if (g_bad++ < 20) fprintf(stderr, "  pack4<true>(%08x, %d): got %02x %x %x, want %02x %x %x\n", w, comp, c, f, l, wc, wf, wl);
        }
        pack4<false>(w, comp != 0, c, f, l);
        if (c != wc || f != wf || l != 0) {
            if (g_bad++ < 20) fprintf(stderr, "  pack4<false>(%08x, %d): got %02x %x %x, want %02x %x 0\n", w, comp, c, f, l, wc, wf);
        }
    }
}

static void every_byte_value()
{
    static const char kLetters[] = "ACGTacgtNn";
    const int before = g_bad;
    uint64_t n = 0;
    for (int pos = 0; pos < 4; pos++)
        for (uint32_t v = 0; v < 256; v++)
            for (int rep = 0; rep < 64; rep++) {
                uint32_t w = 0;
                for (int j = 0; j < 4; j++) {
                    const uint32_t other = rep < 32 ? (uint32_t)(uint8_t)kLetters[rnd() % 10] : (rnd() & 0xFFu);
                    w |= (j == pos ? v : other) << (8 * j);
                }
                check4(w); n++;
            }
    for (uint32_t v = 0; v < 256; v++) check4(v * 0x01010101u); // the same byte four times
    printf("%-44s %8llu words x 2 strands x 2 forms: %s\n", "pack4, every byte value at every position", (unsigned long long)n + 256, g_bad == before ? "ok" : "MISMATCH");
}

// a read of rlen bytes that starts at byte `sh` of an aligned word: every span against pack_read()
static void spans_of(int rlen, int sh, int kind)
{
    static const char kOddLetters[] = "NnacgtRYKMSWBDHVrykmswbdhvUu.-*";
    const size_t n16 = ((size_t)sh + rlen + 15) / 16;
    U4 *buf = (U4 *)aligned_alloc(16, n16 * 16); // exactly the words that hold a byte of the read
    uint8_t *bytes = (uint8_t *)buf;
    for (size_t i = 0; i < n16 * 16; i++) bytes[i] = (uint8_t)rnd(); // (what lies around the read is anything)
    for (int i = 0; i < rlen; i++) {
        uint8_t ch = (uint8_t)"ACGT"[rnd() & 3];
        if (kind == 1 && rnd() % 8 == 0) ch = (uint8_t)kOddLetters[rnd() % (sizeof kOddLetters - 1)];
        if (kind == 2 && rnd() % 4 == 0) ch = (uint8_t)rnd();
        bytes[sh + i] = ch;
    }
    for (int flipped = 0; flipped <= 1; flipped++) {
        std::vector<uint32_t> ref((size_t)packed_words(rlen) + 4);
        ReadRef rd; rd.ascii = bytes + sh; rd.rlen = rlen; rd.flipped = flipped;
        PackedRead pk; pk.w = ref.data(); pk.stride = 1; pk.n_code = 0;
        pack_read(rd, pk);
        const int nc = (rlen + 15) >> 4;
        for (int i0 = 0; i0 < rlen; i0 += 16) {
            const uint32_t want_c = ref[i0 >> 4], mw = ref[nc + 1 + (i0 >> 5)], want_f = (i0 & 16) ? (mw & 0xFFFFu) : (mw >> 16);
            const int n = rlen - i0 < 16 ? rlen - i0 : 16;
            uint32_t want_o = 0; // bytes of the span that are not an upper-case A C G T (bit 15 = base i0)
            for (int k = 0; k < n; k++) {
                const uint8_t ch = bytes[sh + (flipped ? rlen - 1 - (i0 + k) : i0 + k)];
                if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') want_o |= 1u << (15 - k);
            }
            uint32_t c, f, o;
            pack16_span<true>(buf, (uint64_t)sh, rlen, flipped, i0, c, f, o);
            if (c != want_c || f != want_f || o != want_o) {
                if (g_bad++ < 20) fprintf(stderr, "  pack16_span<true>: rlen %d offset %d flipped %d span %d: got %08x %04x %04x, want %08x %04x %04x\n", rlen, sh, flipped, i0, c, f, o, want_c, want_f, want_o);
            }
            pack16_span<false>(buf, (uint64_t)sh, rlen, flipped, i0, c, f, o);
            if (c != want_c || f != want_f || o != 0) {
                if (g_bad++ < 20) fprintf(stderr, "  pack16_span<false>: rlen %d offset %d flipped %d span %d: got %08x %04x %04x, want %08x %04x 0\n", rlen, sh, flipped, i0, c, f, o, want_c, want_f);
            }
        }
    }
    free(buf);
}

static void spans_at_every_offset()
{
    const int before = g_bad;
    int n = 0;
    for (int rlen = 16; rlen <= 83; rlen++)
        for (int sh = 0; sh < 16; sh++)
            for (int kind = 0; kind < 3; kind++) { spans_of(rlen, sh, kind); n++; }
    for (int rlen = 1; rlen < 16; rlen++) // (reads shorter than a span: the aligned words' path)
        for (int sh = 0; sh < 16; sh++) { spans_of(rlen, sh, 1); n++; }
    printf("%-44s %8d reads x 2 strands x 2 forms: %s\n", "pack16_span, every offset of the read start", n, g_bad == before ? "ok" : "MISMATCH");
}

int main()
{
    every_byte_value();
    spans_at_every_offset();
    if (g_bad) { fprintf(stderr, "pack4_check: %d mismatches\n", g_bad); return 1; }
    printf("pack4_check: all cases agree\n");
    return 0;
}
