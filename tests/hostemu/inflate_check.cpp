// tests/hostemu/inflate_check.cpp — the device's inflater (mapcaller_amd/csrc/mcx_inflate.h) compiled for the host: tests/test_inflate_device.py holds it
// against zlib's output.  Built by the test with its own compiler commands, not by this directory's Makefile: once as a shared library (g++ -shared), and
// once as a stand-alone program (-DINFLATE_CHECK_MAIN, with -fsanitize=address,undefined) that reads a file of members and runs every one of them.
#include "../../mapcaller_amd/csrc/mcx_inflate.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {
const uint32_t *crc_table()
{
    static uint32_t tab[256];
    static bool made = false;
    if (!made) { for (uint32_t i = 0; i < 256; i++) tab[i] = mcx::inf::crc_table_entry(i); made = true; }
    return tab;
}
} // namespace

// One member through inflate_member as the kernel calls it (one lane).  longest (may be null): the longest literal / length and distance code the
// stream's dynamic headers declared, and its number of blocks.  Returns the member's mcx_inflate_status.
extern "C" uint32_t inflate_check_member(const uint8_t *src, uint32_t src_len, uint32_t readable, uint8_t *dst, uint32_t isize, uint32_t crc, uint32_t *longest)
{
    static thread_local mcx::inf::Tables t;
    mcx::inf::Info info = {0, 0, 0};
    const uint32_t st = mcx::inf::inflate_member(src, src_len, readable, dst, isize, crc, t, crc_table(), 0, &info);
    if (longest) { longest[0] = info.max_lit_len; longest[1] = info.max_dist_len; longest[2] = info.blocks; }
    return st;
}

#ifdef INFLATE_CHECK_MAIN
// The file: u32 n, then per member  u32 src_len, isize, crc, expect, text_len;  src_len bytes;  text_len bytes (the text, when expect is 0).
// expect: 0 the status must be 0 and the text equal; 1 .. 4 exactly that status; 255 any status but 0.
// Every member runs twice in buffers of exactly the sizes the contract names (so that the sanitizer sees any byte read or written outside them): with eight
// bytes of slack behind the input, and with none.  One line per member: index, status, longest literal / length code, longest distance code.
int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: inflate_check <vector file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    int bad = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t h[5];
        if (fread(h, 4, 5, f) != 5) { fprintf(stderr, "short file\n"); return 2; }
        const uint32_t src_len = h[0], isize = h[1], crc = h[2], expect = h[3], text_len = h[4];
        std::vector<uint8_t> src(src_len), text(text_len);
        if (src_len && fread(src.data(), 1, src_len, f) != src_len) return 2;
        if (text_len && fread(text.data(), 1, text_len, f) != text_len) return 2;
        uint32_t st[2] = {0, 0}, longest[3] = {0, 0, 0};
        for (int slack = 0; slack < 2; slack++) {
            const uint32_t readable = src_len + (slack ? 8u : 0u);
            uint8_t *in = (uint8_t *)malloc(readable ? readable : 1), *out = (uint8_t *)malloc(isize && isize <= 65536 ? isize : 1);
            if (src_len) memcpy(in, src.data(), src_len);
            if (slack) memset(in + src_len, 0xFF, 8); // (what lies behind a member is never consumed, whatever it is)
            st[slack] = inflate_check_member(in, src_len, readable, out, isize, crc, longest);
            if (st[slack] == 0 && expect == 0 && (text_len != isize || (isize && memcmp(out, text.data(), isize) != 0))) { printf("# member %u: the text differs\n", i); bad++; }
            free(in); free(out);
        }
        if (st[0] != st[1]) { printf("# member %u: status %u without slack, %u with\n", i, st[0], st[1]); bad++; }
        if (expect == 255 ? st[0] == 0 : st[0] != expect) { printf("# member %u: status %u, expected %u\n", i, st[0], expect); bad++; }
        printf("%u %u %u %u\n", i, st[0], longest[0], longest[1]);
    }
    fclose(f);
    return bad ? 1 : 0;
}
#endif
