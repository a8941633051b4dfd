// tests/hostemu/deflate_check.cpp — the device's deflater (mapcaller_amd/csrc/mcx_deflate.h) compiled for the host, as a stand-alone program: tests/test_deflate_host.py
// builds it twice (plain, and with -fsanitize=address,undefined) and runs it on a file of vectors.
//   in:  per vector  u32 block (text bytes per BGZF block), u32 n, n bytes of text
//   out: per vector  u32 bytes, then the BGZF blocks of the text back to back (no EOF block)
// Every block is compressed into a slot of its own with 64 guard bytes on either side, and so is every assembled member; a guard byte that changed, or a
// stream longer than its text + 5, ends the program with status 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mapcaller_amd/csrc/mcx_deflate.h"

namespace {
enum { kGuard = 64 };
bool guards_ok(const uint8_t *p, size_t inner)
{
    for (size_t i = 0; i < kGuard; i++) if (p[i] != 0xA5 || p[kGuard + inner + i] != 0xA5) return false;
    return true;
}
bool read_u32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }
} // namespace

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: deflate_check <vector file> <output file>\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "deflate_check: cannot open the files\n"); return 2; }
    static uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; i++) crc_tab[i] = mcx::inf::crc_table_entry(i);
    mcx::def::Work *W = new mcx::def::Work;
    uint32_t block = 0, n = 0, n_vec = 0;
    while (read_u32(in, block) && read_u32(in, n)) {
        if (block < 1 || block > mcx::def::kMaxBlock) { fprintf(stderr, "deflate_check: vector %u: block size %u\n", n_vec, block); return 2; }
        // (the text in a buffer of exactly its size: the sanitizer sees a read behind it)
        uint8_t *text = (uint8_t *)malloc(n ? n : 1);
        if (n && fread(text, 1, n, in) != n) { fprintf(stderr, "deflate_check: vector %u is cut short\n", n_vec); return 2; }
        std::vector<uint8_t> all;
        for (uint32_t at = 0; at < n; at += block) {
            const uint32_t len = n - at < block ? n - at : block;
            const uint32_t slot_bytes = mcx::def::slot_bytes_of(len);
            uint32_t *slot_mem = (uint32_t *)malloc(kGuard + slot_bytes + kGuard); // (malloc: aligned for the words the encoder stores)
            uint8_t *slot = (uint8_t *)slot_mem;
            memset(slot, 0xA5, kGuard + slot_bytes + kGuard);
            uint32_t crc = 0;
            const uint32_t payload = mcx::def::deflate_block(text + at, len, slot + kGuard, slot_bytes, *W, crc_tab, 0, &crc);
            if (!guards_ok(slot, slot_bytes)) { fprintf(stderr, "deflate_check: vector %u, block at %u: a guard byte of the slot changed\n", n_vec, at); return 1; }
            if (payload > len + 5) { fprintf(stderr, "deflate_check: vector %u, block at %u: %u bytes for %u of text\n", n_vec, at, payload, len); return 1; }
            const uint32_t member = payload + mcx::def::kMemberExtra;
            uint8_t *m = (uint8_t *)malloc(kGuard + member + kGuard);
            memset(m, 0xA5, kGuard + member + kGuard);
            for (uint32_t i = 0; i < member; i++) m[kGuard + i] = mcx::def::member_byte(i, slot + kGuard, payload, crc, len);
            if (!guards_ok(m, member)) { fprintf(stderr, "deflate_check: vector %u, block at %u: a guard byte of the member changed\n", n_vec, at); return 1; }
            all.insert(all.end(), m + kGuard, m + kGuard + member);
            free(m); free(slot_mem);
        }
        const uint32_t bytes = (uint32_t)all.size();
        fwrite(&bytes, 4, 1, out);
        if (bytes) fwrite(all.data(), 1, bytes, out);
        free(text);
        n_vec++;
    }
    delete W;
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("deflate_check: %u vectors\n", n_vec);
    return 0;
}
