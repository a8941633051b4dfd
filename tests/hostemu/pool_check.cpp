// tests/hostemu/pool_check.cpp — TEST INFRASTRUCTURE: the file front end's thread pool (mcx_pool.h) by itself, on the host: pool_check THREADS ROUNDS.
// Every round calls run() with a part count drawn between 2 and 41 (fixed seed) and jobs that only count their index; after the round every index below the
// count must have run exactly once and none above it.  Exit status 1 on a miscount (a pool that loses a wake-up does not come back at all: the caller's
// time limit sees that).
#include "../../mapcaller_amd/csrc/mcx_pool.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    const int threads = argc > 1 ? atoi(argv[1]) : 8;
    const long rounds = argc > 2 ? atol(argv[2]) : 20000;
    enum { kMost = 41, kSlots = 64 };
    mcx::files::Pool pool(threads);
    std::atomic<int> ran[kSlots];
    for (auto &r : ran) r.store(0);
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    for (long round = 0; round < rounds; round++) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        const int parts = 2 + (int)((seed >> 33) % (kMost - 1));
        pool.run(parts, [&](int k) { ran[k < 0 || k >= kSlots ? kSlots - 1 : k].fetch_add(1, std::memory_order_relaxed); });
        for (int k = 0; k < kSlots; k++) {
            const int got = ran[k].exchange(0), want = k < parts ? 1 : 0;
            if (got != want) { fprintf(stderr, "round %ld, %d parts: index %d ran %d times\n", round, parts, k, got); return 1; }
        }
    }
    printf("%ld rounds on %d threads: every index ran once\n", rounds, threads);
    return 0;
}
