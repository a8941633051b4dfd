// tests/hostemu/aside_guard_check.cpp — the guard of the "heavy pairs aside" path (mapcaller_amd/csrc/mcx_types.h light_pairs_fit) on the host.
//
// run_pairs clusters the heavy pairs on a side stream and gives the light pairs' launch no early list, because a pair with at most kLightHits
// seed hits cannot run over while clustering — as long as the tier's seeding capacities (hit_seed, cand_seed) are at least kLightHits.  The
// context asks light_pairs_fit() once, where tier 0's capacities are made; here the predicate is called on capacities around that bound.
//
//   aside_guard_check     exit status 0 when every case agrees
#include <cstdio>

#include "../../mapcaller_amd/csrc/mcx_types.h"

using namespace mcx;

static int g_bad = 0;

static void expect(int hit_seed, int cand_seed, bool want)
{
    Caps c{};
    c.hit_cap = 88; c.cand_cap = 24; c.hit_seed = hit_seed; c.cand_seed = cand_seed;
    const bool got = light_pairs_fit(c);
    printf("hit_seed %3d cand_seed %3d: aside %s\n", hit_seed, cand_seed, got ? "allowed" : "refused");
    if (got != want) { fprintf(stderr, "  light_pairs_fit(hit_seed %d, cand_seed %d) = %d, want %d\n", hit_seed, cand_seed, (int)got, (int)want); g_bad++; }
}

int main()
{
    static_assert(kLightHits == 8, "the light classes of work_class(): at most 8 hits a pair");
    expect(56, 12, true);                          // tier 0's capacities
    expect(kLightHits, kLightHits, true);          // at the bound
    expect(kLightHits - 1, 12, false);             // a read of a light pair could hold more hits than seeding may fill
    expect(56, kLightHits - 1, false);             // ... or more clusters than candidates may be made of
    expect(kLightHits - 1, kLightHits - 1, false);
    expect(0, 0, false);
    expect(kLightHits, kLightHits - 1, false);
    expect(kLightHits - 1, kLightHits, false);
    if (g_bad) { fprintf(stderr, "aside_guard_check: %d mismatches\n", g_bad); return 1; }
    printf("aside_guard_check: all cases agree\n");
    return 0;
}
