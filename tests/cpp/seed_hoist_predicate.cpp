// seeds_launch_invariant (toyni_amd/csrc/ntt_route.hpp) against a brute-force walk of every workgroup's tile sequence: the launcher
// tells a column pass to look its twiddle seeds up once per launch exactly where this predicate holds, so it must never hold for a
// launch in which some workgroup changes its column tile.
//
// TEST INFRASTRUCTURE (tests/test_seed_hoist_predicate.py).  The walk uses the kernels' own maps: Pass::tile_order for the tile a
// workgroup runs at virtual index v = b, b + grid, ..., and Pass::tile_of for the first column (col0) of that tile.
// Build: g++ -O2 -std=c++17 -I toyni_amd/csrc tests/cpp/seed_hoist_predicate.cpp
#include <cstdio>
#include <vector>

#include "ntt_plan.hpp"

using namespace toyni;

static_assert(seeds_launch_invariant(256, 32768, 10, 5), "the benchmark's column pass: 32 tiles per prefix, 256 workgroups");
static_assert(!seeds_launch_invariant(304, 32768, 10, 5), "304 workgroups are no multiple of 32 tiles per prefix");
static_assert(!seeds_launch_invariant(256, 1u << 17, 16, 6), "first pass of 2^24: 1024 tiles per prefix, more than the grid");
static_assert(seeds_launch_invariant(256, 1u << 17, 8, 6), "middle pass of 2^24: 4 tiles per prefix");

static unsigned long long checked = 0, held = 0, conservative = 0;
static int failures = 0;

template <class P, uint32_t LC>
static bool brute_force(uint32_t grid, uint32_t ntiles, uint32_t log_S) {
    static_assert(P::C == (1u << LC), "tile width");
    PassArgs a{};
    a.log_S = log_S;
    a.in_prefix_log = log_S + P::LM;
    for (uint32_t b = 0; b < grid && b < ntiles; ++b) {
        const uint32_t first = P::tile_of(a, P::tile_order(b, ntiles)).col0;
        for (uint32_t v = b; v < ntiles; v += grid)
            if (P::tile_of(a, P::tile_order(v, ntiles)).col0 != first) return false;
    }
    return true;
}

template <class P, uint32_t LC>
static void check_shape() {
    const uint32_t exact_grids[] = {1, 32, 48, 256, 304, 512};            // a launch the predicate rejects must really change tiles
    const uint32_t sound_grids[] = {2, 3, 4, 8, 16, 24, 40, 64, 80, 100};   // here it may be conservative, never wrong
    const uint32_t batches[] = {1, 2, 3, 5, 8, 16, 24, 33};               // tiles = tiles per prefix x batch: multiples of 16 and not
    for (uint32_t tiles_log = 0; tiles_log <= 10; ++tiles_log)
        for (uint32_t batch : batches) {
            const uint32_t log_S = tiles_log + LC, ntiles = batch << tiles_log;
            for (int exact = 1; exact >= 0; --exact)
                for (uint32_t grid : exact ? std::vector<uint32_t>(exact_grids, exact_grids + 6) : std::vector<uint32_t>(sound_grids, sound_grids + 10)) {
                    const bool pred = seeds_launch_invariant(grid, ntiles, log_S, LC), brute = brute_force<P, LC>(grid, ntiles, log_S);
                    ++checked;
                    held += pred;
                    if (pred && !brute) { ++failures; std::printf("FAIL unsound: C=%u tiles/prefix=2^%u tiles=%u grid=%u\n", P::C, tiles_log, ntiles, grid); }
                    if (!pred && brute) {
                        if (exact) { ++failures; std::printf("FAIL not exact: C=%u tiles/prefix=2^%u tiles=%u grid=%u\n", P::C, tiles_log, ntiles, grid); }
                        else ++conservative;
                    }
                }
        }
}

int main() {
    check_shape<Pass<KIND_COL, 5, 5, 3>, 3>();
    check_shape<Pass<KIND_COL, 5, 5, 4>, 4>();
    check_shape<Pass<KIND_COL, 5, 5, 5>, 5>();
    check_shape<Pass<KIND_COL, 4, 4, 6>, 6>();
    std::printf("checked %llu launches: predicate true for %llu, conservative for %llu\n", checked, held, conservative);
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "ALL OK", failures);
    return failures ? 1 : 0;
}
