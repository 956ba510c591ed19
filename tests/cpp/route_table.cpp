// The launch route of a transform call (toyni_amd/csrc/ntt_route.hpp) as a table: for each named knob profile and each point of a
// grid of (log_n, batch, lq, log_blowup, chunk_elems) one line with the Route's fields and, for a passes route, the shape every pass
// dispatches to (walked through for_each_pass with a launch that launches nothing).  CPU only, no HIP:
//   g++ -std=c++17 -I toyni_amd/csrc -o build/route_table tests/cpp/route_table.cpp
// tests/test_route_table.py compares the output byte for byte with tests/golden/route_table.txt.
// The `default` block takes its knobs from the environment (launch_knobs()); every other profile writes the struct.
#include <cstdio>
#include <map>
#include <tuple>
#include <vector>

#include "ntt_plan.hpp"

using namespace toyni;

struct Case { int log_n; uint64_t batch; int lq, z; uint64_t chunk_elems; };

struct Profile {
    const char* name;
    int lo, hi;       // sizes 2^lo .. 2^hi of the grid: what the profile's knobs can move
    bool lde;         // with the low-degree extensions of the grid
    LaunchKnobs k;
};

static const NttPlan& plan_of(const LaunchKnobs& k, int log_n, bool latency) {
    static std::map<std::tuple<const LaunchKnobs*, int, bool>, NttPlan> cache;
    NttPlan& p = cache[{&k, log_n, latency}];
    if (p.fwd.empty()) build_plan(k, log_n, p, latency);
    return p;
}

// The points where a decision flips (tests/test_route_table.py lists them)
static std::vector<Case> grid(const Profile& pf) {
    std::vector<Case> g;
    auto add = [&](int log_n, uint64_t batch, int lq = 0, int z = 0, uint64_t ce = 0) {
        if (log_n < pf.lo || log_n > pf.hi || (z && !pf.lde) || z > log_n) return;
        for (const Case& c : g)
            if (c.log_n == log_n && c.batch == batch && c.lq == lq && c.z == z && c.chunk_elems == ce) return;
        g.push_back({log_n, batch, lq, z, ce});
    };
    for (int log_n = 0; log_n <= 27; ++log_n) { add(log_n, 1); add(log_n, 3); }
    for (int log_n : {11, 12}) { add(log_n, 2047); add(log_n, 2048); }                             // the row sweeps' threshold
    for (int log_n : {13, 14, 15}) { add(log_n, (1ull << (25 - log_n)) - 1); add(log_n, 1ull << (25 - log_n)); }   // the LDS sweep's
    add(16, 1ull << 9);                                                                             // 2^25 elements of 2^16: passes
    for (uint64_t b : {1, 4, 64}) add(21, b);
    for (uint64_t b : {1, 2, 3, 64}) add(22, b);
    for (int log_n : {20, 21, 22}) { add(log_n, 1, 2); add(log_n, 4, 2); }                          // Ext vectors
    for (int log_n : {12, 16, 20, 21, 22, 23}) {
        const int m0 = plan_of(pf.k, log_n, false).pass[0].log_m;
        for (int lq : {0, 2})
            for (uint64_t b : {1, 4})
                for (int z : {1, 2, 3, 4, 5, m0, m0 + 1}) add(log_n, b, lq, z);
    }
    for (int log_n : {21, 22})                                                                      // `pad` today
        for (int lq : {0, 2})
            for (int z : {8, 10, 11}) add(log_n, 1, lq, z);
    add(20, 16, 0, 0, 1ull << 22);                                                                  // a chunked context
    add(21, 3, 2, 0, 1ull << 22);                                                                   // ... whose chunk rounds to 4
    add(20, 127); add(20, 128);                                                                     // 512 MiB: the non-temporal twins
    add(7, (1ull << 20) - 1); add(7, 1ull << 20);                                                   // ... never under 256 words
    return g;
}

template <class P> struct KindOf { static constexpr int value = P::PASS_KIND; };
template <int K, int A, int B, int D, int C, bool N, int Q> struct KindOf<Pass3<K, A, B, D, C, N, Q>> { static constexpr int value = K; };

template <int LQ>
static void print_shapes(const LaunchKnobs& k, const NttPlan& plan, const Route& r, uint64_t nb) {
    const bool ok = for_each_pass<LQ>(k, plan, plan.fwd.data(), false, nullptr, nullptr, nullptr, nb, [](auto pass, auto lzc, const PassArgs&, uint64_t) {
        using P = decltype(pass);
        bool stream = false;
        if constexpr (P::STEPS == 3) stream = P::STREAM;
        std::printf(" [s%d m%d c%u k%d st%d nt%d q%d z%d]", P::STEPS, P::LM, (unsigned)P::C, KindOf<P>::value, (int)stream, (int)P::NT, P::LQ, (int)decltype(lzc)::value);
    }, CosetTables(), r.lde_log, r.nt);
    if (!ok) std::printf(" NO-SHAPE");
}

static void print_block(const Profile& pf) {
    static const char* kinds[] = {"copy", "row", "lds", "passes"};
    std::printf("## %s\n", pf.name);
    for (const Case& c : grid(pf)) {
        const NttPlan& plan = plan_of(pf.k, c.log_n, false);
        const NttPlan* lat = has_latency_plan(c.log_n) ? &plan_of(pf.k, c.log_n, true) : nullptr;
        const Route r = route_transform(plan, lat, c.batch, c.lq, c.z, c.chunk_elems, pf.k);
        std::printf("n%d b%llu q%d z%d ce%llu: %s lat%d pad%d lz%d nt%d chunk%llu launches%d", c.log_n, (unsigned long long)c.batch, c.lq, c.z,
                    (unsigned long long)c.chunk_elems, kinds[r.kind], (int)r.lat, (int)r.pad, r.lde_log, (int)r.nt, (unsigned long long)r.chunk, r.launches);
        if (r.kind == ROUTE_PASSES) {
            const NttPlan& run = r.lat ? *lat : plan;
            const uint64_t batch = c.batch << c.lq, first = batch < r.chunk ? batch : r.chunk, tail = batch % r.chunk;
            if (c.lq) print_shapes<2>(pf.k, run, r, first); else print_shapes<0>(pf.k, run, r, first);
            if (tail) {   // the last launch sequence of a chunked call is shorter
                std::printf(" tail%llu", (unsigned long long)tail);
                if (c.lq) print_shapes<2>(pf.k, run, r, tail); else print_shapes<0>(pf.k, run, r, tail);
            }
        }
        std::printf("\n");
    }
}

int main() {
    auto with = [](auto set) { LaunchKnobs k; set(k); return k; };
    // (two_step_nt keeps the whole grid: the test runs `default` under its environment and compares the two blocks)
    static const Profile profiles[] = {
        {"default", 0, 27, true, launch_knobs()},
        // tests/dispatch_matrix.py: PROFILE_ENV
        {"nt", 7, 22, false, with([](LaunchKnobs& k) { k.nt_min_bytes = 0; })},
        {"two_step", 11, 22, true, with([](LaunchKnobs& k) { k.p3_tiles = -1; })},
        {"two_step_nt", 0, 27, true, with([](LaunchKnobs& k) { k.p3_tiles = -1; k.nt_min_bytes = 0; })},
        {"wide", 13, 23, false, with([](LaunchKnobs& k) { k.p3_tiles = -1; k.wide_tiles = 0; })},
        {"wide_nt", 13, 23, false, with([](LaunchKnobs& k) { k.p3_tiles = -1; k.wide_tiles = 0; k.nt_min_bytes = 0; })},
        {"lds", 11, 16, false, with([](LaunchKnobs& k) { k.lds_min_elems = 0; k.lds_max_log = 15; k.lds_rows = 4; })},
        {"s3_tiles_99", 21, 22, true, with([](LaunchKnobs& k) { k.s3_tiles = 99; })},
        {"s3_tiles_8", 21, 22, true, with([](LaunchKnobs& k) { k.s3_tiles = 8; })},
        {"lat_tiles_-1", 21, 22, true, with([](LaunchKnobs& k) { k.lat_tiles = -1; })},
        {"split_small_first_0", 11, 27, true, with([](LaunchKnobs& k) { k.split_small_first = false; })},
    };
    for (const Profile& pf : profiles) print_block(pf);
    return 0;
}
