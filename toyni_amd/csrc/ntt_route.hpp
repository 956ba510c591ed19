// Which kernels a transform call runs, decided ONCE and as a value: the knobs of the environment that steer the decision (LaunchKnobs)
// and the decision itself (Route, route_transform).  toyni_hip.hip switches on the Route, ntt_plan.hpp reads the knobs where it splits a
// size and picks a pass shape, tests/cpp/route_table.cpp prints the whole table on the CPU.  Plain C++, no HIP and no plan types:
// ntt_plan.hpp includes this header, so the plan is a template parameter here (Plan = NttPlan).
#pragma once
#include <cstdlib>
#include <stdint.h>

namespace toyni {

inline int env_int(const char* name, int dflt) { const char* env = std::getenv(name); return env ? std::atoi(env) : dflt; }
inline uint64_t env_u64(const char* name, uint64_t dflt) { const char* env = std::getenv(name); return env ? (uint64_t)std::strtoull(env, nullptr, 0) : dflt; }

// Every knob that influences which kernels a transform runs: the list of record.  The library reads launch_knobs(); tests/emu and
// tests/cpp/route_table.cpp fill a struct of their own to step / tabulate the other settings.
struct LaunchKnobs {
    // TOYNI_P3_TILES.  Launches of at most 2^p3_tiles 32-wide tiles (a single transform, or a handful: the data is cache-resident
    // and the chip is far from full) run the three-step shapes `Pass3` with 4-wide tiles instead: 8x the workgroups of the 32-wide
    // shape and half the serial work per wave.  -1 = never the three-step shapes.
    int p3_tiles = 6;
    // TOYNI_LAT_TILES.  Launches whose first pass has at most this many (log2) 32-wide tiles' worth of columns take the two-pass
    // latency plan of n = 2^21 / 2^22 (has_latency_plan).  -1 = never.
    int lat_tiles = 7;
    // TOYNI_WIDE_TILES.  Launches of at least this many (log2) 32-wide tiles take the 64-wide shapes (dispatch_pass).  99 = never.
    int wide_tiles = 12;
    // TOYNI_S3_TILES.  Launches of at least this many (log2) 32-wide tiles run a 2048-point pass in its streaming three-step shape (16-wide
    // tiles, 32 elements per thread, ntt_pass3s_kernel) and n = 2^21 as the two sweeps of its "latency" plan; 99 = never (the three-pass plan).
    int s3_tiles = 7;
    // TOYNI_SPLIT_SMALL_FIRST.  Uneven splits: which pass gets the extra stage.  A column pass also applies the inter-pass twiddle and
    // reads strided; the closing row pass does neither -- so the larger factor goes LAST (experiment switch, 0: first, as in round 1).
    bool split_small_first = true;
    // TOYNI_SPLIT3="a,b,c" (experiment switch): that split for the size a + b + c (column shapes exist for 6..10 stage bits, closing
    // row shapes for 5..10: split_passes checks the window); the A/B of profiles/r05_ab_split3.txt.  0,0,0 = none.
    int split3[3] = {0, 0, 0};
    // TOYNI_LDS_MAX_LOG (TOYNI_NO_LDS_KERNEL=1: 10) / TOYNI_LDS_MIN_ELEMS.  When the single-sweep kernel runs instead of the two-pass
    // plan: sizes 2^13 .. 2^lds_max_log (default 13; 10 = never; 2^11 / 2^12: Row2048 / Row4096 since round 5, 15 = every size it
    // exists for) and launches of at least lds_min_elems elements (default 2^25).  Measured (profiles/r01_sweep_lds.txt): it halves
    // the HBM traffic and is 5-19 % faster on large batches of 2^11 .. 2^13, but the sweep is VALU-bound where the two-pass plan is
    // HBM-bound, so from 2^14 on the two-pass plan wins; and a lone transform is one 256-thread workgroup's serial work here (7.7-9.6
    // us) against two launches of many small workgroups (5.6-6.8 us).
    int lds_max_log = 13;
    uint64_t lds_min_elems = (uint64_t)1 << 25;
    // TOYNI_LDS_ROWS = 3 | 4 | 5.  Rows per workgroup of the single-sweep kernel, as a power of two (8 rows = four 256-thread workgroups per CU measured best).
    int lds_rows = 3;
    // TOYNI_R2048_MIN_ROWS.  n = 2^11: the one-wave-per-transform kernel from this many transforms up (default 2048 -- measured crossover with the
    // two-pass plan: 19.2 us either way at 2048 rows, 22.0 against 30.1 us at 4096, 0.485 against 0.736 ms at 2^17; 0 = always, a huge value = never).
    uint64_t r2048_min_rows = 2048;
    // TOYNI_R4096_MIN_ROWS.  n = 2^12: the two-waves-per-transform kernel from this many transforms up (default 2048 -- measured crossover with the
    // two-pass plan: 21.2 against 18.4 us at 1024 rows, 24.1 against 29.6 at 2048, 0.568 against 0.772 ms at 2^16; 0 = always, a huge value = never).
    uint64_t r4096_min_rows = 2048;
    // TOYNI_NT_MIN_BYTES.  Footprint (bytes of one launch's data) from which the pass kernels use non-temporal loads / stores;
    // default 512 MiB = twice the Infinity Cache (0 = always, a huge value = never).
    uint64_t nt_min_bytes = (uint64_t)512 << 20;

    static LaunchKnobs from_env() {
        LaunchKnobs k;
        k.p3_tiles = env_int("TOYNI_P3_TILES", k.p3_tiles);
        k.lat_tiles = env_int("TOYNI_LAT_TILES", k.lat_tiles);
        k.wide_tiles = env_int("TOYNI_WIDE_TILES", k.wide_tiles);
        k.s3_tiles = env_int("TOYNI_S3_TILES", k.s3_tiles);
        if (const char* env = std::getenv("TOYNI_SPLIT_SMALL_FIRST")) k.split_small_first = env[0] != '0';
        if (const char* env = std::getenv("TOYNI_SPLIT3")) {   // element i of the comma-separated list (0 where the list ends early)
            for (int i = 0; i < 3; ++i) {
                k.split3[i] = std::atoi(env);
                while (*env && *env != ',') ++env;
                if (!*env) break;
                ++env;
            }
        }
        k.lds_max_log = env_int("TOYNI_LDS_MAX_LOG", k.lds_max_log);
        if (const char* env = std::getenv("TOYNI_NO_LDS_KERNEL")) if (env[0] == '1') k.lds_max_log = 10;
        k.lds_min_elems = env_u64("TOYNI_LDS_MIN_ELEMS", k.lds_min_elems);
        k.lds_rows = env_int("TOYNI_LDS_ROWS", k.lds_rows);
        k.r2048_min_rows = env_u64("TOYNI_R2048_MIN_ROWS", k.r2048_min_rows);
        k.r4096_min_rows = env_u64("TOYNI_R4096_MIN_ROWS", k.r4096_min_rows);
        k.nt_min_bytes = env_u64("TOYNI_NT_MIN_BYTES", k.nt_min_bytes);
        return k;
    }
};

// The process-wide knobs: read from the environment ONCE (a function-local static is initialised thread-safely), never written afterwards.
inline const LaunchKnobs& launch_knobs() {
    static const LaunchKnobs k = LaunchKnobs::from_env();
    return k;
}

// Whether every workgroup of a persistent KIND_COL launch stays on ONE column tile: workgroup b runs the tiles tile_order(v, ntiles),
// v = b, b + grid, ..., and tile `bid` covers the columns (bid mod 2^(log_S - LC)) << LC of its prefix block.  The inter-pass twiddle
// seeds and the forward coset seed of a thread depend on the tile through that column index alone, so where this holds the launcher
// tells the kernel to look them up once per launch instead of once per tile (PassArgs::seeds_invariant).
//   * grid >= ntiles: a workgroup has one tile;
//   * otherwise v -> v + grid must move the tile index by a multiple of the tiles per prefix.  tile_order is the identity when ntiles
//     is no multiple of 16, and otherwise permutes the low four bits of v only: with grid a multiple of 16 the step is exactly
//     `grid` either way.  A paired launch whose grid is NOT a multiple of 16 changes those four bits from tile to tile and with
//     them the column tile (for more than one tile per prefix): excluded, persistent_grid never makes one.
constexpr bool seeds_launch_invariant(uint64_t grid, uint64_t ntiles, uint32_t log_S, uint32_t LC) {
    if (grid == 0 || log_S < LC) return false;
    if (grid >= ntiles) return true;
    const uint32_t tiles_log = log_S - LC;
    if (tiles_log == 0) return true;
    if (tiles_log >= 32) return false;
    if ((grid & (((uint64_t)1 << tiles_log) - 1)) != 0) return false;
    return (ntiles & 15) != 0 || (grid & 15) == 0;
}

// latency = true: the SECOND plan of n = 2^21 / 2^22, two passes with a 2048-point three-step pass.  Rounds 2-4: 4-wide latency tiles
// only -- one launch fewer for a lone transform -- while streaming launches kept the three-pass split below.  Round 5: the 2048-point
// pass also has a STREAMING shape (16-wide tiles, 32 elements per thread), so n = 2^21 runs this plan for launches of every size
// (has_stream2_plan), n = 2^22 for lone transforms and for its low-degree extensions (use_two_pass_plan)
// (n = 2^23 / 2^24 as 4096-point three-step passes were built and measured too: 54.6 against 50.7 us and 124 against 88 us for the
// three-pass plan -- a 4096 x 4 tile is one 1024-thread workgroup per CU with 16-byte row segments; not kept)
inline bool has_latency_plan(int log_n) { return log_n == 21 || log_n == 22; }
// Sizes whose two-pass plan beats the three-pass one on streaming launches.  n = 2^21: 1024-point column pass + 2048-point closing
// pass, 1.05 against 1.32 ms per 2^28 elements.  n = 2^22 as two 2048-point passes was built and measured too and is NOT taken
// (profiles/r05_ab_stream3.txt): 1.28-1.33 ms against 1.24-1.27 for 7/7/8 -- a 16-column tile means 64-byte row segments on both
// sides of the column pass, and with the inter-pass twiddle that pass takes 0.71 ms where the closing pass takes 0.57.  What the
// 16-wide column shape is kept for is the FIRST pass of a low-degree extension of n = 2^22 (it reads 2^-blow-up of its input:
// 0.95 against 1.21 ms for 64 x 2^17 -> 2^22), so only its zero-fraction variants are instantiated (dispatch_pass_lz).
inline bool has_stream2_plan(int log_n) { return log_n == 21; }

template <class Plan> inline bool row2048_enabled(const Plan& plan, uint64_t batch, const LaunchKnobs& k) {
    if (batch < 1) return false;
    return (plan.log_n == 11 && batch >= k.r2048_min_rows) || (plan.log_n == 12 && batch >= k.r4096_min_rows);
}
template <class Plan> inline bool lds_kernel_enabled(const Plan& plan, uint64_t batch, const LaunchKnobs& k) {
    return plan.lds_la != 0 && plan.log_n <= k.lds_max_log && (batch << plan.log_n) >= k.lds_min_elems;
}

// Which plan a launch of `batch` base-field transforms takes at n = 2^21 / 2^22 (the sizes with a second, two-pass plan; plan_lat
// == nullptr elsewhere):
//   * a lone transform (or a few): the two-pass plan in its 4-wide latency shapes, while its first pass has at most
//     2^lat_tiles 32-wide tiles' worth of columns;
//   * (round 5) launches of any size where both passes have streaming shapes (has_stream2_plan): two sweeps where the
//     three-pass plan makes three -- dispatch_pass picks the 16-wide streaming three-step shapes for the 2048-point passes.
// Ext (interleaved) transforms: the two-pass plan at n = 2^21, the three-pass plan elsewhere.
template <class Plan> inline bool use_two_pass_plan(const Plan& plan, const Plan* plan_lat, uint64_t batch, int lq, int lde_log, const LaunchKnobs& k) {
    if (!plan_lat) return false;
    if (lde_log != 0 && lde_log > plan_lat->pass[0].log_m) return false;
    // Ext (interleaved) vectors: only where BOTH passes have interleaved streaming shapes (n = 2^21: the 1024-point column shapes and
    // the 2048-point closing shape; there are no interleaved 2048-point latency or column shapes).  A lone vector is four transforms'
    // worth of tiles -- 2^7 32-wide ones for the closing pass -- so every launch, chunked or not, reaches the streaming shape.
    // (a low-degree extension of Ext vectors to n = 2^22 as well: its first pass is the interleaved 16-wide 2048-point column shape
    // in its zero-fraction variants, 2^8 tiles' worth per vector)
    if (lq != 0) return (has_stream2_plan(plan.log_n) || (lde_log != 0 && has_latency_plan(plan.log_n))) && k.s3_tiles <= 7;
    const bool lat_small = k.p3_tiles >= 0 && k.lat_tiles >= 0 &&
                           ((batch << (plan.log_n - plan_lat->pass[0].log_m)) >> 5) <= (1ull << k.lat_tiles);
    // a low-degree extension reads 2^-lde_log of its first pass's input: the two sweeps win there even where the plain transform's do not
    const bool lat_stream = k.s3_tiles < 99 && (has_stream2_plan(plan.log_n) || (lde_log != 0 && has_latency_plan(plan.log_n)));
    return lat_small || lat_stream;
}

enum RouteKind { ROUTE_COPY = 0, ROUTE_ROW_SWEEP, ROUTE_LDS_SWEEP, ROUTE_PASSES };

struct Route {
    RouteKind kind = ROUTE_COPY;   // n = 1: copy only | n = 2^11 / 2^12: Row2048 / Row4096 | n = 2^13 .. 2^15: LdsPass | for_each_pass
    bool lat = false;              // ROUTE_PASSES: the two-pass plan of n = 2^21 / 2^22, not the main plan
    bool pad = false;              // a low-degree extension whose padding is materialised (memset + 2D copy), then transformed in place
    int lde_log = 0;               // what for_each_pass gets: the blow-up the first pass fuses (0 when pad)
    bool nt = false;               // the non-temporal twins
    uint64_t chunk = 0;            // base-field transforms per launch sequence
    int launches = 0;              // kernel launches per chunk
};

// The whole decision for `batch` transforms (lq = 2: Ext vectors, four interleaved base-field transforms each) of plan.log_n points,
// extended from 2^-log_blowup of their length, on a context whose launches are capped at chunk_elems elements (0: not).
template <class Plan> inline Route route_transform(const Plan& plan, const Plan* plan_lat, uint64_t batch, int lq, int log_blowup, uint64_t chunk_elems, const LaunchKnobs& k) {
    Route r;
    batch <<= lq;   // from here on in base-field transforms (Q interleaved ones per Ext vector)
    const uint64_t n = (uint64_t)1 << plan.log_n;
    // single-pass sizes (n <= 1024) and blow-ups beyond the first pass of the MAIN plan: pad and transform in place
    r.pad = log_blowup != 0 && !(plan.npasses >= 2 && log_blowup <= plan.pass[0].log_m);
    r.lde_log = r.pad ? 0 : log_blowup;
    r.chunk = batch;
    if (plan.log_n == 0) return r;
    if (r.lde_log == 0 && lq == 0 && row2048_enabled(plan, batch, k)) {
        r.kind = ROUTE_ROW_SWEEP;
        r.nt = batch * n * sizeof(uint32_t) >= k.nt_min_bytes;
        r.launches = 1;
        return r;
    }
    if (r.lde_log == 0 && lq == 0 && lds_kernel_enabled(plan, batch, k)) {
        r.kind = ROUTE_LDS_SWEEP;
        r.launches = 1;
        return r;
    }
    r.kind = ROUTE_PASSES;
    r.lat = use_two_pass_plan(plan, plan_lat, batch, lq, r.lde_log, k);
    if (chunk_elems && plan.npasses > 1) {
        r.chunk = chunk_elems / n;
        if (r.chunk < 1) r.chunk = 1;
        if (lq) r.chunk = ((r.chunk + 3) >> 2) << 2;   // whole Ext vectors
        if (r.chunk > batch) r.chunk = batch;
    }
    // streaming launches (footprint well beyond the 256 MiB Infinity Cache) take the non-temporal kernels
    // -- but not the rows under 256 words: there one load instruction covers a fraction of each 128-byte line it touches and
    // the following ones come back for the rest, which only the L1 makes cheap (measured at 2^28 elements per launch, plain
    // vs non-temporal: n = 2^4 351 vs 75 Gel/s, 2^5 331 vs 44, 2^6 545 vs 346, 2^7 633 vs 495; from 2^8 on within +-4 %)
    r.nt = r.lde_log == 0 && plan.log_n >= 8 && r.chunk * n * sizeof(uint32_t) >= k.nt_min_bytes;  // ONE launch's footprint
    r.launches = r.lat ? plan_lat->npasses : plan.npasses;
    return r;
}

}  // namespace toyni
