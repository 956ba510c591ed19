// CPU stepping of the PERSISTENT tile loop of ntt_pass_kernel (toyni_amd/csrc/toyni_hip.hip) with launch-invariant twiddle seeds,
// against the oracle.
//
// TEST INFRASTRUCTURE (tests/test_emu_seed_hoist.py).  tests/emu/emu_ntt.cpp steps a pass tile by tile and looks the seeds of every
// tile up afresh (Pass::phase1 / phase2); the kernel walks `grid` workgroups over the tiles tile_order(b), tile_order(b + grid), ...
// and, where the launcher's predicate seeds_launch_invariant (ntt_route.hpp) holds, looks the inter-pass twiddle seeds and the forward
// coset seed up ONCE per workgroup.  This program restates that loop around the same bodies (load_tile, in_scale_by, step1, step2):
// the seeds of a workgroup's FIRST tile serve all its tiles when the predicate says so, exactly as in the kernel, so a predicate
// that is true for a launch whose workgroups do change their column tile shows up as words that differ from the oracle.
//
// Build: g++ -O2 -std=c++17 -I toyni_amd/csrc tests/emu/emu_seed_hoist.cpp oracle/toyni_oracle.c   (also under ASan + UBSan)
//   emu_seed_hoist          every case
//   emu_seed_hoist light    without the 16 x 2^20 case (the sanitized run)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ntt_plan.hpp"
#include "contract_case.hpp"

extern "C" {
int orc_ntt_canonical(uint64_t*, size_t);
int orc_intt_canonical(uint64_t*, size_t);
void orc_fill_splitmix(uint64_t*, size_t, uint64_t);
int orc_domain_fft(uint64_t*, size_t, const uint64_t*, size_t, uint64_t);
}

using namespace toyni;


static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// launches of two-step column shapes, by what the predicate said and whether a workgroup walked more than one tile
static unsigned long long hoisted_multi = 0, hoisted_single = 0, per_tile_multi = 0, per_tile_single = 0;

template <class P> constexpr uint32_t log_tile_width() {
    uint32_t l = 0;
    while ((1u << l) < P::C) ++l;
    return l;
}

// one persistent launch of `grid` workgroups, workgroup after workgroup; inside a tile every thread runs a step before any thread
// runs the next (the pass' data barrier)
template <class P, int LZ>
static void emu_launch(const char* what, int pass_index, const PassArgs& args, uint64_t nblocks, uint32_t grid_wanted) {
    const uint32_t nt = (uint32_t)nblocks, grid = grid_wanted < nt ? grid_wanted : nt;
    if constexpr (P::STEPS == 2) {
        constexpr bool COL = P::PASS_KIND == KIND_COL && !P::SLAB;
        PassArgs a = args;
        if (COL) a.seeds_invariant = seeds_launch_invariant(grid, nt, a.log_S, log_tile_width<P>()) ? 1u : 0u;   // launch_pass
        const bool hoist = COL && a.seeds_invariant != 0u;
        const uint32_t tiles_per_wg = (nt + grid - 1) / grid;
        if (COL) {
            ++(hoist ? (tiles_per_wg > 1 ? hoisted_multi : hoisted_single) : (tiles_per_wg > 1 ? per_tile_multi : per_tile_single));
            std::printf("LAUNCH %s pass=%d lm=%d c=%u lq=%d grid=%u tiles=%u invariant=%d tiles_per_wg=%u\n", what, pass_index, (int)P::LM, (unsigned)P::C,
                        (int)P::LQ, grid, nt, (int)hoist, tiles_per_wg);
        }
        std::vector<uint32_t> lds(P::LDS_WORDS, 0xDEADBEEFu);   // exact size: an out-of-range LDS word is an ASan error
        std::vector<uint32_t> regs((size_t)P::T * P::E1);
        std::vector<typename P::Seeds> seeds(P::T);
        std::vector<uint32_t> inseed(P::T);
        const typename P::Uniform uni = P::load_uniform(a);
        for (uint32_t b = 0; b < grid; ++b) {
            bool first = true;
            for (uint32_t v = b; v < nt; v += grid) {
                const typename P::Tile t = P::tile_of(a, P::tile_order(v, nt));
                if (first || !hoist) {
                    for (uint32_t tid = 0; tid < P::T; ++tid) {
                        seeds[tid] = P::seeds_finish(a, P::seeds_issue(a, t, tid));
                        inseed[tid] = P::in_seed_finish(a, P::in_seed_issue(a, t, tid));
                    }
                }
                first = false;
                for (uint32_t tid = 0; tid < P::T; ++tid) {
                    uint32_t (&x)[P::E1] = *reinterpret_cast<uint32_t (*)[P::E1]>(&regs[(size_t)tid * P::E1]);
                    P::template load_tile<0, P::E1, LZ>(a, t, tid, x);
                    P::template in_scale_by<LZ>(a, inseed[tid], x);
                    P::template step1<LZ>(a, t, tid, x, lds.data(), uni, P::tw1_global(a), P::tw3_global(a));
                }
                for (uint32_t tid = 0; tid < P::T; ++tid) P::step2(a, t, tid, lds.data(), seeds[tid], uni);
            }
        }
    } else {
        (void)what; (void)pass_index; (void)args; (void)grid;
        CHECK(false, "%s: the cases run two-step shapes only (knobs: no three-step shapes)", what);
    }
}

struct Case {
    const char* what;
    int log_n;
    uint64_t batch;        // base-field transforms (lq = 2: four per Ext vector)
    uint32_t shift;        // 1: plain; else a forward coset transform (cs_mode 1 in the first pass)
    bool inverse;
    int lq;
    int wide_tiles;        // LaunchKnobs::wide_tiles (0: the 64-wide shapes of the 128- / 256- / 512-point passes)
    uint32_t grids[4];     // 0-terminated
    bool must_hoist;       // some launch of the case must run hoisted seeds over more than one tile per workgroup
    bool heavy;
};

template <int LQ>
static void run_passes(const Case& c, const LaunchKnobs& knobs, const NttPlan& plan, const uint32_t* src, uint32_t* work, uint32_t* dst, uint32_t grid,
                       const CosetTables& cs) {
    int p = 0;
    const bool ok = for_each_pass<LQ>(knobs, plan, (c.inverse ? plan.inv : plan.fwd).data(), c.inverse, src, work, dst, c.batch,
                                      [&](auto pass, auto lzc, const PassArgs& a, uint64_t nblocks) {
        using P = decltype(pass);
        emu_launch<P, decltype(lzc)::value>(c.what, p++, a, nblocks, grid);
    }, cs);
    CHECK(ok, "%s: no pass instantiation", c.what);
}

static void run_case(const Case& c) {
    TOYNI_CONTRACT_TAG("seed_hoist %s log_n=%d batch=%llu shift=%u inverse=%d lq=%d", c.what, c.log_n, (unsigned long long)c.batch, c.shift, (int)c.inverse, c.lq);
    LaunchKnobs knobs;          // defaults, not the environment
    knobs.p3_tiles = -1;        // the two-step shapes at every launch size
    knobs.s3_tiles = 99;
    knobs.wide_tiles = c.wide_tiles;
    NttPlan plan;
    if (!build_plan(knobs, c.log_n, plan)) { CHECK(false, "%s: plan", c.what); return; }
    const size_t n = (size_t)1 << c.log_n, q = (size_t)1 << c.lq, vectors = c.batch >> c.lq, total = n * c.batch;
    std::vector<uint64_t> ref(total);
    orc_fill_splitmix(ref.data(), total, 0x5EED0000ull + (uint64_t)c.log_n * 131 + c.batch * 7 + (c.inverse ? 3 : 0));
    std::vector<uint32_t> in(ref.begin(), ref.end()), want(total);
    std::vector<uint64_t> col(n), out(n);
    for (size_t v = 0; v < vectors; ++v)        // layout [vector][element][q]
        for (size_t k = 0; k < q; ++k) {
            for (size_t j = 0; j < n; ++j) col[j] = ref[(v * n + j) * q + k];
            if (c.inverse) { out = col; orc_intt_canonical(out.data(), n); }
            else if (c.shift == 1) { out = col; orc_ntt_canonical(out.data(), n); }
            else orc_domain_fft(out.data(), n, col.data(), n, c.shift);
            for (size_t j = 0; j < n; ++j) want[(v * n + j) * q + k] = (uint32_t)out[j];
        }
    std::vector<uint32_t> cblob;
    CosetTables cs;
    if (c.shift != 1) {
        uint32_t lo_off, hi_off;
        cs.s = c.shift;
        append_two_level(cblob, plan.log_n, cs.s, 1u, lo_off, hi_off, cs.lowbits);
        cs.lo = cblob.data() + lo_off;
        cs.hi = cblob.data() + hi_off;
    }
    const unsigned long long before = hoisted_multi;
    for (int g = 0; g < 4 && c.grids[g]; ++g) {
        // exactly sized buffers: an out-of-range tile word is an ASan error
        std::vector<uint32_t> work(total, 0xABABABABu), buf(total, 0xCDCDCDCDu);
        if (c.lq) run_passes<2>(c, knobs, plan, in.data(), work.data(), buf.data(), c.grids[g], cs);
        else run_passes<0>(c, knobs, plan, in.data(), work.data(), buf.data(), c.grids[g], cs);
        size_t bad = 0;
        for (size_t i = 0; i < total; ++i) bad += buf[i] != want[i];
        CHECK(bad == 0, "%s grid=%u: %zu of %zu words differ from the oracle", c.what, c.grids[g], bad, total);
    }
    if (c.must_hoist) CHECK(hoisted_multi > before, "%s: no launch ran hoisted seeds over more than one tile per workgroup", c.what);
    std::printf("CASE %s failures=%d\n", c.what, failures);
    std::fflush(stdout);
}

// Grids 2 and 32 everywhere; a third grid where neither makes the column pass launch-invariant with several tiles per workgroup.
//   4 x 2^20: 16-wide 1024-point tiles, 64 per prefix, 256 tiles -- grids 2 and 32 change the column tile (per-tile seeds), 64 does not
//   4 x 2^16, 64-wide: 4 tiles per prefix, 16 tiles (paired order) -- grid 2 per tile, grid 32 is one tile per workgroup;
//   5 x / 8 x 2^16 the same shape with 20 tiles (identity order, grid 4) and 32 tiles (paired order, grid 16) walk several tiles hoisted
//   coset / Ext at 2^16: 32-wide 256-point tiles, 8 / 32 per prefix, 64 tiles: grid 32 hoists over two tiles per workgroup
//   16 x 2^20: the 32-wide 1024-point shape of the benchmark, 32 tiles per prefix, 512 tiles, grid 32: sixteen tiles per workgroup
static const Case CASES[] = {
    {"4x2^20 forward", 20, 4, 1, false, 0, 12, {2, 32, 64, 0}, true, false},
    {"4x2^20 inverse", 20, 4, 1, true, 0, 12, {2, 32, 64, 0}, true, false},
    {"4x2^16 64-wide", 16, 4, 1, false, 0, 0, {2, 32, 0, 0}, false, false},
    {"5x2^16 64-wide", 16, 5, 1, false, 0, 0, {2, 32, 4, 0}, true, false},
    {"8x2^16 64-wide inverse", 16, 8, 1, true, 0, 0, {2, 32, 16, 0}, true, false},
    {"8x2^16 forward coset", 16, 8, 7, false, 0, 12, {2, 32, 0, 0}, true, false},
    {"2x2^16 Ext", 16, 8, 1, false, 2, 12, {2, 32, 0, 0}, true, false},
    {"2x2^16 Ext inverse", 16, 8, 1, true, 2, 12, {2, 32, 0, 0}, true, false},
    {"16x2^20 forward", 20, 16, 1, false, 0, 12, {32, 0, 0, 0}, true, true},
};

int main(int argc, char** argv) {
    const bool light = argc > 1 && !std::strcmp(argv[1], "light");
    for (const Case& c : CASES)
        if (!(light && c.heavy)) run_case(c);
    std::printf("column launches: hoisted over several tiles %llu, hoisted one tile per workgroup %llu, per-tile seeds over several tiles %llu, per-tile one tile %llu\n",
                hoisted_multi, hoisted_single, per_tile_multi, per_tile_single);
    CHECK(hoisted_multi > 0 && per_tile_multi > 0, "both forms of the loop must have run");
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "ALL OK", failures);
    return failures ? 1 : 0;
}
