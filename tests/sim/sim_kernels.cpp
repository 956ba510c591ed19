// Runs the __global__ functions of toyni_amd/csrc/toyni_hip.hip themselves -- the text the GPU runs, barriers included -- on the CPU
// under adversarial wave schedules (hip_sim.hpp) and compares what they write with the oracle.
//
// TEST INFRASTRUCTURE (tests/test_sim_schedules.py).  No sanitizer: the fibers would need annotations, and the bounds of the same
// bodies are checked by the sanitized steppers of tests/emu.  Arguments are built by the helpers the launcher itself uses
// (for_each_pass, lds_transform, row2048_transform: ntt_plan.hpp), as tests/emu does; which kernel a pass shape runs in restates the
// six lines of launch_pass.
//
//   sim_kernels                       every case under all eight schedules; prints the instantiations and the sites, then ALL OK
//   sim_kernels --only K              the cases of kernel K alone
//   sim_kernels --selftest            toy kernels that break the simulator's rules one at a time: each must end in its hard failure
//   sim_kernels --drop K:i            the cases of kernel K with its i-th synchronisation site switched off (in the simulator's hook,
//                                     never in the kernel text): DROP ... FAILS under the first schedule that shows a mismatch or
//                                     a hard failure, DROP ... SURVIVES when no schedule does
// Build: clang++ -O1 -std=c++17 -I toyni_amd/csrc -I include tests/sim/sim_kernels.cpp oracle/toyni_oracle.o
#include "hip_sim.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>

#define TOYNI_KERNEL_TEXT_ONLY
#include "toyni_hip.hip"
#include "../emu/contract_case.hpp"

alignas(16) uint32_t air_lds[1u << 16];   // the dynamic LDS of the AIR kernels (at most 160 KiB on the device)

extern "C" {
extern uint32_t __start_hipsim_lds[], __stop_hipsim_lds[];   // every __shared__ array lives in this section
uint64_t orc_bb_mul(uint64_t, uint64_t);
uint64_t orc_bb_add(uint64_t, uint64_t);
uint64_t orc_bb_inverse(uint64_t);
int orc_ntt_canonical(uint64_t*, size_t);
int orc_intt_canonical(uint64_t*, size_t);
void orc_fill_splitmix(uint64_t*, size_t, uint64_t);
int orc_domain_fft(uint64_t*, size_t, const uint64_t*, size_t, uint64_t);
int orc_domain_ifft(uint64_t*, size_t, uint64_t);
void orc_merkle_commit_values(uint8_t*, const uint64_t*, const uint8_t*, size_t);
size_t orc_merkle_total_digests(size_t);
uint64_t orc_poly_eval(const uint64_t*, size_t, uint64_t);
int orc_fib_quotient(uint64_t*, uint64_t*, const uint64_t*, size_t, size_t, uint64_t);
uint64_t orc_bb_root_of_unity(uint32_t);
}

void hipsim::poison_shared() {
    for (uint32_t* p = __start_hipsim_lds; p < __stop_hipsim_lds; ++p) *p = 0xDEADBEEFu;
    for (uint32_t& w : air_lds) w = 0xDEADBEEFu;
}

static int failures = 0;
static std::string only;                       // --only / --drop: the kernel whose cases run
static std::set<std::string> instantiations;   // what ran, for the printed list
static std::set<std::string> launched_now;     // kernel names launched by the case in progress
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class F>
static bool sim_launch(const char* name, const std::string& inst, dim3 grid, uint32_t block, F&& body) {
    instantiations.insert(std::string(name) + inst);
    TOYNI_CONTRACT_TAG("%s%s", name, inst.c_str());
    launched_now.insert(name);
    const bool ok = hipsim::launch(name, inst, grid, block, body);
    if (!ok) ++failures;
    return ok;
}
static bool wanted(const char* tag) { return only.empty() || only == tag; }
// a case must launch the kernel it is filed under: the table below names kernels, the dispatch table picks them
static void case_done(const char* tag, const char* what) {
    CHECK(launched_now.count(tag), "%s: the case never launched %s", what, tag);
    launched_now.clear();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// transforms
// ---------------------------------------------------------------------------------------------------------------------------------
template <class P> static std::string pass_inst(int lz) {
    char b[160];
    std::snprintf(b, sizeof b, "<kind=%d,lm=%d,c=%u,t=%u,nt=%d,lq=%d,lz=%d%s>", (int)P::PASS_KIND, (int)P::LM, (unsigned)P::C, (unsigned)P::T, (int)P::NT, (int)P::LQ, lz,
                  P::STEPS == 2 ? "" : P::STEPS == 1 ? ",single-step" : "");
    return b;
}
template <class P> struct Pass3Kind;
template <int K, int A, int B, int D, int C, bool N, int Q> struct Pass3Kind<Pass3<K, A, B, D, C, N, Q>> { static constexpr int value = K; };
template <class P> static std::string pass3_inst(int lz) {
    char b[160];
    std::snprintf(b, sizeof b, "<kind=%d,lm=%d,c=%u,t=%u,nt=%d,lq=%d,lz=%d", Pass3Kind<P>::value, (int)P::LM, (unsigned)P::C, (unsigned)P::T, (int)P::NT, (int)P::LQ, lz);
    std::string s = b;
    if constexpr (P::STREAM) s += P::WAVE_LOCAL2 ? ",WAVE_LOCAL2=true" : ",WAVE_LOCAL2=false";
    return s + ">";
}

struct NttCase {
    const char* tag;       // the kernel the case is about
    const char* what;
    int log_n;
    uint64_t batch;        // base-field transforms (lq = 2: four per Ext vector)
    uint32_t shift;
    bool inverse;
    int lde_log;
    int lq;
    bool latency;          // the two-pass plan of n = 2^21 / 2^22
    int p3_tiles, s3_tiles;
    uint32_t min_tiles;    // tiles a workgroup of the tagged kernel must walk at grid = 1
};

struct NttData {
    std::vector<uint32_t> in, want;
};
static std::map<const NttCase*, NttData> ntt_cache;   // inputs and the oracle's outputs: computed once, shared by every schedule

static const NttData& ntt_data(const NttCase& c) {
    auto it = ntt_cache.find(&c);
    if (it != ntt_cache.end()) return it->second;
    NttData& d = ntt_cache[&c];
    const size_t n = (size_t)1 << c.log_n, n_in = n >> c.lde_log, q = (size_t)1 << c.lq, vectors = c.batch >> c.lq;
    std::vector<uint64_t> ref(n_in * c.batch);
    orc_fill_splitmix(ref.data(), ref.size(), 0x51A0000ull + (uint64_t)c.log_n * 977 + (uint64_t)c.lde_log * 31 + c.batch);
    d.in.resize(ref.size());
    for (size_t i = 0; i < ref.size(); ++i) d.in[i] = (uint32_t)ref[i];
    d.want.resize(n * c.batch);
    std::vector<uint64_t> col(n_in), out(n);
    for (size_t v = 0; v < vectors; ++v)        // layout [vector][element][q]
        for (size_t k = 0; k < q; ++k) {
            for (size_t j = 0; j < n_in; ++j) col[j] = ref[(v * n_in + j) * q + k];
            if (!c.inverse) {
                if (c.shift == 1 && !c.lde_log) { out = col; orc_ntt_canonical(out.data(), n); }
                else orc_domain_fft(out.data(), n, col.data(), n_in, c.shift);
            } else {
                out = col;
                if (c.shift == 1) orc_intt_canonical(out.data(), n); else orc_domain_ifft(out.data(), n, c.shift);
            }
            for (size_t j = 0; j < n; ++j) d.want[(v * n + j) * q + k] = (uint32_t)out[j];
        }
    return d;
}

template <int LQ>
static void ntt_passes(const NttCase& c, const LaunchKnobs& knobs, const NttPlan& plan, const uint32_t* src, uint32_t* work, uint32_t* dst, uint32_t grid,
                       const CosetTables& cs) {
    const std::vector<uint32_t>& blob = c.inverse ? plan.inv : plan.fwd;
    const bool ok = for_each_pass<LQ>(knobs, plan, blob.data(), c.inverse, src, work, dst, c.batch, [&](auto pass, auto lzc, const PassArgs& a, uint64_t nblocks) {
        using P = decltype(pass);
        constexpr int LZ = decltype(lzc)::value;
        const uint32_t nt = (uint32_t)nblocks, g = grid < nt ? grid : nt;
        if constexpr (P::STEPS == 3) {
            if constexpr (P::STREAM) {
                if (!std::strcmp(c.tag, "ntt_pass3s_kernel") && grid == 1) CHECK(nt >= c.min_tiles, "%s: %u tiles", c.what, nt);
                sim_launch("ntt_pass3s_kernel", pass3_inst<P>(LZ), dim3(g), P::T, [&] { ntt_pass3s_kernel<P, LZ>(a, nt); });
            } else {
                if (!std::strcmp(c.tag, "ntt_pass3_kernel") && grid == 1) CHECK(nt >= c.min_tiles, "%s: %u tiles", c.what, nt);
                sim_launch("ntt_pass3_kernel", pass3_inst<P>(LZ), dim3(g), P::T, [&] { ntt_pass3_kernel<P, LZ>(a, nt); });
            }
        } else {
            if (!std::strcmp(c.tag, "ntt_pass_kernel") && grid == 1) CHECK(nt >= c.min_tiles, "%s: %u tiles", c.what, nt);
            if constexpr (LZ > 0) sim_launch("ntt_pass_kernel", pass_inst<P>(LZ), dim3(g), P::T, [&] { ntt_pass_kernel<P, 32, LZ>(a, nt); });
            else if constexpr (P::LQ > 0) {
                constexpr int PF = (P::PASS_KIND == KIND_ROW_N && P::LM == 10) ? 0 : 32;   // ext_prefetch of the launcher
                sim_launch("ntt_pass_kernel", pass_inst<P>(0), dim3(g), P::T, [&] { ntt_pass_kernel<P, PF>(a, nt); });
            } else sim_launch("ntt_pass_kernel", pass_inst<P>(0), dim3(g), P::T, [&] { ntt_pass_kernel<P, 32>(a, nt); });
        }
    }, cs, c.lde_log);
    CHECK(ok, "%s: no pass instantiation", c.what);
}

static void run_ntt(const NttCase& c, uint32_t grid, bool in_place) {
    LaunchKnobs knobs;
    knobs.p3_tiles = c.p3_tiles;
    knobs.s3_tiles = c.s3_tiles;
    NttPlan plan;
    if (!build_plan(knobs, c.log_n, plan, c.latency)) { CHECK(false, "%s: plan", c.what); return; }
    const NttData& d = ntt_data(c);
    const size_t total = d.want.size();
    std::vector<uint32_t> cblob;
    CosetTables cs;
    if (c.shift != 1) {
        uint32_t lo_off, hi_off;
        cs.s = c.inverse ? bb_inv_host(c.shift) : c.shift;
        append_two_level(cblob, plan.log_n, cs.s, 1u, lo_off, hi_off, cs.lowbits);
        cs.lo = cblob.data() + lo_off;
        cs.hi = cblob.data() + hi_off;
    }
    std::vector<uint32_t> buf(in_place ? d.in : std::vector<uint32_t>(total, 0xCDCDCDCDu)), work(total, 0xABABABABu);
    const uint32_t* src = in_place ? buf.data() : d.in.data();
    if (c.lq) ntt_passes<2>(c, knobs, plan, src, work.data(), buf.data(), grid, cs);
    else ntt_passes<0>(c, knobs, plan, src, work.data(), buf.data(), grid, cs);
    size_t bad = 0;
    for (size_t i = 0; i < total; ++i) bad += buf[i] != d.want[i];
    CHECK(bad == 0, "%s grid=%u in_place=%d [%s]: %zu of %zu words differ from the oracle", c.what, grid, (int)in_place,
          hipsim::schedule_name(hipsim::st().sched.waves * 2 + hipsim::st().sched.lanes_desc).c_str(), bad, total);
    case_done(c.tag, c.what);
}

// the smallest shapes at which each ordering can go wrong; every persistent launch walks at least three tiles per workgroup
static const NttCase NTT_CASES[] = {
    // tag, what, log_n, batch, shift, inverse, lde_log, lq, latency, p3_tiles, s3_tiles, min_tiles
    {"ntt_pass_kernel", "2^14 two-step first + closing pass", 14, 3, 1, false, 0, 0, false, -1, 7, 12},
    {"ntt_pass_kernel", "2^16 two-step first + closing pass", 16, 1, 1, false, 0, 0, false, -1, 7, 8},
    {"ntt_pass_kernel", "2^18 two-step first + closing pass", 18, 1, 1, false, 0, 0, false, -1, 7, 16},
    {"ntt_pass_kernel", "2^14 coset inverse", 14, 3, 7, true, 0, 0, false, -1, 7, 12},
    {"ntt_pass_kernel", "2^14 coset forward (in_scale)", 14, 3, 7, false, 0, 0, false, -1, 7, 12},
    {"ntt_pass_kernel", "2^16 LDE blow-up 2", 16, 1, 7, false, 1, 0, false, -1, 7, 8},
    {"ntt_pass_kernel", "2^16 LDE blow-up 16", 16, 1, 7, false, 4, 0, false, -1, 7, 8},
    {"ntt_pass_kernel", "2^14 interleaved (Ext)", 14, 4, 7, false, 0, 2, false, -1, 7, 16},
    {"ntt_pass_kernel", "2^5 single-step rows", 5, 64 * 6 + 3, 1, false, 0, 0, false, -1, 7, 7},
    {"ntt_pass_kernel", "2^5 single-step rows, inverse", 5, 64 * 6 + 3, 1, true, 0, 0, false, -1, 7, 7},
    {"ntt_pass3_kernel", "2^16 latency shapes", 16, 1, 1, false, 0, 0, false, 6, 7, 64},
    {"ntt_pass3_kernel", "2^16 latency shapes, coset inverse", 16, 1, 7, true, 0, 0, false, 6, 7, 64},
    {"ntt_pass3_kernel", "2^21 two-pass plan, 2048-point latency shape", 21, 1, 1, false, 0, 0, true, 6, 99, 256},
    {"ntt_pass3s_kernel", "2^21 two-pass plan, streaming closing pass (WAVE_LOCAL2)", 21, 1, 1, false, 0, 0, true, 6, 0, 64},
    {"ntt_pass3s_kernel", "2^22 LDE blow-up 32, streaming column pass (LZ > 0) + closing pass", 22, 1, 7, false, 5, 0, true, 6, 0, 128},
};

template <bool NT>
static void run_row_sweep(int log_n, uint64_t rows, uint32_t grid, bool in_place, bool inverse, uint32_t shift, const char* tag) {
    static std::map<std::string, NttData> cache;
    char key[96];
    std::snprintf(key, sizeof key, "%d/%llu/%d/%u", log_n, (unsigned long long)rows, (int)inverse, shift);
    NttData& d = cache[key];
    const size_t n = (size_t)1 << log_n;
    if (d.in.empty()) {
        std::vector<uint64_t> ref(n * rows);
        orc_fill_splitmix(ref.data(), ref.size(), 0x20480000ull + rows * 13 + (uint64_t)log_n);
        d.in.assign(ref.begin(), ref.end());
        for (uint64_t r = 0; r < rows; ++r) {
            if (inverse) { if (shift == 1) orc_intt_canonical(ref.data() + r * n, n); else orc_domain_ifft(ref.data() + r * n, n, shift); }
            else if (shift == 1) orc_ntt_canonical(ref.data() + r * n, n);
            else { std::vector<uint64_t> t(ref.begin() + r * n, ref.begin() + (r + 1) * n); orc_domain_fft(ref.data() + r * n, n, t.data(), n, shift); }
        }
        d.want.assign(ref.begin(), ref.end());
    }
    LaunchKnobs knobs;
    NttPlan plan;
    if (!build_plan(knobs, log_n, plan)) { CHECK(false, "row sweep plan"); return; }
    std::vector<uint32_t> cblob;
    CosetTables cs;
    if (shift != 1) {
        uint32_t lo_off, hi_off;
        cs.s = inverse ? bb_inv_host(shift) : shift;
        append_two_level(cblob, plan.log_n, cs.s, 1u, lo_off, hi_off, cs.lowbits);
        cs.lo = cblob.data() + lo_off;
        cs.hi = cblob.data() + hi_off;
    }
    std::vector<uint32_t> buf(in_place ? d.in : std::vector<uint32_t>(n * rows, 0xCDCDCDCDu));
    const bool ok = row2048_transform(plan, (inverse ? plan.inv : plan.fwd).data(), inverse, in_place ? buf.data() : d.in.data(), buf.data(), rows,
                                      [&](const PassArgs& a, uint64_t nrows) {
        if (log_n == 11) {
            sim_launch("ntt_row2048_kernel", NT ? "<nt=1>" : "<nt=0>", dim3(grid), Row2048::T, [&] { ntt_row2048_kernel<NT>(a); });
        } else {
            const uint32_t ntiles = (uint32_t)((nrows + Row4096::ROWS - 1) / Row4096::ROWS);
            CHECK(ntiles >= 3 * grid, "row4096: %u tiles for %u workgroups", ntiles, grid);
            sim_launch("ntt_row4096_kernel", NT ? "<nt=1>" : "<nt=0>", dim3(grid), Row4096::T, [&] { ntt_row4096_kernel<NT>(a, ntiles); });
        }
    }, cs);
    CHECK(ok, "row sweep rejected");
    size_t bad = 0;
    for (size_t i = 0; i < buf.size(); ++i) bad += buf[i] != d.want[i];
    CHECK(bad == 0, "%s rows=%llu grid=%u in_place=%d inverse=%d shift=%u: %zu words differ from the oracle", tag, (unsigned long long)rows, grid, (int)in_place,
          (int)inverse, shift, bad);
    case_done(tag, tag);
}

static void run_lds(int log_n, uint64_t batch, uint32_t grid, bool in_place, bool inverse, int log_rows) {
    static std::map<std::string, NttData> cache;
    char key[96];
    std::snprintf(key, sizeof key, "%d/%llu/%d", log_n, (unsigned long long)batch, (int)inverse);
    NttData& d = cache[key];
    const size_t n = (size_t)1 << log_n;
    if (d.in.empty()) {
        std::vector<uint64_t> ref(n * batch);
        orc_fill_splitmix(ref.data(), ref.size(), 0x1D50000ull + batch * 7 + (uint64_t)log_n);
        d.in.assign(ref.begin(), ref.end());
        for (uint64_t r = 0; r < batch; ++r) { if (inverse) orc_intt_canonical(ref.data() + r * n, n); else orc_ntt_canonical(ref.data() + r * n, n); }
        d.want.assign(ref.begin(), ref.end());
    }
    LaunchKnobs knobs;
    NttPlan plan;
    if (!build_plan(knobs, log_n, plan)) { CHECK(false, "lds plan"); return; }
    std::vector<uint32_t> buf(in_place ? d.in : std::vector<uint32_t>(n * batch, 0xCDCDCDCDu));
    const bool ok = lds_transform(plan, (inverse ? plan.inv : plan.fwd).data(), inverse, in_place ? buf.data() : d.in.data(), buf.data(), batch,
                                  [&](auto pass, const LdsArgs& g, uint64_t ntiles) {
        using L = decltype(pass);
        CHECK(ntiles >= 3 * (uint64_t)grid, "lds: %llu tiles for %u workgroups", (unsigned long long)ntiles, grid);
        char inst[64];
        std::snprintf(inst, sizeof inst, "<la=%d,rows=%u,t=%u>", plan.lds_la, (unsigned)L::ROWS, (unsigned)L::T);
        sim_launch("ntt_lds_kernel", inst, dim3(grid), L::T, [&] { ntt_lds_kernel<L>(g, (uint32_t)ntiles); });
    }, CosetTables(), log_rows);
    CHECK(ok, "lds transform rejected");
    size_t bad = 0;
    for (size_t i = 0; i < buf.size(); ++i) bad += buf[i] != d.want[i];
    CHECK(bad == 0, "ntt_lds_kernel log_n=%d batch=%llu grid=%u in_place=%d inverse=%d: %zu words differ from the oracle", log_n, (unsigned long long)batch, grid,
          (int)in_place, (int)inverse, bad);
    case_done("ntt_lds_kernel", "lds");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// accumulator columns
// ---------------------------------------------------------------------------------------------------------------------------------
static uint64_t sm_state;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t orc_op(int op, uint64_t a, uint64_t b) { return op == (int)SCAN_PRODUCT ? orc_bb_mul(a, b) : orc_bb_add(a, b); }

template <int OP>
static void run_scan(size_t n, uint32_t batch) {
    sm_state = 0x5CA9ull + n * 3 + OP;
    const size_t stride = n + 3;
    std::vector<uint32_t> num(stride * batch), den(stride * batch), out(stride * batch, 0xFFFFFFF0u), want(stride * batch), want_tot(2 * batch);
    ScanInit in{};
    for (uint32_t b = 0; b < batch; ++b) {
        const uint32_t init = b == 0 ? (OP == (int)SCAN_PRODUCT ? 1u : 0u) : 1u + (uint32_t)(splitmix() % (BB_P - 1));
        in.v[b] = OP == (int)SCAN_PRODUCT ? to_mont_host(init) : init;
        uint64_t acc = init, zeros = 0;
        for (size_t i = 0; i < n; ++i) {
            uint32_t u = 1u + (uint32_t)(splitmix() % (BB_P - 1)), v = 1u + (uint32_t)(splitmix() % (BB_P - 1));
            if (OP == (int)SCAN_SUM && i % 1021 == 7) v = 0;           // zero denominators: the term is 0, and they are counted
            if (i == n - 1 && OP == (int)SCAN_SUM && n > 1) v = 0;
            num[b * stride + i] = u;
            den[b * stride + i] = v;
            want[b * stride + i] = (uint32_t)acc;
            zeros += v == 0;
            acc = orc_op(OP, acc, v ? orc_bb_mul(u, orc_bb_inverse(v)) : 0);
        }
        want_tot[2 * b] = (uint32_t)acc;
        want_tot[2 * b + 1] = (uint32_t)zeros;
    }
    ScanArgs a{};
    a.num = num.data(); a.den = den.data(); a.out = out.data();
    a.num_stride = a.den_stride = a.out_stride = stride;
    a.n = n;
    a.ntiles = (uint32_t)((n + SCAN_TILE - 1) / SCAN_TILE);
    a.single = a.ntiles == 1;
    std::vector<uint32_t> tiles(2 * (size_t)a.ntiles * batch, 0xFFFFFFF0u), totals(2 * batch, 0xFFFFFFF0u);
    a.tiles = tiles.data();
    a.totals = totals.data();
    const char* inst = OP == (int)SCAN_PRODUCT ? "<product>" : "<sum>";
    if (a.single) {
        if (wanted("column_scan_apply_kernel")) sim_launch("column_scan_apply_kernel", inst, dim3(1, batch), SCAN_THREADS, [&] { column_scan_apply_kernel<OP>(a, in); });
        else return;
    } else {
        sim_launch("column_scan_aggregate_kernel", inst, dim3(a.ntiles, batch), SCAN_THREADS, [&] { column_scan_aggregate_kernel<OP>(a); });
        sim_launch("column_scan_prefix_kernel", inst, dim3(batch), SCAN_THREADS, [&] { column_scan_prefix_kernel<OP>(a, in); });
        sim_launch("column_scan_apply_kernel", inst, dim3(a.ntiles, batch), SCAN_THREADS, [&] { column_scan_apply_kernel<OP>(a, in); });
    }
    size_t bad = 0;
    for (uint32_t b = 0; b < batch; ++b) {
        for (size_t i = 0; i < n; ++i) bad += out[b * stride + i] != want[b * stride + i];
        for (size_t i = n; i < stride; ++i) bad += out[b * stride + i] != 0xFFFFFFF0u;
    }
    CHECK(bad == 0, "column scan op=%d n=%zu batch=%u: %zu words differ from the oracle", OP, n, batch, bad);
    CHECK(totals == want_tot, "column scan op=%d n=%zu batch=%u: totals / zero counts differ", OP, n, batch);
    launched_now.clear();
}

// step 2 alone on more aggregates than one round takes (2 SCAN_TILE + 5 of them would need 2^25 elements through steps 1 and 3)
template <int OP>
static void run_scan_prefix(uint32_t ntiles, uint32_t batch) {
    sm_state = 0x9EF1ull + ntiles + OP;
    ScanArgs a{};
    a.ntiles = ntiles;
    std::vector<uint32_t> tiles(2 * (size_t)ntiles * batch), want(tiles.size()), totals(2 * batch), want_tot(2 * batch);
    ScanInit in{};
    for (uint32_t b = 0; b < batch; ++b) {
        const uint32_t init = 1u + (uint32_t)(splitmix() % (BB_P - 1));
        in.v[b] = OP == (int)SCAN_PRODUCT ? to_mont_host(init) : init;
        uint64_t acc = init, zeros = 0;
        for (uint32_t k = 0; k < ntiles; ++k) {
            const uint32_t v = 1u + (uint32_t)(splitmix() % (BB_P - 1)), z = (uint32_t)(splitmix() % 5);
            tiles[(size_t)b * 2 * ntiles + k] = OP == (int)SCAN_PRODUCT ? to_mont_host(v) : v;   // aggregates are in the form the op scans
            tiles[(size_t)b * 2 * ntiles + ntiles + k] = z;
            want[(size_t)b * 2 * ntiles + k] = OP == (int)SCAN_PRODUCT ? to_mont_host((uint32_t)acc) : (uint32_t)acc;
            want[(size_t)b * 2 * ntiles + ntiles + k] = z;
            acc = orc_op(OP, acc, v);
            zeros += z;
        }
        want_tot[2 * b] = (uint32_t)acc;
        want_tot[2 * b + 1] = (uint32_t)zeros;
    }
    a.tiles = tiles.data();
    a.totals = totals.data();
    sim_launch("column_scan_prefix_kernel", OP == (int)SCAN_PRODUCT ? "<product>" : "<sum>", dim3(batch), SCAN_THREADS, [&] { column_scan_prefix_kernel<OP>(a, in); });
    CHECK(tiles == want, "column_scan_prefix_kernel op=%d ntiles=%u: prefixes differ from the oracle", OP, ntiles);
    CHECK(totals == want_tot, "column_scan_prefix_kernel op=%d ntiles=%u: totals differ", OP, ntiles);
    launched_now.clear();
}

static void run_batch_inverse(size_t count, bool in_place) {
    sm_state = 0xB1A5ull + count;
    std::vector<uint32_t> in(count), out(count, 0xFFFFFFF0u), want(count);
    uint32_t zeros = 0;
    for (size_t i = 0; i < count; ++i) {
        in[i] = i % 97 == 5 || i + 1 == count ? 0u : 1u + (uint32_t)(splitmix() % (BB_P - 1));
        want[i] = in[i] ? (uint32_t)orc_bb_inverse(in[i]) : 0u;
        zeros += in[i] == 0;
    }
    uint32_t zero_count = 0;
    uint32_t* o = in_place ? in.data() : out.data();
    sim_launch("batch_inverse_kernel", "", dim3((uint32_t)((count + SCAN_TILE - 1) / SCAN_TILE)), SCAN_THREADS,
               [&] { batch_inverse_kernel(in.data(), o, count, &zero_count); });
    size_t bad = 0;
    for (size_t i = 0; i < count; ++i) bad += o[i] != want[i];
    CHECK(bad == 0 && zero_count == zeros, "batch_inverse_kernel count=%zu: %zu words differ, %u zeros counted of %u", count, bad, zero_count, zeros);
    launched_now.clear();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Merkle levels on two waves per 64 nodes
// ---------------------------------------------------------------------------------------------------------------------------------
static std::vector<Digest> oracle_tree(size_t n) {
    std::vector<uint64_t> vals(n);
    orc_fill_splitmix(vals.data(), n, 0x3E2C1Eull + n);
    std::vector<Digest> t(orc_merkle_total_digests(n));
    orc_merkle_commit_values(reinterpret_cast<uint8_t*>(t.data()), vals.data(), nullptr, n);
    return t;
}
static void run_merkle_coop(size_t m) {
    const std::vector<Digest> tree = oracle_tree(m);
    const size_t up = (m + 1) / 2;
    std::vector<Digest> next(up);
    std::memset(next.data(), 0xEE, up * sizeof(Digest));
    sim_launch("merkle_level_coop_kernel", "", dim3((uint32_t)((up + 63) / 64)), 128, [&] { merkle_level_coop_kernel(tree.data(), next.data(), m, up); });
    CHECK(up == 1 ? tree.size() == m + 1 : true, "tree size");
    CHECK(std::memcmp(next.data(), tree.data() + m, up * sizeof(Digest)) == 0, "merkle_level_coop_kernel m=%zu up=%zu: the level differs from the oracle's", m, up);
    launched_now.clear();
}
static void run_merkle_tail(uint32_t m) {
    const std::vector<Digest> tree = oracle_tree(m);
    std::vector<Digest> next(tree.size() - m + 1);
    std::memset(next.data(), 0xEE, next.size() * sizeof(Digest));
    uint32_t notify[9] = {0};
    sim_launch("merkle_tail_kernel", "", dim3(1), MERKLE_TAIL_T, [&] { merkle_tail_kernel(tree.data(), next.data(), m, notify, 77u); });
    CHECK(std::memcmp(next.data(), tree.data() + m, (tree.size() - m) * sizeof(Digest)) == 0, "merkle_tail_kernel m=%u: the levels differ from the oracle's", m);
    CHECK(std::memcmp(notify, &tree.back(), 32) == 0 && notify[8] == 77u, "merkle_tail_kernel m=%u: the notified root", m);
    launched_now.clear();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// polynomial evaluation, quotients
// ---------------------------------------------------------------------------------------------------------------------------------
static void poly_points(PolyEvalArgs& a, uint32_t npoints, uint32_t (&z)[4]) {
    const uint32_t pts[4] = {987654321u, 1u, BB_P - 1u, 7u};
    a.npoints = npoints;
    for (uint32_t p = 0; p < npoints; ++p) {
        z[p] = pts[p];
        a.zR[p] = to_mont_host(z[p]);
        a.z16R[p] = to_mont_host(bb_pow_host(z[p], POLY_PER_THREAD));
        a.zchunkR[p] = to_mont_host(bb_pow_host(z[p], POLY_CHUNK));
    }
}
static void run_poly(size_t ncoeffs, uint32_t npoints) {
    std::vector<uint64_t> c64(ncoeffs);
    orc_fill_splitmix(c64.data(), ncoeffs, 0x9017 + ncoeffs);
    std::vector<uint32_t> c(c64.begin(), c64.end());
    PolyEvalArgs a{};
    uint32_t z[4];
    poly_points(a, npoints, z);
    a.coeffs = c.data();
    a.ncoeffs = ncoeffs;
    a.nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    std::vector<uint32_t> partial((size_t)a.nblocks * npoints, 0xFFFFFFF0u), out(npoints, 0xFFFFFFF0u);
    a.partial = partial.data();
    a.out = out.data();
    sim_launch("poly_eval_partial_kernel", "", dim3(a.nblocks), POLY_THREADS, [&] { poly_eval_partial_kernel(a); });
    sim_launch("poly_eval_final_kernel", "", dim3(1), 256, [&] { poly_eval_final_kernel(a); });
    for (uint32_t p = 0; p < npoints; ++p)
        CHECK(out[p] == (uint32_t)orc_poly_eval(c64.data(), ncoeffs, z[p]), "poly_eval ncoeffs=%zu point %u of %u differs from the oracle", ncoeffs, p, npoints);
    launched_now.clear();
}
static void run_poly_batch(size_t ncoeffs, uint32_t npoints, uint32_t batch, uint32_t grid_y) {
    const size_t stride = ncoeffs + 3;
    std::vector<uint64_t> c64(stride * batch);
    orc_fill_splitmix(c64.data(), c64.size(), 0xBA7C + ncoeffs);
    std::vector<uint32_t> c(c64.begin(), c64.end());
    PolyBatchArgs a{};
    uint32_t z[4];
    poly_points(a.e, npoints, z);
    a.e.coeffs = c.data();
    a.e.ncoeffs = ncoeffs;
    a.e.nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    a.stride = stride;
    a.batch = batch;
    std::vector<uint32_t> partial((size_t)a.e.nblocks * npoints * batch, 0xFFFFFFF0u), out((size_t)npoints * batch, 0xFFFFFFF0u);
    a.e.partial = partial.data();
    a.e.out = out.data();
    sim_launch("poly_eval_batch_partial_kernel", "", dim3(a.e.nblocks, grid_y), POLY_THREADS, [&] { poly_eval_batch_partial_kernel(a); });
    sim_launch("poly_eval_batch_final_kernel", "", dim3(grid_y), 256, [&] { poly_eval_batch_final_kernel(a); });
    for (uint32_t b = 0; b < batch; ++b)
        for (uint32_t p = 0; p < npoints; ++p)
            CHECK(out[(size_t)b * npoints + p] == (uint32_t)orc_poly_eval(c64.data() + b * stride, ncoeffs, z[p]),
                  "poly_eval_batch ncoeffs=%zu column %u point %u differs from the oracle", ncoeffs, b, p);
    launched_now.clear();
}

// stage 2 alone on more partial sums than a workgroup has threads: only then do two waves' values meet in block_sum_mod's tree
// (300 chunks through stage 1 would be 1.2 M coefficients; the sums of stage 1 are arbitrary residues as far as stage 2 is concerned)
static void run_poly_final(uint32_t nblocks, uint32_t npoints, uint32_t batch) {
    sm_state = 0xF1A7ull + nblocks + batch;
    PolyBatchArgs a{};
    uint32_t z[4];
    poly_points(a.e, npoints, z);
    a.e.nblocks = nblocks;
    a.batch = batch ? batch : 1;
    std::vector<uint32_t> partial((size_t)nblocks * npoints * a.batch), out((size_t)npoints * a.batch, 0xFFFFFFF0u), want(out.size());
    for (uint32_t& v : partial) v = (uint32_t)(splitmix() % BB_P);
    for (uint32_t col = 0; col < a.batch; ++col)
        for (uint32_t p = 0; p < npoints; ++p) {
            uint64_t acc = 0, zc = bb_pow_host(z[p], POLY_CHUNK), pw = 1;
            for (uint32_t b = 0; b < nblocks; ++b) {
                acc = orc_bb_add(acc, orc_bb_mul(partial[((size_t)col * nblocks + b) * npoints + p], pw));
                pw = orc_bb_mul(pw, zc);
            }
            want[(size_t)col * npoints + p] = (uint32_t)acc;
        }
    a.e.partial = partial.data();
    a.e.out = out.data();
    if (batch) sim_launch("poly_eval_batch_final_kernel", "", dim3(2), 256, [&] { poly_eval_batch_final_kernel(a); });
    else sim_launch("poly_eval_final_kernel", "", dim3(1), 256, [&] { poly_eval_final_kernel(a.e); });
    CHECK(out == want, "poly_eval%s_final_kernel nblocks=%u: the sums differ from the oracle", batch ? "_batch" : "", nblocks);
    launched_now.clear();
}

struct QuotientData { std::vector<uint64_t> lde, cw, qw; std::vector<uint32_t> t32; };
static const QuotientData& quotient_data(int log_N, int log_blowup, uint32_t shift) {
    static std::map<int, QuotientData> cache;
    QuotientData& d = cache[log_N * 64 + log_blowup];
    if (d.lde.empty()) {
        const size_t N = (size_t)1 << log_N;
        d.lde.resize(N); d.cw.resize(N); d.qw.resize(N);
        orc_fill_splitmix(d.lde.data(), N, 0xF1B0 + log_N);
        CHECK(orc_fib_quotient(d.cw.data(), d.qw.data(), d.lde.data(), N, N >> log_blowup, shift) == 0, "oracle quotient");
        d.t32.assign(d.lde.begin(), d.lde.end());
    }
    return d;
}
static void run_fib_quotient(int log_N, int log_blowup) {
    const uint32_t shift = 7;
    const QuotientData& d = quotient_data(log_N, log_blowup, shift);
    LaunchKnobs knobs;
    NttPlan plan;
    if (!build_plan(knobs, log_N, plan)) { CHECK(false, "plan"); return; }
    const size_t N = (size_t)1 << log_N, n = N >> log_blowup;
    std::vector<uint32_t> c(N, 0xFFFFFFF0u), q(N, 0xFFFFFFF0u);
    QuotientArgs a{};
    a.trace = d.t32.data();
    a.c_out = c.data();
    a.q_out = q.data();
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.log_N = (uint32_t)log_N;
    a.log_blowup = (uint32_t)log_blowup;
    const uint32_t g = (uint32_t)orc_bb_root_of_unity((uint32_t)(log_N - log_blowup));
    a.b1R = to_mont_host(bb_pow_host(g, n - 1));
    a.b2R = to_mont_host(bb_pow_host(g, n - 2));
    a.shift_nR = to_mont_host(bb_pow_host(shift, n));
    a.wBR = to_mont_host(bb_pow_host((uint32_t)orc_bb_root_of_unity((uint32_t)log_N), n));
    const uint32_t grid = (uint32_t)((N / 4 + 255) / 256);
    sim_launch("fib_quotient_kernel", "", dim3(grid), 256, [&] { fib_quotient_kernel(a); });
    size_t bad = 0;
    for (size_t i = 0; i < N; ++i) bad += c[i] != (uint32_t)d.cw[i] || q[i] != (uint32_t)d.qw[i];
    CHECK(bad == 0, "fib_quotient_kernel log_N=%d blow-up 2^%d: %zu points differ from the oracle", log_N, log_blowup, bad);
    launched_now.clear();
}
// the Fibonacci quotient as a constraint program (the program of tests/emu/emu_air.cpp), 1 / Z_H per residue class in LDS
static void run_air_quotient(int log_N, int log_blowup, bool inline_weights) {
    const uint32_t shift = 7;
    const QuotientData& d = quotient_data(log_N, log_blowup, shift);
    LaunchKnobs knobs;
    NttPlan plan;
    if (!build_plan(knobs, log_N, plan)) { CHECK(false, "plan"); return; }
    const size_t N = (size_t)1 << log_N, n = N >> log_blowup;
    const uint32_t g = bb_root_of_unity_host((uint32_t)(log_N - log_blowup));
    struct Insn { uint32_t op, dst, a, b, imm; };
    const Insn fib[] = {{AIR_OP_CELL, 0, 0, 0, 0}, {AIR_OP_CELL, 1, 1, 0, 0}, {AIR_OP_CELL, 2, 2, 0, 0}, {AIR_OP_ADD, 0, 1, 0, 0},
                        {AIR_OP_SUB, 0, 2, 0, 0}, {AIR_OP_X, 1, 0, 0, 0}, {AIR_OP_CONST, 2, 0, 0, bb_pow_host(g, n - 1)}, {AIR_OP_SUB, 2, 1, 2, 0},
                        {AIR_OP_MUL, 0, 0, 2, 0}, {AIR_OP_CONST, 2, 0, 0, bb_pow_host(g, n - 2)}, {AIR_OP_SUB, 2, 1, 2, 0}, {AIR_OP_MUL, 0, 0, 2, 0},
                        {AIR_OP_EMIT, 0, 0, 0, 0}};
    std::vector<AirInsn> dev;
    for (const Insn& in : fib) dev.push_back(AirInsn{in.op | in.dst << 8 | in.a << 16 | in.b << 24, in.op == AIR_OP_CONST ? to_mont_host(in.imm) : in.imm});
    std::vector<uint32_t> c(N, 0xFFFFFFF0u), q(N, 0xFFFFFFF0u);
    AirArgs a{};
    a.insns = dev.data();
    a.mat[0] = d.t32.data();
    a.col_stride[0] = N;
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.ninsns = (uint32_t)dev.size();
    a.nregs = 3;
    a.log_N = (uint32_t)log_N;
    a.log_blowup = (uint32_t)log_blowup;
    a.wNR = to_mont_host(bb_root_of_unity_host((uint32_t)log_N));
    a.shift_nR = to_mont_host(bb_pow_host(shift, n));
    a.wBR = to_mont_host(bb_pow_host(bb_root_of_unity_host((uint32_t)log_N), n));
    a.divides = 1;
    a.c_out = c.data();
    a.q_out = q.data();
    const AirLaunchShape shape = air_launch_shape(a.nregs, a.divides, a.log_blowup);
    CHECK(shape.zh_lds == 1 && shape.lds_bytes <= sizeof air_lds, "the AIR case must keep 1 / Z_H in LDS");
    a.zh_lds = shape.zh_lds;
    const uint32_t weights[1] = {1u};
    const uint32_t grid = (uint32_t)((N / 4 + shape.threads - 1) / shape.threads);
    if (inline_weights) {
        AirInlineWeights in{};
        in.w[0] = weights[0];
        sim_launch("air_quotient_inline_kernel", "", dim3(grid), shape.threads, [&] { air_quotient_inline_kernel(a, in); });
    } else {
        sim_launch("air_quotient_kernel", "", dim3(grid), shape.threads, [&] { air_quotient_kernel(a, weights); });
    }
    size_t bad = 0;
    for (size_t i = 0; i < N; ++i) bad += c[i] != (uint32_t)d.cw[i] || q[i] != (uint32_t)d.qw[i];
    CHECK(bad == 0, "air_quotient%s_kernel log_N=%d blow-up 2^%d: %zu points differ from the oracle", inline_weights ? "_inline" : "", log_N, log_blowup, bad);
    launched_now.clear();
}

// ---------------------------------------------------------------------------------------------------------------------------------
static void run_all_cases() {
    for (const NttCase& c : NTT_CASES) {
        if (!wanted(c.tag)) continue;
        const bool big = c.log_n >= 21;
        for (uint32_t grid : {1u, 2u, 3u}) {
            if (big && grid == 3) continue;   // (the 2^21 / 2^22 shapes: grid 1 and 2 walk 32+ tiles per workgroup either way)
            if (!c.lde_log && !(big && grid == 2)) run_ntt(c, grid, true);
            if (!(big && grid == 1 && !c.lde_log)) run_ntt(c, grid, false);
        }
    }
    if (wanted("ntt_lds_kernel")) {
        for (bool inverse : {false, true}) {
            run_lds(13, 3, 1, !inverse, inverse, 3);    // 3 tiles, one workgroup
            run_lds(13, 7, 2, inverse, inverse, 3);     // 7 tiles, two workgroups: 4 and 3
        }
        run_lds(13, 13, 1, true, false, 5);             // 32-row tiles of four transforms, the last one ragged
    }
    if (wanted("ntt_row2048_kernel")) {
        run_row_sweep<false>(11, 53, 1, true, false, 1, "ntt_row2048_kernel");    // 16 waves walk 3-4 rows each
        run_row_sweep<false>(11, 53, 1, false, true, 7, "ntt_row2048_kernel");
        run_row_sweep<true>(11, 101, 2, false, false, 7, "ntt_row2048_kernel");   // 32 waves, 3-4 rows each
        run_row_sweep<true>(11, 101, 2, true, true, 1, "ntt_row2048_kernel");
        run_row_sweep<false>(11, 5, 1, true, false, 1, "ntt_row2048_kernel");     // waves 5 .. 15 have no row and return behind the barrier
        run_row_sweep<false>(11, 19, 2, false, false, 1, "ntt_row2048_kernel");   // the second workgroup: three rows, thirteen idle waves
    }
    if (wanted("ntt_row4096_kernel")) {
        run_row_sweep<false>(12, 27, 1, true, false, 1, "ntt_row4096_kernel");    // 4 tiles, the last with 3 of 8 rows
        run_row_sweep<false>(12, 27, 1, false, true, 7, "ntt_row4096_kernel");
        run_row_sweep<true>(12, 51, 2, false, false, 7, "ntt_row4096_kernel");    // 7 tiles over two workgroups, ragged
        run_row_sweep<true>(12, 51, 2, true, true, 1, "ntt_row4096_kernel");
    }
    if (wanted("column_scan_aggregate_kernel") || wanted("column_scan_prefix_kernel") || wanted("column_scan_apply_kernel")) {
        for (size_t n : {(size_t)1, (size_t)SCAN_TILE - 1, (size_t)SCAN_TILE + 1, (size_t)2 * SCAN_TILE + 5}) {
            run_scan<SCAN_SUM>(n, 3);
            run_scan<SCAN_PRODUCT>(n, 3);
        }
        if (wanted("column_scan_prefix_kernel")) {
            run_scan_prefix<SCAN_SUM>(2 * SCAN_TILE + 5, 2);
            run_scan_prefix<SCAN_PRODUCT>(SCAN_TILE + 1, 2);
        }
    }
    if (wanted("batch_inverse_kernel")) {
        run_batch_inverse(SCAN_TILE + 5, false);
        run_batch_inverse(3, true);
    }
    if (wanted("merkle_level_coop_kernel"))
        for (size_t m : {(size_t)2, (size_t)125, (size_t)126, (size_t)129, (size_t)130}) run_merkle_coop(m);   // up = 1, 63, 63, 65, 65 (odd m: the last node twice)
    if (wanted("merkle_tail_kernel"))
        for (uint32_t m : {2u, 3u, 129u, 512u}) run_merkle_tail(m);
    if (wanted("poly_eval_partial_kernel") || wanted("poly_eval_final_kernel"))
        for (size_t nc : {(size_t)1, (size_t)4097}) { run_poly(nc, 2); run_poly(nc, 4); }
    if (wanted("poly_eval_final_kernel")) run_poly_final(300, 2, 0);
    if (wanted("poly_eval_batch_partial_kernel") || wanted("poly_eval_batch_final_kernel"))
        for (size_t nc : {(size_t)1, (size_t)4097}) { run_poly_batch(nc, 2, 3, 2); run_poly_batch(nc, 4, 3, 2); }
    if (wanted("poly_eval_batch_final_kernel")) run_poly_final(300, 2, 3);
    if (wanted("fib_quotient_kernel")) { run_fib_quotient(10, 3); run_fib_quotient(12, 9); }
    if (wanted("air_quotient_kernel")) { run_air_quotient(10, 3, false); run_air_quotient(12, 8, false); }
    if (wanted("air_quotient_inline_kernel")) { run_air_quotient(10, 3, true); run_air_quotient(12, 8, true); }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// --selftest: four toy kernels that each break one rule of the simulator; every one must end in exactly one hard failure
// ---------------------------------------------------------------------------------------------------------------------------------
static void toy_some_return() { if (threadIdx.x == 69) return; __syncthreads(); }
static void toy_two_lines() {
    if (threadIdx.x & 1) __syncthreads();
    else __syncthreads();
}
static void toy_not_uniform() { (void)TOYNI_UNIFORM(threadIdx.x == 3 ? 1u : 0u); __syncthreads(); }
static void toy_never_released() { if (threadIdx.x & 1) TOYNI_WAVE_ORDER(); else __syncthreads(); }
static void toy_well_formed() {   // early return of a whole wave, a wave-uniform value, lanes that leave before a wave rendezvous: all legal
    if (threadIdx.x >= 128) return;
    (void)TOYNI_UNIFORM(threadIdx.x >> 6);
    __syncthreads();
    if (threadIdx.x & 1) return;
    TOYNI_WAVE_ORDER();
}
static int selftest() {
    hipsim::State& s = hipsim::st();
    struct Toy { const char* name; void (*fn)(); const char* expect; };
    const Toy toys[] = {{"toy_some_return", toy_some_return, "some arrived, some returned"}, {"toy_two_lines", toy_two_lines, "different source lines"},
                        {"toy_not_uniform", toy_not_uniform, "TOYNI_UNIFORM value differs"}, {"toy_never_released", toy_never_released, "never be released"},
                        {"toy_well_formed", toy_well_formed, nullptr}};
    int bad = 0;
    for (int k = 0; k < hipsim::NUM_SCHEDULES; ++k) {
        s.sched = hipsim::schedule_of(k);
        for (const Toy& t : toys) {
            const unsigned long long before = s.hard_failures;
            s.last_failure.clear();
            hipsim::launch(t.name, "", dim3(1), 192, t.fn);
            const bool ok = t.expect ? s.hard_failures == before + 1 && s.last_failure.find(t.expect) != std::string::npos : s.hard_failures == before;
            if (!ok) { ++bad; std::printf("SELFTEST %s under %s: expected %s\n", t.name, hipsim::schedule_name(k).c_str(), t.expect ? t.expect : "no failure"); }
        }
    }
    std::printf("%s\n", bad ? "SELFTEST FAILED" : "SELFTEST OK");
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    hipsim::State& s = hipsim::st();
    bool drop = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--selftest")) return selftest();
        else if (!std::strcmp(argv[i], "--only") && i + 1 < argc) only = argv[++i];
        else if (!std::strcmp(argv[i], "--drop") && i + 1 < argc) {
            const char* colon = std::strrchr(argv[++i], ':');
            if (!colon) { std::printf("usage: --drop kernel:ordinal\n"); return 2; }
            only = std::string((const char*)argv[i], (const char*)colon);
            s.drop_kernel = only;
            s.drop_site = std::atoi(colon + 1);
            drop = true;
        } else { std::printf("usage: sim_kernels [--only kernel | --drop kernel:ordinal]\n"); return 2; }
    }
    for (int k = 0; k < hipsim::NUM_SCHEDULES; ++k) {
        s.sched = hipsim::schedule_of(k);
        const int before = failures;
        run_all_cases();
        std::printf("SCHEDULE %s failures=%d\n", hipsim::schedule_name(k).c_str(), failures - before);
        if (drop && failures) {   // the site is shown needed: no further schedule has to run
            const hipsim::KernelSites& ks = s.kernels[only];
            if ((size_t)s.drop_site < ks.sites.size()) {
                s.cur_kernel = &s.kernels[only];
                std::printf("DROP %s:%d %s FAILS under %s (%s)\n", only.c_str(), s.drop_site, hipsim::site_text(s.drop_site).c_str(), hipsim::schedule_name(k).c_str(),
                            s.hard_failures ? "hard failure" : "mismatch");
            }
            return 0;
        }
    }
    for (const std::string& inst : instantiations) std::printf("RAN %s\n", inst.c_str());
    for (auto& kv : s.kernels) {
        s.cur_kernel = &kv.second;
        for (size_t i = 0; i < kv.second.sites.size(); ++i)
            std::printf("SITE %s:%zu %s arrivals=%llu\n", kv.first.c_str(), i, hipsim::site_text((int)i).c_str(), kv.second.sites[i].arrivals);
    }
    std::printf("launches=%llu fiber switches=%llu hard failures=%llu\n", s.launches, s.switches, s.hard_failures);
    if (drop) {
        if ((size_t)s.drop_site >= s.kernels[only].sites.size()) { std::printf("DROP %s:%d NO SUCH SITE\n", only.c_str(), s.drop_site); return 2; }
        s.cur_kernel = &s.kernels[only];
        std::printf("DROP %s:%d %s SURVIVES (%llu calls dropped)\n", only.c_str(), s.drop_site, hipsim::site_text(s.drop_site).c_str(), s.dropped_calls);
        return 0;
    }
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "ALL OK", failures);
    return failures ? 1 : 0;
}
