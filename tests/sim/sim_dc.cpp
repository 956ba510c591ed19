// Runs the __global__ functions of include/toyni_hip.h 3p themselves (toyni_amd/csrc/toyni_hip.hip: air_dc_prepare_kernel,
// air_quotient_ext_dc_kernel, extcol_dc_prepare_kernel, extcol_aggregate_dc_kernel, extcol_apply_dc_kernel) on the CPU under the
// adversarial wave schedules of hip_sim.hpp, the way sim_air_ext.cpp and sim_scan_ext.cpp run the argument-fed kernels.
//
// TEST INFRASTRUCTURE (tests/test_sim_dc.py).  The preparation kernels share nothing between lanes; they run here because the twins
// read what they wrote.  The twins have the synchronisation of their originals: the barrier behind the table of 1 / Z_H, the cross-lane
// steps and the barriers of the block-wide scans.
//   quotient   the record from air_dc_prepare_kernel (raw words >= p among the parameters and the alphas, emit_ext form), then the
//              twin on a program with two PARAMs, against a host model that shares nothing with it: the program interpreted point by
//              point on plain residues with params[j] mod p and the weights alpha_k X^j.  log N = 10 with B = 2^3 (one workgroup) and
//              log N = 12 with B = 2^8 (four), out_stride = N + 1, a c output in the first, accumulation in the second.
//   scan       the record from extcol_dc_prepare_kernel, then the three launches with the twins in steps 1 and 3, against the
//              ARGUMENT-FED kernels on the same columns under the reduced shifts (tests/sim/sim_scan_ext.cpp holds those to a host
//              model): (gamma + a) / (gamma + b) with one index, both ops, n = 5 (one launch) and two tiles + 7, two columns.
//
//   sim_dc                       every case under all eight schedules; prints the instantiations and the sites, then ALL OK
//   sim_dc --only K              the cases of kernel K alone
//   sim_dc --drop K:i            the cases of kernel K with its i-th synchronisation site switched off: DROP ... FAILS / SURVIVES
#include "hip_sim.hpp"

#include <cstdio>
#include <cstring>
#include <set>

#define TOYNI_KERNEL_TEXT_ONLY
#include "toyni_hip.hip"
#include "../emu/contract_case.hpp"

alignas(16) uint32_t air_lds[1u << 14];   // the dynamic LDS of the AIR kernels: 64 KiB

extern "C" {
extern uint32_t __start_hipsim_lds[], __stop_hipsim_lds[];   // every __shared__ array lives in this section
}
void hipsim::poison_shared() {
    for (uint32_t* p = __start_hipsim_lds; p < __stop_hipsim_lds; ++p) *p = 0xDEADBEEFu;
    for (uint32_t& w : air_lds) w = 0xDEADBEEFu;
}

static int failures = 0;
static std::string only;
static std::set<std::string> instantiations;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class F>
static bool sim_launch(const char* name, const std::string& inst, dim3 grid, uint32_t block, F&& body) {
    instantiations.insert(std::string(name) + inst);
    TOYNI_CONTRACT_TAG("%s%s", name, inst.c_str());
    const bool ok = hipsim::launch(name, inst, grid, block, body);
    if (!ok) ++failures;
    return ok;
}
static bool wanted(const char* tag) { return only.empty() || only == tag; }

static uint64_t sm_state;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t rnd() { return (uint32_t)(splitmix() % BB_P); }
static uint32_t h_add(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + b) % BB_P); }
static uint32_t h_sub(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + BB_P - b) % BB_P); }

struct Insn { uint32_t op, dst, a, b, imm; };
constexpr uint32_t SLACK = 0xFFFFFFF0u;
constexpr uint32_t NPARAMS = 3, NALPHAS = 1;   // emit_ext form: four weights

static void run_quotient(int log_N, int log_blowup, bool with_c, bool accumulate) {
    const uint32_t shift = 7;
    sm_state = 0xDCA1ull + (uint64_t)log_N * 31 + (uint64_t)log_blowup;
    NttPlan plan;
    if (!build_plan(log_N, plan)) { CHECK(false, "plan"); return; }
    const size_t N = (size_t)1 << log_N, n = N >> log_blowup, B = (size_t)1 << log_blowup;
    const size_t stride0 = N, stride1 = N + 4, out_stride = N + 1;
    const uint32_t zpoint = 123456789u;   // not on the coset
    // sim_air_ext.cpp's program with its constant a parameter, and a second parameter times x: constraint numbers 0 (twice), 1, 2, 3
    const std::vector<Insn> prog = {{AIR_OP_CELL, 0, 0, 0, 1}, {AIR_OP_CELL, 1, 1, 0, 1}, {AIR_OP_CELL, 2, 0, 1, 2}, {AIR_OP_MUL, 3, 0, 2, 0},
                                    {AIR_OP_SUB, 3, 1, 3, 0}, {AIR_OP_EMIT, 0, 3, 0, 0}, {AIR_OP_PARAM, 4, 0, 0, 2}, {AIR_OP_SUB, 4, 0, 4, 0},
                                    {AIR_OP_XINV, 5, 0, 0, zpoint}, {AIR_OP_MUL, 4, 4, 5, 0}, {AIR_OP_EMIT, 0, 4, 1, 1}, {AIR_OP_X, 5, 0, 0, 0},
                                    {AIR_OP_MUL, 5, 5, 2, 0}, {AIR_OP_EMIT, 0, 5, 0, 2}, {AIR_OP_EMIT, 0, 1, 1, 0}, {AIR_OP_PARAM, 3, 0, 0, 0},
                                    {AIR_OP_MUL, 3, 3, 5, 0}, {AIR_OP_EMIT, 0, 3, 0, 3}};
    std::vector<uint32_t> m0(2 * stride0, SLACK), m1(3 * stride1, SLACK);
    for (size_t c = 0; c < 2; ++c) for (size_t i = 0; i < N; ++i) m0[c * stride0 + i] = i % 97 == 3 ? BB_P - 1u : rnd();
    for (size_t c = 0; c < 3; ++c) for (size_t i = 0; i < N; ++i) m1[c * stride1 + i] = rnd();
    const std::vector<uint32_t> params_raw = {0xFFFFFFFFu, (uint32_t)splitmix(), BB_P + 5u}, alphas_raw = {BB_P + 1u, 0xFFFFFFFFu, (uint32_t)splitmix(), BB_P};
    uint32_t a_red[4], weights[16];
    for (int e = 0; e < 4; ++e) a_red[e] = alphas_raw[e] % BB_P;
    for (int j = 0; j < 4; ++j)
        for (int e = 0; e < 4; ++e) weights[4 * j + (e + j) % 4] = e + j >= 4 ? bb_mul_host(a_red[e], 11u) : a_red[e];
    const size_t out_words = 3 * out_stride + N;
    std::vector<uint32_t> c_out(out_words, SLACK), q_out(out_words, SLACK);
    if (accumulate)
        for (size_t e = 0; e < 4; ++e) for (size_t i = 0; i < N; ++i) { c_out[e * out_stride + i] = rnd(); q_out[e * out_stride + i] = rnd(); }
    std::vector<uint32_t> want_c = c_out, want_q = q_out;
    {
        const uint32_t w = bb_root_of_unity_host((uint32_t)log_N);
        uint32_t x = shift;
        for (size_t i = 0; i < N; ++i, x = bb_mul_host(x, w)) {
            uint32_t r[6] = {}, cs[4] = {}, us[4] = {};
            for (const Insn& in : prog) {
                switch (in.op) {
                    case AIR_OP_CELL: r[in.dst] = (in.b ? m1[in.imm * stride1 + (i + in.a * B) % N] : m0[in.imm * stride0 + (i + in.a * B) % N]); break;
                    case AIR_OP_PARAM: r[in.dst] = params_raw[in.imm] % BB_P; break;
                    case AIR_OP_X: r[in.dst] = x; break;
                    case AIR_OP_XINV: r[in.dst] = bb_inv_host(h_sub(x, in.imm)); break;
                    case AIR_OP_ADD: r[in.dst] = h_add(r[in.a], r[in.b]); break;
                    case AIR_OP_SUB: r[in.dst] = h_sub(r[in.a], r[in.b]); break;
                    case AIR_OP_MUL: r[in.dst] = bb_mul_host(r[in.a], r[in.b]); break;
                    default:
                        for (int e = 0; e < 4; ++e) {
                            uint32_t& acc = in.b ? us[e] : cs[e];
                            acc = h_add(acc, bb_mul_host(r[in.a], weights[4 * in.imm + e]));
                        }
                }
            }
            const uint32_t zh_inv = bb_inv_host(h_sub(bb_pow_host(x, n), 1u));
            for (size_t e = 0; e < 4; ++e) {
                const uint32_t q = h_add(bb_mul_host(cs[e], zh_inv), us[e]);
                want_c[e * out_stride + i] = accumulate ? h_add(want_c[e * out_stride + i], cs[e]) : cs[e];
                want_q[e * out_stride + i] = accumulate ? h_add(want_q[e * out_stride + i], q) : q;
            }
        }
    }
    if (!with_c) want_c = c_out;
    std::vector<AirInsn> dev;
    for (const Insn& in : prog)
        dev.push_back(AirInsn{in.op | in.dst << 8 | in.a << 16 | in.b << 24, in.op == AIR_OP_XINV ? to_mont_host(in.imm) : in.imm});
    AirArgs a{};
    a.insns = dev.data();
    a.mat[0] = m0.data();
    a.col_stride[0] = stride0;
    a.mat[1] = m1.data();
    a.col_stride[1] = stride1;
    a.c_out = with_c ? c_out.data() : nullptr;
    a.q_out = q_out.data();
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.ninsns = (uint32_t)dev.size();
    a.nregs = 6;
    a.log_N = (uint32_t)log_N;
    a.log_blowup = (uint32_t)log_blowup;
    a.wNR = to_mont_host(bb_root_of_unity_host((uint32_t)log_N));
    a.shift_nR = to_mont_host(bb_pow_host(shift, n));
    a.wBR = to_mont_host(bb_pow_host(bb_root_of_unity_host((uint32_t)log_N), n));
    a.divides = 1;
    a.accumulate = accumulate ? 1u : 0u;
    const AirLaunchShape shape = air_launch_shape(a.nregs, a.divides, a.log_blowup);
    CHECK(shape.zh_lds == 1 && shape.lds_bytes <= sizeof air_lds, "the case must keep 1 / Z_H in LDS");
    a.zh_lds = shape.zh_lds;
    const uint32_t grid = (uint32_t)((N / 4 + shape.threads - 1) / shape.threads);
    const uint64_t os = out_stride;
    std::vector<uint32_t> rec(air_dc_record_words(NPARAMS, NALPHAS, AIR_WEIGHTS_EMIT_EXT), SLACK);
    sim_launch("air_dc_prepare_kernel", "", dim3(1), TRANSCRIPT_T,
               [&] { air_dc_prepare_kernel(params_raw.data(), NPARAMS, alphas_raw.data(), NALPHAS, AIR_WEIGHTS_EMIT_EXT, rec.data()); });
    sim_launch("air_quotient_ext_dc_kernel", "", dim3(grid), shape.threads, [&] { air_quotient_ext_dc_kernel(a, os, rec.data(), NPARAMS); });
    size_t bad = 0;
    for (size_t k = 0; k < out_words; ++k) bad += c_out[k] != want_c[k] || q_out[k] != want_q[k];   // the words N .. out_stride keep their filler
    CHECK(bad == 0, "air_quotient_ext_dc_kernel log_N=%d blow-up 2^%d: %zu words differ from the host model", log_N, log_blowup, bad);
}

template <int OP>
static void run_scan(uint64_t n) {
    const char* inst = OP == (int)SCAN_PRODUCT ? "<product>" : "<sum>";
    sm_state = 0xDC5Cull + n * 7 + OP;
    const uint32_t batch = 2;
    const uint64_t stride = n + 1;
    std::vector<uint32_t> num((batch - 1) * stride + n), den((batch - 1) * stride + n);
    for (uint32_t& w : num) w = rnd();
    for (uint32_t& w : den) w = rnd();
    const std::vector<uint32_t> chal = {rnd(), rnd(), rnd(), rnd(), 0xFFFFFFFFu, BB_P + 1u, (uint32_t)splitmix(), BB_P};   // gamma is element 1
    uint32_t gamma[4], z[4];
    for (int k = 0; k < 4; ++k) { gamma[k] = chal[4 + k] % BB_P; z[k] = gamma[k] ? BB_P - gamma[k] : 0u; }
    const uint32_t ntiles = (uint32_t)((n + EXT_ACCUM_TILE - 1) / EXT_ACCUM_TILE);
    ExtAccumSeeds in{};
    for (uint32_t b = 0; b < batch; ++b)
        for (int k = 0; k < 4; ++k) { const uint32_t v = rnd(); in.v[b][k] = OP == (int)SCAN_PRODUCT ? to_mont_host(v) : v; }
    std::vector<uint32_t> out[2], tiles[2], totals[2];
    for (int side = 0; side < 2; ++side) {      // 0: the argument-fed kernels, 1: the record-fed twins
        out[side].assign((4 * batch - 1) * stride + n, SLACK);
        tiles[side].assign((size_t)EXT_ACCUM_TILE_WORDS * ntiles * batch, SLACK);
        totals[side].assign(8 * batch, SLACK);
        ExtAccumArgs a{};
        a.num = ExtAccumOperand{num.data(), stride, 1, {0, 0, 0, 0}};
        a.den = ExtAccumOperand{den.data(), stride, 1, {0, 0, 0, 0}};
        a.out = out[side].data();
        a.out_stride = stride;
        a.n = n;
        a.tiles = tiles[side].data();
        a.totals = totals[side].data();
        a.ntiles = ntiles;
        a.single = ntiles == 1 ? 1u : 0u;
        if (side == 0) {
            for (int k = 0; k < 4; ++k) a.num.shift[k] = a.den.shift[k] = gamma[k];
            a.den_inv = ext_shift_host(z);
            if (a.single) {
                sim_launch("ext_accum_apply_kernel", inst, dim3(1, batch), EXT_ACCUM_THREADS, [&] { ext_accum_apply_kernel<OP>(a, in); });
            } else {
                sim_launch("ext_accum_aggregate_kernel", inst, dim3(ntiles, batch), EXT_ACCUM_THREADS, [&] { ext_accum_aggregate_kernel<OP>(a); });
                sim_launch("ext_accum_prefix_kernel", inst, dim3(batch), EXT_ACCUM_THREADS, [&] { ext_accum_prefix_kernel<OP>(a, in); });
                sim_launch("ext_accum_apply_kernel", inst, dim3(ntiles, batch), EXT_ACCUM_THREADS, [&] { ext_accum_apply_kernel<OP>(a, in); });
            }
        } else {
            ExtAccumRecord* rec = static_cast<ExtAccumRecord*>(::operator new(sizeof(ExtAccumRecord), std::align_val_t(16)));
            std::memset(rec, 0xA5, sizeof *rec);
            sim_launch("extcol_dc_prepare_kernel", "", dim3(1), TRANSCRIPT_T, [&] { extcol_dc_prepare_kernel(chal.data(), 1u, 1u, 1u, rec); });
            if (a.single) {
                sim_launch("extcol_apply_dc_kernel", inst, dim3(1, batch), EXT_ACCUM_THREADS, [&] { extcol_apply_dc_kernel<OP>(a, in, rec); });
            } else {
                sim_launch("extcol_aggregate_dc_kernel", inst, dim3(ntiles, batch), EXT_ACCUM_THREADS, [&] { extcol_aggregate_dc_kernel<OP>(a, rec); });
                sim_launch("ext_accum_prefix_kernel", inst, dim3(batch), EXT_ACCUM_THREADS, [&] { ext_accum_prefix_kernel<OP>(a, in); });
                sim_launch("extcol_apply_dc_kernel", inst, dim3(ntiles, batch), EXT_ACCUM_THREADS, [&] { extcol_apply_dc_kernel<OP>(a, in, rec); });
            }
            ::operator delete(rec, std::align_val_t(16));
        }
    }
    CHECK(out[0] == out[1], "scan op=%d n=%llu: the twins' columns differ from the argument-fed kernels'", OP, (unsigned long long)n);
    CHECK(totals[0] == totals[1], "scan op=%d n=%llu: the twins' totals differ", OP, (unsigned long long)n);
    bool written = true;
    for (uint32_t c = 0; c < 4 * batch; ++c)
        for (uint64_t i = 0; i < n; ++i) written = written && out[1][c * stride + i] < BB_P;
    CHECK(written, "scan op=%d n=%llu: an output word was not written", OP, (unsigned long long)n);
}

static void run_all_cases() {
    if (wanted("air_quotient_ext_dc_kernel") || wanted("air_dc_prepare_kernel")) { run_quotient(10, 3, true, false); run_quotient(12, 8, false, true); }
    if (wanted("extcol_apply_dc_kernel") || wanted("extcol_aggregate_dc_kernel") || wanted("extcol_dc_prepare_kernel")) {
        for (uint64_t n : {(uint64_t)5, (uint64_t)2 * EXT_ACCUM_TILE + 7}) { run_scan<(int)SCAN_SUM>(n); run_scan<(int)SCAN_PRODUCT>(n); }
    }
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    hipsim::State& s = hipsim::st();
    bool drop = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--only") && i + 1 < argc) only = argv[++i];
        else if (!std::strcmp(argv[i], "--drop") && i + 1 < argc) {
            const char* colon = std::strrchr(argv[++i], ':');
            if (!colon) { std::printf("usage: --drop kernel:ordinal\n"); return 2; }
            only = std::string((const char*)argv[i], (const char*)colon);
            s.drop_kernel = only;
            s.drop_site = std::atoi(colon + 1);
            drop = true;
        } else { std::printf("usage: sim_dc [--only kernel | --drop kernel:ordinal]\n"); return 2; }
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
