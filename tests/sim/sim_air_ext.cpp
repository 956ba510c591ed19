// Runs the two __global__ functions of the AIR quotient under Ext weights (air_quotient_ext_kernel and air_quotient_ext_inline_kernel of
// toyni_amd/csrc/toyni_hip.hip, include/toyni_hip.h 3k) themselves on the CPU under the adversarial wave schedules of hip_sim.hpp, the
// way sim_kernels.cpp runs the base kernels.
//
// TEST INFRASTRUCTURE (tests/test_sim_air_ext.py).  What the kernels must write is computed here on the host by a route that shares
// nothing with theirs: the program is interpreted point by point on plain residues (bb_mul_host, bb_inv_host; x_i and Z_H(x_i) as
// powers), and every EMIT adds value x coordinate e of its Ext weight into column e.  The program reads two matrices, with a rotation,
// multiplies, divides by a point off the coset and emits three constraint numbers, one of them twice, divided and undivided.  Cases:
// log N = 10 with B = 2^3 (one workgroup) and log N = 12 with B = 2^8 (four), the 1 / Z_H classes in LDS in both, out_stride = N + 1,
// a c output in the first, accumulation in the second.
//
//   sim_air_ext                       every case under all eight schedules; prints the instantiations and the sites, then ALL OK
//   sim_air_ext --only K              the cases of kernel K alone
//   sim_air_ext --drop K:i            the cases of kernel K with its i-th synchronisation site switched off: DROP ... FAILS / SURVIVES
#include "hip_sim.hpp"

#include <cstdio>
#include <cstring>
#include <set>

#define TOYNI_KERNEL_TEXT_ONLY
#include "toyni_hip.hip"
#include "../emu/contract_case.hpp"

alignas(16) uint32_t air_lds[1u << 14];   // the dynamic LDS of the AIR kernels: 64 KiB

extern "C" {
// every __shared__ array lives in this section; weak: the two kernels here use the dynamic LDS alone, and when no other kernel's static
// array is emitted the section does not exist (both symbols are then null)
extern uint32_t __start_hipsim_lds[] __attribute__((weak)), __stop_hipsim_lds[] __attribute__((weak));
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
constexpr uint32_t NWEIGHTS = 3;

static void run_air_ext(int log_N, int log_blowup, bool inline_weights, bool with_c, bool accumulate) {
    const uint32_t shift = 7;
    sm_state = 0xA1E7ull + (uint64_t)log_N * 31 + (uint64_t)log_blowup;
    NttPlan plan;
    if (!build_plan(log_N, plan)) { CHECK(false, "plan"); return; }
    const size_t N = (size_t)1 << log_N, n = N >> log_blowup, B = (size_t)1 << log_blowup;
    const size_t stride0 = N, stride1 = N + 4, out_stride = N + 1;
    const uint32_t zpoint = 123456789u;   // not on the coset
    // r0 = a(x), r1 = a(g x), r2 = b(x): the constraints  (r1 - r0 r2) [divided, number 0],  (r0 - 5) / (x - z) [undivided, 1],
    // x r2 [divided, 2],  r1 [undivided, 0 again]
    const std::vector<Insn> prog = {{AIR_OP_CELL, 0, 0, 0, 1}, {AIR_OP_CELL, 1, 1, 0, 1}, {AIR_OP_CELL, 2, 0, 1, 2}, {AIR_OP_MUL, 3, 0, 2, 0},
                                    {AIR_OP_SUB, 3, 1, 3, 0}, {AIR_OP_EMIT, 0, 3, 0, 0}, {AIR_OP_CONST, 4, 0, 0, 5}, {AIR_OP_SUB, 4, 0, 4, 0},
                                    {AIR_OP_XINV, 5, 0, 0, zpoint}, {AIR_OP_MUL, 4, 4, 5, 0}, {AIR_OP_EMIT, 0, 4, 1, 1}, {AIR_OP_X, 5, 0, 0, 0},
                                    {AIR_OP_MUL, 5, 5, 2, 0}, {AIR_OP_EMIT, 0, 5, 0, 2}, {AIR_OP_EMIT, 0, 1, 1, 0}};
    std::vector<uint32_t> m0(2 * stride0, SLACK), m1(3 * stride1, SLACK), weights(4 * NWEIGHTS);
    for (size_t c = 0; c < 2; ++c) for (size_t i = 0; i < N; ++i) m0[c * stride0 + i] = i % 97 == 3 ? BB_P - 1u : rnd();
    for (size_t c = 0; c < 3; ++c) for (size_t i = 0; i < N; ++i) m1[c * stride1 + i] = rnd();
    for (uint32_t& w : weights) w = rnd();
    weights[5] = 0u;
    weights[6] = BB_P - 1u;
    const size_t out_words = 3 * out_stride + N;
    std::vector<uint32_t> c_out(out_words, SLACK), q_out(out_words, SLACK);
    if (accumulate)
        for (size_t e = 0; e < 4; ++e) for (size_t i = 0; i < N; ++i) { c_out[e * out_stride + i] = rnd(); q_out[e * out_stride + i] = rnd(); }
    // the host model, on plain residues
    std::vector<uint32_t> want_c = c_out, want_q = q_out;
    {
        const uint32_t w = bb_root_of_unity_host((uint32_t)log_N);
        uint32_t x = shift;
        for (size_t i = 0; i < N; ++i, x = bb_mul_host(x, w)) {
            uint32_t r[6] = {}, cs[4] = {}, us[4] = {};
            for (const Insn& in : prog) {
                switch (in.op) {
                    case AIR_OP_CELL: r[in.dst] = (in.b ? m1[in.imm * stride1 + (i + in.a * B) % N] : m0[in.imm * stride0 + (i + in.a * B) % N]); break;
                    case AIR_OP_CONST: r[in.dst] = in.imm; break;
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
    // what toyni_air_program_create and toyni_air_quotient_ext_device prepare
    std::vector<AirInsn> dev;
    for (const Insn& in : prog)
        dev.push_back(AirInsn{in.op | in.dst << 8 | in.a << 16 | in.b << 24, (in.op == AIR_OP_CONST || in.op == AIR_OP_XINV) ? to_mont_host(in.imm) : in.imm});
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
    if (inline_weights) {
        AirExtInlineWeights in{};
        std::copy(weights.begin(), weights.end(), in.w);
        sim_launch("air_quotient_ext_inline_kernel", "", dim3(grid), shape.threads, [&] { air_quotient_ext_inline_kernel(a, os, in); });
    } else {
        sim_launch("air_quotient_ext_kernel", "", dim3(grid), shape.threads, [&] { air_quotient_ext_kernel(a, os, weights.data()); });
    }
    size_t bad = 0;
    for (size_t k = 0; k < out_words; ++k) bad += c_out[k] != want_c[k] || q_out[k] != want_q[k];   // the words N .. out_stride keep their filler
    CHECK(bad == 0, "air_quotient_ext%s_kernel log_N=%d blow-up 2^%d: %zu words differ from the host model", inline_weights ? "_inline" : "", log_N, log_blowup, bad);
}

static void run_all_cases() {
    if (wanted("air_quotient_ext_kernel")) { run_air_ext(10, 3, false, true, false); run_air_ext(12, 8, false, false, true); }
    if (wanted("air_quotient_ext_inline_kernel")) { run_air_ext(10, 3, true, true, false); run_air_ext(12, 8, true, false, true); }
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
        } else { std::printf("usage: sim_air_ext [--only kernel | --drop kernel:ordinal]\n"); return 2; }
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
