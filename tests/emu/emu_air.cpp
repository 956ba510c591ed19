// Steps the interpreter of constraint programs (air_eval_group, air_zh_inverses, air_cell_load: toyni_amd/csrc/prover_kernels.hpp)
// on the CPU, with the host-side preparation of toyni_air_quotient_device restated here (instruction words, constants in Montgomery
// form, shift^n, w_B, the choice between 1 / Z_H per class and per thread).  The register file has the device's layout for a
// "workgroup" of three threads -- slot r of thread t at regs[(r * 3 + t) * K] -- and owns exactly nregs x 3 x K words, the matrices
// exactly the words their layout owns: an index past either is an AddressSanitizer error, a misaligned 16-byte access a UBSan error.
//     AIR <N> <log_blowup> <shift> <nmats> <ninsns> <nweights> <nregs>
//     MAT <m> <width> <col_stride> <word offset>        (nmats lines)
//     COL <m> <c> <N values>                            (sum of the widths lines)
//     INSN <op> <dst> <a> <b> <imm>                     (ninsns lines, the public form)
//     W <nweights values>
//     C <N values>
//     Q <N values>
//     SHAPE <nregs> <divides> <log_blowup> <threads> <lds bytes> <zh in lds>     (air_launch_shape, the launcher's sizing)
// tests/test_emu_air.py recomputes every word with Python integers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "ntt_plan.hpp"
#include "prover_kernels.hpp"
#include "contract_case.hpp"

using namespace toyni;

// `saturated` as the only argument runs, instead of the cases above, a program whose every product is (p - 1)^2: every cell p - 1,
// the constant and the weight SAT_X, the plain value whose Montgomery form is p - 1 (same record format)

static uint64_t sm_state = 0xA1A1A1ull;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t draw(uint64_t k) {   // {0, 1, p - 1, random}
    switch (k % 5) {
        case 0: return 0u;
        case 1: return 1u;
        case 2: return BB_P - 1u;
        default: return (uint32_t)(splitmix() % BB_P);
    }
}

struct Insn { uint32_t op, dst, a, b, imm; };
struct Mat { uint32_t width; uint64_t stride; uint32_t offset; uint32_t* store; uint32_t* m; };

// a random valid program over `nregs` registers: the first instructions write every register once, the rest read any two
static std::vector<Insn> random_program(uint32_t nregs, uint32_t length, const std::vector<Mat>& mats, uint64_t rows, uint32_t nconstraints,
                                        uint32_t xinv_point, bool may_divide) {
    std::vector<Insn> p;
    for (uint32_t k = 0; p.size() + nconstraints + 1 < length || k < nregs; ++k) {
        Insn in{};
        in.dst = k < nregs ? k : (uint32_t)(splitmix() % nregs);
        const uint32_t written = std::min(k, nregs);
        const uint32_t kind = k < 4 ? k : (uint32_t)(splitmix() % 9);
        if (kind == 0 || written == 0) {
            in.op = AIR_OP_CELL;
            in.b = (uint32_t)(splitmix() % mats.size());
            in.imm = (uint32_t)(splitmix() % mats[in.b].width);
            in.a = (k % 3 == 2) ? (uint32_t)std::min<uint64_t>(rows - 1, 255) : (uint32_t)(splitmix() % std::min<uint64_t>(rows, 256));
        } else if (kind == 1) {
            in.op = AIR_OP_CONST;
            in.imm = draw(k);
        } else if (kind == 2) {
            in.op = AIR_OP_X;
        } else if (kind == 3) {
            in.op = AIR_OP_XINV;
            in.imm = xinv_point;
        } else {
            in.op = AIR_OP_ADD + (kind - 4) % 3;
            in.a = (uint32_t)(splitmix() % written);
            in.b = (uint32_t)(splitmix() % written);
        }
        p.push_back(in);
    }
    for (uint32_t k = 0; k <= nconstraints; ++k)   // every number once, number 0 twice, alternately divided and undivided
        p.push_back(Insn{AIR_OP_EMIT, 0, (uint32_t)(splitmix() % nregs), may_divide ? k & 1u : 1u, k % nconstraints});
    return p;
}

static void air_case(int log_N, int log_blowup, uint32_t shift, std::vector<Mat> mats, const std::vector<Insn>& prog, uint32_t nweights, bool zh_classes,
                     bool sat = false) {
    TOYNI_CONTRACT_TAG("air_eval_group log_N=%d log_blowup=%d ninsns=%zu zh_classes=%d sat=%d", log_N, log_blowup, prog.size(), (int)zh_classes, (int)sat);
    NttPlan plan;
    if (!build_plan(log_N, plan)) { std::printf("FAIL plan\n"); return; }
    const uint64_t N = 1ull << log_N, n = N >> log_blowup;
    for (Mat& m : mats) {
        const size_t words = (size_t)(m.width - 1) * m.stride + N;
        m.store = static_cast<uint32_t*>(::operator new((words + m.offset) * sizeof(uint32_t), std::align_val_t(16)));
        m.m = m.store + m.offset;
        for (size_t k = 0; k < words; ++k) m.m[k] = 0xFFFFFFF0u;
        for (uint32_t c = 0; c < m.width; ++c)
            for (uint64_t i = 0; i < N; ++i) m.m[c * m.stride + i] = sat ? BB_P - 1u : draw(splitmix());
    }
    std::vector<uint32_t> weights(nweights);
    for (uint32_t k = 0; k < nweights; ++k) weights[k] = sat ? SAT_X : draw(k + 3);
    // what toyni_air_program_create and toyni_air_quotient_device prepare
    std::vector<AirInsn> dev(prog.size());
    uint32_t nregs = 0, divides = 0;
    for (size_t k = 0; k < prog.size(); ++k) {
        const Insn& in = prog[k];
        dev[k].w0 = in.op | in.dst << 8 | in.a << 16 | in.b << 24;
        dev[k].imm = (in.op == AIR_OP_CONST || in.op == AIR_OP_XINV) ? to_mont_host(in.imm) : in.imm;
        if (in.op != AIR_OP_EMIT) nregs = std::max(nregs, in.dst + 1);
        else if (in.b == 0) divides = 1;
    }
    AirArgs a{};
    a.insns = dev.data();
    for (size_t m = 0; m < mats.size(); ++m) { a.mat[m] = mats[m].m; a.col_stride[m] = mats[m].stride; }
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.ninsns = (uint32_t)prog.size();
    a.nregs = nregs;
    a.log_N = (uint32_t)log_N;
    a.log_blowup = (uint32_t)log_blowup;
    a.wNR = to_mont_host(bb_root_of_unity_host((uint32_t)log_N));
    a.shift_nR = to_mont_host(bb_pow_host(shift, n));
    a.wBR = to_mont_host(bb_pow_host(bb_root_of_unity_host((uint32_t)log_N), n));
    a.divides = divides;
    const AirLaunchShape shape = air_launch_shape(nregs, divides, (uint32_t)log_blowup);   // what the launcher decides ...
    a.zh_lds = shape.zh_lds && zh_classes;                                                // ... or the per-thread form where the case asks for it
    std::vector<uint32_t> classes;
    if (a.zh_lds)
        for (uint32_t t = 0; t < (1u << log_blowup); ++t) classes.push_back(zh_inv_class(a.shift_nR, a.wBR, t));
    std::vector<uint32_t> c_out(N), q_out(N);
    constexpr uint32_t T = 3;
    const uint32_t K = log_N >= 2 ? 4 : 1;
    uint32_t* regs = static_cast<uint32_t*>(::operator new((size_t)nregs * T * K * sizeof(uint32_t), std::align_val_t(16)));
    for (uint64_t g = 0; g < N / K; ++g) {
        uint32_t* mine = regs + (g % T) * K;
        const uint64_t i0 = g * K;
        if (K == 4) {
            uint32_t zh[4] = {0, 0, 0, 0}, c[4], q[4];
            if (a.zh_lds) for (int j = 0; j < 4; ++j) zh[j] = classes[(i0 + j) & ((1u << log_blowup) - 1)];
            else if (a.divides) air_zh_inverses<4>(a, i0, zh);
            air_eval_group<4>(a, weights.data(), mine, T * K, i0, zh, c, q);
            for (int j = 0; j < 4; ++j) { c_out[i0 + j] = c[j]; q_out[i0 + j] = q[j]; }
        } else {
            uint32_t zh[1] = {0}, c[1], q[1];
            if (a.zh_lds) zh[0] = classes[i0 & ((1u << log_blowup) - 1)];
            else if (a.divides) air_zh_inverses<1>(a, i0, zh);
            air_eval_group<1>(a, weights.data(), mine, T * K, i0, zh, c, q);
            c_out[i0] = c[0];
            q_out[i0] = q[0];
        }
    }
    ::operator delete(regs, std::align_val_t(16));
    std::printf("AIR %llu %d %u %zu %zu %u %u\n", (unsigned long long)N, log_blowup, shift, mats.size(), prog.size(), nweights, nregs);
    for (size_t m = 0; m < mats.size(); ++m) std::printf("MAT %zu %u %llu %u\n", m, mats[m].width, (unsigned long long)mats[m].stride, mats[m].offset);
    for (size_t m = 0; m < mats.size(); ++m)
        for (uint32_t c = 0; c < mats[m].width; ++c) {
            std::printf("COL %zu %u", m, c);
            for (uint64_t i = 0; i < N; ++i) std::printf(" %u", mats[m].m[c * mats[m].stride + i]);
            std::printf("\n");
        }
    for (const Insn& in : prog) std::printf("INSN %u %u %u %u %u\n", in.op, in.dst, in.a, in.b, in.imm);
    std::printf("W");
    for (uint32_t w : weights) std::printf(" %u", w);
    std::printf("\nC");
    for (uint32_t v : c_out) std::printf(" %u", v);
    std::printf("\nQ");
    for (uint32_t v : q_out) std::printf(" %u", v);
    std::printf("\n");
    for (Mat& m : mats) ::operator delete(m.store, std::align_val_t(16));
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "saturated") {
        // cell * SAT_X, that times the next row's cell, emitted under weight SAT_X: the first product undivided, the second divided by Z_H under both weights
        const std::vector<Insn> prog = {{AIR_OP_CELL, 0, 0, 0, 0}, {AIR_OP_CONST, 1, 0, 0, SAT_X}, {AIR_OP_MUL, 2, 0, 1, 0}, {AIR_OP_CELL, 0, 1, 0, 1},
                                        {AIR_OP_MUL, 3, 2, 0, 0}, {AIR_OP_EMIT, 0, 2, 1, 0}, {AIR_OP_EMIT, 0, 3, 0, 1}, {AIR_OP_EMIT, 0, 3, 0, 0}};
        for (int log_blowup : {0, 2})
            for (bool classes : {true, false}) air_case(6, log_blowup, SAT_X, {Mat{2, 64, 0, nullptr, nullptr}}, prog, 2, classes, true);
        std::printf("DONE\n");
        return 0;
    }
    const int log_Ns[] = {1, 2, 3, 6};
    uint32_t k = 0;
    for (int log_N : log_Ns) {
        const uint64_t N = 1ull << log_N;
        for (int log_blowup = 0; log_blowup < log_N; ++log_blowup) {
            // the Fibonacci quotient (src/fibonacci.rs:133-150)
            const uint64_t n = N >> log_blowup;
            const uint32_t g = bb_root_of_unity_host((uint32_t)(log_N - log_blowup));
            const std::vector<Insn> fib = {
                {AIR_OP_CELL, 0, 0, 0, 0}, {AIR_OP_CELL, 1, 1 % (uint32_t)n, 0, 0}, {AIR_OP_CELL, 2, 2 % (uint32_t)n, 0, 0}, {AIR_OP_ADD, 0, 1, 0, 0},
                {AIR_OP_SUB, 0, 2, 0, 0}, {AIR_OP_X, 1, 0, 0, 0}, {AIR_OP_CONST, 2, 0, 0, bb_pow_host(g, n - 1)}, {AIR_OP_SUB, 2, 1, 2, 0},
                {AIR_OP_MUL, 0, 0, 2, 0}, {AIR_OP_CONST, 2, 0, 0, bb_pow_host(g, n - 2)}, {AIR_OP_SUB, 2, 1, 2, 0}, {AIR_OP_MUL, 0, 0, 2, 0},
                {AIR_OP_EMIT, 0, 0, 0, 0}};
            for (uint32_t off = 0; off < 2; ++off, ++k) air_case(log_N, log_blowup, 7u, {Mat{1, N, off, nullptr, nullptr}}, fib, 1, off == 0);
        }
        for (uint32_t nregs : {1u, 7u, 64u})
            for (uint32_t nmats : {1u, 2u, 4u}) {
                ++k;
                const int log_blowup = (int)(k % (uint32_t)(log_N + 1));
                const uint64_t rows = N >> log_blowup;
                std::vector<Mat> mats;
                for (uint32_t m = 0; m < nmats; ++m) mats.push_back(Mat{1 + (k + 2 * m) % 5, N + ((k + m) % 3 ? 0u : 5u), (k + m) % 4, nullptr, nullptr});
                // shift 1: the XINV constant w_N^(N - 1) is the coset's last point (Z_H vanishes on that coset: nothing is divided);
                // otherwise the point is random
                const bool on_coset = k % 2 == 0;
                const uint32_t shift = on_coset ? 1u : 7u;
                const uint32_t point = on_coset ? bb_pow_host(bb_root_of_unity_host((uint32_t)log_N), N - 1) : (uint32_t)(splitmix() % BB_P);
                const uint32_t ncons = 1 + k % 3;
                air_case(log_N, log_blowup, shift, mats, random_program(nregs, nregs == 64 ? 200 : 40, mats, rows, ncons, point, !on_coset), ncons + k % 2, k % 4 < 2);
            }
    }
    // the launcher's arithmetic for every register count: SHAPE <nregs> <divides> <log_blowup> <threads> <lds bytes> <zh in lds>
    for (uint32_t nregs = 1; nregs <= AIR_MAX_REGS; ++nregs)
        for (uint32_t divides = 0; divides < 2; ++divides)
            for (uint32_t lb : {0u, 5u, 8u, 9u, 27u}) {
                const AirLaunchShape sh = air_launch_shape(nregs, divides, lb);
                std::printf("SHAPE %u %u %u %u %u %u\n", nregs, divides, lb, sh.threads, sh.lds_bytes, sh.zh_lds);
            }
    std::printf("DONE\n");
    return 0;
}
