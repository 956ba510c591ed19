// Steps the interpreter of constraint programs under Ext weights (air_eval_group_ext, air_ext_store and the helpers they share with
// the base interpreter: toyni_amd/csrc/prover_kernels.hpp, include/toyni_hip.h 3k) on the CPU, as emu_air.cpp steps the base one, with
// the host-side preparation of toyni_air_quotient_ext_device restated here.  The register file has the device's layout for a workgroup
// of air_launch_shape's thread count -- slot r of thread t at regs[(r * threads + t) * K] -- and owns exactly nregs x threads x K
// words; the matrices and the two outputs own exactly the words their layout names (four columns out_stride apart, the last one N
// words long): an index past any of them is an AddressSanitizer error, a misaligned 16-byte access a UBSan error.  The words between
// N and out_stride of an output column must keep their filler (FAIL otherwise).
//     AIRX <N> <log_blowup> <shift> <nmats> <ninsns> <nweights> <nregs> <out_stride> <accumulate> <has c> <threads> <out word offset>
//     MAT <m> <width> <col_stride> <word offset>        (nmats lines)
//     COL <m> <c> <N values>                            (sum of the widths lines)
//     INSN <op> <dst> <a> <b> <imm>                     (ninsns lines, the public form)
//     W <4 nweights values>                             (coordinate e of weight k at 4 k + e)
//     PREC <e> <N values>  PREQ <e> <N values>          (four lines each, what the outputs held before an accumulating call; PREC only
//                                                       with a c output)
//     C <e> <N values>                                  (four lines, only with a c output)
//     Q <e> <N values>                                  (four lines)
// tests/test_emu_air_ext.py recomputes every word with the numpy model of the base instruction set, run four times under the
// coordinates of the weights.  `saturated` as the only argument: every data word and every weight coordinate p - 1, the constant SAT_X.
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

static uint64_t sm_state = 0xE7A1A1ull;
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
struct Out { uint64_t stride; uint32_t offset; bool accumulate, has_c; };
constexpr uint32_t FILL = 0xFFFFFFF0u;
static int failures = 0;

// a random valid program over `nregs` registers (emu_air.cpp's generator): the first instructions write every register once, the
// rest read any two; every constraint number is emitted once and number 0 twice, alternately divided and undivided
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
    for (uint32_t k = 0; k <= nconstraints; ++k)
        p.push_back(Insn{AIR_OP_EMIT, 0, (uint32_t)(splitmix() % nregs), may_divide ? k & 1u : 1u, k % nconstraints});
    return p;
}

static void print_column(const char* tag, int e, const uint32_t* v, uint64_t N) {
    std::printf("%s %d", tag, e);
    for (uint64_t i = 0; i < N; ++i) std::printf(" %u", v[i]);
    std::printf("\n");
}

static void air_ext_case(int log_N, int log_blowup, uint32_t shift, std::vector<Mat> mats, const std::vector<Insn>& prog, uint32_t nweights, Out o,
                         bool sat = false) {
    TOYNI_CONTRACT_TAG("air_eval_group_ext log_N=%d log_blowup=%d ninsns=%zu stride=%llu acc=%d sat=%d", log_N, log_blowup, prog.size(),
                       (unsigned long long)o.stride, (int)o.accumulate, (int)sat);
    NttPlan plan;
    if (!build_plan(log_N, plan)) { std::printf("FAIL plan\n"); ++failures; return; }
    const uint64_t N = 1ull << log_N, n = N >> log_blowup;
    for (Mat& m : mats) {
        const size_t words = (size_t)(m.width - 1) * m.stride + N;
        m.store = static_cast<uint32_t*>(::operator new((words + m.offset) * sizeof(uint32_t), std::align_val_t(16)));
        m.m = m.store + m.offset;
        for (size_t k = 0; k < words; ++k) m.m[k] = FILL;
        for (uint32_t c = 0; c < m.width; ++c)
            for (uint64_t i = 0; i < N; ++i) m.m[c * m.stride + i] = sat ? BB_P - 1u : draw(splitmix());
    }
    std::vector<uint32_t> weights(4 * (size_t)nweights);
    for (size_t k = 0; k < weights.size(); ++k) weights[k] = sat ? BB_P - 1u : draw(k + 3);
    // what toyni_air_program_create and toyni_air_quotient_ext_device prepare
    std::vector<AirInsn> dev(prog.size());
    uint32_t nregs = 0, divides = 0;
    for (size_t k = 0; k < prog.size(); ++k) {
        const Insn& in = prog[k];
        dev[k].w0 = in.op | in.dst << 8 | in.a << 16 | in.b << 24;
        dev[k].imm = (in.op == AIR_OP_CONST || in.op == AIR_OP_XINV) ? to_mont_host(in.imm) : in.imm;
        if (in.op != AIR_OP_EMIT) nregs = std::max(nregs, in.dst + 1);
        else if (in.b == 0) divides = 1;
    }
    // the outputs: exactly the words of four columns, o.offset words past a 16-byte boundary
    const size_t out_words = 3 * (size_t)o.stride + N;
    uint32_t* stores[2];
    uint32_t* outs[2];
    for (int t = 0; t < 2; ++t) {
        stores[t] = static_cast<uint32_t*>(::operator new((out_words + o.offset) * sizeof(uint32_t), std::align_val_t(16)));
        outs[t] = stores[t] + o.offset;
        for (size_t k = 0; k < out_words; ++k) outs[t][k] = FILL;
        if (o.accumulate && (t == 1 || o.has_c))
            for (int e = 0; e < 4; ++e)
                for (uint64_t i = 0; i < N; ++i) outs[t][e * o.stride + i] = sat ? BB_P - 1u : draw(splitmix());
    }
    AirArgs a{};
    a.insns = dev.data();
    for (size_t m = 0; m < mats.size(); ++m) { a.mat[m] = mats[m].m; a.col_stride[m] = mats[m].stride; }
    a.c_out = o.has_c ? outs[0] : nullptr;
    a.q_out = outs[1];
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
    a.accumulate = o.accumulate ? 1u : 0u;
    const AirLaunchShape shape = air_launch_shape(nregs, divides, (uint32_t)log_blowup);
    a.zh_lds = shape.zh_lds;
    std::vector<uint32_t> classes;
    if (a.zh_lds)
        for (uint32_t t = 0; t < (1u << log_blowup); ++t) classes.push_back(zh_inv_class(a.shift_nR, a.wBR, t));

    std::printf("AIRX %llu %d %u %zu %zu %u %u %llu %d %d %u %u\n", (unsigned long long)N, log_blowup, shift, mats.size(), prog.size(), nweights, nregs,
                (unsigned long long)o.stride, (int)o.accumulate, (int)o.has_c, shape.threads, o.offset);
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
    std::printf("\n");
    if (o.accumulate)
        for (int t = o.has_c ? 0 : 1; t < 2; ++t)
            for (int e = 0; e < 4; ++e) print_column(t ? "PREQ" : "PREC", e, outs[t] + e * o.stride, N);

    const uint32_t T = shape.threads;
    const uint32_t K = log_N >= 2 ? 4 : 1;
    uint32_t* regs = static_cast<uint32_t*>(::operator new((size_t)nregs * T * K * sizeof(uint32_t), std::align_val_t(16)));
    for (uint64_t g = 0; g < N / K; ++g) {
        uint32_t* mine = regs + (g % T) * K;
        const uint64_t i0 = g * K;
        if (K == 4) {
            uint32_t zh[4] = {0, 0, 0, 0}, c[4][4], q[4][4];
            if (a.zh_lds) for (int j = 0; j < 4; ++j) zh[j] = classes[(i0 + j) & ((1u << log_blowup) - 1)];
            else if (a.divides) air_zh_inverses<4>(a, i0, zh);
            air_eval_group_ext<4>(a, weights.data(), mine, T * K, i0, zh, c, q);
            air_ext_store<4>(a.c_out, o.stride, i0, a.accumulate, c);
            air_ext_store<4>(a.q_out, o.stride, i0, a.accumulate, q);
        } else {
            uint32_t zh[1] = {0}, c[4][1], q[4][1];
            if (a.zh_lds) zh[0] = classes[i0 & ((1u << log_blowup) - 1)];
            else if (a.divides) air_zh_inverses<1>(a, i0, zh);
            air_eval_group_ext<1>(a, weights.data(), mine, T * K, i0, zh, c, q);
            air_ext_store<1>(a.c_out, o.stride, i0, a.accumulate, c);
            air_ext_store<1>(a.q_out, o.stride, i0, a.accumulate, q);
        }
    }
    ::operator delete(regs, std::align_val_t(16));
    for (int t = 0; t < 2; ++t) {
        for (int e = 0; e < 3; ++e)
            for (uint64_t i = N; i < o.stride; ++i)
                if (outs[t][e * o.stride + i] != FILL) { std::printf("FAIL a word between N and out_stride was written (output %d column %d)\n", t, e); ++failures; }
        if (t == 0 && !o.has_c) {
            for (size_t k = 0; k < out_words; ++k)
                if (outs[0][k] != FILL) { std::printf("FAIL a null c output was written\n"); ++failures; break; }
            continue;
        }
        for (int e = 0; e < 4; ++e) print_column(t ? "Q" : "C", e, outs[t] + e * o.stride, N);
    }
    for (int t = 0; t < 2; ++t) ::operator delete(stores[t], std::align_val_t(16));
    for (Mat& m : mats) ::operator delete(m.store, std::align_val_t(16));
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "saturated") {
        // cell * SAT_X, that times the next row's cell; the first product undivided, the second divided by Z_H under both weights
        const std::vector<Insn> prog = {{AIR_OP_CELL, 0, 0, 0, 0}, {AIR_OP_CONST, 1, 0, 0, SAT_X}, {AIR_OP_MUL, 2, 0, 1, 0}, {AIR_OP_CELL, 0, 1, 0, 1},
                                        {AIR_OP_MUL, 3, 2, 0, 0}, {AIR_OP_EMIT, 0, 2, 1, 0}, {AIR_OP_EMIT, 0, 3, 0, 1}, {AIR_OP_EMIT, 0, 3, 0, 0}};
        for (int log_blowup : {0, 2})
            for (bool acc : {false, true}) air_ext_case(6, log_blowup, SAT_X, {Mat{2, 64, 0, nullptr, nullptr}}, prog, 2, Out{64u + (acc ? 1u : 0u), 0, acc, true}, true);
        std::printf("%s\n", failures ? "FAILED" : "DONE");
        return failures ? 1 : 0;
    }
    uint32_t k = 0;
    // N = 1, 2, 4, 8, every blow-up 1, 2, 4 that fits: random programs over 7 registers and two matrices, every output option in turn
    for (int log_N : {0, 1, 2, 3})
        for (int log_blowup = 0; log_blowup <= std::min(log_N, 2); ++log_blowup)
            for (uint32_t v = 0; v < 4; ++v, ++k) {
                const uint64_t N = 1ull << log_N, rows = N >> log_blowup;
                std::vector<Mat> mats = {Mat{2, N + (v & 1u ? 5u : 0u), v == 3 ? 1u : 0u, nullptr, nullptr}, Mat{3, N, 0, nullptr, nullptr}};
                const bool on_coset = v == 2;   // shift 1: Z_H vanishes on the coset, nothing is divided, and the XINV point lies on it
                const uint32_t shift = on_coset ? 1u : 7u;
                const uint32_t point = on_coset ? bb_pow_host(bb_root_of_unity_host((uint32_t)log_N), N - 1) : (uint32_t)(splitmix() % BB_P);
                const uint32_t ncons = 1 + k % 3;
                const Out o{N + (v == 1 ? 1u : v == 3 ? 4u : 0u), v == 2 ? 1u : 0u, (k & 2u) != 0, v != 1};
                air_ext_case(log_N, log_blowup, shift, mats, random_program(7, 24, mats, rows, ncons, point, !on_coset), ncons + k % 2, o);
            }
    // rotation 1 with B = 2: the cell of the next row is two words on, never a 16-byte load
    {
        const std::vector<Insn> prog = {{AIR_OP_CELL, 0, 0, 0, 0}, {AIR_OP_CELL, 1, 1, 0, 0}, {AIR_OP_CELL, 2, 1, 0, 1}, {AIR_OP_MUL, 3, 1, 2, 0},
                                        {AIR_OP_SUB, 3, 3, 0, 0}, {AIR_OP_EMIT, 0, 3, 0, 0}, {AIR_OP_EMIT, 0, 1, 1, 1}, {AIR_OP_EMIT, 0, 2, 0, 0}};
        for (int log_N : {1, 2, 3, 6})
            for (uint32_t pad : {0u, 1u}) air_ext_case(log_N, 1, 7u, {Mat{2, 1ull << log_N, 0, nullptr, nullptr}}, prog, 2, Out{(1ull << log_N) + pad, 0, pad != 0, true});
    }
    // the three thread counts of air_launch_shape -- 16 registers: 256 threads, 32: 128, 64: 64 -- over several workgroups' worth of
    // groups, with and without a divided constraint, out_stride = N + 1
    for (uint32_t nregs : {16u, 32u, 64u})
        for (bool divide : {true, false}) {
            ++k;
            const int log_N = 11, log_blowup = 3;
            const uint64_t N = 1ull << log_N;
            std::vector<Mat> mats = {Mat{4, N, 0, nullptr, nullptr}, Mat{8, N + 3, divide ? 0u : 3u, nullptr, nullptr}};
            air_ext_case(log_N, log_blowup, 7u, mats, random_program(nregs, nregs == 64 ? 160 : 80, mats, N >> log_blowup, 4, (uint32_t)(splitmix() % BB_P), divide), 4,
                         Out{N + (divide ? 1u : 0u), 0, !divide, divide});
        }
    std::printf("%s\n", failures ? "FAILED" : "DONE");
    return failures ? 1 : 0;
}
