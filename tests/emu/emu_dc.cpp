// Steps the challenge-dependent preparation of include/toyni_hip.h 3p (toyni_amd/csrc/dc_kernels.hpp: the text the two one-wave
// kernels and the record-fed twins run) on the CPU.  TEST INFRASTRUCTURE (tests/test_emu_dc.py builds it under AddressSanitizer +
// UBSan; tests/test_field_contracts_dc.py rebuilds it with tests/emu/field_contracts.hpp in front).  Every input and output lives in
// a heap block of exactly its size.  Argument `cases` or `saturated`; no stdin.
//
// 1. The quotient's record: for raw parameter and alpha words (0xFFFFFFFF, p, p + 1 among them), both weight forms, stepped as a wave
//    of 1 and of 64 lanes, compared with memcmp against the HOST code -- to_mont_host of the reduced parameters, the rule of
//    air_ext_weights restated in host_weights below -- and printed for the test to judge against Python integers:
//      QPREP nparams nalphas form  |  PAR <words>  |  AL <words>  |  REC <nparams + 4 nweights words>
// 2. The scan's record: per (num index, den index, width-1 denominator) against the reduced shifts and ext_shift_host of the negated
//    denominator shift, as toyni_column_scan_ext_device builds them:
//      SPREP num_index den_index den_norm  |  CH <12 words>  |  SREC <24 words>
// 3. PARAM: air_eval_group_ext_dc on a program with PARAMs and the record of 1, against air_eval_group_ext on the program with CONST
//    (word mod p) in their places under the host's weights, same matrices, same points, K = 4 and K = 1: the c and q words are
//    compared with memcmp (EVAL lines name what ran).
// 4. The record-fed scan bodies: ext_accum_group_terms on arguments filled by ext_accum_args_from_record from the record of 2, against
//    the same call on arguments the host fills, every operand form, both ops (TERMS lines).
// The last lines are BAD <mismatches> and DONE.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "ntt_plan.hpp"
#include "dc_kernels.hpp"
#include "contract_case.hpp"

using namespace toyni;

static uint64_t rng_state = 0xDC0FFEEull;
static uint64_t splitmix() {
    rng_state += 0x9E3779B97F4A7C15ull;
    uint64_t x = rng_state;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static bool g_saturated = false;
// a raw word of device memory: any u32; saturated: one that reduces to p - 1, or the largest word there is
static uint32_t raw_word(uint64_t k) {
    if (g_saturated) return k & 1u ? 0xFFFFFFFFu : 2u * BB_P - 1u;
    switch (k % 7) {
        case 0: return 0xFFFFFFFFu;
        case 1: return BB_P;
        case 2: return BB_P + 1u;
        case 3: return 0u;
        default: return (uint32_t)splitmix();
    }
}
static uint32_t data_word() { return g_saturated ? BB_P - 1u : (uint32_t)(splitmix() % BB_P); }
static void print_words(const char* tag, const uint32_t* w, size_t count) {
    printf("%s", tag);
    for (size_t i = 0; i < count; ++i) printf(" %u", w[i]);
    printf("\n");
}
static int bad = 0;

// the rule of toyni_amd.prover.air_ext_weights: W_{4 k + j} = alpha_k X^j, X^4 = 11, on canonical residues
static std::vector<uint32_t> host_weights(const std::vector<uint32_t>& alphas_reduced, uint32_t form) {
    const size_t nalphas = alphas_reduced.size() / 4;
    if (form == AIR_WEIGHTS_EXT) return alphas_reduced;
    std::vector<uint32_t> w(16 * nalphas, 0u);
    for (size_t k = 0; k < nalphas; ++k)
        for (int j = 0; j < 4; ++j)
            for (int e = 0; e < 4; ++e) {
                const uint32_t a = alphas_reduced[4 * k + e];
                w[16 * k + 4 * j + (e + j) % 4] = e + j >= 4 ? bb_mul_host(a, EXT_W) : a;
            }
    return w;
}
struct QuotientRecord {
    std::vector<uint32_t> params_raw, alphas_raw, rec;     // rec: what the device text wrote
    std::vector<uint32_t> params_reduced, weights;         // what the host-argument call would be given
};
static QuotientRecord quotient_record(uint32_t nparams, uint32_t nalphas, uint32_t form, uint32_t nlanes, bool print) {
    TOYNI_CONTRACT_TAG("emu_dc quotient record nparams=%u nalphas=%u form=%u nlanes=%u", nparams, nalphas, form, nlanes);
    QuotientRecord r;
    for (uint32_t j = 0; j < nparams; ++j) r.params_raw.push_back(raw_word(j + nparams));
    for (uint32_t k = 0; k < 4 * nalphas; ++k) r.alphas_raw.push_back(raw_word(k));
    std::unique_ptr<uint32_t[]> par(new uint32_t[nparams ? nparams : 1]), al(new uint32_t[4 * nalphas]);
    if (nparams) memcpy(par.get(), r.params_raw.data(), 4 * nparams);
    memcpy(al.get(), r.alphas_raw.data(), 16 * nalphas);
    const size_t words = air_dc_record_words(nparams, nalphas, form);
    std::unique_ptr<uint32_t[]> rec(new uint32_t[words]);
    memset(rec.get(), 0xA5, 4 * words);
    for (uint32_t lane = nlanes; lane-- > 0;) air_dc_prepare(nparams ? par.get() : nullptr, nparams, al.get(), nalphas, form, rec.get(), lane, nlanes);
    r.rec.assign(rec.get(), rec.get() + words);
    std::vector<uint32_t> want, reduced;
    for (uint32_t w : r.params_raw) { r.params_reduced.push_back(w % BB_P); want.push_back(to_mont_host(w % BB_P)); }
    for (uint32_t w : r.alphas_raw) reduced.push_back(w % BB_P);
    r.weights = host_weights(reduced, form);
    want.insert(want.end(), r.weights.begin(), r.weights.end());
    if (want.size() != words || memcmp(want.data(), r.rec.data(), 4 * words)) { ++bad; printf("MISMATCH quotient record\n"); }
    if (print) {
        printf("QPREP %u %u %u\n", nparams, nalphas, form);
        print_words("PAR", r.params_raw.data(), nparams);
        print_words("AL", r.alphas_raw.data(), 4 * nalphas);
        print_words("REC", r.rec.data(), words);
    }
    return r;
}

struct ScanRecord { uint32_t chal[12]; ExtAccumRecord rec; uint32_t num_shift[4], den_shift[4]; ExtShift den_inv; };
static ScanRecord scan_record(uint32_t num_index, uint32_t den_index, uint32_t den_norm, const uint32_t* base_gamma, bool print) {
    TOYNI_CONTRACT_TAG("emu_dc scan record num=%u den=%u norm=%u", num_index, den_index, den_norm);
    ScanRecord r{};
    for (int k = 0; k < 12; ++k) r.chal[k] = raw_word(splitmix());
    if (base_gamma) memcpy(r.chal + 8, base_gamma, 16);                      // challenge 2: the caller's (a gamma in the base field)
    std::unique_ptr<uint32_t[]> ch(new uint32_t[12]);
    memcpy(ch.get(), r.chal, 48);
    ExtAccumRecord* rec = static_cast<ExtAccumRecord*>(aligned_alloc(16, sizeof(ExtAccumRecord)));
    memset(rec, 0xA5, sizeof *rec);
    const bool named = num_index != EXT_SHIFT_NONE || den_index != EXT_SHIFT_NONE;
    for (uint32_t lane = 64; lane-- > 0;) ext_accum_dc_prepare(named ? ch.get() : nullptr, num_index, den_index, den_norm, rec, lane);
    r.rec = *rec;
    free(rec);
    // what toyni_column_scan_ext_device does with host shifts
    for (int k = 0; k < 4; ++k) {
        r.num_shift[k] = num_index == EXT_SHIFT_NONE ? 0u : r.chal[4 * num_index + k] % BB_P;
        r.den_shift[k] = den_index == EXT_SHIFT_NONE ? 0u : r.chal[4 * den_index + k] % BB_P;
    }
    if (den_norm) {
        uint32_t z[4];
        for (int k = 0; k < 4; ++k) z[k] = r.den_shift[k] ? BB_P - r.den_shift[k] : 0u;
        r.den_inv = ext_shift_host(z);
    }
    if (memcmp(r.rec.num_shift, r.num_shift, 16) || memcmp(r.rec.den_shift, r.den_shift, 16) || memcmp(&r.rec.den_inv, &r.den_inv, sizeof(ExtShift))) {
        ++bad;
        printf("MISMATCH scan record\n");
    }
    if (print) {
        printf("SPREP %u %u %u\n", num_index, den_index, den_norm);
        print_words("CH", r.chal, 12);
        print_words("SREC", reinterpret_cast<const uint32_t*>(&r.rec), sizeof(ExtAccumRecord) / 4);
    }
    return r;
}

// ---- 3. PARAM against CONST ----
struct Insn { uint32_t op, dst, a, b, imm; };
static std::vector<AirInsn> device_form(const std::vector<Insn>& prog) {
    std::vector<AirInsn> dev(prog.size());
    for (size_t k = 0; k < prog.size(); ++k) {
        const Insn& in = prog[k];
        dev[k].w0 = in.op | in.dst << 8 | in.a << 16 | in.b << 24;
        dev[k].imm = (in.op == AIR_OP_CONST || in.op == AIR_OP_XINV) ? to_mont_host(in.imm) : in.imm;
    }
    return dev;
}
template <int K>
static void eval_both(const AirArgs& with_params, const AirArgs& with_consts, const QuotientRecord& r, uint32_t nparams, uint32_t nregs, uint64_t N) {
    std::unique_ptr<uint32_t[]> rec(new uint32_t[r.rec.size()]), wts(new uint32_t[r.weights.size()]);
    memcpy(rec.get(), r.rec.data(), 4 * r.rec.size());
    memcpy(wts.get(), r.weights.data(), 4 * r.weights.size());
    uint32_t* regs[2];
    for (int t = 0; t < 2; ++t) regs[t] = static_cast<uint32_t*>(::operator new((size_t)nregs * K * sizeof(uint32_t), std::align_val_t(16)));
    for (uint64_t i0 = 0; i0 < N; i0 += K) {
        uint32_t zh[K], c[2][4][K], q[2][4][K];
        if (with_consts.divides) air_zh_inverses<K>(with_consts, i0, zh);
        else for (int j = 0; j < K; ++j) zh[j] = 0u;
        air_eval_group_ext_dc<K>(with_params, rec.get(), rec.get() + nparams, regs[0], K, i0, zh, c[0], q[0]);
        air_eval_group_ext<K>(with_consts, wts.get(), regs[1], K, i0, zh, c[1], q[1]);
        if (memcmp(c[0], c[1], sizeof c[0]) || memcmp(q[0], q[1], sizeof q[0])) { ++bad; printf("MISMATCH eval i0=%llu\n", (unsigned long long)i0); }
    }
    for (int t = 0; t < 2; ++t) ::operator delete(regs[t], std::align_val_t(16));
}
static void param_case(int log_N, int log_blowup, uint32_t nparams, uint32_t nalphas, uint32_t form) {
    TOYNI_CONTRACT_TAG("emu_dc PARAM log_N=%d log_blowup=%d nparams=%u nalphas=%u form=%u", log_N, log_blowup, nparams, nalphas, form);
    NttPlan plan;
    if (!build_plan(log_N, plan)) { ++bad; printf("MISMATCH plan\n"); return; }
    const uint64_t N = 1ull << log_N, n = N >> log_blowup;
    const QuotientRecord r = quotient_record(nparams, nalphas, form, 64, false);
    const uint32_t ncons = (uint32_t)r.weights.size() / 4;
    const uint32_t hi = nparams - 1, lo = 0;
    // registers 0..5; the constraints use the first, the last and (emit_ext form: 4 weights per alpha) a middle weight
    const uint32_t shift = g_saturated ? SAT_X : 7u;
    const std::vector<Insn> prog = {
        {AIR_OP_CELL, 0, 0, 0, 0}, {AIR_OP_PARAM, 1, 0, 0, hi}, {AIR_OP_MUL, 2, 0, 1, 0}, {AIR_OP_CELL, 3, n > 1 ? 1u : 0u, 0, 1}, {AIR_OP_PARAM, 4, 0, 0, lo},
        {AIR_OP_ADD, 3, 3, 4, 0}, {AIR_OP_XINV, 5, 0, 0, g_saturated ? SAT_X : 12345u}, {AIR_OP_MUL, 5, 5, 3, 0}, {AIR_OP_X, 4, 0, 0, 0}, {AIR_OP_SUB, 4, 4, 1, 0},
        {AIR_OP_EMIT, 0, 2, 0, 0}, {AIR_OP_EMIT, 0, 5, 1, ncons - 1}, {AIR_OP_EMIT, 0, 4, 0, ncons / 2}, {AIR_OP_EMIT, 0, 3, 1, 0}};
    std::vector<Insn> consts = prog;
    for (Insn& in : consts)
        if (in.op == AIR_OP_PARAM) { in.op = AIR_OP_CONST; in.imm = r.params_reduced[in.imm]; }
    const std::vector<AirInsn> dev_p = device_form(prog), dev_c = device_form(consts);
    std::unique_ptr<uint32_t[]> mat(new uint32_t[2 * N]);
    for (uint64_t i = 0; i < 2 * N; ++i) mat[i] = data_word();
    AirArgs a{};
    a.mat[0] = mat.get();
    a.col_stride[0] = N;
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.ninsns = (uint32_t)prog.size();
    a.nregs = 6;
    a.log_N = (uint32_t)log_N;
    a.log_blowup = (uint32_t)log_blowup;
    a.wNR = to_mont_host(bb_root_of_unity_host((uint32_t)log_N));
    a.shift_nR = to_mont_host(bb_pow_host(shift, n));
    a.wBR = to_mont_host(bb_pow_host(bb_root_of_unity_host((uint32_t)log_N), n));
    a.divides = 1;
    AirArgs ap = a, ac = a;
    ap.insns = dev_p.data();
    ac.insns = dev_c.data();
    if (log_N >= 2) eval_both<4>(ap, ac, r, nparams, 6, N);
    else eval_both<1>(ap, ac, r, nparams, 6, N);
    printf("EVAL %llu %d %u %u %u\n", (unsigned long long)N, log_blowup, nparams, nalphas, form);
}

// ---- 4. the record-fed scan bodies against the argument-fed ones ----
template <int OP>
static void terms_case(uint32_t nw, uint32_t ni, uint32_t dw, uint32_t di, uint64_t n) {
    TOYNI_CONTRACT_TAG("emu_dc terms op=%d num=%u/%u den=%u/%u n=%llu", OP, nw, ni, dw, di, (unsigned long long)n);
    constexpr int G = (int)EXT_ACCUM_GROUP;
    const uint64_t stride = n + 3;
    const auto column_words = [&](uint32_t width) { return width ? (size_t)(2 * width - 1) * stride + n : (size_t)1; };   // two columns
    std::unique_ptr<uint32_t[]> num(new uint32_t[column_words(nw)]), den(new uint32_t[column_words(dw)]);
    for (size_t k = 0; k < column_words(nw); ++k) num[k] = data_word();
    for (size_t k = 0; k < column_words(dw); ++k) den[k] = data_word();
    uint32_t gamma[4] = {0u, BB_P, BB_P, BB_P};
    const uint64_t hit = n > 3 ? 3 : n - 1;
    if (dw == 1) gamma[0] = (den[stride + hit] ? BB_P - den[stride + hit] : 0u) + BB_P;   // column 1, row `hit`: gamma + v = 0, every word >= p
    const ScanRecord r = scan_record(nw ? ni : EXT_SHIFT_NONE, dw ? di : EXT_SHIFT_NONE, dw == 1 ? 1u : 0u, di == 2 ? gamma : nullptr, false);
    ExtAccumArgs host{};
    host.num = ExtAccumOperand{nw ? num.get() : nullptr, stride, nw, {r.num_shift[0], r.num_shift[1], r.num_shift[2], r.num_shift[3]}};
    host.den = ExtAccumOperand{dw ? den.get() : nullptr, stride, dw, {r.den_shift[0], r.den_shift[1], r.den_shift[2], r.den_shift[3]}};
    host.den_inv = r.den_inv;
    host.n = n;
    ExtAccumArgs fed{};
    fed.num = ExtAccumOperand{nw ? num.get() : nullptr, stride, nw, {0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u}};   // what the twins' arguments leave unset
    fed.den = ExtAccumOperand{dw ? den.get() : nullptr, stride, dw, {0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u}};
    memset(&fed.den_inv, 0xA5, sizeof fed.den_inv);
    fed.n = n;
    std::unique_ptr<ExtAccumRecord> rec(new ExtAccumRecord(r.rec));
    ext_accum_args_from_record(fed, *rec);
    uint32_t zeros_seen = 0;
    for (uint32_t col = 0; col < 2; ++col)
        for (uint64_t i0 = 0; i0 < n; i0 += G) {
            Ext4 t[2][G];
            const uint32_t z0 = ext_accum_group_terms<OP, G>(fed, col, i0, n, t[0]);
            const uint32_t z1 = ext_accum_group_terms<OP, G>(host, col, i0, n, t[1]);
            if (z0 != z1 || memcmp(t[0], t[1], sizeof t[0])) { ++bad; printf("MISMATCH terms col=%u i0=%llu\n", col, (unsigned long long)i0); }
            zeros_seen += z0;
        }
    if (dw == 1 && di == 2 && !g_saturated && zeros_seen == 0) { ++bad; printf("MISMATCH the zero denominator was not met\n"); }
    printf("TERMS %d %u %u %u %u %llu %u\n", OP, nw, ni, dw, di, (unsigned long long)n, zeros_seen);
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode != "cases" && mode != "saturated") {
        fprintf(stderr, "usage: emu_dc cases | saturated\n");
        return 2;
    }
    g_saturated = mode == "saturated";
    // 1. the quotient's record: 0, 1, 4, 256 parameters; 1, 16, 17 and 70 alphas (more than a wave); both forms; one lane and a wave
    for (uint32_t nparams : {0u, 1u, 4u, 256u})
        for (uint32_t nalphas : {1u, 16u, 17u, 70u})
            for (uint32_t form : {AIR_WEIGHTS_EXT, AIR_WEIGHTS_EMIT_EXT})
                for (uint32_t nlanes : {1u, 64u}) quotient_record(nparams, nalphas, form, nlanes, nlanes == 64u);
    // 2. the scan's record
    for (uint32_t den_norm : {0u, 1u})
        for (uint32_t ni : {EXT_SHIFT_NONE, 0u, 2u})
            for (uint32_t di : {EXT_SHIFT_NONE, 0u, 1u}) scan_record(ni, di, den_norm, nullptr, true);
    {
        const uint32_t base[4] = {BB_P + 5u, BB_P, 0u, BB_P};                 // a gamma in the base field
        scan_record(2u, 2u, 1u, base, true);
    }
    // 3. PARAM against CONST
    for (int log_N : {0, 1, 2, 3, 6})
        for (uint32_t form : {AIR_WEIGHTS_EXT, AIR_WEIGHTS_EMIT_EXT}) param_case(log_N, log_N ? 1 : 0, log_N & 1 ? 256u : 4u, form == AIR_WEIGHTS_EXT ? 17u : 1u, form);
    // 4. the scan bodies: the operand forms 1/1, 1 (no shift)/1, 4/4, 0/1 with the zero denominator, 4/0
    struct Form { uint32_t nw, ni, dw, di; };
    for (const Form& f : {Form{1, 0, 1, 0}, Form{1, EXT_SHIFT_NONE, 1, 0}, Form{4, 1, 4, 0}, Form{0, EXT_SHIFT_NONE, 1, 2}, Form{4, 0, 0, EXT_SHIFT_NONE}})
        for (uint64_t n : {1ull, 5ull, 8ull, 13ull}) {
            terms_case<(int)SCAN_SUM>(f.nw, f.ni, f.dw, f.di, n);
            terms_case<(int)SCAN_PRODUCT>(f.nw, f.ni, f.dw, f.di, n);
        }
    printf("BAD %d\nDONE\n", bad);
    return bad ? 1 : 0;
}
