// Operand-domain checks for the lazy field arithmetic of toyni_amd/csrc/bb_field.hpp (test infrastructure; CPU only).
//
// A contract build of a tests/emu or tests/sim program passes `-include tests/emu/field_contracts.hpp`: this file then defines
// TOYNI_FIELD_CONTRACT before bb_field.hpp is read, and every primitive reports its operands here at its top.  Each domain is the one
// the primitive's comment states, evaluated exactly (sums in unsigned __int128, no approximation of a bound); the exact sum is the
// final judge, so a domain that the comments state too widely shows as a violation as well.  Per primitive the calls and the
// violations are counted and the first violation is kept with its operands and the caller tag; at exit one line per primitive goes to
// stderr (stdout stays what the plain build prints):
//     CONTRACT <primitive> calls=<n> violations=<n> [first: <operands> tag=<tag>]
// The caller tag is a thread_local string the drivers set per case with TOYNI_CONTRACT_TAG(fmt, ...); no stack walking.
//
// `--contract-selftest` as the first argument (read by a constructor that runs ahead of main; the programs' own arguments and their
// own --selftest are untouched) runs toy functions that break each contract exactly once instead of the program: see the end.
//
//   primitive          documented domain                                                  exact judge
//   bb_add, bb_sub     a < p, b < p
//   bb_sub_lazy        a < p, b < p                                                       a + (p - b) in (0, 2p)
//   bb_reduce_2p       x < 2p
//   bb_halve           x < p
//   mont_mul_lazy      bR < p (a any u32), or a < p and bR < 2p                           a bR + m p < 2^64, quotient < 2p
//   mont_mul           as mont_mul_lazy
//   mont_dot_sub       a, b, wR < p, wR != 0, nwR == p - wR                               a wR + b nwR + m p < 2^64, quotient < 2p
//   mont_dot2          a, bR, c, dR < p                                                   a bR + c dR + m p < 2^64, quotient < 2p
//   mont_reduce_wide   t < 4 p^2                                                          hi' 2^32 + lo + m p < 2^64, quotient < 2p
//   wide_acc           each factor < p, at most four products before mont_reduce_wide    (the open-coded sums of the DEEP term loops)
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace toyni_contracts {

typedef unsigned __int128 u128;
constexpr uint32_t P = 2013265921u;
constexpr uint64_t TWO_P = 2ull * P;
constexpr uint32_t NPINV = 2013265919u;   // -p^-1 mod 2^32
static_assert((uint32_t)(P * (0u - NPINV)) == 1u, "-p^-1");

enum Prim { BB_ADD, BB_SUB, BB_SUB_LAZY, BB_REDUCE_2P, BB_HALVE, MONT_MUL_LAZY, MONT_MUL, MONT_DOT_SUB, MONT_DOT2, MONT_REDUCE_WIDE, WIDE_ACC, NPRIM };
static const char* const NAMES[NPRIM] = {"bb_add", "bb_sub", "bb_sub_lazy", "bb_reduce_2p", "bb_halve", "mont_mul_lazy", "mont_mul",
                                         "mont_dot_sub", "mont_dot2", "mont_reduce_wide", "wide_acc"};

struct Record {
    uint64_t calls, violations;
    uint64_t operands[4];
    int noperands;
    char tag[96];
};
inline Record g_rec[NPRIM];
inline bool g_report = true;
inline thread_local char g_tag_text[96] = "(no tag)";
inline thread_local const char* g_tag = g_tag_text;

inline void violation(Prim p, int n, uint64_t o0, uint64_t o1 = 0, uint64_t o2 = 0, uint64_t o3 = 0) {
    Record& r = g_rec[p];
    if (r.violations++ == 0) {
        r.noperands = n;
        r.operands[0] = o0, r.operands[1] = o1, r.operands[2] = o2, r.operands[3] = o3;
        strncpy(r.tag, g_tag, sizeof r.tag - 1);
        r.tag[sizeof r.tag - 1] = 0;
    }
}
// the quotient of a Montgomery reduction of `t` with the sum exact: false where t + m p leaves 64 bits or the quotient leaves [0, 2p)
inline bool reduction_fits(u128 t) {
    const uint32_t m = (uint32_t)t * NPINV;
    const u128 u = t + (u128)m * P;
    return (u >> 64) == 0 && (uint64_t)(u >> 32) < TWO_P;
}

inline void check_BB_ADD(uint32_t a, uint32_t b) {
    ++g_rec[BB_ADD].calls;
    if (a >= P || b >= P) violation(BB_ADD, 2, a, b);
}
inline void check_BB_SUB(uint32_t a, uint32_t b) {
    ++g_rec[BB_SUB].calls;
    if (a >= P || b >= P) violation(BB_SUB, 2, a, b);
}
inline void check_BB_SUB_LAZY(uint32_t a, uint32_t b) {
    ++g_rec[BB_SUB_LAZY].calls;
    const u128 r = (u128)a + P - b;   // b <= p holds wherever this is not already a violation
    if (a >= P || b >= P || r == 0 || r >= TWO_P) violation(BB_SUB_LAZY, 2, a, b);
}
inline void check_BB_REDUCE_2P(uint32_t x) {
    ++g_rec[BB_REDUCE_2P].calls;
    if (x >= TWO_P) violation(BB_REDUCE_2P, 1, x);
}
inline void check_BB_HALVE(uint32_t x) {
    ++g_rec[BB_HALVE].calls;
    if (x >= P) violation(BB_HALVE, 1, x);
}
inline void mul_domain(Prim p, uint32_t a, uint32_t bR) {
    ++g_rec[p].calls;
    const bool documented = bR < P || (a < P && bR < TWO_P);
    if (!documented || !reduction_fits((u128)a * bR)) violation(p, 2, a, bR);
}
inline void check_MONT_MUL_LAZY(uint32_t a, uint32_t bR) { mul_domain(MONT_MUL_LAZY, a, bR); }
inline void check_MONT_MUL(uint32_t a, uint32_t bR) { mul_domain(MONT_MUL, a, bR); }
inline void check_MONT_DOT_SUB(uint32_t a, uint32_t b, uint32_t wR, uint32_t nwR) {
    ++g_rec[MONT_DOT_SUB].calls;
    const bool documented = a < P && b < P && wR < P && wR != 0u && nwR == P - wR;
    if (!documented || !reduction_fits((u128)a * wR + (u128)b * nwR)) violation(MONT_DOT_SUB, 4, a, b, wR, nwR);
}
inline void check_MONT_DOT2(uint32_t a, uint32_t bR, uint32_t c, uint32_t dR) {
    ++g_rec[MONT_DOT2].calls;
    const bool documented = a < P && bR < P && c < P && dR < P;
    if (!documented || !reduction_fits((u128)a * bR + (u128)c * dR)) violation(MONT_DOT2, 4, a, bR, c, dR);
}
inline void check_MONT_REDUCE_WIDE(uint64_t t) {
    ++g_rec[MONT_REDUCE_WIDE].calls;
    bool ok = (u128)t < (u128)4 * P * P;
    if (ok) {   // the function's own two steps: the high word drops one p, then one reduction
        const uint32_t lo = (uint32_t)t;
        const uint64_t hi = t >> 32;
        ok = hi < TWO_P && reduction_fits(((u128)(hi >= P ? hi - P : hi) << 32) | lo);
    }
    if (!ok) violation(MONT_REDUCE_WIDE, 1, t);
}
// one product `v * alphaR` joining a 64-bit sum that mont_reduce_wide will reduce; `count` products are in the sum with this one
inline void check_WIDE_ACC(uint32_t v, uint32_t alphaR, uint32_t count) {
    ++g_rec[WIDE_ACC].calls;
    if (v >= P || alphaR >= P || count < 1u || count > 4u) violation(WIDE_ACC, 3, v, alphaR, count);
}

inline void reset() {
    for (Record& r : g_rec) r = Record{};
}
inline void print_lines(FILE* f) {
    for (int p = 0; p < NPRIM; ++p) {
        const Record& r = g_rec[p];
        fprintf(f, "CONTRACT %s calls=%llu violations=%llu", NAMES[p], (unsigned long long)r.calls, (unsigned long long)r.violations);
        if (r.violations) {
            fprintf(f, " first:");
            for (int i = 0; i < r.noperands; ++i) fprintf(f, " %llu", (unsigned long long)r.operands[i]);
            fprintf(f, " tag=%s", r.tag);
        }
        fprintf(f, "\n");
    }
}
struct AtExit {
    ~AtExit() {
        if (g_report) {
            fflush(stdout);
            print_lines(stderr);
        }
    }
};
inline AtExit g_at_exit;

}  // namespace toyni_contracts

#define TOYNI_FIELD_CONTRACT(prim, ...) ::toyni_contracts::check_##prim(__VA_ARGS__)
#define TOYNI_CONTRACT_TAG(...) (snprintf(::toyni_contracts::g_tag_text, sizeof ::toyni_contracts::g_tag_text, __VA_ARGS__), \
                                 ::toyni_contracts::g_tag = ::toyni_contracts::g_tag_text, (void)0)

// ---- the self-test: every contract broken exactly once by a toy, each reported under its own primitive and tag ----
#include "bb_field.hpp"

namespace toyni_contracts {

// what a toy may be flagged for: a bit per primitive
inline unsigned flagged() {
    unsigned mask = 0;
    for (int p = 0; p < NPRIM; ++p) mask |= g_rec[p].violations ? 1u << p : 0u;
    return mask;
}
inline uint64_t total_violations() {
    uint64_t n = 0;
    for (const Record& r : g_rec) n += r.violations;
    return n;
}
// a toy: `body` under tag `name`; exactly `want` (a mask, 0 = nothing) must be flagged, once where `once`, and under this tag
template <class F>
inline bool toy(const char* name, unsigned want, bool once, F body) {
    reset();
    TOYNI_CONTRACT_TAG("selftest %s", name);
    body();
    const unsigned got = flagged();
    bool ok = got == want && (!once || total_violations() == 1);
    char names[256] = "";
    for (int p = 0; p < NPRIM; ++p)
        if (got >> p & 1u) {
            strcat(names, names[0] ? "," : ""), strcat(names, NAMES[p]);
            ok = ok && !strcmp(g_rec[p].tag, g_tag_text);
        }
    printf("TOY %s flagged=%s violations=%llu %s\n", name, names[0] ? names : "none", (unsigned long long)total_violations(), ok ? "ok" : "WRONG");
    return ok;
}

// an 8-point forward transform (decimation in frequency, natural order in, bit-reversed out) on the primitives, and the same by
// definition in plain integers
inline void toy_transform(const uint32_t (&in)[8], uint32_t (&out)[8]) {
    using namespace toyni;
    const uint32_t w8 = bb_root_of_unity_host(3);
    uint32_t v[8];
    for (int i = 0; i < 8; ++i) v[i] = in[i];
    for (int half = 4; half >= 1; half >>= 1)
        for (int base = 0; base < 8; base += 2 * half)
            for (int j = 0; j < half; ++j) {
                const uint32_t wR = to_mont_host(bb_pow_host(w8, (uint64_t)j * (4 / half)));
                const uint32_t a = v[base + j], b = v[base + j + half];
                v[base + j] = bb_add(a, b);
                v[base + j + half] = mont_mul(bb_sub(a, b), wR);
            }
    for (int i = 0; i < 8; ++i) out[bitrev32((uint32_t)i, 3)] = v[i];
}
inline void toy_transform_integers(const uint32_t (&in)[8], uint32_t (&out)[8]) {
    using namespace toyni;
    const uint32_t w8 = bb_root_of_unity_host(3);
    for (int k = 0; k < 8; ++k) {
        uint64_t s = 0;
        for (int i = 0; i < 8; ++i) s = (s + (uint64_t)bb_mul_host(in[i] % BB_P, bb_pow_host(w8, (uint64_t)i * k))) % BB_P;
        out[k] = (uint32_t)s;
    }
}
// a 4-output fold r_i = (a_i + b_i) / 2 + (a_i - b_i) c_i on the primitives, and in plain integers
inline void toy_fold(const uint32_t (&a)[4], const uint32_t (&b)[4], const uint32_t (&c)[4], uint32_t (&r)[4]) {
    using namespace toyni;
    for (int i = 0; i < 4; ++i) r[i] = bb_add(bb_halve(bb_add(a[i], b[i])), mont_mul(bb_sub(a[i], b[i]), to_mont_host(c[i])));
}
inline void toy_fold_integers(const uint32_t (&a)[4], const uint32_t (&b)[4], const uint32_t (&c)[4], uint32_t (&r)[4]) {
    using namespace toyni;
    for (int i = 0; i < 4; ++i) {
        const uint64_t x = a[i] % BB_P, y = b[i] % BB_P;
        r[i] = (uint32_t)(((x + y) * BB_HALF + (x + BB_P - y) % BB_P * c[i]) % BB_P);
    }
}

inline int selftest() {
    using namespace toyni;
    const unsigned none = 0;
    const auto bit = [](Prim p) { return 1u << p; };
    volatile uint32_t sink = 0;
    bool ok = true;
    // a lazy result at or above p reaches bb_add (about every second quotient of two large factors is one)
    ok &= toy("lazy_result_into_bb_add", bit(BB_ADD), true, [&] {
        uint32_t lazy = 0;
        for (uint32_t a = BB_P - 1u; a > BB_P - 1000u && lazy < BB_P; --a) lazy = mont_mul_lazy(a, BB_P - 1u);
        if (lazy < BB_P) { printf("TOY no lazy quotient at or above p was found\n"); return; }
        sink = bb_add(lazy, 1u);
    });
    ok &= toy("reduce_2p_of_2p", bit(BB_REDUCE_2P), true, [&] { sink = bb_reduce_2p(2u * BB_P); });
    ok &= toy("any_u32_times_lazy", bit(MONT_MUL_LAZY), true, [&] { sink = mont_mul_lazy(0xFFFFFFFFu, 2u * BB_P - 1u); });
    ok &= toy("any_u32_times_lazy_through_mont_mul", bit(MONT_MUL) | bit(MONT_MUL_LAZY), false, [&] { sink = mont_mul(0xFFFFFFFFu, 2u * BB_P - 1u); });
    ok &= toy("dot_sub_zero_twiddle", bit(MONT_DOT_SUB), true, [&] { sink = mont_dot_sub(5u, 7u, 0u, BB_P); });
    ok &= toy("dot_sub_wrong_negation", bit(MONT_DOT_SUB), true, [&] { sink = mont_dot_sub(5u, 7u, 9u, BB_P - 9u + 1u); });
    ok &= toy("dot2_lazy_factor", bit(MONT_DOT2), true, [&] { sink = mont_dot2(5u, BB_P, 7u, 9u); });
    // 5 (p - 1)^2 passes 2^64: mont_reduce_wide is handed the wrapped sum, which lies below 4 p^2 -- only the count can tell
    ok &= toy("five_saturated_products", bit(WIDE_ACC), true, [&] {
        uint64_t acc = 0;
        for (uint32_t q = 0; q < 5; ++q) {
            TOYNI_FIELD_CONTRACT(WIDE_ACC, BB_P - 1u, BB_P - 1u, q + 1u);
            acc += (uint64_t)(BB_P - 1u) * (BB_P - 1u);
        }
        sink = mont_reduce_wide(acc);
    });
    ok &= toy("wide_acc_lazy_factor", bit(WIDE_ACC), true, [&] { TOYNI_FIELD_CONTRACT(WIDE_ACC, BB_P, 3u, 1u); });
    ok &= toy("halve_of_p", bit(BB_HALVE), true, [&] { sink = bb_halve(BB_P); });
    ok &= toy("sub_lazy_of_lazy", bit(BB_SUB_LAZY), true, [&] { sink = bb_sub_lazy(BB_P + 1u, 1u); });
    // well-formed toys: saturated operands at every bound the comments claim, and nothing may be reported
    ok &= toy("well_formed_saturated", none, false, [&] {
        const uint32_t m = BB_P - 1u;
        sink = bb_add(m, m), sink = bb_sub(0u, m), sink = bb_sub_lazy(0u, m), sink = bb_sub_lazy(m, 0u), sink = bb_halve(m);
        sink = bb_reduce_2p(2u * BB_P - 1u), sink = mont_mul_lazy(0xFFFFFFFFu, m), sink = mont_mul(m, 2u * BB_P - 1u);
        sink = mont_dot_sub(m, m, 1u, m), sink = mont_dot_sub(m, m, m, 1u), sink = mont_dot2(m, m, m, m);
        uint64_t acc = 0;
        for (uint32_t q = 0; q < 4; ++q) {
            TOYNI_FIELD_CONTRACT(WIDE_ACC, m, m, q + 1u);
            acc += (uint64_t)m * m;
        }
        sink = mont_reduce_wide(acc);
        sink = mont_inv_chain(m), sink = to_mont(m), sink = from_mont(m);
    });
    // what the gap was: the value p (congruent to 0, not canonical) in place of a 0
    const uint32_t good[8] = {0u, 1u, BB_P - 1u, 0u, 12345u, 0u, 7u, 1069547521u};
    uint32_t bad[8], got[8], want[8];
    for (int i = 0; i < 8; ++i) bad[i] = good[i] ? good[i] : BB_P;
    ok &= toy("transform_well_formed", none, false, [&] { toy_transform(good, got); });
    toy_transform_integers(good, want);
    const bool transform_ok = !memcmp(got, want, sizeof got);
    ok &= transform_ok;
    printf("TOY transform_well_formed outputs %s the integer transform\n", transform_ok ? "equal" : "DIFFER FROM");
    reset();
    TOYNI_CONTRACT_TAG("selftest transform_with_p_for_0");
    toy_transform(bad, got);
    const unsigned tf = flagged();
    printf("TOY transform_with_p_for_0 flagged=%s%s%s outputs %s the integer transform (printed, not judged)\n", tf & bit(BB_ADD) ? "bb_add" : "",
           (tf & bit(BB_ADD)) && (tf & bit(BB_SUB)) ? "," : "", tf & bit(BB_SUB) ? "bb_sub" : "", !memcmp(got, want, sizeof got) ? "equal" : "differ from");
    ok &= (tf & (bit(BB_ADD) | bit(BB_SUB))) != 0 && !strcmp(g_rec[tf & bit(BB_ADD) ? BB_ADD : BB_SUB].tag, "selftest transform_with_p_for_0");
    const uint32_t fa[4] = {0u, 5u, BB_P - 1u, 0u}, fb[4] = {3u, 0u, 0u, BB_P - 1u}, fc[4] = {1069547521u, 2u, BB_P - 1u, 77u};
    uint32_t ba[4], bbv[4], fgot[4], fwant[4];
    for (int i = 0; i < 4; ++i) ba[i] = fa[i] ? fa[i] : BB_P, bbv[i] = fb[i] ? fb[i] : BB_P;
    ok &= toy("fold_well_formed", none, false, [&] { toy_fold(fa, fb, fc, fgot); });
    toy_fold_integers(fa, fb, fc, fwant);
    const bool fold_ok = !memcmp(fgot, fwant, sizeof fgot);
    ok &= fold_ok;
    printf("TOY fold_well_formed outputs %s the integer fold\n", fold_ok ? "equal" : "DIFFER FROM");
    reset();
    TOYNI_CONTRACT_TAG("selftest fold_with_p_for_0");
    toy_fold(ba, bbv, fc, fgot);
    const unsigned ff = flagged();
    printf("TOY fold_with_p_for_0 flagged=%s%s%s outputs %s the integer fold (printed, not judged)\n", ff & bit(BB_ADD) ? "bb_add" : "",
           (ff & bit(BB_ADD)) && (ff & bit(BB_SUB)) ? "," : "", ff & bit(BB_SUB) ? "bb_sub" : "", !memcmp(fgot, fwant, sizeof fgot) ? "equal" : "differ from");
    ok &= (ff & (bit(BB_ADD) | bit(BB_SUB))) != 0 && !strcmp(g_rec[ff & bit(BB_ADD) ? BB_ADD : BB_SUB].tag, "selftest fold_with_p_for_0");
    (void)sink;
    printf(ok ? "CONTRACT SELFTEST OK\n" : "CONTRACT SELFTEST FAILED\n");
    return ok ? 0 : 1;
}

// runs ahead of main (glibc hands a constructor the program's arguments): the self-test replaces the program's run
__attribute__((constructor)) static void boot(int argc, char** argv, char**) {
    if (argc > 1 && !strcmp(argv[1], "--contract-selftest")) {
        const int rc = selftest();
        g_report = false;
        fflush(stdout);
        _Exit(rc);
    }
}

}  // namespace toyni_contracts
