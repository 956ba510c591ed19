// Steps the per-element body of the Ext fold-and-commit round (fold_ext_commit_one, toyni_amd/csrc/prover_kernels.hpp; the text
// fri_fold_ext_commit_kernel runs per thread) on the CPU.  One line per case:
//     <salted> <a0..a3> <b0..b3> <x> <beta0..beta3> <salt as hex, 32 digits> <folded0..3> <digest as hex>
// tests/test_emu_fold_ext_commit.py recomputes the fold with the oracle and sha256(00 || [salt] || Ext::to_bytes) with hashlib.
// Cases: every coordinate of a, b and beta walks through {0, 1, p - 1} against random others; beta embedded from the base field;
// x in {1, p - 1, 7, random}; all-zero, all-one and all-(p - 1) elements; then random ones.  The unsalted form is handed a NULL salt:
// it must not read one.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "prover_kernels.hpp"
#include "contract_case.hpp"

using namespace toyni;

// `saturated` as the only argument runs, instead of the cases above, the ones whose every product is (p - 1)^2: every data word
// p - 1 and every challenge coordinate SAT_X, the plain value whose Montgomery form is p - 1 (same record format)

static const uint32_t P = BB_P;
static uint64_t sm_state = 0x243F6A8885A308D3ull;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t rnd() { return (uint32_t)(splitmix() % P); }
static Ext4 rnd_ext() { return Ext4{{rnd(), rnd(), rnd(), rnd()}}; }
static void hex(const uint8_t* b, size_t n) {
    for (size_t i = 0; i < n; ++i) std::printf("%02x", b[i]);
}

struct Case { Ext4 a, b; uint32_t x; uint32_t beta[4]; };

template <bool SALTED>
static void run(const Case& c) {
    TOYNI_CONTRACT_TAG("fold_ext_commit_one salted=%d x=%u beta0=%u", (int)SALTED, c.x, c.beta[0]);
    uint8_t salt[16];
    for (auto& s : salt) s = SALTED ? (uint8_t)splitmix() : 0;
    uint32_t sw[4];
    for (int j = 0; j < 4; ++j)
        sw[j] = (uint32_t)salt[4 * j] | ((uint32_t)salt[4 * j + 1] << 8) | ((uint32_t)salt[4 * j + 2] << 16) | ((uint32_t)salt[4 * j + 3] << 24);
    uint32_t bh[4];
    for (int k = 0; k < 4; ++k) bh[k] = bb_mul_host(c.beta[k], BB_HALF);
    const ExtFactor f = ext_factor_host(bh);
    const uint32_t scaleR = to_mont_host(bb_inv_host(c.x));
    const FoldExtLeaf r = fold_ext_commit_one<SALTED>(c.a, c.b, scaleR, f, SALTED ? sw : nullptr);
    std::printf("%d", SALTED ? 1 : 0);
    for (int k = 0; k < 4; ++k) std::printf(" %u", c.a.c[k]);
    for (int k = 0; k < 4; ++k) std::printf(" %u", c.b.c[k]);
    std::printf(" %u", c.x);
    for (int k = 0; k < 4; ++k) std::printf(" %u", c.beta[k]);
    std::printf(" ");
    hex(salt, 16);
    for (int k = 0; k < 4; ++k) std::printf(" %u", r.folded.c[k]);
    std::printf(" ");
    uint8_t out[32];
    for (int j = 0; j < 8; ++j)
        for (int b = 0; b < 4; ++b) out[4 * j + b] = (uint8_t)(r.leaf.m[j] >> (8 * b));
    hex(out, 32);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "saturated") {   // a - b is saturated against b = 0 (and vanishes against b = a); x^-1 = SAT_X as well
        const Ext4 top{{P - 1u, P - 1u, P - 1u, P - 1u}}, zero{{0u, 0u, 0u, 0u}};
        for (uint32_t x : {bb_inv_host(SAT_X), SAT_X, P - 1u, 7u})
            for (int form = 0; form < 3; ++form) {
                const Case c{form == 2 ? zero : top, form == 1 ? zero : top, x, {SAT_X, SAT_X, SAT_X, SAT_X}};
                run<true>(c);
                run<false>(c);
            }
        std::printf("DONE\n");
        return 0;
    }
    const uint32_t edge[3] = {0u, 1u, P - 1u};
    const uint32_t xs[4] = {1u, P - 1u, 7u, 0u /* random */};
    std::vector<Case> cases;
    auto fresh = [&](size_t k) {
        Case c{rnd_ext(), rnd_ext(), xs[k % 4] ? xs[k % 4] : 1u + (uint32_t)(splitmix() % (P - 1)), {rnd(), rnd(), rnd(), rnd()}};
        return c;
    };
    // one coordinate at an edge value, of a, of b, of beta: 3 x 4 x 3 cases
    for (int which = 0; which < 3; ++which)
        for (int k = 0; k < 4; ++k)
            for (uint32_t e : edge) {
                Case c = fresh(cases.size());
                (which == 0 ? c.a.c[k] : which == 1 ? c.b.c[k] : c.beta[k]) = e;
                cases.push_back(c);
            }
    // whole elements at an edge value, against each other
    for (uint32_t ea : edge)
        for (uint32_t eb : edge)
            for (uint32_t ebeta : edge) {
                Case c = fresh(cases.size());
                c.a = Ext4{{ea, ea, ea, ea}};
                c.b = Ext4{{eb, eb, eb, eb}};
                for (int k = 0; k < 4; ++k) c.beta[k] = ebeta;
                cases.push_back(c);
            }
    // beta embedded from the base field: 0, 1, p - 1 and random
    for (uint32_t b0 : {0u, 1u, P - 1u, rnd(), rnd()}) {
        Case c = fresh(cases.size());
        c.beta[0] = b0; c.beta[1] = c.beta[2] = c.beta[3] = 0u;
        cases.push_back(c);
    }
    for (int k = 0; k < 24; ++k) cases.push_back(fresh(cases.size()));
    for (const Case& c : cases) {
        run<true>(c);
        run<false>(c);
    }
    std::printf("DONE\n");
    return 0;
}
