// Steps the per-thread text of the four-to-one Ext FRI round under coset leaves (include/toyni_hip.h 3m) on the CPU:
//   fold4_ext_commit_leaf   (prover_kernels.hpp)  what fri_fold4_ext_commit_kernel runs per leaf of the folded layer
//   fri4_round_record       (prover_kernels.hpp)  the two factor tables fri4_transcript_round_kernel leaves for the next fold
//   merkle_row_leaf_at<ROWS_EXT_QUARTERS>, coset_value_word  (merkle_kernels.hpp)  the coset leaf and the opening's gather
// The sweep around them (fold4_ext_commit_sweep, device-only text in toyni_hip.hip) is NOT stepped: this program RESTATES its index
// arithmetic on the host -- leaf t of m / 16 reads elements t + k m/16, k < 16, and writes elements t + q m/16, q < 4, the point
// inverses from a host table -- so the kernel's own indexing is held by the GPU tests alone.
// The factors a fold is given are the ones fri4_round_record computed from the plain beta, so a wrong record is a wrong fold.
// Per case (m in {16, 64, 256} x salted x {random, field-edge, all p - 1}) one block of lines:
//     CASE <m> <salted> <x0> <beta0..3>
//     REC <16 words>                     beta/2, 11 beta/2, beta^2/2, 11 beta^2/2 in Montgomery form
//     IN <4 m words>   SALTS_IN <hex, 16 m/4 bytes or ->   SALTS_OUT <hex, 16 m/16 bytes or ->
//     OUT <m words>                      the folded layer, m / 4 elements
//     TREE_OUT <hex>                     every level of the folded layer's coset tree (leaves from the fold body, nodes by merkle_node)
//     TREE_IN <hex>                      every level of the INPUT layer's coset tree (merkle_row_leaf_at as the commit kernel runs it)
//     GATHER <4 m words>                 value words c < 16 of every coset leaf of the input layer, as the open kernel gathers them
// tests/test_emu_fold4_ext_commit.py judges the folds with the oracle's fri_fold_ext applied twice, leaves and trees with hashlib.
// `saturated` as the only argument runs the cases whose every product is (p - 1)^2 instead: every data word p - 1, x0^-1 and every
// coordinate of beta the plain value whose Montgomery form is p - 1 (same format).
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "prover_kernels.hpp"
#include "contract_case.hpp"

using namespace toyni;

static const uint32_t P = BB_P;
static uint64_t sm_state = 0x13198A2E03707344ull;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t rnd() { return (uint32_t)(splitmix() % P); }
static void hex(const uint8_t* b, size_t n) {
    if (n == 0) std::printf("-");
    for (size_t i = 0; i < n; ++i) std::printf("%02x", b[i]);
}
static void hex_digests(const std::vector<Digest>& d) {
    for (const Digest& x : d)
        for (int j = 0; j < 8; ++j)
            for (int b = 0; b < 4; ++b) std::printf("%02x", (unsigned)((x.m[j] >> (8 * b)) & 0xFFu));
}
static void salt_words(const std::vector<uint8_t>& salts, size_t i, uint32_t (&sw)[4]) {
    for (int j = 0; j < 4; ++j) {
        const uint8_t* s = salts.data() + 16 * i + 4 * j;
        sw[j] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
    }
}
// every level above the leaves already in `tree` (src/merkle.rs:25-48: an odd level pairs its last node with itself)
static void build_upper(std::vector<Digest>& tree, size_t n) {
    size_t off = 0;
    while (n > 1) {
        const size_t up = (n + 1) / 2;
        for (size_t i = 0; i < up; ++i) tree.push_back(merkle_node(tree[off + 2 * i], tree[off + (2 * i + 1 < n ? 2 * i + 1 : 2 * i)]));
        off += n;
        n = up;
    }
}

enum Fill { RANDOM, EDGE, TOP };

template <bool SALTED>
static void run(size_t m, Fill fill, const uint32_t (&beta)[4], uint32_t x0) {
    TOYNI_CONTRACT_TAG("fold4_ext_commit_leaf m=%zu salted=%d x0=%u beta0=%u", m, (int)SALTED, x0, beta[0]);
    const size_t nl = m / 16, quarter = m / 4;
    // the layer in an allocation of exactly 4 m words, the salts likewise: AddressSanitizer sees any index past them
    std::vector<uint32_t> layer(4 * m), out(m);
    const uint32_t edge[4] = {0u, 1u, P - 1u, P - 2u};
    for (size_t i = 0; i < 4 * m; ++i) layer[i] = fill == TOP ? P - 1u : fill == EDGE ? edge[splitmix() % 4] : rnd();
    std::vector<uint8_t> salts_in(SALTED ? 16 * quarter : 0), salts_out(SALTED ? 16 * nl : 0);
    for (auto& s : salts_in) s = (uint8_t)splitmix();
    for (auto& s : salts_out) s = (uint8_t)splitmix();
    // the record, from the plain beta and the host constants the phase passes
    const uint32_t half_r2 = to_mont_host(to_mont_host(BB_HALF)), half11_r2 = to_mont_host(to_mont_host(bb_mul_host(BB_HALF, 11u)));
    const uint32_t eleven_r2 = to_mont_host(to_mont_host(11u));
    ExtFactor rec[2];
    fri4_round_record(beta, half_r2, half11_r2, eleven_r2, rec);
    // the points: s_j = 1 / (x0 w_m^j) in Montgomery form (the kernel reads w_m^-j from the context's table), 1 / w_4
    uint32_t log_m = 0;
    while (((size_t)1 << log_m) < m) ++log_m;
    const uint32_t winv = bb_inv_host(bb_root_of_unity_host(log_m)), x0inv = bb_inv_host(x0);
    const uint32_t iinvR = to_mont_host(bb_inv_host(bb_root_of_unity_host(2)));
    std::vector<uint32_t> sR_all(quarter);
    uint32_t wj = 1u;
    for (size_t j = 0; j < quarter; ++j) {
        sR_all[j] = to_mont_host(bb_mul_host(x0inv, wj));
        wj = bb_mul_host(wj, winv);
    }
    std::vector<Digest> tree_out(nl);
    for (size_t t = 0; t < nl; ++t) {
        Ext4 in[16];
        for (size_t k = 0; k < 16; ++k) {
            const uint32_t* p = layer.data() + 4 * (t + k * nl);
            in[k] = Ext4{{p[0], p[1], p[2], p[3]}};
        }
        uint32_t sR[4];
        for (size_t q = 0; q < 4; ++q) sR[q] = sR_all[t + q * nl];
        uint32_t sw[4] = {0u, 0u, 0u, 0u};
        if (SALTED) salt_words(salts_out, t, sw);
        const Fold4ExtLeaf r = fold4_ext_commit_leaf<SALTED>(in, sR, iinvR, rec[0], rec[1], SALTED ? sw : nullptr);
        for (size_t q = 0; q < 4; ++q)
            for (int k = 0; k < 4; ++k) out[4 * (t + q * nl) + k] = r.folded[q].c[k];
        tree_out[t] = r.leaf;
    }
    build_upper(tree_out, nl);
    std::vector<Digest> tree_in(quarter);
    std::vector<uint32_t> gather(4 * m);
    for (size_t i = 0; i < quarter; ++i) {
        uint32_t sw[4] = {0u, 0u, 0u, 0u};
        if (SALTED) salt_words(salts_in, i, sw);
        tree_in[i] = merkle_row_leaf_at<ROWS_EXT_QUARTERS, SALTED>(layer.data(), i, 16u, quarter, true, SALTED ? sw : nullptr);
        for (uint32_t c = 0; c < 16; ++c) gather[16 * i + c] = coset_value_word(layer.data(), quarter, i, c);
    }
    build_upper(tree_in, quarter);
    std::printf("CASE %zu %d %u %u %u %u %u\nREC", m, SALTED ? 1 : 0, x0, beta[0], beta[1], beta[2], beta[3]);
    for (int f = 0; f < 2; ++f) {
        for (int k = 0; k < 4; ++k) std::printf(" %u", rec[f].b[k]);
        for (int k = 0; k < 4; ++k) std::printf(" %u", rec[f].b11[k]);
    }
    std::printf("\nIN");
    for (uint32_t v : layer) std::printf(" %u", v);
    std::printf("\nSALTS_IN ");
    hex(salts_in.data(), salts_in.size());
    std::printf("\nSALTS_OUT ");
    hex(salts_out.data(), salts_out.size());
    std::printf("\nOUT");
    for (uint32_t v : out) std::printf(" %u", v);
    std::printf("\nTREE_OUT ");
    hex_digests(tree_out);
    std::printf("\nTREE_IN ");
    hex_digests(tree_in);
    std::printf("\nGATHER");
    for (uint32_t v : gather) std::printf(" %u", v);
    std::printf("\n");
}

int main(int argc, char** argv) {
    const size_t sizes[3] = {16, 64, 256};
    if (argc > 1 && std::string(argv[1]) == "saturated") {
        const uint32_t beta[4] = {SAT_X, SAT_X, SAT_X, SAT_X};
        for (size_t m : sizes)
            for (uint32_t x0 : {bb_inv_host(SAT_X), P - 1u}) {
                run<true>(m, TOP, beta, x0);
                run<false>(m, TOP, beta, x0);
            }
        std::printf("DONE\n");
        return 0;
    }
    for (size_t m : sizes) {
        const uint32_t random_beta[4] = {rnd(), rnd(), rnd(), rnd()}, edge_beta[4] = {P - 1u, 0u, 1u, rnd()}, base_beta[4] = {rnd(), 0u, 0u, 0u};
        const uint32_t zero_beta[4] = {0u, 0u, 0u, 0u};
        const uint32_t x_random = 1u + (uint32_t)(splitmix() % (P - 1));
        run<true>(m, RANDOM, random_beta, x_random);
        run<false>(m, RANDOM, random_beta, 7u);
        run<true>(m, EDGE, edge_beta, 1u);
        run<false>(m, EDGE, base_beta, x_random);
        run<true>(m, RANDOM, zero_beta, 7u);           // the beta of a transcript whose status is set
        run<true>(m, TOP, edge_beta, P - 1u);          // saturated data: every word p - 1, beta = (p - 1, 0, 1, r), x0 = p - 1
        run<false>(m, TOP, edge_beta, P - 1u);
    }
    std::printf("DONE\n");
    return 0;
}
