// Steps the bodies of the Ext DEEP combination and of the batched evaluation at Ext points (deep_combine_ext_group, poly_ext_*,
// toyni_amd/csrc/prover_kernels.hpp; include/toyni_hip.h 3h) on the CPU, with the host-side preparation of the two entry points
// restated here from the same helpers (table sorted by column, weights in Montgomery form, the claims folded into one Ext constant,
// adj_z / m_z from ext_shift_host, the tables of squarings from poly_ext_powers_host).  Prints inputs and outputs:
//     DEEPX <N> <log_blowup> <shift> <z0 z1 z2 z3> <width> <col_stride> <nterms> <word offset of the matrix>
//     TERM <column> <rotation> <alpha0..3> <value0..3>      (nterms lines, in the caller's order)
//     COL <c> <N values>                                    (width lines)
//     OUT <4 N values>
//     POLYX <ncoeffs> <stride> <batch> <npoints> <4 npoints point words>
//     COEF <b> <ncoeffs values>                             (batch lines)
//     POUT <batch x npoints x 4 values>
// tests/test_emu_deep_ext.py recomputes every word with tests/ext_model.py.  The matrices own exactly the words the layout owns (no
// slack after the last column), so an over-read is an AddressSanitizer error.
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

// `saturated` as the only argument runs, instead of the cases above, the ones whose every product is (p - 1)^2: every data word
// p - 1 and every weight, claim and point SAT_X, the plain value whose Montgomery form is p - 1 (same record format)

static uint64_t sm_state = 0xE47DEE9ull;
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

struct Term { uint32_t column, rotation, alpha[4], value[4]; };

// z_at >= 0: z is the coset's point of that index (a base-field z).  Otherwise `upper` of z's coordinates 1..3 are non-zero
// (upper = 0: a base-field z off the coset).
static void deep_case(int log_N, int log_blowup, uint32_t width, uint32_t nterms, uint32_t pad, uint32_t offset_words, long z_at, int upper, bool sat = false) {
    TOYNI_CONTRACT_TAG("deep_combine_ext_group log_N=%d width=%u nterms=%u sat=%d", log_N, width, nterms, (int)sat);
    NttPlan plan;
    if (!build_plan(log_N, plan)) { std::printf("FAIL plan\n"); return; }
    const uint64_t N = 1ull << log_N, rows = N >> log_blowup, col_stride = N + pad;
    const uint32_t shift = 7u;
    const uint32_t wN = bb_root_of_unity_host((uint32_t)log_N);
    uint32_t z[4] = {0u, 0u, 0u, 0u};
    if (z_at >= 0) {
        z[0] = bb_mul_host(shift, bb_pow_host(wN, (uint64_t)z_at));
    } else {
        z[0] = draw(splitmix());
        const int first = (int)(splitmix() % 3);                       // which upper coordinates: a run of `upper`, starting anywhere
        for (int u = 0; u < upper; ++u) z[1 + (first + u) % 3] = 1u + (uint32_t)(splitmix() % (BB_P - 1));
    }
    std::vector<Term> terms(nterms);
    for (uint32_t t = 0; t < nterms; ++t) {
        terms[t].column = (uint32_t)(splitmix() % width);
        terms[t].rotation = (t % 3 == 2) ? (uint32_t)(rows - 1) : (uint32_t)(splitmix() % rows);   // (i + rotation * B) passes N
        for (int k = 0; k < 4; ++k) {
            terms[t].alpha[k] = sat ? SAT_X : draw(t + nterms + 3u * k);
            terms[t].value[k] = sat ? SAT_X : draw(t + 2 * nterms + 1 + 2u * k);
        }
    }
    if (nterms >= 2) { terms[1].column = terms[0].column; terms[1].rotation = terms[0].rotation; }   // a repeated (column, rotation)
    const size_t words = (size_t)(width - 1) * col_stride + N;
    uint32_t* store = static_cast<uint32_t*>(::operator new((words + offset_words) * sizeof(uint32_t), std::align_val_t(16)));
    uint32_t* m = store + offset_words;
    for (size_t k = 0; k < words; ++k) m[k] = 0xFFFFFFF0u;   // the slack between N and col_stride: never read (>= p would show)
    for (uint32_t c = 0; c < width; ++c)
        for (uint64_t i = 0; i < N; ++i) m[c * col_stride + i] = sat ? BB_P - 1u : draw(splitmix());

    // what toyni_deep_combine_ext_device prepares
    std::vector<DeepExtTerm> table(nterms);
    DeepExtArgs a{};
    for (uint32_t t = 0; t < nterms; ++t) {
        table[t] = DeepExtTerm{};
        table[t].column = terms[t].column;
        table[t].rot = (uint32_t)((uint64_t)terms[t].rotation << log_blowup);
        uint32_t av[4];
        ext_mul_host(terms[t].alpha, terms[t].value, av);
        for (int k = 0; k < 4; ++k) {
            table[t].alphaR[k] = to_mont_host(terms[t].alpha[k]);
            a.claim[k] = (uint32_t)(((uint64_t)a.claim[k] + av[k]) % BB_P);
        }
    }
    std::stable_sort(table.begin(), table.end(), [](const DeepExtTerm& x, const DeepExtTerm& y) { return x.column != y.column ? x.column < y.column : x.rot < y.rot; });
    a.values = m;
    a.col_stride = col_stride;
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.log_N = (uint32_t)log_N;
    a.nterms = nterms;
    a.wNR = to_mont_host(wN);
    a.shift = ext_shift_host(z);
    std::vector<uint32_t> out(4 * N);
    if (log_N >= 2) {
        for (uint64_t i0 = 0; i0 < N; i0 += 4) {
            uint32_t d[4][4];
            deep_combine_ext_group<4>(a, table.data(), i0, d);
            for (int j = 0; j < 4; ++j)
                for (int k = 0; k < 4; ++k) out[4 * (i0 + j) + k] = d[j][k];
        }
    } else {
        for (uint64_t i = 0; i < N; ++i) {
            uint32_t d[1][4];
            deep_combine_ext_group<1>(a, table.data(), i, d);
            for (int k = 0; k < 4; ++k) out[4 * i + k] = d[0][k];
        }
    }
    std::printf("DEEPX %llu %d %u %u %u %u %u %u %llu %u %u\n", (unsigned long long)N, log_blowup, shift, z[0], z[1], z[2], z[3], width,
                (unsigned long long)col_stride, nterms, offset_words);
    for (const Term& t : terms)
        std::printf("TERM %u %u %u %u %u %u %u %u %u %u\n", t.column, t.rotation, t.alpha[0], t.alpha[1], t.alpha[2], t.alpha[3], t.value[0],
                    t.value[1], t.value[2], t.value[3]);
    for (uint32_t c = 0; c < width; ++c) {
        std::printf("COL %u", c);
        for (uint64_t i = 0; i < N; ++i) std::printf(" %u", m[c * col_stride + i]);
        std::printf("\n");
    }
    std::printf("OUT");
    for (uint32_t v : out) std::printf(" %u", v);
    std::printf("\n");
    ::operator delete(store, std::align_val_t(16));
}

static void poly_case(size_t ncoeffs, size_t stride, uint32_t batch, uint32_t npoints, bool sat = false) {
    TOYNI_CONTRACT_TAG("poly_ext ncoeffs=%zu batch=%u npoints=%u sat=%d", ncoeffs, batch, npoints, (int)sat);
    std::vector<uint32_t> coeffs(batch ? (size_t)(batch - 1) * stride + ncoeffs : 0);   // exactly the words the layout owns
    for (auto& c : coeffs) c = 0xFFFFFFF0u;
    for (uint32_t b = 0; b < batch; ++b)
        for (size_t i = 0; i < ncoeffs; ++i) coeffs[b * stride + i] = sat ? BB_P - 1u : draw(splitmix());
    uint32_t points[POLY_MAX_POINTS][4];
    PolyExtArgs a{};
    a.coeffs = coeffs.data();
    a.ncoeffs = ncoeffs;
    a.stride = stride;
    a.batch = batch;
    a.npoints = npoints;
    a.nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    for (uint32_t p = 0; p < npoints; ++p) {
        for (int k = 0; k < 4; ++k) points[p][k] = sat ? (p == 0 ? SAT_X : BB_P - 1u) : p == 0 ? BB_P - 1u : p == 1 ? (k == 0 ? 1u : 0u) : p == 2 ? draw(splitmix()) : (uint32_t)(splitmix() % BB_P);
        // what toyni_poly_eval_ext_batch_device prepares
        uint32_t z16[4], zchunk[4], zstride[4];
        ext_pow_host(points[p], POLY_PER_THREAD, z16);
        ext_pow_host(points[p], POLY_CHUNK, zchunk);
        ext_pow_host(zchunk, POLY_THREADS, zstride);
        a.thread[p] = poly_ext_powers_host(points[p], z16);
        a.chunk[p] = poly_ext_powers_host(zstride, zchunk);
    }
    std::vector<uint32_t> partial((size_t)batch * a.nblocks * npoints * 4), out((size_t)batch * npoints * 4);
    a.partial = partial.data();
    a.out = out.data();
    for (uint32_t col = 0; col < batch; ++col)                                   // stage 1: one block per (chunk, column)
        for (uint32_t chunk = 0; chunk < a.nblocks; ++chunk)
            for (uint32_t p = 0; p < npoints; ++p) {
                uint32_t sum[4] = {0u, 0u, 0u, 0u};
                for (uint32_t t = 0; t < POLY_THREADS; ++t) {
                    uint32_t c[POLY_PER_THREAD];
                    poly_ext_load(a, col, chunk, t, c);
                    const Ext4 v = poly_ext_thread_term(a, p, c, t);
                    for (int k = 0; k < 4; ++k) sum[k] = bb_add(sum[k], v.c[k]);
                }
                for (int k = 0; k < 4; ++k) partial[poly_ext_partial_index(a, col, chunk, p) + k] = sum[k];
            }
    for (uint32_t col = 0; col < batch; ++col)                                   // stage 2: one block per column
        for (uint32_t p = 0; p < npoints; ++p) {
            uint32_t sum[4] = {0u, 0u, 0u, 0u};
            for (uint32_t t = 0; t < POLY_THREADS; ++t) {
                const Ext4 v = poly_ext_final_thread(a, col, p, t);
                for (int k = 0; k < 4; ++k) sum[k] = bb_add(sum[k], v.c[k]);
            }
            for (int k = 0; k < 4; ++k) out[((size_t)col * npoints + p) * 4 + k] = sum[k];
        }
    std::printf("POLYX %zu %zu %u %u", ncoeffs, stride, batch, npoints);
    for (uint32_t p = 0; p < npoints; ++p)
        for (int k = 0; k < 4; ++k) std::printf(" %u", points[p][k]);
    std::printf("\n");
    for (uint32_t b = 0; b < batch; ++b) {
        std::printf("COEF %u", b);
        for (size_t i = 0; i < ncoeffs; ++i) std::printf(" %u", coeffs[b * stride + i]);
        std::printf("\n");
    }
    std::printf("POUT");
    for (uint32_t v : out) std::printf(" %u", v);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "saturated") {
        for (uint32_t nterms : {4u, 5u, 8u, 64u, 65u})
            for (int log_blowup : {0, 2}) deep_case(6, log_blowup, 8, nterms, 0, 0, -1, 3, true);
        for (size_t nc : {(size_t)17, (size_t)4097}) poly_case(nc, nc + 3, 3, 2, true);
        std::printf("DONE\n");
        return 0;
    }
    const int log_Ns[] = {0, 1, 2, 3, 6, 10};
    uint32_t k = 0;
    for (int log_N : log_Ns)
        for (uint32_t width = 1; width <= 9; ++width)
            for (uint32_t nterms = 1; nterms <= 12; ++nterms, ++k) {
                if (log_N == 10 && (width + nterms) % 4) continue;            // a quarter of the largest size is plenty
                const int log_blowup = log_N ? (int)(k % (uint32_t)(log_N + 1)) : 0;
                const uint32_t pad = (k % 3) ? 0u : 5u;                       // col_stride N or N + 5 (the latter misaligns odd columns)
                const uint32_t off = (k % 5 == 4) ? 1u : 0u;                  // every fifth matrix starts 4 bytes off 16-byte alignment
                const long N = 1l << log_N;
                // every sixth case puts a base-field z on the coset: at the first point of the last group, or the last point of the first
                const long z_at = k % 6 == 1 ? (N >= 4 ? 4 * ((N / 4) - 1) : 0) : k % 6 == 4 ? (N >= 4 ? 3 : N - 1) : -1;
                deep_case(log_N, log_blowup, width, nterms, pad, off, z_at, (int)((k / 2) % 4));
            }
    const size_t ncs[] = {1, 15, 16, 17, 4095, 4096, 4097};
    for (size_t nc : ncs)
        for (uint32_t batch : {1u, 2u, 3u})
            poly_case(nc, nc + (batch > 1 ? 3 : 0), batch, 1 + (uint32_t)((nc + batch) % 4));
    poly_case(40, 40, 2, 4);
    // more than POLY_THREADS chunks: the second stage's Horner in (z^POLY_CHUNK)^256 takes more than one step
    poly_case((size_t)POLY_CHUNK * (POLY_THREADS + 2) + 5, (size_t)POLY_CHUNK * (POLY_THREADS + 2) + 5, 1, 2);
    std::printf("DONE\n");
    return 0;
}
