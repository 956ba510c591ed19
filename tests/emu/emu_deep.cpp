// Steps the bodies of the DEEP combination and of the batched polynomial evaluation (deep_combine_group, poly_batch_*,
// toyni_amd/csrc/prover_kernels.hpp) on the CPU, with the host-side preparation of toyni_deep_combine_device (term table sorted by
// column, weights in Montgomery form, the claimed values folded into one constant) restated here.  Prints inputs and outputs:
//     DEEP <N> <log_blowup> <shift> <z> <width> <col_stride> <nterms> <word offset of the matrix>
//     TERM <column> <rotation> <alpha> <value>          (nterms lines, in the caller's order)
//     COL <c> <N values>                                (width lines)
//     OUT <N values>
//     POLY <ncoeffs> <stride> <batch> <npoints> <points...>
//     COEF <b> <ncoeffs values>                         (batch lines)
//     POUT <batch x npoints values>
// tests/test_emu_deep.py recomputes every word with Python integers.  The matrices own exactly the words the layout owns (no slack
// after the last column), so an over-read is an AddressSanitizer error.
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

static uint64_t sm_state = 0xD1CEDEE9ull;
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

struct Term { uint32_t column, rotation, alpha, value; };

// z_at >= 0: z is the coset's point of that index
static void deep_case(int log_N, int log_blowup, uint32_t width, uint32_t nterms, uint32_t pad, uint32_t offset_words, long z_at, bool sat = false) {
    TOYNI_CONTRACT_TAG("deep_combine_group log_N=%d width=%u nterms=%u sat=%d", log_N, width, nterms, (int)sat);
    NttPlan plan;
    if (!build_plan(log_N, plan)) { std::printf("FAIL plan\n"); return; }
    const uint64_t N = 1ull << log_N, rows = N >> log_blowup, col_stride = N + pad;
    const uint32_t shift = 7u;
    const uint32_t wN = bb_root_of_unity_host((uint32_t)log_N);
    const uint32_t z = z_at >= 0 ? bb_mul_host(shift, bb_pow_host(wN, (uint64_t)z_at)) : (uint32_t)(splitmix() % BB_P);
    std::vector<Term> terms(nterms);
    for (uint32_t t = 0; t < nterms; ++t) {
        terms[t].column = (uint32_t)(splitmix() % width);
        // rotations up to rows - 1: (i + rotation * B) passes N for the later points
        terms[t].rotation = (t % 3 == 2) ? (uint32_t)(rows - 1) : (uint32_t)(splitmix() % rows);
        terms[t].alpha = sat ? SAT_X : draw(t + nterms);
        terms[t].value = sat ? SAT_X : draw(t + 2 * nterms + 1);
    }
    if (nterms >= 2) terms[1] = Term{terms[0].column, terms[0].rotation, terms[1].alpha, terms[1].value};   // a repeated (column, rotation)
    const size_t words = (size_t)(width - 1) * col_stride + N;
    uint32_t* store = static_cast<uint32_t*>(::operator new((words + offset_words) * sizeof(uint32_t), std::align_val_t(16)));
    uint32_t* m = store + offset_words;
    for (size_t k = 0; k < words; ++k) m[k] = 0xFFFFFFF0u;   // the slack between N and col_stride: never read (>= p would show)
    for (uint32_t c = 0; c < width; ++c)
        for (uint64_t i = 0; i < N; ++i) m[c * col_stride + i] = sat ? BB_P - 1u : draw(splitmix());

    // what toyni_deep_combine_device prepares
    std::vector<DeepTerm> table(nterms);
    uint32_t claim = 0;
    for (uint32_t t = 0; t < nterms; ++t) {
        table[t] = DeepTerm{terms[t].column, (uint32_t)((uint64_t)terms[t].rotation << log_blowup), to_mont_host(terms[t].alpha), 0u};
        claim = (uint32_t)((claim + (uint64_t)terms[t].alpha * terms[t].value) % BB_P);
    }
    std::stable_sort(table.begin(), table.end(), [](const DeepTerm& x, const DeepTerm& y) { return x.column != y.column ? x.column < y.column : x.rot < y.rot; });
    DeepCombineArgs a{};
    a.values = m;
    a.col_stride = col_stride;
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.log_N = (uint32_t)log_N;
    a.nterms = nterms;
    a.wNR = to_mont_host(wN);
    a.zR = to_mont_host(z);
    a.claim = claim;
    std::vector<uint32_t> out(N);
    if (log_N >= 3) {
        for (uint64_t i0 = 0; i0 < N; i0 += 8) {
            uint32_t d[8];
            deep_combine_group<8>(a, table.data(), i0, d);
            for (int j = 0; j < 8; ++j) out[i0 + j] = d[j];
        }
    } else {
        for (uint64_t i = 0; i < N; ++i) {
            uint32_t d[1];
            deep_combine_group<1>(a, table.data(), i, d);
            out[i] = d[0];
        }
    }
    std::printf("DEEP %llu %d %u %u %u %llu %u %u\n", (unsigned long long)N, log_blowup, shift, z, width, (unsigned long long)col_stride, nterms, offset_words);
    for (const Term& t : terms) std::printf("TERM %u %u %u %u\n", t.column, t.rotation, t.alpha, t.value);
    for (uint32_t c = 0; c < width; ++c) {
        std::printf("COL %u", c);
        for (uint64_t i = 0; i < N; ++i) std::printf(" %u", m[c * col_stride + i]);
        std::printf("\n");
    }
    std::printf("OUT");
    for (uint64_t i = 0; i < N; ++i) std::printf(" %u", out[i]);
    std::printf("\n");
    ::operator delete(store, std::align_val_t(16));
}

static void poly_case(size_t ncoeffs, size_t stride, uint32_t batch, uint32_t npoints, bool sat = false) {
    TOYNI_CONTRACT_TAG("poly_batch ncoeffs=%zu batch=%u npoints=%u sat=%d", ncoeffs, batch, npoints, (int)sat);
    std::vector<uint32_t> coeffs(batch ? (size_t)(batch - 1) * stride + ncoeffs : 0);   // exactly the words the layout owns
    for (auto& c : coeffs) c = 0xFFFFFFF0u;
    for (uint32_t b = 0; b < batch; ++b)
        for (size_t i = 0; i < ncoeffs; ++i) coeffs[b * stride + i] = sat ? BB_P - 1u : draw(splitmix());
    uint32_t points[POLY_MAX_POINTS];
    PolyBatchArgs a{};
    a.e.coeffs = coeffs.data();
    a.e.ncoeffs = ncoeffs;
    a.e.npoints = npoints;
    a.e.nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    a.stride = stride;
    a.batch = batch;
    for (uint32_t p = 0; p < npoints; ++p) {
        points[p] = sat ? (p == 0 ? SAT_X : BB_P - 1u) : p == 0 ? BB_P - 1u : p == 1 ? 1u : (uint32_t)(splitmix() % BB_P);
        a.e.zR[p] = to_mont_host(points[p]);
        a.e.z16R[p] = to_mont_host(bb_pow_host(points[p], POLY_PER_THREAD));
        a.e.zchunkR[p] = to_mont_host(bb_pow_host(points[p], POLY_CHUNK));
    }
    std::vector<uint32_t> partial((size_t)batch * a.e.nblocks * npoints), out((size_t)batch * npoints);
    a.e.partial = partial.data();
    a.e.out = out.data();
    for (uint32_t col = 0; col < batch; ++col)                                   // stage 1: one block per (chunk, column)
        for (uint32_t chunk = 0; chunk < a.e.nblocks; ++chunk)
            for (uint32_t p = 0; p < npoints; ++p) {
                uint32_t sum = 0;
                for (uint32_t t = 0; t < POLY_THREADS; ++t) {
                    uint32_t c[POLY_PER_THREAD];
                    poly_batch_load(a, col, chunk, t, c);
                    sum = bb_add(sum, poly_thread_term(a.e, p, c, t));
                }
                partial[poly_batch_partial_index(a, col, chunk, p)] = sum;
            }
    for (uint32_t col = 0; col < batch; ++col)                                   // stage 2: one block per column
        for (uint32_t p = 0; p < npoints; ++p) {
            uint32_t sum = 0;
            for (uint32_t t = 0; t < 256; ++t) sum = bb_add(sum, poly_batch_final_thread(a, col, p, t, 256));
            out[(size_t)col * npoints + p] = sum;
        }
    std::printf("POLY %zu %zu %u %u", ncoeffs, stride, batch, npoints);
    for (uint32_t p = 0; p < npoints; ++p) std::printf(" %u", points[p]);
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
            for (int log_blowup : {0, 2}) deep_case(6, log_blowup, 8, nterms, 0, 0, -1, true);
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
                const long z_at = k % 4 == 1 ? (N >= 8 ? 8 * ((N / 8) - 1) : 0)            // first point of the last group
                                 : k % 4 == 3 ? (N >= 8 ? 7 : N - 1)                          // last point of the first group
                                              : -1;
                deep_case(log_N, log_blowup, width, nterms, pad, off, z_at);
            }
    const size_t ncs[] = {1, 15, 16, 17, 4095, 4096, 4097, 9000};
    for (size_t nc : ncs)
        for (uint32_t batch : {1u, 3u})
            poly_case(nc, nc + (batch > 1 ? 3 : 0), batch, 1 + (uint32_t)((nc + batch) % 4));
    poly_case(40, 40, 2, 4);
    std::printf("DONE\n");
    return 0;
}
