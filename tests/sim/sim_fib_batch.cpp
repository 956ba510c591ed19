// Runs the kernels of include/toyni_hip.h 3s themselves -- the thirteen batch kernels of the first half of a Fibonacci proof in
// toyni_amd/csrc/batch/toyni_hip_fib_batch.hip -- on the CPU through hip_sim.hpp (unchanged), every GPU thread a fiber, under the eight wave / lane
// schedules of that header: THREE proofs per launch, a stride apart in one block of memory whose gaps must keep their fill.
//
// TEST INFRASTRUCTURE (tests/test_sim_fib_batch.py; tests/test_field_contracts_fib_batch.py rebuilds it with
// tests/emu/field_contracts.hpp in front).  Two judges: the SINGLE kernel of 3c / 3o / 3q on proof b's pointers, run through the same
// simulator, and plain host arithmetic (% p on 64-bit integers).  The buffers are arranged as the entry points arrange them (for the
// evaluation: batch x nblocks x npoints partial sums, then `batch` records).
//   sim_fib_batch [--saturated]            every case under all eight schedules; prints RAN / SITE lines; exit 1 on a failure
//   sim_fib_batch --only K                 the cases that launch kernel K
//   sim_fib_batch --drop K:i               the cases of kernel K with its i-th synchronisation site switched off: DROP ... FAILS / SURVIVES
#include "hip_sim.hpp"

#include <cstdio>
#include <cstring>
#include <new>
#include <set>
#include <string>
#include <vector>

#define TOYNI_KERNEL_TEXT_ONLY
#include "toyni_hip.hip"
#include "batch/toyni_hip_fib_batch.hip"   // section 3s: behind toyni_hip.hip, whose TRANSCRIPT_T and block_sum_mod it then uses
#include "../emu/contract_case.hpp"

alignas(16) uint32_t air_lds[4];   // named by the kernel section; no kernel that uses it runs here

extern "C" {
extern uint32_t __start_hipsim_lds[] __attribute__((weak)), __stop_hipsim_lds[] __attribute__((weak));
}
void hipsim::poison_shared() {
    for (uint32_t* p = __start_hipsim_lds; p < __stop_hipsim_lds; ++p) *p = 0xDEADBEEFu;
}

static int failures = 0;
static bool saturated = false;
static std::string only;
static std::set<std::string> instantiations;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class F>
static bool sim_launch(const char* name, dim3 grid, uint32_t block, F&& body) {
    instantiations.insert(name);
    TOYNI_CONTRACT_TAG("%s", name);
    const bool ok = hipsim::launch(name, "", grid, block, body);
    if (!ok) ++failures;
    return ok;
}
static bool wanted(std::initializer_list<const char*> tags) {
    if (only.empty()) return true;
    for (const char* t : tags) if (only == t) return true;
    return false;
}

static uint64_t sm_state;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t draw() {   // {0, 1, p - 1, random}; saturated: p - 1
    if (saturated) return BB_P - 1u;
    const uint64_t k = splitmix();
    return k % 8 == 0 ? 0u : k % 8 == 1 ? 1u : k % 8 == 2 ? BB_P - 1u : (uint32_t)(splitmix() % BB_P);
}
static uint32_t h_add(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + b) % BB_P); }
static uint32_t h_sub(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + BB_P - b) % BB_P); }

constexpr size_t NB = 3;                 // proofs per launch
constexpr uint32_t FILL = 0xCDCDCDCDu;   // never a canonical residue
// NB regions of `extent` words, `stride` words apart, behind a 16-byte boundary; everything starts as FILL
struct Strided {
    uint32_t* p;
    size_t extent, stride, total;
    Strided(size_t extent_, size_t stride_) : extent(extent_), stride(stride_), total((NB - 1) * stride_ + extent_) {
        p = static_cast<uint32_t*>(::operator new((total ? total : 1) * 4, std::align_val_t(16)));
        for (size_t i = 0; i < total; ++i) p[i] = FILL;
    }
    ~Strided() { ::operator delete(p, std::align_val_t(16)); }
    Strided(const Strided&) = delete;
    uint32_t* at(size_t b) { return p + b * stride; }
    void gaps(const char* what) {
        for (size_t b = 0; b + 1 < NB; ++b)
            for (size_t i = b * stride + extent; i < (b + 1) * stride; ++i)
                if (p[i] != FILL) { CHECK(false, "%s: the gap behind proof %zu was written at word %zu", what, b, i); return; }
    }
};
template <class T> struct Block {   // exactly `n` elements behind a 16-byte boundary
    T* p;
    explicit Block(size_t n) { p = static_cast<T*>(::operator new((n ? n : 1) * sizeof(T), std::align_val_t(16))); }
    ~Block() { ::operator delete(p, std::align_val_t(16)); }
    Block(const Block&) = delete;
};
static void draw_keys(uint32_t* keys) {
    for (size_t i = 0; i < 8 * NB; ++i) keys[i] = saturated ? 0xFFFFFFFFu : (uint32_t)splitmix();
}

// ---- salts ----
static void run_fill(uint64_t blocks) {
    sm_state = 0xF111ull + blocks;
    Block<uint32_t> keys(8 * NB);
    draw_keys(keys.p);
    Strided out(16 * blocks, 16 * blocks + 12);
    ChaChaBatchArgs a{};
    a.keys = keys.p;
    a.nonce[1] = 3u;
    a.blocks = blocks;
    a.out = reinterpret_cast<uint8_t*>(out.p);
    a.out_stride = 4 * out.stride;
    sim_launch("chacha20_fill_batch_kernel", dim3((unsigned)((blocks + 255) / 256), NB), 256, [&] { chacha20_fill_batch_kernel(a); });
    out.gaps("fill");
    for (size_t b = 0; b < NB; ++b) {
        Block<uint32_t> one(16 * blocks);
        ChaChaArgs s{};
        memcpy(s.key, keys.p + 8 * b, 32);
        s.nonce[1] = 3u;
        s.blocks = blocks;
        s.out = reinterpret_cast<uint4*>(one.p);
        sim_launch("chacha20_fill_kernel", dim3((unsigned)((blocks + 255) / 256)), 256, [&] { chacha20_fill_kernel(s); });
        CHECK(!memcmp(one.p, out.at(b), 64 * blocks), "fill: proof %zu differs from the single kernel", b);
        uint32_t ks[16];
        chacha20_block(s.key, (uint32_t)(blocks - 1), s.nonce, ks);
        CHECK(!memcmp(ks, out.at(b) + 16 * (blocks - 1), 64), "fill: proof %zu, last block", b);
    }
}

// ---- mask ----
static void run_mask(uint64_t n, uint32_t d) {
    sm_state = 0x3A5Cull + n * 3 + d;
    Block<uint32_t> keys(8 * NB);
    draw_keys(keys.p);
    Strided c(n + d, n + d + 3);
    std::vector<std::vector<uint32_t>> start(NB, std::vector<uint32_t>(n + d));
    for (size_t b = 0; b < NB; ++b)
        for (uint64_t i = 0; i < n + d; ++i) start[b][i] = c.at(b)[i] = i < n ? draw() : 0u;
    FibMaskArgs a{};
    a.coeffs = c.p;
    a.n = n;
    a.mask_degree = d;
    a.nonce[1] = 1u;
    const uint64_t items = fib_mask_items(n, d);
    sim_launch("fib_mask_batch_kernel", dim3((unsigned)((items + 255) / 256), NB), 256, [&] { fib_mask_batch_kernel(a, c.stride, keys.p); });
    c.gaps("mask");
    for (size_t b = 0; b < NB; ++b) {
        Block<uint32_t> one(n + d);
        memcpy(one.p, start[b].data(), 4 * (n + d));
        FibMaskArgs s = a;
        s.coeffs = one.p;
        memcpy(s.key, keys.p + 8 * b, 32);
        sim_launch("fib_mask_kernel", dim3((unsigned)((items + 255) / 256)), 256, [&] { fib_mask_kernel(s); });
        CHECK(!memcmp(one.p, c.at(b), 4 * (n + d)), "mask n=%llu: proof %zu differs from the single kernel", (unsigned long long)n, b);
        std::vector<uint32_t> want = start[b];
        uint32_t ks[16];
        for (uint32_t i = 0; i < d; ++i) {   // the loop of csrc/host/fib_prover.hpp
            if (i % 8 == 0) chacha20_block(s.key, i / 8, s.nonce, ks);
            const uint32_t r = (uint32_t)(((uint64_t)ks[2 * (i % 8)] | (uint64_t)ks[2 * (i % 8) + 1] << 32) % BB_P);
            want[i] = h_sub(want[i], r);
            want[n + i] = h_add(want[n + i], r);
        }
        for (uint64_t i = 0; i < n + d; ++i) CHECK(c.at(b)[i] == want[i], "mask n=%llu d=%u proof %zu word %llu", (unsigned long long)n, d, b, (unsigned long long)i);
    }
}

// ---- quotient ----
static void run_quotient(int log_N, int log_b, bool with_c, size_t gap) {
    sm_state = 0x9007ull + (uint64_t)log_N * 11 + gap;
    NttPlan plan;
    if (!build_plan(log_N, plan)) { CHECK(false, "plan"); return; }
    const uint64_t N = 1ull << log_N, B = 1ull << log_b, n = N >> log_b;
    const uint32_t shift = 7u, wN = bb_root_of_unity_host((uint32_t)log_N), g = bb_root_of_unity_host((uint32_t)(log_N - log_b));
    Strided trace(N, N + gap), cev(N, N + gap), q(N, N + gap);
    for (size_t b = 0; b < NB; ++b)
        for (uint64_t i = 0; i < N; ++i) trace.at(b)[i] = draw();
    QuotientArgs a{};
    a.trace = trace.p;
    a.c_out = with_c ? cev.p : nullptr;
    a.q_out = q.p;
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.log_N = (uint32_t)log_N;
    a.log_blowup = (uint32_t)log_b;
    a.b1R = to_mont_host(bb_pow_host(g, n - 1));
    a.b2R = to_mont_host(bb_pow_host(g, n - 2));
    a.shift_nR = to_mont_host(bb_pow_host(shift, n));
    a.wBR = to_mont_host(bb_pow_host(wN, n));
    const bool quads = log_b >= 2 && log_N >= 2 && !(gap & 3);
    const uint64_t items = quads ? N / 4 : N;
    const QuotientBatch st{trace.stride, cev.stride, q.stride};
    sim_launch("fib_quotient_batch_kernel", dim3((unsigned)((items + 255) / 256), NB), 256, [&] { fib_quotient_batch_kernel(a, st); });
    trace.gaps("quotient trace"), cev.gaps("quotient c"), q.gaps("quotient q");
    for (size_t b = 0; b < NB; ++b) {
        Block<uint32_t> c1(N), q1(N);
        QuotientArgs s = a;
        s.trace = trace.at(b);
        s.c_out = c1.p;
        s.q_out = q1.p;
        sim_launch("fib_quotient_kernel", dim3((unsigned)((N / 4 + 255) / 256)), 256, [&] { fib_quotient_kernel(s); });
        CHECK(!memcmp(q1.p, q.at(b), 4 * N), "quotient log_N=%d gap=%zu: proof %zu differs from the single kernel", log_N, gap, b);
        if (with_c) CHECK(!memcmp(c1.p, cev.at(b), 4 * N), "constraint log_N=%d: proof %zu differs from the single kernel", log_N, b);
        else CHECK(cev.at(b)[0] == FILL && cev.at(b)[N - 1] == FILL, "a null c_out was written");
        uint32_t x = shift;
        const uint32_t b1 = bb_pow_host(g, n - 1), b2 = bb_pow_host(g, n - 2);
        for (uint64_t i = 0; i < N; ++i) {
            const uint32_t* t = trace.at(b);
            const uint32_t fib = h_sub(t[(i + 2 * B) & (N - 1)], h_add(t[(i + B) & (N - 1)], t[i]));
            const uint32_t c = bb_mul_host(bb_mul_host(fib, h_sub(x, b1)), h_sub(x, b2));
            const uint32_t want = bb_mul_host(c, bb_inv_host(h_sub(bb_pow_host(x, n), 1u)));
            CHECK(q.at(b)[i] == want && (!with_c || cev.at(b)[i] == c), "quotient log_N=%d proof %zu point %llu", log_N, b, (unsigned long long)i);
            x = bb_mul_host(x, wN);
        }
    }
}

// ---- the transcripts: the middle one has its status set; the last one is so long that four fields overflow it ----
static void fill_transcripts(TranscriptState* tr, bool long_last) {
    for (size_t b = 0; b < NB; ++b) {
        memset(&tr[b], 0, sizeof tr[b]);
        memset(tr[b].bytes, 0x5A, sizeof tr[b].bytes);
        memcpy(tr[b].bytes, "toyni-stark-v1", 14);
        const uint64_t i = 3 * b;
        memcpy(tr[b].bytes + 14, &i, 8);
        tr[b].len = 22;
    }
    tr[1].status = TRANSCRIPT_E_RANGE;
    if (long_last) tr[NB - 1].len = TRANSCRIPT_CAPACITY - 31u;
}
static void run_point(uint32_t log_N) {
    alignas(16) static TranscriptState tr[NB], ref[NB], one[NB];
    fill_transcripts(tr, false);
    memcpy(ref, tr, sizeof tr);
    memcpy(one, tr, sizeof tr);
    const uint32_t inv = to_mont_host(bb_inv_host(7u));
    Strided z(1, 3);
    sim_launch("transcript_squeeze_point_batch_kernel", dim3(NB), TRANSCRIPT_T, [&] { transcript_squeeze_point_batch_kernel(tr, log_N, inv, z.p, z.stride); });
    z.gaps("point");
    for (size_t b = 0; b < NB; ++b) {
        uint32_t zr = FILL;
        transcript_squeeze_point(ref[b], log_N, inv, FIB_POINT_TRIES, &zr);           // the body, once, outside the simulator
        Block<uint32_t> z1(1);
        z1.p[0] = FILL;
        sim_launch("transcript_squeeze_point_kernel", dim3(1), TRANSCRIPT_T, [&] { transcript_squeeze_point_kernel(&one[b], log_N, inv, z1.p); });
        CHECK(z.at(b)[0] == zr && z1.p[0] == zr && !memcmp(&tr[b], &ref[b], sizeof tr[b]) && !memcmp(&tr[b], &one[b], sizeof tr[b]), "point: proof %zu", b);
        if (b == 1) CHECK(zr == 0u && tr[b].len == 22u && tr[b].status == TRANSCRIPT_E_RANGE, "point: a set status writes zero and keeps the state");
        else CHECK(tr[b].len == 32u && tr[b].status == 0u, "point: proof %zu state", b);
    }
}
static void run_absorb() {
    sm_state = 0xAB50ull;
    alignas(16) static TranscriptState tr[NB], before[NB], one[NB];
    fill_transcripts(tr, true);
    memcpy(before, tr, sizeof tr);
    memcpy(one, tr, sizeof tr);
    Strided w(4, 6);
    for (size_t b = 0; b < NB; ++b)
        for (int k = 0; k < 4; ++k) w.at(b)[k] = saturated ? BB_P - 1u : k == 1 ? BB_P + 3u : draw();     // one word needs the reduction
    sim_launch("transcript_absorb_fields_batch_kernel", dim3(NB), TRANSCRIPT_T, [&] { transcript_absorb_fields_batch_kernel(tr, w.p, w.stride, 4u); });
    w.gaps("absorb");
    for (size_t b = 0; b < NB; ++b) {
        sim_launch("transcript_absorb_fields_kernel", dim3(1), TRANSCRIPT_T, [&] { transcript_absorb_fields_kernel(&one[b], w.at(b), 4u); });
        CHECK(!memcmp(&tr[b], &one[b], sizeof tr[b]), "absorb: proof %zu differs from the single kernel", b);
    }
    // proof 0 absorbed 32 bytes: per word the LE64 of its residue; proof 1 (status set) is as it was; proof 2 overflowed: status, nothing else
    CHECK(tr[0].len == 54u && tr[0].status == 0u, "absorb: proof 0 len %u", tr[0].len);
    for (int k = 0; k < 4; ++k) {
        const uint64_t v = w.at(0)[k] % BB_P;
        CHECK(!memcmp(tr[0].bytes + 22 + 8 * k, &v, 8), "absorb: proof 0 word %d", k);
    }
    CHECK(!memcmp(&tr[1], &before[1], sizeof tr[1]), "absorb: a set status keeps the state");
    CHECK(tr[2].status == TRANSCRIPT_E_RANGE && tr[2].len == before[2].len && !memcmp(tr[2].bytes, before[2].bytes, sizeof tr[2].bytes), "absorb: the overflow");
}

// ---- the out-of-domain values: the buffer as toyni_poly_eval_dz_batch_device lays it out ----
struct PolySetup {
    uint32_t zc[NB];
    PolyDzMults m{};
};
static PolySetup poly_points(Strided& z, uint32_t npoints) {
    PolySetup s;
    const uint32_t g = bb_root_of_unity_host(6);
    const uint32_t mults[4] = {1u, g, bb_mul_host(g, g), BB_P - 1u};
    for (uint32_t p = 0; p < npoints; ++p) s.m.v[p] = saturated ? BB_P - 1u : mults[p];
    for (size_t b = 0; b < NB; ++b) {
        s.zc[b] = saturated ? BB_P - 1u : (uint32_t)(splitmix() % BB_P);
        z.at(b)[0] = (b & 1) ? s.zc[b] + BB_P : s.zc[b];        // the middle proof's z needs the reduction
    }
    return s;
}
static void run_poly(uint64_t ncoeffs, uint32_t npoints) {
    sm_state = 0xF1B0ull + ncoeffs * 7 + npoints;
    const uint32_t nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    const size_t partial_words = (NB * (size_t)nblocks * npoints + 3) & ~(size_t)3, rec_words = sizeof(PolyDzRecord) / 4;
    Strided coeffs(ncoeffs, ncoeffs + 5), z(1, 2), out(npoints, npoints + 1);
    Block<uint32_t> buffer(partial_words + NB * rec_words);
    for (size_t b = 0; b < NB; ++b)
        for (uint64_t i = 0; i < ncoeffs; ++i) coeffs.at(b)[i] = draw();
    const PolySetup s = poly_points(z, npoints);
    PolyEvalDzArgs a{};
    a.coeffs = coeffs.p;
    a.ncoeffs = ncoeffs;
    a.npoints = npoints;
    a.nblocks = nblocks;
    a.partial = buffer.p;
    a.out = out.p;
    PolyDzRecord* rec = reinterpret_cast<PolyDzRecord*>(buffer.p + partial_words);
    for (size_t i = 0; i < partial_words + NB * rec_words; ++i) buffer.p[i] = FILL;
    const PolyDzBatch st{coeffs.stride, out.stride};
    sim_launch("poly_dz_prepare_batch_kernel", dim3(NB), TRANSCRIPT_T, [&] { poly_dz_prepare_batch_kernel(z.p, z.stride, s.m, npoints, rec); });
    if (nblocks) sim_launch("poly_eval_partial_dz_batch_kernel", dim3(nblocks, NB), POLY_THREADS, [&] { poly_eval_partial_dz_batch_kernel(a, st, rec); });
    sim_launch("poly_eval_final_dz_batch_kernel", dim3(1, NB), 256, [&] { poly_eval_final_dz_batch_kernel(a, st, rec); });
    out.gaps("poly out"), coeffs.gaps("poly coeffs");
    for (size_t b = 0; b < NB; ++b) {
        // the single chain on proof b's pointers, its own buffer
        Block<uint32_t> one(npoints), buf1(partial_words + rec_words);
        PolyEvalDzArgs s1 = a;
        s1.coeffs = coeffs.at(b);
        s1.partial = buf1.p;
        s1.out = one.p;
        PolyDzRecord* rec1 = reinterpret_cast<PolyDzRecord*>(buf1.p + partial_words);
        sim_launch("poly_dz_prepare_kernel", dim3(1), TRANSCRIPT_T, [&] { poly_dz_prepare_kernel(z.at(b), s.m, npoints, rec1); });
        if (nblocks) sim_launch("poly_eval_partial_dz_kernel", dim3(nblocks), POLY_THREADS, [&] { poly_eval_partial_dz_kernel(s1, rec1); });
        sim_launch("poly_eval_final_dz_kernel", dim3(1), 256, [&] { poly_eval_final_dz_kernel(s1, rec1); });
        CHECK(!memcmp(one.p, out.at(b), 4 * npoints), "poly ncoeffs=%llu: proof %zu differs from the single kernels", (unsigned long long)ncoeffs, b);
        for (uint32_t p = 0; p < npoints; ++p) {
            CHECK(rec1->zR[p] == rec[b].zR[p] && rec1->z16R[p] == rec[b].z16R[p] && rec1->zchunkR[p] == rec[b].zchunkR[p], "poly: record %zu point %u", b, p);
            const uint32_t x = bb_mul_host(s.zc[b], s.m.v[p]);
            uint32_t acc = 0;
            for (uint64_t i = ncoeffs; i-- > 0;) acc = h_add(bb_mul_host(acc, x), coeffs.at(b)[i]);
            CHECK(out.at(b)[p] == acc, "poly ncoeffs=%llu proof %zu point %u: %u, want %u", (unsigned long long)ncoeffs, b, p, out.at(b)[p], acc);
        }
    }
}
// stage 2 alone on 300 partial sums per proof: only then do two waves' values meet in block_sum_mod's tree
static void run_poly_final(uint32_t nblocks, uint32_t npoints) {
    sm_state = 0xF1A7ull + nblocks;
    const size_t partial_words = (NB * (size_t)nblocks * npoints + 3) & ~(size_t)3, rec_words = sizeof(PolyDzRecord) / 4;
    Strided z(1, 2), out(npoints, npoints + 1);
    Block<uint32_t> buffer(partial_words + NB * rec_words);
    for (size_t i = 0; i < partial_words; ++i) buffer.p[i] = draw();
    const PolySetup s = poly_points(z, npoints);
    PolyEvalDzArgs a{};
    a.npoints = npoints;
    a.nblocks = nblocks;
    a.partial = buffer.p;
    a.out = out.p;
    PolyDzRecord* rec = reinterpret_cast<PolyDzRecord*>(buffer.p + partial_words);
    const PolyDzBatch st{0, out.stride};
    sim_launch("poly_dz_prepare_batch_kernel", dim3(NB), TRANSCRIPT_T, [&] { poly_dz_prepare_batch_kernel(z.p, z.stride, s.m, npoints, rec); });
    sim_launch("poly_eval_final_dz_batch_kernel", dim3(1, NB), 256, [&] { poly_eval_final_dz_batch_kernel(a, st, rec); });
    out.gaps("poly final");
    for (size_t b = 0; b < NB; ++b)
        for (uint32_t p = 0; p < npoints; ++p) {
            const uint32_t xc = bb_pow_host(bb_mul_host(s.zc[b], s.m.v[p]), POLY_CHUNK);
            uint32_t acc = 0, pw = 1;
            for (uint32_t k = 0; k < nblocks; ++k) {
                acc = h_add(acc, bb_mul_host(buffer.p[(b * nblocks + k) * npoints + p], pw));
                pw = bb_mul_host(pw, xc);
            }
            CHECK(out.at(b)[p] == acc, "poly final nblocks=%u proof %zu point %u: %u, want %u", nblocks, b, p, out.at(b)[p], acc);
        }
}

// ---- the DEEP layer ----
static void run_deep(int log_N, int log_b, bool with_check) {
    sm_state = 0xDEE9ull + (uint64_t)log_N * 5;
    NttPlan plan;
    if (!build_plan(log_N, plan)) { CHECK(false, "plan"); return; }
    const uint64_t N = 1ull << log_N, B = 1ull << log_b, n = N >> log_b;
    const uint32_t shift = 7u, wN = bb_root_of_unity_host((uint32_t)log_N);
    Strided trace(N, N + 1), quot(N, N + 2), out(N, N + 3), z(1, 3), ood(4, 5), chk(1, 2);
    Block<uint32_t> recw(NB * sizeof(FibDeepRecord) / 4);
    uint32_t zc[NB], v[NB][4];
    for (size_t b = 0; b < NB; ++b) {
        for (uint64_t i = 0; i < N; ++i) { trace.at(b)[i] = draw(); quot.at(b)[i] = draw(); }
        // proof 1's z lies on the coset (x_i = z at the last point) and its words need the reduction
        zc[b] = saturated ? BB_P - 1u : b == 1 ? bb_mul_host(shift, bb_pow_host(wN, N - 1)) : (uint32_t)(splitmix() % BB_P);
        z.at(b)[0] = b == 1 ? zc[b] + BB_P : zc[b];
        for (int k = 0; k < 4; ++k) {
            v[b][k] = draw();
            ood.at(b)[k] = b == 1 && v[b][k] + (uint64_t)BB_P <= 0xFFFFFFFFull ? v[b][k] + BB_P : v[b][k];
        }
    }
    FibDeepRecord* rec = reinterpret_cast<FibDeepRecord*>(recw.p);
    FibCheckArgs k{};
    k.log_n = (uint32_t)(log_N - log_b);
    const uint32_t gn = bb_root_of_unity_host(k.log_n), g_inv = bb_inv_host(gn);
    k.b1R = to_mont_host(g_inv);
    k.b2R = to_mont_host(bb_mul_host(g_inv, g_inv));
    DeepArgs a{};
    a.trace = trace.p;
    a.quot = quot.p;
    a.out = out.p;
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.log_N = (uint32_t)log_N;
    a.log_blowup = (uint32_t)log_b;
    a.wNR = to_mont_host(wN);
    const FibDeepBatch st{trace.stride, quot.stride, out.stride, z.stride, ood.stride, chk.stride};
    uint32_t* check = with_check ? chk.p : nullptr;
    sim_launch("fib_deep_prepare_batch_kernel", dim3(NB), TRANSCRIPT_T, [&] { fib_deep_prepare_batch_kernel(z.p, ood.p, k, st, rec, check); });
    const uint64_t items = log_N >= 3 ? N / 8 : N;
    sim_launch("fib_deep_dz_batch_kernel", dim3((unsigned)((items + 255) / 256), NB), 256, [&] { fib_deep_dz_batch_kernel(a, st, rec); });
    out.gaps("deep out"), chk.gaps("deep check"), trace.gaps("deep trace");
    for (size_t b = 0; b < NB; ++b) {
        Block<uint32_t> one(N), chk1(1), rec1w(sizeof(FibDeepRecord) / 4);
        FibDeepRecord* rec1 = reinterpret_cast<FibDeepRecord*>(rec1w.p);
        chk1.p[0] = FILL;
        DeepArgs s = a;
        s.trace = trace.at(b);
        s.quot = quot.at(b);
        s.out = one.p;
        sim_launch("fib_deep_prepare_kernel", dim3(1), TRANSCRIPT_T, [&] { fib_deep_prepare_kernel(z.at(b), ood.at(b), k, rec1, with_check ? chk1.p : nullptr); });
        sim_launch("fib_deep_dz_kernel", dim3((unsigned)((items + 255) / 256)), 256, [&] { fib_deep_dz_kernel(s, rec1); });
        CHECK(!memcmp(one.p, out.at(b), 4 * N) && chk1.p[0] == chk.at(b)[0], "deep log_N=%d: proof %zu differs from the single kernels", log_N, b);
        uint32_t x = shift;
        for (uint64_t i = 0; i < N; ++i) {
            const uint32_t* t = trace.at(b);
            const uint32_t num = h_add(h_add(h_sub(quot.at(b)[i], v[b][3]), h_sub(t[(i + 2 * B) & (N - 1)], v[b][2])),
                                       h_add(h_sub(t[(i + B) & (N - 1)], v[b][1]), h_sub(t[i], v[b][0])));
            const uint32_t d = h_sub(x, zc[b]), want = d ? bb_mul_host(num, bb_inv_host(d)) : 0u;
            CHECK(out.at(b)[i] == want, "deep log_N=%d proof %zu point %llu: %u, want %u", log_N, b, (unsigned long long)i, out.at(b)[i], want);
            x = bb_mul_host(x, wN);
        }
        const uint32_t lhs = bb_mul_host(bb_mul_host(h_sub(v[b][2], h_add(v[b][1], v[b][0])), h_sub(zc[b], bb_pow_host(gn, n - 1))),
                                         h_sub(zc[b], bb_pow_host(gn, (2 * n - 2) % n)));
        const uint32_t rhs = bb_mul_host(v[b][3], h_sub(bb_pow_host(zc[b], n), 1u));
        CHECK(chk.at(b)[0] == (with_check ? (lhs == rhs ? 1u : 0u) : FILL), "check word of proof %zu: %u", b, chk.at(b)[0]);
    }
}

// ---- rows, roots, copies ----
static void run_rows(uint32_t count, uint64_t n) {
    sm_state = 0x7035ull + count;
    Strided idx(count, count + 1), out(3 * (size_t)count, 3 * (size_t)count + 2);
    for (size_t b = 0; b < NB; ++b)
        for (uint32_t i = 0; i < count; ++i) idx.at(b)[i] = saturated ? (uint32_t)(n - 1) : (uint32_t)(splitmix() % n);
    QueryRowOffsets off{};
    off.v[0] = 0u; off.v[1] = (uint32_t)(n / 8); off.v[2] = (uint32_t)(n - 1);
    const uint64_t total = 3ull * count;
    sim_launch("query_rows_batch_kernel", dim3((unsigned)((total + 255) / 256), NB), 256,
               [&] { query_rows_batch_kernel(idx.p, idx.stride, off, 3u, n, total, out.p, out.stride); });
    out.gaps("rows");
    for (size_t b = 0; b < NB; ++b)
        for (uint64_t t = 0; t < total; ++t)
            CHECK(out.at(b)[t] == (uint32_t)(((uint64_t)idx.at(b)[t / 3] + off.v[t % 3]) % n), "rows: proof %zu word %llu", b, (unsigned long long)t);
}
static void run_roots(uint64_t m_first, uint32_t rounds) {
    sm_state = 0x2007ull + m_first;
    uint64_t digests = 0;
    for (uint32_t k = 0; k < rounds; ++k) digests += 2 * (m_first >> k) - 1;
    Strided levels(8 * digests, 8 * digests + 4), roots(8 * rounds, 8 * rounds + 1);
    for (size_t b = 0; b < NB; ++b)
        for (uint64_t i = 0; i < 8 * digests; ++i) levels.at(b)[i] = (uint32_t)splitmix();
    sim_launch("fri_phase_roots_batch_kernel", dim3(NB), 256, [&] { fri_phase_roots_batch_kernel(levels.p, levels.stride, m_first, rounds, roots.p, roots.stride); });
    roots.gaps("roots");
    for (size_t b = 0; b < NB; ++b) {
        uint64_t end = 0;
        for (uint32_t k = 0; k < rounds; ++k) {
            end += 2 * (m_first >> k) - 1;
            CHECK(!memcmp(roots.at(b) + 8 * k, levels.at(b) + 8 * (end - 1), 32), "roots: proof %zu root %u", b, k);
        }
    }
}
static void run_copy(uint64_t row_bytes, bool aligned) {
    sm_state = 0xC0B7ull + row_bytes;
    const size_t words = row_bytes / 4, round = (words + 3) & ~(size_t)3;
    Strided src(words, round + (aligned ? 4 : 1)), dst(words, round + (aligned ? 8 : 3));
    for (size_t b = 0; b < NB; ++b)
        for (size_t i = 0; i < words; ++i) src.at(b)[i] = (uint32_t)splitmix();
    const uint64_t quads = aligned ? row_bytes / 16 : 0;
    const uint64_t items = quads > words - 4 * quads ? quads : words - 4 * quads;
    sim_launch("copy_rows_kernel", dim3((unsigned)((items + 255) / 256), NB), 256,
               [&] { copy_rows_kernel(reinterpret_cast<uint8_t*>(dst.p), 4 * dst.stride, reinterpret_cast<const uint8_t*>(src.p), 4 * src.stride, row_bytes, quads); });
    dst.gaps("copy");
    for (size_t b = 0; b < NB; ++b) CHECK(!memcmp(dst.at(b), src.at(b), row_bytes), "copy %llu bytes: row %zu", (unsigned long long)row_bytes, b);
}

static void run_all_cases() {
    if (wanted({"chacha20_fill_batch_kernel"})) { run_fill(1); run_fill(300); }
    if (wanted({"fib_mask_batch_kernel"})) { run_mask(8, 140); run_mask(256, 140); run_mask(300, 1); }
    if (wanted({"fib_quotient_batch_kernel"})) {
        run_quotient(2, 1, true, 4);          // N = 4, log_blowup = 1: the scalar path
        run_quotient(8, 5, true, 4);          // N = 256, 16-byte accesses in every proof
        run_quotient(8, 5, false, 5);         // the middle proof loses the alignment; no constraint output
    }
    if (wanted({"transcript_squeeze_point_batch_kernel"})) { run_point(27); run_point(5); }
    if (wanted({"transcript_absorb_fields_batch_kernel"})) run_absorb();
    if (wanted({"poly_dz_prepare_batch_kernel", "poly_eval_partial_dz_batch_kernel", "poly_eval_final_dz_batch_kernel"})) {
        run_poly(POLY_CHUNK + 1, 3);
        if (only.empty()) { run_poly(0, 2); run_poly(1, 1); run_poly(POLY_CHUNK - 1, 4); }
    }
    if (wanted({"poly_dz_prepare_batch_kernel", "poly_eval_final_dz_batch_kernel"})) run_poly_final(300, 2);
    if (wanted({"fib_deep_prepare_batch_kernel", "fib_deep_dz_batch_kernel"})) {
        run_deep(2, 1, true);                 // N = 4: the scalar path
        run_deep(8, 5, true);
        run_deep(8, 5, false);
    }
    if (wanted({"query_rows_batch_kernel"})) { run_rows(44, 256); run_rows(300, 1ull << 32); }
    if (wanted({"fri_phase_roots_batch_kernel"})) { run_roots(256, 7); run_roots(1, 1); }
    if (wanted({"copy_rows_kernel"}))
        for (uint64_t bytes : {4, 32, 36, 4 * 1100})
            for (bool aligned : {true, false}) run_copy(bytes, aligned);
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    hipsim::State& s = hipsim::st();
    bool drop = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--only") && i + 1 < argc) only = argv[++i];
        else if (!std::strcmp(argv[i], "--saturated")) saturated = true;
        else if (!std::strcmp(argv[i], "--drop") && i + 1 < argc) {
            const char* colon = std::strrchr(argv[++i], ':');
            if (!colon) { std::printf("usage: --drop kernel:ordinal\n"); return 2; }
            only = std::string((const char*)argv[i], (const char*)colon);
            s.drop_kernel = only;
            s.drop_site = std::atoi(colon + 1);
            drop = true;
        } else { std::printf("usage: sim_fib_batch [--saturated] [--only kernel | --drop kernel:ordinal]\n"); return 2; }
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
