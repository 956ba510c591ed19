// Runs the kernels of include/toyni_hip.h 3q themselves -- fib_mask_kernel, transcript_squeeze_point_kernel, poly_dz_prepare_kernel,
// poly_eval_partial_dz_kernel, poly_eval_final_dz_kernel, fib_deep_prepare_kernel, fib_deep_dz_kernel, fri_phase_roots_kernel of
// toyni_amd/csrc/toyni_hip.hip -- on the CPU through hip_sim.hpp (unchanged), every GPU thread a fiber, under the eight wave / lane
// schedules of that header.
//
// TEST INFRASTRUCTURE (tests/test_sim_fib_dz.py; tests/test_field_contracts_fib_dz.py rebuilds it with tests/emu/field_contracts.hpp in
// front).  The driver arranges the buffers as the entry points do (the partial sums and then the record) and checks every output word
// against plain host arithmetic (% p on 64-bit integers): Horner per point, the DEEP quotient per point by a Fermat inverse, the mask
// by the loop of csrc/host/fib_prover.hpp, the point rule by the body run once outside the simulator (tests/test_emu_fib_dz.py holds
// that body to Python integers).
//   sim_fib_dz [--saturated]               every case under all eight schedules; prints RAN / SITE lines; exit 1 on a failure
//   sim_fib_dz --only K                    the cases that launch kernel K
//   sim_fib_dz --drop K:i                  the cases of kernel K with its i-th synchronisation site switched off: DROP ... FAILS / SURVIVES
#include "hip_sim.hpp"

#include <cstdio>
#include <cstring>
#include <new>
#include <set>
#include <string>
#include <vector>

#define TOYNI_KERNEL_TEXT_ONLY
#include "toyni_hip.hip"
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
template <class T> struct Block {   // exactly `n` elements behind a 16-byte boundary
    T* p;
    explicit Block(size_t n) { p = static_cast<T*>(::operator new((n ? n : 1) * sizeof(T), std::align_val_t(16))); }
    ~Block() { ::operator delete(p, std::align_val_t(16)); }
    Block(const Block&) = delete;
};

// z as a device word: canonical, or the same residue as a word that needs the reduction
static void run_poly(uint64_t ncoeffs, uint32_t npoints, bool lifted) {
    sm_state = 0xF1B0ull + ncoeffs * 7 + npoints;
    const uint32_t nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    const size_t partial_words = ((size_t)nblocks * npoints + 3) & ~(size_t)3;
    Block<uint32_t> coeffs(ncoeffs), z(1), out(npoints), buffer(partial_words + sizeof(PolyDzRecord) / 4);
    for (uint64_t i = 0; i < ncoeffs; ++i) coeffs.p[i] = draw();
    const uint32_t zc = saturated ? BB_P - 1u : (uint32_t)(splitmix() % BB_P), g = bb_root_of_unity_host(6);
    z.p[0] = lifted ? zc + BB_P : zc;
    PolyDzMults m{};
    const uint32_t mults[4] = {1u, g, bb_mul_host(g, g), BB_P - 1u};
    for (uint32_t p = 0; p < npoints; ++p) m.v[p] = saturated ? BB_P - 1u : mults[p];
    PolyEvalDzArgs a{};
    a.coeffs = coeffs.p;
    a.ncoeffs = ncoeffs;
    a.npoints = npoints;
    a.nblocks = nblocks;
    a.partial = buffer.p;
    a.out = out.p;
    PolyDzRecord* rec = reinterpret_cast<PolyDzRecord*>(buffer.p + partial_words);
    for (size_t i = 0; i < partial_words + sizeof(PolyDzRecord) / 4; ++i) buffer.p[i] = 0xCDCDCDCDu;
    for (uint32_t p = 0; p < npoints; ++p) out.p[p] = 0xCDCDCDCDu;
    sim_launch("poly_dz_prepare_kernel", dim3(1), TRANSCRIPT_T, [&] { poly_dz_prepare_kernel(z.p, m, npoints, rec); });
    sim_launch("poly_eval_partial_dz_kernel", dim3(nblocks), POLY_THREADS, [&] { poly_eval_partial_dz_kernel(a, rec); });
    sim_launch("poly_eval_final_dz_kernel", dim3(1), 256, [&] { poly_eval_final_dz_kernel(a, rec); });
    for (uint32_t p = 0; p < npoints; ++p) {
        const uint32_t x = bb_mul_host(zc, m.v[p]);
        uint32_t acc = 0;
        for (uint64_t i = ncoeffs; i-- > 0;) acc = h_add(bb_mul_host(acc, x), coeffs.p[i]);
        CHECK(out.p[p] == acc, "poly ncoeffs=%llu point %u: %u, want %u", (unsigned long long)ncoeffs, p, out.p[p], acc);
    }
}

// stage 2 alone on more partial sums than a wave has lanes: only then do two waves' values meet in block_sum_mod's tree (300 chunks
// through stage 1 would be 1.2 M coefficients; the sums of stage 1 are arbitrary residues as far as stage 2 is concerned)
static void run_poly_final(uint32_t nblocks, uint32_t npoints) {
    sm_state = 0xF1A7ull + nblocks;
    const size_t partial_words = ((size_t)nblocks * npoints + 3) & ~(size_t)3;
    Block<uint32_t> z(1), out(npoints), buffer(partial_words + sizeof(PolyDzRecord) / 4);
    for (size_t i = 0; i < partial_words; ++i) buffer.p[i] = draw();
    const uint32_t zc = saturated ? BB_P - 1u : (uint32_t)(splitmix() % BB_P);
    z.p[0] = zc;
    PolyDzMults m{};
    for (uint32_t p = 0; p < npoints; ++p) m.v[p] = saturated ? BB_P - 1u : p ? (uint32_t)(splitmix() % BB_P) : 1u;
    PolyEvalDzArgs a{};
    a.npoints = npoints;
    a.nblocks = nblocks;
    a.partial = buffer.p;
    a.out = out.p;
    PolyDzRecord* rec = reinterpret_cast<PolyDzRecord*>(buffer.p + partial_words);
    sim_launch("poly_dz_prepare_kernel", dim3(1), TRANSCRIPT_T, [&] { poly_dz_prepare_kernel(z.p, m, npoints, rec); });
    for (uint32_t p = 0; p < npoints; ++p) out.p[p] = 0xCDCDCDCDu;
    sim_launch("poly_eval_final_dz_kernel", dim3(1), 256, [&] { poly_eval_final_dz_kernel(a, rec); });
    for (uint32_t p = 0; p < npoints; ++p) {
        const uint32_t xc = bb_pow_host(bb_mul_host(zc, m.v[p]), POLY_CHUNK);
        uint32_t acc = 0, pw = 1;
        for (uint32_t b = 0; b < nblocks; ++b) {
            acc = h_add(acc, bb_mul_host(buffer.p[(size_t)b * npoints + p], pw));
            pw = bb_mul_host(pw, xc);
        }
        CHECK(out.p[p] == acc, "poly final nblocks=%u point %u: %u, want %u", nblocks, p, out.p[p], acc);
    }
}

static void run_deep(int log_N, int log_b, bool on_coset, bool lifted) {
    sm_state = 0xDEE9ull + (uint64_t)log_N * 5 + on_coset;
    NttPlan plan;
    if (!build_plan(log_N, plan)) { CHECK(false, "plan"); return; }
    const uint64_t N = 1ull << log_N, B = 1ull << log_b, n = N >> log_b;
    const uint32_t shift = 7u, wN = bb_root_of_unity_host((uint32_t)log_N);
    Block<uint32_t> trace(N), quot(N), out(N), z(1), ood(4), chk(1), recw(sizeof(FibDeepRecord) / 4);
    for (uint64_t i = 0; i < N; ++i) { trace.p[i] = draw(); quot.p[i] = draw(); out.p[i] = 0xCDCDCDCDu; }
    const uint32_t zc = saturated ? BB_P - 1u : on_coset ? bb_mul_host(shift, bb_pow_host(wN, N - 1)) : (uint32_t)(splitmix() % BB_P);
    uint32_t v[4];
    for (int k = 0; k < 4; ++k) v[k] = draw();
    z.p[0] = lifted ? zc + BB_P : zc;
    for (int k = 0; k < 4; ++k) ood.p[k] = lifted && v[k] + (uint64_t)BB_P <= 0xFFFFFFFFull ? v[k] + BB_P : v[k];
    chk.p[0] = 0xCDCDCDCDu;
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
    sim_launch("fib_deep_prepare_kernel", dim3(1), TRANSCRIPT_T, [&] { fib_deep_prepare_kernel(z.p, ood.p, k, rec, chk.p); });
    const uint64_t items = log_N >= 3 ? N / 8 : N;
    sim_launch("fib_deep_dz_kernel", dim3((unsigned)((items + 255) / 256)), 256, [&] { fib_deep_dz_kernel(a, rec); });
    uint32_t x = shift;
    for (uint64_t i = 0; i < N; ++i) {
        const uint32_t num = h_add(h_add(h_sub(quot.p[i], v[3]), h_sub(trace.p[(i + 2 * B) & (N - 1)], v[2])),
                                   h_add(h_sub(trace.p[(i + B) & (N - 1)], v[1]), h_sub(trace.p[i], v[0])));
        const uint32_t d = h_sub(x, zc), want = d ? bb_mul_host(num, bb_inv_host(d)) : 0u;
        CHECK(out.p[i] == want, "deep log_N=%d point %llu: %u, want %u", log_N, (unsigned long long)i, out.p[i], want);
        x = bb_mul_host(x, wN);
    }
    const uint32_t lhs = bb_mul_host(bb_mul_host(h_sub(v[2], h_add(v[1], v[0])), h_sub(zc, bb_pow_host(gn, n - 1))), h_sub(zc, bb_pow_host(gn, (2 * n - 2) % n)));
    const uint32_t rhs = bb_mul_host(v[3], h_sub(bb_pow_host(zc, n), 1u));
    CHECK(chk.p[0] == (lhs == rhs ? 1u : 0u), "check word %u", chk.p[0]);
}

static void run_mask(uint64_t n, uint32_t d) {
    sm_state = 0x3A5Cull + n * 3 + d;
    Block<uint32_t> c(n + d);
    std::vector<uint32_t> want(n + d);
    for (uint64_t i = 0; i < n + d; ++i) want[i] = c.p[i] = i < n ? draw() : 0u;
    FibMaskArgs a{};
    a.coeffs = c.p;
    a.n = n;
    a.mask_degree = d;
    for (int k = 0; k < 8; ++k) a.key[k] = saturated ? 0xFFFFFFFFu : (uint32_t)splitmix();
    a.nonce[1] = 1u;
    uint32_t ks[16];
    for (uint32_t i = 0; i < d; ++i) {   // the loop of csrc/host/fib_prover.hpp
        if (i % 8 == 0) chacha20_block(a.key, i / 8, a.nonce, ks);
        const uint32_t r = (uint32_t)(((uint64_t)ks[2 * (i % 8)] | (uint64_t)ks[2 * (i % 8) + 1] << 32) % BB_P);
        want[i] = h_sub(want[i], r);
        want[n + i] = h_add(want[n + i], r);
    }
    const uint64_t items = fib_mask_items(n, d);
    sim_launch("fib_mask_kernel", dim3((unsigned)((items + 255) / 256)), 256, [&] { fib_mask_kernel(a); });
    for (uint64_t i = 0; i < n + d; ++i) CHECK(c.p[i] == want[i], "mask n=%llu d=%u word %llu: %u, want %u", (unsigned long long)n, d, (unsigned long long)i, c.p[i], want[i]);
}

static void run_point(uint64_t i, uint32_t log_N) {
    alignas(16) static TranscriptState tr, ref;
    memset(&ref, 0, sizeof ref);
    memset(ref.bytes, 0x5A, sizeof ref.bytes);
    memcpy(ref.bytes, "toyni-stark-v1", 14);
    memcpy(ref.bytes + 14, &i, 8);
    ref.len = 22;
    tr = ref;
    const uint32_t inv = to_mont_host(bb_inv_host(7u));
    uint32_t zr = 0xCDCDCDCDu;
    transcript_squeeze_point(ref, log_N, inv, FIB_POINT_TRIES, &zr);
    Block<uint32_t> z(1);
    z.p[0] = 0xCDCDCDCDu;
    sim_launch("transcript_squeeze_point_kernel", dim3(1), TRANSCRIPT_T, [&] { transcript_squeeze_point_kernel(&tr, log_N, inv, z.p); });
    CHECK(z.p[0] == zr && !memcmp(&tr, &ref, sizeof tr) && tr.len == 32 && tr.status == 0, "point i=%llu", (unsigned long long)i);
}

static void run_roots(uint64_t m_first, uint32_t rounds) {
    sm_state = 0x2007ull + m_first;
    uint64_t digests = 0;
    for (uint32_t k = 0; k < rounds; ++k) digests += 2 * (m_first >> k) - 1;
    Block<uint32_t> levels(8 * digests), roots(8 * rounds + 8);
    for (uint64_t i = 0; i < 8 * digests; ++i) levels.p[i] = (uint32_t)splitmix();
    for (uint32_t i = 0; i < 8 * rounds + 8; ++i) roots.p[i] = 0xCDCDCDCDu;
    sim_launch("fri_phase_roots_kernel", dim3(1), 256, [&] { fri_phase_roots_kernel(levels.p, m_first, rounds, roots.p); });
    uint64_t end = 0;
    for (uint32_t k = 0; k < rounds; ++k) {
        end += 2 * (m_first >> k) - 1;
        CHECK(!memcmp(roots.p + 8 * k, levels.p + 8 * (end - 1), 32), "root %u", k);
    }
    for (uint32_t i = 0; i < 8; ++i) CHECK(roots.p[8 * rounds + i] == 0xCDCDCDCDu, "word behind the roots");
}

static void run_all_cases() {
    if (wanted({"poly_dz_prepare_kernel", "poly_eval_partial_dz_kernel", "poly_eval_final_dz_kernel"})) {
        run_poly(4097, 3, false);
        run_poly(64 + 140, 3, true);
        if (only.empty()) { run_poly(1, 1, false); run_poly(4095, 4, true); }
        run_poly(2 * 4096 + 5, 2, false);
    }
    if (wanted({"poly_dz_prepare_kernel", "poly_eval_final_dz_kernel"})) run_poly_final(300, 2);
    if (wanted({"fib_deep_prepare_kernel", "fib_deep_dz_kernel"})) {
        run_deep(2, 1, false, false);
        run_deep(3, 1, true, true);
        run_deep(8, 5, false, true);
        run_deep(11, 5, true, false);
    }
    if (wanted({"fib_mask_kernel"}))
        for (uint64_t n : {8, 128, 140, 141, 256}) { run_mask(n, 140); run_mask(n, 1); }
    if (wanted({"transcript_squeeze_point_kernel"})) { run_point(0, 27); run_point(3, 27); run_point(92, 5); }
    if (wanted({"fri_phase_roots_kernel"})) { run_roots(256, 7); run_roots(1, 1); run_roots(1ull << 11, 12); }
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
        } else { std::printf("usage: sim_fib_dz [--saturated] [--only kernel | --drop kernel:ordinal]\n"); return 2; }
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
