// Runs the four __global__ functions of the Ext accumulator columns (ext_accum_aggregate / _prefix / _apply_kernel and
// ext_invert_columns_kernel of toyni_amd/csrc/toyni_hip.hip, include/toyni_hip.h 3i) themselves on the CPU under the adversarial wave
// schedules of hip_sim.hpp, the way sim_kernels.cpp runs the other kernels.
//
// TEST INFRASTRUCTURE (tests/test_sim_scan_ext.py).  What the kernels must write is computed here on the host by a route that shares
// nothing with theirs -- Ext products by ext_mul_host, the inverse through the Frobenius norm a a^p a^(p^2) a^(p^3) -- and printed once
// (records CASE / ... / WANT) so that the test recomputes it with tests/ext_model.py in Python integers; under every schedule the
// kernels' words are compared with it here.
//
//   sim_scan_ext                      every case under all eight schedules; prints the records, the instantiations and the sites, ALL OK
//   sim_scan_ext --only K             the cases of kernel K alone
//   sim_scan_ext --drop K:i           the cases of kernel K with its i-th synchronisation site switched off: DROP ... FAILS / SURVIVES
#include "hip_sim.hpp"

#include <cstdio>
#include <cstring>
#include <set>

#define TOYNI_KERNEL_TEXT_ONLY
#include "toyni_hip.hip"
#include "../emu/contract_case.hpp"

alignas(16) uint32_t air_lds[4];   // named by the kernel section; no kernel that uses it runs here

extern "C" {
extern uint32_t __start_hipsim_lds[], __stop_hipsim_lds[];   // every __shared__ array lives in this section
}
void hipsim::poison_shared() {
    for (uint32_t* p = __start_hipsim_lds; p < __stop_hipsim_lds; ++p) *p = 0xDEADBEEFu;
}

static int failures = 0;
static bool print_records = true;              // the first schedule prints what the test recomputes
static std::string only;
static std::set<std::string> instantiations;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class F>
static bool sim_launch(const char* name, const std::string& inst, dim3 grid, uint32_t block, F&& body) {
    instantiations.insert(std::string(name) + inst);
    TOYNI_CONTRACT_TAG("%s%s", name, inst.c_str());
    const bool ok = hipsim::launch(name, inst, grid, block, body);
    if (!ok) ++failures;
    return ok;
}
static bool wanted(const char* tag) { return only.empty() || only == tag; }

static uint64_t sm_state;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t rnd() { return (uint32_t)(splitmix() % BB_P); }
static uint32_t rnd_nonzero() { return 1u + (uint32_t)(splitmix() % (BB_P - 1)); }

// ---- the host model ----
struct E4 { uint32_t c[4]; };
static bool is_zero(const E4& a) { return !(a.c[0] | a.c[1] | a.c[2] | a.c[3]); }
static E4 e_add(const E4& a, const E4& b) {
    E4 r;
    for (int k = 0; k < 4; ++k) r.c[k] = (uint32_t)(((uint64_t)a.c[k] + b.c[k]) % BB_P);
    return r;
}
static E4 e_mul(const E4& a, const E4& b) { E4 r; ext_mul_host(a.c, b.c, r.c); return r; }
static E4 e_inv(const E4& a) {   // a^p a^(p^2) a^(p^3) / N(a), N(a) = a a^p a^(p^2) a^(p^3) in F_p; 0 for 0
    if (is_zero(a)) return a;
    E4 f1, f2, f3;
    ext_pow_host(a.c, BB_P, f1.c);
    ext_pow_host(f1.c, BB_P, f2.c);
    ext_pow_host(f2.c, BB_P, f3.c);
    const E4 adj = e_mul(e_mul(f1, f2), f3), nrm = e_mul(a, adj);
    if (nrm.c[1] | nrm.c[2] | nrm.c[3]) { ++failures; std::printf("FAIL the norm of the host model left the base field\n"); }
    const uint32_t ni = bb_inv_host(nrm.c[0]);
    E4 r;
    for (int k = 0; k < 4; ++k) r.c[k] = bb_mul_host(adj.c[k], ni);
    return r;
}
template <int OP> static E4 e_op(const E4& a, const E4& b) { return OP == (int)SCAN_PRODUCT ? e_mul(a, b) : e_add(a, b); }
static E4 e_to_mont(const E4& a) { return E4{{to_mont_host(a.c[0]), to_mont_host(a.c[1]), to_mont_host(a.c[2]), to_mont_host(a.c[3])}}; }

static void print_words(const char* tag, uint32_t b, int k, const uint32_t* v, size_t n) {
    if (!print_records) return;
    std::printf("%s %u %d", tag, b, k);
    for (size_t i = 0; i < n; ++i) std::printf(" %u", v[i]);
    std::printf("\n");
}
static E4 operand_at(const ExtAccumOperand& o, uint32_t b, size_t i) {
    E4 v = {{1u, 0u, 0u, 0u}};
    if (o.width == 1) v = E4{{o.values[b * o.stride + i], 0u, 0u, 0u}};
    if (o.width == 4) for (int k = 0; k < 4; ++k) v.c[k] = o.values[(4 * b + k) * o.stride + i];
    if (o.width) v = e_add(v, E4{{o.shift[0], o.shift[1], o.shift[2], o.shift[3]}});
    return v;
}

constexpr uint32_t SLACK = 0xFFFFFFF0u;

// inplace: 0 no, 1 on the (width-4) numerator, 2 on the (width-4) denominator.  Zero denominators: a width-4 one stores -shift; a
// width-1 one gets the base shift (s, 0, 0, 0) and stores p - s.
template <int OP>
static void run_accum(size_t n, uint32_t batch, uint32_t nw, uint32_t dw, int inplace) {
    sm_state = 0xE5CAull + n * 7 + batch * 3 + nw * 11 + dw * 13 + OP;
    const size_t stride = n + 3;
    std::vector<uint32_t> num(nw ? stride * nw * batch : 1, SLACK), den(dw ? stride * dw * batch : 1, SLACK), out(stride * 4 * batch, SLACK);
    ExtAccumArgs a{};
    a.num = ExtAccumOperand{nw ? num.data() : nullptr, stride, nw, {0, 0, 0, 0}};
    a.den = ExtAccumOperand{dw ? den.data() : nullptr, stride, dw, {0, 0, 0, 0}};
    for (int k = 0; k < 4; ++k) {
        if (nw) a.num.shift[k] = rnd_nonzero();
        if (dw && (dw == 4 || k == 0)) a.den.shift[k] = rnd_nonzero();
    }
    for (uint32_t b = 0; b < batch; ++b)
        for (size_t i = 0; i < n; ++i) {
            const bool zero = i % 509 == 7 || (i == n - 1 && n > 1) || i % EXT_ACCUM_TILE == EXT_ACCUM_TILE - 1;
            for (uint32_t k = 0; k < nw; ++k) num[(nw * b + k) * stride + i] = rnd();
            for (uint32_t k = 0; k < dw; ++k) {
                uint32_t v = rnd();
                if (dw == 1 && v == BB_P - a.den.shift[0]) v = 1u;
                if (zero) v = BB_P - a.den.shift[k];
                den[(dw * b + k) * stride + i] = v;
            }
        }
    if (dw == 1) {
        const uint32_t z[4] = {BB_P - a.den.shift[0], 0u, 0u, 0u};
        a.den_inv = ext_shift_host(z);
    }
    ExtAccumSeeds in{};
    std::vector<uint32_t> init(4 * batch), want(stride * 4 * batch, SLACK), want_tot(8 * batch, 0u);
    for (uint32_t b = 0; b < batch; ++b) {
        E4 acc = {{OP == (int)SCAN_PRODUCT ? 1u : 0u, 0u, 0u, 0u}};
        if (b) acc = E4{{rnd_nonzero(), rnd(), rnd(), rnd()}};
        for (int k = 0; k < 4; ++k) { init[4 * b + k] = acc.c[k]; in.v[b][k] = OP == (int)SCAN_PRODUCT ? to_mont_host(acc.c[k]) : acc.c[k]; }
        uint32_t zeros = 0;
        for (size_t i = 0; i < n; ++i) {
            for (int k = 0; k < 4; ++k) want[(4 * b + k) * stride + i] = acc.c[k];
            const E4 d = operand_at(a.den, b, i);
            zeros += is_zero(d);
            acc = e_op<OP>(acc, e_mul(operand_at(a.num, b, i), e_inv(d)));
        }
        for (int k = 0; k < 4; ++k) want_tot[8 * b + k] = acc.c[k];
        want_tot[8 * b + 4] = zeros;
    }
    if (print_records) {
        std::printf("CASE ACCUM %d %zu %u %u %u\nINIT", OP, n, batch, nw, dw);
        for (uint32_t v : init) std::printf(" %u", v);
        std::printf("\nNSHIFT %u %u %u %u\nDSHIFT %u %u %u %u\n", a.num.shift[0], a.num.shift[1], a.num.shift[2], a.num.shift[3], a.den.shift[0], a.den.shift[1],
                    a.den.shift[2], a.den.shift[3]);
    }
    for (uint32_t b = 0; b < batch; ++b) {
        for (uint32_t k = 0; k < nw; ++k) print_words("NUM", b, (int)k, &num[(nw * b + k) * stride], n);
        for (uint32_t k = 0; k < dw; ++k) print_words("DEN", b, (int)k, &den[(dw * b + k) * stride], n);
        for (uint32_t k = 0; k < 4; ++k) print_words("WANT", b, (int)k, &want[(4 * b + k) * stride], n);
        print_words("WTOT", b, 0, &want_tot[8 * b], 8);
    }
    a.out = inplace == 1 ? num.data() : inplace == 2 ? den.data() : out.data();
    a.out_stride = stride;
    a.n = n;
    a.ntiles = (uint32_t)((n + EXT_ACCUM_TILE - 1) / EXT_ACCUM_TILE);
    a.single = a.ntiles == 1;
    std::vector<uint32_t> tiles((size_t)EXT_ACCUM_TILE_WORDS * a.ntiles * batch, SLACK), totals(8 * batch, SLACK);
    a.tiles = tiles.data();
    a.totals = totals.data();
    const char* inst = OP == (int)SCAN_PRODUCT ? "<product>" : "<sum>";
    if (a.single) {
        if (!wanted("ext_accum_apply_kernel")) return;
        sim_launch("ext_accum_apply_kernel", inst, dim3(1, batch), EXT_ACCUM_THREADS, [&] { ext_accum_apply_kernel<OP>(a, in); });
    } else {
        sim_launch("ext_accum_aggregate_kernel", inst, dim3(a.ntiles, batch), EXT_ACCUM_THREADS, [&] { ext_accum_aggregate_kernel<OP>(a); });
        sim_launch("ext_accum_prefix_kernel", inst, dim3(batch), EXT_ACCUM_THREADS, [&] { ext_accum_prefix_kernel<OP>(a, in); });
        sim_launch("ext_accum_apply_kernel", inst, dim3(a.ntiles, batch), EXT_ACCUM_THREADS, [&] { ext_accum_apply_kernel<OP>(a, in); });
    }
    size_t bad = 0;
    for (size_t w = 0; w < want.size(); ++w) bad += a.out[w] != want[w];   // the words between n and the stride keep their value
    CHECK(bad == 0, "ext accum op=%d n=%zu batch=%u widths=(%u,%u): %zu words differ from the model", OP, n, batch, nw, dw, bad);
    CHECK(totals == want_tot, "ext accum op=%d n=%zu batch=%u widths=(%u,%u): totals / zero counts differ", OP, n, batch, nw, dw);
}

// step 2 alone on more aggregates than one round takes (EXT_ACCUM_TILE + 5 of them would need 2^20 elements through steps 1 and 3)
template <int OP>
static void run_prefix(uint32_t ntiles, uint32_t batch) {
    sm_state = 0x9EF7ull + ntiles + OP;
    ExtAccumArgs a{};
    a.ntiles = ntiles;
    const size_t per = (size_t)EXT_ACCUM_TILE_WORDS * ntiles;
    std::vector<uint32_t> tiles(per * batch), plain(per * batch), want(per * batch), want_plain(per * batch), totals(8 * batch, SLACK), want_tot(8 * batch, 0u), init(4 * batch);
    ExtAccumSeeds in{};
    for (uint32_t b = 0; b < batch; ++b) {
        E4 acc = {{rnd_nonzero(), rnd(), rnd(), rnd()}};
        for (int k = 0; k < 4; ++k) { init[4 * b + k] = acc.c[k]; in.v[b][k] = OP == (int)SCAN_PRODUCT ? to_mont_host(acc.c[k]) : acc.c[k]; }
        uint32_t zeros = 0;
        for (uint32_t t = 0; t < ntiles; ++t) {
            const E4 v = {{rnd(), rnd(), rnd_nonzero(), rnd()}};
            const uint32_t z = (uint32_t)(splitmix() % 5);
            const E4 vf = OP == (int)SCAN_PRODUCT ? e_to_mont(v) : v, af = OP == (int)SCAN_PRODUCT ? e_to_mont(acc) : acc;   // the form the op scans
            for (int k = 0; k < 4; ++k) {
                plain[per * b + (size_t)k * ntiles + t] = v.c[k];
                tiles[per * b + (size_t)k * ntiles + t] = vf.c[k];
                want_plain[per * b + (size_t)k * ntiles + t] = acc.c[k];
                want[per * b + (size_t)k * ntiles + t] = af.c[k];
            }
            plain[per * b + 4 * (size_t)ntiles + t] = tiles[per * b + 4 * (size_t)ntiles + t] = z;
            want_plain[per * b + 4 * (size_t)ntiles + t] = want[per * b + 4 * (size_t)ntiles + t] = z;
            acc = e_op<OP>(acc, v);
            zeros += z;
        }
        for (int k = 0; k < 4; ++k) want_tot[8 * b + k] = acc.c[k];
        want_tot[8 * b + 4] = zeros;
    }
    if (print_records) {
        std::printf("CASE PREFIX %d %u %u\nINIT", OP, ntiles, batch);
        for (uint32_t v : init) std::printf(" %u", v);
        std::printf("\n");
    }
    for (uint32_t b = 0; b < batch; ++b) {
        for (int k = 0; k < 5; ++k) print_words("AGG", b, k, &plain[per * b + (size_t)k * ntiles], ntiles);
        for (int k = 0; k < 4; ++k) print_words("WANT", b, k, &want_plain[per * b + (size_t)k * ntiles], ntiles);
        print_words("WTOT", b, 0, &want_tot[8 * b], 8);
    }
    a.tiles = tiles.data();
    a.totals = totals.data();
    sim_launch("ext_accum_prefix_kernel", OP == (int)SCAN_PRODUCT ? "<product>" : "<sum>", dim3(batch), EXT_ACCUM_THREADS, [&] { ext_accum_prefix_kernel<OP>(a, in); });
    CHECK(tiles == want, "ext_accum_prefix_kernel op=%d ntiles=%u: prefixes differ from the model", OP, ntiles);
    CHECK(totals == want_tot, "ext_accum_prefix_kernel op=%d ntiles=%u: totals differ", OP, ntiles);
}

static void run_invert(size_t count, bool in_place) {
    sm_state = 0x1A7Eull + count;
    const size_t stride = count + 1;
    std::vector<uint32_t> in(4 * stride, SLACK), out(4 * stride, SLACK), want(4 * stride, SLACK);
    uint32_t want_zeros = 0, zeros = 0;
    for (size_t i = 0; i < count; ++i) {
        E4 v = {{rnd(), rnd(), rnd(), rnd()}};
        if (i % 3 == 1) v.c[i % 4] = v.c[(i + 1) % 4] = 0u;
        if (i % 61 == 5 || i == count - 1) v = E4{{0u, 0u, 0u, 0u}};
        want_zeros += is_zero(v);
        const E4 r = e_inv(v);
        for (int k = 0; k < 4; ++k) { in[k * stride + i] = v.c[k]; want[k * stride + i] = r.c[k]; }
    }
    if (print_records) std::printf("CASE INVERT %zu\n", count);
    for (int k = 0; k < 4; ++k) print_words("IN", 0, k, &in[k * stride], count);
    for (int k = 0; k < 4; ++k) print_words("WANT", 0, k, &want[k * stride], count);
    if (print_records) std::printf("WZEROS %u\n", want_zeros);
    uint32_t* dst = in_place ? in.data() : out.data();
    sim_launch("ext_invert_columns_kernel", "", dim3((unsigned)((count + EXT_ACCUM_TILE - 1) / EXT_ACCUM_TILE)), EXT_ACCUM_THREADS,
               [&] { ext_invert_columns_kernel(in.data(), stride, dst, stride, count, &zeros); });
    size_t bad = 0;
    for (size_t w = 0; w < want.size(); ++w) bad += dst[w] != want[w];
    CHECK(bad == 0, "ext_invert_columns_kernel count=%zu in_place=%d: %zu words differ from the model", count, (int)in_place, bad);
    CHECK(zeros == want_zeros, "ext_invert_columns_kernel count=%zu: %u zeros counted, %u present", count, zeros, want_zeros);
}

static void run_all_cases() {
    if (wanted("ext_accum_aggregate_kernel") || wanted("ext_accum_prefix_kernel") || wanted("ext_accum_apply_kernel")) {
        run_accum<SCAN_SUM>(5, 2, 1, 1, 0);                                   // a single launch
        run_accum<SCAN_PRODUCT>(EXT_ACCUM_TILE, 2, 1, 1, 0);
        run_accum<SCAN_SUM>(EXT_ACCUM_TILE + 3, 2, 4, 4, 2);                  // two tiles, in place on the denominator
        run_accum<SCAN_PRODUCT>(2 * EXT_ACCUM_TILE + 1, 1, 4, 1, 1);          // three tiles, in place on the numerator
        run_accum<SCAN_PRODUCT>(EXT_ACCUM_TILE + 9, 1, 0, 4, 0);
        run_accum<SCAN_SUM>(EXT_ACCUM_TILE + 9, 1, 1, 0, 0);
        if (wanted("ext_accum_prefix_kernel")) {                              // more tiles than one prefix round
            run_prefix<SCAN_SUM>(2 * EXT_ACCUM_TILE + 5, 2);
            run_prefix<SCAN_PRODUCT>(EXT_ACCUM_TILE + 1, 2);
        }
    }
    if (wanted("ext_invert_columns_kernel")) {
        run_invert(5, false);
        run_invert(EXT_ACCUM_TILE + 3, true);
    }
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    hipsim::State& s = hipsim::st();
    bool drop = false;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--only") && i + 1 < argc) only = argv[++i];
        else if (!std::strcmp(argv[i], "--drop") && i + 1 < argc) {
            const char* colon = std::strrchr(argv[++i], ':');
            if (!colon) { std::printf("usage: --drop kernel:ordinal\n"); return 2; }
            only = std::string((const char*)argv[i], (const char*)colon);
            s.drop_kernel = only;
            s.drop_site = std::atoi(colon + 1);
            drop = true;
        } else { std::printf("usage: sim_scan_ext [--only kernel | --drop kernel:ordinal]\n"); return 2; }
    }
    for (int k = 0; k < hipsim::NUM_SCHEDULES; ++k) {
        s.sched = hipsim::schedule_of(k);
        const int before = failures;
        run_all_cases();
        print_records = false;
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
