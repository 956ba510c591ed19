// Runs the barrier-free __global__ functions of toyni_amd/csrc/toyni_hip.hip whose arithmetic text lives in that file and that no
// other CPU program runs -- fourstep_twiddle_kernel, slab_relayout_kernel (forward, and inverse through relayout_quad's lazy chain),
// domain_elements_kernel, deep_combine_kernel / _inline_kernel, deep_combine_ext_kernel / _inline_kernel, fri_fold_ext_kernel and
// fri_fold_ext_stream_kernel -- on the CPU on hip_sim.hpp, the way sim_kernels.cpp runs the kernels that have barriers.
//
// TEST INFRASTRUCTURE (tests/test_field_contracts.py).  Every word the kernels write is compared with the oracle (orc_bb_pow chains,
// orc_domain_elements, orc_fri_fold_ext) or, for the DEEP combinations, with the defining sum in host integers (bb_mul_host,
// ext_mul_host, the Ext inverse through the Frobenius norm).  The arguments are prepared as the entry points of toyni_hip.hip prepare
// them.  The kernels have no synchronisation site, so what they write does not depend on the schedule: one schedule runs (the
// simulator still checks that every TOYNI_UNIFORM value agrees across a wave).  Shapes: every grid-stride loop runs at least twice
// and every tail is non-empty.  Prints RAN kernel<instantiation> like its siblings, then ALL OK.
//
//   sim_pointwise                     every case
//   sim_pointwise --only K            the cases of kernel K alone
#include "hip_sim.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <set>

#define TOYNI_KERNEL_TEXT_ONLY
#include "toyni_hip.hip"
#include "../emu/contract_case.hpp"


alignas(16) uint32_t air_lds[4];   // named by the kernel section; no kernel that uses it runs here
// none of these kernels has a __shared__ array: one word keeps the section (and the linker's bounds of it) in existence
__attribute__((used, section("hipsim_lds"))) static uint32_t lds_anchor[1];

extern "C" {
extern uint32_t __start_hipsim_lds[], __stop_hipsim_lds[];
uint64_t orc_bb_mul(uint64_t, uint64_t);
uint64_t orc_bb_inverse(uint64_t);
uint64_t orc_bb_pow(uint64_t, uint64_t);
uint64_t orc_bb_root_of_unity(uint32_t);
void orc_fill_splitmix(uint64_t*, size_t, uint64_t);
int orc_domain_elements(uint64_t*, size_t, uint64_t);
int orc_fri_fold_ext(uint64_t*, const uint64_t*, size_t, const uint64_t*, const uint64_t*);
}
void hipsim::poison_shared() {
    for (uint32_t* p = __start_hipsim_lds; p < __stop_hipsim_lds; ++p) *p = 0xDEADBEEFu;
}

static int failures = 0;
static std::string only;
static std::set<std::string> instantiations;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class F>
static bool sim_launch(const char* name, const std::string& inst, dim3 grid, uint32_t block, F&& body) {
    instantiations.insert(std::string(name) + inst);
    const bool ok = hipsim::launch(name, inst, grid, block, body);
    if (!ok) ++failures;
    return ok;
}
static bool wanted(const char* tag) { return only.empty() || only == tag; }

static uint64_t sm_state = 0x90117715Eull;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t draw() {   // {0, 1, p - 1, random}
    const uint64_t k = splitmix();
    return k % 8 == 0 ? 0u : k % 8 == 1 ? 1u : k % 8 == 2 ? BB_P - 1u : (uint32_t)(splitmix() % BB_P);
}
template <class T> struct Aligned {   // `words` words behind a 16-byte boundary, `off` words past it
    T* store;
    T* p;
    Aligned(size_t words, size_t off = 0) {
        store = static_cast<T*>(::operator new((words + off) * sizeof(T), std::align_val_t(16)));
        p = store + off;
    }
    ~Aligned() { ::operator delete(store, std::align_val_t(16)); }
    Aligned(const Aligned&) = delete;
};

// ---- data[r][k] *= w_n^(+-(row0 + r) k) ----
static void run_fourstep(int log_n, uint32_t rows, uint32_t row_len, uint32_t row0, bool inverse, uint32_t grid) {
    TOYNI_CONTRACT_TAG("fourstep_twiddle log_n=%d rows=%u row_len=%u row0=%u inverse=%d", log_n, rows, row_len, row0, (int)inverse);
    NttPlan plan;
    if (!build_plan(log_n, plan)) { CHECK(false, "plan %d", log_n); return; }
    const uint64_t total = (uint64_t)rows * row_len;
    std::vector<uint32_t> data(total), in(total);
    for (auto& v : in) v = draw();
    data = in;
    const uint32_t* t = (inverse ? plan.inv : plan.fwd).data();
    uint32_t log_len = 0;
    while ((1u << log_len) < row_len) ++log_len;
    sim_launch("fourstep_twiddle_kernel", inverse ? "<inverse>" : "<forward>", dim3(grid), 256,
               [&] { fourstep_twiddle_kernel(data.data(), total, log_len, row0, t + plan.dom_lo_off, t + plan.dom_hi_off, plan.dom_lowbits); });
    CHECK((uint64_t)grid * 256 * 2 <= total && total % ((uint64_t)grid * 256), "fourstep: the loop must run twice and end ragged");
    uint64_t w = orc_bb_root_of_unity((uint32_t)log_n);
    if (inverse) w = orc_bb_inverse(w);
    size_t bad = 0;
    for (uint32_t r = 0; r < rows; ++r)
        for (uint32_t k = 0; k < row_len; ++k)
            bad += data[(size_t)r * row_len + k] != (uint32_t)orc_bb_mul(in[(size_t)r * row_len + k], orc_bb_pow(w, (uint64_t)(row0 + r) * k));
    CHECK(bad == 0, "fourstep_twiddle_kernel inverse=%d: %zu of %llu words differ from the oracle", (int)inverse, bad, (unsigned long long)total);
}

// ---- the relayout around the exchange of a multi-device transform ----
static void run_relayout(int log_n, uint32_t rows_local, uint32_t row0, uint32_t parts, bool inverse, uint32_t grid, uint32_t block, bool saturated) {
    TOYNI_CONTRACT_TAG("slab_relayout log_n=%d rows=%u row0=%u parts=%u inverse=%d sat=%d", log_n, rows_local, row0, parts, (int)inverse, (int)saturated);
    NttPlan plan;
    if (!build_plan(log_n, plan) || plan.npasses < 2) { CHECK(false, "plan %d", log_n); return; }
    const uint64_t n = 1ull << log_n, m1 = 1ull << plan.pass[0].log_m, s1 = n / m1, W = s1 / parts;
    CHECK(W >= 32 && row0 + rows_local <= m1, "relayout shape");
    const uint64_t words = (uint64_t)rows_local * s1, quads = words / 4, stride = (uint64_t)grid * block;
    Aligned<uint32_t> in(words), out(words);
    for (uint64_t i = 0; i < words; ++i) { in.p[i] = saturated ? BB_P - 1u : draw(); out.p[i] = 0xCDCDCDCDu; }
    RelayoutArgs a{};
    a.in = in.p;
    a.out = out.p;
    auto lg = [](uint64_t v) { uint32_t l = 0; while ((1ull << l) < v) ++l; return l; };
    a.log_rows = lg(rows_local);
    a.log_parts = lg(parts);
    a.log_w = lg(W);
    a.inverse = inverse ? 1u : 0u;
    a.row0 = row0;
    a.lo = plan.inv.data() + plan.dom_lo_off;
    a.hi = plan.inv.data() + plan.dom_hi_off;
    a.lowbits = plan.dom_lowbits;
    char inst[96];
    std::snprintf(inst, sizeof inst, "<%s,%s>", inverse ? "inverse" : "forward", quads > 4 * stride ? "four-in-flight+tail" : "tail-only");
    sim_launch("slab_relayout_kernel", inst, dim3(grid), block, [&] { slab_relayout_kernel(a, quads); });
    // the four-in-flight loop takes 4 * stride quads a round: above 8 * stride it runs twice; what is left must not be a whole round
    CHECK(quads % (4 * stride) != 0 && (quads < 4 * stride ? quads > stride : quads > 8 * stride), "relayout: loops and tails, quads=%llu stride=%llu",
          (unsigned long long)quads, (unsigned long long)stride);
    const uint64_t winv = orc_bb_inverse(orc_bb_root_of_unity((uint32_t)log_n));
    size_t bad = 0;
    for (uint64_t r = 0; r < rows_local; ++r)
        for (uint64_t g = 0; g < parts; ++g)
            for (uint64_t w = 0; w < W; ++w) {
                const uint64_t pieces = (g * rows_local + r) * W + w, rowwise = (r * parts + g) * W + w;   // [parts][rows][W], [rows][parts][W]
                if (!inverse) bad += out.p[rowwise] != in.p[pieces];
                else bad += out.p[pieces] != (uint32_t)orc_bb_mul(in.p[rowwise], orc_bb_pow(winv, (uint64_t)(row0 + r) * (g * W + w)));
            }
    CHECK(bad == 0, "slab_relayout_kernel %s: %zu of %llu words differ from the oracle", inst, bad, (unsigned long long)words);
}

static void run_domain_elements(int log_n, uint64_t m, uint32_t shift, uint32_t grid) {
    TOYNI_CONTRACT_TAG("domain_elements log_n=%d m=%llu shift=%u", log_n, (unsigned long long)m, shift);
    NttPlan plan;
    if (!build_plan(log_n, plan)) { CHECK(false, "plan %d", log_n); return; }
    int log_m = 0;
    while ((1ull << log_m) < m) ++log_m;
    std::vector<uint32_t> out(m, 0xCDCDCDCDu);
    std::vector<uint64_t> want(m);
    orc_domain_elements(want.data(), m, shift);
    sim_launch("domain_elements_kernel", "", dim3(grid), 256, [&] { domain_elements_kernel(out.data(), m, shift, sub_domain(plan, plan.fwd.data(), log_n - log_m)); });
    CHECK((uint64_t)grid * 256 * 2 <= m, "domain_elements: the loop must run twice");
    size_t bad = 0;
    for (uint64_t i = 0; i < m; ++i) bad += out[i] != (uint32_t)want[i];
    CHECK(bad == 0, "domain_elements_kernel m=%llu shift=%u: %zu words differ from the oracle", (unsigned long long)m, shift, bad);
}

// ---- Ext in host integers ----
struct E4 { uint32_t c[4]; };
static E4 e_mul(const E4& a, const E4& b) { E4 r; ext_mul_host(a.c, b.c, r.c); return r; }
static E4 e_inv(const E4& a) {   // a^p a^(p^2) a^(p^3) / N(a); 0 for 0
    if (!(a.c[0] | a.c[1] | a.c[2] | a.c[3])) return a;
    E4 f1, f2, f3;
    ext_pow_host(a.c, BB_P, f1.c);
    ext_pow_host(f1.c, BB_P, f2.c);
    ext_pow_host(f2.c, BB_P, f3.c);
    const E4 adj = e_mul(e_mul(f1, f2), f3), nrm = e_mul(a, adj);
    CHECK(!(nrm.c[1] | nrm.c[2] | nrm.c[3]), "the norm of the host model left the base field");
    const uint32_t ni = bb_inv_host(nrm.c[0]);
    E4 r;
    for (int k = 0; k < 4; ++k) r.c[k] = bb_mul_host(adj.c[k], ni);
    return r;
}
static uint32_t h_sub(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + BB_P - b) % BB_P); }
static uint32_t h_add(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + b) % BB_P); }

struct DeepShape { int log_N, log_blowup; uint32_t width, nterms; bool table, accumulate, saturated; uint32_t out_off; long z_at; };

// d_i = sum_t alpha_t (M(column_t, (i + rotation_t B) mod N) - value_t) / (x_i - z), 0 where x_i = z
static void run_deep(const DeepShape& s) {
    TOYNI_CONTRACT_TAG("deep_combine log_N=%d nterms=%u table=%d accumulate=%d sat=%d", s.log_N, s.nterms, (int)s.table, (int)s.accumulate, (int)s.saturated);
    NttPlan plan;
    if (!build_plan(s.log_N, plan)) { CHECK(false, "plan"); return; }
    const uint64_t N = 1ull << s.log_N, rows = N >> s.log_blowup, col_stride = N + 4;
    const uint32_t shift = 7u, wN = bb_root_of_unity_host((uint32_t)s.log_N);
    const uint32_t z = s.z_at >= 0 ? bb_mul_host(shift, bb_pow_host(wN, (uint64_t)s.z_at)) : s.saturated ? SAT_X : (uint32_t)(splitmix() % BB_P);
    struct Term { uint32_t column, rotation, alpha, value; };
    std::vector<Term> terms(s.nterms);
    for (uint32_t t = 0; t < s.nterms; ++t)
        terms[t] = Term{(uint32_t)(splitmix() % s.width), (t % 3 == 2) ? (uint32_t)(rows - 1) : (uint32_t)(splitmix() % rows), s.saturated ? SAT_X : draw(),
                        s.saturated ? SAT_X : draw()};
    Aligned<uint32_t> m((size_t)s.width * col_stride), out(N, s.out_off), prev(N);
    for (size_t k = 0; k < (size_t)s.width * col_stride; ++k) m.p[k] = k % col_stride < N ? (s.saturated ? BB_P - 1u : draw()) : 0xFFFFFFF0u;
    for (uint64_t i = 0; i < N; ++i) out.p[i] = prev.p[i] = s.accumulate ? (s.saturated ? BB_P - 1u : draw()) : 0xCDCDCDCDu;
    // what toyni_deep_combine_device prepares
    std::vector<DeepTerm> table(s.nterms);
    uint32_t claim = 0;
    for (uint32_t t = 0; t < s.nterms; ++t) {
        table[t] = DeepTerm{terms[t].column, (uint32_t)((uint64_t)terms[t].rotation << s.log_blowup), to_mont_host(terms[t].alpha), 0u};
        claim = h_add(claim, bb_mul_host(terms[t].alpha, terms[t].value));
    }
    std::stable_sort(table.begin(), table.end(), [](const DeepTerm& x, const DeepTerm& y) { return x.column != y.column ? x.column < y.column : x.rot < y.rot; });
    DeepCombineArgs a{};
    a.values = m.p;
    a.out = out.p;
    a.col_stride = col_stride;
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.log_N = (uint32_t)s.log_N;
    a.nterms = s.nterms;
    a.wNR = to_mont_host(wN);
    a.zR = to_mont_host(z);
    a.claim = claim;
    a.accumulate = s.accumulate ? 1u : 0u;
    char inst[64];
    std::snprintf(inst, sizeof inst, "<nterms=%u,%s>", s.nterms, s.log_N >= 3 ? "groups" : "points");
    if (s.table) {
        sim_launch("deep_combine_kernel", inst, dim3(1), 256, [&] { deep_combine_kernel(a, table.data()); });
    } else {
        DeepInlineTerms in{};
        for (uint32_t t = 0; t < s.nterms; ++t) in.t[t] = table[t];
        sim_launch("deep_combine_inline_kernel", inst, dim3(1), 256, [&] { deep_combine_inline_kernel(a, in); });
    }
    size_t bad = 0;
    uint32_t x = shift;
    for (uint64_t i = 0; i < N; ++i, x = bb_mul_host(x, wN)) {
        uint32_t num = 0;
        for (const Term& t : terms) num = h_add(num, bb_mul_host(t.alpha, h_sub(m.p[t.column * col_stride + ((i + ((uint64_t)t.rotation << s.log_blowup)) & (N - 1))], t.value)));
        uint32_t want = x == z ? 0u : bb_mul_host(num, bb_inv_host(h_sub(x, z)));
        if (s.accumulate) want = h_add(want, prev.p[i]);
        bad += out.p[i] != want;
    }
    CHECK(bad == 0, "deep_combine%s_kernel %s accumulate=%d sat=%d: %zu of %llu words differ from the integer sum", s.table ? "" : "_inline", inst, (int)s.accumulate,
          (int)s.saturated, bad, (unsigned long long)N);
}

static void run_deep_ext(const DeepShape& s) {
    TOYNI_CONTRACT_TAG("deep_combine_ext log_N=%d nterms=%u table=%d accumulate=%d sat=%d", s.log_N, s.nterms, (int)s.table, (int)s.accumulate, (int)s.saturated);
    NttPlan plan;
    if (!build_plan(s.log_N, plan)) { CHECK(false, "plan"); return; }
    const uint64_t N = 1ull << s.log_N, rows = N >> s.log_blowup, col_stride = N + 4;
    const uint32_t shift = 7u, wN = bb_root_of_unity_host((uint32_t)s.log_N);
    E4 z{{0u, 0u, 0u, 0u}};
    if (s.z_at >= 0) z.c[0] = bb_mul_host(shift, bb_pow_host(wN, (uint64_t)s.z_at));
    else for (int k = 0; k < 4; ++k) z.c[k] = s.saturated ? SAT_X : (uint32_t)(splitmix() % BB_P);
    struct Term { uint32_t column, rotation; E4 alpha, value; };
    std::vector<Term> terms(s.nterms);
    for (uint32_t t = 0; t < s.nterms; ++t) {
        terms[t].column = (uint32_t)(splitmix() % s.width);
        terms[t].rotation = (t % 3 == 2) ? (uint32_t)(rows - 1) : (uint32_t)(splitmix() % rows);
        for (int k = 0; k < 4; ++k) { terms[t].alpha.c[k] = s.saturated ? SAT_X : draw(); terms[t].value.c[k] = s.saturated ? SAT_X : draw(); }
    }
    Aligned<uint32_t> m((size_t)s.width * col_stride), out(4 * N), prev(4 * N);
    for (size_t k = 0; k < (size_t)s.width * col_stride; ++k) m.p[k] = k % col_stride < N ? (s.saturated ? BB_P - 1u : draw()) : 0xFFFFFFF0u;
    for (uint64_t i = 0; i < 4 * N; ++i) out.p[i] = prev.p[i] = s.accumulate ? (s.saturated ? BB_P - 1u : draw()) : 0xCDCDCDCDu;
    // what toyni_deep_combine_ext_device prepares
    std::vector<DeepExtTerm> table(s.nterms);
    DeepExtArgs a{};
    for (uint32_t t = 0; t < s.nterms; ++t) {
        table[t] = DeepExtTerm{};
        table[t].column = terms[t].column;
        table[t].rot = (uint32_t)((uint64_t)terms[t].rotation << s.log_blowup);
        const E4 av = e_mul(terms[t].alpha, terms[t].value);
        for (int k = 0; k < 4; ++k) { table[t].alphaR[k] = to_mont_host(terms[t].alpha.c[k]); a.claim[k] = h_add(a.claim[k], av.c[k]); }
    }
    std::stable_sort(table.begin(), table.end(), [](const DeepExtTerm& x, const DeepExtTerm& y) { return x.column != y.column ? x.column < y.column : x.rot < y.rot; });
    a.values = m.p;
    a.out = out.p;
    a.col_stride = col_stride;
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.log_N = (uint32_t)s.log_N;
    a.nterms = s.nterms;
    a.wNR = to_mont_host(wN);
    a.accumulate = s.accumulate ? 1u : 0u;
    a.shift = ext_shift_host(z.c);
    char inst[64];
    std::snprintf(inst, sizeof inst, "<nterms=%u,%s>", s.nterms, s.log_N >= 2 ? "groups" : "points");
    if (s.table) {
        sim_launch("deep_combine_ext_kernel", inst, dim3(1), 256, [&] { deep_combine_ext_kernel(a, table.data()); });
    } else {
        DeepExtInlineTerms in{};
        for (uint32_t t = 0; t < s.nterms; ++t) in.t[t] = table[t];
        sim_launch("deep_combine_ext_inline_kernel", inst, dim3(1), 256, [&] { deep_combine_ext_inline_kernel(a, in); });
    }
    size_t bad = 0;
    uint32_t x = shift;
    for (uint64_t i = 0; i < N; ++i, x = bb_mul_host(x, wN)) {
        E4 num{{0u, 0u, 0u, 0u}};
        for (const Term& t : terms) {
            E4 d = t.value;
            for (int k = 0; k < 4; ++k) d.c[k] = h_sub(k ? 0u : m.p[t.column * col_stride + ((i + ((uint64_t)t.rotation << s.log_blowup)) & (N - 1))], d.c[k]);
            const E4 p = e_mul(t.alpha, d);
            for (int k = 0; k < 4; ++k) num.c[k] = h_add(num.c[k], p.c[k]);
        }
        E4 den = z;
        for (int k = 0; k < 4; ++k) den.c[k] = h_sub(k ? 0u : x, den.c[k]);
        const E4 want = e_mul(num, e_inv(den));
        for (int k = 0; k < 4; ++k) bad += out.p[4 * i + k] != (s.accumulate ? h_add(want.c[k], prev.p[4 * i + k]) : want.c[k]);
    }
    CHECK(bad == 0, "deep_combine_ext%s_kernel %s accumulate=%d sat=%d: %zu of %llu words differ from the integer sum", s.table ? "" : "_inline", inst,
          (int)s.accumulate, (int)s.saturated, bad, (unsigned long long)(4 * N));
}

// ---- the Ext fold on structured points: both kernel shapes ----
static void run_fold_ext(int log_n, uint64_t m, bool stream, uint32_t grid, bool saturated) {
    TOYNI_CONTRACT_TAG("fri_fold_ext log_n=%d m=%llu stream=%d sat=%d", log_n, (unsigned long long)m, (int)stream, (int)saturated);
    NttPlan plan;
    if (!build_plan(log_n, plan)) { CHECK(false, "plan %d", log_n); return; }
    int log_m = 0;
    while ((1ull << log_m) < m) ++log_m;
    const uint64_t half = m / 2;
    const uint32_t x0 = saturated ? SAT_X : 7u;
    std::vector<uint64_t> evals(4 * m), xs(m), want(4 * half);
    orc_fill_splitmix(evals.data(), evals.size(), 0xF01DE47ull + m);
    if (saturated)
        for (uint64_t i = 0; i < 4 * m; ++i) evals[i] = i < 4 * half ? BB_P - 1u : ((i / 4) & 1 ? BB_P - 1u : 0u);   // a - b saturated at every other point
    orc_domain_elements(xs.data(), m, x0);
    const uint64_t beta[4] = {saturated ? SAT_X : 123456789ull, saturated ? SAT_X : 987654321ull, saturated ? SAT_X : 0ull, saturated ? SAT_X : BB_P - 1ull};
    orc_fri_fold_ext(want.data(), evals.data(), m, xs.data(), beta);
    Aligned<uint32_t> e32(4 * m), out(4 * half);
    for (uint64_t i = 0; i < 4 * m; ++i) e32.p[i] = (uint32_t)evals[i];
    for (uint64_t i = 0; i < 4 * half; ++i) out.p[i] = 0xCDCDCDCDu;
    // what toyni_fri_fold_ext_device prepares
    FoldExtArgs fa{};
    uint32_t bh[4];
    for (int k = 0; k < 4; ++k) bh[k] = bb_mul_host((uint32_t)beta[k], BB_HALF);
    fa.beta_half = ext_factor_host(bh);
    fa.base.evals = e32.p;
    fa.base.out = out.p;
    fa.base.dom = sub_domain(plan, plan.inv.data(), log_n - log_m);
    fa.base.coef = to_mont_host(bb_inv_host(x0));
    fa.base.half = half;
    if (stream) {
        const uint64_t chunks = (half + 2047) / 2048;
        sim_launch("fri_fold_ext_stream_kernel", chunks > grid ? "<NT=true,T=1024,U=2,chunks>grid>" : "<NT=true,T=1024,U=2,ragged-chunk>", dim3(grid), 1024,
                   [&] { fri_fold_ext_stream_kernel<true, 1024, 2>(fa); });
    } else {
        sim_launch("fri_fold_ext_kernel", "", dim3(grid), 256, [&] { fri_fold_ext_kernel(fa); });
        CHECK((uint64_t)grid * 256 * 2 <= half, "fri_fold_ext: the loop must run twice");
    }
    size_t bad = 0;
    for (uint64_t i = 0; i < 4 * half; ++i) bad += out.p[i] != (uint32_t)want[i];
    CHECK(bad == 0, "fri_fold_ext%s_kernel m=%llu sat=%d: %zu of %llu words differ from the oracle", stream ? "_stream" : "", (unsigned long long)m, (int)saturated, bad,
          (unsigned long long)(4 * half));
}

static void run_all_cases() {
    if (wanted("fourstep_twiddle_kernel"))
        for (bool inverse : {false, true}) run_fourstep(12, 10, 64, 3, inverse, 1);               // 640 words under a stride of 256: three rounds, the last ragged
    if (wanted("slab_relayout_kernel"))
        for (bool inverse : {false, true}) {
            // 2^14 = 128 x 128: rows of 128 words in two pieces of 64.  Stride 192 quads: 2048 quads = two four-in-flight rounds and up
            // to three tail rounds; 256 quads = the tail alone, twice for the first 64 threads
            run_relayout(14, 64, 64, 2, inverse, 3, 64, false);
            run_relayout(14, 8, 5, 2, inverse, 3, 64, false);
            run_relayout(14, 8, 120, 4, inverse, 3, 64, true);
        }
    if (wanted("domain_elements_kernel")) {
        run_domain_elements(12, 1024, 7, 2);
        run_domain_elements(12, 4096, SAT_X, 3);
    }
    for (bool ext : {false, true}) {
        const char* names[2] = {ext ? "deep_combine_ext_inline_kernel" : "deep_combine_inline_kernel", ext ? "deep_combine_ext_kernel" : "deep_combine_kernel"};
        for (int table = 0; table < 2; ++table) {
            if (!wanted(names[table])) continue;
            uint32_t k = 0;
            for (uint32_t nterms : {3u, 4u, 5u, 64u, 65u}) {
                if (!table && nterms > 64) continue;                                              // the inline table holds 64 entries
                for (bool saturated : {false, true}) {
                    ++k;
                    // 2^6 points, blow-up 4, width 8; z on the coset (first point of the last group) in one case of four; the base
                    // kernel's word stores behind an output 4 bytes off alignment in one of three
                    const DeepShape s{6, 2, 8, nterms, table != 0, (k & 1) != 0, saturated, (!ext && k % 3 == 0) ? 1u : 0u, (!saturated && k % 4 == 1) ? 56 : -1};
                    if (ext) run_deep_ext(s); else run_deep(s);
                }
            }
            const DeepShape points{1, 0, 2, 5, table != 0, true, false, 0u, 1};                // below a group: single points, z on the coset
            if (ext) run_deep_ext(points); else run_deep(points);
        }
    }
    if (wanted("fri_fold_ext_kernel")) {
        run_fold_ext(12, 1024, false, 1, false);                                                  // 512 outputs under a stride of 256
        run_fold_ext(12, 2048, false, 2, true);
    }
    if (wanted("fri_fold_ext_stream_kernel")) {
        run_fold_ext(13, 8192, true, 1, false);                                                   // two chunks of 2048 outputs, one workgroup
        run_fold_ext(13, 2048, true, 2, false);                                                   // half a chunk: the second load pair of every lane is masked; an idle workgroup
        run_fold_ext(13, 8192, true, 1, true);
    }
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    hipsim::State& s = hipsim::st();
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--only") && i + 1 < argc) only = argv[++i];
        else { std::printf("usage: sim_pointwise [--only kernel]\n"); return 2; }
    }
    s.sched = hipsim::schedule_of(0);
    run_all_cases();
    std::printf("SCHEDULE %s failures=%d\n", hipsim::schedule_name(0).c_str(), failures);
    for (const std::string& inst : instantiations) std::printf("RAN %s\n", inst.c_str());
    for (auto& kv : s.kernels) CHECK(kv.second.sites.empty(), "%s reached a synchronisation site: it belongs in sim_kernels", kv.first.c_str());
    std::printf("launches=%llu fiber switches=%llu hard failures=%llu\n", s.launches, s.switches, s.hard_failures);
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "ALL OK", failures);
    return failures ? 1 : 0;
}
