// Runs the one-workgroup batch twins of include/toyni_hip.h 3r -- fri_tail_rounds_batch_kernel<false> and <true> and
// merkle_tail_batch_kernel of toyni_amd/csrc/toyni_hip.hip -- themselves on the CPU under the adversarial wave schedules of
// hip_sim.hpp, three proofs per launch (gridDim.x = 3: one workgroup per proof), the way sim_fri_tail.cpp runs the single kernels.
//
// TEST INFRASTRUCTURE (tests/test_sim_fri_tail_batch.py).  What a launch must leave for every proof -- every folded layer, every tree
// level, the betas and the transcript -- is computed here on the host by the model of sim_fri_tail.cpp, restated: the fold on plain
// residues, a byte-oriented SHA-256, the transcript as a byte vector (with the sticky status of 3l).  The proofs lie a stride apart
// with the strides larger than the extents; the gaps must keep their fill.  The three transcripts are 32, 55 and 1008 - 32 bytes long
// (the one-block / two-block seam of SHA-256 and the capacity edge); one more launch per kernel sets the status of the middle one,
// whose neighbours' bytes must not move.
// Cases: the rounds kernels, salted (the final layer unsalted), m = 2^10 -> 1, 2^6 -> 4, 2 -> 1; the Merkle tail at m = 512, 3, 1.
//
//   sim_fri_tail_batch                every case under all eight schedules; prints the instantiations and the sites, then ALL OK
//   sim_fri_tail_batch --only K       the cases of kernel K alone (fri_tail_rounds_batch_kernel_base | fri_tail_rounds_batch_kernel_ext |
//                                     merkle_tail_batch_kernel)
//   sim_fri_tail_batch --drop K:i     the cases of kernel K with its i-th synchronisation site switched off: DROP ... FAILS / SURVIVES
#include "hip_sim.hpp"

#include <cstdio>
#include <cstring>
#include <set>

#define TOYNI_KERNEL_TEXT_ONLY
#include "toyni_hip.hip"
#include "../emu/contract_case.hpp"

extern "C" {
extern uint32_t __start_hipsim_lds[] __attribute__((weak)), __stop_hipsim_lds[] __attribute__((weak));
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
static uint32_t h_add(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + b) % BB_P); }
static uint32_t h_sub(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + BB_P - b) % BB_P); }
static int ilog2_host(uint32_t v) { int l = 0; while ((1u << l) < v) ++l; return l; }

// ---- the host model (that of sim_fri_tail.cpp, restated) ----
typedef std::vector<uint8_t> Bytes;
static Bytes plain_sha256(const Bytes& msg) {   // FIPS 180-4 on bytes
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
        0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
        0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
        0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
        0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
        0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    Bytes m = msg;
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    const uint64_t bits = (uint64_t)msg.size() * 8;
    for (int i = 7; i >= 0; --i) m.push_back((uint8_t)(bits >> (8 * i)));
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
    for (size_t off = 0; off < m.size(); off += 64) {
        uint32_t w[64];
        for (int i = 0; i < 16; ++i) w[i] = (uint32_t)m[off + 4 * i] << 24 | (uint32_t)m[off + 4 * i + 1] << 16 | (uint32_t)m[off + 4 * i + 2] << 8 | m[off + 4 * i + 3];
        for (int i = 16; i < 64; ++i)
            w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
        uint32_t v[8];
        memcpy(v, h, sizeof v);
        for (int i = 0; i < 64; ++i) {
            const uint32_t t1 = v[7] + (rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) + K[i] + w[i];
            const uint32_t t2 = (rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
            for (int j = 7; j > 0; --j) v[j] = v[j - 1];
            v[4] += t1;
            v[0] = t1 + t2;
        }
        for (int j = 0; j < 8; ++j) h[j] += v[j];
    }
    Bytes out;
    for (int j = 0; j < 8; ++j) for (int i = 3; i >= 0; --i) out.push_back((uint8_t)(h[j] >> (8 * i)));
    return out;
}
static uint32_t model_squeeze(Bytes& state) {   // src/transcript.rs:34-40
    state = plain_sha256(state);
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = v << 8 | state[i];
    return (uint32_t)(v % BB_P);
}
// Ext = F_p[X] / (X^4 - 11), src/ext.rs
static void ext_mul_plain(const uint32_t a[4], const uint32_t b[4], uint32_t r[4]) {
    uint32_t t[7] = {};
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) t[i + j] = h_add(t[i + j], bb_mul_host(a[i], b[j]));
    for (int k = 0; k < 4; ++k) r[k] = k < 3 ? h_add(t[k], bb_mul_host(11u, t[k + 4])) : t[k];
}
// every level of the tree over `level` (leaf digests), appended to `all`; returns the root
static Bytes model_tree(std::vector<Bytes> level, std::vector<Bytes>& all) {
    for (;;) {
        for (const Bytes& d : level) all.push_back(d);
        if (level.size() == 1) return level[0];
        std::vector<Bytes> up;
        for (size_t i = 0; i < level.size(); i += 2) {
            Bytes node{0x01};
            node.insert(node.end(), level[i].begin(), level[i].end());
            const Bytes& r = i + 1 < level.size() ? level[i + 1] : level[i];
            node.insert(node.end(), r.begin(), r.end());
            up.push_back(plain_sha256(node));
        }
        level = up;
    }
}

constexpr uint32_t B = 3, FILL = 0xA5A5A5A5u;
static const uint32_t STATE_LEN[B] = {32, 55, TRANSCRIPT_CAPACITY - 32};

// status_at: the proof whose transcript starts with its status set (B: none)
template <bool EXT>
static void run_tail(uint32_t m0, uint32_t final_size, uint32_t status_at) {
    constexpr uint32_t W = EXT ? 4u : 1u, NSQ = W;
    const int log_n = 12;   // the context's domain is larger than the layer: the SubDomain view has a stride
    sm_state = 0xB71ull + m0 * 131ull + final_size * 7ull + W + 1000ull * status_at;
    NttPlan plan;
    if (!build_plan(log_n, plan)) { CHECK(false, "plan"); return; }
    const uint32_t x0 = 7;
    std::vector<uint32_t> sizes;
    for (uint32_t m = m0; m > final_size; m >>= 1) sizes.push_back(m >> 1);
    size_t words = 0, digests = 0, salted = 0;
    for (size_t k = 0; k < sizes.size(); ++k) { words += sizes[k] * W; digests += 2 * sizes[k] - 1; salted += k + 1 < sizes.size() ? sizes[k] : 0; }
    const size_t nbetas = NSQ * sizes.size();
    // strides larger than the extents: words, words, bytes (a multiple of 16), bytes (a multiple of 16), words
    const FriTailBatch st{(size_t)m0 * W + 4, words + 8, digests * 32 + 48, salted * 16 + 32, nbetas + 3};
    std::vector<uint32_t> layer0(B * st.cur_stride, FILL), out(B * st.out_stride, FILL), betas(B * st.beta_stride, FILL);
    std::vector<uint4> salts(B * st.salt_stride / 16);
    std::vector<uint8_t> levels(B * st.level_stride, 0xA5);
    for (uint4& s : salts) s = make_uint4((uint32_t)splitmix(), (uint32_t)splitmix(), (uint32_t)splitmix(), (uint32_t)splitmix());
    alignas(16) static TranscriptState tr[B];
    Bytes state[B];
    uint32_t status[B];
    for (uint32_t b = 0; b < B; ++b) {
        for (uint32_t i = 0; i < m0 * W; ++i) layer0[b * st.cur_stride + i] = i % 53 == 5 ? BB_P - 1u : (i % 97 == 1 ? 0u : rnd());
        memset(&tr[b], 0, sizeof tr[b]);
        memset(tr[b].bytes, 0x5A, sizeof tr[b].bytes);   // stale bytes beyond the state
        state[b].resize(STATE_LEN[b]);
        for (uint32_t i = 0; i < STATE_LEN[b]; ++i) state[b][i] = tr[b].bytes[i] = (uint8_t)splitmix();
        tr[b].len = STATE_LEN[b];
        tr[b].status = status[b] = b == status_at ? (uint32_t)TRANSCRIPT_E_RANGE : 0u;
    }
    const std::vector<uint32_t> layer0_before = layer0;
    // ---- the model, proof by proof ----
    std::vector<uint32_t> want_out[B], want_betas[B];
    std::vector<Bytes> want_levels[B];
    for (uint32_t b = 0; b < B; ++b) {
        std::vector<uint32_t> cur(layer0.begin() + b * st.cur_stride, layer0.begin() + b * st.cur_stride + m0 * W);
        const uint4* sl = salts.data() + b * st.salt_stride / 16;
        uint32_t x = x0;
        size_t soff = 0;
        for (size_t k = 0; k < sizes.size(); ++k) {
            const uint32_t half = sizes[k], m = 2 * half;
            uint32_t beta[4] = {};
            for (uint32_t q = 0; q < NSQ; ++q) want_betas[b].push_back(beta[q] = status[b] ? 0u : model_squeeze(state[b]));
            const uint32_t winv = bb_inv_host(bb_root_of_unity_host((uint32_t)ilog2_host(m)));
            std::vector<uint32_t> next(half * W);
            uint32_t xi_inv = bb_inv_host(x);
            for (uint32_t i = 0; i < half; ++i, xi_inv = bb_mul_host(xi_inv, winv)) {
                uint32_t avg[4], hd[4], prod[4];
                for (uint32_t c = 0; c < W; ++c) {
                    const uint32_t a = cur[i * W + c], e = cur[(i + half) * W + c];
                    avg[c] = bb_mul_host(h_add(a, e), BB_HALF);
                    hd[c] = bb_mul_host(bb_mul_host(h_sub(a, e), BB_HALF), xi_inv);
                }
                if (EXT) ext_mul_plain(hd, beta, prod);
                else prod[0] = bb_mul_host(hd[0], beta[0]);
                for (uint32_t c = 0; c < W; ++c) next[i * W + c] = h_add(avg[c], prod[c]);
            }
            const bool has_salt = k + 1 < sizes.size();
            std::vector<Bytes> level;
            for (uint32_t i = 0; i < half; ++i) {
                Bytes leaf{0x00};
                if (has_salt) {
                    const uint4 s = sl[soff + i];
                    for (uint32_t wd : {s.x, s.y, s.z, s.w}) for (int j = 0; j < 4; ++j) leaf.push_back((uint8_t)(wd >> (8 * j)));
                }
                for (uint32_t c = 0; c < W; ++c) for (int j = 0; j < 8; ++j) leaf.push_back(j < 4 ? (uint8_t)(next[i * W + c] >> (8 * j)) : 0);
                level.push_back(plain_sha256(leaf));
            }
            if (has_salt) soff += half;
            const Bytes root = model_tree(level, want_levels[b]);
            if (!status[b]) state[b].insert(state[b].end(), root.begin(), root.end());   // absorb the root
            want_out[b].insert(want_out[b].end(), next.begin(), next.end());
            cur = next;
            x = bb_mul_host(x, x);
        }
    }
    // ---- the launch: one workgroup per proof ----
    FriTailArgs a{};
    a.cur = layer0.data();
    a.out = out.data();
    a.levels = reinterpret_cast<Digest*>(levels.data());
    a.salts = salted ? salts.data() : nullptr;
    a.tr = tr;
    a.betas = betas.data();
    a.dom = sub_domain(plan, plan.inv.data(), log_n - ilog2_host(m0));
    a.m = m0;
    a.final_size = final_size;
    a.xinvR = to_mont_host(bb_inv_host(x0));
    a.half_r2 = to_mont_host(to_mont_host(BB_HALF));
    a.half11_r2 = to_mont_host(to_mont_host(bb_mul_host(BB_HALF, 11u)));
    const char* name = EXT ? "fri_tail_rounds_batch_kernel_ext" : "fri_tail_rounds_batch_kernel_base";
    sim_launch(name, "", dim3(B), MERKLE_TAIL_T, [&] { fri_tail_rounds_batch_kernel<EXT>(a, st); });
    for (uint32_t b = 0; b < B; ++b) {
        size_t bad = 0;
        for (size_t i = 0; i < st.out_stride; ++i) bad += out[b * st.out_stride + i] != (i < words ? want_out[b][i] : FILL);
        CHECK(bad == 0, "%s m=%u->%u proof %u: %zu layer words differ from the host model (or a gap was written)", name, m0, final_size, b, bad);
        bad = 0;
        const uint8_t* lv = levels.data() + b * st.level_stride;
        for (size_t i = 0; i < digests; ++i) bad += memcmp(lv + 32 * i, want_levels[b][i].data(), 32) != 0;
        for (size_t i = digests * 32; i < st.level_stride; ++i) bad += lv[i] != 0xA5;
        CHECK(bad == 0 && want_levels[b].size() == digests, "%s m=%u->%u proof %u: %zu digests differ from the host model", name, m0, final_size, b, bad);
        bad = 0;
        for (size_t i = 0; i < st.beta_stride; ++i) bad += betas[b * st.beta_stride + i] != (i < nbetas ? want_betas[b][i] : FILL);
        CHECK(bad == 0, "%s m=%u->%u proof %u: %zu betas differ", name, m0, final_size, b, bad);
        CHECK(tr[b].status == status[b] && tr[b].len == state[b].size() && !memcmp(tr[b].bytes, state[b].data(), state[b].size()),
              "%s m=%u->%u proof %u: the transcript differs (len %u, status %u)", name, m0, final_size, b, tr[b].len, tr[b].status);
        if (status[b]) CHECK(tr[b].len == STATE_LEN[b], "a transcript whose status is set stays as it is");
    }
    CHECK(layer0 == layer0_before, "layer 0 was written");
}

static void run_merkle_tail(uint32_t m) {
    sm_state = 0x7A11ull + m;
    const size_t at = 5;                                   // the level lies `at` digests into a proof's region
    size_t above = 0;
    for (uint32_t k = m; k > 1; k = (k + 1) / 2) above += (k + 1) / 2;
    const size_t stride = (at + m + above) * 32 + 48;
    std::vector<uint8_t> levels(B * stride, 0xA5);
    std::vector<Bytes> want[B];
    for (uint32_t b = 0; b < B; ++b) {
        std::vector<Bytes> level(m, Bytes(32));
        for (uint32_t i = 0; i < m; ++i)
            for (int j = 0; j < 32; ++j) levels[b * stride + (at + i) * 32 + j] = level[i][j] = (uint8_t)splitmix();
        model_tree(level, want[b]);
    }
    sim_launch("merkle_tail_batch_kernel", "", dim3(B), MERKLE_TAIL_T, [&] { merkle_tail_batch_kernel(levels.data(), stride, at, m); });
    for (uint32_t b = 0; b < B; ++b) {
        size_t bad = 0;
        const uint8_t* lv = levels.data() + b * stride;
        for (size_t i = 0; i < at * 32; ++i) bad += lv[i] != 0xA5;
        for (size_t i = 0; i < want[b].size(); ++i) bad += memcmp(lv + (at + i) * 32, want[b][i].data(), 32) != 0;
        for (size_t i = (at + m + above) * 32; i < stride; ++i) bad += lv[i] != 0xA5;
        CHECK(bad == 0 && want[b].size() == m + above, "merkle_tail_batch_kernel m=%u proof %u: %zu digests differ from the host model (or a gap was written)", m, b, bad);
    }
}

template <bool EXT>
static void rounds_cases() {
    run_tail<EXT>(1u << 10, 1, B);
    run_tail<EXT>(1u << 6, 4, B);
    run_tail<EXT>(2, 1, B);
    run_tail<EXT>(1u << 6, 4, 1);   // the middle transcript's status is set
}
static void run_all_cases() {
    if (wanted("fri_tail_rounds_batch_kernel_base")) rounds_cases<false>();
    if (wanted("fri_tail_rounds_batch_kernel_ext")) rounds_cases<true>();
    if (wanted("merkle_tail_batch_kernel")) { run_merkle_tail(512); run_merkle_tail(3); run_merkle_tail(1); }
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
        } else { std::printf("usage: sim_fri_tail_batch [--only kernel | --drop kernel:ordinal]\n"); return 2; }
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
