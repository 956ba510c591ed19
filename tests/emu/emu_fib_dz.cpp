// Steps the bodies of include/toyni_hip.h 3q (toyni_amd/csrc/fib_dz_kernels.hpp: the text the new kernels run) on the CPU.
// TEST INFRASTRUCTURE (tests/test_emu_fib_dz.py builds it under AddressSanitizer + UBSan; tests/test_field_contracts_fib_dz.py
// rebuilds it with tests/emu/field_contracts.hpp in front).  Every input and output lives in a heap block of exactly its size.
//
// Part 1 (argument `records` or `saturated`, no stdin): for z and the claimed values drawn from {0, p - 1, p, p + 1, 0xFFFFFFFF} (and a
// few random words) both records are compared with memcmp against what the HOST code of toyni_poly_eval_device and
// toyni_fib_deep_device builds for the reduced values, and printed for the test to judge against Python integers:
//   POLY z mult | PR zR z16R zchunkR          DEEP z o0 o1 o2 o3 | DR zR t_z t_gz t_ggz q_z
//   CHECK n z t_z t_gz t_ggz q_z got          (a tuple that satisfies the constraint, then each value off by one)
// Part 2 (argument `script`, commands on stdin):
//   mask <n> <d> <keyhex> : <n + d + 2 words>   -> M <words after the mask>  (and HOSTLOOP 0|1: the loop of csrc/host/fib_prover.hpp agrees)
//   rule <z> <log_N> <shift>                    -> R 0|1
//   init <hex|-> | status <v> | point <log_N> <shift> <tries> -> Z z | state -> T len status hex
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "fib_dz_kernels.hpp"
#include "contract_case.hpp"

using namespace toyni;

static uint64_t rng_state = 0xF1B0F1B0ull;
static uint32_t rnd() {
    rng_state += 0x9E3779B97F4A7C15ull;
    uint64_t x = rng_state;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((x ^ (x >> 31)) % BB_P);
}
static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return v;
}

static int records(bool saturated) {
    int bad = 0;
    std::vector<uint32_t> words = saturated ? std::vector<uint32_t>{BB_P - 1u} : std::vector<uint32_t>{0u, BB_P - 1u, BB_P, BB_P + 1u, 0xFFFFFFFFu, rnd(), rnd()};
    const uint32_t g = bb_root_of_unity_host(6);
    // ---- the three arrays of PolyEvalArgs, per point ----
    for (uint32_t zw : words)
        for (uint32_t mult : {1u, saturated ? BB_P - 1u : g, saturated ? BB_P - 1u : bb_mul_host(g, g)}) {
            TOYNI_CONTRACT_TAG("emu_fib_dz poly z=%u mult=%u", zw, mult);
            std::unique_ptr<uint32_t[]> z(new uint32_t[1]);
            z[0] = zw;
            std::unique_ptr<PolyDzRecord> rec(new PolyDzRecord);
            memset(rec.get(), 0xA5, sizeof(PolyDzRecord));
            poly_dz_record_point(z.get(), mult, 2u, *rec);
            const uint32_t point = bb_mul_host(zw % BB_P, mult);   // what the caller of toyni_poly_eval_device passes
            const uint32_t want[3] = {to_mont_host(point), to_mont_host(bb_pow_host(point, POLY_PER_THREAD)), to_mont_host(bb_pow_host(point, POLY_CHUNK))};
            const uint32_t got[3] = {rec->zR[2], rec->z16R[2], rec->zchunkR[2]};
            if (memcmp(want, got, sizeof want)) { ++bad; printf("MISMATCH poly\n"); }
            for (int p : {0, 1, 3})
                if (rec->zR[p] != 0xA5A5A5A5u || rec->z16R[p] != 0xA5A5A5A5u || rec->zchunkR[p] != 0xA5A5A5A5u) { ++bad; printf("MISMATCH poly slot\n"); }
            printf("POLY %u %u\nPR %u %u %u\n", zw, mult, got[0], got[1], got[2]);
        }
    // ---- the record of the DEEP layer ----
    for (size_t i = 0; i < words.size(); ++i) {
        std::unique_ptr<uint32_t[]> z(new uint32_t[1]), ood(new uint32_t[4]);
        z[0] = words[i];
        for (size_t k = 0; k < 4; ++k) ood[k] = words[(i + 1 + k) % words.size()];
        TOYNI_CONTRACT_TAG("emu_fib_dz deep z=%u", z[0]);
        std::unique_ptr<FibDeepRecord> rec(new FibDeepRecord);
        memset(rec.get(), 0xA5, sizeof(FibDeepRecord));
        fib_deep_prepare(z.get(), ood.get(), FibCheckArgs{}, rec.get(), nullptr);
        DeepArgs host{};                                             // toyni_fib_deep_device on the reduced values
        host.zR = to_mont_host(z[0] % BB_P);
        host.t_z = ood[0] % BB_P; host.t_gz = ood[1] % BB_P; host.t_ggz = ood[2] % BB_P; host.q_z = ood[3] % BB_P;
        DeepArgs dev{};
        fib_deep_args_from_record(dev, *rec);
        if (memcmp(&host, &dev, sizeof host) || rec->pad[0] != 0xA5A5A5A5u) { ++bad; printf("MISMATCH deep\n"); }
        printf("DEEP %u %u %u %u %u\nDR %u %u %u %u %u\n", z[0], ood[0], ood[1], ood[2], ood[3], rec->zR, rec->t_z, rec->t_gz, rec->t_ggz, rec->q_z);
    }
    // ---- the check word: a tuple that satisfies the constraint, then each value off by one ----
    for (uint32_t log_n : {0u, 1u, 3u, 6u, 16u}) {
        const uint64_t n = 1ull << log_n;
        const uint32_t gn = bb_root_of_unity_host(log_n), g_inv = bb_inv_host(gn);
        const FibCheckArgs k{to_mont_host(g_inv), to_mont_host(bb_mul_host(g_inv, g_inv)), log_n};
        for (int rep = 0; rep < (saturated ? 1 : 3); ++rep) {
            const uint32_t zv = saturated ? BB_P - 1u : rnd(), t_z = saturated ? BB_P - 1u : rnd(), t_gz = saturated ? BB_P - 1u : rnd(), q_z = saturated ? BB_P - 1u : rnd();
            const uint32_t den = bb_mul_host((zv + BB_P - bb_pow_host(gn, n - 1)) % BB_P, (zv + BB_P - bb_pow_host(gn, (n + n - 2) % n)) % BB_P);
            if (den == 0) continue;
            const uint32_t fib = bb_mul_host(bb_mul_host(q_z, (bb_pow_host(zv, n) + BB_P - 1u) % BB_P), bb_inv_host(den));
            const uint32_t good[4] = {t_z, t_gz, (uint32_t)(((uint64_t)fib + t_gz + t_z) % BB_P), q_z};
            for (int off = -1; off < 4; ++off) {
                TOYNI_CONTRACT_TAG("emu_fib_dz check log_n=%u off=%d", log_n, off);
                std::unique_ptr<uint32_t[]> z(new uint32_t[1]), ood(new uint32_t[4]), chk(new uint32_t[1]);
                z[0] = rep == 1 ? zv + BB_P : zv;                    // (once as a word that needs the reduction; zv + p < 2^32)
                for (int j = 0; j < 4; ++j) ood[j] = (good[j] + (j == off ? 1u : 0u)) % BB_P;
                chk[0] = 0xA5A5A5A5u;
                FibDeepRecord rec;
                fib_deep_prepare(z.get(), ood.get(), k, &rec, chk.get());
                // the reference's own evaluation (src/fibonacci.rs:173-177) in host arithmetic; with z^n = 1 a wrong q_z still passes
                const uint32_t lhs = bb_mul_host((uint32_t)(((uint64_t)ood[2] + 2ull * BB_P - ood[1] - ood[0]) % BB_P), den);
                const uint32_t rhs = bb_mul_host(ood[3], (bb_pow_host(zv, n) + BB_P - 1u) % BB_P);
                if (chk[0] != (lhs == rhs ? 1u : 0u) || (off < 0 && chk[0] != 1u)) { ++bad; printf("MISMATCH check\n"); }
                printf("CHECK %llu %u %u %u %u %u %u\n", (unsigned long long)n, z[0], ood[0], ood[1], ood[2], ood[3], chk[0]);
            }
        }
    }
    printf("BAD %d\nDONE\n", bad);
    return bad ? 1 : 0;
}

// the mask loop of csrc/host/fib_prover.hpp (Prover::generate_proof, step 1) on a host copy: minus R at x^i, plus R at x^(n + i)
static void host_mask_loop(std::vector<uint32_t>& c, size_t n, unsigned d, const uint32_t kw[8], const uint32_t nonce[3]) {
    uint32_t ks[16];
    for (unsigned i = 0; i < d; ++i) {
        if (i % 8 == 0) chacha20_block(kw, i / 8, nonce, ks);
        const uint64_t v = (uint64_t)ks[2 * (i % 8)] | (uint64_t)ks[2 * (i % 8) + 1] << 32;
        const uint32_t r = (uint32_t)(v % BB_P);
        c[i] = (uint32_t)(((uint64_t)c[i] + BB_P - r) % BB_P);
        c[n + i] = (uint32_t)(((uint64_t)c[n + i] + r) % BB_P);
    }
}

static int script() {
    TranscriptState* tr = static_cast<TranscriptState*>(aligned_alloc(16, sizeof(TranscriptState)));
    memset(tr, 0, sizeof *tr);
    std::string line;
    unsigned long lineno = 0;
    while (std::getline(std::cin, line)) {
        ++lineno;
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        TOYNI_CONTRACT_TAG("emu_fib_dz line %lu: %s", lineno, cmd.c_str());
        if (cmd == "mask") {
            unsigned long long n = 0, v;
            unsigned d = 0;
            std::string keyhex, colon;
            in >> n >> d >> keyhex >> colon;
            std::vector<uint32_t> w;
            while (in >> v) w.push_back((uint32_t)v);
            const std::vector<uint8_t> key = unhex(keyhex);
            if (key.size() != 32 || w.size() != n + d + 2) return 2;
            FibMaskArgs a{};
            std::unique_ptr<uint32_t[]> buf(new uint32_t[w.size()]);
            memcpy(buf.get(), w.data(), 4 * w.size());
            a.coeffs = buf.get();
            a.n = n;
            a.mask_degree = d;
            memcpy(a.key, key.data(), 32);
            a.nonce[0] = 0u; a.nonce[1] = 1u; a.nonce[2] = 0u;
            // one thread per output word, in an order no launch would take: the last thread first
            for (uint64_t t = fib_mask_items(n, d); t-- > 0;) {
                const uint64_t j = fib_mask_item_word(n, d, t);
                buf[j] = fib_mask_output(a, j, buf[j]);
            }
            std::vector<uint32_t> host(w.begin(), w.end());
            for (size_t j = 0; j < n + d; ++j) host[j] %= BB_P;      // (the host loop meets canonical words)
            host_mask_loop(host, n, d, a.key, a.nonce);
            bool same = true;
            for (size_t j = 0; j < w.size(); ++j) {
                const bool touched = j < d || (j >= n && j < n + d);
                same &= buf[j] == (touched ? host[j] : w[j]);
            }
            printf("M");
            for (size_t j = 0; j < w.size(); ++j) printf(" %u", buf[j]);
            printf("\nHOSTLOOP %d\n", same ? 1 : 0);
        } else if (cmd == "rule") {
            unsigned long long z, log_N, shift;
            in >> z >> log_N >> shift;
            printf("R %d\n", fib_point_rejected((uint32_t)z, (uint32_t)log_N, to_mont_host(bb_inv_host((uint32_t)shift))) ? 1 : 0);
        } else if (cmd == "init") {
            std::string hex;
            in >> hex;
            const std::vector<uint8_t> b = unhex(hex);
            if (b.size() > TRANSCRIPT_CAPACITY) return 2;
            memset(tr, 0, 16);
            memset(tr->bytes, 0xA5, TRANSCRIPT_CAPACITY);
            if (!b.empty()) memcpy(tr->bytes, b.data(), b.size());
            tr->len = (uint32_t)b.size();
        } else if (cmd == "status") {
            in >> tr->status;
        } else if (cmd == "point") {
            unsigned log_N = 0, shift = 1, tries = 0;
            in >> log_N >> shift >> tries;
            std::unique_ptr<uint32_t[]> z(new uint32_t[1]);
            z[0] = 0xDEADBEEFu;
            transcript_squeeze_point(*tr, log_N, to_mont_host(bb_inv_host(shift)), tries, z.get());
            printf("Z %u\n", z[0]);
        } else if (cmd == "state") {
            printf("T %u %u ", tr->len, tr->status);
            for (uint32_t k = 0; k < TRANSCRIPT_CAPACITY; ++k) printf("%02x", tr->bytes[k]);
            printf("\n");
        } else {
            fprintf(stderr, "unknown command: %s\n", cmd.c_str());
            return 2;
        }
    }
    free(tr);
    printf("DONE\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "records") return records(false);
    if (mode == "saturated") return records(true);
    if (mode == "script") return script();
    fprintf(stderr, "usage: emu_fib_dz records | saturated | script\n");
    return 2;
}
