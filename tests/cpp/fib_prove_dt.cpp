// Driver of the stream-ordered compiled prover toyni_amd/csrc/host/fib_prover_dt.hpp (toyni::fib::StreamProver): the proof of
// tests/cpp/fib_prove.cpp, byte for byte, from one chain of enqueues and one synchronisation.  Run by tests/test_gpu_fib_prove_dt.py.
//   fib_prove_dt <trace_len> <seed> <reps> [proof.json] [--corrupt-row R] [--in-flight K]
// The test key rule and the JSON proof file are those of fib_prove.  --in-flight K (1-4): K provers; per repetition the one thread
// calls enqueue on all of them (the same trace, the same key) and then collect on all of them; prover k > 0 writes its last proof to
// <proof.json>.<k>, prover 0 to <proof.json>.
// stdout: one JSON line {"gpu":..,"trace_len":..,"in_flight":K,"ms_per_proof":[..],"enqueue_ms_per_proof":[..],"pcie":{..,
// "synchronisations":..}} -- the counts are those of the last (warm) proof of prover 0; enqueue_ms_per_proof is the part of
// ms_per_proof the one thread spent inside enqueue() (the rest it spent waiting in collect()).
#include "launch_dump.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../toyni_amd/csrc/host/fib_prover_dt.hpp"

using namespace toyni::fib;

static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; ++i) { s[2 * i] = d[p[i] >> 4]; s[2 * i + 1] = d[p[i] & 15]; }
    return s;
}

static bool write_proof(const char* path, const Proof& pr, const uint8_t key[32]) {
    FILE* f = std::fopen(path, "w");
    if (!f) return false;
    std::fprintf(f, "{\"key\": \"%s\",\n \"trace_len\": %zu, \"lde_size\": %zu, \"trace_commitment\": \"%s\", \"quotient_commitment\": \"%s\",\n", hex(key, 32).c_str(), pr.trace_len, pr.lde_size,
                 hex(pr.trace_commitment.data(), 32).c_str(), hex(pr.quotient_commitment.data(), 32).c_str());
    std::fprintf(f, " \"t_z\": %u, \"t_gz\": %u, \"t_ggz\": %u, \"q_z\": %u,\n \"fri_commitments\": [", pr.t_z, pr.t_gz, pr.t_ggz, pr.q_z);
    for (size_t i = 0; i < pr.fri_commitments.size(); ++i) std::fprintf(f, "%s\"%s\"", i ? ", " : "", hex(pr.fri_commitments[i].data(), 32).c_str());
    std::fprintf(f, "],\n \"fri_final_layer\": [");
    for (size_t i = 0; i < pr.fri_final_layer.size(); ++i) std::fprintf(f, "%s%u", i ? ", " : "", pr.fri_final_layer[i]);
    std::fprintf(f, "],\n \"query_indices\": [");
    for (size_t i = 0; i < pr.query_indices.size(); ++i) std::fprintf(f, "%s%u", i ? ", " : "", pr.query_indices[i]);
    std::fprintf(f, "],\n \"opening_groups\": [");
    for (size_t k = 0; k < pr.opening_groups.size(); ++k) {
        const auto& g = pr.opening_groups[k];
        std::fprintf(f, "%s[%zu, %s, [", k ? ", " : "", g.tree_leaves, g.salted ? "true" : "false");
        for (size_t i = 0; i < g.indices.size(); ++i) std::fprintf(f, "%s%u", i ? ", " : "", g.indices[i]);
        std::fprintf(f, "]]");
    }
    std::fprintf(f, "],\n \"opening_records\": \"%s\"}\n", hex(pr.opening_records.data(), pr.opening_records.size()).c_str());
    return std::fclose(f) == 0;
}

int main(int argc, char** argv) {
    struct DumpAtReturn { ~DumpAtReturn() { toyni_test_dump_launched_kernels(); } } dump_at_return;   // kernel-coverage guard of the test session
    if (argc < 4) { std::fprintf(stderr, "usage: %s <trace_len> <seed> <reps> [proof.json] [--corrupt-row R] [--in-flight K]\n", argv[0]); return 2; }
    const size_t n = std::strtoull(argv[1], nullptr, 0);
    const uint64_t seed = std::strtoull(argv[2], nullptr, 0);
    const int reps = std::atoi(argv[3]);
    const char* out_path = nullptr;
    long corrupt = -1;
    int in_flight = 1;
    for (int i = 4; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--corrupt-row") && i + 1 < argc) corrupt = std::atol(argv[++i]);
        else if (!std::strcmp(argv[i], "--in-flight") && i + 1 < argc) in_flight = std::atoi(argv[++i]);
        else out_path = argv[i];
    }
    if (in_flight < 1 || in_flight > 4) { std::fprintf(stderr, "--in-flight takes 1 to 4\n"); return 2; }
    int count = 0;
    if (toyni_device_count(&count) != 0 || count <= 0) { std::printf("{\"gpu\": false}\n"); return 0; }   // self-skip like src/ntt.rs:265-268
    auto trace = fibonacci_trace(n);
    if (corrupt >= 0 && (size_t)corrupt < n) trace[(size_t)corrupt] = addmod(trace[(size_t)corrupt], 1);     // src/fibonacci.rs:430-442
    uint8_t key[32];
    for (int i = 0; i < 32; ++i) key[i] = (uint8_t)((seed * 0x9E3779B97F4A7C15ull + 0x1234567u * (unsigned)i) >> (8 * (i % 8)));   // a TEST key (a prover draws it from the OS)
    std::vector<std::unique_ptr<StreamProver>> provers;
    for (int k = 0; k < in_flight; ++k) provers.emplace_back(new StreamProver(n));
    std::vector<Proof> proofs((size_t)in_flight);
    double enqueue_ms = 0;
    const auto round = [&]() -> std::string {   // every prover enqueues, then every prover collects: one thread
        const auto e0 = std::chrono::steady_clock::now();
        for (auto& p : provers) { std::string err = p->enqueue(trace.data(), key); if (!err.empty()) return err; }
        enqueue_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - e0).count();
        std::string first;
        for (int k = 0; k < in_flight; ++k) { std::string err = provers[(size_t)k]->collect(proofs[(size_t)k]); if (first.empty()) first = err; }
        return first;
    };
    std::string err = round();   // warm: contexts, tables, buffers
    if (!err.empty()) { std::printf("{\"gpu\": true, \"error\": \"%s\"}\n", err.c_str()); return 1; }
    std::string ms = "[", ems = "[";
    for (int r = 0; r < reps; ++r) {
        key[0] = (uint8_t)(key[0] + 1);
        const auto t0 = std::chrono::steady_clock::now();
        err = round();
        const auto t1 = std::chrono::steady_clock::now();
        if (!err.empty()) { std::printf("{\"gpu\": true, \"error\": \"%s\"}\n", err.c_str()); return 1; }
        char buf[64];
        std::snprintf(buf, sizeof buf, "%s%.4f", r ? ", " : "", std::chrono::duration<double, std::milli>(t1 - t0).count() / in_flight);
        ms += buf;
        std::snprintf(buf, sizeof buf, "%s%.4f", r ? ", " : "", enqueue_ms / in_flight);
        ems += buf;
    }
    ms += "]";
    ems += "]";
    if (out_path)
        for (int k = 0; k < in_flight; ++k) {
            const std::string path = k ? std::string(out_path) + "." + std::to_string(k) : std::string(out_path);
            if (!write_proof(path.c_str(), proofs[(size_t)k], key)) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        }
    const Proof& proof = proofs[0];
    const StreamProver::Traffic& tr = provers[0]->traffic();
    std::printf("{\"gpu\": true, \"trace_len\": %zu, \"lde_size\": %zu, \"folds\": %zu, \"final_layer_size\": %zu, \"in_flight\": %d, \"ms_per_proof\": %s, \"enqueue_ms_per_proof\": %s, "
                "\"proof_bytes\": %zu, "
                "\"pcie\": {\"h2d_bytes\": %zu, \"d2h_bytes\": %zu, \"h2d_copies\": %zu, \"d2h_copies\": %zu, \"pinned_root_writes\": %zu, \"synchronisations\": %zu}}\n",
                proof.trace_len, proof.lde_size, provers[0]->folds(), provers[0]->final_layer_size(), in_flight, ms.c_str(), ems.c_str(),
                proof.opening_records.size() + 32 * (2 + proof.fri_commitments.size()) + 4 * (4 + proof.fri_final_layer.size()),
                tr.h2d_bytes, tr.d2h_bytes, tr.h2d_copies, tr.d2h_copies, tr.pinned_root_writes, tr.synchronisations);
    return 0;
}
