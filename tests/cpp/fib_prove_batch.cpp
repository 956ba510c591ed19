// Driver of the batched stream-ordered prover toyni_amd/csrc/host/fib_prover_batch.hpp (toyni::fib::BatchStreamProver): `batch` proofs
// of one trace length from one chain of launches, each the proof of tests/cpp/fib_prove_dt.cpp byte for byte.  Run by
// tests/test_gpu_fib_prove_batch.py.
//   fib_prove_batch <trace_len> <seed> <reps> <batch> [proof.json] [--corrupt-proof B --corrupt-row R]
// Proof b uses fib_prove's test-key rule with seed + b; its trace is the Fibonacci column started at (1 + b, 1 + b) (the AIR has no
// boundary constraint, so any start satisfies it).  Proof b is written to <proof.json>.<b>, proof 0 also to <proof.json>; a proof
// that failed writes no file.  --corrupt-proof B --corrupt-row R adds one to row R of trace B.
// stdout: one JSON line like fib_prove_dt's, with "batch" and "errors" (one string per proof, "" = proved); ms_per_proof is the
// batch's time divided by `batch`; the counts are those of the last (warm) batch.
#include "launch_dump.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../toyni_amd/csrc/host/fib_prover_batch.hpp"

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
    if (argc < 5) { std::fprintf(stderr, "usage: %s <trace_len> <seed> <reps> <batch> [proof.json] [--corrupt-proof B --corrupt-row R]\n", argv[0]); return 2; }
    const size_t n = std::strtoull(argv[1], nullptr, 0);
    const uint64_t seed = std::strtoull(argv[2], nullptr, 0);
    const int reps = std::atoi(argv[3]);
    const size_t batch = std::strtoull(argv[4], nullptr, 0);
    const char* out_path = nullptr;
    long corrupt_proof = -1, corrupt_row = -1;
    for (int i = 5; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--corrupt-proof") && i + 1 < argc) corrupt_proof = std::atol(argv[++i]);
        else if (!std::strcmp(argv[i], "--corrupt-row") && i + 1 < argc) corrupt_row = std::atol(argv[++i]);
        else out_path = argv[i];
    }
    if (batch < 1 || batch > 65535) { std::fprintf(stderr, "batch takes 1 to 65535\n"); return 2; }
    int count = 0;
    if (toyni_device_count(&count) != 0 || count <= 0) { std::printf("{\"gpu\": false}\n"); return 0; }   // self-skip like src/ntt.rs:265-268
    std::vector<uint32_t> traces(batch * n);
    std::vector<uint8_t> keys(32 * batch);
    for (size_t b = 0; b < batch; ++b) {
        uint32_t* t = traces.data() + b * n;
        uint32_t x = (uint32_t)((1 + b) % P), y = x;
        for (size_t i = 0; i < n; ++i) { t[i] = x; const uint32_t nx = addmod(x, y); x = y; y = nx; }
        const uint64_t sb = seed + b;
        for (int i = 0; i < 32; ++i) keys[32 * b + i] = (uint8_t)((sb * 0x9E3779B97F4A7C15ull + 0x1234567u * (unsigned)i) >> (8 * (i % 8)));   // a TEST key
    }
    if (corrupt_proof >= 0 && (size_t)corrupt_proof < batch && corrupt_row >= 0 && (size_t)corrupt_row < n) {
        uint32_t& w = traces[(size_t)corrupt_proof * n + (size_t)corrupt_row];
        w = addmod(w, 1);
    }
    BatchStreamProver prover(n, batch);
    std::vector<Proof> proofs;
    std::vector<std::string> errors;
    double enqueue_ms = 0;
    const auto round = [&]() -> std::string {
        const auto e0 = std::chrono::steady_clock::now();
        std::string err = prover.enqueue(traces.data(), keys.data());
        if (!err.empty()) return err;
        enqueue_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - e0).count();
        return prover.collect(proofs, errors);
    };
    std::string err = round();   // warm: contexts, tables, buffers
    if (!err.empty()) { std::printf("{\"gpu\": true, \"error\": \"%s\"}\n", err.c_str()); return 1; }
    std::string ms = "[", ems = "[";
    for (int r = 0; r < reps; ++r) {
        for (size_t b = 0; b < batch; ++b) keys[32 * b] = (uint8_t)(keys[32 * b] + 1);   // fib_prove_dt's rule: a new key per repetition
        const auto t0 = std::chrono::steady_clock::now();
        err = round();
        const auto t1 = std::chrono::steady_clock::now();
        if (!err.empty()) { std::printf("{\"gpu\": true, \"error\": \"%s\"}\n", err.c_str()); return 1; }
        char buf[64];
        std::snprintf(buf, sizeof buf, "%s%.4f", r ? ", " : "", std::chrono::duration<double, std::milli>(t1 - t0).count() / (double)batch);
        ms += buf;
        std::snprintf(buf, sizeof buf, "%s%.4f", r ? ", " : "", enqueue_ms / (double)batch);
        ems += buf;
    }
    ms += "]";
    ems += "]";
    std::string errs = "[";
    size_t proof_bytes = 0;
    for (size_t b = 0; b < batch; ++b) {
        errs += std::string(b ? ", " : "") + "\"" + errors[b] + "\"";
        if (!errors[b].empty()) continue;
        const Proof& p = proofs[b];
        if (!proof_bytes) proof_bytes = p.opening_records.size() + 32 * (2 + p.fri_commitments.size()) + 4 * (4 + p.fri_final_layer.size());
        if (!out_path) continue;
        const std::string path = std::string(out_path) + "." + std::to_string(b);
        if (!write_proof(path.c_str(), p, keys.data() + 32 * b) || (b == 0 && !write_proof(out_path, p, keys.data()))) {
            std::fprintf(stderr, "cannot write %s\n", path.c_str());
            return 1;
        }
    }
    errs += "]";
    const BatchStreamProver::Traffic& tr = prover.traffic();
    std::printf("{\"gpu\": true, \"trace_len\": %zu, \"lde_size\": %zu, \"folds\": %zu, \"final_layer_size\": %zu, \"batch\": %zu, \"ms_per_proof\": %s, "
                "\"enqueue_ms_per_proof\": %s, \"proof_bytes\": %zu, \"errors\": %s, "
                "\"pcie\": {\"h2d_bytes\": %zu, \"d2h_bytes\": %zu, \"h2d_copies\": %zu, \"d2h_copies\": %zu, \"pinned_root_writes\": %zu, \"synchronisations\": %zu}}\n",
                n, n << LOG_BLOWUP, prover.folds(), prover.final_layer_size(), batch, ms.c_str(), ems.c_str(), proof_bytes, errs.c_str(),
                tr.h2d_bytes, tr.d2h_bytes, tr.h2d_copies, tr.d2h_copies, tr.pinned_root_writes, tr.synchronisations);
    return 0;
}
