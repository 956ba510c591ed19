// Driver of the device verifier's C++ caller toyni_amd/csrc/host/fib_verifier.hpp (toyni::fib::BatchVerifier): proves `batch` Fibonacci
// traces with BatchStreamProver (tests/cpp/fib_prove_batch.cpp's traces and test keys), verifies them in one chain of launches and
// prints the verdicts.  Run by tests/test_gpu_fib_verify_cpp.py.
//   fib_verify_batch <trace_len> <seed> <reps> <batch> [proof.json] [--tamper B KIND]
// KIND: t_z (t_z + 1), path (a path byte of the first trace record), index (a claimed query index), final (every final value + 1).
// Proof b is written to <proof.json>.<b> as tampered.  stdout: one JSON line -- the verdict words, their names, the verifier's traffic
// of the last batch and ms per verified batch (host clock around upload, chain, download and the one synchronisation).
#include "launch_dump.hpp"
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../toyni_amd/csrc/host/fib_prover_batch.hpp"
#include "../../toyni_amd/csrc/host/fib_verifier.hpp"

using namespace toyni::fib;

static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s(2 * n, '0');
    for (size_t i = 0; i < n; ++i) { s[2 * i] = d[p[i] >> 4]; s[2 * i + 1] = d[p[i] & 15]; }
    return s;
}

static bool write_proof(const char* path, const Proof& pr) {
    FILE* f = std::fopen(path, "w");
    if (!f) return false;
    std::fprintf(f, "{\"trace_len\": %zu, \"lde_size\": %zu, \"trace_commitment\": \"%s\", \"quotient_commitment\": \"%s\",\n", pr.trace_len, pr.lde_size,
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
    if (argc < 5) { std::fprintf(stderr, "usage: %s <trace_len> <seed> <reps> <batch> [proof.json] [--tamper B KIND]\n", argv[0]); return 2; }
    const size_t n = std::strtoull(argv[1], nullptr, 0);
    const uint64_t seed = std::strtoull(argv[2], nullptr, 0);
    const int reps = std::atoi(argv[3]);
    const size_t batch = std::strtoull(argv[4], nullptr, 0);
    const char* out_path = nullptr;
    long tamper = -1;
    std::string kind;
    for (int i = 5; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--tamper") && i + 2 < argc) { tamper = std::atol(argv[i + 1]); kind = argv[i + 2]; i += 2; }
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
    std::vector<Proof> proofs;
    {
        BatchStreamProver prover(n, batch);
        std::vector<std::string> errors;
        std::string err = prover.enqueue(traces.data(), keys.data());
        if (err.empty()) err = prover.collect(proofs, errors);
        for (size_t b = 0; err.empty() && b < batch; ++b)
            if (!errors[b].empty()) err = "proof " + std::to_string(b) + ": " + errors[b];
        if (!err.empty()) { std::printf("{\"gpu\": true, \"error\": \"%s\"}\n", err.c_str()); return 1; }
    }
    if (tamper >= 0 && (size_t)tamper < batch) {
        Proof& p = proofs[(size_t)tamper];
        if (kind == "t_z") p.t_z = addmod(p.t_z, 1);
        else if (kind == "path") p.opening_records[5] ^= 0x20;
        else if (kind == "index") p.query_indices[3] ^= 1u;
        else if (kind == "final") { for (uint32_t& v : p.fri_final_layer) v = addmod(v, 1); }
        else { std::fprintf(stderr, "--tamper takes t_z, path, index or final\n"); return 2; }
    }
    for (size_t b = 0; out_path && b < batch; ++b)
        if (!write_proof((std::string(out_path) + "." + std::to_string(b)).c_str(), proofs[b])) { std::fprintf(stderr, "cannot write %s.%zu\n", out_path, b); return 1; }
    BatchVerifier verifier(n, batch);
    std::vector<uint32_t> verdicts;
    std::string err = verifier.verify(proofs, verdicts);   // warm: context, buffers, code objects
    if (!err.empty()) { std::printf("{\"gpu\": true, \"error\": \"%s\"}\n", err.c_str()); return 1; }
    std::string ms = "[";
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        err = verifier.verify(proofs, verdicts);
        const auto t1 = std::chrono::steady_clock::now();
        if (!err.empty()) { std::printf("{\"gpu\": true, \"error\": \"%s\"}\n", err.c_str()); return 1; }
        char buf[64];
        std::snprintf(buf, sizeof buf, "%s%.4f", r ? ", " : "", std::chrono::duration<double, std::milli>(t1 - t0).count());
        ms += buf;
    }
    ms += "]";
    std::string words = "[", names = "[";
    for (size_t b = 0; b < batch; ++b) {
        words += std::string(b ? ", " : "") + std::to_string(verdicts[b]);
        names += std::string(b ? ", " : "") + "\"" + toyni_fib_verdict_string(verdicts[b]) + "\"";
    }
    const BatchVerifier::Traffic& tr = verifier.traffic();
    std::printf("{\"gpu\": true, \"trace_len\": %zu, \"batch\": %zu, \"folds\": %zu, \"final_layer_size\": %zu, \"image_bytes\": %zu, \"verdicts\": %s], \"names\": %s], "
                "\"ms_per_batch\": %s, \"traffic\": {\"h2d_bytes\": %zu, \"d2h_bytes\": %zu, \"h2d_copies\": %zu, \"d2h_copies\": %zu, \"synchronisations\": %zu}}\n",
                n, batch, verifier.layout().folds, verifier.layout().final_size, verifier.layout().image_bytes, words.c_str(), names.c_str(), ms.c_str(),
                tr.h2d_bytes, tr.d2h_bytes, tr.h2d_copies, tr.d2h_copies, tr.synchronisations);
    return 0;
}
