// Measurement program of tools/fibbatchbench.py: the three compiled Fibonacci provers in ONE process,
//   a  toyni::fib::Prover             host transcript, blocking
//   s  toyni::fib::StreamProver       device transcript, one synchronisation per proof
//   b  toyni::fib::BatchStreamProver  `batch` proofs in one chain of launches, one synchronisation per batch
// alternating inside every round.  Before anything is timed, every proof of the batch is compared with the proof StreamProver writes
// for the same trace under the same key, and proof 0 with the blocking prover's.
//   fibbatchbench <trace_len> <batch> <rounds> <reps>
// stdout: one JSON line {"trace_len":..,"batch":..,"equal":true,"a":[ms per proof..],"s":[..],"b":[ms per proof = ms per batch / batch..]}
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../toyni_amd/csrc/host/fib_prover_batch.hpp"

using namespace toyni::fib;

static bool same(const Proof& x, const Proof& y) {
    if (x.trace_len != y.trace_len || x.lde_size != y.lde_size || x.trace_commitment != y.trace_commitment || x.quotient_commitment != y.quotient_commitment) return false;
    if (x.t_z != y.t_z || x.t_gz != y.t_gz || x.t_ggz != y.t_ggz || x.q_z != y.q_z) return false;
    if (x.fri_commitments != y.fri_commitments || x.fri_final_layer != y.fri_final_layer || x.query_indices != y.query_indices) return false;
    if (x.opening_records != y.opening_records || x.opening_groups.size() != y.opening_groups.size()) return false;
    for (size_t i = 0; i < x.opening_groups.size(); ++i)
        if (x.opening_groups[i].tree_leaves != y.opening_groups[i].tree_leaves || x.opening_groups[i].indices != y.opening_groups[i].indices) return false;
    return true;
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: %s <trace_len> <batch> <rounds> <reps>\n", argv[0]); return 2; }
    const size_t n = std::strtoull(argv[1], nullptr, 0), batch = std::strtoull(argv[2], nullptr, 0);
    const int rounds = std::atoi(argv[3]), reps = std::atoi(argv[4]);
    int count = 0;
    if (toyni_device_count(&count) != 0 || count <= 0) { std::printf("{\"gpu\": false}\n"); return 0; }
    std::vector<uint32_t> traces(batch * n);
    std::vector<uint8_t> keys(32 * batch);
    for (size_t b = 0; b < batch; ++b) {
        uint32_t x = (uint32_t)(1 + b), y = x;
        for (size_t i = 0; i < n; ++i) { traces[b * n + i] = x; const uint32_t nx = addmod(x, y); x = y; y = nx; }
        for (int i = 0; i < 32; ++i) keys[32 * b + i] = (uint8_t)(((17 + b) * 0x9E3779B97F4A7C15ull + 0x1234567u * (unsigned)i) >> (8 * (i % 8)));
    }
    Prover pa(n);
    StreamProver ps(n);
    BatchStreamProver pb(n, batch);
    std::vector<Proof> proofs;
    std::vector<std::string> errors;
    Proof one;
    std::string err;
    const auto fail = [](const std::string& what) { std::printf("{\"gpu\": true, \"error\": \"%s\"}\n", what.c_str()); return 1; };
    // ---- the proofs first (this also warms every prover) ----
    if (!(err = pb.enqueue(traces.data(), keys.data())).empty() || !(err = pb.collect(proofs, errors)).empty()) return fail(err);
    for (size_t b = 0; b < batch; ++b) {
        if (!errors[b].empty()) return fail(errors[b]);
        if (!(err = ps.enqueue(traces.data() + b * n, keys.data() + 32 * b)).empty() || !(err = ps.collect(one)).empty()) return fail(err);
        if (!same(one, proofs[b])) return fail("proof " + std::to_string(b) + " of the batch differs from the stream prover's");
    }
    if (!(err = pa.generate_proof(traces.data(), keys.data(), one)).empty()) return fail(err);
    if (!same(one, proofs[0])) return fail("proof 0 of the batch differs from the blocking prover's");
    // ---- the clock ----
    std::vector<double> ta, ts, tb;
    for (int r = 0; r < rounds; ++r) {
        for (int k = 0; k < reps; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            if (!(err = pa.generate_proof(traces.data(), keys.data(), one)).empty()) return fail(err);
            ta.push_back(ms_since(t0));
        }
        for (int k = 0; k < reps; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            if (!(err = ps.enqueue(traces.data(), keys.data())).empty() || !(err = ps.collect(one)).empty()) return fail(err);
            ts.push_back(ms_since(t0));
        }
        for (int k = 0; k < reps; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            if (!(err = pb.enqueue(traces.data(), keys.data())).empty() || !(err = pb.collect(proofs, errors)).empty()) return fail(err);
            tb.push_back(ms_since(t0) / (double)batch);
        }
    }
    const auto list = [](const std::vector<double>& v) {
        std::string s = "[";
        char buf[32];
        for (size_t i = 0; i < v.size(); ++i) { std::snprintf(buf, sizeof buf, "%s%.4f", i ? ", " : "", v[i]); s += buf; }
        return s + "]";
    };
    const BatchStreamProver::Traffic& tr = pb.traffic();
    std::printf("{\"gpu\": true, \"trace_len\": %zu, \"batch\": %zu, \"equal\": true, \"open_launches\": %zu, \"h2d_copies\": %zu, \"d2h_copies\": %zu, "
                "\"synchronisations\": %zu, \"a\": %s, \"s\": %s, \"b\": %s}\n",
                n, batch, pb.open_launches(), tr.h2d_copies, tr.d2h_copies, tr.synchronisations, list(ta).c_str(), list(ts).c_str(), list(tb).c_str());
    return 0;
}
