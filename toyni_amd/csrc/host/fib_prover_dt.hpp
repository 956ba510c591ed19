// The Fibonacci prover of fib_prover.hpp as ONE stream-ordered chain on the device transcript (include/toyni_hip.h 3l, 3o, 3q):
// the same protocol, the same proof byte for byte, but nothing between the trace upload and the final download waits for the host.
// `Prover::generate_proof` stops its stream six times per proof (mask coefficients, the two roots, the out-of-domain values, the DEEP
// root, every fold round, the final layer) because its transcript lives on the host; here the transcript is a toyni_transcript in
// device memory, z never leaves the device, and the host reads everything it needs from one contiguous "tail" buffer:
//   trace / quotient / DEEP roots | the round roots | z | t_z t_gz t_ggz q_z | check word | 44 indices | final layer |
//   transcript len, status | opening records
// enqueue() only enqueues (on a warm prover: no synchronisation, one device-to-host copy -- the tail); collect() synchronises once
// and fills Proof exactly as Prover::generate_proof does.  Because enqueue() returns at once, one thread can keep several proofs in
// flight (one StreamProver each), which the blocking prover cannot.
//   step                                         call
//   salts (side stream)                          toyni_chacha20_fill_device
//   clear, upload, INTT                          toyni_memset_async, toyni_memcpy_h2d_async, toyni_ntt_device
//   mask                                         toyni_mask_poly_device                      (3q)
//   LDE; trace tree (side stream)                toyni_lde_device, toyni_merkle_commit_device
//   quotient, two INTTs, quotient tree           toyni_fib_quotient_device, toyni_coset_ntt_device, toyni_merkle_commit_device
//   absorb both roots where they lie             toyni_transcript_absorb_device              (3l)
//   z                                            toyni_transcript_squeeze_point_device       (3q)
//   T(z), T(g z), T(g^2 z), Q(z)                 toyni_poly_eval_dz_device x 2               (3q)
//   absorb the four values                       toyni_transcript_absorb_fields_device       (3o)
//   constraint check at z, DEEP layer            toyni_fib_deep_dz_device                    (3q)
//   DEEP tree, absorb its root                   toyni_merkle_commit_device, toyni_transcript_absorb_device
//   fold loop                                    toyni_fri_commit_phase_transcript_device    (3l)
//   queries                                      toyni_transcript_squeeze_indices_device, toyni_fri_query_positions_device,
//                                                toyni_query_rows_device, toyni_merkle_open_groups_device
//   round roots                                  toyni_fri_phase_roots_device                (3q)
//   one download                                 toyni_memcpy_d2h_async
#pragma once
#include "fib_prover.hpp"

namespace toyni {
namespace fib {

class StreamProver {
   public:
    explicit StreamProver(size_t trace_len, int device = -1) : n_(trace_len), device_(device) {}
    ~StreamProver() { release(); }
    StreamProver(const StreamProver&) = delete;
    StreamProver& operator=(const StreamProver&) = delete;

    // Prover::Traffic and the stream / device synchronisations this class issued for the last proof (enqueue + collect)
    struct Traffic : Prover::Traffic { size_t synchronisations = 0; };

#define TOYNI_FIB_DT_TRY(expr, what) do { st = (expr); if (st) return std::string(what) + ": " + toyni_error_string(st); } while (0)
    // Allocates every buffer of a proof once and builds the two contexts (which blocks).  "" = ok.
    std::string prepare() {
        if (ready_) return "";
        if (n_ < 8 || (n_ & (n_ - 1)) || n_ > ((size_t)1 << 22)) return "trace length must be a power of two in [8, 2^22]";
        log_n_ = 0;
        while (((size_t)1 << log_n_) < n_) ++log_n_;
        N_ = n_ << LOG_BLOWUP;
        log_N_ = log_n_ + LOG_BLOWUP;
        log_c_ = 0;
        while (((size_t)1 << log_c_) < n_ + MASK_DEGREE) ++log_c_;
        size_t bound = 1;
        while (bound < n_ + MASK_DEGREE) bound <<= 1;
        final_size_ = N_ / bound;
        if (final_size_ < 1 || log_c_ > log_N_) return "trace too short for this blow-up";
        sizes_.clear();
        for (size_t m = N_ / 2; m >= final_size_; m /= 2) { sizes_.push_back(m); if (m == final_size_) break; }
        salted_fri_ = 0;
        fri_digests_ = 0;
        fri_words_ = 0;
        for (size_t h : sizes_) { if (h != final_size_) salted_fri_ += h; fri_digests_ += toyni_merkle_total_digests(h); fri_words_ += h; }
        // the tail buffer: every offset a multiple of 4, the records at a multiple of 8
        const size_t rounds = sizes_.size();
        off_roots_ = 0;
        off_z_ = 32 * (3 + rounds);
        off_ood_ = off_z_ + 4;
        off_check_ = off_ood_ + 16;
        off_idx_ = off_check_ + 4;
        off_final_ = off_idx_ + 4 * NUM_QUERIES;
        off_state_ = off_final_ + 4 * final_size_;
        off_records_ = (off_state_ + 8 + 7) & ~(size_t)7;
        record_bytes_ = 0;
        record_bytes_ += NUM_QUERIES * (3 + 1 + 2) * toyni_merkle_open_record_bytes(N_);
        for (size_t li = 0; li + 1 < sizes_.size(); ++li) record_bytes_ += 2 * NUM_QUERIES * toyni_merkle_open_record_bytes(sizes_[li]);
        tail_bytes_ = off_records_ + record_bytes_;
        int st;
        TOYNI_FIB_DT_TRY(toyni_ntt_ctx_create((uint32_t)n_, device_, &ctx_n_), "trace-domain context");
        TOYNI_FIB_DT_TRY(toyni_ntt_ctx_create((uint32_t)N_, device_, &ctx_N_), "LDE-domain context");
        TOYNI_FIB_DT_TRY(toyni_stream_create(&stream_, toyni_ntt_ctx_device(ctx_N_)), "stream");
        TOYNI_FIB_DT_TRY(toyni_stream_create(&side_, toyni_ntt_ctx_device(ctx_N_)), "stream");
        TOYNI_FIB_DT_TRY(toyni_event_create(&salts_ready_), "event");
        const size_t tree_bytes = toyni_merkle_total_digests(N_) * 32;
        salt_bytes_ = ((3 * N_ + salted_fri_) * 16 + 63) & ~(size_t)63;
        struct { void** p; size_t bytes; } bufs[] = {
            {(void**)&d_compact_, ((size_t)4 << log_c_)}, {(void**)&d_trace_lde_, 4 * N_}, {(void**)&d_c_, 4 * N_}, {(void**)&d_q_, 4 * N_},
            {(void**)&d_qpoly_, 4 * N_}, {(void**)&d_deep_, 4 * N_}, {(void**)&d_layers_, 4 * fri_words_}, {(void**)&d_trace_tree_, tree_bytes},
            {(void**)&d_quot_tree_, tree_bytes}, {(void**)&d_deep_tree_, tree_bytes}, {(void**)&d_fri_trees_, fri_digests_ * 32},
            {(void**)&d_salts_, salt_bytes_}, {(void**)&d_pos_, 4 * positions()}, {(void**)&d_tr_, sizeof(toyni_transcript)}, {(void**)&d_tail_, tail_bytes_}};
        for (auto& b : bufs) TOYNI_FIB_DT_TRY(toyni_malloc(b.p, b.bytes), "device allocation");
        TOYNI_FIB_DT_TRY(toyni_host_alloc((void**)&h_pinned_, 4 * n_ + 64 + tail_bytes_), "pinned staging");
        ready_ = true;
        return "";
    }

    // Enqueues a whole proof, from the trace upload to the copy of the tail buffer into pinned memory, and returns.  The trace is
    // copied before the call returns.  One proof per StreamProver is in flight at a time: collect() closes it.
    std::string enqueue(const uint32_t* trace, const uint8_t key[32]) {
        if (in_flight_) return "a proof is already in flight";
        std::string err = prepare();
        if (!err.empty()) return err;
        int st;
        void* s = stream_;
        traffic_ = Traffic{};
        auto up = [&](void* d, const void* h, size_t bytes) { traffic_.h2d_bytes += bytes; ++traffic_.h2d_copies; return toyni_memcpy_h2d_async(d, h, bytes, s); };
        const uint32_t g = root_of_unity(log_n_);
        const size_t B = (size_t)1 << LOG_BLOWUP, rounds = sizes_.size();
        uint32_t* hp = reinterpret_cast<uint32_t*>(h_pinned_);
        uint8_t* h_state = h_pinned_ + 4 * n_;                       // the transcript's header and first bytes: 32 bytes
        uint32_t* t_z = reinterpret_cast<uint32_t*>(d_tail_ + off_z_);
        uint32_t* t_ood = reinterpret_cast<uint32_t*>(d_tail_ + off_ood_);
        uint32_t* t_check = reinterpret_cast<uint32_t*>(d_tail_ + off_check_);
        uint32_t* t_idx = reinterpret_cast<uint32_t*>(d_tail_ + off_idx_);
        const uint8_t* salts_trace = d_salts_;
        const uint8_t* salts_quot = d_salts_ + 16 * N_;
        const uint8_t* salts_deep = d_salts_ + 32 * N_;
        const uint8_t* salts_fri = d_salts_ + 48 * N_;
        const size_t root_off = (toyni_merkle_total_digests(N_) - 1) * 32;

        TOYNI_FIB_DT_TRY(toyni_chacha20_fill_device(d_salts_, salt_bytes_, key, 0, side_), "salts");
        TOYNI_FIB_DT_TRY(toyni_event_record(salts_ready_, side_), "event");
        // ---- 1. trace polynomial, mask, LDE, trace tree ----
        TOYNI_FIB_DT_TRY(toyni_memset_async(d_compact_, 0, (size_t)4 << log_c_, s), "clear");
        std::memcpy(hp, trace, 4 * n_);
        TOYNI_FIB_DT_TRY(up(d_compact_, hp, 4 * n_), "trace upload");
        {   // the transcript starts as the reference's does (src/transcript.rs:12-17): len = 14, status = 0
            std::memset(h_state, 0, 32);
            const uint32_t len = 14;
            std::memcpy(h_state, &len, 4);
            std::memcpy(h_state + 16, "toyni-stark-v1", 14);
            TOYNI_FIB_DT_TRY(up(d_tr_, h_state, 32), "transcript upload");
        }
        TOYNI_FIB_DT_TRY(toyni_ntt_device(ctx_n_, d_compact_, d_compact_, 1, 1, s), "interpolation (INTT)");
        TOYNI_FIB_DT_TRY(toyni_mask_poly_device(d_compact_, n_, MASK_DEGREE, key, 1, s), "mask");   // nonce 1 (nonce 0 is the salts')
        const size_t ncoef_t = n_ + MASK_DEGREE;
        TOYNI_FIB_DT_TRY(toyni_lde_device(ctx_N_, d_compact_, d_trace_lde_, 1, log_N_ - log_c_, COSET_SHIFT, s), "LDE");
        TOYNI_FIB_DT_TRY(toyni_stream_wait(side_, s), "stream order");
        TOYNI_FIB_DT_TRY(toyni_merkle_commit_device(d_trace_lde_, salts_trace, N_, d_trace_tree_, side_), "trace commitment");
        // ---- 2. constraint, quotient, quotient tree ----
        TOYNI_FIB_DT_TRY(toyni_fib_quotient_device(ctx_N_, d_trace_lde_, d_c_, d_q_, LOG_BLOWUP, COSET_SHIFT, s), "constraint / quotient");
        TOYNI_FIB_DT_TRY(toyni_coset_ntt_device(ctx_N_, d_c_, d_c_, 1, COSET_SHIFT, 1, s), "ifft (c_poly)");
        TOYNI_FIB_DT_TRY(toyni_coset_ntt_device(ctx_N_, d_q_, d_qpoly_, 1, COSET_SHIFT, 1, s), "ifft (q_poly)");
        TOYNI_FIB_DT_TRY(toyni_stream_wait_event(s, salts_ready_), "stream order");
        TOYNI_FIB_DT_TRY(toyni_merkle_commit_device(d_q_, salts_quot, N_, d_quot_tree_, s), "quotient commitment");
        TOYNI_FIB_DT_TRY(toyni_stream_wait(s, side_), "stream order");
        // ---- 3./4. Fiat-Shamir and the out-of-domain values, z in device memory ----
        TOYNI_FIB_DT_TRY(toyni_transcript_absorb_device(d_tr_, d_trace_tree_ + root_off, 32, s), "absorb");
        TOYNI_FIB_DT_TRY(toyni_transcript_absorb_device(d_tr_, d_quot_tree_ + root_off, 32, s), "absorb");
        TOYNI_FIB_DT_TRY(toyni_transcript_squeeze_point_device(d_tr_, log_N_, COSET_SHIFT, t_z, s), "derive z");
        const uint32_t mults[3] = {1u, g, mulmod(g, g)};
        TOYNI_FIB_DT_TRY(toyni_poly_eval_dz_device(ctx_N_, d_compact_, ncoef_t, t_z, mults, 3, t_ood, s), "OOD evaluations of T");
        TOYNI_FIB_DT_TRY(toyni_poly_eval_dz_device(ctx_N_, d_qpoly_, N_, t_z, mults, 1, t_ood + 3, s), "OOD evaluation of Q");
        TOYNI_FIB_DT_TRY(toyni_transcript_absorb_fields_device(d_tr_, t_ood, 4, s), "absorb");
        // ---- 5. the constraint check at z and the DEEP layer ----
        TOYNI_FIB_DT_TRY(toyni_fib_deep_dz_device(ctx_N_, d_trace_lde_, d_q_, d_deep_, LOG_BLOWUP, COSET_SHIFT, t_z, t_ood, (uint32_t)n_, t_check, s), "DEEP layer");
        // ---- 6. FRI on the device transcript ----
        TOYNI_FIB_DT_TRY(toyni_merkle_commit_device(d_deep_, salts_deep, N_, d_deep_tree_, s), "DEEP commitment");
        TOYNI_FIB_DT_TRY(toyni_transcript_absorb_device(d_tr_, d_deep_tree_ + root_off, 32, s), "absorb");
        TOYNI_FIB_DT_TRY(toyni_fri_commit_phase_transcript_device(ctx_N_, d_deep_, N_, COSET_SHIFT, final_size_, salted_fri_ ? salts_fri : nullptr, d_tr_, d_layers_,
                                                                  d_fri_trees_, nullptr, s), "FRI commit phase");
        // ---- 7. queries: indices, positions, every opening in one launch ----
        TOYNI_FIB_DT_TRY(toyni_transcript_squeeze_indices_device(d_tr_, NUM_QUERIES, (uint32_t)(N_ / 2), t_idx, s), "query indices");
        uint32_t* pos_trace = d_pos_;                       // 3 per query: T(x), T(g x), T(g^2 x)
        uint32_t* pos_fri = d_pos_ + 3 * NUM_QUERIES;       // `rounds` lists of 2 per query: the DEEP layer, then the folded layers but the final one
        const uint32_t offsets[3] = {0u, (uint32_t)B, (uint32_t)(2 * B)};
        TOYNI_FIB_DT_TRY(toyni_query_rows_device(t_idx, NUM_QUERIES, N_, offsets, 3, pos_trace, s), "query rows");
        TOYNI_FIB_DT_TRY(toyni_fri_query_positions_device(t_idx, NUM_QUERIES, N_, final_size_, pos_fri, s), "query positions");
        {
            std::vector<toyni_merkle_open_group> og;
            uint8_t* rec = d_tail_ + off_records_;
            auto add = [&](const uint8_t* levels, size_t leaves, const uint32_t* values, const uint8_t* salts, const uint32_t* idx, size_t nidx) {
                og.push_back(toyni_merkle_open_group{levels, leaves, values, salts, idx, nidx, rec});
                rec += nidx * toyni_merkle_open_record_bytes(leaves);
            };
            add(d_trace_tree_, N_, d_trace_lde_, salts_trace, pos_trace, 3 * NUM_QUERIES);
            add(d_quot_tree_, N_, d_q_, salts_quot, t_idx, NUM_QUERIES);
            add(d_deep_tree_, N_, d_deep_, salts_deep, pos_fri, 2 * NUM_QUERIES);
            size_t lo = 0, dlo = 0, slo = 0;
            for (size_t li = 0; li + 1 < rounds; ++li) {
                const size_t h = sizes_[li];
                add(d_fri_trees_ + dlo * 32, h, d_layers_ + lo, salts_fri + slo * 16, pos_fri + 2 * NUM_QUERIES * (li + 1), 2 * NUM_QUERIES);
                lo += h; dlo += toyni_merkle_total_digests(h); slo += h;
            }
            if ((size_t)(rec - (d_tail_ + off_records_)) != record_bytes_) return "opening buffers too small";
            TOYNI_FIB_DT_TRY(toyni_merkle_open_groups_device(og.data(), og.size(), s), "openings");
        }
        // ---- the rest of the tail: roots, final layer, the transcript's len and status ----
        TOYNI_FIB_DT_TRY(toyni_memcpy_d2d_async(d_tail_ + off_roots_, d_trace_tree_ + root_off, 32, s), "root");
        TOYNI_FIB_DT_TRY(toyni_memcpy_d2d_async(d_tail_ + off_roots_ + 32, d_quot_tree_ + root_off, 32, s), "root");
        TOYNI_FIB_DT_TRY(toyni_memcpy_d2d_async(d_tail_ + off_roots_ + 64, d_deep_tree_ + root_off, 32, s), "root");
        TOYNI_FIB_DT_TRY(toyni_fri_phase_roots_device(d_fri_trees_, N_ / 2, (unsigned)rounds, d_tail_ + off_roots_ + 96, s), "round roots");
        TOYNI_FIB_DT_TRY(toyni_memcpy_d2d_async(d_tail_ + off_final_, d_layers_ + (fri_words_ - final_size_), 4 * final_size_, s), "final layer");
        TOYNI_FIB_DT_TRY(toyni_memcpy_d2d_async(d_tail_ + off_state_, d_tr_, 8, s), "transcript state");
        traffic_.d2h_bytes += tail_bytes_;
        ++traffic_.d2h_copies;
        TOYNI_FIB_DT_TRY(toyni_memcpy_d2h_async(h_tail(), d_tail_, tail_bytes_, s), "tail down");
        in_flight_ = true;
        return "";
    }

    // The one synchronisation; fills `proof` exactly as Prover::generate_proof does.  "Constraint check at z failed" = the trace is not a
    // Fibonacci column.
    std::string collect(Proof& proof) {
        if (!in_flight_) return "no proof in flight";
        in_flight_ = false;
        int st;
        ++traffic_.synchronisations;
        TOYNI_FIB_DT_TRY(toyni_stream_synchronize(nullptr, stream_), "sync");
        const uint8_t* t = h_tail();
        uint32_t state[2];
        std::memcpy(state, t + off_state_, 8);
        if (state[1] != 0) return std::string("device transcript status: ") + toyni_error_string((int)state[1]);
        uint32_t check;
        std::memcpy(&check, t + off_check_, 4);
        if (check == 0) return "Constraint check at z failed";   // src/fibonacci.rs:173-177
        const size_t rounds = sizes_.size(), half0 = N_ / 2, B = (size_t)1 << LOG_BLOWUP;
        std::memcpy(proof.trace_commitment.data(), t + off_roots_, 32);
        std::memcpy(proof.quotient_commitment.data(), t + off_roots_ + 32, 32);
        uint32_t ood[4];
        std::memcpy(ood, t + off_ood_, 16);
        proof.t_z = ood[0]; proof.t_gz = ood[1]; proof.t_ggz = ood[2]; proof.q_z = ood[3];
        proof.fri_commitments.assign(1 + rounds, {});
        for (size_t k = 0; k < 1 + rounds; ++k) std::memcpy(proof.fri_commitments[k].data(), t + off_roots_ + 64 + 32 * k, 32);
        proof.fri_final_layer.assign(final_size_, 0);
        std::memcpy(proof.fri_final_layer.data(), t + off_final_, 4 * final_size_);
        proof.query_indices.assign(NUM_QUERIES, 0);
        std::memcpy(proof.query_indices.data(), t + off_idx_, 4 * NUM_QUERIES);
        // the groups' index lists, rebuilt from the 44 indices as the device built them (src/fibonacci.rs:249-295)
        proof.opening_groups.clear();
        {
            OpeningGroup gt{N_, true, {}}, gq{N_, true, {}}, gd{N_, true, {}};
            for (uint32_t q : proof.query_indices) {
                gt.indices.push_back(q); gt.indices.push_back((uint32_t)((q + B) % N_)); gt.indices.push_back((uint32_t)((q + 2 * B) % N_));
                gq.indices.push_back(q);
                gd.indices.push_back(q); gd.indices.push_back((uint32_t)(q + half0));
            }
            proof.opening_groups.push_back(gt); proof.opening_groups.push_back(gq); proof.opening_groups.push_back(gd);
            std::vector<uint32_t> cur = proof.query_indices;
            for (size_t li = 0; li + 1 < sizes_.size(); ++li) {
                const size_t half = sizes_[li] / 2;
                OpeningGroup gf{sizes_[li], true, {}};
                for (auto& c : cur) { c = (uint32_t)(c % half); gf.indices.push_back(c); gf.indices.push_back((uint32_t)(c + half)); }
                proof.opening_groups.push_back(gf);
            }
        }
        proof.opening_records.assign(t + off_records_, t + off_records_ + record_bytes_);
        proof.trace_len = n_;
        proof.lde_size = N_;
        return "";
    }
#undef TOYNI_FIB_DT_TRY

    const Traffic& traffic() const { return traffic_; }   // of the last proof: enqueue's copies, and collect's synchronisation once it ran
    size_t folds() const { return sizes_.size(); }
    size_t final_layer_size() const { return final_size_; }

   private:
    size_t positions() const { return NUM_QUERIES * (3 + 2 * sizes_.size()); }
    uint8_t* h_tail() const { return h_pinned_ + 4 * n_ + 64; }
    void release() {
        if (stream_) (void)toyni_stream_synchronize(nullptr, stream_);
        for (void* p : {(void*)d_compact_, (void*)d_trace_lde_, (void*)d_c_, (void*)d_q_, (void*)d_qpoly_, (void*)d_deep_, (void*)d_layers_, (void*)d_trace_tree_,
                        (void*)d_quot_tree_, (void*)d_deep_tree_, (void*)d_fri_trees_, (void*)d_salts_, (void*)d_pos_, (void*)d_tr_, (void*)d_tail_})
            if (p) (void)toyni_free(p);
        if (h_pinned_) (void)toyni_host_free(h_pinned_);
        if (stream_) (void)toyni_stream_destroy(stream_);
        if (side_) (void)toyni_stream_destroy(side_);
        if (salts_ready_) (void)toyni_event_destroy(salts_ready_);
        if (ctx_n_) (void)toyni_ntt_ctx_destroy(ctx_n_);
        if (ctx_N_) (void)toyni_ntt_ctx_destroy(ctx_N_);
    }

    size_t n_, N_ = 0, final_size_ = 0, salted_fri_ = 0, fri_digests_ = 0, fri_words_ = 0, salt_bytes_ = 0;
    size_t off_roots_ = 0, off_z_ = 0, off_ood_ = 0, off_check_ = 0, off_idx_ = 0, off_final_ = 0, off_state_ = 0, off_records_ = 0, record_bytes_ = 0,
           tail_bytes_ = 0;
    unsigned log_n_ = 0, log_N_ = 0, log_c_ = 0;
    int device_;
    bool ready_ = false, in_flight_ = false;
    Traffic traffic_;
    std::vector<size_t> sizes_;       // folded layer sizes N/2 ... final_size
    toyni_ntt_ctx *ctx_n_ = nullptr, *ctx_N_ = nullptr;
    void *stream_ = nullptr, *side_ = nullptr, *salts_ready_ = nullptr;
    uint32_t *d_compact_ = nullptr, *d_trace_lde_ = nullptr, *d_c_ = nullptr, *d_q_ = nullptr, *d_qpoly_ = nullptr, *d_deep_ = nullptr, *d_layers_ = nullptr,
             *d_pos_ = nullptr;
    uint8_t *d_trace_tree_ = nullptr, *d_quot_tree_ = nullptr, *d_deep_tree_ = nullptr, *d_fri_trees_ = nullptr, *d_salts_ = nullptr, *d_tail_ = nullptr;
    toyni_transcript* d_tr_ = nullptr;
    uint8_t* h_pinned_ = nullptr;
};

}  // namespace fib
}  // namespace toyni
