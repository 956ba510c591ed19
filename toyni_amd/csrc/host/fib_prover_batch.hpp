// The stream-ordered Fibonacci prover of fib_prover_dt.hpp for `batch` traces of one length in ONE chain of launches (include/toyni_hip.h
// 3r, 3s): StreamProver's chain step for step, every call replaced by its batch form, so `batch` proofs cost the number of launches one
// proof costs, with one upload phase (traces, keys, transcript heads), one download and one synchronisation.  Proof b is byte for byte
// what StreamProver writes for trace b under key b.
// Every per-proof array is one buffer with a stride; the tail buffer is `batch` tails of StreamProver's layout, tail_stride (a multiple
// of 16) apart, downloaded in one copy.  One stream: the side stream of StreamProver hid one proof's trace tree behind its quotient,
// and a batch fills the chip itself.
//   step                                         call
//   upload traces, keys, transcript heads        toyni_memcpy_h2d_async x 3, toyni_copy_rows_device (heads into the 1 KiB slots)
//   salts                                        toyni_chacha20_fill_batch_device            (3s)
//   INTT; spread into the coefficient slots      toyni_ntt_device(batch), toyni_memset_async, toyni_copy_rows_device
//   mask                                         toyni_mask_poly_batch_device                (3s)
//   LDE; trace trees                             toyni_lde_device(batch), toyni_merkle_commit_batch_device (3r)
//   quotient, two INTTs, quotient trees          toyni_fib_quotient_batch_device (3s), toyni_coset_ntt_device(batch), toyni_merkle_commit_batch_device
//   absorb both roots where they lie             toyni_transcript_absorb_batch_device        (3r)
//   z                                            toyni_transcript_squeeze_point_batch_device (3s)
//   T(z), T(g z), T(g^2 z), Q(z)                 toyni_poly_eval_dz_batch_device x 2         (3s)
//   absorb the four values                       toyni_transcript_absorb_fields_batch_device (3s)
//   constraint check at z, DEEP layer            toyni_fib_deep_dz_batch_device              (3s)
//   DEEP trees, absorb their roots               toyni_merkle_commit_batch_device, toyni_transcript_absorb_batch_device
//   fold loop                                    toyni_fri_commit_phase_transcript_batch_device (3r)
//   queries                                      toyni_transcript_squeeze_indices_batch_device, toyni_fri_query_positions_batch_device (3r),
//                                                toyni_query_rows_batch_device (3s), toyni_merkle_open_groups_device (32 groups a launch)
//   roots, final layers, transcript states       toyni_copy_rows_device x 5, toyni_fri_phase_roots_batch_device (3s)
//   one download                                 toyni_memcpy_d2h_async
#pragma once
#include "fib_prover_dt.hpp"

namespace toyni {
namespace fib {

class BatchStreamProver {
   public:
    BatchStreamProver(size_t trace_len, size_t batch, int device = -1) : n_(trace_len), batch_(batch), device_(device) {}
    ~BatchStreamProver() { release(); }
    BatchStreamProver(const BatchStreamProver&) = delete;
    BatchStreamProver& operator=(const BatchStreamProver&) = delete;

    using Traffic = StreamProver::Traffic;   // of the whole batch

#define TOYNI_FIB_B_TRY(expr, what) do { st = (expr); if (st) return std::string(what) + ": " + toyni_error_string(st); } while (0)
    // Allocates every buffer of the batch once and builds the two contexts (which blocks).  "" = ok.
    std::string prepare() {
        if (ready_) return "";
        if (n_ < 8 || (n_ & (n_ - 1)) || n_ > ((size_t)1 << 22)) return "trace length must be a power of two in [8, 2^22]";
        if (batch_ < 1 || batch_ > 65535) return "batch must lie in [1, 65535]";
        log_n_ = 0;
        while (((size_t)1 << log_n_) < n_) ++log_n_;
        N_ = n_ << LOG_BLOWUP;
        log_N_ = log_n_ + LOG_BLOWUP;
        log_c_ = 0;
        while (((size_t)1 << log_c_) < n_ + MASK_DEGREE) ++log_c_;
        C_ = (size_t)1 << log_c_;
        final_size_ = N_ / C_;
        if (final_size_ < 1 || log_c_ > log_N_) return "trace too short for this blow-up";
        sizes_.clear();
        for (size_t m = N_ / 2; m >= final_size_; m /= 2) { sizes_.push_back(m); if (m == final_size_) break; }
        salted_fri_ = fri_digests_ = fri_words_ = 0;
        for (size_t h : sizes_) { if (h != final_size_) salted_fri_ += h; fri_digests_ += toyni_merkle_total_digests(h); fri_words_ += h; }
        // one proof's tail: StreamProver's layout
        const size_t rounds = sizes_.size();
        off_roots_ = 0;
        off_z_ = 32 * (3 + rounds);
        off_ood_ = off_z_ + 4;
        off_check_ = off_ood_ + 16;
        off_idx_ = off_check_ + 4;
        off_final_ = off_idx_ + 4 * NUM_QUERIES;
        off_state_ = off_final_ + 4 * final_size_;
        off_records_ = (off_state_ + 8 + 7) & ~(size_t)7;
        record_bytes_ = NUM_QUERIES * (3 + 1 + 2) * toyni_merkle_open_record_bytes(N_);
        for (size_t li = 0; li + 1 < sizes_.size(); ++li) record_bytes_ += 2 * NUM_QUERIES * toyni_merkle_open_record_bytes(sizes_[li]);
        tail_bytes_ = off_records_ + record_bytes_;
        tail_stride_ = (tail_bytes_ + 15) & ~(size_t)15;
        tree_stride_ = toyni_merkle_total_digests(N_) * 32;
        salt_stride_ = ((3 * N_ + salted_fri_) * 16 + 63) & ~(size_t)63;
        pos_stride_ = NUM_QUERIES * (3 + 2 * rounds);
        int st;
        TOYNI_FIB_B_TRY(toyni_ntt_ctx_create((uint32_t)n_, device_, &ctx_n_), "trace-domain context");
        TOYNI_FIB_B_TRY(toyni_ntt_ctx_create((uint32_t)N_, device_, &ctx_N_), "LDE-domain context");
        TOYNI_FIB_B_TRY(toyni_stream_create(&stream_, toyni_ntt_ctx_device(ctx_N_)), "stream");
        const size_t B = batch_;
        struct { void** p; size_t bytes; } bufs[] = {
            {(void**)&d_traces_, 4 * n_ * B}, {(void**)&d_compact_, 4 * C_ * B}, {(void**)&d_trace_lde_, 4 * N_ * B}, {(void**)&d_c_, 4 * N_ * B},
            {(void**)&d_q_, 4 * N_ * B}, {(void**)&d_qpoly_, 4 * N_ * B}, {(void**)&d_deep_, 4 * N_ * B}, {(void**)&d_layers_, 4 * fri_words_ * B},
            {(void**)&d_trace_tree_, tree_stride_ * B}, {(void**)&d_quot_tree_, tree_stride_ * B}, {(void**)&d_deep_tree_, tree_stride_ * B},
            {(void**)&d_fri_trees_, fri_digests_ * 32 * B}, {(void**)&d_salts_, salt_stride_ * B}, {(void**)&d_pos_, 4 * pos_stride_ * B},
            {(void**)&d_tr_, sizeof(toyni_transcript) * B}, {(void**)&d_keys_, 32 * B}, {(void**)&d_heads_, 32 * B}, {(void**)&d_tail_, tail_stride_ * B}};
        for (auto& b : bufs) TOYNI_FIB_B_TRY(toyni_malloc(b.p, b.bytes), "device allocation");
        TOYNI_FIB_B_TRY(toyni_host_alloc((void**)&h_pinned_, (4 * n_ + 64) * B + tail_stride_ * B), "pinned staging");
        ready_ = true;
        return "";
    }

    // Enqueues the whole batch, from the uploads to the copy of the tails into pinned memory, and returns.  traces: batch x n words, trace
    // b at traces + b n; keys: batch x 32 bytes.  Both are copied before the call returns.  One batch is in flight at a time.
    std::string enqueue(const uint32_t* traces, const uint8_t* keys) {
        if (in_flight_) return "a batch is already in flight";
        std::string err = prepare();
        if (!err.empty()) return err;
        int st;
        void* s = stream_;
        traffic_ = Traffic{};
        auto up = [&](void* d, const void* h, size_t bytes) { traffic_.h2d_bytes += bytes; ++traffic_.h2d_copies; return toyni_memcpy_h2d_async(d, h, bytes, s); };
        const uint32_t g = root_of_unity(log_n_);
        const size_t B = (size_t)1 << LOG_BLOWUP, rounds = sizes_.size(), nb = batch_;
        uint8_t* h_traces = h_pinned_;
        uint8_t* h_keys = h_pinned_ + 4 * n_ * nb;
        uint8_t* h_heads = h_keys + 32 * nb;
        const size_t ts = tail_stride_ / 4;                             // the tail stride in words
        uint32_t* t_z = reinterpret_cast<uint32_t*>(d_tail_ + off_z_);
        uint32_t* t_ood = reinterpret_cast<uint32_t*>(d_tail_ + off_ood_);
        uint32_t* t_check = reinterpret_cast<uint32_t*>(d_tail_ + off_check_);
        uint32_t* t_idx = reinterpret_cast<uint32_t*>(d_tail_ + off_idx_);
        const uint8_t* salts_trace = d_salts_;
        const uint8_t* salts_quot = d_salts_ + 16 * N_;
        const uint8_t* salts_deep = d_salts_ + 32 * N_;
        const uint8_t* salts_fri = d_salts_ + 48 * N_;
        const size_t root_off = tree_stride_ - 32;

        // ---- the one upload phase ----
        std::memcpy(h_traces, traces, 4 * n_ * nb);
        std::memcpy(h_keys, keys, 32 * nb);
        for (size_t b = 0; b < nb; ++b) {   // every transcript starts as the reference's does (src/transcript.rs:12-17): len = 14, status = 0
            uint8_t* h = h_heads + 32 * b;
            std::memset(h, 0, 32);
            const uint32_t len = 14;
            std::memcpy(h, &len, 4);
            std::memcpy(h + 16, "toyni-stark-v1", 14);
        }
        TOYNI_FIB_B_TRY(up(d_traces_, h_traces, 4 * n_ * nb), "trace upload");
        TOYNI_FIB_B_TRY(up(d_keys_, h_keys, 32 * nb), "key upload");
        TOYNI_FIB_B_TRY(up(d_heads_, h_heads, 32 * nb), "transcript upload");
        TOYNI_FIB_B_TRY(toyni_copy_rows_device(d_tr_, sizeof(toyni_transcript), d_heads_, 32, 32, nb, s), "transcript heads");
        TOYNI_FIB_B_TRY(toyni_chacha20_fill_batch_device(d_salts_, salt_stride_, salt_stride_, d_keys_, 0, nb, s), "salts");
        // ---- 1. trace polynomials, mask, LDE, trace trees ----
        TOYNI_FIB_B_TRY(toyni_ntt_device(ctx_n_, d_traces_, d_traces_, nb, 1, s), "interpolation (INTT)");
        TOYNI_FIB_B_TRY(toyni_memset_async(d_compact_, 0, 4 * C_ * nb, s), "clear");
        TOYNI_FIB_B_TRY(toyni_copy_rows_device(d_compact_, 4 * C_, d_traces_, 4 * n_, 4 * n_, nb, s), "coefficient slots");
        TOYNI_FIB_B_TRY(toyni_mask_poly_batch_device(d_compact_, C_, n_, MASK_DEGREE, d_keys_, 1, nb, s), "mask");   // nonce 1 (nonce 0 is the salts')
        const size_t ncoef_t = n_ + MASK_DEGREE;
        TOYNI_FIB_B_TRY(toyni_lde_device(ctx_N_, d_compact_, d_trace_lde_, nb, log_N_ - log_c_, COSET_SHIFT, s), "LDE");
        TOYNI_FIB_B_TRY(toyni_merkle_commit_batch_device(d_trace_lde_, N_, salts_trace, salt_stride_, N_, nb, d_trace_tree_, tree_stride_, s), "trace commitment");
        // ---- 2. constraint, quotient, quotient trees ----
        TOYNI_FIB_B_TRY(toyni_fib_quotient_batch_device(ctx_N_, d_trace_lde_, N_, d_c_, N_, d_q_, N_, LOG_BLOWUP, COSET_SHIFT, nb, s), "constraint / quotient");
        TOYNI_FIB_B_TRY(toyni_coset_ntt_device(ctx_N_, d_c_, d_c_, nb, COSET_SHIFT, 1, s), "ifft (c_poly)");
        TOYNI_FIB_B_TRY(toyni_coset_ntt_device(ctx_N_, d_q_, d_qpoly_, nb, COSET_SHIFT, 1, s), "ifft (q_poly)");
        TOYNI_FIB_B_TRY(toyni_merkle_commit_batch_device(d_q_, N_, salts_quot, salt_stride_, N_, nb, d_quot_tree_, tree_stride_, s), "quotient commitment");
        // ---- 3./4. Fiat-Shamir and the out-of-domain values, every z in device memory ----
        TOYNI_FIB_B_TRY(toyni_transcript_absorb_batch_device(d_tr_, nb, d_trace_tree_ + root_off, tree_stride_, 32, s), "absorb");
        TOYNI_FIB_B_TRY(toyni_transcript_absorb_batch_device(d_tr_, nb, d_quot_tree_ + root_off, tree_stride_, 32, s), "absorb");
        TOYNI_FIB_B_TRY(toyni_transcript_squeeze_point_batch_device(d_tr_, nb, log_N_, COSET_SHIFT, t_z, ts, s), "derive z");
        const uint32_t mults[3] = {1u, g, mulmod(g, g)};
        TOYNI_FIB_B_TRY(toyni_poly_eval_dz_batch_device(ctx_N_, d_compact_, C_, ncoef_t, t_z, ts, mults, 3, nb, t_ood, ts, s), "OOD evaluations of T");
        TOYNI_FIB_B_TRY(toyni_poly_eval_dz_batch_device(ctx_N_, d_qpoly_, N_, N_, t_z, ts, mults, 1, nb, t_ood + 3, ts, s), "OOD evaluation of Q");
        TOYNI_FIB_B_TRY(toyni_transcript_absorb_fields_batch_device(d_tr_, nb, t_ood, ts, 4, s), "absorb");
        // ---- 5. the constraint checks at z and the DEEP layers ----
        TOYNI_FIB_B_TRY(toyni_fib_deep_dz_batch_device(ctx_N_, d_trace_lde_, N_, d_q_, N_, d_deep_, N_, LOG_BLOWUP, COSET_SHIFT, t_z, ts, t_ood, ts, (uint32_t)n_,
                                                       t_check, ts, nb, s), "DEEP layer");
        // ---- 6. FRI on the device transcripts ----
        TOYNI_FIB_B_TRY(toyni_merkle_commit_batch_device(d_deep_, N_, salts_deep, salt_stride_, N_, nb, d_deep_tree_, tree_stride_, s), "DEEP commitment");
        TOYNI_FIB_B_TRY(toyni_transcript_absorb_batch_device(d_tr_, nb, d_deep_tree_ + root_off, tree_stride_, 32, s), "absorb");
        TOYNI_FIB_B_TRY(toyni_fri_commit_phase_transcript_batch_device(ctx_N_, d_deep_, N_, N_, COSET_SHIFT, final_size_, salted_fri_ ? salts_fri : nullptr,
                                                                       salt_stride_, d_tr_, nb, d_layers_, fri_words_, d_fri_trees_, fri_digests_ * 32, nullptr, 0, s),
                        "FRI commit phase");
        // ---- 7. queries: indices, positions, the openings of all proofs ----
        TOYNI_FIB_B_TRY(toyni_transcript_squeeze_indices_batch_device(d_tr_, nb, NUM_QUERIES, (uint32_t)(N_ / 2), t_idx, ts, s), "query indices");
        uint32_t* pos_trace = d_pos_;                       // per proof 3 per query: T(x), T(g x), T(g^2 x)
        uint32_t* pos_fri = d_pos_ + 3 * NUM_QUERIES;       // then `rounds` lists of 2 per query
        const uint32_t offsets[3] = {0u, (uint32_t)B, (uint32_t)(2 * B)};
        TOYNI_FIB_B_TRY(toyni_query_rows_batch_device(t_idx, ts, NUM_QUERIES, N_, offsets, 3, nb, pos_trace, pos_stride_, s), "query rows");
        TOYNI_FIB_B_TRY(toyni_fri_query_positions_batch_device(t_idx, ts, NUM_QUERIES, N_, final_size_, nb, pos_fri, pos_stride_, s), "query positions");
        {
            std::vector<toyni_merkle_open_group> og;
            og.reserve(nb * (3 + rounds));
            for (size_t b = 0; b < nb; ++b) {
                uint8_t* rec0 = d_tail_ + b * tail_stride_ + off_records_;
                uint8_t* rec = rec0;
                auto add = [&](const uint8_t* levels, size_t leaves, const uint32_t* values, const uint8_t* salts, const uint32_t* idx, size_t nidx) {
                    og.push_back(toyni_merkle_open_group{levels, leaves, values, salts, idx, nidx, rec});
                    rec += nidx * toyni_merkle_open_record_bytes(leaves);
                };
                const size_t so = b * salt_stride_, to = b * tree_stride_, po = b * pos_stride_;
                add(d_trace_tree_ + to, N_, d_trace_lde_ + b * N_, salts_trace + so, pos_trace + po, 3 * NUM_QUERIES);
                add(d_quot_tree_ + to, N_, d_q_ + b * N_, salts_quot + so, t_idx + b * ts, NUM_QUERIES);
                add(d_deep_tree_ + to, N_, d_deep_ + b * N_, salts_deep + so, pos_fri + po, 2 * NUM_QUERIES);
                size_t lo = 0, dlo = 0, slo = 0;
                for (size_t li = 0; li + 1 < rounds; ++li) {
                    const size_t h = sizes_[li];
                    add(d_fri_trees_ + (b * fri_digests_ + dlo) * 32, h, d_layers_ + b * fri_words_ + lo, salts_fri + so + slo * 16,
                        pos_fri + po + 2 * NUM_QUERIES * (li + 1), 2 * NUM_QUERIES);
                    lo += h; dlo += toyni_merkle_total_digests(h); slo += h;
                }
                if ((size_t)(rec - rec0) != record_bytes_) return "opening buffers too small";
            }
            TOYNI_FIB_B_TRY(toyni_merkle_open_groups_device(og.data(), og.size(), s), "openings");
        }
        // ---- the rest of every tail: roots, final layer, the transcript's len and status ----
        TOYNI_FIB_B_TRY(toyni_copy_rows_device(d_tail_ + off_roots_, tail_stride_, d_trace_tree_ + root_off, tree_stride_, 32, nb, s), "root");
        TOYNI_FIB_B_TRY(toyni_copy_rows_device(d_tail_ + off_roots_ + 32, tail_stride_, d_quot_tree_ + root_off, tree_stride_, 32, nb, s), "root");
        TOYNI_FIB_B_TRY(toyni_copy_rows_device(d_tail_ + off_roots_ + 64, tail_stride_, d_deep_tree_ + root_off, tree_stride_, 32, nb, s), "root");
        TOYNI_FIB_B_TRY(toyni_fri_phase_roots_batch_device(d_fri_trees_, fri_digests_ * 32, N_ / 2, (unsigned)rounds, nb, d_tail_ + off_roots_ + 96, tail_stride_, s),
                        "round roots");
        TOYNI_FIB_B_TRY(toyni_copy_rows_device(d_tail_ + off_final_, tail_stride_, d_layers_ + (fri_words_ - final_size_), 4 * fri_words_, 4 * final_size_, nb, s),
                        "final layer");
        TOYNI_FIB_B_TRY(toyni_copy_rows_device(d_tail_ + off_state_, tail_stride_, d_tr_, sizeof(toyni_transcript), 8, nb, s), "transcript state");
        traffic_.d2h_bytes += tail_stride_ * nb;
        ++traffic_.d2h_copies;
        TOYNI_FIB_B_TRY(toyni_memcpy_d2h_async(h_tail(), d_tail_, tail_stride_ * nb, s), "tail down");
        in_flight_ = true;
        return "";
    }

    // The one synchronisation.  proofs[b] is filled exactly as StreamProver::collect fills it and errors[b] is "", or errors[b] names
    // what went wrong with proof b alone ("Constraint check at z failed", a transcript status) and proofs[b] is left empty: the
    // outcomes are independent.  The return value is for what concerns the whole batch.
    std::string collect(std::vector<Proof>& proofs, std::vector<std::string>& errors) {
        if (!in_flight_) return "no batch in flight";
        in_flight_ = false;
        int st;
        ++traffic_.synchronisations;
        TOYNI_FIB_B_TRY(toyni_stream_synchronize(nullptr, stream_), "sync");
        proofs.assign(batch_, Proof{});
        errors.assign(batch_, "");
        const size_t rounds = sizes_.size(), half0 = N_ / 2, B = (size_t)1 << LOG_BLOWUP;
        for (size_t b = 0; b < batch_; ++b) {
            const uint8_t* t = h_tail() + b * tail_stride_;
            Proof& proof = proofs[b];
            uint32_t state[2];
            std::memcpy(state, t + off_state_, 8);
            if (state[1] != 0) { errors[b] = std::string("device transcript status: ") + toyni_error_string((int)state[1]); continue; }
            uint32_t check;
            std::memcpy(&check, t + off_check_, 4);
            if (check == 0) { errors[b] = "Constraint check at z failed"; continue; }   // src/fibonacci.rs:173-177
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
            proof.opening_records.assign(t + off_records_, t + off_records_ + record_bytes_);
            proof.trace_len = n_;
            proof.lde_size = N_;
        }
        return "";
    }
#undef TOYNI_FIB_B_TRY

    const Traffic& traffic() const { return traffic_; }   // of the last batch: enqueue's copies, and collect's synchronisation once it ran
    size_t batch() const { return batch_; }
    size_t folds() const { return sizes_.size(); }
    size_t final_layer_size() const { return final_size_; }
    // launches of toyni_merkle_open_groups_device per batch: it takes 32 groups a launch
    size_t open_launches() const { return (batch_ * (2 + sizes_.size()) + 31) / 32; }

   private:
    uint8_t* h_tail() const { return h_pinned_ + (4 * n_ + 64) * batch_; }
    void release() {
        if (stream_) (void)toyni_stream_synchronize(nullptr, stream_);
        for (void* p : {(void*)d_traces_, (void*)d_compact_, (void*)d_trace_lde_, (void*)d_c_, (void*)d_q_, (void*)d_qpoly_, (void*)d_deep_, (void*)d_layers_,
                        (void*)d_trace_tree_, (void*)d_quot_tree_, (void*)d_deep_tree_, (void*)d_fri_trees_, (void*)d_salts_, (void*)d_pos_, (void*)d_tr_,
                        (void*)d_keys_, (void*)d_heads_, (void*)d_tail_})
            if (p) (void)toyni_free(p);
        if (h_pinned_) (void)toyni_host_free(h_pinned_);
        if (stream_) (void)toyni_stream_destroy(stream_);
        if (ctx_n_) (void)toyni_ntt_ctx_destroy(ctx_n_);
        if (ctx_N_) (void)toyni_ntt_ctx_destroy(ctx_N_);
    }

    size_t n_, batch_, N_ = 0, C_ = 0, final_size_ = 0, salted_fri_ = 0, fri_digests_ = 0, fri_words_ = 0;
    size_t off_roots_ = 0, off_z_ = 0, off_ood_ = 0, off_check_ = 0, off_idx_ = 0, off_final_ = 0, off_state_ = 0, off_records_ = 0, record_bytes_ = 0,
           tail_bytes_ = 0, tail_stride_ = 0, tree_stride_ = 0, salt_stride_ = 0, pos_stride_ = 0;
    unsigned log_n_ = 0, log_N_ = 0, log_c_ = 0;
    int device_;
    bool ready_ = false, in_flight_ = false;
    Traffic traffic_;
    std::vector<size_t> sizes_;       // folded layer sizes N/2 ... final_size
    toyni_ntt_ctx *ctx_n_ = nullptr, *ctx_N_ = nullptr;
    void* stream_ = nullptr;
    uint32_t *d_traces_ = nullptr, *d_compact_ = nullptr, *d_trace_lde_ = nullptr, *d_c_ = nullptr, *d_q_ = nullptr, *d_qpoly_ = nullptr, *d_deep_ = nullptr,
             *d_layers_ = nullptr, *d_pos_ = nullptr;
    uint8_t *d_trace_tree_ = nullptr, *d_quot_tree_ = nullptr, *d_deep_tree_ = nullptr, *d_fri_trees_ = nullptr, *d_salts_ = nullptr, *d_tail_ = nullptr,
            *d_keys_ = nullptr, *d_heads_ = nullptr;
    toyni_transcript* d_tr_ = nullptr;
    uint8_t* h_pinned_ = nullptr;
};

}  // namespace fib
}  // namespace toyni
