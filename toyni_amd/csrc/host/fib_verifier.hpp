// C++ caller of the device verifier (include/toyni_hip.h 3t): packs `batch` proofs of one trace length -- toyni::fib::Proof, what the
// three provers of this directory fill -- into proof images, uploads them ONCE, enqueues toyni_fib_verify_batch_device, downloads the
// 4 x batch verdict bytes ONCE and synchronises ONCE.  The counterpart of `StarkVerifier::verify` (src/verifier.rs:14-232) for a
// caller that holds many proofs: an aggregator, or a node that checks proofs before it relays them.
// pack_proof refuses on the host, under the reference's names, what the reference refuses on a proof's structure (lde_size,
// fold_count, final_size, query_count, fri_opening_count): an image of the right size cannot carry those defects.  It reads nothing
// beyond the vectors' sizes, whatever those are.
// No CPU fallback: the checks themselves run on the device only.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "fib_prover.hpp"

namespace toyni {
namespace fib {

// "" and the image written (layout.image_bytes bytes, every byte), or the name of the structural refusal and the image untouched
inline std::string pack_proof(const Proof& p, const toyni_fib_proof_layout& l, uint8_t* image) {
    if (p.trace_len != l.trace_len || p.lde_size != l.lde_size) return "lde_size";
    if (p.fri_commitments.size() != l.folds + 1) return "fold_count";
    if (p.fri_final_layer.size() != l.final_size) return "final_size";
    if (p.query_indices.size() != l.queries) return "query_count";
    size_t want = 0;
    for (size_t g = 0; g < l.ngroups; ++g) want += l.group_records[g] * l.group_record_bytes[g];
    if (p.opening_records.size() != want) return "fri_opening_count";
    std::memset(image, 0, l.image_bytes);
    std::memcpy(image + l.roots_offset, p.trace_commitment.data(), 32);
    std::memcpy(image + l.roots_offset + 32, p.quotient_commitment.data(), 32);
    for (size_t k = 0; k < p.fri_commitments.size(); ++k) std::memcpy(image + l.roots_offset + 32 * (2 + k), p.fri_commitments[k].data(), 32);
    const uint32_t ood[4] = {p.t_z, p.t_gz, p.t_ggz, p.q_z};
    std::memcpy(image + l.ood_offset, ood, 16);
    std::memcpy(image + l.indices_offset, p.query_indices.data(), 4 * p.query_indices.size());
    std::memcpy(image + l.final_offset, p.fri_final_layer.data(), 4 * p.fri_final_layer.size());
    if (want) std::memcpy(image + l.records_offset, p.opening_records.data(), want);
    return "";
}

class BatchVerifier {
   public:
    BatchVerifier(size_t trace_len, size_t batch, int device = -1) : n_(trace_len), batch_(batch), device_(device) {}
    ~BatchVerifier() { release(); }
    BatchVerifier(const BatchVerifier&) = delete;
    BatchVerifier& operator=(const BatchVerifier&) = delete;

    struct Traffic { size_t h2d_bytes = 0, d2h_bytes = 0, h2d_copies = 0, d2h_copies = 0, synchronisations = 0; };

#define TOYNI_FIB_V_TRY(expr, what) do { st = (expr); if (st) return std::string(what) + ": " + toyni_error_string(st); } while (0)
    // Allocates the device buffers and the pinned staging once and builds the context.  "" = ok.
    std::string prepare() {
        if (ready_) return "";
        if (batch_ < 1 || batch_ > 65535) return "batch takes 1 to 65535";
        int st;
        TOYNI_FIB_V_TRY(toyni_fib_proof_layout_of(n_, &layout_), "proof layout");
        stride_ = layout_.image_bytes;
        TOYNI_FIB_V_TRY(toyni_ntt_ctx_create((uint32_t)layout_.lde_size, device_, &ctx_), "LDE-domain context");
        TOYNI_FIB_V_TRY(toyni_stream_create(&stream_, toyni_ntt_ctx_device(ctx_)), "stream");
        TOYNI_FIB_V_TRY(toyni_malloc((void**)&d_images_, batch_ * stride_), "device allocation");
        TOYNI_FIB_V_TRY(toyni_malloc((void**)&d_work_, toyni_fib_verify_work_bytes(n_, batch_)), "device allocation");
        TOYNI_FIB_V_TRY(toyni_malloc((void**)&d_verdicts_, 4 * batch_), "device allocation");
        TOYNI_FIB_V_TRY(toyni_host_alloc((void**)&h_pinned_, batch_ * stride_ + 4 * batch_), "pinned staging");
        ready_ = true;
        return "";
    }

    // proofs: exactly `batch` of them.  Returns "" and the verdict words (include/toyni_hip.h 3t), or what failed: "proof <b>: <name>"
    // for a structural refusal (nothing is enqueued then), or the failing call.
    std::string verify(const std::vector<Proof>& proofs, std::vector<uint32_t>& verdicts) {
        std::string err = prepare();
        if (!err.empty()) return err;
        if (proofs.size() != batch_) return "the verifier was built for " + std::to_string(batch_) + " proofs";
        for (size_t b = 0; b < batch_; ++b) {
            const std::string why = pack_proof(proofs[b], layout_, h_pinned_ + b * stride_);
            if (!why.empty()) return "proof " + std::to_string(b) + ": " + why;
        }
        int st;
        traffic_ = Traffic{};
        uint32_t* h_verdicts = reinterpret_cast<uint32_t*>(h_pinned_ + batch_ * stride_);
        traffic_.h2d_bytes += batch_ * stride_;
        ++traffic_.h2d_copies;
        TOYNI_FIB_V_TRY(toyni_memcpy_h2d_async(d_images_, h_pinned_, batch_ * stride_, stream_), "image upload");
        TOYNI_FIB_V_TRY(toyni_fib_verify_batch_device(ctx_, d_images_, stride_, n_, batch_, d_work_, d_verdicts_, stream_), "verification");
        traffic_.d2h_bytes += 4 * batch_;
        ++traffic_.d2h_copies;
        TOYNI_FIB_V_TRY(toyni_memcpy_d2h_async(h_verdicts, d_verdicts_, 4 * batch_, stream_), "verdict download");
        ++traffic_.synchronisations;
        TOYNI_FIB_V_TRY(toyni_stream_synchronize(nullptr, stream_), "sync");
        verdicts.assign(h_verdicts, h_verdicts + batch_);
        return "";
    }
#undef TOYNI_FIB_V_TRY

    const Traffic& traffic() const { return traffic_; }   // of the last batch
    const toyni_fib_proof_layout& layout() const { return layout_; }
    size_t batch() const { return batch_; }

   private:
    void release() {
        for (void* p : {(void*)d_images_, d_work_, (void*)d_verdicts_})
            if (p) (void)toyni_free(p);
        if (h_pinned_) (void)toyni_host_free(h_pinned_);
        if (stream_) (void)toyni_stream_destroy(stream_);
        if (ctx_) (void)toyni_ntt_ctx_destroy(ctx_);
    }

    size_t n_, batch_, stride_ = 0;
    int device_;
    bool ready_ = false;
    toyni_fib_proof_layout layout_{};
    Traffic traffic_;
    toyni_ntt_ctx* ctx_ = nullptr;
    void* stream_ = nullptr;
    uint8_t* d_images_ = nullptr;
    void* d_work_ = nullptr;
    uint32_t* d_verdicts_ = nullptr;
    uint8_t* h_pinned_ = nullptr;
};

}  // namespace fib
}  // namespace toyni
