// Section 3t of include/toyni_hip.h -- verifying a batch of Fibonacci proofs on the device -- as a translation unit of its own, linked
// into libtoyni_hip.so next to toyni_hip.hip and batch/toyni_hip_fib_batch.hip: five kernels and their entry points.  It is separate
// for the reason 3s is: the builds of the other two units stay, symbol for symbol and resource line for resource line, what they were;
// the remarks of this unit are kept beside the library in a file of their own.
// The device bodies are the TOYNI_HD functions of verify_kernels.hpp.  Under TOYNI_KERNEL_TEXT_ONLY (tests/sim) only the kernels are
// compiled.  What the entry points need of a context comes through toyni_internal (defined in toyni_hip.hip, not part of the C ABI).
#ifndef TOYNI_KERNEL_TEXT_ONLY
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>

#include "toyni_hip.h"

namespace toyni_internal {
int ctx_log_n(const toyni_ntt_ctx* c);
bool note_launch(const void* kernel);
int ctx_enqueue(toyni_ntt_ctx* c, void* stream, size_t words, int (*enqueue)(void* user, uint32_t* d_words), void* user);
}  // namespace toyni_internal

// every launch site files its kernel in toyni_hip.hip's registry (toyni_launched_kernels), as that unit's sites do
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...)                                      \
    do {                                                                                                 \
        static std::atomic<bool> _toyni_site_seen{false};                                                \
        if (!_toyni_site_seen.load(std::memory_order_acquire)) {                                         \
            if (toyni_internal::note_launch(reinterpret_cast<const void*>(kernel)))                      \
                _toyni_site_seen.store(true, std::memory_order_release);                                 \
        }                                                                                                \
        kernel<<<(grid), (block), (shmem), (stream)>>>(__VA_ARGS__);                                     \
    } while (0)
#endif  // TOYNI_KERNEL_TEXT_ONLY

#include "verify_kernels.hpp"

using namespace toyni;

// ---- the kernels ----
// a. transcript replay: one wave per proof, one lane of it active -- the chain is serial by definition
__global__ void __launch_bounds__(VERIFY_WAVE) fib_verify_replay_kernel(const FibVerifyArgs a, const uint8_t* __restrict__ images, uint32_t* __restrict__ work) {
    const size_t pb = blockIdx.x;   // the proof: a block coordinate
    if (threadIdx.x != 0) return;
    fib_verify_replay(a, images + pb * a.image_stride, work + pb * a.work_stride);
}
// b. / c. the global checks and the positions: one wave per proof
__global__ void __launch_bounds__(VERIFY_WAVE) fib_verify_global_kernel(const FibVerifyArgs a, const uint8_t* __restrict__ images, uint32_t* __restrict__ work) {
    __shared__ Digest tree[FIBV_MAX_FINAL];
    __shared__ uint32_t flag;
    const size_t pb = blockIdx.x;   // the proof: a block coordinate
    // "some lane saw it": through one LDS word.  The LDS operations of a wave execute in program order, so clear / set / read need no
    // barrier, only the compiler kept from moving them (as in transcript_squeeze_indices_kernel).
    const auto any_lane = [](bool hit) {
        if (threadIdx.x == 0) flag = 0u;
        TOYNI_WAVE_ORDER();
        if (hit) flag = 1u;
        TOYNI_WAVE_ORDER();
        const uint32_t some = flag;
        TOYNI_WAVE_ORDER();
        return some != 0u;
    };
    fib_verify_global(a, images + pb * a.image_stride, work + pb * a.work_stride, tree, threadIdx.x, VERIFY_WAVE, any_lane);
}
// d. one thread per (group, record, proof), the proof index fastest
__global__ void __launch_bounds__(256) merkle_verify_records_batch_kernel(const MerkleVerifyGroups a) {
    const uint64_t total = a.first[a.ngroups] * a.batch, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) merkle_verify_item(a, t);
}
// e. one thread per (proof, query): one wave per proof, 44 lanes of it active
__global__ void __launch_bounds__(VERIFY_WAVE) fib_verify_query_kernel(const FibVerifyArgs a, const uint8_t* __restrict__ images, uint32_t* __restrict__ work) {
    const size_t pb = blockIdx.x;   // the proof: a block coordinate
    uint32_t* w = work + pb * a.work_stride;
    if (threadIdx.x < FIBV_QUERIES) w[FIBV_W_QKEYS + threadIdx.x] = fib_verify_query(a, images + pb * a.image_stride, w, threadIdx.x);
}
// f. one wave per proof, one lane of it active: 45 words
__global__ void __launch_bounds__(VERIFY_WAVE) fib_verify_verdict_kernel(const uint32_t* __restrict__ work, size_t work_stride, uint32_t* __restrict__ verdicts) {
    const size_t pb = blockIdx.x;   // the proof: a block coordinate
    if (threadIdx.x == 0) verdicts[pb] = fib_verify_verdict(work + pb * work_stride);
}

#ifndef TOYNI_KERNEL_TEXT_ONLY
// ---- the entry points ----
namespace {
constexpr size_t BATCH_MAX = 65535;   // the proof index is a block coordinate
bool batch_ok(size_t batch) { return batch >= 1 && batch <= BATCH_MAX; }
bool trace_len_ok(size_t n) { return n >= 8 && n <= ((size_t)1 << 22) && !(n & (n - 1)); }
unsigned ceil_log2(size_t v) { unsigned l = 0; while (((size_t)1 << l) < v) ++l; return l; }
int grid_for(uint64_t items, int block = 256) {   // 8 workgroups per CU, grid-stride beyond: the rule of toyni_hip.hip
    uint64_t g = (items + block - 1) / block;
    const uint64_t cap = 256 * 8;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
size_t work_stride_words(const toyni_fib_proof_layout& l) { return (FIBV_W_POS + 2 * l.nrecords + 3) & ~(size_t)3; }

// enqueues one launch per VERIFY_MAX_GROUPS groups with records; the groups have been validated
int enqueue_groups(const toyni_merkle_verify_group* groups, size_t ngroups, size_t batch, hipStream_t s) {
    for (size_t k0 = 0; k0 < ngroups;) {
        MerkleVerifyGroups gs{};
        gs.batch = (uint32_t)batch;
        uint32_t cnt = 0;
        size_t k = k0;
        for (; k < ngroups && cnt < VERIFY_MAX_GROUPS; ++k) {
            const toyni_merkle_verify_group& q = groups[k];
            if (q.nrecords == 0) continue;
            gs.records[cnt] = q.d_records;
            gs.record_stride[cnt] = q.record_stride;
            gs.indices[cnt] = q.d_indices;
            gs.index_stride[cnt] = q.index_stride;
            gs.root[cnt] = q.d_root;
            gs.root_stride[cnt] = q.root_stride;
            gs.flags[cnt] = q.d_flags;
            gs.flag_stride[cnt] = q.flag_stride;
            gs.leaves[cnt] = q.leaves;
            gs.depth[cnt] = ceil_log2(q.leaves);
            gs.salted[cnt] = q.salted ? 1u : 0u;
            gs.first[cnt + 1] = gs.first[cnt] + q.nrecords;
            ++cnt;
        }
        k0 = k;
        if (!cnt) continue;
        gs.ngroups = cnt;
        for (uint32_t g = cnt + 1; g <= VERIFY_MAX_GROUPS; ++g) gs.first[g] = gs.first[cnt];
        hipLaunchKernelGGL(merkle_verify_records_batch_kernel, dim3(grid_for(gs.first[cnt] * batch)), dim3(256), 0, s, gs);
        const int st = (int)hipGetLastError();
        if (st) return st;
    }
    return TOYNI_OK;
}
}  // namespace

extern "C" {
int toyni_fib_proof_layout_of(size_t trace_len, toyni_fib_proof_layout* l) {
    if (!l) return TOYNI_E_NULL;
    if (!trace_len_ok(trace_len)) return TOYNI_E_INVALID_SIZE;
    std::memset(l, 0, sizeof(*l));
    const size_t n = trace_len, N = n << FIBV_LOG_BLOWUP, Q = FIBV_QUERIES;
    size_t C = 1;
    while (C < n + FIBV_MASK_DEGREE) C <<= 1;
    l->trace_len = n;
    l->lde_size = N;
    l->folds = ceil_log2(C);
    l->final_size = N / C;
    l->queries = Q;
    l->roots_offset = 0;
    l->nroots = l->folds + 3;
    l->ood_offset = 32 * l->nroots;
    l->indices_offset = l->ood_offset + 16;
    l->final_offset = l->indices_offset + 4 * Q;
    l->records_offset = (l->final_offset + 4 * l->final_size + 7) & ~(size_t)7;
    l->ngroups = l->folds + 2;
    size_t at = l->records_offset;
    for (size_t g = 0; g < l->ngroups; ++g) {
        l->group_leaves[g] = g < 3 ? N : N >> (g - 2);
        l->group_records[g] = g == 0 ? 3 * Q : g == 1 ? Q : 2 * Q;
        l->group_record_bytes[g] = toyni_merkle_open_record_bytes(l->group_leaves[g]);
        l->group_offset[g] = at;
        at += l->group_records[g] * l->group_record_bytes[g];
        l->nrecords += l->group_records[g];
    }
    l->image_bytes = (at + 15) & ~(size_t)15;
    return TOYNI_OK;
}

size_t toyni_fib_proof_image_bytes(size_t trace_len) {
    toyni_fib_proof_layout l;
    return toyni_fib_proof_layout_of(trace_len, &l) == TOYNI_OK ? l.image_bytes : 0;
}

const char* toyni_fib_verdict_string(uint32_t word) {
    if (word == 0) return "accept";
    const uint32_t code = word & 0xFFu, q1 = word >> 8;
    if (q1 == 0) {
        switch (code) {
            case FIBV_MALFORMED: return "malformed";
            case FIBV_OOD: return "ood";
            case FIBV_FINAL_NOT_CONSTANT: return "final_not_constant";
            case FIBV_FINAL_COMMITMENT: return "final_commitment";
            default: return "unknown";
        }
    }
    if (q1 > FIBV_QUERIES) return "unknown";
    switch (code) {
        case FIBV_QUERY_INDEX: return "query_index";
        case FIBV_TRACE_MERKLE: return "trace_merkle";
        case FIBV_QUOTIENT_MERKLE: return "quotient_merkle";
        case FIBV_DEEP_MERKLE: return "deep_merkle";
        case FIBV_DEEP_VALUE: return "deep_value";
        case FIBV_FINAL_VALUE: return "final_value";
        default: break;
    }
    if (code >= FIBV_FRI_FIRST && code < FIBV_FRI_FIRST + 2 * (FIBV_MAX_FOLDS - 1)) return (code & 1u) ? "fri_consistency" : "fri_merkle";
    return "unknown";
}

int toyni_merkle_verify_records_batch_device(const toyni_merkle_verify_group* groups, size_t ngroups, size_t batch, void* stream) {
    if (!groups && ngroups) return TOYNI_E_NULL;
    for (size_t k = 0; k < ngroups; ++k) {
        const toyni_merkle_verify_group& q = groups[k];
        if (q.nrecords && (!q.d_records || !q.d_indices || !q.d_root || !q.d_flags)) return TOYNI_E_NULL;
    }
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    for (size_t k = 0; k < ngroups; ++k) {
        const toyni_merkle_verify_group& q = groups[k];
        if (q.nrecords == 0) continue;
        if (q.leaves == 0 || (uint64_t)q.leaves > ((uint64_t)1 << 32) || (uint64_t)q.nrecords > ((uint64_t)1 << 26)) return TOYNI_E_RANGE;
        if (((uintptr_t)q.d_records & 7) || (q.record_stride & 7) || ((uintptr_t)q.d_indices & 3) || ((uintptr_t)q.d_root & 3) || (q.root_stride & 3) ||
            ((uintptr_t)q.d_flags & 3))
            return TOYNI_E_RANGE;
        if (q.record_stride < q.nrecords * toyni_merkle_open_record_bytes(q.leaves) || q.index_stride < q.nrecords || q.root_stride < 32 ||
            q.flag_stride < q.nrecords)
            return TOYNI_E_RANGE;
    }
    return enqueue_groups(groups, ngroups, batch, (hipStream_t)stream);
}

size_t toyni_fib_verify_work_bytes(size_t trace_len, size_t batch) {
    toyni_fib_proof_layout l;
    if (!batch_ok(batch) || toyni_fib_proof_layout_of(trace_len, &l) != TOYNI_OK) return 0;
    return batch * work_stride_words(l) * 4;
}

int toyni_fib_verify_batch_device(toyni_ntt_ctx* c, const uint8_t* d_images, size_t image_stride, size_t trace_len, size_t batch, void* d_work,
                                  uint32_t* d_verdicts, void* stream) {
    if (!c || !d_images || !d_work || !d_verdicts) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    struct Call {
        toyni_fib_proof_layout l;
        FibVerifyArgs a;
        const uint8_t* images;
        uint32_t *work, *verdicts;
        size_t batch;
        hipStream_t s;
    } call{};
    const int lst = toyni_fib_proof_layout_of(trace_len, &call.l);
    if (lst) return lst;
    const toyni_fib_proof_layout& l = call.l;
    if (toyni_internal::ctx_log_n(c) != (int)ceil_log2(l.lde_size)) return TOYNI_E_RANGE;
    if (((uintptr_t)d_images & 15) || ((uintptr_t)d_work & 15) || ((uintptr_t)d_verdicts & 3) || image_stride < l.image_bytes || (image_stride & 15)) return TOYNI_E_RANGE;
    FibVerifyArgs& a = call.a;
    a.log_n = ceil_log2(l.trace_len);
    a.log_N = a.log_n + FIBV_LOG_BLOWUP;
    a.folds = (uint32_t)l.folds;
    a.final_size = (uint32_t)l.final_size;
    a.ood_word = (uint32_t)(l.ood_offset / 4);
    a.index_word = (uint32_t)(l.indices_offset / 4);
    a.final_word = (uint32_t)(l.final_offset / 4);
    a.nrecords = (uint32_t)l.nrecords;
    a.image_stride = image_stride;
    a.work_stride = work_stride_words(l);
    const uint32_t g_inv = bb_inv_host(bb_root_of_unity_host(a.log_n));   // g^(n-1) = g^-1, g^(n-2) = g^-2
    a.b1R = to_mont_host(g_inv);
    a.b2R = to_mont_host(bb_mul_host(g_inv, g_inv));
    a.shift_invR = to_mont_host(bb_inv_host(FIBV_SHIFT));
    a.wNR = to_mont_host(bb_root_of_unity_host(a.log_N));
    a.ngroups = (uint32_t)l.ngroups;
    for (size_t g = 0; g < l.ngroups; ++g) {
        a.group_first[g + 1] = a.group_first[g] + (uint32_t)l.group_records[g];
        a.group_depth[g] = ceil_log2(l.group_leaves[g]);
        a.group_byte[g] = l.group_offset[g];
    }
    for (size_t g = l.ngroups + 1; g <= VERIFY_MAX_GROUPS; ++g) a.group_first[g] = a.group_first[l.ngroups];
    call.images = d_images;
    call.work = static_cast<uint32_t*>(d_work);
    call.verdicts = d_verdicts;
    call.batch = batch;
    call.s = (hipStream_t)stream;
    return toyni_internal::ctx_enqueue(c, stream, 0, [](void* user, uint32_t*) -> int {
        Call& k = *static_cast<Call*>(user);
        const FibVerifyArgs& a = k.a;
        const unsigned by = (unsigned)k.batch;
        hipLaunchKernelGGL(fib_verify_replay_kernel, dim3(by), dim3(VERIFY_WAVE), 0, k.s, a, k.images, k.work);
        hipLaunchKernelGGL(fib_verify_global_kernel, dim3(by), dim3(VERIFY_WAVE), 0, k.s, a, k.images, k.work);
        toyni_merkle_verify_group groups[VERIFY_MAX_GROUPS];
        uint32_t* pos = k.work + FIBV_W_POS;
        for (uint32_t g = 0; g < a.ngroups; ++g) {
            const uint32_t root = g == 0 ? 0u : g == 1 ? 1u : g;   // trace, quotient, fri_commitments[g - 2] = root g
            groups[g] = toyni_merkle_verify_group{k.images + a.group_byte[g], (size_t)a.image_stride, k.l.group_records[g], k.l.group_leaves[g], 1,
                                                  pos + a.group_first[g], (size_t)a.work_stride, k.images + 32u * root, (size_t)a.image_stride,
                                                  pos + a.nrecords + a.group_first[g], (size_t)a.work_stride};
        }
        const int st = enqueue_groups(groups, a.ngroups, k.batch, k.s);
        if (st) return st;
        hipLaunchKernelGGL(fib_verify_query_kernel, dim3(by), dim3(VERIFY_WAVE), 0, k.s, a, k.images, k.work);
        hipLaunchKernelGGL(fib_verify_verdict_kernel, dim3(by), dim3(VERIFY_WAVE), 0, k.s, static_cast<const uint32_t*>(k.work), (size_t)a.work_stride, k.verdicts);
        return (int)hipGetLastError();
    }, &call);
}
}  // extern "C"
#endif  // TOYNI_KERNEL_TEXT_ONLY
