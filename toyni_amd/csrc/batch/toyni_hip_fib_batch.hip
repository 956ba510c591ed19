// Section 3s of include/toyni_hip.h -- the batch dimension of the first half of a Fibonacci proof -- as a translation unit of its
// own, linked into libtoyni_hip.so next to toyni_hip.hip: thirteen kernels and their ten entry points.  It is separate so that the
// build of toyni_hip.hip stays, symbol for symbol and resource line for resource line, the build it was (tests/test_batch_resources.py
// holds that unit to its kernel list); the remarks of this unit are kept beside the library in a file of their own.
// The kernels share the __device__ bodies of the headers with their originals.  Two things they need are defined in toyni_hip.hip and
// not in a header, TRANSCRIPT_T and block_sum_mod: a product build of this unit restates them below, word for word; under TOYNI_KERNEL_TEXT_ONLY (tests/sim) this file is included BEHIND toyni_hip.hip and uses that file's.
// What the entry points need of a context comes through toyni_internal (defined in toyni_hip.hip, not part of the C ABI).
#ifndef TOYNI_KERNEL_TEXT_ONLY
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>

#include "toyni_hip.h"
#include "ntt_plan.hpp"
#include "merkle_kernels.hpp"
#include "prover_kernels.hpp"
#include "transcript_kernels.hpp"
#include "dz_kernels.hpp"
#include "fib_dz_kernels.hpp"

using namespace toyni;

namespace toyni_internal {
int ctx_log_n(const toyni_ntt_ctx* c);
DomainArgs ctx_domain_args(toyni_ntt_ctx* c, unsigned log_m, uint32_t shift);
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

constexpr uint32_t TRANSCRIPT_T = 64;   // one wave, as in toyni_hip.hip
// block-wide sum mod p through LDS (256 threads): the text of toyni_hip.hip's block_sum_mod
__device__ __forceinline__ uint32_t block_sum_mod(uint32_t v, uint32_t* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = bb_add(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    const uint32_t r = red[0];
    __syncthreads();
    return r;
}
#endif  // TOYNI_KERNEL_TEXT_ONLY

// ---- a batch dimension for the first half of a Fibonacci proof (include/toyni_hip.h 3s) ----
// Batch twins of the kernels of 3c / 3o / 3q that a Fibonacci proof launches before its tail, by the rules of the 3r twins above: the
// same launches, proof b a BLOCK coordinate (blockIdx.x where one block is one proof, blockIdx.y for the sweeps), every offset 64-bit,
// the bodies written out so that the originals' code cannot move.  Every barrier condition stays a function of the shared sizes.
// A proof's secret key is read from device memory (keys + 8 b words) by scalar loads: it is the same in every lane of a workgroup.
struct ChaChaBatchArgs {
    const uint32_t* keys;    // batch x 8 words
    uint32_t nonce[3];
    uint64_t blocks;         // per proof
    uint8_t* out;
    size_t out_stride;       // bytes, a multiple of 16
};
__global__ void __launch_bounds__(256) chacha20_fill_batch_kernel(const ChaChaBatchArgs a) {
    const size_t pb = blockIdx.y;   // the proof: a block coordinate, wave-uniform
    uint32_t key[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) key[k] = TOYNI_UNIFORM_LOAD(a.keys + 8 * pb + k);
    uint4* out = reinterpret_cast<uint4*>(a.out + pb * a.out_stride);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < a.blocks; b += stride) {
        uint32_t o[16];
        chacha20_block(key, (uint32_t)b, a.nonce, o);
#pragma unroll
        for (int q = 0; q < 4; ++q) out[4 * b + q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
}
// `in` carries proof 0's coefficients and no key
__global__ void __launch_bounds__(256) fib_mask_batch_kernel(const FibMaskArgs in, const size_t coeff_stride, const uint32_t* __restrict__ keys) {
    const size_t pb = blockIdx.y;   // the proof: a block coordinate, wave-uniform
    FibMaskArgs a = in;
    a.coeffs = in.coeffs + pb * coeff_stride;
#pragma unroll
    for (int k = 0; k < 8; ++k) a.key[k] = TOYNI_UNIFORM_LOAD(keys + 8 * pb + k);
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= fib_mask_items(a.n, a.mask_degree)) return;
    const uint64_t j = fib_mask_item_word(a.n, a.mask_degree, t);
    a.coeffs[j] = fib_mask_output(a, j, a.coeffs[j]);
}
struct QuotientBatch { size_t trace, c, q; };   // strides in words
__global__ void __launch_bounds__(256) fib_quotient_batch_kernel(const QuotientArgs in, const QuotientBatch st) {
    __shared__ uint32_t zh_inv[1024];
    const size_t pb = blockIdx.y;   // the proof: a block coordinate; the barrier below hangs on the shared log_blowup alone
    QuotientArgs a = in;
    a.trace = in.trace + pb * st.trace;
    a.c_out = in.c_out ? in.c_out + pb * st.c : nullptr;
    a.q_out = in.q_out + pb * st.q;
    const uint32_t B = 1u << a.log_blowup;
    for (uint32_t t = threadIdx.x; t < B; t += blockDim.x) zh_inv[t] = quotient_zh_inv(a, t);
    __syncthreads();
    const uint64_t N = (uint64_t)1 << a.log_N, mask = N - 1;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // the load width is chosen per proof, on its own pointers: a block-uniform choice, and both paths write the same words
    if (a.log_blowup >= 2 && a.log_N >= 2 && !(((uintptr_t)a.trace | (uintptr_t)a.c_out | (uintptr_t)a.q_out) & 15)) {
        const uint4* tr = reinterpret_cast<const uint4*>(a.trace);
        for (uint64_t qd = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; qd < N / 4; qd += stride) {
            const uint64_t i = 4 * qd;
            const uint4 v0 = tr[qd], v1 = tr[((i + B) & mask) >> 2], v2 = tr[((i + 2 * B) & mask) >> 2];
            const uint32_t t0[4] = {v0.x, v0.y, v0.z, v0.w}, t1[4] = {v1.x, v1.y, v1.z, v1.w}, t2[4] = {v2.x, v2.y, v2.z, v2.w};
            uint32_t c[4], qv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) quotient_one(a, i + j, t0[j], t1[j], t2[j], zh_inv[(i + j) & (B - 1)], c[j], qv[j]);
            if (a.c_out) reinterpret_cast<uint4*>(a.c_out)[qd] = make_uint4(c[0], c[1], c[2], c[3]);
            reinterpret_cast<uint4*>(a.q_out)[qd] = make_uint4(qv[0], qv[1], qv[2], qv[3]);
        }
    } else {
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
            uint32_t c, qv;
            quotient_one(a, i, a.trace[i], a.trace[(i + B) & mask], a.trace[(i + 2 * B) & mask], zh_inv[i & (B - 1)], c, qv);
            if (a.c_out) a.c_out[i] = c;
            a.q_out[i] = qv;
        }
    }
}
// one wave per transcript
__global__ void __launch_bounds__(TRANSCRIPT_T) transcript_squeeze_point_batch_kernel(TranscriptState* __restrict__ tr, uint32_t log_N, uint32_t shift_invR,
                                                                                       uint32_t* __restrict__ z, size_t z_stride) {
    const size_t pb = blockIdx.x;   // the proof: a block coordinate, wave-uniform
    if (threadIdx.x == 0) transcript_squeeze_point(tr[pb], log_N, shift_invR, FIB_POINT_TRIES, z + pb * z_stride);
}
__global__ void __launch_bounds__(TRANSCRIPT_T) transcript_absorb_fields_batch_kernel(TranscriptState* __restrict__ tr, const uint32_t* __restrict__ words,
                                                                                       size_t word_stride, uint32_t count) {
    const size_t pb = blockIdx.x;   // the proof: a block coordinate, wave-uniform
    transcript_absorb_fields_wave(tr[pb], words + pb * word_stride, count, threadIdx.x, TRANSCRIPT_T);
}
// one wave per proof, lane p: the three powers of point mults[p] * z_b, into record b
__global__ void __launch_bounds__(TRANSCRIPT_T) poly_dz_prepare_batch_kernel(const uint32_t* __restrict__ z, size_t z_stride, const PolyDzMults mults,
                                                                             uint32_t npoints, PolyDzRecord* __restrict__ rec) {
    const size_t pb = blockIdx.x;   // the proof: a block coordinate, wave-uniform
    if (threadIdx.x < npoints) poly_dz_record_point(z + pb * z_stride, mults.v[threadIdx.x], threadIdx.x, rec[pb]);
}
// `a` carries proof 0's coefficients and outputs; the partial sums of proof b are the nblocks x npoints words behind proof b - 1's
struct PolyDzBatch { size_t coeffs, out; };   // strides in words
__global__ void __launch_bounds__(256) poly_eval_partial_dz_batch_kernel(const PolyEvalDzArgs a, const PolyDzBatch st, const PolyDzRecord* __restrict__ rec0) {
    __shared__ uint32_t red[256];
    const size_t pb = blockIdx.y;   // the proof: a block coordinate; block_sum_mod's barriers hang on npoints alone
    const uint32_t* coeffs = a.coeffs + pb * st.coeffs;
    const PolyDzRecord* rec = rec0 + pb;
    uint32_t* partial = a.partial + pb * ((size_t)a.nblocks * a.npoints);
    const uint64_t base = (uint64_t)blockIdx.x * POLY_CHUNK + (uint64_t)threadIdx.x * POLY_PER_THREAD;
    uint32_t c[POLY_PER_THREAD];
#pragma unroll
    for (uint32_t j = 0; j < POLY_PER_THREAD; ++j) c[j] = base + j < a.ncoeffs ? coeffs[base + j] : 0u;
    for (uint32_t p = 0; p < a.npoints; ++p) {
        const uint32_t sum = block_sum_mod(poly_thread_term(poly_dz_point_args(rec, p), 0u, c, threadIdx.x), red);
        if (threadIdx.x == 0) partial[(uint64_t)blockIdx.x * a.npoints + p] = sum;
    }
}
__global__ void __launch_bounds__(256) poly_eval_final_dz_batch_kernel(const PolyEvalDzArgs a, const PolyDzBatch st, const PolyDzRecord* __restrict__ rec0) {
    __shared__ uint32_t red[256];
    const size_t pb = blockIdx.y;   // the proof: a block coordinate; block_sum_mod's barriers hang on npoints alone
    const PolyDzRecord* rec = rec0 + pb;
    const uint32_t* partial = a.partial + pb * ((size_t)a.nblocks * a.npoints);
    uint32_t* out = a.out + pb * st.out;
    for (uint32_t p = 0; p < a.npoints; ++p) {
        const uint32_t zchunkR = TOYNI_UNIFORM_LOAD(&rec->zchunkR[p]);
        uint32_t acc = 0;
        for (uint32_t b = threadIdx.x; b < a.nblocks; b += blockDim.x)
            acc = bb_add(acc, mont_mul(partial[(uint64_t)b * a.npoints + p], mont_pow(zchunkR, b)));
        const uint32_t sum = block_sum_mod(acc, red);
        if (threadIdx.x == 0) out[p] = sum;
    }
}
struct FibDeepBatch { size_t trace, quot, out, z, ood, check; };   // strides in words
// one wave per proof: record b, and proof b's check word
__global__ void __launch_bounds__(TRANSCRIPT_T) fib_deep_prepare_batch_kernel(const uint32_t* __restrict__ z, const uint32_t* __restrict__ ood, const FibCheckArgs k,
                                                                              const FibDeepBatch st, FibDeepRecord* __restrict__ rec, uint32_t* __restrict__ check) {
    const size_t pb = blockIdx.x;   // the proof: a block coordinate, wave-uniform
    if (threadIdx.x == 0) fib_deep_prepare(z + pb * st.z, ood + pb * st.ood, k, rec + pb, check ? check + pb * st.check : nullptr);
}
__global__ void __launch_bounds__(256) fib_deep_dz_batch_kernel(const DeepArgs in, const FibDeepBatch st, const FibDeepRecord* __restrict__ rec) {
    constexpr int K = 8;
    const size_t pb = blockIdx.y;   // the proof: a block coordinate, wave-uniform
    DeepArgs a = in;
    a.trace = in.trace + pb * st.trace;
    a.quot = in.quot + pb * st.quot;
    a.out = in.out + pb * st.out;
    fib_deep_args_from_record(a, rec[pb]);
    const uint64_t N = (uint64_t)1 << a.log_N, mask = N - 1, B = (uint64_t)1 << a.log_blowup;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    if (a.log_N >= 3) {
        for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < N / K; g += stride) {
            const uint64_t i0 = g * K;
            uint32_t t0[K], t1[K], t2[K], qv[K], out[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                t0[j] = a.trace[i0 + j];
                t1[j] = a.trace[(i0 + j + B) & mask];
                t2[j] = a.trace[(i0 + j + 2 * B) & mask];
                qv[j] = a.quot[i0 + j];
            }
            deep_group<K>(a, i0, t0, t1, t2, qv, out);
#pragma unroll
            for (int j = 0; j < K; ++j) a.out[i0 + j] = out[j];
        }
    } else {
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
            const uint32_t t0[1] = {a.trace[i]}, t1[1] = {a.trace[(i + B) & mask]}, t2[1] = {a.trace[(i + 2 * B) & mask]}, qv[1] = {a.quot[i]};
            uint32_t out[1];
            deep_group<1>(a, i, t0, t1, t2, qv, out);
            a.out[i] = out[0];
        }
    }
}
__global__ void __launch_bounds__(256) query_rows_batch_kernel(const uint32_t* __restrict__ indices, size_t index_stride, const QueryRowOffsets off,
                                                               uint32_t noffsets, uint64_t n, uint64_t total, uint32_t* __restrict__ out, size_t out_stride) {
    const size_t pb = blockIdx.y;   // the proof: a block coordinate, wave-uniform
    const uint32_t* idx = indices + pb * index_stride;
    uint32_t* o = out + pb * out_stride;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) o[t] = query_row(idx, off, noffsets, n, t);
}
// one block per proof; both strides in words
__global__ void __launch_bounds__(256) fri_phase_roots_batch_kernel(const uint32_t* __restrict__ levels, size_t level_stride, uint64_t m_first, uint32_t rounds,
                                                                    uint32_t* __restrict__ roots, size_t root_stride) {
    const size_t pb = blockIdx.x;   // the proof: a block coordinate, wave-uniform
    const uint32_t* lv = levels + pb * level_stride;
    uint32_t* r = roots + pb * root_stride;
    for (uint32_t t = threadIdx.x; t < 8u * rounds; t += blockDim.x) r[t] = fri_phase_root_word(lv, m_first, t);
}
// `rows` copies of row_bytes bytes (a multiple of 4) in one launch: row blockIdx.y; 16-byte accesses for the first `quads` quads of a
// row (the host passes 0 unless both pointers and both strides are multiples of 16), words for the rest
__global__ void __launch_bounds__(256) copy_rows_kernel(uint8_t* dst0, size_t dst_stride, const uint8_t* src0, size_t src_stride, uint64_t row_bytes,
                                                        uint64_t quads) {
    const size_t row = blockIdx.y;
    uint8_t* dst = dst0 + row * dst_stride;
    const uint8_t* src = src0 + row * src_stride;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t q = first; q < quads; q += stride) reinterpret_cast<uint4*>(dst)[q] = reinterpret_cast<const uint4*>(src)[q];
    for (uint64_t w = 4 * quads + first; w < row_bytes / 4; w += stride) reinterpret_cast<uint32_t*>(dst)[w] = reinterpret_cast<const uint32_t*>(src)[w];
}

#ifndef TOYNI_KERNEL_TEXT_ONLY
// ---- the entry points ----
// Order of the refusals as in 3r: null pointers, batch, the single call's own in the single call's order, the strides (and d_keys).
namespace {
constexpr size_t BATCH_MAX = 65535;   // the proof index is a block coordinate: gridDim.y
bool batch_ok(size_t batch) { return batch >= 1 && batch <= BATCH_MAX; }
bool is_pow2(size_t v) { return v && !(v & (v - 1)); }
int ilog2(size_t v) { int l = 0; while (((size_t)1 << l) < v) ++l; return l; }
TranscriptState* transcript_of(toyni_transcript* d_tr) { return reinterpret_cast<TranscriptState*>(d_tr); }
int grid_for(size_t items, int block = 256) {   // 8 workgroups per CU, grid-stride beyond: the rule of toyni_hip.hip
    size_t g = (items + block - 1) / block;
    const size_t cap = 256 * 8;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
}  // namespace

extern "C" {
int toyni_chacha20_fill_batch_device(void* d_out, size_t out_stride, size_t bytes, const uint8_t* d_keys, uint64_t nonce, size_t batch, void* stream) {
    if (!d_out || !d_keys) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (((uintptr_t)d_out & 15) || (bytes & 63)) return TOYNI_E_RANGE;
    if (bytes / 64 > 0xFFFFFFFFull) return TOYNI_E_RANGE;
    if (out_stride < bytes || (out_stride & 15) || ((uintptr_t)d_keys & 3)) return TOYNI_E_RANGE;
    if (bytes == 0) return TOYNI_OK;
    ChaChaBatchArgs a{};
    a.keys = reinterpret_cast<const uint32_t*>(d_keys);
    a.nonce[0] = 0u;
    a.nonce[1] = (uint32_t)nonce;
    a.nonce[2] = (uint32_t)(nonce >> 32);
    a.blocks = bytes / 64;
    a.out = static_cast<uint8_t*>(d_out);
    a.out_stride = out_stride;
    hipLaunchKernelGGL(chacha20_fill_batch_kernel, dim3(grid_for(a.blocks), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int toyni_mask_poly_batch_device(uint32_t* d_coeffs, size_t coeff_stride, size_t n, unsigned mask_degree, const uint8_t* d_keys, uint64_t nonce, size_t batch,
                                 void* stream) {
    if (!d_coeffs || !d_keys) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (mask_degree == 0 || mask_degree > FIB_MASK_MAX_DEGREE || n == 0 || ((uintptr_t)d_coeffs & 3)) return TOYNI_E_RANGE;
    if (coeff_stride < mask_degree || coeff_stride - mask_degree < n || ((uintptr_t)d_keys & 3)) return TOYNI_E_RANGE;
    FibMaskArgs a{};
    a.coeffs = d_coeffs;
    a.n = n;
    a.mask_degree = mask_degree;
    a.nonce[0] = 0u;
    a.nonce[1] = (uint32_t)nonce;
    a.nonce[2] = (uint32_t)(nonce >> 32);
    const uint64_t items = fib_mask_items(n, mask_degree);   // <= 2 x 4096: the grid is never capped
    hipLaunchKernelGGL(fib_mask_batch_kernel, dim3((unsigned)((items + 255) / 256), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, a, coeff_stride,
                       reinterpret_cast<const uint32_t*>(d_keys));
    return (int)hipGetLastError();
}

int toyni_transcript_squeeze_point_batch_device(toyni_transcript* d_tr, size_t batch, unsigned log_N, uint32_t shift, uint32_t* d_z, size_t z_stride,
                                                void* stream) {
    if (!d_tr || !d_z) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (((uintptr_t)d_tr & 15) || ((uintptr_t)d_z & 3) || log_N > FIB_POINT_MAX_LOG_N || shift == 0 || shift >= BB_P) return TOYNI_E_RANGE;
    if (z_stride < 1) return TOYNI_E_RANGE;
    hipLaunchKernelGGL(transcript_squeeze_point_batch_kernel, dim3((unsigned)batch), dim3(TRANSCRIPT_T), 0, (hipStream_t)stream, transcript_of(d_tr),
                       (uint32_t)log_N, to_mont_host(bb_inv_host(shift)), d_z, z_stride);
    return (int)hipGetLastError();
}

int toyni_transcript_absorb_fields_batch_device(toyni_transcript* d_tr, size_t batch, const uint32_t* d_words, size_t word_stride, size_t count,
                                                void* stream) {
    if (!d_tr || (!d_words && count)) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (((uintptr_t)d_tr & 15) || ((uintptr_t)d_words & 3) || count > TRANSCRIPT_MAX_FIELDS) return TOYNI_E_RANGE;
    if (word_stride < count) return TOYNI_E_RANGE;
    if (count == 0) return TOYNI_OK;
    hipLaunchKernelGGL(transcript_absorb_fields_batch_kernel, dim3((unsigned)batch), dim3(TRANSCRIPT_T), 0, (hipStream_t)stream, transcript_of(d_tr), d_words,
                       word_stride, (uint32_t)count);
    return (int)hipGetLastError();
}

int toyni_query_rows_batch_device(const uint32_t* d_indices, size_t index_stride, size_t count, size_t n, const uint32_t* offsets, unsigned noffsets,
                                  size_t batch, uint32_t* d_out, size_t out_stride, void* stream) {
    if (!d_indices || !d_out || !offsets) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (((uintptr_t)d_indices & 3) || ((uintptr_t)d_out & 3) || noffsets < 1 || noffsets > QUERY_ROWS_MAX_OFFSETS || n < 1 ||
        (uint64_t)n > ((uint64_t)1 << 32) || count > 65536)
        return TOYNI_E_RANGE;
    QueryRowOffsets off{};
    for (unsigned r = 0; r < noffsets; ++r) {
        if (offsets[r] >= n) return TOYNI_E_RANGE;
        off.v[r] = offsets[r];
    }
    const uint64_t total = (uint64_t)count * noffsets;
    if (index_stride < count || out_stride < total) return TOYNI_E_RANGE;
    if (count == 0) return TOYNI_OK;
    hipLaunchKernelGGL(query_rows_batch_kernel, dim3(grid_for(total), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, d_indices, index_stride, off,
                       (uint32_t)noffsets, (uint64_t)n, total, d_out, out_stride);
    return (int)hipGetLastError();
}

int toyni_fri_phase_roots_batch_device(const uint8_t* d_levels, size_t level_stride, size_t m_first, unsigned rounds, size_t batch, uint8_t* d_roots,
                                       size_t root_stride, void* stream) {
    if (!d_levels || !d_roots) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (!is_pow2(m_first) || (uint64_t)m_first > ((uint64_t)1 << 32)) return TOYNI_E_INVALID_SIZE;
    if (rounds > FRI_PHASE_MAX_ROUNDS || (rounds && (m_first >> (rounds - 1)) == 0) || ((uintptr_t)d_levels & 15) || ((uintptr_t)d_roots & 3)) return TOYNI_E_RANGE;
    uint64_t digests = 0;
    for (unsigned k = 0; k < rounds; ++k) digests += 2u * ((uint64_t)m_first >> k) - 1u;
    if (level_stride < digests * 32 || (level_stride & 15) || root_stride < 32u * (size_t)rounds || (root_stride & 3)) return TOYNI_E_RANGE;
    if (rounds == 0) return TOYNI_OK;
    hipLaunchKernelGGL(fri_phase_roots_batch_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t*>(d_levels),
                       level_stride / 4, (uint64_t)m_first, (uint32_t)rounds, reinterpret_cast<uint32_t*>(d_roots), root_stride / 4);
    return (int)hipGetLastError();
}

int toyni_copy_rows_device(void* d_dst, size_t dst_stride, const void* d_src, size_t src_stride, size_t row_bytes, size_t rows, void* stream) {
    if (!d_dst || !d_src) return TOYNI_E_NULL;
    if (rows > BATCH_MAX) return TOYNI_E_RANGE;                       // the row is a block coordinate
    if ((((uintptr_t)d_dst | (uintptr_t)d_src) & 3) || ((dst_stride | src_stride | row_bytes) & 3)) return TOYNI_E_RANGE;
    if (dst_stride < row_bytes || src_stride < row_bytes) return TOYNI_E_RANGE;
    if (rows == 0 || row_bytes == 0) return TOYNI_OK;
    const bool wide = !((((uintptr_t)d_dst | (uintptr_t)d_src) & 15) || ((dst_stride | src_stride) & 15));
    const uint64_t quads = wide ? row_bytes / 16 : 0;
    const uint64_t items = std::max<uint64_t>(quads, row_bytes / 4 - 4 * quads);
    hipLaunchKernelGGL(copy_rows_kernel, dim3(grid_for(items), (unsigned)rows), dim3(256), 0, (hipStream_t)stream, static_cast<uint8_t*>(d_dst), dst_stride,
                       static_cast<const uint8_t*>(d_src), src_stride, (uint64_t)row_bytes, quads);
    return (int)hipGetLastError();
}

int toyni_fib_quotient_batch_device(toyni_ntt_ctx* c, const uint32_t* d_trace_lde, size_t trace_stride, uint32_t* d_c_evals, size_t c_stride,
                                    uint32_t* d_q_evals, size_t q_stride, unsigned log_blowup, uint32_t shift, size_t batch, void* stream) {
    if (!c || !d_trace_lde || !d_q_evals) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    const int log_N = toyni_internal::ctx_log_n(c);
    if ((int)log_blowup > log_N || log_blowup > 10 || shift == 0 || shift >= BB_P) return TOYNI_E_RANGE;
    const int log_n = log_N - (int)log_blowup;
    if (log_n < 1) return TOYNI_E_RANGE;
    struct Call {
        toyni_ntt_ctx* c;
        QuotientArgs a;
        QuotientBatch st;
        int log_N, log_n;
        unsigned log_blowup;
        uint32_t shift;
        size_t batch;
        hipStream_t s;
    } call{c, QuotientArgs{}, QuotientBatch{trace_stride, c_stride, q_stride}, log_N, log_n, log_blowup, shift, batch, (hipStream_t)stream};
    call.a.trace = d_trace_lde;
    call.a.c_out = d_c_evals;
    call.a.q_out = d_q_evals;
    return toyni_internal::ctx_enqueue(c, stream, 0, [](void* user, uint32_t*) -> int {
        Call& k = *static_cast<Call*>(user);
        QuotientArgs& a = k.a;
        a.dom = toyni_internal::ctx_domain_args(k.c, (unsigned)k.log_N, k.shift);
        a.log_N = (uint32_t)k.log_N;
        a.log_blowup = k.log_blowup;
        const uint64_t n = 1ull << k.log_n, N = 1ull << k.log_N;
        const uint32_t g = bb_root_of_unity_host((uint32_t)k.log_n);
        a.b1R = to_mont_host(bb_pow_host(g, n - 1));
        a.b2R = to_mont_host(bb_pow_host(g, n - 2));
        a.shift_nR = to_mont_host(bb_pow_host(k.shift, n));
        a.wBR = to_mont_host(bb_pow_host(bb_root_of_unity_host((uint32_t)k.log_N), n));
        if (bb_pow_host(bb_pow_host(k.shift, n), 1ull << k.log_blowup) == 1u) return TOYNI_E_ZERO_INVERSE;
        if (k.st.trace < N || k.st.q < N || (a.c_out && k.st.c < N)) return TOYNI_E_RANGE;
        // every proof takes the 16-byte path only if proof 0 does and the strides keep the alignment; otherwise the grid covers single words
        const bool quads = k.log_blowup >= 2 && k.log_N >= 2 && !(((uintptr_t)a.trace | (uintptr_t)a.c_out | (uintptr_t)a.q_out) & 15) &&
                           !((k.st.trace | k.st.q | (a.c_out ? k.st.c : 0)) & 3);
        const uint64_t items = quads ? N / 4 : N;
        hipLaunchKernelGGL(fib_quotient_batch_kernel, dim3(grid_for(items), (unsigned)k.batch), dim3(256), 0, k.s, a, k.st);
        return (int)hipGetLastError();
    }, &call);
}

int toyni_poly_eval_dz_batch_device(toyni_ntt_ctx* c, const uint32_t* d_coeffs, size_t coeff_stride, size_t ncoeffs, const uint32_t* d_z, size_t z_stride,
                                    const uint32_t* mults, unsigned npoints, size_t batch, uint32_t* d_out, size_t out_stride, void* stream) {
    if (!c || !d_z || !mults || !d_out || (!d_coeffs && ncoeffs)) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (npoints < 1 || npoints > (unsigned)POLY_MAX_POINTS) return TOYNI_E_RANGE;
    struct Call {
        PolyEvalDzArgs a;
        PolyDzBatch st;
        PolyDzMults m;
        const uint32_t* d_z;
        size_t z_stride, batch, partial_words;
        hipStream_t s;
    } call{};
    for (unsigned p = 0; p < npoints; ++p) {
        if (mults[p] >= BB_P) return TOYNI_E_RANGE;
        call.m.v[p] = mults[p];
    }
    if (((uintptr_t)d_coeffs | (uintptr_t)d_out | (uintptr_t)d_z) & 3) return TOYNI_E_RANGE;
    if (coeff_stride < ncoeffs || z_stride < 1 || out_stride < npoints) return TOYNI_E_RANGE;
    const size_t nblocks = (ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK;
    if (nblocks > 0xFFFFFFFFull) return TOYNI_E_RANGE;
    call.a.coeffs = d_coeffs;
    call.a.ncoeffs = ncoeffs;
    call.a.npoints = npoints;
    call.a.nblocks = (uint32_t)nblocks;
    call.a.out = d_out;
    call.st = PolyDzBatch{coeff_stride, out_stride};
    call.d_z = d_z;
    call.z_stride = z_stride;
    call.batch = batch;
    call.s = (hipStream_t)stream;
    // the stream's buffer: batch x nblocks x npoints partial sums, rounded up to a multiple of four words, then `batch` records
    call.partial_words = (batch * nblocks * npoints + 3) & ~(size_t)3;
    return toyni_internal::ctx_enqueue(c, stream, call.partial_words + batch * (sizeof(PolyDzRecord) / sizeof(uint32_t)), [](void* user, uint32_t* d_words) -> int {
        Call& k = *static_cast<Call*>(user);
        k.a.partial = d_words;
        PolyDzRecord* rec = reinterpret_cast<PolyDzRecord*>(d_words + k.partial_words);
        const unsigned by = (unsigned)k.batch;
        hipLaunchKernelGGL(poly_dz_prepare_batch_kernel, dim3(by), dim3(TRANSCRIPT_T), 0, k.s, k.d_z, k.z_stride, k.m, k.a.npoints, rec);
        // ncoeffs == 0: the zero polynomial -- stage 2 alone sums no partial and writes the zeros
        if (k.a.nblocks)
            hipLaunchKernelGGL(poly_eval_partial_dz_batch_kernel, dim3(k.a.nblocks, by), dim3(POLY_THREADS), 0, k.s, k.a, k.st, static_cast<const PolyDzRecord*>(rec));
        hipLaunchKernelGGL(poly_eval_final_dz_batch_kernel, dim3(1, by), dim3(256), 0, k.s, k.a, k.st, static_cast<const PolyDzRecord*>(rec));
        return (int)hipGetLastError();
    }, &call);
}

int toyni_fib_deep_dz_batch_device(toyni_ntt_ctx* c, const uint32_t* d_trace_lde, size_t trace_stride, const uint32_t* d_q_evals, size_t q_stride,
                                   uint32_t* d_out, size_t out_stride, unsigned log_blowup, uint32_t shift, const uint32_t* d_z, size_t z_stride,
                                   const uint32_t* d_ood, size_t ood_stride, uint32_t trace_len, uint32_t* d_check, size_t check_stride, size_t batch,
                                   void* stream) {
    if (!c || !d_trace_lde || !d_q_evals || !d_out || !d_z || !d_ood) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (shift == 0 || shift >= BB_P || !is_pow2(trace_len) || trace_len > (1u << 27) || (((uintptr_t)d_z | (uintptr_t)d_ood | (uintptr_t)d_check) & 3))
        return TOYNI_E_RANGE;
    const int log_N = toyni_internal::ctx_log_n(c);
    if ((int)log_blowup > log_N) return TOYNI_E_RANGE;
    const uint64_t N = 1ull << log_N;
    if (trace_stride < N || q_stride < N || out_stride < N || z_stride < 1 || ood_stride < 4 || (d_check && check_stride < 1)) return TOYNI_E_RANGE;
    struct Call {
        toyni_ntt_ctx* c;
        DeepArgs a;
        FibDeepBatch st;
        FibCheckArgs k;
        const uint32_t *d_z, *d_ood;
        uint32_t* d_check;
        uint32_t shift;
        size_t batch;
        hipStream_t s;
    } call{c, DeepArgs{}, FibDeepBatch{trace_stride, q_stride, out_stride, z_stride, ood_stride, check_stride}, FibCheckArgs{}, d_z, d_ood, d_check, shift, batch,
           (hipStream_t)stream};
    call.a.trace = d_trace_lde;
    call.a.quot = d_q_evals;
    call.a.out = d_out;
    call.a.log_N = (uint32_t)log_N;
    call.a.log_blowup = log_blowup;
    call.a.wNR = to_mont_host(bb_root_of_unity_host((uint32_t)log_N));
    call.k.log_n = (uint32_t)ilog2(trace_len);
    const uint32_t g_inv = bb_inv_host(bb_root_of_unity_host(call.k.log_n));   // g^(n-1) = g^-1, g^(n-2) = g^-2
    call.k.b1R = to_mont_host(g_inv);
    call.k.b2R = to_mont_host(bb_mul_host(g_inv, g_inv));
    return toyni_internal::ctx_enqueue(c, stream, batch * (sizeof(FibDeepRecord) / sizeof(uint32_t)), [](void* user, uint32_t* d_words) -> int {   // `batch` records
        Call& k = *static_cast<Call*>(user);
        k.a.dom = toyni_internal::ctx_domain_args(k.c, k.a.log_N, k.shift);
        FibDeepRecord* rec = reinterpret_cast<FibDeepRecord*>(d_words);
        hipLaunchKernelGGL(fib_deep_prepare_batch_kernel, dim3((unsigned)k.batch), dim3(TRANSCRIPT_T), 0, k.s, k.d_z, k.d_ood, k.k, k.st, rec, k.d_check);
        const uint64_t N = 1ull << k.a.log_N;
        const uint64_t items = k.a.log_N >= 3 ? N / 8 : N;
        hipLaunchKernelGGL(fib_deep_dz_batch_kernel, dim3(grid_for(items), (unsigned)k.batch), dim3(256), 0, k.s, k.a, k.st, static_cast<const FibDeepRecord*>(rec));
        return (int)hipGetLastError();
    }, &call);
}
}  // extern "C"
#endif  // TOYNI_KERNEL_TEXT_ONLY
