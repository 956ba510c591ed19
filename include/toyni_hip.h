/*
 * toyni_hip.h -- C ABI of libtoyni_hip.so: the MI355X (gfx950) backend for Toyni's BabyBear NTT and
 * FRI fold.  This is the drop-in boundary: it is what `src/ntt.rs::cuda` (reference
 * /root/reference/src/ntt.rs:95-110) binds, re-implemented from scratch in HIP.  Plain pointers and
 * sizes only.  Every new entry point returns an int status (0 = success, otherwise a hipError_t value
 * or one of the TOYNI_E_* codes below; toyni_error_string() names both).
 *
 * Element formats
 *   host / "u64" : one uint64_t per element, canonical residue mod p = 2013265921
 *                  (= #[repr(C)] struct BabyBear { value: u64 }, src/babybear.rs:10-14)
 *   device "u32" : packed uint32_t canonical residues (the native device format; 8 B/element of HBM
 *                  traffic per pass instead of 16).
 *
 * Pointer alignment of the device entry points.  Every rule above 4 bytes is checked: a pointer that breaks it is refused with
 * TOYNI_E_RANGE before anything is enqueued (the narrow / widen pair also refuses a u32 pointer below 4 bytes):
 *   4 bytes  every packed-u32 pointer not listed below: the transforms (plain, coset, Ext, LDE, Ext LDE), domain points, the
 *            four-step twiddle, the slab pass, the structured and explicit-point folds and the fold loop (16-byte aligned layers of
 *            whole quads take 16-byte accesses, others word accesses), the fold round's d_evals / d_out, the commit phase's
 *            d_layer0 / d_layers, quotient, DEEP, polynomial evaluation and its d_out, the openings' d_values / d_indices; the row commitment's and
 *            row openings' d_values / d_indices (checked: TOYNI_E_RANGE below 4 bytes; a 16-byte aligned row-major matrix whose width
 *            is a multiple of 4 takes 16-byte loads, others word loads)
 *   8 bytes  u64 pointers (toyni_ntt_device_u64, the narrow / widen pair) and the openings' d_out (row openings included)
 *   16 bytes the Ext folds' d_evals / d_out (one 16-byte access per Ext element; d_xs needs 4), the Ext DEEP combination's d_out (3h),
 *            the Ext fold round's d_evals / d_out and the Ext commit phase's d_layer0 / d_layers (toyni_fri_fold_commit_ext_device,
 *            toyni_fri_commit_phase_ext_device, 3j), the slab relayout's and the fused
 *            slab rows' d_in / d_out, every Merkle d_levels / d_salts, the ChaCha20 fill's d_out
 *
 * Threading and streams: a context serialises the ENQUEUEING of its calls with an internal mutex, and keeps its
 * intermediate buffers per stream: calls enqueued on one stream are ordered by that stream, calls enqueued on different
 * streams use different buffers.  So one context may be driven from several host threads and several streams at once
 * (the reference's single shared d_data -- SURVEY.md F8, cuda/ntt_kernel.cu:205 -- has no counterpart).  At most 8 streams'
 * buffer sets are kept per context (least recently used first out).  Memory stays bounded without any call from the user
 * (round 3): a buffer that was outgrown, or that belonged to an evicted set, carries a HIP event recorded on its stream after its
 * last use, and the next call on the context that finds the event complete frees it (hipFree synchronises the device, so this
 * never happens on the enqueue path of a steady-state caller -- there is nothing to free there).  A context that serves ONE stream
 * with small calls (intermediates under 64 MiB: the latency path) records no events at all; with several streams, or large
 * intermediates, every call ends with one hipEventRecord (TOYNI_FENCE=always|never overrides).
 * Synchronising a stream through this API (blocking entry points, toyni_stream_synchronize), toyni_ntt_ctx_trim and
 * toyni_ntt_ctx_destroy release retired buffers as before.  Calls captured into a HIP graph leave no fence.
 */
#ifndef TOYNI_HIP_H
#define TOYNI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TOYNI_OK 0
#define TOYNI_E_INVALID_SIZE 10001   /* n not a power of two, or > 2^27 (src/ntt.rs:229-230) */
#define TOYNI_E_NULL 10002           /* null context / pointer */
#define TOYNI_E_ODD_LENGTH 10003     /* fri_fold: "Evaluations length must be even" (src/math/fri.rs:28) */
#define TOYNI_E_NO_DEVICE 10004      /* no usable GPU ("CUDA not available", src/ntt.rs:225-227) */
#define TOYNI_E_ZERO_INVERSE 10005   /* fri_fold: a point x_i = 0 ("Cannot invert zero", src/babybear.rs:112) */
#define TOYNI_E_RANGE 10006          /* argument out of range (layer larger than the context's domain, ...) */
#define TOYNI_E_NO_RCCL 10007        /* the RCCL exchange was requested and librccl could not be loaded */
#define TOYNI_E_RCCL 10008           /* an RCCL call failed */
#define TOYNI_E_NO_PEER_ACCESS 10009 /* two devices of a multi-device group cannot access each other directly (hipDeviceCanAccessPeer);
                                      * TOYNI_ALLOW_STAGED_PEER=1 accepts host-staged copies instead */
#define TOYNI_E_REENTRANT 10011      /* an entry point was called on a context from inside that context's transcript callback */
#define TOYNI_E_SELF_CHECK 10010     /* the first-use check of a multi-device group disagreed with the single-device transform */

typedef struct toyni_ntt_ctx toyni_ntt_ctx;

/* ------------------------------------------------------------------------------------------------
 * 1. The reference's ABI, symbol for symbol (cuda/ntt_kernel.cu:211-318; extern block src/ntt.rs:95-110).
 *    The reference's own extern block binds all ten of its symbols with ONE edit: the link name
 *    (`ntt_cuda` -> `toyni_hip`).
 *    `count` is in u64 ELEMENTS.
 * ---------------------------------------------------------------------------------------------- */
void* ntt_ctx_create(uint32_t n);                       /* cuda/ntt_kernel.cu:213-234; NULL on error */
void ntt_ctx_destroy(void* ctx);                        /* :236-242; null-safe */
void ntt_run_inplace(void* ctx, uint64_t* h_data);      /* :249-268; host pointer, ctx->n elements, blocking */
void intt_run_inplace(void* ctx, uint64_t* h_data);     /* :272-292 */
int cuda_malloc(uint64_t** d_ptr, size_t count);        /* :298-300 */
int cuda_free(uint64_t* d_ptr);                         /* :302-304 */
int cuda_copy_to_device(uint64_t* d_dest, const uint64_t* h_src, size_t count);    /* :306-308 */
int cuda_copy_from_device(uint64_t* h_dest, const uint64_t* d_src, size_t count);  /* :310-312 */
const char* cuda_get_error_string(int error);           /* :314-316 */

/* The tenth symbol of the reference's extern block, `cudaGetDeviceCount` (src/ntt.rs:102,147), comes from libcudart there.  It is
 * exported here under the same name and signature (count of HIP devices, 0 = success), so the reference's extern block links against
 * this library with ONE edit, the link name (`ntt_cuda` -> `toyni_hip`); toyni_device_count is the same call under a neutral name,
 * which rust/src/ntt_gpu.rs binds. */
int cudaGetDeviceCount(int* count);
int toyni_device_count(int* count);
const char* toyni_error_string(int status);

/* ------------------------------------------------------------------------------------------------
 * 2. Status-returning context API (superset of section 1)
 * ---------------------------------------------------------------------------------------------- */
/* n: power of two, 1 <= n <= 2^27.  device: HIP device ordinal, or -1 for the current device.
 * Builds both directions' twiddle tables (cuda/ntt_kernel.cu:160-185,213-234) and owns a stream. */
int toyni_ntt_ctx_create(uint32_t n, int device, toyni_ntt_ctx** out);
int toyni_ntt_ctx_destroy(toyni_ntt_ctx* ctx);
uint32_t toyni_ntt_ctx_n(const toyni_ntt_ctx* ctx);
int toyni_ntt_ctx_device(const toyni_ntt_ctx* ctx);
int toyni_ntt_ctx_passes(const toyni_ntt_ctx* ctx);     /* HBM sweeps per transform of the context's plan (1..3); large batches
                                                          * of n = 2^11..2^13 run a single-sweep kernel instead of their 2 passes */
/* HBM sweeps (= kernel launches) one toyni_ntt_device call on `batch` base-field transforms makes: the single-sweep kernel for large
 * batches of n = 2^11..2^13, the two-pass plan of n = 2^21 (every batch) and of a lone n = 2^22 transform, else as above. */
int toyni_ntt_ctx_passes_for(const toyni_ntt_ctx* ctx, size_t batch);
/* Multi-pass transforms of a large batch are issued in chunks of about chunk_elems elements so that the
 * intermediate buffer stays cache-resident; 0 = whole batch at once (also env TOYNI_CHUNK_ELEMS). */
int toyni_ntt_ctx_set_chunk(toyni_ntt_ctx* ctx, size_t chunk_elems);

/* Host-slice entry points -- what ntt_cuda / intt_cuda (src/ntt.rs:224-251) call.  h_data: batch * n
 * u64 elements, overwritten in place, natural order in and out, canonical root w_n.  Blocking.
 * H2D -> narrow -> fused passes -> widen -> D2H. */
int toyni_ntt_host(toyni_ntt_ctx* ctx, uint64_t* h_data, size_t batch, int inverse);

/* The same over several GPUs from ONE host process: the batch is sharded contiguously over `devices` (ordinals; a
 * device may be listed more than once), one host thread per entry, no collective.  Contexts are cached per
 * (device, lane, n) for the life of the process, like get_or_create_ctx (src/ntt.rs:128-141).  Blocking. */
int toyni_ntt_host_multi_gpu(const int* devices, int ndev, uint32_t n, uint64_t* h_data, size_t batch, int inverse);

/* Device-resident, packed u32, in place (d_in == d_out) or out of place.  Enqueued on `stream`
 * (a hipStream_t; NULL = HIP's default stream, as everywhere in HIP) and NOT synchronised: this is the
 * entry point the roofline numbers are measured on.  batch transforms are contiguous (stride n); the pointers need
 * 4-byte alignment only; elements are canonical residues (< p), outputs are canonical.
 * Any number of streams per context (intermediates are per stream, see "Threading and streams" above). */
int toyni_ntt_device(toyni_ntt_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, size_t batch, int inverse, void* stream);

/* Device-resident on the reference's u64 element layout (what a CudaBuffer holds, src/ntt.rs:153-215). */
int toyni_ntt_device_u64(toyni_ntt_ctx* ctx, uint64_t* d_data, size_t batch, int inverse, void* stream);

/* Coset transforms of BabyBearDomain (src/math/domain.rs:85-123,154-174) with the host's serial
 * shift^i loop fused on the device: forward = scale by shift^i then NTT; inverse = INTT then scale by
 * shift^-i.  shift is a canonical nonzero residue; shift == 1 is the plain transform. */
int toyni_coset_ntt_device(toyni_ntt_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, size_t batch, uint32_t shift, int inverse, void* stream);
int toyni_coset_ntt_host(toyni_ntt_ctx* ctx, uint64_t* h_data, size_t batch, uint64_t shift, int inverse);

/* Low-degree extension: the forward coset transform of `batch` coefficient vectors of n >> log_blowup words each
 * (contiguous, stride n >> log_blowup), zero-padded to n -- what the prover does with every column (src/fibonacci.rs:101-103;
 * BabyBearDomain::fft pads, src/math/domain.rs:107-123).  The padding is implied, not stored: the first pass reads only the
 * words that exist and skips the butterflies whose partner is a padding zero.  Out of place; d_out holds batch * n words.
 * Identical results to zero-padding by hand and calling toyni_coset_ntt_device. */
int toyni_lde_device(toyni_ntt_ctx* ctx, const uint32_t* d_coeffs, uint32_t* d_out, size_t batch, unsigned log_blowup, uint32_t shift, void* stream);
/* Host-slice form = BabyBearDomain::fft(coeffs) in one call (src/math/domain.rs:107-123): ncoeffs <= n coefficients in
 * (any count; u64 elements, reduced mod p like BabyBear::new), n evaluations on shift * <w_n> out.  Only the
 * coefficients are uploaded (the reference pads on the host and uploads n elements).  Blocking. */
int toyni_lde_host(toyni_ntt_ctx* ctx, const uint64_t* h_coeffs, size_t ncoeffs, uint64_t* h_out, uint64_t shift);

/* Extension-field transforms, fft_ext / ifft_ext (src/math/domain.rs:129-151): n Ext elements = 4 words each (AoS,
 * #[repr(C)] Ext { c: [BabyBear; 4] }).  The transform is base-linear, i.e. the base transform of every coordinate (the reference
 * de-interleaves into four vectors, transforms each and re-interleaves, :140-151).  Here the AoS vector is transformed AS IT IS: the
 * pass kernels have an interleaved form in which the four coordinates of an element are four neighbouring columns (first / middle
 * passes) or four interleaved rows (last pass), so an Ext transform costs exactly the passes of the plan -- no de-interleave sweep
 * on either side -- and `batch` vectors go through one launch sequence.  shift = coset shift (1 = standard domain).
 * _batch_device: d_in == d_out allowed; batch * n * 4 words each. */
int toyni_ntt_ext_host(toyni_ntt_ctx* ctx, uint64_t* h_data, uint64_t shift, int inverse);
int toyni_ntt_ext_device(toyni_ntt_ctx* ctx, uint32_t* d_data, uint32_t shift, int inverse, void* stream);
int toyni_ntt_ext_batch_device(toyni_ntt_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, size_t batch, uint32_t shift, int inverse, void* stream);

/* fft_ext of a coefficient vector shorter than the domain (src/math/domain.rs:134-151 pads every coordinate column): the interleaved
 * low-degree extension, padding implied (see toyni_lde_device).  Ext elements are 4 words each (AoS) on both sides.
 * host: ncoeffs <= n Ext coefficients (4 * ncoeffs u64) in, n Ext evaluations (4 * n u64) out, only the coefficients uploaded;
 * device: `batch` vectors of (n >> log_blowup) Ext coefficients (packed u32 AoS) in, n Ext evaluations each out, out of place. */
int toyni_lde_ext_host(toyni_ntt_ctx* ctx, const uint64_t* h_coeffs, size_t ncoeffs, uint64_t* h_out, uint64_t shift);
int toyni_lde_ext_device(toyni_ntt_ctx* ctx, const uint32_t* d_coeffs, uint32_t* d_out, unsigned log_blowup, uint32_t shift, void* stream);
int toyni_lde_ext_batch_device(toyni_ntt_ctx* ctx, const uint32_t* d_coeffs, uint32_t* d_out, size_t batch, unsigned log_blowup, uint32_t shift, void* stream);

/* Multi-GPU 4-step transform of one size-n vector (n = n1 * n2 over G ranks, one all-to-all): the twiddle between
 * the two local stages, d_data[r][k] *= w_n^(+-(row0 + r) * k) for r < rows, k < row_len (ctx of size n;
 * (row0 + rows) * row_len <= n).  The local stages are toyni_ntt_device batches; the exchange is the caller's
 * RCCL all-to-all (toyni_amd/dist.py). */
int toyni_fourstep_twiddle_device(toyni_ntt_ctx* ctx, uint32_t* d_data, size_t rows, size_t row_len, size_t row0, int inverse, void* stream);

/* 2b. One size-n transform over G devices WITHOUT local transposes (one process per GPU; the exchange is the caller's
 * all-to-all).  View x as [M1][S1], M1 = toyni_ntt_ctx_first_pass_points(ctx) (0 when n <= 1024: nothing to split),
 * S1 = n / M1.  The transform's first pass couples only elements of one column, so a rank that owns a block of
 * columns runs it alone (the same strided pass kernel the single-device transform uses); what remains for every k1
 * is an ordinary size-S1 transform (toyni_ntt_device on a size-S1 context):
 *   forward: slab pass (twiddle fused) -> all-to-all of contiguous row blocks -> relayout(0) -> size-S1 row transforms
 *   inverse: size-S1 inverse row transforms -> relayout(1) (twiddle fused) -> all-to-all -> slab pass(inverse)
 * Four HBM sweeps per direction at n = 2^27 instead of the eight of the transpose-based 4-step above -- three with
 * toyni_ntt_slab_rows_device, which folds the relayout into the row transforms' addressing.
 * Layouts: forward input / inverse output = slab [M1][cols_local], element (j1, c) = x[j1 S1 + col_base + c];
 *          forward output / inverse input = rows [rows_local][S1], element (r, k') = X[(row0 + r) + M1 k'].
 * cols_local and rows_local are powers of two, cols_local >= 32.  (src/ntt.rs:11-81 has no multi-device form: values
 * are pinned by the single-device transform and the oracle on the gathered result.) */
size_t toyni_ntt_ctx_first_pass_points(const toyni_ntt_ctx* ctx);
size_t toyni_first_pass_points(uint32_t n);   /* the same from n alone: no context, no device (0: n <= 1024 or not a valid size) */
/* in place on the slab.  inverse = 0: M1-point column transforms times w_n^((col_base + c) k1);
 * inverse = 1: the closing inverse column transforms, scaled by 1/M1 (col_base is not used: the twiddle was applied
 * by the relayout on the other side of the exchange) */
int toyni_ntt_slab_pass_device(toyni_ntt_ctx* ctx, uint32_t* d_slab, size_t cols_local, size_t col_base, int inverse, void* stream);
/* W = S1 / parts.  inverse = 0 (after the exchange):  in [parts][rows_local][W] -> out [rows_local][parts][W] = [rows_local][S1];
 * inverse = 1 (before the exchange): in [rows_local][S1] -> out [parts][rows_local][W], times w_n^-((row0 + r) j').
 * Out of place (d_in != d_out), both 16-byte aligned. */
int toyni_ntt_slab_relayout_device(toyni_ntt_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, size_t rows_local, size_t row0,
                                   size_t parts, int inverse, void* stream);
/* The relayout and the size-S1 row transforms as ONE step either side of the exchange (round 5), `row_ctx` = a context of size S1 on
 * the same device:
 *   inverse = 0: d_in = the received pieces [parts][rows_local][W]  ->  d_out = rows [rows_local][S1], transformed
 *   inverse = 1: d_in = rows [rows_local][S1]  ->  d_out = pieces, inverse-transformed (1/S1) and times w_n^-((row0 + r) j')
 * Where the pass shapes the launch takes can address the pieces layout, no relayout sweep exists: the first pass of the forward row
 * transforms reads the pieces, the last pass of the inverse ones writes them -- three HBM sweeps per direction around the exchange
 * instead of four; otherwise (a few rows, rows of at most 1024 points, a chunked context) the two steps above run one after the
 * other.  Same results either way; *fused (may be NULL) reports which ran.  Out of place; the inverse form may overwrite d_in.
 * d_in and d_out 16-byte aligned (TOYNI_E_RANGE otherwise, whichever form would run). */
int toyni_ntt_slab_rows_device(toyni_ntt_ctx* ctx, toyni_ntt_ctx* row_ctx, uint32_t* d_in, uint32_t* d_out, size_t rows_local, size_t row0,
                               size_t parts, int inverse, int* fused, void* stream);

/* 2c. The same transform driven from ONE host process over G = ndev devices (G a power of two; Toyni is a single process,
 * src/ntt.rs:128-141): slab pass -> ONE exchange -> relayout -> row transforms on every device, contexts, streams and
 * landing buffers cached per (device list, n).  `exchange` selects how the one exchange step moves its G x G blocks:
 *   TOYNI_EXCHANGE_PEER_COPY  every destination pulls its blocks with hipMemcpyPeerAsync (xGMI), one copy stream per
 *                             source so that all incoming links are busy at once; the only form that accepts a device
 *                             listed more than once (lanes on one device: the copy is then device-local).  The environment
 *                             variable TOYNI_SLAB_PIECES = K (power of two, default 1) issues the exchange as K pieces of every
 *                             row block, so that the work on piece q overlaps the transfer of the pieces after it
 *   TOYNI_EXCHANGE_RCCL       one ncclGroupStart / ncclSend + ncclRecv per peer / ncclGroupEnd over ncclCommInitAll
 *                             communicators; librccl is loaded on first use (dlopen), TOYNI_E_NO_RCCL if it is absent
 * Both entry points block until the transform is complete on every device -- on error paths too: no stream of the group still
 * touches the caller's buffers when they return.  Peer access between the listed devices is checked (TOYNI_E_NO_PEER_ACCESS), and the
 * first call on a device list that spans more than one device runs one n = 2^18 transform through the same exchange and compares
 * it with the single-device result (TOYNI_E_SELF_CHECK on a mismatch; a few ms, once per device list and exchange kind).
 * TOYNI_VERBOSE=1 prints the lane -> device / PCI bus table and the self-check's verdict to stderr.
 * _device: d_slabs[g] = device g's [M1][S1/G] column slab, d_rows[g] = its [M1/G][S1] row block (layouts of 2b, packed u32,
 *          resident on devices[g]).  forward: slabs in (OVERWRITTEN), rows out; inverse: rows in (OVERWRITTEN), slabs out.
 * _host:   n u64 elements in natural order, in place (x -> X or X -> x); every lane uploads / downloads its own strided share. */
#define TOYNI_EXCHANGE_PEER_COPY 0
#define TOYNI_EXCHANGE_RCCL 1
int toyni_ntt_slab_multi_gpu_device(const int* devices, int ndev, uint32_t n, uint32_t* const* d_slabs, uint32_t* const* d_rows,
                                    int inverse, int exchange);
int toyni_ntt_slab_multi_gpu_host(const int* devices, int ndev, uint32_t n, uint64_t* h_data, int inverse, int exchange);

/* Domain points on the device: d_out[i] = shift * w_m^i, i < m (roots_of_unity_domain, src/ntt.rs:69-81, with shift = 1;
 * BabyBearDomain::elements, src/math/domain.rs:61-69) -- the xs that fri_fold and the prover's pointwise steps consume.
 * m: power of two <= the context's n.  The reference's serial multiply chain becomes independent table lookups. */
int toyni_domain_elements_device(toyni_ntt_ctx* ctx, uint32_t* d_out, size_t m, uint32_t shift, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3. FRI pairwise fold (net-new on the device; oracle src/math/fri.rs:27-48)
 *    out[i] = (a + b)/2 + (a - b)/2 * beta / x_i,  a = evals[i], b = evals[i + m/2],  i < m/2
 * ---------------------------------------------------------------------------------------------- */
/* Structured points x_i = x0 * w_m^i (the prover's layers: x0 = shift^(2^k), src/fibonacci.rs:214,228-231).
 * ctx: any context whose n >= m (its inverse-root table is used).  m even power of two >= 2.  Async on stream. */
int toyni_fri_fold_device(toyni_ntt_ctx* ctx, const uint32_t* d_evals, uint32_t* d_out, size_t m, uint32_t beta, uint32_t x0, void* stream);

/* The prover's whole fold loop (src/fibonacci.rs:222-245) without the Merkle commits: nfolds layers of
 * a size-n codeword on the coset shift * <w_n>; layer k (size n >> (k+1)) is written at
 * d_layers + (n - (n >> k)) ... i.e. back to back: n/2, n/4, ...  betas: host array of nfolds challenges. */
int toyni_fri_fold_layers_device(toyni_ntt_ctx* ctx, const uint32_t* d_evals, uint32_t* d_layers, const uint32_t* betas, unsigned nfolds, uint32_t shift, void* stream);

/* Explicit points, the reference's signature fri_fold(evals, xs, beta): only xs[0 .. m/2) is read. */
int toyni_fri_fold_xs_device(const uint32_t* d_evals, const uint32_t* d_xs, uint32_t* d_out, size_t m, uint32_t beta, void* stream);
/* Host-slice form of the same (u64 elements, blocking): out has len/2 elements. */
int toyni_fri_fold_host(uint64_t* h_out, const uint64_t* h_evals, size_t len, const uint64_t* h_xs, uint64_t beta);

/* Extension-field codewords, fri_fold_ext (src/math/fri.rs:7-25): values and beta in Ext = F_p[X]/(X^4 - 11)
 * (src/ext.rs), points in the base field.  Elements are AoS: 4 consecutive words c0..c3 (u32 on the device, u64 on
 * the host = #[repr(C)] Ext { c: [BabyBear; 4] }).  m / len count ELEMENTS.  beta = 4 canonical coordinates.  Device forms: d_evals and
 * d_out 16-byte aligned (TOYNI_E_RANGE otherwise), d_xs 4-byte. */
int toyni_fri_fold_ext_device(toyni_ntt_ctx* ctx, const uint32_t* d_evals, uint32_t* d_out, size_t m, const uint32_t beta[4], uint32_t x0, void* stream);
int toyni_fri_fold_ext_xs_device(const uint32_t* d_evals, const uint32_t* d_xs, uint32_t* d_out, size_t m, const uint32_t beta[4], void* stream);
int toyni_fri_fold_ext_host(uint64_t* h_out, const uint64_t* h_evals, size_t len, const uint64_t* h_xs, const uint64_t beta[4]);

/* ------------------------------------------------------------------------------------------------
 * 3b. Merkle commitment of a layer (oracle: src/merkle.rs:25-48,105-123 and the leaf format of
 *     build_merkle_tree / build_unsalted_tree, src/fibonacci.rs:340-361).  leaf = SHA256(0x00 || salt[16] || value as 8 LE
 *     bytes) -- or 0x00 || value bytes when salts == NULL; node = SHA256(0x01 || left || right); odd levels duplicate
 *     their last node.  Output: ALL levels back to back as 32-byte digests (leaf hashes first, root last) =
 *     MerkleTree::levels; toyni_merkle_total_digests(n) digests.  d_levels / d_salts 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
size_t toyni_merkle_total_digests(size_t n);
int toyni_merkle_commit_device(const uint32_t* d_values, const uint8_t* d_salts, size_t n, uint8_t* d_levels, void* stream);
int toyni_merkle_commit_host(const uint64_t* h_values, const uint8_t* h_salts, size_t n, uint8_t* h_levels);

/* ------------------------------------------------------------------------------------------------
 * 3d. Merkle commitment whose leaf is one ROW of an n x width matrix of field elements, and the openings of such rows: a trace of
 *     `width` columns under ONE tree, one authentication path per query.  Byte for byte MerkleTree::new (src/merkle.rs:16-48,
 *     108-114) over
 *         leaf_i = [salt_i (16 bytes)] || v(i,0).to_bytes() || ... || v(i,width-1).to_bytes()
 *     (to_bytes = 8 LE bytes of the canonical residue, src/babybear.rs:53-55; salt first as in build_merkle_tree, absent when the
 *     salts pointer is NULL).  width = 1 is the leaf of 3b: the same bytes as toyni_merkle_commit_device.  Two layouts:
 *       TOYNI_ROWS_COLUMN_MAJOR  element (i, c) at d_values[c * col_stride + i], col_stride >= n: what the batched transforms and
 *                                toyni_lde_device(batch = width) write (col_stride = n), committed as it lies -- no transpose.  The
 *                                words between n and col_stride of a column are never read.
 *       TOYNI_ROWS_ROW_MAJOR     element (i, c) at d_values[i * width + c] (col_stride ignored): an Ext vector (AoS) is width 4,
 *                                its leaf Ext::to_bytes (src/ext.rs:83-89).  16-byte loads when width is a multiple of 4 and d_values
 *                                is 16-byte aligned, word loads otherwise; same result.
 *     d_levels: the layout of toyni_merkle_commit_device (toyni_merkle_total_digests(n) digests, leaf hashes first, root last).
 *     Refused with TOYNI_E_RANGE before anything is enqueued: width == 0 or > 65536, an unknown layout, col_stride < n (column-major),
 *     d_levels / d_salts not 16-byte aligned, d_values / d_indices not 4-byte aligned, d_out not 8-byte aligned.  n == 0 succeeds and
 *     writes nothing.  A leaf costs ceil((8 width + 16 salted + 10) / 64) compressions.
 * ---------------------------------------------------------------------------------------------- */
#define TOYNI_ROWS_COLUMN_MAJOR 0
#define TOYNI_ROWS_ROW_MAJOR 1
size_t toyni_merkle_row_leaf_bytes(size_t width, int salted);          /* 16 * salted + 8 * width */
int toyni_merkle_commit_rows_device(const uint32_t* d_values, size_t n, size_t width, int layout, size_t col_stride,
                                    const uint8_t* d_salts, uint8_t* d_levels, void* stream);
/* Host-slice form: h_values row-major n x width u64 elements, reduced mod p like BabyBear::new; h_salts n x 16 bytes or NULL;
 * h_levels toyni_merkle_total_digests(n) x 32 bytes out.  Blocking. */
int toyni_merkle_commit_rows_host(const uint64_t* h_values, size_t n, size_t width, const uint8_t* h_salts, uint8_t* h_levels);
/* Openings of nidx rows, gathered on the device into nidx records of toyni_merkle_open_rows_record_bytes(n, width) bytes each:
 * depth x 32 path bytes | 16 salt bytes (zero if d_salts is NULL) | width x 8 value bytes in leaf order | depth position bytes
 * (1 = the sibling is the LEFT input), padding zero to a multiple of 8.  Every byte of a record is written.  For width = 1 this is
 * the record of toyni_merkle_open_device.  The indices are device data: each < n is the caller's contract. */
size_t toyni_merkle_open_rows_record_bytes(size_t n, size_t width);
int toyni_merkle_open_rows_device(const uint8_t* d_levels, size_t n, const uint32_t* d_values, size_t width, int layout,
                                  size_t col_stride, const uint8_t* d_salts, const uint32_t* d_indices, size_t nidx,
                                  uint8_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3e. Between "committed" and "folded" for a trace of several columns: the out-of-domain values of every column in one call, and the
 *     DEEP codeword of any set of (column, rotation) terms over a column-major matrix -- the general form of toyni_poly_eval_device
 *     and toyni_fib_deep_device (3c), inside the same protocol shape: z and the weights are base-field elements (squeeze_challenge,
 *     src/transcript.rs:34-40) and there is one common denominator x - z (src/fibonacci.rs:193-196).  With 3d the sequence
 *         batched inverse transform -> toyni_lde_device(batch = w) -> toyni_merkle_commit_rows_device -> toyni_poly_eval_batch_device
 *         -> toyni_deep_combine_device -> toyni_fri_commit_phase_device -> toyni_merkle_open_rows_device
 *     stays on the device; the AIR's constraint evaluation between the commitment and the quotient is 3f.  A staged AIR adds one stage
 *     after the main columns' commitment: the per-row terms from a 3f program at log_blowup = 0 -> toyni_column_scan_device (3g) -> the
 *     accumulator columns through the same inverse transform, toyni_lde_device and toyni_merkle_commit_rows_device as a second matrix.
 *     Under an Ext challenge gamma that stage is toyni_column_scan_ext_device (3i): each accumulator is four base columns of that matrix.
 *     Both calls are asynchronous on `stream`, take packed-u32 canonical residues and write canonical residues.  Device pointers are
 *     4-byte aligned.  `points` and `terms` are host arrays that the caller may reuse as soon as the call returns.  Both calls may use the
 *     context's per-stream intermediate buffer (calls on one stream run in order; use one stream per concurrent call).
 *     Refused before anything is enqueued -- TOYNI_E_NULL for a null context or pointer; TOYNI_E_RANGE for: npoints outside 1..4; a
 *     point, z, alpha or value >= p; shift == 0 or >= p; log_blowup > log2 N; stride < ncoeffs with batch > 1; batch >= 2^32; col_stride < N;
 *     width == 0 or > 65536; column >= width; rotation >= N / B; nterms > 2^20; a device pointer that is not 4-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
/* d_out[b * npoints + p] = sum_i d_coeffs[b * stride + i] * points[p]^i,  i < ncoeffs,  b < batch,  1 <= npoints <= 4: every column
 * equals toyni_poly_eval_device on that column.  Two launches for the whole batch.  ncoeffs == 0 writes batch x npoints zeros (the
 * zero polynomial); batch == 0 succeeds and writes nothing. */
int toyni_poly_eval_batch_device(toyni_ntt_ctx* ctx, const uint32_t* d_coeffs, size_t ncoeffs, size_t stride, size_t batch,
                                 const uint32_t* points, unsigned npoints, uint32_t* d_out, void* stream);
typedef struct { uint32_t column, rotation, alpha, value; } toyni_deep_term;
/* With N = the context's n, B = 1 << log_blowup, x_i = shift * w_N^i, M(c, i) = d_values[c * col_stride + i] (the column-major layout
 * of 3d; the words between N and col_stride of a column are never read):
 *   d_i = ( sum_t alpha_t * (M(column_t, (i + rotation_t * B) mod N) - value_t) ) / (x_i - z)
 * i.e. term t is the column's polynomial at g^rotation_t x, g = w_(N/B), against its claimed value at g^rotation_t z.
 * accumulate != 0: d_out[i] = d_out[i] + d_i, so a second matrix (the quotient's, say) is a second call.  The Fibonacci layer of
 * toyni_fib_deep_device is the four terms (0,0,1,t_z) (0,1,1,t_gz) (0,2,1,t_ggz) (1,0,1,q_z), word for word.  Terms may repeat and
 * come in any order.  A point with x_i = z yields 0 for that point alone (with accumulate: adds 0), the rule of
 * toyni_fib_deep_device.  nterms == 0 writes N zeros, or leaves d_out alone when accumulating.  d_out must not overlap the matrix.
 * The matrix is read by 16-byte loads where the column's first word is 16-byte aligned and rotation * B is a multiple of 4 (N >= 8),
 * by word loads otherwise; the result is the same.  Up to 64 terms travel inside the kernel's arguments.  A longer table is copied
 * from a pinned staging ring of the context into its per-stream buffer by a stream-ordered copy (the call stays asynchronous; when
 * the ring wraps, once per 64 KiB of tables at the least, the call first waits for the stream): with more than 64 terms the call
 * cannot be captured into a HIP graph. */
int toyni_deep_combine_device(toyni_ntt_ctx* ctx, const uint32_t* d_values, size_t width, size_t col_stride, unsigned log_blowup,
                              uint32_t shift, uint32_t z, const toyni_deep_term* terms, size_t nterms, int accumulate,
                              uint32_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3f. The constraints of any AIR, evaluated into the quotient codeword: the step between toyni_merkle_commit_rows_device and the
 *     quotient's own commitment that 3e left to the caller, and the general form of toyni_fib_quotient_device (3c).  A constraint
 *     system is a small straight-line program over registers r[0 .. nregs), nregs <= TOYNI_AIR_MAX_REGS; every point of the LDE
 *     coset runs it on a register file of its own.  With N = the context's n, B = 1 << log_blowup, n = N / B, x_i = shift * w_N^i,
 *     g = w_n, M_m(c, i) = mats[m].d_values[c * mats[m].col_stride + i] (the column-major layout toyni_lde_device(batch = w) writes
 *     and 3d / 3e read; the words between N and col_stride are never read), an instruction does at point i:
 *         TOYNI_AIR_CELL    r[dst] = M_b(imm, (i + a * B) mod N)   matrix b < 4, rotation a, column imm: the column's polynomial at g^a x_i
 *         TOYNI_AIR_CONST   r[dst] = imm                            imm < p
 *         TOYNI_AIR_X       r[dst] = x_i
 *         TOYNI_AIR_XINV    r[dst] = (x_i - imm)^-1                 imm < p; 0 where x_i = imm, the rule of toyni_deep_combine_device
 *         TOYNI_AIR_ADD / _SUB / _MUL   r[dst] = r[a] o r[b]
 *         TOYNI_AIR_EMIT    constraint number imm has the value r[a]; b = 0: it joins the numerator that is divided by
 *                           Z_H(x) = x^n - 1; b = 1: it is added undivided (a boundary constraint already divided through XINV)
 *     and a call with the weights of its Fiat-Shamir challenge (base-field elements, as in 3e) computes
 *         c_i = sum_{EMIT k, b = 0} weights[k] * value_k(i)
 *         q_i = c_i / (x_i^n - 1) + sum_{EMIT k, b = 1} weights[k] * value_k(i)
 *     A constraint number may be emitted more than once; its values add.  Exact field arithmetic on canonical residues throughout.
 *     The quotient of toyni_fib_quotient_device (src/fibonacci.rs:133-150) is the 13 instructions
 *         CELL(0,0) CELL(0,1) CELL(0,2) ADD SUB X CONST(g^(n-1)) SUB MUL CONST(g^(n-2)) SUB MUL EMIT(0, b = 0)   with weights = {1},
 *     word for word.
 * ---------------------------------------------------------------------------------------------- */
#define TOYNI_AIR_MAX_REGS 64
#define TOYNI_AIR_MAX_MATRICES 4
#define TOYNI_AIR_CELL 0
#define TOYNI_AIR_CONST 1
#define TOYNI_AIR_X 2
#define TOYNI_AIR_XINV 3
#define TOYNI_AIR_ADD 4
#define TOYNI_AIR_SUB 5
#define TOYNI_AIR_MUL 6
#define TOYNI_AIR_EMIT 7
typedef struct { uint8_t op, dst, a, b; uint32_t imm; } toyni_air_insn;
typedef struct { const uint32_t* d_values; size_t width, col_stride; } toyni_air_matrix;
/* What a call must supply: nregs = highest register + 1, nconstraints = highest EMIT number + 1, nmatrices = highest matrix + 1,
 * min_width[m] = highest column of matrix m + 1 (0: the program does not read it), max_rotation, divides_by_zh = some EMIT has b = 0. */
typedef struct { uint32_t ninsns, nregs, nconstraints, nmatrices, max_rotation, divides_by_zh;
                 uint32_t min_width[TOYNI_AIR_MAX_MATRICES]; } toyni_air_info;
typedef struct toyni_air_program toyni_air_program;
/* Validation, on the host alone (no device, no context).  TOYNI_E_NULL for a null argument; TOYNI_E_RANGE for: ninsns == 0 or
 * > 65536; an unknown op; a dst, a or b register >= 64; a register read before any instruction wrote it (the program is a straight
 * line: one scan); CONST or XINV with imm >= p; CELL with matrix >= 4 or column >= 65536; EMIT with imm >= 65536 or b > 1; no EMIT.
 * The register rules bind the fields an op uses as registers: dst of every op but EMIT, a and b of ADD / SUB / MUL, a of EMIT.  CELL's
 * a and b are a rotation and a matrix, EMIT's b is the flag.  The fields an op does not use (a and b of CONST / X / XINV, imm of X and
 * of ADD / SUB / MUL, dst of EMIT) are ignored and not checked: write 0 there. */
int toyni_air_program_check(const toyni_air_insn* insns, size_t ninsns, toyni_air_info* info);
/* The same check, then the program in the device's form (constants in Montgomery form) uploaded to ctx's device; blocking.  The
 * program serves every context on that device, any number of calls and streams at a time.  toyni_air_program_destroy is null-safe
 * and waits for the device first. */
int toyni_air_program_create(toyni_ntt_ctx* ctx, const toyni_air_insn* insns, size_t ninsns, toyni_air_program** out);
int toyni_air_program_destroy(toyni_air_program* prog);
int toyni_air_program_info(const toyni_air_program* prog, toyni_air_info* info);
/* Runs the program at every point of the coset and writes q (and c, unless d_c_out is NULL).  Asynchronous on `stream`; packed-u32
 * canonical residues in and out; `mats` and `weights` are host arrays that the caller may reuse as soon as the call returns.
 * accumulate != 0: d_q_out[i] += q_i and d_c_out[i] += c_i.  Outputs must not overlap a matrix.
 * Refused before anything is enqueued, the outputs untouched -- TOYNI_E_NULL for a null context, program, weights or d_q_out (or
 * mats with nmats > 0); TOYNI_E_RANGE for: nmats < info.nmatrices or > 4; a matrix the program reads with a null d_values,
 * width < min_width[m], width > 65536 or col_stride < N; max_rotation >= N / B; log_blowup > log2 N; shift == 0 or >= p;
 * nweights < nconstraints or > 65536; a weight >= p; a device pointer that is not 4-byte aligned; a program created on another
 * device.  TOYNI_E_ZERO_INVERSE, as toyni_fib_quotient_device, when divides_by_zh is set and Z_H vanishes on the coset.
 * Cells are read by 16-byte loads where the column's first word is 16-byte aligned and rotation * B is a multiple of 4 (N >= 4), by
 * word loads otherwise, and the outputs are written by 16-byte stores where they are 16-byte aligned; the result is the same.  The
 * register file lives in LDS, nregs x 16 bytes per thread, in workgroups of the largest of 256 / 128 / 64 threads that keeps it within
 * 64 KiB: a program that needs few registers runs at a higher occupancy.  1 / Z_H costs one inversion per residue class i mod B and
 * workgroup where B <= 256 and the 4 B bytes fit behind the register file, one per four points otherwise.
 * Up to 64 weights travel inside the kernel's arguments, and such a call can be captured into a HIP graph.  More are copied from the
 * context's pinned staging ring into its per-stream buffer by a stream-ordered copy, as the term table of toyni_deep_combine_device
 * (the call stays asynchronous; it cannot be captured). */
int toyni_air_quotient_device(toyni_ntt_ctx* ctx, const toyni_air_program* prog, const toyni_air_matrix* mats, size_t nmats,
                              unsigned log_blowup, uint32_t shift, const uint32_t* weights, size_t nweights, uint32_t* d_c_out,
                              uint32_t* d_q_out, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3g. Accumulator columns: the auxiliary columns of a staged AIR, built from committed columns and a challenge gamma --
 *         the running product of a permutation argument   z_{i+1} = z_i * (gamma + a_i) / (gamma + b_i)
 *         the running sum of a LogUp lookup               s_{i+1} = s_i + 1 / (gamma + v_i) - m_i / (gamma + t_i)
 *     (src/ext.rs:1-8 names "lookup/permutation challenges" and "accumulators" as what a STARK over this field carries).  The per-row
 *     numerator and denominator of such a term come from 3f: a program with undivided EMITs, run with log_blowup = 0 and shift = 1
 *     on a context of the trace length, weights (1, 0) and (0, 1).  What is new here is the inversion of n values that are data, and
 *     the one dependency from row i to row i + 1 in this library.  Inside the protocol shape of 3e / 3f: base-field challenges and
 *     base-field columns.
 *     Asynchronous on `stream`; packed-u32 canonical residues in and out.  The context lends its device, its lock and its per-stream
 *     intermediate buffer (2 words per tile and column); n is NOT tied to the context's size.
 *     Size: 1 <= n <= 2^27, any n, not only powers of two.  batch == 0 or n == 0 succeeds and writes nothing.
 *     Exactness: + and * mod p are associative and commutative, so every evaluation order gives the same words: the result is the
 *     exact residue, bit for bit, at every launch shape.
 *     In place: d_out may be exactly d_num or exactly d_den, with the same stride.  Any other overlap is the caller's error.
 *     Refused before anything is enqueued, the outputs untouched and the context not touched -- TOYNI_E_NULL for a null ctx, d_out or
 *     init, or both operands null; TOYNI_E_RANGE for: an unknown op; n > 2^27; a stride < n with batch > 1; batch >= 2^16; an init
 *     value >= p; a device pointer that is not 4-byte aligned.
 *     Loads and stores: a column whose first word is 16-byte aligned is read and written 16 bytes at a time, any other by word
 *     accesses; the result is the same.
 *     Three launches, each ordered after the last by the stream -- per-tile aggregates on a grid of (tile, column); one workgroup per
 *     column scanning that column's aggregates; the scan inside every tile on the same grid -- and a single launch, grid = the columns,
 *     for n <= one tile.  No workgroup waits for another.  The seeds travel inside the kernel arguments, 64 columns to a launch
 *     sequence, so a call on a warm context only enqueues kernels and can be captured into a HIP graph (with the caveat of section 4).
 * ---------------------------------------------------------------------------------------------- */
#define TOYNI_SCAN_SUM 0
#define TOYNI_SCAN_PRODUCT 1
size_t toyni_column_scan_tile(void);      /* elements one workgroup owns (a power of two): n <= this takes the single launch */
/* out[i] = in[i]^-1, and 0 where in[i] = 0 (the rule of XINV / toyni_deep_combine_device).  *d_zero_count (may be NULL) = number of
 * zeros met (cleared by a stream-ordered fill ahead of the kernel).  d_out == d_in allowed.  No context: the current device.
 * One Fermat inversion per 8 values (Montgomery's trick).  TOYNI_E_NULL for a null d_in or d_out; TOYNI_E_RANGE for count > 2^32 or a
 * pointer that is not 4-byte aligned.  count == 0 succeeds (and clears the count). */
int toyni_batch_inverse_device(const uint32_t* d_in, uint32_t* d_out, size_t count, uint32_t* d_zero_count, void* stream);
/* For each of `batch` columns b (column b of an operand starts at ptr + b * its stride; strides >= n), with
 *   term_i = num_i / den_i   (d_num == NULL: 1 / den_i;  d_den == NULL: num_i;  den_i == 0: term_i = 0 and the zero is counted)
 * the EXCLUSIVE running value, which is what an accumulator column is:
 *   out[0] = init[b];  out[i] = out[i-1] (+ or *) term_{i-1},  0 < i < n
 *   d_totals[2b] = out[n-1] (+ or *) term_{n-1}   (the wrap-around value: a valid argument has it equal to init[b])
 *   d_totals[2b+1] = zero denominators met in column b.
 * init: host array of `batch` canonical residues, reusable on return.  d_totals may be NULL.  The words between n and the stride of
 * a column are neither read nor written. */
int toyni_column_scan_device(toyni_ntt_ctx* ctx, const uint32_t* d_num, size_t num_stride, const uint32_t* d_den, size_t den_stride,
                             uint32_t* d_out, size_t out_stride, size_t n, size_t batch, int op, const uint32_t* init,
                             uint32_t* d_totals, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3h. The two steps of 3e under Ext-valued challenges: the protocol shape a STARK over this field uses (src/ext.rs:1-8 -- the trace and
 *     the evaluation domain stay in the base field, the random challenges and what derives from them live in the quartic extension;
 *     src/transcript.rs:41-55 squeeze_ext_challenge / absorb_ext).  This is the one step that takes base-field columns to an Ext-valued
 *     codeword; with it the sequence
 *         batched inverse transform -> toyni_lde_device(batch = w) -> toyni_merkle_commit_rows_device
 *         -> toyni_poly_eval_ext_batch_device -> toyni_deep_combine_ext_device
 *         -> toyni_fri_commit_phase_ext_device (3j: every round's fold and commitment, the transcript behind a callback)
 *         -> toyni_merkle_open_rows_device(TOYNI_ROWS_ROW_MAJOR, width = 4) per layer
 *     stays on the device. The quotient under Ext weights is toyni_air_quotient_ext_device (3k): toyni_air_quotient_device is linear
 *     in its weights, so four calls with the coordinates of the weights write the same four base columns, at four times the cost of
 *     interpreting the program; the columns join the DEEP combination as a second matrix (accumulate).  An Ext-valued polynomial held as four base columns q_0..q_3 (that quotient, or an Ext
 *     accumulator of 3i) needs no entry point of its own either: evaluate the four columns here and combine on the host,
 *     q(z) = sum_j X^j q_j(z).
 *     Ext = F_p[X]/(X^4 - 11), four consecutive words c0..c3 (section 3).  Every convention is that of 3e: asynchronous on `stream`,
 *     packed-u32 canonical residues in and out, `points`, `z` and `terms` are host arrays that the caller may reuse as soon as the call
 *     returns, the context lends its device, its lock and its per-stream intermediate buffer.
 *     Refused before anything is enqueued, the outputs untouched -- TOYNI_E_NULL for a null context or pointer; TOYNI_E_RANGE for the
 *     list of 3e, with "a point, z, alpha or value >= p" read per coordinate, and for a d_out of toyni_deep_combine_ext_device that is
 *     not 16-byte aligned (the Ext folds that consume it demand that; every other device pointer: 4 bytes).
 * ---------------------------------------------------------------------------------------------- */
/* d_out[(b * npoints + p) * 4 + k] = coordinate k of sum_i d_coeffs[b * stride + i] * points[p]^i,  i < ncoeffs,  b < batch,
 * 1 <= npoints <= 4; points: npoints x 4 words.  Base coefficients, Ext points and values; with a point embedded from the base field
 * coordinate 0 is toyni_poly_eval_batch_device's word and the others are 0.  Two launches for the whole batch.  ncoeffs == 0 writes
 * batch x npoints x 4 zeros; batch == 0 succeeds and writes nothing. */
int toyni_poly_eval_ext_batch_device(toyni_ntt_ctx* ctx, const uint32_t* d_coeffs, size_t ncoeffs, size_t stride, size_t batch,
                                     const uint32_t* points, unsigned npoints, uint32_t* d_out, void* stream);
typedef struct { uint32_t column, rotation; uint32_t alpha[4]; uint32_t value[4]; } toyni_deep_ext_term;
/* With N, B, x_i and M(c, i) as in toyni_deep_combine_device (a base-field, column-major matrix):
 *   d_i = ( sum_t alpha_t * (M(column_t, (i + rotation_t * B) mod N) - value_t) ) / (x_i - z)        in Ext
 * d_out receives N Ext elements (4 N words, element i at d_out + 4 i) and must be 16-byte aligned.  accumulate != 0 adds
 * coordinate-wise, so a second matrix is a second call.  A point with x_i = z (possible only when z1 = z2 = z3 = 0) yields 0 for that
 * point alone.  nterms == 0 writes 4 N zeros, or leaves d_out alone when accumulating.  d_out must not overlap the matrix.  With z, the
 * weights and the values embedded from the base field, coordinate 0 is toyni_deep_combine_device's word and the others are 0.
 * The matrix is read as 3e reads it: 16-byte loads where the column's first word is 16-byte aligned and rotation * B is a multiple of
 * 4 (N >= 4), word loads otherwise.  Up to 64 terms travel inside the kernel's arguments (such a call can be captured into a HIP
 * graph); a longer table goes through the context's pinned staging ring and per-stream buffer exactly as in 3e.
 * The division costs one base-field inversion per 4 points: (x - z)^-1 = adj_z(x) / m_z(x), adj_z(x) = prod_{j=1..3} (x - phi^j(z)) with
 * the conjugates phi^j(z)_k = z_k * zeta^(j k), zeta = 11^((p-1)/4), and m_z = (x - z) adj_z the norm, a quartic with base coefficients. */
int toyni_deep_combine_ext_device(toyni_ntt_ctx* ctx, const uint32_t* d_values, size_t width, size_t col_stride, unsigned log_blowup,
                                  uint32_t shift, const uint32_t z[4], const toyni_deep_ext_term* terms, size_t nterms,
                                  int accumulate, uint32_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3i. The accumulator columns of 3g under an Ext challenge: the permutation product and the LogUp sum with gamma in Ext (about 124
 *     bits instead of 31), so that the staged AIR of 3g lives in the protocol shape of 3h.  The accumulator is then an Ext-valued
 *     column and its terms are Ext quotients.  With it the sequence for a staged AIR
 *         committed main columns -> toyni_column_scan_ext_device -> the 4 x batch base columns through the batched inverse transform,
 *         toyni_lde_device and toyni_merkle_commit_rows_device as a second matrix -> toyni_air_quotient_ext_device (3k: the quotient under Ext
 *         weights) -> toyni_poly_eval_ext_batch_device -> toyni_deep_combine_ext_device
 *     stays on the device.
 *     Layout: an Ext column is FOUR base columns, one per coordinate: coordinate k of element i of Ext column b is at
 *     ptr[(4 b + k) * stride + i], stride >= n, packed-u32 canonical residues -- what four 3f calls with the coordinates of Ext weights
 *     write, what the batched transforms and the column-major row commitment read, and what 3h calls an Ext polynomial held as four
 *     base columns.
 *     Semantics: those of 3g with every value in Ext.  term_i = num_i / den_i; where den_i = 0 (all four coordinates) term_i = 0 and
 *     the zero is counted;  out[0] = init[b];  out[i] = out[i-1] (+ or *) term_{i-1};  d_totals[8 b .. 8 b + 3] = the wrap-around value
 *     out[n-1] (+ or *) term_{n-1},  d_totals[8 b + 4] = the zero denominators met,  d_totals[8 b + 5 .. 8 b + 7] = 0.
 *     Forms: the permutation argument z * (gamma + a_i) / (gamma + b_i) is two width-1 operands with shift = gamma; LogUp
 *     m_i / (gamma + t_i) is a width-1 numerator with shift 0 and a width-1 denominator with shift gamma; arguments over several
 *     columns combined under Ext weights use width-4 operands (four 3f calls: 3f is linear in its weights).
 *     Size: 1 <= n <= 2^27, any n; batch < 2^14; n == 0 or batch == 0 succeeds and writes nothing.  n is NOT tied to the context's size:
 *     the context lends its device, its lock and its per-stream intermediate buffer (5 words per tile and column).
 *     Asynchronous on `stream`.  Exactness: Ext is a commutative field, so every evaluation order gives the same words, at every launch
 *     shape.  In place: d_out may be exactly a width-4 operand's d_values with the same stride; any other overlap is the caller's error.
 *     Loads and stores: 16 bytes at a time where a coordinate column's first word is 16-byte aligned, word accesses otherwise; the result
 *     is the same.  The words between n and a stride are neither read nor written.
 *     Refused before anything is enqueued, the outputs and the context untouched -- TOYNI_E_NULL for a null ctx, d_out or init;
 *     TOYNI_E_RANGE for: both operands absent; a width not in {0, 1, 4}; width > 0 with null d_values; an unknown op; n > 2^27; an operand
 *     stride < n where more than one base column is addressed (width 4, or batch > 1); out_stride < n; batch >= 2^14; an init or shift
 *     coordinate >= p; a device pointer that is not 4-byte aligned.
 *     The launches are those of 3g (per-tile aggregates; one workgroup per column scanning them in rounds; the scan inside each tile;
 *     one launch for n <= one tile), no workgroup waits for another.  Seeds and shifts travel inside the kernel arguments, 16 Ext
 *     columns to a launch sequence, so a call on a warm context only enqueues kernels and can be captured into a HIP graph (with the
 *     caveat of section 4).  A width-1 denominator costs one base inversion per 4 elements through the norm form of 3h (z = -shift, the
 *     column's values as points); a width-4 denominator one per 4 elements through the tower F_p < F_p[Y]/(Y^2 - 11) < Ext, Y = X^2:
 *     a = A0 + A1 X,  B = A0^2 - Y A1^2 = B0 + B1 Y,  N = B0^2 - 11 B1^2,  a^-1 = (A0 - A1 X)(B0 - B1 Y) / N,  N = 0 only for a = 0.
 * ---------------------------------------------------------------------------------------------- */
typedef struct { const uint32_t* d_values; size_t stride; uint32_t width; uint32_t shift[4]; } toyni_ext_operand;
/* element i of column b of an operand:
 *   width 4: shift + (d_values[(4 b + k) * stride + i])_k       an Ext column
 *   width 1: shift + embed(d_values[b * stride + i])            a base column plus an Ext constant: gamma + v_i
 *   width 0 (or a NULL operand pointer): the constant 1; the other fields are ignored                         */
size_t toyni_column_scan_ext_tile(void);  /* elements one workgroup owns (a power of two): n <= this takes the single launch */
/* init: host array of batch x 4 canonical residues, reusable on return, as the operands are.  d_totals: batch x 8 words, may be NULL. */
int toyni_column_scan_ext_device(toyni_ntt_ctx* ctx, const toyni_ext_operand* num, const toyni_ext_operand* den, uint32_t* d_out,
                                 size_t out_stride, size_t n, size_t batch, int op, const uint32_t* init, uint32_t* d_totals, void* stream);
/* out_i = in_i^-1 in Ext, and 0 for 0, counted into *d_zero_count (may be NULL; cleared by a stream-ordered fill ahead of the kernel).
 * The input and the output are each ONE Ext column of `count` elements (four base columns in_stride / out_stride apart, strides >=
 * count).  d_out == d_in is allowed with equal strides.  No context: the current device.  TOYNI_E_NULL for a null d_in or d_out;
 * TOYNI_E_RANGE for count > 2^32, a stride < count or a pointer that is not 4-byte aligned.  count == 0 succeeds (and clears the count). */
int toyni_batch_inverse_ext_device(const uint32_t* d_in, size_t in_stride, uint32_t* d_out, size_t out_stride, size_t count,
                                   uint32_t* d_zero_count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3j. The FRI commit phase over Ext-valued layers: what 3c's toyni_fri_fold_commit_device and toyni_fri_commit_phase_device are to a
 *     base-field codeword, for the Ext codeword that toyni_deep_combine_ext_device (3h) leaves on the device.  An Ext layer is a
 *     row-major matrix of width 4 (element i at ptr + 4 i, section 3), its commitment the row commitment of 3d: leaf i =
 *     [salt_i (16)] || Ext::to_bytes (32), tree layout and opening record as 3d fixes them.  The leaf message 00 || leaf is 49 bytes
 *     salted and 33 unsalted: ONE SHA-256 block, hashed in the fold's own sweep from the registers that hold the folded element.
 *     Openings need nothing new: a layer is opened with toyni_merkle_open_rows_device(width = 4, TOYNI_ROWS_ROW_MAJOR), one call per
 *     layer, on the layer's words in d_out / d_layers and its tree in d_levels.
 *     Alignment: every device pointer here (d_evals, d_out, d_layer0, d_layers, d_salts, d_levels) is 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
/* One round: d_out = fri_fold_ext(d_evals) on the points x0 w_m^i with the Ext challenge beta, AND the Merkle tree of the folded
 * layer in d_levels -- byte for byte what
 *     toyni_fri_fold_ext_device(ctx, d_evals, d_out, m, beta, x0) followed by
 *     toyni_merkle_commit_rows_device(d_out, m / 2, 4, TOYNI_ROWS_ROW_MAJOR, 0, d_salts, d_levels)
 * write, in one launch less and without the second read of the layer.  m counts Ext elements (4 m words in, 2 m out);
 * d_salts = (m / 2) x 16 bytes, or NULL for an unsalted tree; d_levels = toyni_merkle_total_digests(m / 2) x 32 bytes.  d_out must not
 * overlap d_evals.  m == 0 succeeds and writes nothing; m == 2 gives a tree of one digest, the leaf.  Asynchronous on `stream`; on a
 * warm context the call only enqueues a linear chain of kernels and can be captured into a HIP graph (caveat of section 4).
 * Refused before anything is enqueued, the outputs untouched: TOYNI_E_NULL for a null ctx, d_evals, d_out, beta or d_levels;
 * TOYNI_E_ODD_LENGTH for an odd m; TOYNI_E_RANGE for an m that is not a power of two or exceeds the context's n;
 * TOYNI_E_ZERO_INVERSE for x0 == 0; TOYNI_E_RANGE for x0 >= p, a beta coordinate >= p, or a device pointer that is not 16-byte
 * aligned.  All of these but "m exceeds n" are decided on the arguments alone, before the context is read. */
int toyni_fri_fold_commit_ext_device(toyni_ntt_ctx* ctx, const uint32_t* d_evals, uint32_t* d_out, size_t m, const uint32_t beta[4], uint32_t x0,
                                     const uint8_t* d_salts, uint8_t* d_levels, void* stream);
/* The WHOLE fold loop in one blocking call: toyni_fri_commit_phase_device with Ext values and an Ext beta per round
 * (squeeze_ext_challenge, src/transcript.rs:41-55: beta_out receives four canonical residues).  Everything else is 3c's call word for
 * word: it blocks on every path (the stream has drained when it returns, also after a failing callback); the callback runs on the
 * calling thread with the context locked (TOYNI_E_REENTRANT for an entry point on the same context from inside it) and is called once
 * more after the last round with beta_out = NULL; each root reaches the host through the context's pinned notification word; h_roots
 * and rounds_out as there; d_salts holds 16 bytes per leaf for every salted layer back to back, the final layer unsalted; round k
 * folds on x0^(2^k).
 *   d_layer0 : m0 Ext elements (4 m0 words)
 *   d_layers : out, the folded layers back to back: 4 (m0/2 + m0/4 + ... + final_size) words, so every layer starts 16-byte aligned
 *   d_levels : out, their trees back to back (toyni_merkle_total_digests(m_k) x 32 bytes each)
 * Refused before anything is enqueued, the outputs untouched: TOYNI_E_NULL for a null ctx, d_layer0, callback, d_layers or d_levels;
 * TOYNI_E_INVALID_SIZE for an m0 or final_size that is not a power of two, or m0 > n; TOYNI_E_ZERO_INVERSE for x0 == 0; TOYNI_E_RANGE
 * for x0 >= p or a device pointer that is not 16-byte aligned.  A beta coordinate >= p from the callback ends the call with
 * TOYNI_E_RANGE (the rounds before it stay committed). */
typedef int (*toyni_fri_ext_challenge_fn)(void* user, unsigned round, const uint8_t* prev_root32, uint32_t beta_out[4]);
int toyni_fri_commit_phase_ext_device(toyni_ntt_ctx* ctx, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size,
                                      const uint8_t* d_salts, toyni_fri_ext_challenge_fn challenge, void* user, uint32_t* d_layers,
                                      uint8_t* d_levels, uint8_t* h_roots, unsigned* rounds_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3k. The quotient of 3f under Ext weights in ONE call: the last step of the protocol shape of 3h / 3i that was spelled as a
 *     workaround (four calls of toyni_air_quotient_device, one per coordinate of the weights).  The programs, the matrices, the coset
 *     and the TOYNI_AIR_* instruction set are those of 3f, unchanged: toyni_air_program_check / _create serve both calls, and a
 *     program's constraint values stay in the base field.  Only the weights of the Fiat-Shamir challenge are Ext:
 *         C_i = sum_{EMIT k, b = 0} W_k * value_k(i)                                   in Ext = F_p[X]/(X^4 - 11)
 *         Q_i = C_i / Z_H(x_i) + sum_{EMIT k, b = 1} W_k * value_k(i)
 *     weights4: host array of nweights Ext weights, plain canonical residues, coordinate e of weight k at weights4[4 k + e]; reusable
 *     as soon as the call returns.  For constraints written with emit_ext (base constraint 4 k + j = coordinate j of Ext constraint k)
 *     under Ext challenges alpha_k, W_{4 k + j} = alpha_k * X^j.
 *     Outputs: four base columns each, column-major -- coordinate e of Q_i at d_q_out[e * out_stride + i], of C_i at
 *     d_c_out[e * out_stride + i] (d_c_out may be NULL), out_stride >= N: the layout of 3i, which
 *     toyni_merkle_commit_rows_device(TOYNI_ROWS_COLUMN_MAJOR, 4), the batched inverse coset transform,
 *     toyni_poly_eval_ext_batch_device and toyni_deep_combine_ext_device read as it lies.  The words N .. out_stride of a column are
 *     never touched.  accumulate != 0 adds into every column, as in 3f.
 *     By definition column e is, word for word, what toyni_air_quotient_device writes under the base weights weights4[4 k + e]: the
 *     arithmetic is exact, so the four calls and this one agree in every byte.  What differs is the cost: the program is decoded, its
 *     cells are loaded and its register file is walked once per point instead of four times; an EMIT costs four products per point.
 *     Refused before anything is enqueued, the outputs untouched: every refusal of toyni_air_quotient_device (with weights4 for
 *     weights, "a weight >= p" read per coordinate), and TOYNI_E_RANGE for out_stride < N.
 *     The launch shape, the LDS register file and the 1 / Z_H classes are those of 3f.  Each output column is written by 16-byte stores
 *     where that column's own first word is 16-byte aligned (with an out_stride that is no multiple of 4 the columns differ), by word
 *     stores otherwise; the result is the same.  Up to TOYNI_AIR_EXT_INLINE_WEIGHTS Ext weights (1 KiB) travel inside the kernel's
 *     arguments, and such a call can be captured into a HIP graph; more go through the context's pinned staging ring and per-stream
 *     buffer exactly as in 3f (the call stays asynchronous; it cannot be captured).
 * ---------------------------------------------------------------------------------------------- */
#define TOYNI_AIR_EXT_INLINE_WEIGHTS 64
int toyni_air_quotient_ext_device(toyni_ntt_ctx* ctx, const toyni_air_program* prog, const toyni_air_matrix* mats, size_t nmats,
                                  unsigned log_blowup, uint32_t shift, const uint32_t* weights4, size_t nweights,
                                  uint32_t* d_c_out, uint32_t* d_q_out, size_t out_stride, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3l. The Fiat-Shamir transcript in device memory, and the FRI commit phase on it: FiatShamirTranscript (src/transcript.rs) as a
 *     plain struct that kernels absorb into and squeeze from, so that a round's root never has to reach the host before the next
 *     beta exists.  The commit phases of 3c / 3j block on every round (a polled word, a host callback, a launch into an empty
 *     queue); the phases here are asynchronous, take no callback and can be captured into a HIP graph (caveat of section 4), and the
 *     path from the DEEP codeword to the opening records becomes stream-ordered: enqueue everything, synchronise once.
 *     (3m runs the Ext phase on this transcript with FOUR-to-one rounds under coset leaves: half the rounds, lower trees.)
 *     The state has a public layout.  A caller initialises it with toyni_memcpy_h2d_async of a host copy (len = the bytes absorbed so
 *     far, status = 0, reserved = 0; the reference's transcript starts as the 14 bytes "toyni-stark-v1"); there is no init call.
 *     d_tr is device memory, 16-byte aligned.
 *     What the host cannot see -- it never reads len -- is reported through `status`, which is sticky and which the caller reads
 *     after its next synchronisation: an absorb that would pass TOYNI_TRANSCRIPT_CAPACITY leaves the state as it is and stores
 *     TOYNI_E_RANGE there; every operation on a transcript whose status is not 0 leaves the transcript unchanged and writes ZEROS to
 *     its outputs.  (A len beyond the capacity, which only a caller's own copy can produce, is treated the same way.)
 *     All calls are asynchronous on `stream`; each of the four helpers is one small launch (the chains are serial by definition: one
 *     wave).  Refused on the host before anything is enqueued, the outputs untouched: TOYNI_E_NULL for a null pointer (d_bytes with
 *     len == 0 may be null); TOYNI_E_RANGE for a d_tr that is not 16-byte aligned, a word array that is not 4-byte aligned, and what
 *     each call lists.
 * ---------------------------------------------------------------------------------------------- */
#define TOYNI_TRANSCRIPT_CAPACITY 1008
typedef struct { uint32_t len, status, reserved[2]; uint8_t bytes[TOYNI_TRANSCRIPT_CAPACITY]; } toyni_transcript;  /* 1024 B, device, 16-byte aligned */
/* absorb (src/transcript.rs:19-21): appends `len` device-resident bytes -- a root at the end of a d_levels, out-of-domain values.
 * TOYNI_E_RANGE for len > TOYNI_TRANSCRIPT_CAPACITY; len == 0 enqueues nothing. */
int toyni_transcript_absorb_device(toyni_transcript* d_tr, const uint8_t* d_bytes, size_t len, void* stream);
/* squeeze_challenge (:34-40) `count` times: h = SHA256(state), state = h, d_out[k] = (the first 8 bytes of h as a little-endian u64)
 * mod p.  An Ext challenge (:43-50) is count = 4.  TOYNI_E_RANGE for count > 65536; count == 0 enqueues nothing. */
int toyni_transcript_squeeze_device(toyni_transcript* d_tr, uint32_t* d_out, size_t count, void* stream);
/* squeeze_indices(count, max) (:58-72): the same chain with the value taken mod max; a repeated value is dropped, the others are
 * written in order of first appearance.  TOYNI_E_RANGE for count == 0, count > 256, max == 0 or count > max.  The loop is bounded at
 * 64 count + 64 hashes, after which it sets `status` as above (for count <= max unreachable in practice: no input can make the kernel
 * spin). */
int toyni_transcript_squeeze_indices_device(toyni_transcript* d_tr, size_t count, uint32_t max, uint32_t* d_out, void* stream);
/* The positions the queries open in every layer but the final one (src/fibonacci.rs:268-283): layer k = 0 .. rounds - 1 has
 * m_k = m0 >> k elements (rounds = log2(m0 / final_size)) and gets 2 count positions, [i mod (m_k / 2), i mod (m_k / 2) + m_k / 2] per
 * query i = d_indices[q]; the layers' lists lie back to back in d_out (rounds x 2 count words).  Each list feeds
 * toyni_merkle_open_groups_device / toyni_merkle_open_rows_device as it lies.  TOYNI_E_RANGE for an m0 or final_size that is not a
 * power of two, m0 > 2^32, or count > 65536; count == 0 or m0 <= final_size writes nothing. */
int toyni_fri_query_positions_device(const uint32_t* d_indices, size_t count, size_t m0, size_t final_size, uint32_t* d_out, void* stream);
/* The commit phases of 3c (base field) and 3j (Ext) on a device transcript.  Per round: squeeze beta from d_tr (one squeeze; four for
 * the Ext call), fold and commit the folded layer exactly as toyni_fri_fold_commit_device / _ext_device do, absorb the 32-byte root --
 * the operation sequence of the callback phases, where the callback absorbs the previous root and then squeezes and a last call
 * absorbs the last root.  As there, the caller absorbs layer 0's root first (src/fibonacci.rs:205-245).
 * d_layer0, m0, x0, final_size, d_salts, d_layers, d_levels, the alignment rules and the size refusals are those of the callback
 * call with the same element type.  d_betas (may be NULL) receives the plain canonical beta of every round: `rounds` words, 4 rounds
 * for the Ext call.  After the call d_tr is what the host transcript would be: toyni_transcript_squeeze_indices_device continues
 * from it.  m0 <= final_size enqueues nothing and leaves d_tr untouched.  A d_tr whose status is set gives beta = 0 in every round;
 * the layers and trees are still written.
 * No host in the loop: no callback, no pinned word, no download, and the context is locked for the enqueue only.  On a warm context
 * (one earlier call on this stream: the per-stream record buffer exists) the call enqueues one linear chain of kernels.  beta reaches
 * a fold through a small record in that buffer, written by the one-wave kernel behind each tree in the form the fold consumes (the
 * Montgomery form of beta / (2 x_k); the factor tables of beta / 2 for Ext).  From the first round whose folded layer has at most
 * 2^TOYNI_FRI_TAIL_LOG leaves (environment, read once; default 9 = 512 leaves, the most one workgroup holds; -1 = never) one
 * workgroup runs ALL remaining rounds in one launch, layer, tree level and transcript in LDS; both settings write the same bytes. */
int toyni_fri_commit_phase_transcript_device(toyni_ntt_ctx* ctx, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size,
                                             const uint8_t* d_salts, toyni_transcript* d_tr, uint32_t* d_layers, uint8_t* d_levels,
                                             uint32_t* d_betas, void* stream);
int toyni_fri_commit_phase_transcript_ext_device(toyni_ntt_ctx* ctx, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size,
                                                 const uint8_t* d_salts, toyni_transcript* d_tr, uint32_t* d_layers, uint8_t* d_levels,
                                                 uint32_t* d_betas, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3m. The Ext commit phase folding FOUR to one per round, under COSET leaves, on the device transcript of 3l.  The phases of 3c / 3j
 *     / 3l are chains of dependent hashes -- a tree of log m - 1 levels per round, a serial squeeze between rounds -- and this
 *     section makes that chain shorter instead of faster: half the rounds, each tree two levels lower.  The protocol shape is this
 *     library's own (the reference, src/fibonacci.rs, folds two to one; its proof format is untouched).
 *     A layer L of m Ext elements (AoS, section 3) lies on the points x_i = x0 w_m^i.  One round with the Ext challenge beta is
 *         L'  = fri_fold_ext(L,  beta,   points x0   w_m^i)          (toyni_fri_fold_ext_device with x0)
 *         L'' = fri_fold_ext(L', beta^2, points x0^2 w_(m/2)^i)      (toyni_fri_fold_ext_device with x0^2)
 *     so L''[j] = f0 + beta f1 + beta^2 f2 + beta^3 f3 of the cubic through the coset {x, I x, -x, -I x}, I = w_m^(m/4), and depends
 *     on exactly L[j], L[j + m/4], L[j + m/2], L[j + 3m/4].  The arithmetic is exact: the one-sweep kernel and the two calls agree
 *     in every byte.
 *     COSET LEAF: a committed layer of m >= 4 elements has m / 4 leaves,
 *         leaf_j = [salt_j (16)] || to_bytes(L[j]) || to_bytes(L[j + m/4]) || to_bytes(L[j + m/2]) || to_bytes(L[j + 3m/4])
 *     -- the row leaf of 3d with width 16, row j gathered from the four quarters of the layer.  00 || leaf is 145 bytes salted, 129
 *     unsalted: three SHA-256 blocks either way.  Tree layout, node hash and opening record are 3d's with n = m / 4, width = 16:
 *     toyni_merkle_total_digests(m / 4) digests, toyni_merkle_open_rows_record_bytes(m / 4, 16) bytes per record.
 *     THE PHASE: layer k has m_k = m0 >> 2k elements on x0^(4^k) w_(m_k)^i; log2(m0 / final_size) is even and final_size >= 4; every
 *     layer, the final one included, is committed under coset leaves, the final one unsalted.  The transcript sequence is 3l's with
 *     half the rounds: the caller absorbs layer 0's root; per round four squeezes (an Ext beta), fold and commit, absorb the root.
 *     Query indices are drawn with toyni_transcript_squeeze_indices_device(count, max = m0 / 4); query i opens leaf i mod (m_k / 4) of
 *     layer k < R = log2(m0 / final_size) / 2, one record per layer; the final layer travels whole.
 *     Alignment: every device pointer here is 16-byte aligned, except index and word arrays (d_indices, d_betas, the positions),
 *     which are 4-byte aligned, and the opening records (d_out of the open call), 8-byte aligned as in 3d.
 *     All calls are asynchronous on `stream`, enqueue linear chains of kernels and can be captured into a HIP graph (caveat of
 *     section 4; the phase needs a warm context as in 3l).  There is no callback or blocking variant and no base-field variant.
 * ---------------------------------------------------------------------------------------------- */
/* The coset tree of a layer as it lies, and openings of it: byte for byte what toyni_merkle_commit_rows_device /
 * toyni_merkle_open_rows_device (TOYNI_ROWS_ROW_MAJOR, width 16) write on a copy of the layer gathered into m / 4 rows of 16 words.
 * d_salts = (m / 4) x 16 bytes or NULL; d_levels = toyni_merkle_total_digests(m / 4) x 32 bytes; d_indices: nidx leaf numbers, each
 * below m / 4 (not checked, as in 3d); d_out: nidx records.  Layer 0 is committed, and every layer is opened, with these.
 * m == 0 (and nidx == 0) succeeds and writes nothing.  Refused before anything is enqueued, the outputs untouched: TOYNI_E_NULL for
 * a null d_layer, d_levels, d_indices or d_out; TOYNI_E_INVALID_SIZE for an m that is not a power of two or is below 4;
 * TOYNI_E_RANGE for a misaligned pointer, m > 2^33 or nidx >= 2^32. */
int toyni_merkle_commit_cosets_ext_device(const uint32_t* d_layer, size_t m, const uint8_t* d_salts, uint8_t* d_levels, void* stream);
int toyni_merkle_open_cosets_ext_device(const uint8_t* d_levels, size_t m, const uint32_t* d_layer, const uint8_t* d_salts,
                                        const uint32_t* d_indices, size_t nidx, uint8_t* d_out, void* stream);
/* One four-to-one round in one sweep: d_out = L'' (m / 4 elements) and the coset tree of d_out in d_levels (m / 16 leaves; d_salts =
 * (m / 16) x 16 bytes, or NULL for an unsalted tree).  One thread per leaf reads the 16 elements the leaf depends on, folds them in
 * registers and hashes the leaf from the folded words; beta^2 is computed on the host.  d_out must not overlap d_evals; d_evals is
 * only read.  m == 0 succeeds and writes nothing; m == 16 gives a tree of one digest, the leaf.
 * Refused before anything is enqueued, the outputs untouched: TOYNI_E_NULL for a null ctx, d_evals, d_out, beta or d_levels;
 * TOYNI_E_RANGE for an m that is not a power of two, is below 16 or exceeds the context's n; TOYNI_E_ZERO_INVERSE for x0 == 0;
 * TOYNI_E_RANGE for x0 >= p, a beta coordinate >= p, or a device pointer that is not 16-byte aligned.  All of these but "m exceeds n"
 * are decided on the arguments alone, before the context is read. */
int toyni_fri_fold4_commit_ext_device(toyni_ntt_ctx* ctx, const uint32_t* d_evals, uint32_t* d_out, size_t m, const uint32_t beta[4],
                                      uint32_t x0, const uint8_t* d_salts, uint8_t* d_levels, void* stream);
/* The leaves the queries open: R lists of `count` words back to back, list k = d_indices[q] mod (m0 >> (2 k + 2)); each list feeds
 * toyni_merkle_open_cosets_ext_device as it lies.  The refusals of toyni_fri_query_positions_device, and TOYNI_E_INVALID_SIZE for an
 * odd log2(m0 / final_size) or final_size < 4; count == 0 or m0 <= final_size writes nothing. */
int toyni_fri4_query_positions_device(const uint32_t* d_indices, size_t count, size_t m0, size_t final_size, uint32_t* d_out, void* stream);
/* The phase.  Arguments as in toyni_fri_commit_phase_transcript_ext_device, with these sizes:
 *   d_layers : out, the folded layers back to back: 4 (m0/4 + m0/16 + ... + final_size) words
 *   d_salts  : 16 bytes per LEAF of every salted folded layer back to back (m0/16 + m0/64 + ... leaves, the final layer excluded),
 *              or NULL for unsalted trees throughout
 *   d_levels : out, the coset trees back to back (toyni_merkle_total_digests(m_k / 4) x 32 bytes each)
 *   d_betas  : out (may be NULL), 4 R words: beta of every round, plain canonical (beta^2 is not stored)
 * Every round writes exactly what toyni_fri_fold4_commit_ext_device writes for its beta.  m0 <= final_size enqueues nothing and
 * leaves d_tr untouched.  A d_tr whose status is set gives beta = beta^2 = 0 in every round; the layers and trees are still written.
 * No host in the loop, no callback, no blocking; the context is locked for the enqueue only.  beta reaches a fold through a record
 * of two factor tables (beta / 2 and beta^2 / 2, the product formed on the device) in the per-stream buffer of 3l, whose layout for
 * the two-to-one phases is unchanged.  Small rounds run as the same plain chain: the fused tail of 3l is not used here.
 * Refused before anything is enqueued, the outputs untouched: TOYNI_E_NULL for a null ctx, d_layer0, d_tr, d_layers or d_levels;
 * TOYNI_E_INVALID_SIZE for an m0 or final_size that is not a power of two, final_size < 4, an odd log2(m0 / final_size), or m0 > n;
 * TOYNI_E_ZERO_INVERSE for x0 == 0; TOYNI_E_RANGE for x0 >= p or a misaligned pointer. */
int toyni_fri4_commit_phase_transcript_ext_device(toyni_ntt_ctx* ctx, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size,
                                                  const uint8_t* d_salts, toyni_transcript* d_tr, uint32_t* d_layers, uint8_t* d_levels,
                                                  uint32_t* d_betas, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3n. A proof-of-work nonce ("grinding") on the device transcript of 3l: the step between the last absorbed root and
 *     toyni_transcript_squeeze_indices_device.  It buys `bits` bits of soundness that would otherwise be paid in queries, without the
 *     transcript leaving the device.  The protocol is this library's own (the reference has no grinding).  For a transcript whose
 *     state is the bytes S and a 64-bit nonce:
 *         accept(S, nonce, bits)  <=>  the first `bits` bits of SHA256(S || LE64(nonce)) are zero, the most significant bit of digest
 *                                      byte 0 first; 0 <= bits <= 32; bits = 0 accepts every nonce
 *         grind(S, bits, start, log_tries) = the SMALLEST nonce of [start, start + 2^log_tries) that is accepted
 *     and the transcript then absorbs the 8 bytes LE64(nonce), exactly as toyni_transcript_absorb_device would.  The answer is a
 *     function of the arguments alone: never of the grid, the schedule or the run.  A verifier recomputes one hash
 *     (toyni_pow_check_host), checks it and absorbs the same 8 bytes.  bits = 0 still absorbs a nonce (the value `start`).
 * ---------------------------------------------------------------------------------------------- */
#define TOYNI_POW_MAX_BITS 32
#define TOYNI_POW_MAX_LOG_TRIES 40
/* Asynchronous on `stream`: one linear chain of three launches (arm, one wave; search, up to 768 workgroups; finish, one wave), no
 * context, no allocation, no callback, no host read, no environment variable; it can be captured into a graph like its siblings.
 * d_nonce: one word of device memory, 8-byte aligned -- the result and the only scratch the call needs.  Afterwards *d_nonce holds
 * the nonce and d_tr is S || LE64(nonce).  What the host cannot see goes into the sticky `status` by 3l's rules; in each of these
 * cases the transcript's bytes and length stay as they are and *d_nonce = 0: a d_tr whose status is already set; a state with
 * len + 8 > TOYNI_TRANSCRIPT_CAPACITY (sets TOYNI_E_RANGE); a window without an accepted nonce (sets TOYNI_E_RANGE).  The work is
 * bounded by the window: no thread tests more than 2^log_tries / (number of threads) candidates, rounded up.
 * Refused on the host before anything is enqueued, the outputs untouched: TOYNI_E_NULL for a null d_tr or d_nonce; TOYNI_E_RANGE for
 * a d_tr that is not 16-byte or a d_nonce that is not 8-byte aligned, bits > TOYNI_POW_MAX_BITS, log_tries > TOYNI_POW_MAX_LOG_TRIES,
 * or a start + 2^log_tries that exceeds 2^64. */
int toyni_transcript_grind_device(toyni_transcript* d_tr, unsigned bits, uint64_t start, unsigned log_tries, uint64_t* d_nonce,
                                  void* stream);
/* accept(state[0 .. len), nonce, bits) on the host: plain host code, no device.  *accepted = 1 or 0.  TOYNI_E_NULL for a null
 * `accepted` or a null `state` with len > 0 (state may be null when len == 0); TOYNI_E_RANGE for bits > TOYNI_POW_MAX_BITS, with
 * *accepted untouched.  `len` is not bounded by the transcript's capacity. */
int toyni_pow_check_host(const uint8_t* state, size_t len, uint64_t nonce, unsigned bits, int* accepted);

/* ------------------------------------------------------------------------------------------------
 * 3o. From the quotient's root onward without the host: the out-of-domain point z, the out-of-domain values, the DEEP weights and the
 *     DEEP layer of 3h with everything that depends on a challenge read from DEVICE memory.  The host-argument calls of 3h take z, the
 *     weights and the claimed values as host arrays, which costs a caller of 3l a download and a synchronisation per step; with the
 *     calls below the sequence
 *         toyni_transcript_squeeze_ext_point_device -> toyni_poly_eval_ext_batch_dz_device (once per matrix, into one buffer)
 *         -> toyni_transcript_absorb_fields_device -> toyni_transcript_squeeze_device (4 words per DEEP term)
 *         -> toyni_deep_combine_ext_dz_device (once per matrix) -> toyni_merkle_commit_rows_device -> toyni_transcript_absorb_device
 *         -> a commit phase of 3l or 3m -> toyni_transcript_squeeze_indices_device -> toyni_fri_query_positions_device,
 *            toyni_query_rows_device -> the openers
 *     only enqueues.  Conventions of 3h and 3l: asynchronous on `stream`, packed-u32 words, the sticky `status` of toyni_transcript, no
 *     callback, no host read, no environment variable; on a warm context each call is a linear chain of kernels and can be captured
 *     into a HIP graph (caveat of section 4; the one exception is named at toyni_deep_combine_ext_dz_device).  Host arrays (`mults`,
 *     `slots`, `offsets`) may be reused as soon as the call returns.  Every field word read from device memory (z, a weight, a claimed
 *     value, an absorbed word) is reduced mod p by the one-wave kernel that first touches it, as BabyBear::new does: the result is that
 *     of the host-argument call on the reduced values.  Refusals happen on the host before anything is enqueued, the outputs untouched.
 * ---------------------------------------------------------------------------------------------- */
/* The protocol's out-of-domain point: four challenges (toyni_transcript_squeeze_device, count 4), squeezed again while
 * z1 = z2 = z3 = 0 (a z in the base field could lie on the evaluation domain); d_z receives the four words of the accepted z.  One
 * launch of one wave.  At most 8 tries: after the eighth rejection (probability p^-24) d_z is zeros, the state stays as it was and
 * status = TOYNI_E_RANGE.  A transcript whose status is set writes zeros.  TOYNI_E_NULL for a null pointer; TOYNI_E_RANGE for a d_tr that
 * is not 16-byte or a d_z that is not 4-byte aligned. */
int toyni_transcript_squeeze_ext_point_device(toyni_transcript* d_tr, uint32_t* d_z, void* stream);
/* absorb_field (src/transcript.rs) for `count` words of device memory: per word the 8 little-endian bytes of its canonical residue;
 * byte for byte toyni_transcript_absorb_device of the expanded bytes.  count <= 126 (126 x 8 = TOYNI_TRANSCRIPT_CAPACITY), otherwise
 * TOYNI_E_RANGE; count == 0 enqueues nothing; an overflow the host cannot see sets the status by 3l's rule.  TOYNI_E_NULL for a null
 * d_tr, or a null d_words with count > 0. */
int toyni_transcript_absorb_fields_device(toyni_transcript* d_tr, const uint32_t* d_words, size_t count, void* stream);
/* toyni_poly_eval_ext_batch_device at the points mults[p] * z: z is four words of device memory, mults a host array of npoints
 * canonical base-field multipliers (1, and the trace generator g for a column that is also opened at g z).  Three launches: a
 * one-wave kernel expands the points into a record behind the partial sums in the context's per-stream buffer (per point 20
 * dependent Ext squarings), then the two stages of 3h read the record.  The output bytes are those of the host-point call.  Refusals
 * are those of the host-point call, with "a point >= p" read as "a multiplier >= p", and a null or misaligned d_z. */
int toyni_poly_eval_ext_batch_dz_device(toyni_ntt_ctx* ctx, const uint32_t* d_coeffs, size_t ncoeffs, size_t stride, size_t batch,
                                        const uint32_t* d_z, const uint32_t* mults, unsigned npoints, uint32_t* d_out, void* stream);
/* Term t of toyni_deep_combine_ext_dz_device: (column, rotation) as in toyni_deep_ext_term; its weight is the Ext element
 * d_alphas[4 alpha_index ..], its claimed value d_claims[4 value_index ..]. */
typedef struct { uint32_t column, rotation, alpha_index, value_index; } toyni_deep_ext_slot;
/* toyni_deep_combine_ext_device with z, the weights and the claimed values in device memory; the per-matrix calls of a proof share
 * one array of weights and one buffer of out-of-domain values as they lie.  A one-wave kernel writes the Montgomery forms of the
 * weights into the term table, C = sum_t alpha_t value_t and the expansion of z (the conjugates' cubic and the norm) into a record in
 * the per-stream buffer; the combine kernel reads both.  The (column, rotation) sort does not depend on z and stays on the host.
 * The output bytes are those of toyni_deep_combine_ext_device on the same values, the x_i = z rule, accumulate and both load widths
 * included; nslots == 0 behaves as nterms == 0 there.  Up to 64 slots travel in the kernel arguments and the call can be captured; a
 * longer table goes through the pinned staging ring as in 3h and cannot.  Refusals: those of toyni_deep_combine_ext_device that do not
 * concern a host value; TOYNI_E_RANGE for an alpha_index or value_index >= 2^20 or a misaligned d_z, d_alphas or d_claims;
 * TOYNI_E_NULL for a null d_z, d_alphas or d_claims.  Staying inside the two arrays is the caller's contract, as with the indices
 * of 3d. */
int toyni_deep_combine_ext_dz_device(toyni_ntt_ctx* ctx, const uint32_t* d_values, size_t width, size_t col_stride, unsigned log_blowup,
                                     uint32_t shift, const uint32_t* d_z, const uint32_t* d_alphas, const uint32_t* d_claims,
                                     const toyni_deep_ext_slot* slots, size_t nslots, int accumulate, uint32_t* d_out, void* stream);
/* d_out[q * noffsets + r] = (d_indices[q] + offsets[r]) mod n, the sum in 64 bits: the rows a matrix with next-row terms opens per
 * query -- (i, (i + B) mod N) -- in wire order, from device-resident query indices; the list feeds toyni_merkle_open_rows_device as
 * it lies.  offsets: host array, 1 <= noffsets <= 8, every offset < n; 1 <= n <= 2^32; count <= 65536 (count == 0 enqueues nothing).
 * Outside that: TOYNI_E_RANGE; a null pointer: TOYNI_E_NULL. */
int toyni_query_rows_device(const uint32_t* d_indices, size_t count, size_t n, const uint32_t* offsets, unsigned noffsets,
                            uint32_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3p. The first half of a staged-AIR proof without the host: gamma and the constraint weights read from DEVICE memory.  3o carries a
 *     proof from "quotient root absorbed" onward; before that the host-argument calls take gamma as toyni_ext_operand.shift (3i), as
 *     CONST immediates of the constraint program (3f: a program per proof, and toyni_air_program_create blocks) and the weights as a
 *     host array (3k), which costs a caller of 3l three downloads and synchronisations.  With the calls below the sequence
 *         toyni_transcript_absorb_device (main root) -> toyni_transcript_squeeze_device (4 words: gamma)
 *         -> toyni_column_scan_ext_dc_device -> ... commit, absorb -> toyni_transcript_squeeze_device (the alphas)
 *         -> toyni_air_quotient_ext_dc_device -> ... commit, absorb -> 3o
 *     only enqueues, and the constraint program is created once per AIR.  Conventions of 3o: asynchronous on `stream`, packed-u32
 *     words, host arrays reusable on return, refusals on the host before anything is enqueued with the outputs untouched; every field
 *     word read from device memory is reduced mod p by the one-wave kernel that first touches it, and the bytes written are those of
 *     the host-argument call on the reduced values.  No existing entry point, record layout or written byte changes.
 * ---------------------------------------------------------------------------------------------- */
/* One more instruction for constraint programs: a value that is not known when the program is created. */
#define TOYNI_AIR_PARAM 8          /* r[dst] = params[imm], imm < TOYNI_AIR_MAX_PARAMS; a and b unused */
#define TOYNI_AIR_MAX_PARAMS 256
/* toyni_air_program_check / _create with TOYNI_AIR_PARAM accepted (it writes dst as CONST does; TOYNI_E_RANGE for imm >= 256); every
 * other rule is theirs.  toyni_air_info stays as it is: *nparams = highest parameter index + 1, or 0.  The calls of 3f keep refusing
 * op 8.  A program created here WITHOUT a PARAM is accepted by every quotient call; one WITH a PARAM is refused with TOYNI_E_RANGE by
 * toyni_air_quotient_device and toyni_air_quotient_ext_device, which have no parameter array.  TOYNI_E_NULL for a null argument. */
int toyni_air_program_check_params(const toyni_air_insn* insns, size_t ninsns, toyni_air_info* info, uint32_t* nparams);
int toyni_air_program_create_params(toyni_ntt_ctx* ctx, const toyni_air_insn* insns, size_t ninsns, toyni_air_program** out);
int toyni_air_program_nparams(const toyni_air_program* prog, uint32_t* nparams);   /* 0 for a program of toyni_air_program_create */
/* toyni_air_quotient_ext_device (3k) with the parameters and the weights in device memory.  d_params: nparams words; d_alphas:
 * nalphas Ext elements (4 words each); the weights follow from the alphas by weights_form: */
#define TOYNI_AIR_WEIGHTS_EXT 0        /* W_k = the Ext element d_alphas[4 k ..],            nweights = nalphas   */
#define TOYNI_AIR_WEIGHTS_EMIT_EXT 1   /* W_{4 k + j} = alpha_k * X^j (emit_ext constraints), nweights = 4 nalphas */
/* Two launches, a linear chain for any nweights (no staging ring: the call can always be captured, caveat of section 4): a one-wave
 * kernel writes a record into the context's per-stream buffer -- the parameters, reduced and in Montgomery form, then the 4 x nweights
 * plain canonical weight words (alpha * X = (11 a3, a0, a1, a2)); its lanes stride over the parameters and the alphas.  A twin of 3k's
 * kernel takes the record as a read-only argument and fetches its words by scalar loads where they are used: PARAM is one such load.
 * By definition the output is byte for byte what toyni_air_quotient_ext_device writes for the program with every PARAM j replaced by
 * CONST (params[j] mod p) under the weights of the reduced alphas -- accumulate, a null d_c_out, both store widths, every launch shape
 * and every source of 1 / Z_H of 3f included.
 * Refused: what 3k refuses that does not concern a host value; TOYNI_E_NULL for a null d_alphas, or a null d_params with nparams > 0;
 * TOYNI_E_RANGE for nparams < the program's nparams or > TOYNI_AIR_MAX_PARAMS, nweights < nconstraints or > 65536, an unknown form, a
 * d_params or d_alphas that is not 4-byte aligned. */
int toyni_air_quotient_ext_dc_device(toyni_ntt_ctx* ctx, const toyni_air_program* prog, const toyni_air_matrix* mats, size_t nmats,
                                     unsigned log_blowup, uint32_t shift, const uint32_t* d_params, size_t nparams,
                                     const uint32_t* d_alphas, size_t nalphas, int weights_form,
                                     uint32_t* d_c_out, uint32_t* d_q_out, size_t out_stride, int accumulate, void* stream);
/* toyni_column_scan_ext_device (3i) with the operands' shifts in device memory: an operand's shift is the Ext element
 * d_challenges[4 * shift_index ..], reduced; TOYNI_EXT_SHIFT_NONE means 0; shift_index < 2^20 otherwise (staying inside the array is
 * the caller's contract).  init stays a host array: a protocol constant, not a challenge.  A one-wave kernel writes
 * {num shift, den shift, adj_z / m_z of z = -(den shift)} into the per-stream buffer behind the tile words of the same call, 16-byte
 * aligned; twins of the two 3i kernels that read an operand take that record, the prefix kernel is launched as it is; with batch > 16
 * the one record serves every launch sequence.  Launch structure, exactness, the in-place rule, load widths and the d_totals layout are
 * those of 3i, and the output is byte for byte toyni_column_scan_ext_device with the reduced shifts.
 * Refused: what 3i refuses, without "a shift coordinate >= p"; TOYNI_E_NULL for a null d_challenges when some operand names an index;
 * TOYNI_E_RANGE for a d_challenges that is not 4-byte aligned or an index >= 2^20. */
#define TOYNI_EXT_SHIFT_NONE 0xffffffffu
typedef struct { const uint32_t* d_values; size_t stride; uint32_t width; uint32_t shift_index; } toyni_ext_operand_dc;
int toyni_column_scan_ext_dc_device(toyni_ntt_ctx* ctx, const toyni_ext_operand_dc* num, const toyni_ext_operand_dc* den,
                                    const uint32_t* d_challenges, uint32_t* d_out, size_t out_stride, size_t n, size_t batch, int op,
                                    const uint32_t* init, uint32_t* d_totals, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3q. The base-field first half of a Fibonacci proof (the reference's own protocol, src/fibonacci.rs:99-310) without the host: the
 *     mask, derive_z, the out-of-domain values, the constraint check at z and the DEEP layer of 3c with z and the claimed values read
 *     from DEVICE memory.  Together with 3l and 3o the sequence
 *         upload, INTT -> toyni_mask_poly_device -> LDE, trees, quotient (3c) -> toyni_transcript_absorb_device (both roots)
 *         -> toyni_transcript_squeeze_point_device -> toyni_poly_eval_dz_device (T at z, g z, g^2 z; Q at z, into one buffer)
 *         -> toyni_transcript_absorb_fields_device -> toyni_fib_deep_dz_device -> toyni_merkle_commit_device, absorb
 *         -> toyni_fri_commit_phase_transcript_device -> toyni_transcript_squeeze_indices_device
 *         -> toyni_fri_query_positions_device, toyni_query_rows_device -> toyni_merkle_open_groups_device
 *         -> toyni_fri_phase_roots_device -> one download
 *     only enqueues (csrc/host/fib_prover_dt.hpp is that caller).  Conventions of 3o / 3p: asynchronous on `stream`, packed-u32 words,
 *     no environment variable, no callback, no host read; refusals on the host before anything is enqueued, the outputs untouched;
 *     every field word read from device memory is reduced mod p by the one-wave kernel that first touches it, and the result is that
 *     of the host-argument call on the reduced values; the transcript's `status` is sticky (3l); on a warm context each call is a
 *     linear chain of kernels and can be captured into a HIP graph (caveat of section 4).  No existing entry point, record layout or
 *     written byte changes.
 * ---------------------------------------------------------------------------------------------- */
/* T_hat = T - R + x^n R in place on d_coeffs[0 .. n + mask_degree): R_i = (the little-endian u64 of keystream words 2 i, 2 i + 1) mod p
 * of the ChaCha20 stream of toyni_chacha20_fill_device under key / nonce (block i / 8), i < mask_degree.  One launch, one thread per
 * OUTPUT word: R_j is subtracted where j < mask_degree and R_(j - n) added where n <= j < n + mask_degree, so the overlapping case
 * n < mask_degree has no two threads on one word.  Words outside the two ranges are not touched; the touched ones are reduced.
 * TOYNI_E_NULL for a null d_coeffs or key; TOYNI_E_RANGE for mask_degree == 0, mask_degree > 4096, n == 0 or a d_coeffs that is not
 * 4-byte aligned. */
int toyni_mask_poly_device(uint32_t* d_coeffs, size_t n, unsigned mask_degree, const uint8_t key[32], uint64_t nonce, void* stream);
/* derive_z_from_transcript (src/fibonacci.rs:379-399): one challenge, squeezed again while z^N == 1 or (z / shift)^N == 1, N = 2^log_N
 * (z on the trace domain's extension or on the LDE coset); d_z receives the one word.  One launch of one wave, log_N squarings per
 * test.  At most 8 tries: after the eighth rejection d_z is zero, the state stays as it was and status = TOYNI_E_RANGE.  A transcript
 * whose status is set writes zero.  TOYNI_E_NULL for a null pointer; TOYNI_E_RANGE for log_N > 27, shift == 0, shift >= p, a d_tr that
 * is not 16-byte or a d_z that is not 4-byte aligned. */
int toyni_transcript_squeeze_point_device(toyni_transcript* d_tr, unsigned log_N, uint32_t shift, uint32_t* d_z, void* stream);
/* toyni_poly_eval_device at the points mults[p] * z: z is one word of device memory, mults a host array of npoints canonical
 * multipliers (1, g, g^2).  Three launches: a one-wave kernel writes z, z^16 and z^4096 of every point (Montgomery forms) into a
 * record behind the partial sums in the context's per-stream buffer, then twins of the two stages read the record.  The output bytes
 * are those of the host-point call; ncoeffs == 0 writes zeros.  Refusals are those of the host-point call, with "a point >= p" read
 * as "a multiplier >= p", a null d_z (TOYNI_E_NULL) and a d_coeffs, d_z or d_out that is not 4-byte aligned (TOYNI_E_RANGE). */
int toyni_poly_eval_dz_device(toyni_ntt_ctx* ctx, const uint32_t* d_coeffs, size_t ncoeffs, const uint32_t* d_z, const uint32_t* mults,
                              unsigned npoints, uint32_t* d_out, void* stream);
/* toyni_fib_deep_device with z (d_z, one word) and the claimed values (d_ood = {t_z, t_gz, t_ggz, q_z}) in device memory.  Two
 * launches: a one-wave kernel writes the record the layer kernel's twin reads.  If d_check is not NULL that kernel also evaluates the
 * prover's own check (src/fibonacci.rs:173-177) with n = trace_len (a power of two <= 2^27) and g the root of unity of order n:
 *     d_check[0] = 1 if (t_ggz - t_gz - t_z)(z - g^(n-1))(z - g^(n-2)) == q_z (z^n - 1), else 0.
 * The output bytes are those of toyni_fib_deep_device on the reduced values, the x_i = z rule and the N < 8 path included.
 * Refusals: those of toyni_fib_deep_device that do not concern a host value; TOYNI_E_NULL for a null d_z or d_ood; TOYNI_E_RANGE for
 * a trace_len that is not a power of two or exceeds 2^27, or a d_z, d_ood or d_check that is not 4-byte aligned. */
int toyni_fib_deep_dz_device(toyni_ntt_ctx* ctx, const uint32_t* d_trace_lde, const uint32_t* d_q_evals, uint32_t* d_out, unsigned log_blowup,
                             uint32_t shift, const uint32_t* d_z, const uint32_t* d_ood, uint32_t trace_len, uint32_t* d_check, void* stream);
/* The roots of the trees a commit phase of 3l / 3m left back to back in d_levels: tree k = 0 .. rounds - 1 has m_first >> k leaves
 * (for toyni_fri_commit_phase_transcript_device m_first = m0 / 2); its root goes to d_roots[32 k ..].  One launch.  rounds == 0 enqueues
 * nothing.  TOYNI_E_NULL for a null pointer; TOYNI_E_INVALID_SIZE for an m_first that is not a power of two or exceeds 2^32;
 * TOYNI_E_RANGE for rounds > 64, m_first >> (rounds - 1) == 0, a d_levels that is not 16-byte or a d_roots that is not 4-byte aligned. */
int toyni_fri_phase_roots_device(const uint8_t* d_levels, size_t m_first, unsigned rounds, uint8_t* d_roots, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3r. A BATCH dimension for the latency-bound tail of a proof: from "the DEEP codewords of `batch` proofs lie on the device" to "every
 *     proof's query positions are known", and the tree-building call that also serves the trace, quotient and DEEP commitments of
 *     `batch` proofs.  The chains of 3l are launch-bound -- a 2^12-element layer's largest launch hashes 2048 leaves on a chip of
 *     65 536 lanes -- and proofs in flight on several streams do not overlap; here every launch of the chain works on
 *     `batch` independent proofs instead: the same number of launches, the proof index a block coordinate of each.
 *     THE SPECIFICATION: every call writes, for proof b < batch, exactly the bytes the single call of 3a / 3l writes when given proof
 *     b's pointers.  The single calls are the reference; batch == 1 enqueues a chain that writes what the single call writes.
 *     ADDRESSING: proof b's part of an array starts b * stride behind the base pointer.  Strides are size_t, in elements of the
 *     pointed-to type (u32 words for uint32_t*, bytes for uint8_t*); a stride may exceed the proof's extent (guard bands between the
 *     proofs stay untouched); all offset arithmetic is 64-bit.  The transcripts are an array toyni_transcript d_tr[batch], 1 KiB apart.
 *     `status` is sticky PER PROOF: a transcript whose status is set behaves as in 3l and its neighbours do not notice.
 *     x0, m0, final_size and the context are shared: all proofs of a batch live on the same domain.
 *     Conventions of 3l / 3o / 3q: asynchronous on `stream`, packed-u32 words, no callback, no host read, no new environment variable;
 *     each call is a linear chain of kernels and can be captured into a HIP graph (caveat of section 4; the phases need a context
 *     warmed by one call on this stream with at least this batch and these sizes: the per-stream record buffer grows to `batch`
 *     records per round).  TOYNI_FRI_TAIL_LOG and TOYNI_MERKLE_COOP_LOG keep their meaning and every setting writes the same bytes; a
 *     tree level takes the two-wave node hash when batch x nodes <= 2^TOYNI_MERKLE_COOP_LOG, since that product is what fills the chip.
 *     REFUSALS, on the host before anything is enqueued, the outputs untouched, in this order: TOYNI_E_NULL for a null pointer (the
 *     pointers the single call allows to be null may be null); TOYNI_E_RANGE for batch == 0 or batch > 65535; then the single call's
 *     refusals, with its codes and in its order; then TOYNI_E_RANGE for a stride smaller than the proof's extent or one that breaks
 *     the single call's alignment rule for that pointer (a multiple of 16 bytes where the single call wants 16-byte alignment).  The
 *     stride of a pointer that is null is not looked at.  What the single call accepts as "nothing to do" enqueues nothing here.
 *     No existing entry point, kernel symbol, record layout or written byte changes.
 *     OUT OF SCOPE: the four-to-one phase of 3m, grinding (3n), and the first half of a proof (mask, quotient, out-of-domain values,
 *     DEEP) -- so there is no batched prover yet, and no caller inside this library is switched to these calls.
 * ---------------------------------------------------------------------------------------------- */
/* `batch` trees of toyni_merkle_commit_device over n leaves each (any n >= 1; n == 0 writes nothing).  Extents: value_stride >= n words;
 * salt_stride >= 16 n bytes and a multiple of 16 (d_salts may be NULL: unsalted); level_stride in BYTES, a multiple of 16 and at least
 * toyni_merkle_total_digests(n) * 32. */
int toyni_merkle_commit_batch_device(const uint32_t* d_values, size_t value_stride, const uint8_t* d_salts, size_t salt_stride, size_t n,
                                     size_t batch, uint8_t* d_levels, size_t level_stride, void* stream);
/* Transcript b absorbs the `len` bytes at d_bytes + b * byte_stride (byte_stride >= len): one launch, one wave per transcript.  For the
 * roots of trees built by the call above, d_bytes = the root of tree 0 and byte_stride = level_stride. */
int toyni_transcript_absorb_batch_device(toyni_transcript* d_tr, size_t batch, const uint8_t* d_bytes, size_t byte_stride, size_t len,
                                         void* stream);
/* The commit phases of 3l for `batch` proofs: the arguments of the single calls, `batch` behind d_tr and a stride behind each of
 * d_layer0, d_salts, d_layers, d_levels and d_betas.  Extents (W = 1, or 4 for the Ext call; rounds = log2(m0 / final_size)):
 *   layer0_stride >= W m0 words; layers_stride >= W (m0 - final_size) words; both multiples of 4 for the Ext call
 *   salt_stride   >= 16 (m0 - 2 final_size) bytes, a multiple of 16 (d_salts not NULL)
 *   level_stride  >= 32 x the digests of all trees of a proof, in bytes, a multiple of 16
 *   beta_stride   >= W rounds words (d_betas not NULL)
 * beta of proof b reaches its fold through record b of the round's `batch` records in the per-stream buffer. */
int toyni_fri_commit_phase_transcript_batch_device(toyni_ntt_ctx* ctx, const uint32_t* d_layer0, size_t layer0_stride, size_t m0, uint32_t x0,
                                                   size_t final_size, const uint8_t* d_salts, size_t salt_stride, toyni_transcript* d_tr,
                                                   size_t batch, uint32_t* d_layers, size_t layers_stride, uint8_t* d_levels, size_t level_stride,
                                                   uint32_t* d_betas, size_t beta_stride, void* stream);
int toyni_fri_commit_phase_transcript_ext_batch_device(toyni_ntt_ctx* ctx, const uint32_t* d_layer0, size_t layer0_stride, size_t m0, uint32_t x0,
                                                       size_t final_size, const uint8_t* d_salts, size_t salt_stride, toyni_transcript* d_tr,
                                                       size_t batch, uint32_t* d_layers, size_t layers_stride, uint8_t* d_levels,
                                                       size_t level_stride, uint32_t* d_betas, size_t beta_stride, void* stream);
/* toyni_transcript_squeeze_indices_device on every transcript: proof b's `count` indices at d_out + b * out_stride (out_stride >= count). */
int toyni_transcript_squeeze_indices_batch_device(toyni_transcript* d_tr, size_t batch, size_t count, uint32_t max, uint32_t* d_out,
                                                  size_t out_stride, void* stream);
/* toyni_fri_query_positions_device for every proof: index_stride >= count, out_stride >= rounds x 2 count words.  The openings need
 * nothing new: toyni_merkle_open_groups_device takes the groups of any number of trees in one launch. */
int toyni_fri_query_positions_batch_device(const uint32_t* d_indices, size_t index_stride, size_t count, size_t m0, size_t final_size,
                                           size_t batch, uint32_t* d_out, size_t out_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3s. The BATCH dimension for the first half of a Fibonacci proof: batch forms of every call of the chain of 3q that 3r left single
 *     (salts, mask, quotient, derive_z, the out-of-domain values, absorb_field, the DEEP layer, the query rows, the round roots), and a
 *     strided copy.  With 3r and the transforms' own `batch` argument, `batch` proofs of one trace length are one chain of as many
 *     launches as one proof (csrc/host/fib_prover_batch.hpp is that caller).
 *     THE SPECIFICATION is 3r's: every call writes, for proof b < batch, exactly the bytes the single call writes when given proof b's
 *     pointers.  ADDRESSING, the transcript array, the sticky per-proof `status`, the conventions (asynchronous on `stream`, no callback,
 *     no host read, no new environment variable) and the ORDER OF THE REFUSALS (null pointers; batch == 0 or > 65535: TOYNI_E_RANGE; the
 *     single call's own, with its codes and in its order; strides below the extent or against the single call's alignment rule:
 *     TOYNI_E_RANGE) are 3r's.  The context, shift, log_blowup, n, mults and offsets are shared by the batch.  What the single call
 *     accepts as "nothing to do" enqueues nothing.
 *     KEYS: a proof's ChaCha key is read from DEVICE memory -- d_keys is batch x 32 bytes, contiguous, 4-byte aligned (otherwise
 *     TOYNI_E_RANGE, judged with the strides), the key of proof b at d_keys + 32 b: a kernel-argument block cannot hold 65 535 keys.
 *     RECORDS: toyni_poly_eval_dz_batch_device keeps batch x nblocks x npoints partial sums and then `batch` records in the context's
 *     per-stream buffer, toyni_fib_deep_dz_batch_device `batch` records; with batch == 1 both layouts are the single call's.  On a
 *     context warmed by one call on this stream with at least this batch and these sizes each call is a linear chain of kernels and
 *     can be captured into a HIP graph (caveat of section 4).
 *     No existing entry point, kernel symbol, record layout or written byte changes.  The section is implemented in a translation unit
 *     of its own, csrc/batch/toyni_hip_fib_batch.hip, linked into the same library (a static archive of toyni_hip.hip alone, INTEGRATION.md 1,
 *     does not contain these ten calls).
 *     WHAT REMAINS single: the four-to-one phase of 3m, grinding (3n) and the staged-AIR chain of 3o / 3p.
 * ---------------------------------------------------------------------------------------------- */
/* toyni_chacha20_fill_device per proof: out_stride in BYTES, >= bytes and a multiple of 16. */
int toyni_chacha20_fill_batch_device(void* d_out, size_t out_stride, size_t bytes, const uint8_t* d_keys, uint64_t nonce, size_t batch, void* stream);
/* toyni_mask_poly_device per proof: coeff_stride >= n + mask_degree words. */
int toyni_mask_poly_batch_device(uint32_t* d_coeffs, size_t coeff_stride, size_t n, unsigned mask_degree, const uint8_t* d_keys, uint64_t nonce,
                                 size_t batch, void* stream);
/* toyni_fib_quotient_device per proof (d_c_evals may be NULL; its stride is then not looked at): every stride >= N words.  A proof
 * whose three pointers are 16-byte aligned takes the 16-byte accesses, any other the single words; the bytes are the same. */
int toyni_fib_quotient_batch_device(toyni_ntt_ctx* ctx, const uint32_t* d_trace_lde, size_t trace_stride, uint32_t* d_c_evals, size_t c_stride,
                                    uint32_t* d_q_evals, size_t q_stride, unsigned log_blowup, uint32_t shift, size_t batch, void* stream);
/* toyni_transcript_squeeze_point_device on every transcript: proof b's z at d_z + b * z_stride (z_stride >= 1).  One wave per proof. */
int toyni_transcript_squeeze_point_batch_device(toyni_transcript* d_tr, size_t batch, unsigned log_N, uint32_t shift, uint32_t* d_z, size_t z_stride,
                                                void* stream);
/* toyni_poly_eval_dz_device per proof: coeff_stride >= ncoeffs, z_stride >= 1, out_stride >= npoints.  Three launches; ncoeffs == 0
 * writes zeros (two launches). */
int toyni_poly_eval_dz_batch_device(toyni_ntt_ctx* ctx, const uint32_t* d_coeffs, size_t coeff_stride, size_t ncoeffs, const uint32_t* d_z,
                                    size_t z_stride, const uint32_t* mults, unsigned npoints, size_t batch, uint32_t* d_out, size_t out_stride,
                                    void* stream);
/* toyni_transcript_absorb_fields_device on every transcript: proof b's `count` words at d_words + b * word_stride (word_stride >= count). */
int toyni_transcript_absorb_fields_batch_device(toyni_transcript* d_tr, size_t batch, const uint32_t* d_words, size_t word_stride, size_t count,
                                                void* stream);
/* toyni_fib_deep_dz_device per proof (d_check may be NULL; its stride is then not looked at): trace_stride, q_stride and out_stride
 * >= N words, ood_stride >= 4, z_stride and check_stride >= 1.  Two launches. */
int toyni_fib_deep_dz_batch_device(toyni_ntt_ctx* ctx, const uint32_t* d_trace_lde, size_t trace_stride, const uint32_t* d_q_evals, size_t q_stride,
                                   uint32_t* d_out, size_t out_stride, unsigned log_blowup, uint32_t shift, const uint32_t* d_z, size_t z_stride,
                                   const uint32_t* d_ood, size_t ood_stride, uint32_t trace_len, uint32_t* d_check, size_t check_stride, size_t batch,
                                   void* stream);
/* toyni_query_rows_device per proof: index_stride >= count, out_stride >= count x noffsets. */
int toyni_query_rows_batch_device(const uint32_t* d_indices, size_t index_stride, size_t count, size_t n, const uint32_t* offsets, unsigned noffsets,
                                  size_t batch, uint32_t* d_out, size_t out_stride, void* stream);
/* toyni_fri_phase_roots_device per proof: level_stride in BYTES, a multiple of 16 and at least the trees' extent (32 bytes x the sum of
 * 2 (m_first >> k) - 1 over the rounds); root_stride in bytes, >= 32 x rounds and a multiple of 4.  One launch, one block per proof. */
int toyni_fri_phase_roots_batch_device(const uint8_t* d_levels, size_t level_stride, size_t m_first, unsigned rounds, size_t batch, uint8_t* d_roots,
                                       size_t root_stride, void* stream);
/* `rows` stream-ordered copies in ONE launch: row r copies row_bytes bytes from d_src + r * src_stride to d_dst + r * dst_stride (strides in
 * bytes) -- what `rows` calls of toyni_memcpy_d2d_async would write.  It gathers roots that lie level_stride apart, copies final layers,
 * and spreads n-word rows into wider coefficient slots.  16-byte accesses where both pointers and both strides are multiples of 16, words
 * otherwise.  Overlapping ranges are the caller's contract.  rows == 0 or row_bytes == 0 enqueues nothing.  TOYNI_E_NULL for a null
 * pointer; TOYNI_E_RANGE for rows > 65535, a pointer, stride or row_bytes that is no multiple of 4, or a stride below row_bytes. */
int toyni_copy_rows_device(void* d_dst, size_t dst_stride, const void* d_src, size_t src_stride, size_t row_bytes, size_t rows, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3t. VERIFYING a batch of Fibonacci proofs of one trace length on the device: what StarkVerifier::verify does (src/verifier.rs:14-232),
 *     one verdict word per proof, in FIVE launches whatever the batch, with no host in the loop: the caller uploads the images once,
 *     downloads 4 x batch bytes once and synchronises once.  The chain is linear and can be captured into a HIP graph.
 *     THE PROOF IMAGE.  A proof of trace length n is a fixed-size byte image; N = 32 n, C = next_pow2(n + 140), F = log2 C folds,
 *     final_size = N / C <= 16, Q = 44.  In order:
 *       roots            trace root, quotient root, fri_commitments[0 .. F]: (F + 3) x 32 bytes
 *       OOD values       t_z, t_gz, t_ggz, q_z: 4 words
 *       claimed indices  QueryProof::index of the Q queries: Q words
 *       final layer      fri_final_layer: final_size words; then zero padding to a multiple of 8 bytes
 *       opening records  back to back, each the record of toyni_merkle_open_device (3c), in the provers' order: 3 Q over the trace tree
 *                        (N leaves; rows qi, qi + 32, qi + 64 mod N per query), Q over the quotient tree (N), 2 Q over layer 0 = the DEEP
 *                        tree (N; qi and qi + N / 2), 2 Q over the tree of N >> k leaves for every layer k = 1 .. F - 1
 *     -- the records are Proof::opening_records of csrc/host/fib_prover.hpp as they lie.  image_bytes is rounded up to a multiple of 16;
 *     images lie image_stride bytes apart (a multiple of 16, >= image_bytes).  The image carries NO opening indices, no z and no transcript
 *     state: the verifier derives them.  The reference's structural refusals (lde_size, fold_count, final_size, query_count,
 *     fri_opening_count) cannot occur in an image of the right size; the packers (toyni_amd/verifier.py, csrc/host/fib_verifier.hpp)
 *     refuse them on the host under those names.
 *     THE VERDICT WORD.  0 = accept; otherwise (q + 1) << 8 | code, q the query (q + 1 = 0 for the checks made once per proof) and the
 *     codes in the order in which the reference visits its checks, so that the word names exactly the check at which src/verifier.rs
 *     returns false.  It is a function of the image alone, never of the grid or the schedule (no atomics: every query leaves the key of
 *     its first failing check in the work buffer and the last kernel takes the minimum).  A proof that fails, fails alone.
 *     STRICTER THAN THE REFERENCE in one point: a record counts only if its `depth` position bytes spell the index the VERIFIER derived
 *     (byte l = bit l of the index, 1 = the sibling is the left input).  The reference trusts the prover's position flags for the FRI
 *     openings (src/verifier.rs:176-205) and compares indices only for the trace rows.  An honest prover's records pass both.  Also: a
 *     value word >= p or a non-zero upper value word -- nothing a BabyBear can hold -- is TOYNI_FIB_MALFORMED, and fails its record.
 *     The section is a translation unit of its own, csrc/verify/toyni_hip_verify.hip, linked into the same library.
 *     OUT OF SCOPE: verifying a batch prover's buffers where they lie, the Ext / staged-AIR proofs, four-to-one layers, grinding.
 * ---------------------------------------------------------------------------------------------- */
#define TOYNI_FIB_ACCEPT 0
#define TOYNI_FIB_MALFORMED 1             /* a field word of the image is not canonical ("malformed") */
#define TOYNI_FIB_OOD 2                   /* C(z) != Q(z) Z(z) ("ood") */
#define TOYNI_FIB_FINAL_NOT_CONSTANT 3    /* "final_not_constant" */
#define TOYNI_FIB_FINAL_COMMITMENT 4      /* the tree over the final layer does not have the last commitment as its root ("final_commitment") */
#define TOYNI_FIB_QUERY_INDEX 5           /* a claimed index differs from the derived one ("query_index") */
#define TOYNI_FIB_TRACE_MERKLE 6          /* "trace_merkle" */
#define TOYNI_FIB_QUOTIENT_MERKLE 7       /* "quotient_merkle" */
#define TOYNI_FIB_DEEP_MERKLE 8           /* "deep_merkle" */
#define TOYNI_FIB_DEEP_VALUE 9            /* "deep_value" */
#define TOYNI_FIB_FRI_MERKLE(k) (16 + 2 * ((k) - 1))        /* layer k = 1 .. F - 1 ("fri_merkle") */
#define TOYNI_FIB_FRI_CONSISTENCY(k) (17 + 2 * ((k) - 1))   /* "fri_consistency" */
#define TOYNI_FIB_FINAL_VALUE 255         /* the fold chain does not land on fri_final_layer[pos] ("final_value") */
#define TOYNI_FIB_MAX_GROUPS 32
typedef struct {
    size_t trace_len, lde_size, folds, final_size, queries;
    size_t roots_offset, nroots;                       /* byte offsets into an image from here on */
    size_t ood_offset, indices_offset, final_offset, records_offset;
    size_t ngroups;                                    /* folds + 2: trace, quotient, layer 0 (DEEP), layers 1 .. folds - 1 */
    size_t group_offset[TOYNI_FIB_MAX_GROUPS];         /* first record of the group */
    size_t group_leaves[TOYNI_FIB_MAX_GROUPS];
    size_t group_records[TOYNI_FIB_MAX_GROUPS];
    size_t group_record_bytes[TOYNI_FIB_MAX_GROUPS];   /* toyni_merkle_open_record_bytes(group_leaves) */
    size_t nrecords, image_bytes;
} toyni_fib_proof_layout;
/* Host only.  TOYNI_E_NULL; TOYNI_E_INVALID_SIZE unless trace_len is a power of two in [8, 2^22] (toyni_fib_proof_image_bytes: 0). */
int toyni_fib_proof_layout_of(size_t trace_len, toyni_fib_proof_layout* layout);
size_t toyni_fib_proof_image_bytes(size_t trace_len);
/* The name of the check a verdict word stands for, as tests/harness/fib_verifier.py puts it into `why` ("accept" for 0, "unknown"). */
const char* toyni_fib_verdict_string(uint32_t word);

/* The general call any AIR verifier needs: records of several trees of `batch` proofs checked in ONE launch (one per 32 groups with
 * records).  Record r of proof b of a group lies at d_records + b * record_stride + r * toyni_merkle_open_record_bytes(leaves), the
 * index it must open at d_indices[b * index_stride + r] (device data), its root at d_root + b * root_stride, and
 * d_flags[b * flag_stride + r] receives 1 if the record's leaf and path hash to the root AND its position bytes spell that index AND its
 * value is canonical, else 0 (byte l = bit l of the index -- or 1 where an odd level pairs its last node with itself, as MerkleTree::get_proof
 * writes it; leaves need not be a power of two).  Nothing read from a record or from d_indices is used as an address.  A group with nrecords == 0 is skipped.
 * TOYNI_E_NULL for a null pointer; TOYNI_E_RANGE for batch == 0 or > 65535, leaves == 0 or > 2^32, nrecords > 2^32 / 64, d_records or
 * record_stride no multiple of 8, another pointer no multiple of 4, root_stride no multiple of 4, or a stride below its extent
 * (nrecords records; nrecords words; 32 bytes).
 * The call takes no context: it launches on the CURRENT device, which the caller has made the device of these pointers (toyni_set_device);
 * the composite call below names its device through its context. */
typedef struct {
    const uint8_t* d_records;
    size_t record_stride;     /* bytes */
    size_t nrecords, leaves;
    int salted;               /* the leaf is SHA256(00 || salt || value) -- or SHA256(00 || value), the record's salt bytes ignored */
    const uint32_t* d_indices;
    size_t index_stride;      /* words */
    const uint8_t* d_root;
    size_t root_stride;       /* bytes */
    uint32_t* d_flags;
    size_t flag_stride;       /* words */
} toyni_merkle_verify_group;
int toyni_merkle_verify_records_batch_device(const toyni_merkle_verify_group* groups, size_t ngroups, size_t batch, void* stream);

/* Verifies the `batch` images at d_images + b * image_stride and writes d_verdicts[b].  ctx: a context of size N = 32 trace_len (it names
 * the device; nothing of it is written).  d_work: toyni_fib_verify_work_bytes(trace_len, batch) bytes, 16-byte aligned, scratch of the
 * call; nothing of its earlier contents is read.  Defined after the call, per proof: the transcript's length, status and its `len` state
 * bytes (initialised on the device to "toyni-stark-v1"), z, the key of the global checks, the F betas, the 44 derived indices, the keys of
 * the 44 queries, the expected index and the word of every record.  The rest -- two spare words, the unused betas, the state bytes beyond
 * `len`, the padding up to the proof's stride -- is never written.  Five launches:
 *   fib_verify_replay_kernel        one wave per proof (one lane active): absorb both roots, derive_z, absorb the four values and
 *                                   fri_commitments[0], squeeze beta_(k-1) and absorb root k for k = 1 .. F, squeeze_indices(44, N / 2)
 *   fib_verify_global_kernel        one wave per proof, 516 bytes of LDS (16 digests and one word): every field word canonical, C(z) =
 *                                   Q(z) Z(z), the final layer constant, its unsalted tree's root the last commitment; the positions
 *                                   every record must open, from the DERIVED indices
 *   merkle_verify_records_batch_kernel   the call above over all F + 2 groups, the proof index fastest
 *   fib_verify_query_kernel         one thread per (proof, query): claimed index, record words, the DEEP value rebuilt over
 *                                   (x_i - z)^-1, the fold chain with x = (7 w_N^lo)^(2^k) and one inversion per layer, the final value
 *   fib_verify_verdict_kernel       one wave per proof (one lane active): the minimum key
 * REFUSALS, before anything is enqueued and with the outputs untouched, in this order: TOYNI_E_NULL for a null pointer; TOYNI_E_RANGE for
 * batch == 0 or > 65535; TOYNI_E_INVALID_SIZE unless trace_len is a power of two in [8, 2^22]; TOYNI_E_RANGE unless the context's n is
 * 32 trace_len; TOYNI_E_RANGE for d_images or d_work not 16-byte aligned, d_verdicts not 4-byte aligned, image_stride below
 * toyni_fib_proof_image_bytes(trace_len) or no multiple of 16. */
size_t toyni_fib_verify_work_bytes(size_t trace_len, size_t batch);
int toyni_fib_verify_batch_device(toyni_ntt_ctx* ctx, const uint8_t* d_images, size_t image_stride, size_t trace_len, size_t batch, void* d_work,
                                  uint32_t* d_verdicts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 3c. One FRI round, and the pointwise steps of the Fibonacci prover on the LDE coset (oracle:
 *     src/fibonacci.rs:133-150,186-198,222-245, src/math/polynomial.rs:134-144, src/merkle.rs:50-80).  All asynchronous on
 *     `stream`; packed u32 device data; ctx = a context of size N = the LDE size (its domain table supplies x_i = shift w_N^i).
 * ---------------------------------------------------------------------------------------------- */
/* One round of the fold loop (src/fibonacci.rs:222-245): d_out = fri_fold(d_evals) on the points x0 w_m^i with challenge
 * beta, AND the Merkle tree of the folded layer in d_levels (layout of toyni_merkle_commit_device over m/2 leaves; the leaf
 * hashes are computed in the fold's own sweep; d_salts = (m/2) x 16 bytes, or NULL for the unsalted final layer).  The next
 * beta depends on this tree's root (the last 32 bytes of d_levels), so a round is as far as the protocol lets the fusion go. */
int toyni_fri_fold_commit_device(toyni_ntt_ctx* ctx, const uint32_t* d_evals, uint32_t* d_out, size_t m, uint32_t beta, uint32_t x0,
                                 const uint8_t* d_salts, uint8_t* d_levels, void* stream);
/* The WHOLE fold loop of the commit phase (src/fibonacci.rs:222-245) in one blocking call: rounds of toyni_fri_fold_commit_device
 * while the layer is longer than final_size (a power of two, >= 1).  The protocol's dependency is kept, not broken: before every
 * fold the library calls `challenge(user, round, root, &beta)` with the root committed by the previous round (root = NULL in
 * round 0) -- the caller's Fiat-Shamir transcript absorbs it (absorb_commitment, src/transcript.rs:29-32) and squeezes beta
 * (squeeze_challenge, :34-40); after the last round it is called once more with beta_out = NULL to absorb the last root.  A
 * non-zero return of the callback aborts with that code (after the stream has drained).  The callback runs on the calling thread
 * with the context locked: entry points on the SAME context return TOYNI_E_REENTRANT from inside it (other contexts are fine).
 * Per round only the 32-byte root crosses PCIe.
 *   d_layer0 : m0 words on the points x0 w_m0^i (the DEEP layer, :205-214); round k folds on x0^(2^k) (the squared domain, :228-231)
 *   d_salts  : 16 bytes per leaf for every SALTED layer back to back (m0/2 + m0/4 + ... leaves, the final layer excluded:
 *              build_unsalted_tree, :236-240), or NULL for unsalted trees throughout
 *   d_layers : out, the folded layers back to back (m0/2 + m0/4 + ... + final_size words)
 *   d_levels : out, their trees back to back (toyni_merkle_total_digests(m_k) x 32 bytes each, 16-byte aligned)
 *   h_roots  : out, rounds x 32 bytes (may be NULL); *rounds_out = number of rounds = log2(m0 / final_size)
 * `stream` carries the kernels; the call returns after the last root has been read back. */
typedef int (*toyni_fri_challenge_fn)(void* user, unsigned round, const uint8_t* prev_root32, uint32_t* beta_out);
int toyni_fri_commit_phase_device(toyni_ntt_ctx* ctx, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size,
                                  const uint8_t* d_salts, toyni_fri_challenge_fn challenge, void* user, uint32_t* d_layers,
                                  uint8_t* d_levels, uint8_t* h_roots, unsigned* rounds_out, void* stream);
/* Constraint and quotient evaluations (src/fibonacci.rs:133-150): with n = N >> log_blowup, g = w_n, T(g x_i) = trace[(i + B) mod N]:
 *   c_i = (T(g^2 x_i) - (T(g x_i) + T(x_i))) (x_i - g^(n-1)) (x_i - g^(n-2)),   q_i = c_i / (x_i^n - 1).
 * d_c_evals may be NULL.  TOYNI_E_ZERO_INVERSE if Z_H vanishes on the coset (shift^n a B-th root of unity). */
int toyni_fib_quotient_device(toyni_ntt_ctx* ctx, const uint32_t* d_trace_lde, uint32_t* d_c_evals, uint32_t* d_q_evals, unsigned log_blowup,
                              uint32_t shift, void* stream);
/* DEEP layer (src/fibonacci.rs:186-198): d_i = ((q_i - q_z) + (T(g^2 x_i) - t_ggz) + (T(g x_i) - t_gz) + (T(x_i) - t_z)) / (x_i - z);
 * ood = {t_z, t_gz, t_ggz, q_z}.  z must lie outside the coset (derive_z_from_transcript, :379-399, guarantees it); a point
 * with x_i = z yields 0 for that point alone (the reference panics: "Cannot invert zero"). */
int toyni_fib_deep_device(toyni_ntt_ctx* ctx, const uint32_t* d_trace_lde, const uint32_t* d_q_evals, uint32_t* d_out, unsigned log_blowup,
                          uint32_t shift, uint32_t z, const uint32_t ood[4], void* stream);
/* Polynomial::evaluate (src/math/polynomial.rs:134-144) of ncoeffs device-resident coefficients at 1..4 points (host values):
 * d_out[p] = sum_i c_i points[p]^i.  The OOD evaluations t_z, t_gz, t_ggz share one read of the coefficients. */
int toyni_poly_eval_device(toyni_ntt_ctx* ctx, const uint32_t* d_coeffs, size_t ncoeffs, const uint32_t* points, unsigned npoints,
                           uint32_t* d_out, void* stream);
/* Openings (open_merkle, src/fibonacci.rs:366-375, over MerkleTree::get_proof, src/merkle.rs:50-80) of nidx leaves of a tree built
 * by toyni_merkle_commit_device / toyni_fri_fold_commit_device, gathered on the device into nidx records of
 * toyni_merkle_open_record_bytes(n) bytes each:  depth x 32 path bytes | 16 salt bytes (zero if d_salts is NULL) | the value as
 * 8 LE bytes | depth position bytes (1 = the sibling is the LEFT input), padding zero to a multiple of 8.  Every byte of a
 * record is written.  d_out 8-byte aligned. */
size_t toyni_merkle_open_record_bytes(size_t n);
int toyni_merkle_open_device(const uint8_t* d_levels, size_t n, const uint32_t* d_values, const uint8_t* d_salts, const uint32_t* d_indices,
                             size_t nidx, uint8_t* d_out, void* stream);
/* The same for several trees at once (the query phase of a proof opens the trace, quotient and DEEP trees and every FRI layer's:
 * src/fibonacci.rs:249-295): one launch per 32 trees instead of one per tree.  Every field as in toyni_merkle_open_device. */
typedef struct {
    const uint8_t* d_levels;
    size_t n;
    const uint32_t* d_values;
    const uint8_t* d_salts;
    const uint32_t* d_indices;
    size_t nidx;
    uint8_t* d_out;
} toyni_merkle_open_group;
int toyni_merkle_open_groups_device(const toyni_merkle_open_group* groups, size_t ngroups, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 4. Plumbing
 * ---------------------------------------------------------------------------------------------- */
int toyni_malloc(void** d_ptr, size_t bytes);
/* Pinned (page-locked) host memory.  A host-slice entry point that is handed pinned memory (from here, or registered by the
 * caller with hipHostRegister) and at least two chunks of data (2 x 64 MiB; TOYNI_PIPE_CHUNK_BYTES) runs pipelined: the upload of
 * chunk k + 1, the kernels of chunk k and the download of chunk k - 1 overlap on three streams (PCIe is full duplex).  Pageable
 * memory (a Rust Vec, what the reference passes: src/ntt.rs:233) takes the plain upload - kernels - download path: its copies
 * are staged by the runtime and do not overlap. */
int toyni_host_alloc(void** h_ptr, size_t bytes);
int toyni_host_free(void* h_ptr);
int toyni_free(void* d_ptr);
int toyni_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int toyni_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
/* Stream-ordered copies and fills (asynchronous with pinned host memory; pageable host memory makes them block like HIP does). */
int toyni_memcpy_h2d_async(void* d_dst, const void* h_src, size_t bytes, void* stream);
int toyni_memcpy_d2h_async(void* h_dst, const void* d_src, size_t bytes, void* stream);
int toyni_memcpy_d2d_async(void* d_dst, const void* d_src, size_t bytes, void* stream);
int toyni_memset_async(void* d_ptr, int value, size_t bytes, void* stream);
/* Merkle salts on the device: bytes of the ChaCha20 keystream (RFC 8439: 256-bit key, block counter from 0, 96-bit nonce =
 * 0 || nonce as two little-endian words).  The reference draws 16 bytes per leaf from rand::thread_rng(), a ChaCha CSPRNG on the
 * host (src/fibonacci.rs:341-343); this keeps ~130 MB of salts per 2^16-row proof off PCIe.  bytes: a multiple of 64; d_out
 * 16-byte aligned.  The key is the caller's secret: draw it from the OS (getrandom) per proof. */
int toyni_chacha20_fill_device(void* d_out, size_t bytes, const uint8_t key[32], uint64_t nonce, void* stream);
int toyni_narrow_u64_to_u32(const uint64_t* d_in, uint32_t* d_out, size_t count, void* stream);
int toyni_widen_u32_to_u64(const uint32_t* d_in, uint64_t* d_out, size_t count, void* stream);
/* Streams for host languages that bind only this library: device -1 = the current device; the stream is non-blocking with respect
 * to HIP's legacy default stream.  toyni_stream_destroy waits for the stream's work first. */
int toyni_stream_create(void** stream, int device);
int toyni_stream_destroy(void* stream);
/* Ordering between two streams: what is enqueued on `stream` after this call runs after everything enqueued on `after` so far. */
int toyni_stream_wait(void* stream, void* after);
/* The same in two steps: mark a point of one stream now (toyni_event_record), make another stream wait for it later. */
int toyni_event_create(void** event);
int toyni_event_destroy(void* event);
int toyni_event_record(void* event, void* stream);
int toyni_stream_wait_event(void* stream, void* event);
int toyni_stream_synchronize(toyni_ntt_ctx* ctx, void* stream);   /* hipStreamSynchronize(stream); with a context: also releases what that stream outgrew */
int toyni_ntt_ctx_trim(toyni_ntt_ctx* ctx);                       /* hipDeviceSynchronize, then frees every intermediate buffer of the context */
/* Stream capture: a warm context only enqueues kernels, so its device-resident calls can be captured into a HIP graph.  One caveat:
 * after a context has outgrown or evicted an intermediate buffer, the next call on it that finds the buffer's event complete frees it
 * (hipFree: a device-wide synchronisation, illegal under a GLOBAL-mode capture).  The library skips that sweep while a stream the
 * CURRENT call enqueued on (or the context's own stream) is capturing, and runs it in relaxed mode on the calling thread; it never asks
 * about streams of earlier calls (the caller may have destroyed them since), so a global-mode capture that another thread has open on
 * some other stream is not visible to it.  Callers that capture on several threads use hipStreamCaptureModeThreadLocal / Relaxed, or
 * call toyni_ntt_ctx_trim (or a blocking entry point) before they start capturing.  A stream the context has carried may be destroyed
 * at any time; calling toyni_stream_synchronize(ctx, stream) first also releases what the context kept for it. */
int toyni_set_device(int device);
/* Diagnostics: the symbols (one per line) of every kernel this process has launched through the library so far.  Returns the bytes
 * needed including the terminating 0; (NULL, 0) asks for the size.  An in-memory list only: the library writes no file and reads no
 * environment variable for it.  Used by the test suite to prove that every kernel of the shipped binary was run (child processes of a
 * test session dump this list at exit through the test harness). */
size_t toyni_launched_kernels(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* TOYNI_HIP_H */
