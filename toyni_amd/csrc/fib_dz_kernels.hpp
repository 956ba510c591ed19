// The base-field first half of a Fibonacci proof on the device transcript (include/toyni_hip.h 3q).
//
// 3l - 3p carry an Ext-challenge proof without the host; the reference's own protocol (src/fibonacci.rs, one base-field z) still met
// the host at the mask, at derive_z, at the out-of-domain values, at the constraint check and at the DEEP layer.  Here each of those
// is a body that reads what depends on a challenge from device memory: a ONE-WAVE kernel expands z (and the claimed values) into a
// record in the stream's buffer and the hot kernels of 3c read the record.  Every function below produces, word for word, what the
// host code of toyni_poly_eval_device / toyni_fib_deep_device / csrc/host/fib_prover.hpp produces for the same canonical values: all
// of it is exact arithmetic mod p.  Every word read from device memory is reduced first (dz_reduce).
// Plain C++ so tests/emu can step it.
#pragma once
#include "dz_kernels.hpp"

namespace toyni {

// ---- the mask: T_hat = T - R + x^n R, R_i = (LE64 of keystream words 2 i, 2 i + 1) mod p ----
constexpr uint32_t FIB_MASK_MAX_DEGREE = 4096;
struct FibMaskArgs {
    uint32_t* coeffs;        // n + mask_degree words, in place
    uint64_t n;
    uint32_t mask_degree;
    uint32_t key[8];
    uint32_t nonce[3];       // 0 || nonce as two little-endian words (RFC 8439 layout of toyni_chacha20_fill_device)
};
// R_i: keystream block i / 8 holds eight of them (the block is computed whole: a thread needs one or two blocks)
TOYNI_HD uint32_t fib_mask_word(const FibMaskArgs& a, uint32_t i) {
    uint32_t ks[16];
    chacha20_block(a.key, i / 8u, a.nonce, ks);
    uint32_t lo = 0u, hi = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k)   // a constant register index per pass: no indexed access to ks
        if ((i & 7u) == k) { lo = ks[2u * k]; hi = ks[2u * k + 1u]; }
    return bb_reduce_u64((uint64_t)hi << 32 | lo);
}
// the words the mask touches, one per thread: [0, n + d) when the two ranges overlap (n < d), [0, d) and [n, n + d) otherwise
TOYNI_HD uint64_t fib_mask_items(uint64_t n, uint32_t d) { return n < d ? n + d : 2ull * d; }
TOYNI_HD uint64_t fib_mask_item_word(uint64_t n, uint32_t d, uint64_t t) { return (n < d || t < d) ? t : n + (t - d); }
// OUTPUT word j from its present value: minus R_j below d, plus R_(j - n) in [n, n + d); both where the ranges overlap
TOYNI_HD uint32_t fib_mask_output(const FibMaskArgs& a, uint64_t j, uint32_t cur) {
    uint32_t v = dz_reduce(cur);
    if (j < a.mask_degree) v = bb_sub(v, fib_mask_word(a, (uint32_t)j));
    if (j >= a.n && j - a.n < a.mask_degree) v = bb_add(v, fib_mask_word(a, (uint32_t)(j - a.n)));
    return v;
}

// ---- derive_z_from_transcript (src/fibonacci.rs:379-399): one challenge, again while z lies in <w_N> or in shift <w_N> ----
constexpr uint32_t FIB_POINT_TRIES = 8;
constexpr uint32_t FIB_POINT_MAX_LOG_N = 27;
// z plain canonical; shift_invR the Montgomery form of shift^-1.  True: z^N = 1 or (z / shift)^N = 1, N = 2^log_N.
TOYNI_HD bool fib_point_rejected(uint32_t z, uint32_t log_N, uint32_t shift_invR) {
    uint32_t a = to_mont(z);                 // z R
    uint32_t b = mont_mul(a, shift_invR);    // (z / shift) R
    for (uint32_t i = 0; i < log_N; ++i) {
        a = mont_mul(a, a);
        b = mont_mul(b, b);
    }
    return a == BB_R1 || b == BB_R1;
}
// One thread.  Accepted: z and the state after the last squeeze.  Not within `tries`, or a status already set: zero, the state as it
// was (and TRANSCRIPT_E_RANGE in the first case).  `tries` is a parameter so that a CPU test reaches the bound.
TOYNI_HD void transcript_squeeze_point(TranscriptState& tr, uint32_t log_N, uint32_t shift_invR, uint32_t tries, uint32_t* z) {
    const uint32_t len = tr.len, status = tr.status;
    bool ok = false;
    uint32_t v = 0u;
    TranscriptChain c{Digest{}, false};
    if (status == 0u && len <= TRANSCRIPT_CAPACITY) {
        for (uint32_t t = 0; t < tries && !ok; ++t) {
            transcript_step(tr, len, c);
            v = bb_reduce_u64(transcript_value(c.d));
            ok = !fib_point_rejected(v, log_N, shift_invR);
        }
    }
    z[0] = ok ? v : 0u;
    if (ok) transcript_store_digest(tr, c.d);
    else if (status == 0u) tr.status = TRANSCRIPT_E_RANGE;
}

// ---- the powers of the evaluation points mults[p] * z: the three arrays of PolyEvalArgs ----
static_assert(POLY_PER_THREAD == 16u && POLY_CHUNK == 4096u, "z^16 and z^POLY_CHUNK are 4 and 12 squarings");
struct alignas(16) PolyDzRecord { uint32_t zR[POLY_MAX_POINTS], z16R[POLY_MAX_POINTS], zchunkR[POLY_MAX_POINTS]; };
TOYNI_HD void poly_dz_record_point(const uint32_t* z, uint32_t mult, uint32_t p, PolyDzRecord& rec) {
    uint32_t s = to_mont(mont_mul(dz_reduce(z[0]), to_mont(mult)));   // (mult z) R
    rec.zR[p] = s;
    for (int i = 0; i < 12; ++i) {
        s = mont_mul(s, s);
        if (i == 3) rec.z16R[p] = s;
    }
    rec.zchunkR[p] = s;
}
// PolyEvalArgs without the three arrays: the twins take the record as a second, read-only argument
struct PolyEvalDzArgs {
    const uint32_t* coeffs;
    uint64_t ncoeffs;
    uint32_t npoints, nblocks;
    uint32_t* partial;
    uint32_t* out;
};
// the arguments of poly_thread_term for point p, in slot 0: the record's words by scalar loads, as kernel arguments are fetched
TOYNI_HD PolyEvalArgs poly_dz_point_args(const PolyDzRecord* rec, uint32_t p) {
    PolyEvalArgs b{};
    b.zR[0] = TOYNI_UNIFORM_LOAD(&rec->zR[p]);
    b.z16R[0] = TOYNI_UNIFORM_LOAD(&rec->z16R[p]);
    return b;
}

// ---- the Fibonacci DEEP layer: z and the four claimed values as DeepArgs carries them, and the constraint check at z ----
struct alignas(16) FibDeepRecord { uint32_t zR, t_z, t_gz, t_ggz, q_z, pad[3]; };
struct FibCheckArgs {
    uint32_t b1R, b2R;       // Montgomery forms of g^(n-1), g^(n-2), g = the root of order n = trace_len
    uint32_t log_n;
};
// One thread.  ood = {t_z, t_gz, t_ggz, q_z}.  check (may be null): 1 where
// (t_ggz - t_gz - t_z)(z - g^(n-1))(z - g^(n-2)) == q_z (z^n - 1)   (src/fibonacci.rs:173-177), else 0.
TOYNI_HD void fib_deep_prepare(const uint32_t* z, const uint32_t* ood, const FibCheckArgs& k, FibDeepRecord* rec, uint32_t* check) {
    const uint32_t zR = to_mont(dz_reduce(z[0]));
    const uint32_t t_z = dz_reduce(ood[0]), t_gz = dz_reduce(ood[1]), t_ggz = dz_reduce(ood[2]), q_z = dz_reduce(ood[3]);
    rec->zR = zR;
    rec->t_z = t_z;
    rec->t_gz = t_gz;
    rec->t_ggz = t_ggz;
    rec->q_z = q_z;
    if (!check) return;
    const uint32_t fib = bb_sub(t_ggz, bb_add(t_gz, t_z));
    const uint32_t c_z = mont_mul(mont_mul(fib, bb_sub(zR, k.b1R)), bb_sub(zR, k.b2R));   // plain
    uint32_t znR = zR;
    for (uint32_t i = 0; i < k.log_n; ++i) znR = mont_mul(znR, znR);
    check[0] = c_z == mont_mul(q_z, bb_sub(znR, BB_R1)) ? 1u : 0u;
}
// the layer kernel's arguments from the record, in registers that are the same in every lane
TOYNI_HD void fib_deep_args_from_record(DeepArgs& a, const FibDeepRecord& rec) {
    a.zR = TOYNI_UNIFORM(rec.zR);
    a.t_z = TOYNI_UNIFORM(rec.t_z);
    a.t_gz = TOYNI_UNIFORM(rec.t_gz);
    a.t_ggz = TOYNI_UNIFORM(rec.t_ggz);
    a.q_z = TOYNI_UNIFORM(rec.q_z);
}

// ---- the roots of a commit phase's trees ----
// The phases of 3l / 3m write their trees back to back; tree k has m_first >> k leaves (a power of two) and 2 leaves - 1 digests,
// the root last.  Word t of rounds x 8: word t mod 8 of root t / 8.
constexpr uint32_t FRI_PHASE_MAX_ROUNDS = 64;
TOYNI_HD uint64_t fri_phase_root_digest(uint64_t m_first, uint32_t k) {
    uint64_t off = 0;
    for (uint32_t j = 0; j < k; ++j) off += 2u * (m_first >> j) - 1u;
    return off + 2u * (m_first >> k) - 2u;
}
TOYNI_HD uint32_t fri_phase_root_word(const uint32_t* levels, uint64_t m_first, uint32_t t) {
    return levels[8u * fri_phase_root_digest(m_first, t / 8u) + (t & 7u)];
}

}  // namespace toyni
