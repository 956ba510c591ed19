// Pointwise steps of the Fibonacci STARK prover on the LDE coset, for gfx950.
//
// What they restate (reference src/fibonacci.rs, `StarkProver::generate_proof`), element for element and exactly (field
// arithmetic, canonical outputs):
//   fib_quotient   :133-150  c(x) = (T(g^2 x) - (T(g x) + T(x))) (x - g^(n-1)) (x - g^(n-2)),  q(x) = c(x) / (x^n - 1)
//   fib_deep       :186-198  d(x) = (q(x) - q_z)/(x - z) + (T(g^2 x) - t_ggz)/(x - z) + (T(g x) - t_gz)/(x - z) + (T(x) - t_z)/(x - z)
//   poly_eval      src/math/polynomial.rs:134-144 (Horner), as per-thread Horner runs joined by powers of the point
//   merkle_open    src/merkle.rs:50-80 (get_proof) + open_merkle src/fibonacci.rs:366-375
//   fold + commit  src/fibonacci.rs:222-245: fri_fold of layer k fused with the leaf hashes of layer k + 1's tree
// on x_i = shift * w_N^i, where T(g x_i) = trace_lde[(i + B) mod N] (g = w_n = w_N^B, B = N / n the blow-up).
// The reference evaluates every one of these by Horner per point on one core (O(N d)); here they are HBM-bound sweeps.
// Bodies are plain C++ (tests/emu can step them); the kernels wrapping them live in toyni_hip.hip.
#pragma once
#include "merkle_kernels.hpp"
#include "ntt_kernels.hpp"

namespace toyni {

// x_i = shift * w_N^i from the context's forward two-level domain table; returned in MONTGOMERY form (x_i * R)
struct DomainArgs {
    SubDomain dom;        // w_N'^(i << s): the order-N subgroup inside the context's (possibly larger) forward domain table (ntt_kernels.hpp)
    uint32_t shiftR;      // Montgomery form of the coset shift
};
TOYNI_HD uint32_t domain_point_mont(const DomainArgs& d, uint64_t i) {
    return mont_mul(subdomain_mont(d.dom, (uint32_t)i), d.shiftR);   // shift * w^i * R
}

// a^-1 in Montgomery form (aR -> a^-1 R) by Fermat, as BabyBear::inverse (src/babybear.rs:111-114); 0 -> 0
TOYNI_HD uint32_t mont_inv(uint32_t aR) { return mont_inv_chain(aR); }   // bb_field.hpp: 41 products instead of the ladder's 60
TOYNI_HD uint32_t mont_pow(uint32_t aR, uint64_t e) {
    uint32_t r = BB_R1;
    while (e) {
        if (e & 1u) r = mont_mul(r, aR);
        aR = mont_mul(aR, aR);
        e >>= 1;
    }
    return r;
}

// ---- constraint and quotient (src/fibonacci.rs:133-150) ----
struct QuotientArgs {
    const uint32_t* trace;   // trace_lde, N words
    uint32_t* c_out;         // constraint evaluations (may be null)
    uint32_t* q_out;         // quotient evaluations
    DomainArgs dom;
    uint32_t log_N, log_blowup;
    uint32_t b1R, b2R;       // Montgomery forms of g^(n-1), g^(n-2) (boundary_constraint_1/2, :318-324)
    uint32_t shift_nR;       // Montgomery form of shift^n: x_i^n = shift^n * w_B^(i mod B), only B distinct values
    uint32_t wBR;            // Montgomery form of w_B = w_N^n
};
// 1 / Z_H(x_i) = 1 / (x_i^n - 1) for residue class t = i mod B, Montgomery form (one Fermat inversion per class, not per point)
TOYNI_HD uint32_t zh_inv_class(uint32_t shift_nR, uint32_t wBR, uint32_t t) {
    const uint32_t xnR = mont_mul(shift_nR, mont_pow(wBR, t));   // (shift^n w_B^t) R
    return mont_inv(bb_sub(xnR, BB_R1));
}
TOYNI_HD uint32_t quotient_zh_inv(const QuotientArgs& a, uint32_t t) { return zh_inv_class(a.shift_nR, a.wBR, t); }
TOYNI_HD void quotient_one(const QuotientArgs& a, uint64_t i, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t zh_invR, uint32_t& c, uint32_t& q) {
    const uint32_t xR = domain_point_mont(a.dom, i);
    const uint32_t fib = bb_sub(t2, bb_add(t1, t0));                      // fibonacci_constraint, :313-315
    const uint32_t u = mont_mul(fib, bb_sub(xR, a.b1R));                  // fib * (x - g^(n-1))      (plain)
    c = mont_mul(u, bb_sub(xR, a.b2R));                                   // ... * (x - g^(n-2))       (plain)
    q = mont_mul(c, zh_invR);                                             // c / Z_H(x)
}

// ---- DEEP layer (src/fibonacci.rs:186-198) ----
struct DeepArgs {
    const uint32_t* trace;
    const uint32_t* quot;
    uint32_t* out;
    DomainArgs dom;
    uint32_t log_N, log_blowup;
    uint32_t wNR;            // Montgomery form of w_N (step between consecutive points)
    uint32_t zR;             // Montgomery form of z
    uint32_t t_z, t_gz, t_ggz, q_z;  // plain
};
// K consecutive points share ONE Fermat inversion (Montgomery's trick); a zero x_i - z (excluded by derive_z,
// src/fibonacci.rs:379-399) is kept out of the product and contributes x^-1 = 0 for that point alone.
template <int K>
TOYNI_HD void deep_group(const DeepArgs& a, uint64_t i0, const uint32_t (&t0)[K], const uint32_t (&t1)[K], const uint32_t (&t2)[K],
                         const uint32_t (&qv)[K], uint32_t (&out)[K]) {
    uint32_t dR[K], pre[K];
    uint32_t xR = domain_point_mont(a.dom, i0);
    uint32_t acc = BB_R1;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        dR[j] = bb_sub(xR, a.zR);                 // (x_j - z) R
        if (dR[j] == 0u) dR[j] = BB_R1 | 0x80000000u;   // marker (never a canonical value): handled below
        pre[j] = acc;
        acc = mont_mul(acc, (dR[j] & 0x80000000u) ? BB_R1 : dR[j]);
        if (j + 1 < K) xR = mont_mul(xR, a.wNR);
    }
    uint32_t inv = mont_inv(acc);
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
        const bool zero = (dR[j] & 0x80000000u) != 0u;
        const uint32_t invR = zero ? 0u : mont_mul(inv, pre[j]);          // (x_j - z)^-1 R
        if (!zero) inv = mont_mul(inv, dR[j]);
        const uint32_t num = bb_add(bb_add(bb_sub(qv[j], a.q_z), bb_sub(t2[j], a.t_ggz)), bb_add(bb_sub(t1[j], a.t_gz), bb_sub(t0[j], a.t_z)));
        out[j] = mont_mul(num, invR);
    }
}

// ---- DEEP combination of a column-major matrix (include/toyni_hip.h 3e): the layer above for any set of columns ----
//   d_i = ( sum_t alpha_t M(column_t, (i + rot_t) mod N) - C ) / (x_i - z),   C = sum_t alpha_t value_t  (host, once)
// One table entry per term, sorted by (column, rot) on the host so that the rotations of a column are read back to back.
struct alignas(16) DeepTerm {
    uint32_t column;
    uint32_t rot;            // rotation * B: the distance in words, < N
    uint32_t alphaR;         // Montgomery form of the weight
    uint32_t pad;
};
struct DeepCombineArgs {
    const uint32_t* values;  // element (i, c) at values[c * col_stride + i]
    uint32_t* out;
    uint64_t col_stride;
    DomainArgs dom;
    uint32_t log_N, nterms;
    uint32_t wNR;            // Montgomery form of w_N
    uint32_t zR;             // Montgomery form of z
    uint32_t claim;          // C, plain
    uint32_t accumulate;
};
typedef uint32_t DeepQuad __attribute__((vector_size(16)));   // one 16-byte load as a whole (a struct of four words is split and re-merged unevenly)
// the K words of one term for the points i0 .. i0 + K - 1 (i0 a multiple of K; N a multiple of K): two 16-byte loads where the
// column's first word is 16-byte aligned and the rotation a multiple of 4 (each quad then lies inside the column: N is a multiple
// of 8, so only a whole quad wraps), word loads otherwise
template <int K>
TOYNI_HD void deep_term_load(const DeepCombineArgs& a, const DeepTerm& t, uint64_t i0, uint32_t (&v)[K]) {
    const uint64_t mask = ((uint64_t)1 << a.log_N) - 1;
    const uint32_t* col = a.values + (uint64_t)t.column * a.col_stride;
    if (K == 8 && !(((uintptr_t)col & 15) | (t.rot & 3u))) {
        const DeepQuad lo = *reinterpret_cast<const DeepQuad*>(col + ((i0 + t.rot) & mask));
        const DeepQuad hi = *reinterpret_cast<const DeepQuad*>(col + ((i0 + t.rot + 4) & mask));
        const uint32_t w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = w[j & 7];
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = col[(i0 + (uint64_t)j + t.rot) & mask];
    }
}
// (x_j - z)^-1 R for the K points from i0 on, by ONE Fermat inversion (Montgomery's trick, as deep_group); 0 where x_j = z
template <int K>
TOYNI_HD void deep_point_inverses(const DomainArgs& dom, uint32_t wNR, uint32_t zR, uint64_t i0, uint32_t (&invR)[K]) {
    uint32_t dR[K], pre[K];
    uint32_t xR = domain_point_mont(dom, i0);
    uint32_t acc = BB_R1;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        dR[j] = bb_sub(xR, zR);
        if (dR[j] == 0u) dR[j] = BB_R1 | 0x80000000u;   // marker (never a canonical value)
        pre[j] = acc;
        acc = mont_mul(acc, (dR[j] & 0x80000000u) ? BB_R1 : dR[j]);
        if (j + 1 < K) xR = mont_mul(xR, wNR);
    }
    uint32_t inv = mont_inv(acc);
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
        const bool zero = (dR[j] & 0x80000000u) != 0u;
        invR[j] = zero ? 0u : mont_mul(inv, pre[j]);
        if (!zero) inv = mont_mul(inv, dR[j]);
    }
}
// entry t of the table: the same in every lane, so scalar registers and uniform branches
TOYNI_HD DeepTerm deep_term_at(const DeepTerm* terms, uint32_t t) {
    return DeepTerm{TOYNI_UNIFORM(terms[t].column), TOYNI_UNIFORM(terms[t].rot), TOYNI_UNIFORM(terms[t].alphaR), 0u};
}
// The products of four terms share one Montgomery reduction (mont_reduce_wide): 4 multiply-adds + 9 operations per point, 3.25 per
// term, where one mont_mul + bb_add per term spends 8 and pairs through mont_dot2 spend 4.5.  The term loop's trip count is data;
// everything inside it indexes registers with constants.
template <int K>
TOYNI_HD void deep_combine_group(const DeepCombineArgs& a, const DeepTerm* terms, uint64_t i0, uint32_t (&d)[K]) {
    uint32_t sum[K];
#pragma unroll
    for (int j = 0; j < K; ++j) sum[j] = 0u;
    uint32_t t = 0;
    for (; t + 4 <= a.nterms; t += 4) {
        uint64_t acc[K];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const DeepTerm tm = deep_term_at(terms, t + q);
            uint32_t v[K];
            deep_term_load<K>(a, tm, i0, v);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                TOYNI_FIELD_CONTRACT(WIDE_ACC, v[j], tm.alphaR, q + 1);
                acc[j] = (q ? acc[j] : 0ull) + (uint64_t)v[j] * tm.alphaR;
            }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) sum[j] = bb_add(sum[j], mont_reduce_wide(acc[j]));
    }
    if (t < a.nterms) {   // one to three terms left
        uint64_t acc[K];
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] = 0ull;
        const uint32_t tail0 = t;   // where the sums were zeroed: the contract hook counts the products from here
        (void)tail0;
        for (; t < a.nterms; ++t) {
            const DeepTerm tm = deep_term_at(terms, t);
            uint32_t v[K];
            deep_term_load<K>(a, tm, i0, v);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                TOYNI_FIELD_CONTRACT(WIDE_ACC, v[j], tm.alphaR, t - tail0 + 1u);
                acc[j] += (uint64_t)v[j] * tm.alphaR;
            }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) sum[j] = bb_add(sum[j], mont_reduce_wide(acc[j]));
    }
    uint32_t invR[K];
    deep_point_inverses<K>(a.dom, a.wNR, a.zR, i0, invR);
#pragma unroll
    for (int j = 0; j < K; ++j) d[j] = mont_mul(bb_sub(sum[j], a.claim), invR[j]);
}

// ---- the same under Ext challenges (include/toyni_hip.h 3h): base-field matrix, z and the weights in Ext = F_p[X]/(X^4 - 11) ----
//   d_i = ( sum_t alpha_t M(column_t, (i + rot_t) mod N) - C ) / (x_i - z)   in Ext,   C = sum_t alpha_t value_t  (host, once)
// Host-side Ext arithmetic on plain residues (src/ext.rs:178-192), for what a call prepares once.
constexpr uint32_t EXT_W = 11u;                                     // X^4 = EXT_W
constexpr uint32_t EXT_W_R = cx_mulmod(EXT_W, BB_R1);              // its Montgomery form
constexpr uint32_t EXT_ZETA = cx_powmod(EXT_W, (BB_P - 1) / 4);    // X^p = EXT_ZETA X: the Frobenius map scales coordinate k by EXT_ZETA^k
static_assert(cx_mulmod(EXT_ZETA, EXT_ZETA) == BB_P - 1u, "zeta has order 4");
inline void ext_mul_host(const uint32_t a[4], const uint32_t b[4], uint32_t r[4]) {
    uint64_t t[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) t[i + j] = (t[i + j] + (uint64_t)bb_mul_host(a[i], b[j])) % BB_P;
    for (int k = 0; k < 4; ++k) r[k] = (uint32_t)((t[k] + (k < 3 ? (uint64_t)EXT_W * t[k + 4] : 0ull)) % BB_P);
}
inline void ext_pow_host(const uint32_t b[4], uint64_t e, uint32_t r[4]) {
    uint32_t acc[4] = {1u, 0u, 0u, 0u}, sq[4] = {b[0], b[1], b[2], b[3]};
    for (; e; e >>= 1) {
        if (e & 1u) ext_mul_host(acc, sq, acc);
        ext_mul_host(sq, sq, sq);
    }
    for (int k = 0; k < 4; ++k) r[k] = acc[k];
}
// (x - z)^-1 for BASE x and Ext z behind one BASE inversion.  The conjugates of z are coordinate-wise, phi^j(z)_k = z_k zeta^(j k), so
//   (x - z)^-1 = adj_z(x) / m_z(x),   adj_z(x) = prod_{j=1..3} (x - phi^j(z))  (a cubic in x, Ext coefficients),
//                                     m_z(x) = (x - z) adj_z(x)                (the norm: a monic quartic, base coefficients)
// and m_z(x) = 0 only where x = z.  The host expands both once per z; coefficient i belongs to x^i, the leading ones are 1.
struct ExtShift {
    uint32_t adjR[3][4];     // Montgomery forms
    uint32_t mR[4];
};
inline ExtShift ext_shift_host(const uint32_t z[4]) {
    uint32_t c[3][4], zj = 1u;
    for (int j = 0; j < 3; ++j) {
        zj = bb_mul_host(zj, EXT_ZETA);                 // zeta^(j + 1)
        uint32_t zjk = 1u;
        for (int k = 0; k < 4; ++k) { c[j][k] = bb_mul_host(z[k], zjk); zjk = bb_mul_host(zjk, zj); }
    }
    const auto neg = [](uint32_t v) { return v ? BB_P - v : 0u; };
    uint32_t a[3][4], c01[4], s01[4], t[4], m[4];
    ext_mul_host(c[0], c[1], c01);
    for (int k = 0; k < 4; ++k) s01[k] = (uint32_t)(((uint64_t)c[0][k] + c[1][k]) % BB_P);
    ext_mul_host(s01, c[2], t);
    ext_mul_host(c01, c[2], a[0]);
    for (int k = 0; k < 4; ++k) {
        a[2][k] = neg((uint32_t)(((uint64_t)s01[k] + c[2][k]) % BB_P));    // -(c1 + c2 + c3)
        a[1][k] = (uint32_t)(((uint64_t)c01[k] + t[k]) % BB_P);            // c1 c2 + (c1 + c2) c3
        a[0][k] = neg(a[0][k]);                                           // -c1 c2 c3
    }
    // (x - z)(x^3 + a2 x^2 + a1 x + a0): coordinate 0 of each coefficient (the others cancel)
    m[3] = (uint32_t)(((uint64_t)a[2][0] + neg(z[0])) % BB_P);
    for (int i = 2; i >= 1; --i) { ext_mul_host(z, a[i], t); m[i] = (uint32_t)(((uint64_t)a[i - 1][0] + neg(t[0])) % BB_P); }
    ext_mul_host(z, a[0], t);
    m[0] = neg(t[0]);
    ExtShift s;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 4; ++k) s.adjR[i][k] = to_mont_host(a[i][k]);
    for (int i = 0; i < 4; ++i) s.mR[i] = to_mont_host(m[i]);
    return s;
}
// invR[j] = (x_j - z)^-1 as four Montgomery forms, for the K base points xR[j] (Montgomery forms): both polynomials by Horner, then ONE
// Fermat inversion for the K norms (Montgomery's trick, a zero norm kept out of the chain with the marker of deep_point_inverses);
// all four coordinates 0 where x_j = z.  An Ext LogUp term 1 / (gamma + v) is this with z = -gamma and the column's values as points.
template <int K>
TOYNI_HD void ext_shifted_inverses(const ExtShift& s, const uint32_t (&xR)[K], uint32_t (&invR)[K][4]) {
    uint32_t dR[K], pre[K];
    uint32_t acc = BB_R1;
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t t = k ? s.adjR[2][k] : bb_add(s.adjR[2][0], xR[j]);
            t = bb_add(mont_mul(t, xR[j]), s.adjR[1][k]);
            invR[j][k] = bb_add(mont_mul(t, xR[j]), s.adjR[0][k]);      // adj_z(x_j), coordinate k
        }
        uint32_t m = bb_add(s.mR[3], xR[j]);
#pragma unroll
        for (int i = 2; i >= 0; --i) m = bb_add(mont_mul(m, xR[j]), s.mR[i]);
        dR[j] = m;                                                     // m_z(x_j)
        if (dR[j] == 0u) dR[j] = BB_R1 | 0x80000000u;                  // marker (never a canonical value)
        pre[j] = acc;
        acc = mont_mul(acc, (dR[j] & 0x80000000u) ? BB_R1 : dR[j]);
    }
    uint32_t inv = mont_inv(acc);
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
        const bool zero = (dR[j] & 0x80000000u) != 0u;
        const uint32_t mi = zero ? 0u : mont_mul(inv, pre[j]);        // m_z(x_j)^-1 R
        if (!zero) inv = mont_mul(inv, dR[j]);
#pragma unroll
        for (int k = 0; k < 4; ++k) invR[j][k] = mont_mul(invR[j][k], mi);
    }
}
// One table entry per term, 32 bytes, sorted by (column, rot) on the host as the base table is
struct alignas(16) DeepExtTerm {
    uint32_t column;
    uint32_t rot;            // rotation * B: the distance in words, < N
    uint32_t alphaR[4];      // Montgomery forms of the weight's coordinates
    uint32_t pad[2];
};
struct DeepExtArgs {
    const uint32_t* values;  // element (i, c) at values[c * col_stride + i]: base field
    uint32_t* out;           // N Ext elements, four consecutive words each; 16-byte aligned
    uint64_t col_stride;
    DomainArgs dom;
    uint32_t log_N, nterms;
    uint32_t wNR;            // Montgomery form of w_N
    uint32_t accumulate;
    uint32_t claim[4];       // C, plain
    ExtShift shift;          // adj_z and m_z
};
// the K words of one term for the points i0 .. i0 + K - 1 (i0 a multiple of K; N a multiple of K): one 16-byte load where the column's
// first word is 16-byte aligned and the rotation a multiple of 4 (the quad then lies inside the column), word loads otherwise
template <int K>
TOYNI_HD void deep_ext_term_load(const DeepExtArgs& a, const uint32_t column, const uint32_t rot, uint64_t i0, uint32_t (&v)[K]) {
    const uint64_t mask = ((uint64_t)1 << a.log_N) - 1;
    const uint32_t* col = a.values + (uint64_t)column * a.col_stride;
    if (K == 4 && !(((uintptr_t)col & 15) | (rot & 3u))) {
        const DeepQuad q = *reinterpret_cast<const DeepQuad*>(col + ((i0 + rot) & mask));
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = q[j & 3];
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = col[(i0 + (uint64_t)j + rot) & mask];
    }
}
// entry t of the table: the same in every lane, so scalar registers and uniform branches
TOYNI_HD DeepExtTerm deep_ext_term_at(const DeepExtTerm* terms, uint32_t t) {
    return DeepExtTerm{TOYNI_UNIFORM(terms[t].column), TOYNI_UNIFORM(terms[t].rot),
                       {TOYNI_UNIFORM(terms[t].alphaR[0]), TOYNI_UNIFORM(terms[t].alphaR[1]), TOYNI_UNIFORM(terms[t].alphaR[2]),
                        TOYNI_UNIFORM(terms[t].alphaR[3])}, {0u, 0u}};
}
// Per term and point four multiply-adds, one per coordinate of the weight, into 64-bit accumulators; four terms share a reduction as in
// deep_combine_group.  Then (S_j - C) * (x_j - z)^-1 as one Ext product by the point's inverse (ext_mul: the right factor in
// Montgomery form with its multiples of 11).  d[j]: the four plain coordinates of point i0 + j.
template <int K>
TOYNI_HD void deep_combine_ext_group(const DeepExtArgs& a, const DeepExtTerm* terms, uint64_t i0, uint32_t (&d)[K][4]) {
    uint32_t sum[K][4];
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) sum[j][k] = 0u;
    uint32_t t = 0;
    for (; t + 4 <= a.nterms; t += 4) {
        uint64_t acc[K][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const DeepExtTerm tm = deep_ext_term_at(terms, t + q);
            uint32_t v[K];
            deep_ext_term_load<K>(a, tm.column, tm.rot, i0, v);
#pragma unroll
            for (int j = 0; j < K; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    TOYNI_FIELD_CONTRACT(WIDE_ACC, v[j], tm.alphaR[k], q + 1);
                    acc[j][k] = (q ? acc[j][k] : 0ull) + (uint64_t)v[j] * tm.alphaR[k];
                }
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) sum[j][k] = bb_add(sum[j][k], mont_reduce_wide(acc[j][k]));
    }
    if (t < a.nterms) {   // one to three terms left
        uint64_t acc[K][4];
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[j][k] = 0ull;
        const uint32_t tail0 = t;   // where the sums were zeroed: the contract hook counts the products from here
        (void)tail0;
        for (; t < a.nterms; ++t) {
            const DeepExtTerm tm = deep_ext_term_at(terms, t);
            uint32_t v[K];
            deep_ext_term_load<K>(a, tm.column, tm.rot, i0, v);
#pragma unroll
            for (int j = 0; j < K; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    TOYNI_FIELD_CONTRACT(WIDE_ACC, v[j], tm.alphaR[k], t - tail0 + 1u);
                    acc[j][k] += (uint64_t)v[j] * tm.alphaR[k];
                }
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) sum[j][k] = bb_add(sum[j][k], mont_reduce_wide(acc[j][k]));
    }
    uint32_t xR[K], invR[K][4];
    xR[0] = domain_point_mont(a.dom, i0);
#pragma unroll
    for (int j = 1; j < K; ++j) xR[j] = mont_mul(xR[j - 1], a.wNR);
    ext_shifted_inverses<K>(a.shift, xR, invR);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        Ext4 s;
        ExtFactor f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s.c[k] = bb_sub(sum[j][k], a.claim[k]);
            f.b[k] = invR[j][k];
            f.b11[k] = mont_mul(invR[j][k], EXT_W_R);
        }
        const Ext4 r = ext_mul(s, f);
#pragma unroll
        for (int k = 0; k < 4; ++k) d[j][k] = r.c[k];
    }
}

// ---- constraint programs of any AIR over up to four column-major matrices (include/toyni_hip.h 3f) ----
//   c_i = sum_{EMIT k, b = 0} weights[k] value_k(i),   q_i = c_i / (x_i^n - 1) + sum_{EMIT k, b = 1} weights[k] value_k(i)
// A straight-line program, the same in every lane, is interpreted once per group of K consecutive points.  Its registers hold
// MONTGOMERY forms (a cell is converted when it is read, constants are converted on the host, x_i and the inverses come out of the
// domain table in that form), so MUL is one mont_mul; the weights stay plain, so that an EMIT's product is a plain residue.
// The register file is indexed by program data and therefore lives in memory the caller hands in (LDS on the device): slot r of a
// thread is the K words at regs[r * stride], stride = K x the workgroup's threads -- every lane of a wave reads its own 4 K
// consecutive bytes, no bank is asked twice.  The program was validated on the host (toyni_air_program_check): no index is checked here.
// A word of a table that nothing in the kernel writes, at an address that is the same in every lane: read through the constant
// address space it is a scalar load whatever else the kernel loads and stores (the compiler proves that by itself only for some shapes)
#if defined(__HIP_DEVICE_COMPILE__)
#define TOYNI_UNIFORM_LOAD(p) (*reinterpret_cast<const __attribute__((address_space(4))) uint32_t*>((uintptr_t)(p)))
#else
#define TOYNI_UNIFORM_LOAD(p) (*(p))
#endif
constexpr uint32_t AIR_MAX_REGS = 64, AIR_MAX_MATRICES = 4, AIR_MAX_INSNS = 65536, AIR_INLINE_WEIGHTS = 64;
constexpr uint32_t AIR_ZH_LDS_CLASSES = 256;   // 1 / Z_H per residue class i mod B sits in LDS up to this B, per thread beyond
enum : uint32_t { AIR_OP_CELL = 0, AIR_OP_CONST, AIR_OP_X, AIR_OP_XINV, AIR_OP_ADD, AIR_OP_SUB, AIR_OP_MUL, AIR_OP_EMIT, AIR_OP_COUNT };
struct AirInsn {
    uint32_t w0;             // op | dst << 8 | a << 16 | b << 24
    uint32_t imm;            // CONST, XINV: Montgomery form
};
struct AirArgs {
    const AirInsn* insns;
    const uint32_t* mat[AIR_MAX_MATRICES];      // element (i, c) of matrix m at mat[m][c * col_stride[m] + i]
    uint64_t col_stride[AIR_MAX_MATRICES];
    uint32_t* c_out;         // may be null
    uint32_t* q_out;
    DomainArgs dom;
    uint32_t ninsns, nregs;
    uint32_t log_N, log_blowup;
    uint32_t wNR;            // Montgomery form of w_N
    uint32_t shift_nR, wBR;  // as QuotientArgs: x_i^n = shift^n w_B^(i mod B)
    uint32_t divides;        // some EMIT has b = 0: Z_H is needed (and does not vanish on the coset)
    uint32_t zh_lds;         // the workgroup keeps 1 / Z_H of all B classes in LDS
    uint32_t accumulate;
};
// The launch shape of a program (host side; tests/emu steps it too).  threads: the largest of 256 / 128 / 64 whose register file,
// 16 bytes per register and thread, fits AIR_LDS_MAX -- the register file alone decides it.  zh_lds: the B classes of 1 / Z_H go
// behind the register file when a divided constraint needs them, B <= AIR_ZH_LDS_CLASSES and the bytes that are left hold them;
// otherwise every thread inverts for its own points.  lds_bytes is what the launch allocates.
constexpr uint32_t AIR_LDS_MAX = 64u << 10;
struct AirLaunchShape { uint32_t threads, lds_bytes, zh_lds; };
inline AirLaunchShape air_launch_shape(uint32_t nregs, uint32_t divides, uint32_t log_blowup) {
    AirLaunchShape s{256u, 0u, 0u};
    while (s.threads > 64u && nregs * s.threads * 16u > AIR_LDS_MAX) s.threads >>= 1;
    s.lds_bytes = nregs * s.threads * 16u;
    if (divides && log_blowup < 32u && (1ull << log_blowup) <= AIR_ZH_LDS_CLASSES && s.lds_bytes + (4u << log_blowup) <= AIR_LDS_MAX) {
        s.zh_lds = 1u;
        s.lds_bytes += 4u << log_blowup;
    }
    return s;
}
// 1 / Z_H(x_j) R for the K points from i0 on by ONE Fermat inversion (no factor is zero: the host refuses a coset Z_H vanishes on)
template <int K>
TOYNI_HD void air_zh_inverses(const AirArgs& a, uint64_t i0, uint32_t (&zhR)[K]) {
    uint32_t z[K], pre[K];
    uint32_t xnR = mont_mul(a.shift_nR, mont_pow(a.wBR, i0 & (((uint64_t)1 << a.log_blowup) - 1)));
    uint32_t acc = BB_R1;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        z[j] = bb_sub(xnR, BB_R1);
        pre[j] = acc;
        acc = mont_mul(acc, z[j]);
        if (j + 1 < K) xnR = mont_mul(xnR, a.wBR);   // w_B^B = 1: running past a class boundary wraps by itself
    }
    uint32_t inv = mont_inv(acc);
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
        zhR[j] = mont_mul(inv, pre[j]);
        inv = mont_mul(inv, z[j]);
    }
}
// the K words of one cell for the points i0 .. i0 + K - 1 (i0 and N multiples of K): one 16-byte load under deep_term_load's
// conditions (the column's first word 16-byte aligned, the distance a multiple of 4), word loads otherwise
template <int K>
TOYNI_HD void air_cell_load(const AirArgs& a, uint32_t m, uint32_t column, uint32_t rotation, uint64_t i0, uint32_t (&v)[K]) {
    const uint64_t mask = ((uint64_t)1 << a.log_N) - 1;
    const uint32_t* col = a.mat[m] + (uint64_t)column * a.col_stride[m];
    const uint64_t rot = (uint64_t)rotation << a.log_blowup;   // < N
    if (K == 4 && !(((uintptr_t)col & 15) | (rot & 3u))) {
        const DeepQuad w = *reinterpret_cast<const DeepQuad*>(col + ((i0 + rot) & mask));
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = w[j & 3];
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = col[(i0 + (uint64_t)j + rot) & mask];
    }
}
template <int K>
TOYNI_HD void air_reg_load(const uint32_t* regs, uint32_t stride, uint32_t r, uint32_t (&v)[K]) {
    if (K == 4) {
        const DeepQuad w = *reinterpret_cast<const DeepQuad*>(regs + r * stride);
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = w[j & 3];
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = regs[r * stride + j];
    }
}
template <int K>
TOYNI_HD void air_reg_store(uint32_t* regs, uint32_t stride, uint32_t r, const uint32_t (&v)[K]) {
    if (K == 4) {
        *reinterpret_cast<DeepQuad*>(regs + r * stride) = DeepQuad{v[0], v[1 % K], v[2 % K], v[3 % K]};
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) regs[r * stride + j] = v[j];
    }
}
// zhR: 1 / Z_H of the K points (unused without a divided constraint).  c and q come out as plain canonical residues.
template <int K>
TOYNI_HD void air_eval_group(const AirArgs& a, const uint32_t* weights, uint32_t* regs, uint32_t stride, uint64_t i0, const uint32_t (&zhR)[K],
                             uint32_t (&c)[K], uint32_t (&q)[K]) {
    uint32_t xR[K], undiv[K];
    xR[0] = domain_point_mont(a.dom, i0);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j) xR[j] = mont_mul(xR[j - 1], a.wNR);
        c[j] = 0u;
        undiv[j] = 0u;
    }
    for (uint32_t pc = 0; pc < a.ninsns; ++pc) {
        const uint32_t w0 = TOYNI_UNIFORM_LOAD(&a.insns[pc].w0), imm = TOYNI_UNIFORM_LOAD(&a.insns[pc].imm);   // the same in every lane
        const uint32_t op = w0 & 255u, dst = (w0 >> 8) & 255u, ra = (w0 >> 16) & 255u, rb = w0 >> 24;
        uint32_t v[K];
        if (op == AIR_OP_EMIT) {
            const uint32_t wt = TOYNI_UNIFORM(weights[imm]);   // (the inline table is a kernel argument: taking its address as a number would spill it)
            air_reg_load<K>(regs, stride, ra, v);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t term = mont_mul(wt, v[j]);   // plain weight x Montgomery value = plain product
                if (rb) undiv[j] = bb_add(undiv[j], term);
                else c[j] = bb_add(c[j], term);
            }
            continue;
        }
        if (op >= AIR_OP_ADD) {
            uint32_t u[K], w[K];
            air_reg_load<K>(regs, stride, ra, u);
            air_reg_load<K>(regs, stride, rb, w);
            if (op == AIR_OP_MUL) {   // op is uniform: three branches, not three results and a select
#pragma unroll
                for (int j = 0; j < K; ++j) v[j] = mont_mul(u[j], w[j]);
            } else if (op == AIR_OP_ADD) {
#pragma unroll
                for (int j = 0; j < K; ++j) v[j] = bb_add(u[j], w[j]);
            } else {
#pragma unroll
                for (int j = 0; j < K; ++j) v[j] = bb_sub(u[j], w[j]);
            }
        } else if (op == AIR_OP_CELL) {
            air_cell_load<K>(a, rb, imm, ra, i0, v);
#pragma unroll
            for (int j = 0; j < K; ++j) v[j] = to_mont(v[j]);
        } else if (op == AIR_OP_XINV) {
            deep_point_inverses<K>(a.dom, a.wNR, imm, i0, v);
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) v[j] = op == AIR_OP_X ? xR[j] : imm;
        }
        air_reg_store<K>(regs, stride, dst, v);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) q[j] = a.divides ? bb_add(mont_mul(c[j], zhR[j]), undiv[j]) : undiv[j];
}

// ---- the same programs under Ext weights (include/toyni_hip.h 3k) ----
//   C_i = sum_{EMIT k, b = 0} W_k value_k(i),   Q_i = C_i / Z_H(x_i) + sum_{EMIT k, b = 1} W_k value_k(i),   W_k in Ext, values in F_p
// A base value times an Ext weight is four base products, so coordinate e of the result is air_eval_group's word under the base
// weights weights4[4 k + e]: ONE interpretation of the program with four accumulators, where four calls of the base kernel decode
// every instruction, load every cell and walk the LDS register file four times.  Everything but EMIT and the closing step is
// air_eval_group's text (the base function is left alone so that the base kernels' code objects stay what they are).  An EMIT loads
// the value group once and multiplies it by the four coordinates (plain, in scalar registers): mont_mul of a plain canonical weight
// and a canonical Montgomery value is a plain canonical product, bb_add keeps the accumulators canonical -- the operand domains of
// bb_field.hpp hold at every step, whatever the number and order of the EMITs.
constexpr uint32_t AIR_EXT_INLINE_WEIGHTS = 64;   // Ext weights inside the kernel arguments: 1 KiB (TOYNI_AIR_EXT_INLINE_WEIGHTS)
template <int K>
TOYNI_HD void air_eval_group_ext(const AirArgs& a, const uint32_t* weights4, uint32_t* regs, uint32_t stride, uint64_t i0, const uint32_t (&zhR)[K],
                                 uint32_t (&c)[4][K], uint32_t (&q)[4][K]) {
    uint32_t xR[K];
    xR[0] = domain_point_mont(a.dom, i0);
#pragma unroll
    for (int j = 1; j < K; ++j) xR[j] = mont_mul(xR[j - 1], a.wNR);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < K; ++j) c[e][j] = q[e][j] = 0u;   // q gathers the undivided constraints until the closing step
    for (uint32_t pc = 0; pc < a.ninsns; ++pc) {
        const uint32_t w0 = TOYNI_UNIFORM_LOAD(&a.insns[pc].w0), imm = TOYNI_UNIFORM_LOAD(&a.insns[pc].imm);   // the same in every lane
        const uint32_t op = w0 & 255u, dst = (w0 >> 8) & 255u, ra = (w0 >> 16) & 255u, rb = w0 >> 24;
        uint32_t v[K];
        if (op == AIR_OP_EMIT) {
            uint32_t wt[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) wt[e] = TOYNI_UNIFORM(weights4[4u * imm + e]);
            air_reg_load<K>(regs, stride, ra, v);
            if (rb) {   // rb is uniform: two branches, not two sums and a select
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < K; ++j) q[e][j] = bb_add(q[e][j], mont_mul(wt[e], v[j]));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < K; ++j) c[e][j] = bb_add(c[e][j], mont_mul(wt[e], v[j]));
            }
            continue;
        }
        if (op >= AIR_OP_ADD) {
            uint32_t u[K], w[K];
            air_reg_load<K>(regs, stride, ra, u);
            air_reg_load<K>(regs, stride, rb, w);
            if (op == AIR_OP_MUL) {
#pragma unroll
                for (int j = 0; j < K; ++j) v[j] = mont_mul(u[j], w[j]);
            } else if (op == AIR_OP_ADD) {
#pragma unroll
                for (int j = 0; j < K; ++j) v[j] = bb_add(u[j], w[j]);
            } else {
#pragma unroll
                for (int j = 0; j < K; ++j) v[j] = bb_sub(u[j], w[j]);
            }
        } else if (op == AIR_OP_CELL) {
            air_cell_load<K>(a, rb, imm, ra, i0, v);
#pragma unroll
            for (int j = 0; j < K; ++j) v[j] = to_mont(v[j]);
        } else if (op == AIR_OP_XINV) {
            deep_point_inverses<K>(a.dom, a.wNR, imm, i0, v);
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) v[j] = op == AIR_OP_X ? xR[j] : imm;
        }
        air_reg_store<K>(regs, stride, dst, v);
    }
    if (a.divides) {   // four products with 1 / Z_H per point
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < K; ++j) q[e][j] = bb_add(mont_mul(c[e][j], zhR[j]), q[e][j]);
    }
}
// The K words of the points i0 .. i0 + K - 1 into the four coordinate columns out + e * out_stride (out may be null: nothing is
// written).  Whether a column takes the 16-byte store (and load, when accumulating) is decided from that column's OWN first word:
// with an out_stride that is no multiple of 4 the columns 1..3 are not aligned even where the base pointer is.
template <int K>
TOYNI_HD void air_ext_store(uint32_t* out, uint64_t out_stride, uint64_t i0, uint32_t accumulate, const uint32_t (&v)[4][K]) {
    if (!out) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uint32_t* col = out + (uint64_t)e * out_stride;
        if (K == 4 && !((uintptr_t)col & 15)) {
            DeepQuad* d4 = reinterpret_cast<DeepQuad*>(col + i0);
            DeepQuad r = DeepQuad{v[e][0], v[e][1 % K], v[e][2 % K], v[e][3 % K]};
            if (accumulate) {
                const DeepQuad p = *d4;
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = bb_add(p[j], r[j]);
            }
            *d4 = r;
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) col[i0 + j] = accumulate ? bb_add(col[i0 + j], v[e][j]) : v[e][j];
        }
    }
}

// ---- accumulator columns: a running sum or product along a column (include/toyni_hip.h 3g) ----
//   term_i = num_i / den_i (0 where den_i = 0),  out[0] = init,  out[i] = out[i-1] o term_{i-1},  o = + or *
// The only dependency from row to row in this library.  + and * mod p are associative and commutative, so the column is cut into
// tiles of SCAN_TILE elements and every partial result is exact whatever the order: (1) one aggregate and one zero count per tile,
// (2) an exclusive scan of a column's aggregates by one workgroup, (3) the scan inside each tile on top of the tile's prefix.
// Each launch is ordered after the last by the stream; no workgroup ever waits for another.
// Sums run on plain residues.  Products run on MONTGOMERY forms (identity R, one mont_mul per step) and are converted when stored.
constexpr uint32_t SCAN_SUM = 0, SCAN_PRODUCT = 1, SCAN_COUNT = 2;   // SCAN_COUNT: integer addition, for the zero counts
constexpr uint32_t SCAN_GROUP = 8, SCAN_THREADS = 256, SCAN_TILE = SCAN_GROUP * SCAN_THREADS, SCAN_WAVE = 64;
constexpr uint32_t SCAN_INLINE_COLUMNS = 64;    // columns of one launch sequence: their seeds ride in the kernel arguments
constexpr uint32_t SCAN_MAX_LOG_N = 27;
constexpr uint32_t BB_RINV = cx_powmod(BB_R1, BB_P - 2);   // R^-1 mod p
static_assert(cx_mulmod(BB_RINV, BB_R1) == 1u, "R^-1");
template <int OP> TOYNI_HD uint32_t scan_identity() { return OP == (int)SCAN_PRODUCT ? BB_R1 : 0u; }
template <int OP> TOYNI_HD uint32_t scan_combine(uint32_t a, uint32_t b) {
    return OP == (int)SCAN_SUM ? bb_add(a, b) : OP == (int)SCAN_PRODUCT ? mont_mul(a, b) : a + b;
}
template <int OP> TOYNI_HD uint32_t scan_to_plain(uint32_t v) { return OP == (int)SCAN_PRODUCT ? from_mont(v) : v; }
struct ScanArgs {
    const uint32_t* num;     // column b at num + b * num_stride; null: every numerator is 1
    const uint32_t* den;     // null: every denominator is 1
    uint32_t* out;
    uint64_t num_stride, den_stride, out_stride;
    uint64_t n;
    uint32_t* tiles;         // column b: ntiles aggregates (step 2 turns them into prefixes in place), then ntiles zero counts
    uint32_t* totals;        // [column][2], may be null
    uint32_t ntiles;
    uint32_t single;         // n <= one tile: step 3 alone, seeded by init, writes the totals
};
struct ScanInit { uint32_t v[SCAN_INLINE_COLUMNS]; };   // init[b]: plain for sums, Montgomery form for products
TOYNI_HD uint32_t* scan_tile_aggregates(const ScanArgs& a, uint32_t col) { return a.tiles + (uint64_t)col * 2u * a.ntiles; }
TOYNI_HD uint32_t* scan_tile_zeros(const ScanArgs& a, uint32_t col) { return scan_tile_aggregates(a, col) + a.ntiles; }
// the G words of a column from i0 on (i0 a multiple of G, G a multiple of 4): 16-byte loads where the column's first word is 16-byte
// aligned and the group lies inside the column, guarded word loads otherwise; `fill` past the end
template <int G>
TOYNI_HD void scan_group_load(const uint32_t* col, uint64_t i0, uint64_t n, uint32_t fill, uint32_t (&v)[G]) {
    static_assert(G % 4 == 0, "a group is whole quads");
    if (!((uintptr_t)col & 15) && i0 + G <= n) {
#pragma unroll
        for (int q = 0; q < G / 4; ++q) {
            const DeepQuad w = *reinterpret_cast<const DeepQuad*>(col + i0 + 4 * q);
            v[4 * q] = w[0]; v[4 * q + 1] = w[1]; v[4 * q + 2] = w[2]; v[4 * q + 3] = w[3];
        }
    } else {
#pragma unroll
        for (int j = 0; j < G; ++j) v[j] = i0 + (uint64_t)j < n ? col[i0 + j] : fill;
    }
}
template <int G>
TOYNI_HD void scan_group_store(uint32_t* col, uint64_t i0, uint64_t n, const uint32_t (&v)[G]) {
    if (!((uintptr_t)col & 15) && i0 + G <= n) {
#pragma unroll
        for (int q = 0; q < G / 4; ++q) *reinterpret_cast<DeepQuad*>(col + i0 + 4 * q) = DeepQuad{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    } else {
#pragma unroll
        for (int j = 0; j < G; ++j)
            if (i0 + (uint64_t)j < n) col[i0 + j] = v[j];
    }
}
// x_j = den_j^-1 * R * c (0 where den_j = 0) for the G plain residues den[]: ONE Fermat inversion (Montgomery's trick, zeros kept out
// of the chain with the marker of deep_point_inverses).  A plain residue d is read as the Montgomery form of d / R, so no operand is
// converted: the chain yields (d / R)^-1 R = d^-1 R^2, and the one factor c that the inverted product is multiplied by decides the form
// of all G results -- c = R: d^-1 R^2 (times a plain numerator: a Montgomery form), c = 1: d^-1 R, c = R^-1: d^-1.  Returns the zeros met.
template <int G>
TOYNI_HD uint32_t scan_group_inverses(uint32_t (&d)[G], uint32_t c, uint32_t (&x)[G]) {
    uint32_t pre[G];
    uint32_t acc = BB_R1, zeros = 0;
#pragma unroll
    for (int j = 0; j < G; ++j) {
        if (d[j] == 0u) d[j] = BB_R1 | 0x80000000u;   // marker (never a canonical value)
        pre[j] = acc;
        acc = mont_mul(acc, (d[j] & 0x80000000u) ? BB_R1 : d[j]);
    }
    uint32_t inv = mont_mul(mont_inv_chain(acc), c);
#pragma unroll
    for (int j = G - 1; j >= 0; --j) {
        const bool zero = (d[j] & 0x80000000u) != 0u;
        x[j] = zero ? 0u : mont_mul(inv, pre[j]);
        if (!zero) inv = mont_mul(inv, d[j]);
        zeros += zero ? 1u : 0u;
    }
    return zeros;
}
// the G terms from i0 on in the form the op scans (plain for a sum, Montgomery for a product); the identity past n.  numc / denc: the
// column's operands (one of them may be null).  Returns the zero denominators met below n.
template <int OP, int G>
TOYNI_HD uint32_t scan_group_terms(const uint32_t* numc, const uint32_t* denc, uint64_t i0, uint64_t n, uint32_t (&t)[G]) {
    constexpr bool PROD = OP == (int)SCAN_PRODUCT;
    uint32_t zeros = 0;
    if (denc) {
        uint32_t d[G], x[G];
        scan_group_load<G>(denc, i0, n, 1u, d);   // past n: 1, which is no zero
        zeros = scan_group_inverses<G>(d, numc ? (PROD ? BB_R1 : 1u) : (PROD ? 1u : BB_RINV), x);
        if (numc) {
            uint32_t u[G];
            scan_group_load<G>(numc, i0, n, 0u, u);
#pragma unroll
            for (int j = 0; j < G; ++j) t[j] = mont_mul(u[j], x[j]);
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j) t[j] = x[j];
        }
    } else {
        scan_group_load<G>(numc, i0, n, 0u, t);
        if (PROD) {
#pragma unroll
            for (int j = 0; j < G; ++j) t[j] = to_mont(t[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < G; ++j)
        if (i0 + (uint64_t)j >= n) t[j] = scan_identity<OP>();
    return zeros;
}
// thread-serial part: ex[j] = t[0] o ... o t[j-1]; returns the group's total
template <int OP, int G>
TOYNI_HD uint32_t scan_thread_serial(const uint32_t (&t)[G], uint32_t (&ex)[G]) {
    uint32_t acc = scan_identity<OP>();
#pragma unroll
    for (int j = 0; j < G; ++j) {
        ex[j] = acc;
        acc = scan_combine<OP>(acc, t[j]);
    }
    return acc;
}
// THE cross-lane step of the scans: the value of the lane `delta` below (a lane below `delta` gets its own value back).  On the device
// one ds_bpermute_b32 (__shfl_up); on the CPU the wave is an array of 64 values that tests/emu steps lane by lane.
#if defined(__HIPCC__) || defined(TOYNI_KERNEL_TEXT_ONLY)
TOYNI_DEV uint32_t scan_lane_up(uint32_t v, uint32_t delta) { return (uint32_t)__shfl_up((int)v, delta, (int)SCAN_WAVE); }
#endif
inline uint32_t scan_lane_up(const uint32_t (&wave)[SCAN_WAVE], uint32_t lane, uint32_t delta) { return wave[lane >= delta ? lane - delta : lane]; }
// one of the log2(64) steps of the inclusive scan across a wave's lanes (Hillis-Steele: delta = 1, 2, 4 ... 32)
template <int OP> TOYNI_HD uint32_t scan_wave_step(uint32_t v, uint32_t below, uint32_t lane, uint32_t delta) {
    return lane >= delta ? scan_combine<OP>(below, v) : v;
}
// from the waves' totals (LDS): what the waves below `wave` add up to; `total` = all of them
template <int OP, int NW>
TOYNI_HD uint32_t scan_waves_below(const uint32_t* wave_tot, uint32_t wave, uint32_t& total) {
    uint32_t pre = scan_identity<OP>();
    total = scan_identity<OP>();
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if ((uint32_t)w == wave) pre = total;
        total = scan_combine<OP>(total, wave_tot[w]);
    }
    return pre;
}
// what step 3 stores: base o ex[j], as plain residues
template <int OP, int G>
TOYNI_HD void scan_group_finish(uint32_t base, const uint32_t (&ex)[G], uint32_t (&o)[G]) {
#pragma unroll
    for (int j = 0; j < G; ++j) o[j] = scan_to_plain<OP>(scan_combine<OP>(base, ex[j]));
}

// ---- accumulator columns under an Ext challenge (include/toyni_hip.h 3i) ----
// The recurrence and the three launches of 3g with every value in Ext = F_p[X]/(X^4 - 11); Ext is a commutative field, so every
// partial result is exact whatever the order.  An Ext column is FOUR base columns: coordinate k of element i of column b at
// values[(4 b + k) * stride + i].  Sums run coordinate-wise on plain residues; products on Montgomery forms, one general Ext x Ext
// product per step.  A thread owns EXT_ACCUM_GROUP consecutive elements (16 words of terms and 16 of running values: no scratch).
constexpr uint32_t EXT_ACCUM_GROUP = 4, EXT_ACCUM_THREADS = 256, EXT_ACCUM_TILE = EXT_ACCUM_GROUP * EXT_ACCUM_THREADS;
constexpr uint32_t EXT_ACCUM_INLINE_COLUMNS = 16;   // Ext columns of one launch sequence: their seeds ride in the kernel arguments
constexpr uint32_t EXT_ACCUM_TILE_WORDS = 5;        // per tile and column: four aggregate coordinates and a zero count
struct ExtAccumOperand {
    const uint32_t* values;  // column 0 (null with width 0)
    uint64_t stride;
    uint32_t width;          // 4: an Ext column; 1: a base column; 0: the constant 1
    uint32_t shift[4];       // plain: added to every element
};
struct ExtAccumArgs {
    ExtAccumOperand num, den;
    ExtShift den_inv;        // a width-1 denominator: 1 / (shift + v) = 1 / (v - z), z = -shift (ext_shift_host)
    uint32_t* out;           // Ext columns
    uint64_t out_stride;
    uint64_t n;
    uint32_t* tiles;         // column b: an Ext column of ntiles aggregates (step 2 turns them into prefixes in place), then ntiles zero counts
    uint32_t* totals;        // [column][8], may be null
    uint32_t ntiles;
    uint32_t single;         // n <= one tile: step 3 alone, seeded by init, writes the totals
};
struct ExtAccumSeeds { uint32_t v[EXT_ACCUM_INLINE_COLUMNS][4]; };   // init[b]: plain for sums, Montgomery forms for products
TOYNI_HD uint32_t* ext_accum_tile_aggregates(const ExtAccumArgs& a, uint32_t col) { return a.tiles + (uint64_t)col * EXT_ACCUM_TILE_WORDS * a.ntiles; }
TOYNI_HD uint32_t* ext_accum_tile_zeros(const ExtAccumArgs& a, uint32_t col) { return ext_accum_tile_aggregates(a, col) + 4ull * a.ntiles; }

template <int OP> TOYNI_HD Ext4 ext_accum_identity() { return Ext4{{OP == (int)SCAN_PRODUCT ? BB_R1 : 0u, 0u, 0u, 0u}}; }
// a * b, all three in Montgomery form: b becomes the prepared right factor of ext_mul (its multiples of 11 through X^4 = EXT_W_R)
TOYNI_HD Ext4 ext_mul_general(const Ext4& a, const Ext4& b) {
    ExtFactor f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f.b[k] = b.c[k];
        f.b11[k] = k ? mont_mul(b.c[k], EXT_W_R) : 0u;   // ext_mul never reads b11[0]
    }
    return ext_mul(a, f);
}
template <int OP> TOYNI_HD Ext4 ext_accum_combine(const Ext4& a, const Ext4& b) {
    if (OP == (int)SCAN_PRODUCT) return ext_mul_general(a, b);
    Ext4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.c[k] = bb_add(a.c[k], b.c[k]);
    return r;
}
template <int OP> TOYNI_HD Ext4 ext_accum_to_plain(const Ext4& v) {
    if (OP != (int)SCAN_PRODUCT) return v;
    return Ext4{{from_mont(v.c[0]), from_mont(v.c[1]), from_mont(v.c[2]), from_mont(v.c[3])}};
}
// the G elements of an Ext column from i0 on (coordinate columns `stride` apart), each coordinate column as scan_group_load reads it
template <int G>
TOYNI_HD void ext_column_group_load(const uint32_t* col0, uint64_t stride, uint64_t i0, uint64_t n, Ext4 (&v)[G]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t w[G];
        scan_group_load<G>(col0 + (uint64_t)k * stride, i0, n, 0u, w);
#pragma unroll
        for (int j = 0; j < G; ++j) v[j].c[k] = w[j];
    }
}
template <int G>
TOYNI_HD void ext_column_group_store(uint32_t* col0, uint64_t stride, uint64_t i0, uint64_t n, const Ext4 (&v)[G]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t w[G];
#pragma unroll
        for (int j = 0; j < G; ++j) w[j] = v[j].c[k];
        scan_group_store<G>(col0 + (uint64_t)k * stride, i0, n, w);
    }
}
// the G elements of column `col` of an operand from i0 on, plain, the shift added; past n: the shift (width 4, 1) -- never used
template <int G>
TOYNI_HD void ext_accum_operand_load(const ExtAccumOperand& o, uint32_t col, uint64_t i0, uint64_t n, Ext4 (&v)[G]) {
    if (o.width == 4u) {
        ext_column_group_load<G>(o.values + 4ull * col * o.stride, o.stride, i0, n, v);
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[j].c[k] = bb_add(v[j].c[k], o.shift[k]);
    } else if (o.width == 1u) {
        uint32_t w[G];
        scan_group_load<G>(o.values + (uint64_t)col * o.stride, i0, n, 0u, w);
#pragma unroll
        for (int j = 0; j < G; ++j) v[j] = Ext4{{bb_add(w[j], o.shift[0]), o.shift[1], o.shift[2], o.shift[3]}};
    } else {
#pragma unroll
        for (int j = 0; j < G; ++j) v[j] = Ext4{{1u, 0u, 0u, 0u}};
    }
}
// invR[j] = a_j^-1 in Montgomery form (0 for a_j = 0) for G PLAIN Ext elements behind ONE base inversion, through the tower
// F_p < F_p[Y]/(Y^2 - 11) < Ext, Y = X^2:  a = A0 + A1 X with A0 = a0 + a2 Y, A1 = a1 + a3 Y;  B = A0^2 - Y A1^2 = B0 + B1 Y;
// N = B0^2 - 11 B1^2 in F_p;  a^-1 = (A0 - A1 X)(B0 - B1 Y) / N.  N = 0 only for a = 0 (two norms of field extensions).  The G norms
// share the inversion by Montgomery's trick, a zero norm kept out of the chain with the marker of deep_point_inverses.
// The plain coordinates are read as Montgomery forms of a / R, as scan_group_inverses reads its residues: every step is then a
// Montgomery-domain step for a / R, whose inverse a^-1 R in Montgomery form is a^-1 R^2; the one from_mont of the inverted product
// takes that R back out of all G results.
template <int G>
TOYNI_HD void ext_tower_inverses(const Ext4 (&a)[G], uint32_t (&invR)[G][4]) {
    uint32_t b0[G], b1[G], dR[G], pre[G];
    uint32_t acc = BB_R1;
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const uint32_t a2w = mont_mul(a[j].c[2], EXT_W_R), a3w = mont_mul(a[j].c[3], EXT_W_R);   // 11 a2, 11 a3
        const uint32_t t13 = mont_mul(a[j].c[1], a3w), t02 = mont_mul(a[j].c[0], a[j].c[2]);
        b0[j] = bb_sub(mont_dot2(a[j].c[0], a[j].c[0], a[j].c[2], a2w), bb_add(t13, t13));       // a0^2 + 11 a2^2 - 22 a1 a3
        b1[j] = bb_sub(bb_add(t02, t02), mont_dot2(a[j].c[1], a[j].c[1], a[j].c[3], a3w));       // 2 a0 a2 - a1^2 - 11 a3^2
        dR[j] = bb_sub(mont_mul(b0[j], b0[j]), mont_mul(mont_mul(b1[j], b1[j]), EXT_W_R));       // N
        if (dR[j] == 0u) dR[j] = BB_R1 | 0x80000000u;                                            // marker (never a canonical value)
        pre[j] = acc;
        acc = mont_mul(acc, (dR[j] & 0x80000000u) ? BB_R1 : dR[j]);
    }
    uint32_t inv = from_mont(mont_inv(acc));
#pragma unroll
    for (int j = G - 1; j >= 0; --j) {
        const bool zero = (dR[j] & 0x80000000u) != 0u;
        const uint32_t ni = zero ? 0u : mont_mul(inv, pre[j]);
        if (!zero) inv = mont_mul(inv, dR[j]);
        const uint32_t c0 = mont_mul(b0[j], ni), c1 = mont_mul(bb_sub(0u, b1[j]), ni);           // (B0 - B1 Y) / N
        const uint32_t c1w = mont_mul(c1, EXT_W_R);
        invR[j][0] = mont_dot2(a[j].c[0], c0, a[j].c[2], c1w);                                 // A0 C
        invR[j][2] = mont_dot2(a[j].c[0], c1, a[j].c[2], c0);
        invR[j][1] = bb_sub(0u, mont_dot2(a[j].c[1], c0, a[j].c[3], c1w));                     // -A1 C
        invR[j][3] = bb_sub(0u, mont_dot2(a[j].c[1], c1, a[j].c[3], c0));
    }
}
TOYNI_HD uint32_t ext_is_zero(const Ext4& v) { return (v.c[0] | v.c[1] | v.c[2] | v.c[3]) == 0u ? 1u : 0u; }
// the inverses of column `col`'s G denominators from i0 on, in Montgomery form (0 for a zero denominator); returns the zeros below n.
// An inverse is zero only where the denominator is (a field), so the zeros are read off the results.
template <int G>
TOYNI_HD uint32_t ext_accum_group_inverses(const ExtAccumArgs& a, uint32_t col, uint64_t i0, uint64_t n, Ext4 (&invR)[G]) {
    uint32_t r[G][4];   // both forms write the one array
    if (a.den.width == 1u) {   // gamma + v_i for a base column: the norm form of 3h with the column's values as points
        uint32_t xR[G];
        scan_group_load<G>(a.den.values + (uint64_t)col * a.den.stride, i0, n, 0u, xR);
#pragma unroll
        for (int j = 0; j < G; ++j) xR[j] = to_mont(xR[j]);
        ext_shifted_inverses<G>(a.den_inv, xR, r);
    } else {
        Ext4 d[G];
        ext_accum_operand_load<G>(a.den, col, i0, n, d);
        ext_tower_inverses<G>(d, r);
    }
    uint32_t zeros = 0;
#pragma unroll
    for (int j = 0; j < G; ++j) {
        invR[j] = Ext4{{r[j][0], r[j][1], r[j][2], r[j][3]}};
        zeros += i0 + (uint64_t)j < n ? ext_is_zero(invR[j]) : 0u;
    }
    return zeros;
}
// the G terms num / den of column `col` from i0 on in the form the op scans (plain for a sum, Montgomery forms for a product); the
// identity past n.  Returns the zero denominators met below n.
template <int OP, int G>
TOYNI_HD uint32_t ext_accum_group_terms(const ExtAccumArgs& a, uint32_t col, uint64_t i0, uint64_t n, Ext4 (&t)[G]) {
    constexpr bool PROD = OP == (int)SCAN_PRODUCT;
    uint32_t zeros = 0;
    if (a.den.width != 0u) {
        Ext4 invR[G];
        zeros = ext_accum_group_inverses<G>(a, col, i0, n, invR);
        if (a.num.width != 0u) {
            ext_accum_operand_load<G>(a.num, col, i0, n, t);
#pragma unroll
            for (int j = 0; j < G; ++j) {
                if (PROD) t[j] = Ext4{{to_mont(t[j].c[0]), to_mont(t[j].c[1]), to_mont(t[j].c[2]), to_mont(t[j].c[3])}};
                t[j] = ext_mul_general(t[j], invR[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j) t[j] = PROD ? invR[j] : Ext4{{from_mont(invR[j].c[0]), from_mont(invR[j].c[1]), from_mont(invR[j].c[2]), from_mont(invR[j].c[3])}};
        }
    } else {
        ext_accum_operand_load<G>(a.num, col, i0, n, t);
        if (PROD) {
#pragma unroll
            for (int j = 0; j < G; ++j) t[j] = Ext4{{to_mont(t[j].c[0]), to_mont(t[j].c[1]), to_mont(t[j].c[2]), to_mont(t[j].c[3])}};
        }
    }
#pragma unroll
    for (int j = 0; j < G; ++j)
        if (i0 + (uint64_t)j >= n) t[j] = ext_accum_identity<OP>();
    return zeros;
}
// thread-serial part: ex[j] = t[0] o ... o t[j-1]; returns the group's total
template <int OP, int G>
TOYNI_HD Ext4 ext_accum_thread_serial(const Ext4 (&t)[G], Ext4 (&ex)[G]) {
    Ext4 acc = ext_accum_identity<OP>();
#pragma unroll
    for (int j = 0; j < G; ++j) {
        ex[j] = acc;
        acc = ext_accum_combine<OP>(acc, t[j]);
    }
    return acc;
}
// from the waves' totals (LDS, 16 bytes per wave): what the waves below `wave` combine to; `total` = all of them
template <int OP, int NW>
TOYNI_HD Ext4 ext_accum_waves_below(const Ext4* wave_tot, uint32_t wave, Ext4& total) {
    Ext4 pre = ext_accum_identity<OP>();
    total = ext_accum_identity<OP>();
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if ((uint32_t)w == wave) pre = total;
        total = ext_accum_combine<OP>(total, wave_tot[w]);
    }
    return pre;
}
// what step 3 stores: base o ex[j], as plain residues
template <int OP, int G>
TOYNI_HD void ext_accum_group_finish(const Ext4& base, const Ext4 (&ex)[G], Ext4 (&o)[G]) {
#pragma unroll
    for (int j = 0; j < G; ++j) o[j] = ext_accum_to_plain<OP>(ext_accum_combine<OP>(base, ex[j]));
}
// out_j = in_j^-1 (0 for 0), plain in and out, for the G elements of one Ext column from i0 on; returns the zeros below `count`
template <int G>
TOYNI_HD uint32_t ext_invert_group(const uint32_t* in, uint64_t in_stride, uint32_t* out, uint64_t out_stride, uint64_t i0, uint64_t count) {
    Ext4 v[G];
    uint32_t invR[G][4];
    ext_column_group_load<G>(in, in_stride, i0, count, v);
    ext_tower_inverses<G>(v, invR);
    uint32_t zeros = 0;
#pragma unroll
    for (int j = 0; j < G; ++j) {
        v[j] = Ext4{{from_mont(invR[j][0]), from_mont(invR[j][1]), from_mont(invR[j][2]), from_mont(invR[j][3])}};
        zeros += i0 + (uint64_t)j < count ? ext_is_zero(v[j]) : 0u;
    }
    ext_column_group_store<G>(out, out_stride, i0, count, v);
    return zeros;
}

// ---- polynomial evaluation at up to POLY_MAX_POINTS points ----
constexpr int POLY_MAX_POINTS = 4;
constexpr uint32_t POLY_PER_THREAD = 16, POLY_THREADS = 256, POLY_CHUNK = POLY_PER_THREAD * POLY_THREADS;
struct PolyEvalArgs {
    const uint32_t* coeffs;
    uint64_t ncoeffs;
    uint32_t npoints;
    uint32_t zR[POLY_MAX_POINTS];        // points, Montgomery form
    uint32_t z16R[POLY_MAX_POINTS];      // z^16
    uint32_t zchunkR[POLY_MAX_POINTS];   // z^POLY_CHUNK
    uint32_t* partial;                   // [blocks][npoints]: sum over the block's chunk of c_i z^(i - chunk start)
    uint32_t* out;                       // [npoints]
    uint32_t nblocks;
};
// the 16 coefficients of one thread: sum_j c_j z^j by Horner (src/math/polynomial.rs:139-142 on a run of 16), then times z^(16 t)
TOYNI_HD uint32_t poly_thread_term(const PolyEvalArgs& a, uint32_t p, const uint32_t (&c)[POLY_PER_THREAD], uint32_t t) {
    uint32_t r = c[POLY_PER_THREAD - 1];
#pragma unroll
    for (int j = (int)POLY_PER_THREAD - 2; j >= 0; --j) r = bb_add(mont_mul(r, a.zR[p]), c[j]);
    return mont_mul(r, mont_pow(a.z16R[p], t));
}

// The same for `batch` coefficient vectors `stride` words apart (include/toyni_hip.h 3e): stage 1 runs one block per (chunk, column),
// stage 2 one block per column.  e.coeffs is column 0, e.partial holds [column][chunk][point], e.out holds [column][point].
struct PolyBatchArgs {
    PolyEvalArgs e;
    uint64_t stride;
    uint32_t batch;
};
TOYNI_HD void poly_batch_load(const PolyBatchArgs& a, uint32_t col, uint32_t chunk, uint32_t t, uint32_t (&c)[POLY_PER_THREAD]) {
    const uint32_t* src = a.e.coeffs + (uint64_t)col * a.stride;
    const uint64_t base = (uint64_t)chunk * POLY_CHUNK + (uint64_t)t * POLY_PER_THREAD;
#pragma unroll
    for (uint32_t j = 0; j < POLY_PER_THREAD; ++j) c[j] = base + j < a.e.ncoeffs ? src[base + j] : 0u;
}
TOYNI_HD uint64_t poly_batch_partial_index(const PolyBatchArgs& a, uint32_t col, uint32_t chunk, uint32_t p) {
    return ((uint64_t)col * a.e.nblocks + chunk) * a.e.npoints + p;
}
// stage 2, thread t of nthreads: its share of sum_chunk partial[col][chunk][p] * (z^POLY_CHUNK)^chunk
TOYNI_HD uint32_t poly_batch_final_thread(const PolyBatchArgs& a, uint32_t col, uint32_t p, uint32_t t, uint32_t nthreads) {
    uint32_t acc = 0;
    for (uint32_t b = t; b < a.e.nblocks; b += nthreads)
        acc = bb_add(acc, mont_mul(a.e.partial[poly_batch_partial_index(a, col, b, p)], mont_pow(a.e.zchunkR[p], b)));
    return acc;
}

// The same at Ext points (include/toyni_hip.h 3h): base coefficients, Ext values.  Every product is an ext_mul by a factor the host
// prepared: the Horner step by the point itself, the powers z^(16 t) and (z^POLY_CHUNK)^chunk from a table of squarings that rides in
// the kernel arguments (one bit of the thread's or chunk's index per entry).
constexpr int POLY_EXT_BITS = 8;                 // POLY_THREADS = 2^8: the bits of a thread's index, and of a chunk's index within a stride
static_assert((1u << POLY_EXT_BITS) == POLY_THREADS, "one squaring per bit of the thread index");
struct PolyExtPowers {
    ExtFactor step;                              // stage 1: z                  stage 2: (z^POLY_CHUNK)^POLY_THREADS
    ExtFactor sq[POLY_EXT_BITS];                 // stage 1: (z^16)^(2^i)       stage 2: (z^POLY_CHUNK)^(2^i)
};
inline PolyExtPowers poly_ext_powers_host(const uint32_t step[4], const uint32_t base[4]) {
    PolyExtPowers pw;
    pw.step = ext_factor_host(step);
    uint32_t s[4] = {base[0], base[1], base[2], base[3]};
    for (int i = 0; i < POLY_EXT_BITS; ++i) { pw.sq[i] = ext_factor_host(s); ext_mul_host(s, s, s); }
    return pw;
}
struct PolyExtArgs {
    const uint32_t* coeffs;                      // column 0; column b starts b * stride words on
    uint64_t ncoeffs, stride;
    uint32_t batch, npoints, nblocks;
    uint32_t* partial;                           // [column][chunk][point][4]
    uint32_t* out;                               // [column][point][4]
    PolyExtPowers thread[POLY_MAX_POINTS], chunk[POLY_MAX_POINTS];
};
// (the shape fields are read through a template: the device-record twins of 3o carry them in a PolyExtDzArgs, dz_kernels.hpp)
template <class Args>
TOYNI_HD void poly_ext_load(const Args& a, uint32_t col, uint32_t chunk, uint32_t t, uint32_t (&c)[POLY_PER_THREAD]) {
    const uint32_t* src = a.coeffs + (uint64_t)col * a.stride;
    const uint64_t base = (uint64_t)chunk * POLY_CHUNK + (uint64_t)t * POLY_PER_THREAD;
#pragma unroll
    for (uint32_t j = 0; j < POLY_PER_THREAD; ++j) c[j] = base + j < a.ncoeffs ? src[base + j] : 0u;
}
template <class Args>
TOYNI_HD uint64_t poly_ext_partial_index(const Args& a, uint32_t col, uint32_t chunk, uint32_t p) {
    return (((uint64_t)col * a.nblocks + chunk) * a.npoints + p) * 4u;
}
// r * base^e for e < POLY_THREADS, base^(2^i) = pw.sq[i]
TOYNI_HD Ext4 poly_ext_times_power(const PolyExtPowers& pw, Ext4 r, uint32_t e) {
#pragma unroll
    for (int i = 0; i < POLY_EXT_BITS; ++i)
        if ((e >> i) & 1u) r = ext_mul(r, pw.sq[i]);
    return r;
}
// the 16 coefficients of one thread: sum_j c_j z^j by Horner (the coefficient enters coordinate 0), then times z^(16 t)
TOYNI_HD Ext4 poly_ext_thread_term(const PolyExtPowers& pw, const uint32_t (&c)[POLY_PER_THREAD], uint32_t t) {
    Ext4 r = {{c[POLY_PER_THREAD - 1], 0u, 0u, 0u}};
#pragma unroll
    for (int j = (int)POLY_PER_THREAD - 2; j >= 0; --j) {
        r = ext_mul(r, pw.step);
        r.c[0] = bb_add(r.c[0], c[j]);
    }
    return poly_ext_times_power(pw, r, t);
}
TOYNI_HD Ext4 poly_ext_thread_term(const PolyExtArgs& a, uint32_t p, const uint32_t (&c)[POLY_PER_THREAD], uint32_t t) {
    return poly_ext_thread_term(a.thread[p], c, t);
}
// stage 2, thread t of POLY_THREADS: its share of sum_chunk partial[col][chunk][p] * (z^POLY_CHUNK)^chunk -- the chunks t, t + 256, ...
// by Horner in (z^POLY_CHUNK)^256 from the last one down, then times (z^POLY_CHUNK)^t
template <class Args>
TOYNI_HD Ext4 poly_ext_final_thread(const Args& a, const PolyExtPowers& pw, uint32_t col, uint32_t p, uint32_t t) {
    Ext4 r = {{0u, 0u, 0u, 0u}};
    if (t >= a.nblocks) return r;
    for (uint32_t k = (a.nblocks - 1u - t) / POLY_THREADS + 1u; k-- > 0u;) {
        const uint32_t* w = a.partial + poly_ext_partial_index(a, col, t + k * POLY_THREADS, p);
        r = ext_mul(r, pw.step);
#pragma unroll
        for (int q = 0; q < 4; ++q) r.c[q] = bb_add(r.c[q], w[q]);
    }
    return poly_ext_times_power(pw, r, t);
}
TOYNI_HD Ext4 poly_ext_final_thread(const PolyExtArgs& a, uint32_t col, uint32_t p, uint32_t t) {
    return poly_ext_final_thread(a, a.chunk[p], col, p, t);
}

// ---- one output of an Ext FRI round that commits what it folds (include/toyni_hip.h 3j) ----
// fold_ext_one, then the row leaf of the folded element -- 00 || salt(16) || Ext::to_bytes(32): width 4, ONE SHA-256 block either way
// (12 or 8 data words + padding + length) -- hashed from the registers the fold left it in.  `salt_words`: 4 LE words when SALTED,
// not read otherwise.  What fri_fold_ext_commit_kernel runs per thread, and what tests/emu steps on the CPU.
struct FoldExtLeaf { Ext4 folded; Digest leaf; };
template <bool SALTED>
TOYNI_HD FoldExtLeaf fold_ext_commit_one(const Ext4& a, const Ext4& b, uint32_t scaleR, const ExtFactor& beta_half, const uint32_t* salt_words) {
    FoldExtLeaf r;
    r.folded = fold_ext_one(a, b, scaleR, beta_half);
    const Ext4 v = r.folded;
    r.leaf = merkle_row_leaf<SALTED>(4u, salt_words, [&v](int, uint32_t (&c)[8]) {   // the one chunk: columns 0 .. 3, the rest ignored
        c[0] = v.c[0]; c[1] = v.c[1]; c[2] = v.c[2]; c[3] = v.c[3];
    });
    return r;
}

// ---- one LEAF of a four-to-one Ext FRI round that commits what it folds (include/toyni_hip.h 3m) ----
// The folded layer L'' (m / 4 elements) is committed under coset leaves: leaf t < m / 16 holds L''[t + q m/16], q = 0 .. 3, and
//   L''[j] = fold( fold(L[j], L[j + m/2]; s, beta), fold(L[j + m/4], L[j + 3m/4]; s / I, beta); s^2, beta^2 ),  s = 1 / (x0 w_m^j),
// I = w_m^(m/4) = w_4: the two pairwise rounds of fri_fold_ext on the points x0 w_m^i and x0^2 w_(m/2)^i, in registers.
//   in[q + 4 r] = L[t + q m/16 + r m/4]       the 16 elements one leaf depends on (stride m / 16 in memory)
//   sR[q]       = Montgomery form of 1 / (x0 w_m^(t + q m/16))
//   iinvR       = Montgomery form of 1 / w_4
//   f1, f2      = ExtFactor of beta / 2 and of beta^2 / 2
// 12 fold_ext_one; then the coset leaf 00 || salt(16) || four Ext::to_bytes: the row leaf of width 16, three SHA-256 blocks either
// way, hashed from the 16 folded words.  Every array index is a constant: the chunk loader below selects, it does not index.
// What fri_fold4_ext_commit_kernel runs per thread, and what tests/emu steps on the CPU.
struct Fold4ExtLeaf { Ext4 folded[4]; Digest leaf; };
template <bool SALTED>
TOYNI_HD Fold4ExtLeaf fold4_ext_commit_leaf(const Ext4 (&in)[16], const uint32_t (&sR)[4], uint32_t iinvR, const ExtFactor& f1, const ExtFactor& f2,
                                            const uint32_t* salt_words) {
    Fold4ExtLeaf r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const Ext4 u = fold_ext_one(in[q], in[q + 8], sR[q], f1);
        const Ext4 v = fold_ext_one(in[q + 4], in[q + 12], mont_mul(sR[q], iinvR), f1);
        r.folded[q] = fold_ext_one(u, v, mont_mul(sR[q], sR[q]), f2);
    }
    const Ext4 e0 = r.folded[0], e1 = r.folded[1], e2 = r.folded[2], e3 = r.folded[3];
    r.leaf = merkle_row_leaf<SALTED>(16u, salt_words, [&](int j, uint32_t (&c)[8]) {   // chunk 0: elements 0 and 1; chunk 1: 2 and 3
        const Ext4& lo = j == 0 ? e0 : e2;
        const Ext4& hi = j == 0 ? e1 : e3;
#pragma unroll
        for (int k = 0; k < 4; ++k) { c[k] = lo.c[k]; c[4 + k] = hi.c[k]; }
    });
    return r;
}

// The record a round of the four-to-one phase leaves for the next fold: two ExtFactors, of beta / 2 and of beta^2 / 2 (16 words).
// beta: plain canonical coordinates; half_r2 / half11_r2 = (1 / 2) R^2 and (11 / 2) R^2 as in the two-to-one phase, eleven_r2 =
// 11 R^2.  beta^2 is ONE Ext product of the canonical beta by its own factor table (Montgomery forms of beta and 11 beta).
TOYNI_HD void fri4_round_record(const uint32_t (&beta)[4], uint32_t half_r2, uint32_t half11_r2, uint32_t eleven_r2, ExtFactor (&rec)[2]) {
    ExtFactor fb;
    Ext4 b;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b.c[k] = beta[k];
        fb.b[k] = mont_mul(beta[k], BB_R2);
        fb.b11[k] = mont_mul(beta[k], eleven_r2);
        rec[0].b[k] = mont_mul(beta[k], half_r2);
        rec[0].b11[k] = mont_mul(beta[k], half11_r2);
    }
    const Ext4 sq = ext_mul(b, fb);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        rec[1].b[k] = mont_mul(sq.c[k], half_r2);
        rec[1].b11[k] = mont_mul(sq.c[k], half11_r2);
    }
}

// ---- Merkle openings (src/merkle.rs:50-80, src/fibonacci.rs:366-375) ----
// record of one opening: depth x 32 path bytes | 16 salt bytes (zero when unsalted) | value as 8 LE bytes | depth position bytes
// (1 = the sibling is the LEFT input of the node hash), padding zero to a multiple of 8
TOYNI_HD uint32_t merkle_depth(uint64_t n) {
    uint32_t d = 0;
    while (n > 1) { n = (n + 1) / 2; ++d; }
    return d;
}
TOYNI_HD uint64_t merkle_open_record_bytes(uint64_t n) {
    const uint32_t d = merkle_depth(n);
    return (uint64_t)d * 32u + 24u + ((d + 7u) & ~7u);
}
// sibling row (index into the flat level array) and position flag of level `level` for leaf `index`
TOYNI_HD uint64_t merkle_sibling_row(uint64_t n, uint64_t index, uint32_t level, bool& is_left) {
    uint64_t off = 0, m = n, cur = index;
    for (uint32_t l = 0; l < level; ++l) { off += m; m = (m + 1) / 2; cur >>= 1; }
    const uint64_t sib = (cur & 1u) ? cur - 1 : cur + 1;
    if (sib >= m) { is_left = true; return off + cur; }   // last node of an odd level: paired with itself (src/merkle.rs:67-70)
    is_left = (cur & 1u) != 0;
    return off + sib;
}


// ---- salts: a ChaCha20 keystream (RFC 8439 2.3: constants | key | 32-bit block counter | 96-bit nonce, 20 rounds) ----
// The reference salts every Merkle leaf with 16 bytes of `rand::thread_rng()` (src/fibonacci.rs:341-343), a ChaCha-based CSPRNG
// on the host; a device-resident prover wants them where the leaves are hashed instead of 130 MB over PCIe per proof.  One block
// = 64 bytes = the salts of four leaves.
TOYNI_HD uint32_t chacha_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
TOYNI_HD void chacha20_block(const uint32_t key[8], uint32_t counter, const uint32_t nonce[3], uint32_t out[16]) {
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                      counter, nonce[0], nonce[1], nonce[2]};
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = s[i];
#define TOYNI_QR(a, b, c, d)                                      \
    x[a] += x[b]; x[d] = chacha_rotl(x[d] ^ x[a], 16);            \
    x[c] += x[d]; x[b] = chacha_rotl(x[b] ^ x[c], 12);            \
    x[a] += x[b]; x[d] = chacha_rotl(x[d] ^ x[a], 8);             \
    x[c] += x[d]; x[b] = chacha_rotl(x[b] ^ x[c], 7)
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        TOYNI_QR(0, 4, 8, 12); TOYNI_QR(1, 5, 9, 13); TOYNI_QR(2, 6, 10, 14); TOYNI_QR(3, 7, 11, 15);
        TOYNI_QR(0, 5, 10, 15); TOYNI_QR(1, 6, 11, 12); TOYNI_QR(2, 7, 8, 13); TOYNI_QR(3, 4, 9, 14);
    }
#undef TOYNI_QR
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = x[i] + s[i];   // little-endian words = the keystream bytes on this (little-endian) target
}

}  // namespace toyni
