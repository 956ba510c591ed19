// What depends on the out-of-domain point z, prepared on the device (include/toyni_hip.h 3o).
//
// The host-argument calls of 3h expand z and the DEEP weights on the host (ext_pow_host, poly_ext_powers_host, ext_shift_host, the
// claim sum, the Montgomery forms) and pass the result in the kernel arguments.  Here z, the weights and the claimed values are words
// of device memory that the host never sees, so a ONE-WAVE kernel expands them into a record in the stream's buffer and the hot
// kernels read the record.  Every function below produces, word for word, what the host code produces for the same canonical
// values: all of it is exact arithmetic mod p and every stored word is a canonical residue or a canonical Montgomery form.
// Every word read from device memory is reduced first (dz_reduce: BabyBear::new), so the operand domains of bb_field.hpp hold
// whatever arrives.  Plain C++ so tests/emu can step it; the transcript helpers of 3o are here too.
#pragma once
#include "prover_kernels.hpp"
#include "transcript_kernels.hpp"

namespace toyni {

// any u32 -> its canonical residue: a Montgomery product takes any u32 on the left, and w * R / R = w mod p
TOYNI_HD uint32_t dz_reduce(uint32_t w) { return mont_mul(w, BB_R1); }
TOYNI_HD Ext4 dz_load_ext(const uint32_t* src) { return Ext4{{dz_reduce(src[0]), dz_reduce(src[1]), dz_reduce(src[2]), dz_reduce(src[3])}}; }
// ext_factor_host on the device: plain canonical coordinates -> their Montgomery forms and those of 11 times them
TOYNI_HD ExtFactor ext_factor_dev(const Ext4& v) {
    ExtFactor f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f.b[k] = to_mont(v.c[k]);
        f.b11[k] = mont_mul(f.b[k], EXT_W_R);
    }
    return f;
}

// ---- the out-of-domain point (derive_z of the harness protocol): four challenges, again while z1 = z2 = z3 = 0 ----
// The accept predicate is a macro, as pow_stop's is, so that a CPU test can make the rejection branch and the bound run.
#ifndef TOYNI_DZ_POINT_ACCEPT
#define TOYNI_DZ_POINT_ACCEPT(z) (((z)[1] | (z)[2] | (z)[3]) != 0u)
#endif
constexpr uint32_t DZ_POINT_TRIES = 8;   // a rejection has probability p^-3: the bound only keeps ANY input from spinning
// One thread.  Accepted: z and the state after the last squeeze.  Not within DZ_POINT_TRIES, or a status already set: zeros, the state
// as it was (and TRANSCRIPT_E_RANGE in the first case).
TOYNI_HD void transcript_squeeze_ext_point(TranscriptState& tr, uint32_t* z) {
    const uint32_t len = tr.len, status = tr.status;
    bool ok = false;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    TranscriptChain c{Digest{}, false};
    if (status == 0u && len <= TRANSCRIPT_CAPACITY) {
        for (uint32_t tries = 0; tries < DZ_POINT_TRIES && !ok; ++tries) {
            for (int k = 0; k < 4; ++k) {
                transcript_step(tr, len, c);
                v[k] = bb_reduce_u64(transcript_value(c.d));
            }
            ok = TOYNI_DZ_POINT_ACCEPT(v);
        }
    }
    for (int k = 0; k < 4; ++k) z[k] = ok ? v[k] : 0u;
    if (ok) transcript_store_digest(tr, c.d);
    else if (status == 0u) tr.status = TRANSCRIPT_E_RANGE;
}

// ---- absorb_field for `count` words of device memory: 8 little-endian bytes of the canonical residue each ----
constexpr uint32_t TRANSCRIPT_MAX_FIELDS = TRANSCRIPT_CAPACITY / 8u;
// the lanes of one wave share the words; every lane reads length and status before lane 0 stores either (transcript_absorb_wave)
TOYNI_HD void transcript_absorb_fields_wave(TranscriptState& tr, const uint32_t* words, uint32_t count, uint32_t lane, uint32_t nlanes) {
    const uint32_t len = tr.len, status = tr.status;
    TOYNI_WAVE_ORDER();
    if (status != 0u) return;
    if (count > TRANSCRIPT_MAX_FIELDS || !transcript_fits(len, 8u * count)) {
        if (lane == 0u) tr.status = TRANSCRIPT_E_RANGE;
        return;
    }
    for (uint32_t i = lane; i < count; i += nlanes) {
        const uint32_t w = dz_reduce(words[i]);
        uint8_t* dst = tr.bytes + len + 8u * i;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            dst[k] = (uint8_t)(w >> (8u * k));
            dst[4u + k] = 0u;
        }
    }
    if (lane == 0u) tr.len = len + 8u * count;
}

// ---- the rows a matrix with next-row terms opens per query ----
constexpr uint32_t QUERY_ROWS_MAX_OFFSETS = 8;
struct QueryRowOffsets { uint32_t v[QUERY_ROWS_MAX_OFFSETS]; };
// item t of count x noffsets: (indices[t / noffsets] + offsets[t mod noffsets]) mod n, the sum in 64 bits (n <= 2^32)
TOYNI_HD uint32_t query_row(const uint32_t* indices, const QueryRowOffsets& off, uint32_t noffsets, uint64_t n, uint64_t t) {
    return (uint32_t)(((uint64_t)indices[t / noffsets] + off.v[t % noffsets]) % n);
}

// ---- the powers of the evaluation points mults[p] * z ----
// One chain of squarings per point serves all four things the host computes with three ext_pow_host and two poly_ext_powers_host:
// with s_i = point^(2^i), z^16 = s_4, z^POLY_CHUNK = s_12, (z^POLY_CHUNK)^POLY_THREADS = s_20, and the two tables of squarings are
// s_4 .. s_11 and s_12 .. s_19: 20 dependent Ext products.
constexpr int POLY_LOG_PER_THREAD = 4, POLY_LOG_CHUNK = POLY_LOG_PER_THREAD + POLY_EXT_BITS;
static_assert((1u << POLY_LOG_PER_THREAD) == POLY_PER_THREAD && (1u << POLY_LOG_CHUNK) == POLY_CHUNK, "the exponents of the chain");
struct alignas(16) PolyExtRecord { PolyExtPowers thread[POLY_MAX_POINTS], chunk[POLY_MAX_POINTS]; };
struct PolyDzMults { uint32_t v[POLY_MAX_POINTS]; };   // canonical base-field multipliers (host-checked)
TOYNI_HD void poly_ext_record_point(const uint32_t* z, uint32_t mult, PolyExtPowers& thread, PolyExtPowers& chunk) {
    const uint32_t mR = to_mont(mult);
    Ext4 s;
#pragma unroll
    for (int k = 0; k < 4; ++k) s.c[k] = mont_mul(dz_reduce(z[k]), mR);
    for (int i = 0; i <= POLY_LOG_CHUNK + POLY_EXT_BITS; ++i) {
        const ExtFactor f = ext_factor_dev(s);
        if (i == 0) thread.step = f;
        if (i >= POLY_LOG_PER_THREAD && i < POLY_LOG_CHUNK) thread.sq[i - POLY_LOG_PER_THREAD] = f;
        if (i >= POLY_LOG_CHUNK && i < POLY_LOG_CHUNK + POLY_EXT_BITS) chunk.sq[i - POLY_LOG_CHUNK] = f;
        if (i == POLY_LOG_CHUNK + POLY_EXT_BITS) chunk.step = f;
        else s = ext_mul(s, f);
    }
}
// the argument-fed stages' PolyExtArgs without the two tables: the twins take the record as a second, read-only argument, so that
// its words are fetched by scalar loads on demand as the kernel arguments are
struct PolyExtDzArgs {
    const uint32_t* coeffs;
    uint64_t ncoeffs, stride;
    uint32_t batch, npoints, nblocks;
    uint32_t* partial;
    uint32_t* out;
};

// ---- what the DEEP combination needs from z, the weights and the claimed values ----
// ext_shift_host on the device.  zeta has order 4, so the conjugates' factors zeta^(j k) are four constants.
constexpr uint32_t EXT_ZETA_R = cx_mulmod(EXT_ZETA, BB_R1), EXT_ZETA2_R = cx_mulmod(cx_powmod(EXT_ZETA, 2), BB_R1),
                   EXT_ZETA3_R = cx_mulmod(cx_powmod(EXT_ZETA, 3), BB_R1);
TOYNI_HD uint32_t ext_zeta_pow_r(int e) { return (e & 3) == 0 ? BB_R1 : (e & 3) == 1 ? EXT_ZETA_R : (e & 3) == 2 ? EXT_ZETA2_R : EXT_ZETA3_R; }
TOYNI_HD uint32_t bb_neg(uint32_t v) { return bb_sub(0u, v); }
TOYNI_HD ExtShift ext_shift_dev(const Ext4& z) {
    Ext4 c[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) c[j].c[k] = mont_mul(z.c[k], ext_zeta_pow_r((j + 1) * k));
    const ExtFactor f2 = ext_factor_dev(c[2]), fz = ext_factor_dev(z);
    const Ext4 c01 = ext_mul(c[0], ext_factor_dev(c[1]));
    Ext4 s01, a[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) s01.c[k] = bb_add(c[0].c[k], c[1].c[k]);
    const Ext4 t = ext_mul(s01, f2), c012 = ext_mul(c01, f2);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a[2].c[k] = bb_neg(bb_add(s01.c[k], c[2].c[k]));   // -(c1 + c2 + c3)
        a[1].c[k] = bb_add(c01.c[k], t.c[k]);              // c1 c2 + (c1 + c2) c3
        a[0].c[k] = bb_neg(c012.c[k]);                     // -c1 c2 c3
    }
    // (x - z)(x^3 + a2 x^2 + a1 x + a0): coordinate 0 of each coefficient (the others cancel)
    uint32_t m[4];
    m[3] = bb_sub(a[2].c[0], z.c[0]);
    m[2] = bb_sub(a[1].c[0], ext_mul(a[2], fz).c[0]);
    m[1] = bb_sub(a[0].c[0], ext_mul(a[1], fz).c[0]);
    m[0] = bb_neg(ext_mul(a[0], fz).c[0]);
    ExtShift s;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) s.adjR[i][k] = to_mont(a[i].c[k]);
#pragma unroll
    for (int i = 0; i < 4; ++i) s.mR[i] = to_mont(m[i]);
    return s;
}
// A term of the caller, sorted by (column, rot) on the host (the sort does not depend on z): where its weight and its claimed value
// lie in the caller's two arrays, in Ext elements
struct DeepExtSlot { uint32_t column, rot, alpha_index, value_index; };
constexpr uint32_t DEEP_EXT_INLINE_SLOTS = 64;
struct DeepExtInlineSlots { DeepExtSlot s[DEEP_EXT_INLINE_SLOTS]; };
// the record: C = sum_t alpha_t value_t (plain) and adj_z / m_z; the term table follows it in memory
struct alignas(16) DeepExtRecord {
    uint32_t claim[4];
    ExtShift shift;
};
static_assert(sizeof(DeepExtRecord) % alignof(DeepExtTerm) == 0, "the table starts where the record ends");
TOYNI_HD DeepExtTerm* deep_ext_record_table(DeepExtRecord* rec) { return reinterpret_cast<DeepExtTerm*>(rec + 1); }
TOYNI_HD const DeepExtTerm* deep_ext_record_table(const DeepExtRecord* rec) { return reinterpret_cast<const DeepExtTerm*>(rec + 1); }
// One wave.  Lane l: the table entries of the slots l, l + nlanes, ... and their share of C, into part[4 l ..] (4 nlanes words the
// whole wave can read: LDS); lane 0 then adds the shares and expands z.
TOYNI_HD void deep_ext_prepare(const DeepExtSlot* slots, uint32_t nslots, const uint32_t* z, const uint32_t* alphas, const uint32_t* claims,
                               DeepExtRecord* rec, uint32_t* part, uint32_t lane, uint32_t nlanes) {
    DeepExtTerm* table = deep_ext_record_table(rec);
    Ext4 acc = {{0u, 0u, 0u, 0u}};
    for (uint32_t t = lane; t < nslots; t += nlanes) {
        const DeepExtSlot sl = slots[t];
        const ExtFactor f = ext_factor_dev(dz_load_ext(alphas + 4ull * sl.alpha_index));
        const Ext4 av = ext_mul(dz_load_ext(claims + 4ull * sl.value_index), f);
        table[t] = DeepExtTerm{sl.column, sl.rot, {f.b[0], f.b[1], f.b[2], f.b[3]}, {0u, 0u}};
#pragma unroll
        for (int k = 0; k < 4; ++k) acc.c[k] = bb_add(acc.c[k], av.c[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) part[4u * lane + k] = acc.c[k];
    TOYNI_WAVE_ORDER();   // the wave's own LDS stores, read back by lane 0 in program order
    if (lane != 0u) return;
    const uint32_t live = nslots < nlanes ? nslots : nlanes;   // the lanes beyond hold zeros
    for (uint32_t l = 1; l < live; ++l)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc.c[k] = bb_add(acc.c[k], part[4u * l + k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) rec->claim[k] = acc.c[k];
    rec->shift = ext_shift_dev(dz_load_ext(z));
}
// the combine kernel's arguments from the record, in registers that are the same in every lane
TOYNI_HD void deep_ext_args_from_record(DeepExtArgs& a, const DeepExtRecord& rec) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a.claim[k] = TOYNI_UNIFORM(rec.claim[k]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) a.shift.adjR[i][k] = TOYNI_UNIFORM(rec.shift.adjR[i][k]);
#pragma unroll
    for (int i = 0; i < 4; ++i) a.shift.mR[i] = TOYNI_UNIFORM(rec.shift.mR[i]);
}

}  // namespace toyni
