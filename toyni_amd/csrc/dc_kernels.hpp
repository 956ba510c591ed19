// The first two challenges of a staged-AIR proof, prepared on the device (include/toyni_hip.h 3p; "dc" = device challenges).
//
// The host-argument calls of 3i and 3k take gamma as toyni_ext_operand.shift (and expand ext_shift_host from it), take gamma again as
// CONST immediates of the constraint program, and take the constraint weights as a host array.  Here gamma and the alphas are words of
// device memory that the host never sees: a ONE-WAVE kernel turns them into a record in the stream's buffer and the hot kernels read
// the record.  Every function below produces, word for word, what the host code produces for the same canonical values
// (ext_shift_host, to_mont_host, the rule of air_ext_weights); every word read from device memory is reduced first (dz_reduce), so
// the operand domains of bb_field.hpp hold whatever arrives.  No lane reads what another lane wrote: there is no barrier and no LDS.
// Plain C++ so tests/emu can step it.
#pragma once
#include "dz_kernels.hpp"

namespace toyni {

// ---- constraint programs with parameters ----
// r[dst] = params[imm]: the one instruction past the set of 3f.  Only toyni_air_program_check_params / _create_params accept it, and
// only the kernel below interprets it.
constexpr uint32_t AIR_OP_PARAM = 8, AIR_MAX_PARAMS = 256;
static_assert(AIR_OP_PARAM == AIR_OP_COUNT, "the first op the checks of 3f refuse");
constexpr uint32_t AIR_WEIGHTS_EXT = 0, AIR_WEIGHTS_EMIT_EXT = 1;
constexpr uint32_t AIR_DC_MAX_WEIGHTS = 65536;

// The record of one call: nparams Montgomery forms, then 4 x nweights plain canonical weight words (the layout of weights4 in 3k).
TOYNI_HD uint32_t air_dc_nweights(uint32_t nalphas, uint32_t form) { return form == AIR_WEIGHTS_EMIT_EXT ? 4u * nalphas : nalphas; }
TOYNI_HD size_t air_dc_record_words(uint32_t nparams, uint32_t nalphas, uint32_t form) { return (size_t)nparams + 4u * (size_t)air_dc_nweights(nalphas, form); }
// alpha * X^j in F_p[X]/(X^4 - 11): the coordinates move up by j, those that wrap past X^3 times 11 (air_ext_weights);
// a11 = 11 alpha, plain (mont_mul of a plain residue by the Montgomery form of 11)
TOYNI_HD void air_dc_emit_ext_weights(const Ext4& a, uint32_t* w16) {
    uint32_t a11[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) a11[e] = mont_mul(a.c[e], EXT_W_R);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) w16[4 * j + ((e + j) & 3)] = e + j >= 4 ? a11[e] : a.c[e];
}
// One wave; the lanes stride over the parameters and over the alphas, and every lane writes words no other lane touches.
TOYNI_HD void air_dc_prepare(const uint32_t* params, uint32_t nparams, const uint32_t* alphas, uint32_t nalphas, uint32_t form, uint32_t* rec,
                             uint32_t lane, uint32_t nlanes) {
    for (uint32_t j = lane; j < nparams; j += nlanes) rec[j] = to_mont(dz_reduce(params[j]));
    uint32_t* w = rec + nparams;
    for (uint32_t k = lane; k < nalphas; k += nlanes) {
        const Ext4 a = dz_load_ext(alphas + 4ull * k);
        if (form == AIR_WEIGHTS_EMIT_EXT) {
            air_dc_emit_ext_weights(a, w + 16ull * k);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) w[4ull * k + e] = a.c[e];
        }
    }
}
// air_eval_group_ext with the weights AND the parameters in a record that nothing in the kernel writes: every word of it is fetched
// where it is used, through the constant address space (a scalar load, as an instruction word is).  `params`: Montgomery forms;
// `weights4`: plain.  Everything but EMIT's four loads and the PARAM case is air_eval_group_ext's text, which stays as it is.
template <int K>
TOYNI_HD void air_eval_group_ext_dc(const AirArgs& a, const uint32_t* params, const uint32_t* weights4, uint32_t* regs, uint32_t stride, uint64_t i0,
                                    const uint32_t (&zhR)[K], uint32_t (&c)[4][K], uint32_t (&q)[4][K]) {
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
            for (int e = 0; e < 4; ++e) wt[e] = TOYNI_UNIFORM_LOAD(weights4 + 4u * imm + e);
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
        if (op == AIR_OP_PARAM) {
            const uint32_t pv = TOYNI_UNIFORM_LOAD(params + imm);
#pragma unroll
            for (int j = 0; j < K; ++j) v[j] = pv;
        } else if (op >= AIR_OP_ADD) {
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

// ---- the Ext accumulators with gamma in device memory ----
constexpr uint32_t EXT_SHIFT_NONE = 0xffffffffu, EXT_SHIFT_MAX_INDEX = 1u << 20;
// what toyni_column_scan_ext_device derives from its operands' shifts on the host: the shifts themselves (plain), and for a width-1
// denominator adj_z / m_z of z = -shift (zeros otherwise, as ExtAccumArgs{} leaves them)
struct alignas(16) ExtAccumRecord {
    uint32_t num_shift[4], den_shift[4];
    ExtShift den_inv;
};
TOYNI_HD Ext4 ext_accum_dc_shift(const uint32_t* challenges, uint32_t index) {
    return index == EXT_SHIFT_NONE ? Ext4{{0u, 0u, 0u, 0u}} : dz_load_ext(challenges + 4ull * index);
}
// One wave: lane 0 writes the numerator's shift, lane 1 the denominator's and its norm form.  `den_norm`: the denominator has width 1.
TOYNI_HD void ext_accum_dc_prepare(const uint32_t* challenges, uint32_t num_index, uint32_t den_index, uint32_t den_norm, ExtAccumRecord* rec,
                                   uint32_t lane) {
    if (lane == 0u) {
        const Ext4 s = ext_accum_dc_shift(challenges, num_index);
#pragma unroll
        for (int k = 0; k < 4; ++k) rec->num_shift[k] = s.c[k];
    } else if (lane == 1u) {
        const Ext4 s = ext_accum_dc_shift(challenges, den_index);
#pragma unroll
        for (int k = 0; k < 4; ++k) rec->den_shift[k] = s.c[k];
        ExtShift inv{};
        if (den_norm) inv = ext_shift_dev(Ext4{{bb_neg(s.c[0]), bb_neg(s.c[1]), bb_neg(s.c[2]), bb_neg(s.c[3])}});
        rec->den_inv = inv;
    }
}
// the scan kernels' arguments from the record, in registers that are the same in every lane
TOYNI_HD void ext_accum_args_from_record(ExtAccumArgs& a, const ExtAccumRecord& rec) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a.num.shift[k] = TOYNI_UNIFORM(rec.num_shift[k]);
        a.den.shift[k] = TOYNI_UNIFORM(rec.den_shift[k]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) a.den_inv.adjR[i][k] = TOYNI_UNIFORM(rec.den_inv.adjR[i][k]);
#pragma unroll
    for (int i = 0; i < 4; ++i) a.den_inv.mR[i] = TOYNI_UNIFORM(rec.den_inv.mR[i]);
}

}  // namespace toyni
