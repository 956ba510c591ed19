"""Device-resident steps of the Fibonacci prover around the hot path (include/toyni_hip.h 3c): one FRI round with its
commitment, constraint / quotient / DEEP evaluation on the LDE coset, polynomial evaluation at the out-of-domain points, and
Merkle openings.  Mirrors the corresponding lines of `StarkProver::generate_proof` (src/fibonacci.rs:133-150,186-198,222-245,
366-375) as calls on packed-u32 device pointers; no host arithmetic, no CPU path."""
import ctypes

import numpy as np

from ._lib import check, lib


def fri_fold_commit_device(ctx, d_evals: int, d_out: int, m: int, beta: int, x0: int, d_salts: int, d_levels: int, stream: int = 0) -> None:
    """fold a layer of m values and commit the folded layer (all tree levels to d_levels) in one call."""
    check(lib.toyni_fri_fold_commit_device(ctx.handle, d_evals, d_out, m, beta, x0, d_salts or None, d_levels, stream or None),
          "GPU fold + commit failed")


def fri_commit_phase_device(ctx, d_layer0: int, m0: int, x0: int, final_size: int, d_salts: int, challenge, d_layers: int, d_levels: int,
                            stream: int = 0):
    """The fold loop of the commit phase (src/fibonacci.rs:222-245) in one call.  `challenge(round, prev_root: bytes | None,
    want_beta: bool) -> int` is the caller's transcript: absorb prev_root when it is not None, return the squeezed beta when
    want_beta (anything otherwise).  Returns the list of roots (bytes), one per round."""
    def store(beta_ptr, beta):
        beta_ptr[0] = int(beta)

    return _commit_phase(lib.toyni_fri_commit_phase_device, store, ctx, d_layer0, m0, x0, final_size, d_salts, challenge, d_layers, d_levels, stream)


def _commit_phase(entry, store_beta, ctx, d_layer0, m0, x0, final_size, d_salts, challenge, d_layers, d_levels, stream):
    """The commit-phase call of either element type: `entry` the library's loop, `store_beta(beta_ptr, beta)` writes what the
    caller's transcript squeezed (one word, or four)."""
    from ._lib import FRI_CHALLENGE_FN
    failure = []

    def _cb(_user, rnd, root_ptr, beta_ptr):
        try:
            root = bytes(root_ptr[:32]) if root_ptr else None
            beta = challenge(int(rnd), root, bool(beta_ptr))
            if beta_ptr:
                store_beta(beta_ptr, beta)
            return 0
        except BaseException as e:  # noqa: BLE001  (nothing may unwind through the C frames -- KeyboardInterrupt included: ctypes
            failure.append(e)       # would print and swallow it, return 0, and the C loop would go on with beta = 0; re-raised below)
            return 1

    cb = FRI_CHALLENGE_FN(_cb)
    rounds = ctypes.c_uint(0)
    max_rounds = max(0, (m0 // max(final_size, 1)).bit_length() - 1)
    roots = np.zeros(max(max_rounds, 1) * 32, dtype=np.uint8)
    rc = entry(ctx.handle, d_layer0, m0, x0, final_size, d_salts or None, ctypes.cast(cb, ctypes.c_void_p), None,
               d_layers, d_levels, roots.ctypes.data, ctypes.byref(rounds), stream or None)
    if failure:
        raise failure[0]
    check(rc, "GPU FRI commit phase failed")
    return [roots[32 * k:32 * k + 32].tobytes() for k in range(rounds.value)]


def fri_fold_commit_ext_device(ctx, d_evals: int, d_out: int, m: int, beta4, x0: int, d_salts: int, d_levels: int, stream: int = 0) -> None:
    """fold a layer of m Ext elements with the Ext challenge beta4 and commit the folded layer (row leaves of width 4, all tree levels
    to d_levels) in one call (include/toyni_hip.h 3j)."""
    b = np.ascontiguousarray(beta4, dtype=np.uint32)
    assert b.size == 4
    check(lib.toyni_fri_fold_commit_ext_device(ctx.handle, d_evals, d_out, m, b.ctypes.data, x0, d_salts or None, d_levels, stream or None),
          "GPU fold + commit (Ext) failed")


def fri_commit_phase_ext_device(ctx, d_layer0: int, m0: int, x0: int, final_size: int, d_salts: int, challenge, d_layers: int, d_levels: int,
                                stream: int = 0):
    """fri_commit_phase_device over Ext-valued layers: `challenge(round, prev_root: bytes | None, want_beta: bool)` returns four
    ints, the coordinates of the squeezed Ext beta, when want_beta.  Returns the list of roots (bytes), one per round."""
    def store(beta_ptr, beta):
        c = [int(v) for v in beta]
        if len(c) != 4:
            raise ValueError("an Ext challenge has four coordinates")
        for k in range(4):
            beta_ptr[k] = c[k]

    return _commit_phase(lib.toyni_fri_commit_phase_ext_device, store, ctx, d_layer0, m0, x0, final_size, d_salts, challenge, d_layers, d_levels,
                         stream)


def fib_quotient_device(ctx, d_trace_lde: int, d_c_evals: int, d_q_evals: int, log_blowup: int, shift: int, stream: int = 0) -> None:
    check(lib.toyni_fib_quotient_device(ctx.handle, d_trace_lde, d_c_evals or None, d_q_evals, log_blowup, shift, stream or None),
          "GPU constraint / quotient evaluation failed")


def fib_deep_device(ctx, d_trace_lde: int, d_q_evals: int, d_out: int, log_blowup: int, shift: int, z: int, ood, stream: int = 0) -> None:
    o = np.ascontiguousarray(ood, dtype=np.uint32)
    assert o.size == 4
    check(lib.toyni_fib_deep_device(ctx.handle, d_trace_lde, d_q_evals, d_out, log_blowup, shift, z, o.ctypes.data, stream or None),
          "GPU DEEP evaluation failed")


def poly_eval_device(ctx, d_coeffs: int, ncoeffs: int, points, d_out: int, stream: int = 0) -> None:
    p = np.ascontiguousarray(points, dtype=np.uint32)
    check(lib.toyni_poly_eval_device(ctx.handle, d_coeffs, ncoeffs, p.ctypes.data, p.size, d_out, stream or None), "GPU polynomial evaluation failed")


def poly_eval_batch_device(ctx, d_coeffs: int, ncoeffs: int, stride: int, batch: int, points, d_out: int, stream: int = 0) -> None:
    """d_out[b * npoints + p] = column b (d_coeffs + b * stride words) evaluated at points[p]: the out-of-domain values of a whole
    trace in two launches (include/toyni_hip.h 3e)."""
    p = np.ascontiguousarray(points, dtype=np.uint32)
    check(lib.toyni_poly_eval_batch_device(ctx.handle, d_coeffs or None, ncoeffs, stride, batch, p.ctypes.data, p.size, d_out, stream or None),
          "GPU batched polynomial evaluation failed")


class DeepTerm(ctypes.Structure):   # toyni_deep_term (include/toyni_hip.h 3e)
    _fields_ = [("column", ctypes.c_uint32), ("rotation", ctypes.c_uint32), ("alpha", ctypes.c_uint32), ("value", ctypes.c_uint32)]


def deep_terms(columns, rotations, alphas, values):
    """The term table of deep_combine_device: term t weighs column columns[t], read rotations[t] trace rows ahead, by alphas[t]
    against the claimed value values[t]."""
    cols, rots, als, vals = (np.asarray(v, dtype=np.uint32).ravel() for v in (columns, rotations, alphas, values))
    assert cols.size == rots.size == als.size == vals.size
    return (DeepTerm * cols.size)(*[DeepTerm(int(c), int(r), int(a), int(v)) for c, r, a, v in zip(cols, rots, als, vals)])


def deep_combine_device(ctx, d_values: int, width: int, col_stride: int, log_blowup: int, shift: int, z: int, terms, d_out: int,
                        accumulate: bool = False, stream: int = 0) -> None:
    """d_out[i] (+)= sum_t alpha_t (M(column_t, i + rotation_t B) - value_t) / (x_i - z) over a column-major matrix on the LDE coset
    (include/toyni_hip.h 3e).  terms: what deep_terms returns."""
    check(lib.toyni_deep_combine_device(ctx.handle, d_values, width, col_stride, log_blowup, shift, z, terms if len(terms) else None, len(terms),
                                        1 if accumulate else 0, d_out, stream or None), "GPU DEEP combination failed")


def poly_eval_ext_batch_device(ctx, d_coeffs: int, ncoeffs: int, stride: int, batch: int, points4, d_out: int, stream: int = 0) -> None:
    """d_out[(b * npoints + p) * 4 + k] = coordinate k of column b (base-field coefficients) evaluated at the Ext point points4[p]
    (npoints x 4 words): the out-of-domain values under Ext challenges (include/toyni_hip.h 3h)."""
    p = np.ascontiguousarray(points4, dtype=np.uint32).reshape(-1, 4)
    check(lib.toyni_poly_eval_ext_batch_device(ctx.handle, d_coeffs or None, ncoeffs, stride, batch, p.ctypes.data, p.shape[0], d_out, stream or None),
          "GPU batched Ext polynomial evaluation failed")


class DeepExtTerm(ctypes.Structure):   # toyni_deep_ext_term (include/toyni_hip.h 3h)
    _fields_ = [("column", ctypes.c_uint32), ("rotation", ctypes.c_uint32), ("alpha", ctypes.c_uint32 * 4), ("value", ctypes.c_uint32 * 4)]


def deep_ext_terms(columns, rotations, alphas4, values4):
    """The term table of deep_combine_ext_device: term t weighs column columns[t], read rotations[t] trace rows ahead, by the Ext
    weight alphas4[t] against the claimed Ext value values4[t] (four coordinates each)."""
    cols, rots = (np.asarray(v, dtype=np.uint32).ravel() for v in (columns, rotations))
    als, vals = (np.asarray(v, dtype=np.uint32).reshape(-1, 4) for v in (alphas4, values4))
    assert cols.size == rots.size == als.shape[0] == vals.shape[0]
    U4 = ctypes.c_uint32 * 4
    return (DeepExtTerm * cols.size)(*[DeepExtTerm(int(c), int(r), U4(*map(int, a)), U4(*map(int, v))) for c, r, a, v in zip(cols, rots, als, vals)])


def deep_combine_ext_device(ctx, d_values: int, width: int, col_stride: int, log_blowup: int, shift: int, z4, terms, d_out: int,
                            accumulate: bool = False, stream: int = 0) -> None:
    """d_out[4 i .. 4 i + 3] (+)= sum_t alpha_t (M(column_t, i + rotation_t B) - value_t) / (x_i - z) in Ext over a base-field
    column-major matrix on the LDE coset (include/toyni_hip.h 3h).  z4: four coordinates; terms: what deep_ext_terms returns;
    d_out: 16-byte aligned."""
    z = np.ascontiguousarray(z4, dtype=np.uint32)
    assert z.size == 4
    check(lib.toyni_deep_combine_ext_device(ctx.handle, d_values, width, col_stride, log_blowup, shift, z.ctypes.data,
                                            terms if len(terms) else None, len(terms), 1 if accumulate else 0, d_out, stream or None),
          "GPU Ext DEEP combination failed")


# ---- the same two steps with z, the weights and the claimed values in device memory (include/toyni_hip.h 3o) ----
def poly_eval_ext_batch_dz_device(ctx, d_coeffs: int, ncoeffs: int, stride: int, batch: int, d_z: int, mults, d_out: int, stream: int = 0) -> None:
    """poly_eval_ext_batch_device at the points mults[p] * z, z four words at the device pointer d_z; mults: canonical base-field
    multipliers (1, and g for a column that is also opened at g z)."""
    m = np.ascontiguousarray(mults, dtype=np.uint32).ravel()
    check(lib.toyni_poly_eval_ext_batch_dz_device(ctx.handle, d_coeffs or None, ncoeffs, stride, batch, d_z or None, m.ctypes.data, m.size, d_out,
                                                  stream or None), "GPU batched Ext polynomial evaluation (device point) failed")


class DeepExtSlot(ctypes.Structure):   # toyni_deep_ext_slot (include/toyni_hip.h 3o)
    _fields_ = [("column", ctypes.c_uint32), ("rotation", ctypes.c_uint32), ("alpha_index", ctypes.c_uint32), ("value_index", ctypes.c_uint32)]


def deep_ext_slots(columns, rotations, alpha_indices, value_indices):
    """The slot table of deep_combine_ext_dz_device: term t weighs column columns[t], read rotations[t] trace rows ahead, by the Ext
    element alpha_indices[t] of the device array of weights against the Ext element value_indices[t] of the device array of values."""
    cols, rots, ais, vis = (np.asarray(v, dtype=np.uint32).ravel() for v in (columns, rotations, alpha_indices, value_indices))
    assert cols.size == rots.size == ais.size == vis.size
    return (DeepExtSlot * cols.size)(*[DeepExtSlot(int(c), int(r), int(a), int(v)) for c, r, a, v in zip(cols, rots, ais, vis)])


def deep_combine_ext_dz_device(ctx, d_values: int, width: int, col_stride: int, log_blowup: int, shift: int, d_z: int, d_alphas: int, d_claims: int,
                               slots, d_out: int, accumulate: bool = False, stream: int = 0) -> None:
    """deep_combine_ext_device with z (d_z, four words), the weights (d_alphas) and the claimed values (d_claims) in device memory;
    slots: what deep_ext_slots returns; d_out: 16-byte aligned."""
    check(lib.toyni_deep_combine_ext_dz_device(ctx.handle, d_values, width, col_stride, log_blowup, shift, d_z or None, d_alphas or None,
                                               d_claims or None, slots if len(slots) else None, len(slots), 1 if accumulate else 0, d_out,
                                               stream or None), "GPU Ext DEEP combination (device point) failed")


def query_rows_device(d_indices: int, count: int, n: int, offsets, d_out: int, stream: int = 0) -> None:
    """d_out[q * len(offsets) + r] = (d_indices[q] + offsets[r]) mod n: the rows a matrix with next-row terms opens per query."""
    off = np.ascontiguousarray(offsets, dtype=np.uint32).ravel()
    check(lib.toyni_query_rows_device(d_indices or None, count, n, off.ctypes.data, off.size, d_out or None, stream or None), "GPU query rows failed")


# ---- the base-field first half of a Fibonacci proof with z in device memory (include/toyni_hip.h 3q) ----
def mask_poly_device(d_coeffs: int, n: int, mask_degree: int, key: bytes, nonce: int = 1, stream: int = 0) -> None:
    """T_hat = T - R + x^n R in place on d_coeffs[0 .. n + mask_degree); R from the ChaCha20 keystream under (key, nonce)."""
    k = (ctypes.c_uint8 * 32).from_buffer_copy(bytes(key)) if key is not None else None
    check(lib.toyni_mask_poly_device(d_coeffs or None, n, mask_degree, k, nonce, stream or None), "GPU mask failed")


def poly_eval_dz_device(ctx, d_coeffs: int, ncoeffs: int, d_z: int, mults, d_out: int, stream: int = 0) -> None:
    """poly_eval_device at the points mults[p] * z, z one word at the device pointer d_z; mults: canonical multipliers (1, g, g^2)."""
    m = np.ascontiguousarray(mults, dtype=np.uint32).ravel()
    check(lib.toyni_poly_eval_dz_device(ctx.handle, d_coeffs or None, ncoeffs, d_z or None, m.ctypes.data, m.size, d_out or None, stream or None),
          "GPU polynomial evaluation (device point) failed")


def fib_deep_dz_device(ctx, d_trace_lde: int, d_q_evals: int, d_out: int, log_blowup: int, shift: int, d_z: int, d_ood: int, trace_len: int,
                       d_check: int = 0, stream: int = 0) -> None:
    """fib_deep_device with z (d_z) and {t_z, t_gz, t_ggz, q_z} (d_ood) in device memory; d_check (optional): one word that
    receives 1 where the constraint check at z holds for a trace of trace_len rows, else 0."""
    check(lib.toyni_fib_deep_dz_device(ctx.handle, d_trace_lde, d_q_evals, d_out, log_blowup, shift, d_z or None, d_ood or None, trace_len,
                                       d_check or None, stream or None), "GPU DEEP evaluation (device point) failed")


def fri_phase_roots_device(d_levels: int, m_first: int, rounds: int, d_roots: int, stream: int = 0) -> None:
    """The roots of the `rounds` trees a commit phase left back to back in d_levels (tree k: m_first >> k leaves) to d_roots, 32 bytes each."""
    check(lib.toyni_fri_phase_roots_device(d_levels or None, m_first, rounds, d_roots or None, stream or None), "GPU phase roots failed")


# ---- constraint programs (include/toyni_hip.h 3f) ----
AIR_CELL, AIR_CONST, AIR_X, AIR_XINV, AIR_ADD, AIR_SUB, AIR_MUL, AIR_EMIT = range(8)
AIR_PARAM, AIR_MAX_PARAMS = 8, 256   # include/toyni_hip.h 3p: r[dst] = params[imm], a value the program does not carry
AIR_MAX_REGS, AIR_MAX_MATRICES = 64, 4
_P = 2013265921


class AirInsn(ctypes.Structure):   # toyni_air_insn
    _fields_ = [("op", ctypes.c_uint8), ("dst", ctypes.c_uint8), ("a", ctypes.c_uint8), ("b", ctypes.c_uint8), ("imm", ctypes.c_uint32)]


class AirMatrix(ctypes.Structure):   # toyni_air_matrix
    _fields_ = [("d_values", ctypes.c_void_p), ("width", ctypes.c_size_t), ("col_stride", ctypes.c_size_t)]


class AirInfo(ctypes.Structure):   # toyni_air_info
    _fields_ = [("ninsns", ctypes.c_uint32), ("nregs", ctypes.c_uint32), ("nconstraints", ctypes.c_uint32), ("nmatrices", ctypes.c_uint32),
                ("max_rotation", ctypes.c_uint32), ("divides_by_zh", ctypes.c_uint32), ("min_width", ctypes.c_uint32 * AIR_MAX_MATRICES)]


def air_insns(insns):
    """The instruction array of a constraint program from (op, dst, a, b, imm) tuples."""
    return (AirInsn * len(insns))(*[AirInsn(int(op), int(dst), int(a), int(b), int(imm)) for op, dst, a, b, imm in insns])


def air_program_check(insns) -> AirInfo:
    """toyni_air_program_check: host only.  insns: what air_insns returns, or the tuples it takes."""
    arr = insns if isinstance(insns, ctypes.Array) else air_insns(insns)
    info = AirInfo()
    check(lib.toyni_air_program_check(arr if len(arr) else None, len(arr), ctypes.byref(info)), "constraint program refused")
    return info


def air_program_check_params(insns):
    """toyni_air_program_check_params: the same check with AIR_PARAM accepted.  -> (AirInfo, nparams)"""
    arr = insns if isinstance(insns, ctypes.Array) else air_insns(insns)
    info, nparams = AirInfo(), ctypes.c_uint32()
    check(lib.toyni_air_program_check_params(arr if len(arr) else None, len(arr), ctypes.byref(info), ctypes.byref(nparams)),
          "constraint program refused")
    return info, nparams.value


class AirProgram:
    """A validated constraint program on ctx's device (toyni_air_program_create); a context manager.  params=True:
    toyni_air_program_create_params, which accepts AIR_PARAM; such a program runs under air_quotient_ext_dc_device."""

    def __init__(self, ctx, insns, params=False):
        arr = insns if isinstance(insns, ctypes.Array) else air_insns(insns)
        h = ctypes.c_void_p()
        create = lib.toyni_air_program_create_params if params else lib.toyni_air_program_create
        check(create(ctx.handle, arr if len(arr) else None, len(arr), ctypes.byref(h)), "constraint program refused")
        self.handle = h
        self.info = AirInfo()
        check(lib.toyni_air_program_info(h, ctypes.byref(self.info)), "constraint program info failed")
        self.nparams = 0
        if params:
            n = ctypes.c_uint32()
            check(lib.toyni_air_program_nparams(h, ctypes.byref(n)), "constraint program info failed")
            self.nparams = n.value

    def destroy(self) -> None:
        if self.handle:
            lib.toyni_air_program_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()


def air_quotient_device(ctx, prog, mats, log_blowup: int, shift: int, weights, d_q_out: int, d_c_out: int = 0, accumulate: bool = False,
                        stream=None) -> None:
    """Runs the program at every point of the LDE coset (include/toyni_hip.h 3f): d_q_out (+)= c / Z_H + the undivided constraints,
    d_c_out (+)= c.  mats: up to four (d_values, width, col_stride) column-major matrices; weights: one per constraint number."""
    m = (AirMatrix * len(mats))(*[AirMatrix(d or None, w, cs) for d, w, cs in mats])
    w = np.ascontiguousarray(weights, dtype=np.uint32)
    check(lib.toyni_air_quotient_device(ctx.handle, prog.handle, m if len(mats) else None, len(mats), log_blowup, shift, w.ctypes.data, w.size,
                                        d_c_out or None, d_q_out, 1 if accumulate else 0, stream or None), "GPU constraint program failed")


AIR_EXT_INLINE_WEIGHTS = 64   # TOYNI_AIR_EXT_INLINE_WEIGHTS: up to this many Ext weights ride in the kernel arguments (capturable)


def air_quotient_ext_device(ctx, prog, mats, log_blowup: int, shift: int, weights4, d_q_out: int, out_stride: int, d_c_out: int = 0,
                            accumulate: bool = False, stream=None) -> None:
    """The program under Ext weights in one call (include/toyni_hip.h 3k): coordinate e of Q_i = C_i / Z_H + the undivided constraints
    goes to d_q_out[e * out_stride + i], of C_i to d_c_out likewise; (+)= with accumulate.  weights4: one Ext weight (four canonical
    residues) per constraint number, as rows or flat; air_ext_weights builds it from the challenges of emit_ext constraints."""
    m = (AirMatrix * len(mats))(*[AirMatrix(d or None, w, cs) for d, w, cs in mats])
    w = np.ascontiguousarray(weights4, dtype=np.uint32).reshape(-1)
    if w.size % 4:
        raise ValueError("weights4 holds four words per Ext weight")
    check(lib.toyni_air_quotient_ext_device(ctx.handle, prog.handle, m if len(mats) else None, len(mats), log_blowup, shift, w.ctypes.data, w.size // 4,
                                            d_c_out or None, d_q_out, out_stride, 1 if accumulate else 0, stream or None),
          "GPU constraint program under Ext weights failed")


AIR_WEIGHTS_EXT, AIR_WEIGHTS_EMIT_EXT = 0, 1


def air_quotient_ext_dc_device(ctx, prog, mats, log_blowup: int, shift: int, d_params: int, nparams: int, d_alphas: int, nalphas: int,
                               weights_form: int, d_q_out: int, out_stride: int, d_c_out: int = 0, accumulate: bool = False, stream=None) -> None:
    """air_quotient_ext_device with the parameters of an AirProgram(params=True) and the weights in device memory (include/toyni_hip.h
    3p).  d_params: nparams words; d_alphas: nalphas Ext elements.  AIR_WEIGHTS_EXT: the alphas are the weights; AIR_WEIGHTS_EMIT_EXT:
    alpha_k weighs the four base constraints of emit_ext constraint k (what air_ext_weights builds on the host).  Two launches, nothing
    read back: the call only enqueues."""
    m = (AirMatrix * len(mats))(*[AirMatrix(d or None, w, cs) for d, w, cs in mats])
    check(lib.toyni_air_quotient_ext_dc_device(ctx.handle, prog.handle, m if len(mats) else None, len(mats), log_blowup, shift, d_params or None,
                                               nparams, d_alphas or None, nalphas, weights_form, d_c_out or None, d_q_out, out_stride,
                                               1 if accumulate else 0, stream or None), "GPU constraint program under device challenges failed")


def air_ext_weights(alphas):
    """The weight table of air_quotient_ext_device for constraints written with AirBuilder.emit_ext: base constraint 4 k + j is
    coordinate j of Ext constraint k, so it carries alphas[k] * X^j in F_p[X]/(X^4 - 11) -- a shift of the coordinates by j, those that
    wrap past X^3 times 11.  alphas: one Ext challenge (four canonical residues) per Ext constraint.  -> (4 len(alphas), 4) uint32."""
    out = np.zeros((4 * len(alphas), 4), dtype=np.uint32)
    for k, alpha in enumerate(alphas):
        a = [int(c) % _P for c in alpha]
        if len(a) != 4:
            raise ValueError("an Ext challenge has four coordinates")
        for j in range(4):
            for e in range(4):                       # X^j * a_e X^e = a_e X^(e + j),  X^4 = 11
                out[4 * k + j, (e + j) % 4] = a[e] * 11 % _P if e + j >= 4 else a[e]
    return out


class AirExpr:
    """A node of AirBuilder's expression graph: key = (op, operand nodes or fields...)."""

    def __init__(self, builder, key):
        self.builder, self.key = builder, key

    def _bin(self, op, other, swap=False):
        if isinstance(other, AirExt):      # base o Ext: the Ext operand's reflected method answers
            return NotImplemented
        o = other if isinstance(other, AirExpr) else self.builder.const(other)
        return self.builder._node((op, o, self) if swap else (op, self, o))

    def __add__(self, o): return self._bin(AIR_ADD, o)
    def __radd__(self, o): return self._bin(AIR_ADD, o, True)
    def __sub__(self, o): return self._bin(AIR_SUB, o)
    def __rsub__(self, o): return self._bin(AIR_SUB, o, True)
    def __mul__(self, o): return self._bin(AIR_MUL, o)
    def __rmul__(self, o): return self._bin(AIR_MUL, o, True)


class AirBuilder:
    """Expressions -> a constraint program.  cell / const / x / xinv return expressions that support + - * (ints become constants);
    emit records a constraint; compile shares common subexpressions (equal nodes are one object), orders the nodes so that operands
    come first, and gives every node a register that is free again after the node's last use."""

    def __init__(self):
        self.nodes, self.emits = {}, []

    def _node(self, key):
        ident = tuple(id(k) if isinstance(k, AirExpr) else k for k in key)   # operands are already unique objects
        if ident not in self.nodes:
            self.nodes[ident] = AirExpr(self, key)
        return self.nodes[ident]

    def cell(self, matrix, column, rotation=0): return self._node((AIR_CELL, int(matrix), int(column), int(rotation)))
    def const(self, v): return self._node((AIR_CONST, int(v) % _P))
    def x(self): return self._node((AIR_X,))
    def xinv(self, v): return self._node((AIR_XINV, int(v) % _P))

    def param(self, j):
        """params[j] of air_quotient_ext_dc_device (include/toyni_hip.h 3p): a value the call reads from device memory."""
        if not 0 <= int(j) < AIR_MAX_PARAMS:
            raise ValueError("a parameter index is below 256")
        return self._node((AIR_PARAM, int(j)))

    def emit(self, k, expr, divide=True):
        self.emits.append((int(k), expr if isinstance(expr, AirExpr) else self.const(expr), bool(divide)))

    def compile(self):
        """-> list of (op, dst, a, b, imm) tuples (air_insns takes them).  ValueError beyond 64 live registers."""
        order, seen = [], set()
        for _, root, _ in self.emits:             # operands first, depth first, without recursion (a long sum is a deep chain)
            stack = [(root, False)]
            while stack:
                node, done = stack.pop()
                if done:
                    order.append(node)
                elif id(node) not in seen:
                    seen.add(id(node))
                    stack.append((node, True))
                    stack.extend((k, False) for k in reversed(node.key[1:]) if isinstance(k, AirExpr))
        steps = [("node", nd) for nd in order]
        pos = {id(nd): i for i, nd in enumerate(order)}
        for k, root, divide in self.emits:        # an EMIT goes right after its value, so the value's register is free early
            steps.append(("emit", (k, root, divide, pos[id(root)])))
        steps.sort(key=lambda s: (pos[id(s[1])], 0) if s[0] == "node" else (s[1][3], 1))
        last = {}
        for i, (kind, what) in enumerate(steps):
            for k in (what.key[1:] if kind == "node" else (what[1],)):
                if isinstance(k, AirExpr):
                    last[id(k)] = i
        free, reg, insns = list(range(AIR_MAX_REGS - 1, -1, -1)), {}, []
        for i, (kind, what) in enumerate(steps):
            if kind == "emit":
                k, root, divide, _ = what
                insns.append((AIR_EMIT, 0, reg[id(root)], 0 if divide else 1, k))
                ops = [root]
            else:
                ops = [k for k in what.key[1:] if isinstance(k, AirExpr)]
            srcs = [reg[id(k)] for k in ops]
            for k in {id(k): k for k in ops}.values():           # operands whose last use this is give their register to the result
                if last[id(k)] == i:
                    free.append(reg[id(k)])
            if kind == "emit":
                continue
            if not free:
                raise ValueError("the program needs more than 64 live registers")
            dst = reg[id(what)] = free.pop()
            op = what.key[0]
            if op == AIR_CELL:
                insns.append((op, dst, what.key[3], what.key[1], what.key[2]))
            elif op in (AIR_CONST, AIR_XINV, AIR_PARAM):
                insns.append((op, dst, 0, 0, what.key[1]))
            elif op == AIR_X:
                insns.append((op, dst, 0, 0, 0))
            else:
                insns.append((op, dst, srcs[0], srcs[1], 0))
            if id(what) not in last:                             # unreachable for emitted roots; kept for safety of the free list
                free.append(dst)
        return insns

    # Ext = F_p[X]/(X^4 - 11) on top of the base-field expressions (include/toyni_hip.h 3i): an Ext expression is an AirExt of four
    # AirExpr, one per coordinate, so the constraints that tie an Ext accumulator (four base columns) to the trace compile to
    # ordinary base-field programs.  Nothing above changes: a program that uses none of this compiles as before.
    def ext_cell(self, matrix, first_column, rotation=0):
        """The Ext column held in columns first_column .. first_column + 3 of `matrix`."""
        return AirExt(tuple(self.cell(matrix, int(first_column) + k, rotation) for k in range(4)))

    def ext_const(self, v4):
        v = [int(c) for c in v4]
        assert len(v) == 4
        return AirExt(tuple(self.const(c) for c in v))

    def ext_param(self, first):
        """The Ext value held in the parameters first .. first + 3: usable wherever ext_const is."""
        return AirExt(tuple(self.param(int(first) + k) for k in range(4)))

    def ext(self, e):
        """An Ext expression from an AirExt (itself), a base-field AirExpr or an int (embedded in coordinate 0)."""
        if isinstance(e, AirExt):
            return e
        zero = self.const(0)
        return AirExt((e if isinstance(e, AirExpr) else self.const(e), zero, zero, zero))

    def emit_ext(self, k, e, divide=True):
        """The Ext constraint number k: base constraints 4 k .. 4 k + 3, one per coordinate (an Ext weight's four coordinates, each
        in its own call, weigh them)."""
        e = self.ext(e)
        for j in range(4):
            self.emit(4 * int(k) + j, e.c[j], divide)


EXT_W = 11   # X^4 = EXT_W


class AirExt:
    """An Ext-valued expression: four AirExpr coordinates; + - * with AirExt, AirExpr (base field) and ints."""

    def __init__(self, c):
        assert len(c) == 4
        self.c = tuple(c)

    def _other(self, o):
        return self.c[0].builder.ext(o)

    def __add__(self, o):
        o = self._other(o)
        return AirExt(tuple(a + b for a, b in zip(self.c, o.c)))

    __radd__ = __add__

    def __sub__(self, o):
        o = self._other(o)
        return AirExt(tuple(a - b for a, b in zip(self.c, o.c)))

    def __rsub__(self, o):
        return self._other(o) - self

    def __mul__(self, o):
        if not isinstance(o, AirExt):      # a base-field factor scales every coordinate
            return AirExt(tuple(a * o for a in self.c))
        out = []
        for k in range(4):                 # schoolbook, the high half folded back through X^4 = 11
            lo = [self.c[i] * o.c[k - i] for i in range(k + 1)]
            hi = [self.c[i] * o.c[k + 4 - i] for i in range(k + 1, 4)]
            acc = lo[0]
            for t in lo[1:]:
                acc = acc + t
            if hi:
                h = hi[0]
                for t in hi[1:]:
                    h = h + t
                acc = acc + h * EXT_W
            out.append(acc)
        return AirExt(tuple(out))

    __rmul__ = __mul__


# ---- accumulator columns (include/toyni_hip.h 3g) ----
SCAN_SUM, SCAN_PRODUCT = 0, 1


def column_scan_tile() -> int:
    """Elements one workgroup owns: a column of at most this many takes a single launch."""
    return lib.toyni_column_scan_tile()


def batch_inverse_device(d_in: int, d_out: int, count: int, d_zero_count: int = 0, stream=None) -> None:
    """d_out[i] = d_in[i]^-1, 0 for 0; d_zero_count (one device word, optional) receives the number of zeros.  d_out may be d_in."""
    check(lib.toyni_batch_inverse_device(d_in, d_out, count, d_zero_count or None, stream or None), "GPU batch inversion failed")


def column_scan_device(ctx, num: int, den: int, out: int, n: int, batch: int = 1, op: int = SCAN_SUM, init=None, totals: int = 0, strides=None,
                       stream=None) -> None:
    """out[0] = init[b], out[i] = out[i-1] (+ or *) num[i-1] / den[i-1] for each of `batch` columns (include/toyni_hip.h 3g): the
    accumulator column of a LogUp sum or of a permutation product.  num or den may be 0 (absent: ones); a zero denominator makes the
    term 0.  init: one residue per column (default: the op's identity).  totals: 2 * batch device words, optional: the wrap-around
    value and the zero denominators of each column.  strides: (num, den, out) words between columns, default n each."""
    if init is None:
        init = [1 if op == SCAN_PRODUCT else 0] * batch
    i = np.ascontiguousarray(init, dtype=np.uint32)
    assert i.size == batch
    ns, ds, os_ = strides if strides is not None else (n, n, n)
    check(lib.toyni_column_scan_device(ctx.handle, num or None, ns, den or None, ds, out, os_, n, batch, op, i.ctypes.data, totals or None,
                                       stream or None), "GPU column scan failed")


# ---- accumulator columns under an Ext challenge (include/toyni_hip.h 3i) ----
class _ExtOperand(ctypes.Structure):   # toyni_ext_operand
    _fields_ = [("d_values", ctypes.c_void_p), ("stride", ctypes.c_size_t), ("width", ctypes.c_uint32), ("shift", ctypes.c_uint32 * 4)]


def ExtOperand(d_values: int = 0, stride: int = 0, width: int = 0, shift=(0, 0, 0, 0)) -> _ExtOperand:
    """An operand of column_scan_ext_device.  width 4: an Ext column (four base columns `stride` words apart) per accumulator; width 1:
    a base column embedded in Ext; width 0: the constant 1.  shift (four coordinates) is added to every element: gamma + v_i."""
    sh = [int(c) for c in shift]
    assert len(sh) == 4
    return _ExtOperand(d_values or None, stride, width, (ctypes.c_uint32 * 4)(*sh))


def column_scan_ext_tile() -> int:
    """Ext elements one workgroup owns: a column of at most this many takes a single launch."""
    return lib.toyni_column_scan_ext_tile()


def batch_inverse_ext_device(d_in: int, in_stride: int, d_out: int, out_stride: int, count: int, d_zero_count: int = 0, stream=None) -> None:
    """out_i = in_i^-1 in Ext, 0 for 0, on one Ext column (four base columns a stride apart); d_zero_count (one device word, optional)
    receives the number of zeros.  d_out may be d_in with equal strides."""
    check(lib.toyni_batch_inverse_ext_device(d_in, in_stride, d_out, out_stride, count, d_zero_count or None, stream or None),
          "GPU Ext batch inversion failed")


def column_scan_ext_device(ctx, num, den, out: int, out_stride: int, n: int, batch: int = 1, op: int = SCAN_SUM, init=None, totals: int = 0,
                           stream=None) -> None:
    """out[0] = init[b], out[i] = out[i-1] (+ or *) num[i-1] / den[i-1] in Ext for each of `batch` Ext columns (include/toyni_hip.h 3i).
    num, den: ExtOperand or None (the constant 1); a zero denominator makes the term 0.  out: 4 * batch base columns out_stride words
    apart.  init: batch x 4 residues (default: the op's identity).  totals: 8 * batch device words, optional: per column the
    wrap-around value (4), the zero denominators (1) and three zero words."""
    if init is None:
        init = [[1 if op == SCAN_PRODUCT else 0, 0, 0, 0]] * batch
    i = np.ascontiguousarray(init, dtype=np.uint32)
    assert i.size == 4 * batch
    check(lib.toyni_column_scan_ext_device(ctx.handle, ctypes.byref(num) if num is not None else None, ctypes.byref(den) if den is not None else None,
                                           out, out_stride, n, batch, op, i.ctypes.data, totals or None, stream or None), "GPU Ext column scan failed")


# ---- the same with gamma in device memory (include/toyni_hip.h 3p) ----
EXT_SHIFT_NONE = 0xFFFFFFFF


class _ExtOperandDc(ctypes.Structure):   # toyni_ext_operand_dc
    _fields_ = [("d_values", ctypes.c_void_p), ("stride", ctypes.c_size_t), ("width", ctypes.c_uint32), ("shift_index", ctypes.c_uint32)]


def ExtOperandDc(d_values: int = 0, stride: int = 0, width: int = 0, shift_index: int = EXT_SHIFT_NONE) -> _ExtOperandDc:
    """ExtOperand whose shift is the Ext element number shift_index of the call's d_challenges (EXT_SHIFT_NONE: no shift)."""
    return _ExtOperandDc(d_values or None, stride, width, shift_index)


def column_scan_ext_dc_device(ctx, num, den, d_challenges: int, out: int, out_stride: int, n: int, batch: int = 1, op: int = SCAN_SUM, init=None,
                              totals: int = 0, stream=None) -> None:
    """column_scan_ext_device with the operands' shifts read from device memory: num, den are ExtOperandDc or None.  The call only
    enqueues; the words are reduced mod p on the device."""
    if init is None:
        init = [[1 if op == SCAN_PRODUCT else 0, 0, 0, 0]] * batch
    i = np.ascontiguousarray(init, dtype=np.uint32)
    assert i.size == 4 * batch
    check(lib.toyni_column_scan_ext_dc_device(ctx.handle, ctypes.byref(num) if num is not None else None, ctypes.byref(den) if den is not None else None,
                                              d_challenges or None, out, out_stride, n, batch, op, i.ctypes.data, totals or None, stream or None),
          "GPU Ext column scan under device challenges failed")


# ---- the Fiat-Shamir transcript in device memory and the commit phases on it (include/toyni_hip.h 3l) ----
TRANSCRIPT_CAPACITY = 1008
POW_MAX_BITS = 32
POW_MAX_LOG_TRIES = 40
POW_WINDOW_SLACK = 8         # default window of a grind: 2^(bits + 8) candidates -- a window without a hit has probability e^-256


def pow_default_log_tries(bits: int) -> int:
    """The window DeviceTranscript.grind searches when the caller names none: a search ends at its first hit, so the window only bounds
    a search that has none -- and that one occupies the whole device until the window is exhausted (2^40 candidates are most of a
    minute).  bits + 8 keeps a failing call at 256 times the expected work of a succeeding one."""
    return min(POW_MAX_LOG_TRIES, bits + POW_WINDOW_SLACK)


def pow_check(state: bytes, nonce: int, bits: int) -> bool:
    """accept(state, nonce, bits) of include/toyni_hip.h 3n on the host (toyni_pow_check_host): what a verifier computes before it
    absorbs the nonce's 8 little-endian bytes."""
    state = bytes(state)
    if not 0 <= nonce < 1 << 64:
        raise ValueError("a proof-of-work nonce is a 64-bit value")
    if not 0 <= bits <= POW_MAX_BITS:
        raise ValueError(f"proof-of-work bits lie in 0..{POW_MAX_BITS}")
    accepted = ctypes.c_int(-1)
    buf = (ctypes.c_uint8 * len(state)).from_buffer_copy(state) if state else None
    check(lib.toyni_pow_check_host(buf, len(state), nonce, bits, ctypes.byref(accepted)), "proof-of-work check failed")
    return bool(accepted.value)


class DeviceTranscript:
    """toyni_transcript: FiatShamirTranscript (src/transcript.rs) as 1024 bytes of device memory.  Every method but `download` and
    `status` only enqueues on `stream`; outputs are device pointers.  What the host cannot check -- an absorb beyond the capacity --
    sets the sticky status word, after which every operation writes zeros: read `status()` once the work has been synchronised."""

    def __init__(self):
        p = ctypes.c_void_p()
        check(lib.toyni_malloc(ctypes.byref(p), 1024), "device allocation of a transcript failed")
        self.ptr = p.value
        self._staged = []    # host copies that an enqueued upload may still read

    @classmethod
    def from_bytes(cls, state: bytes = b"toyni-stark-v1", stream: int = 0) -> "DeviceTranscript":
        tr = cls()
        tr.load(state, stream)
        return tr

    def load(self, state: bytes, stream: int = 0) -> None:
        """Replace the transcript by `state` (status cleared): one stream-ordered upload of a host copy, no kernel."""
        if len(state) > TRANSCRIPT_CAPACITY:
            raise ValueError(f"a device transcript holds at most {TRANSCRIPT_CAPACITY} bytes")
        host = np.zeros(1024, dtype=np.uint8)
        host[:4] = np.frombuffer(np.uint32(len(state)).tobytes(), dtype=np.uint8)
        host[16:16 + len(state)] = np.frombuffer(bytes(state), dtype=np.uint8)
        self._staged = self._staged[-7:] + [host]
        check(lib.toyni_memcpy_h2d_async(self.ptr, host.ctypes.data, 1024, stream or None), "upload of a transcript failed")

    def absorb_device(self, d_bytes: int, length: int, stream: int = 0) -> None:
        check(lib.toyni_transcript_absorb_device(self.ptr, d_bytes or None, length, stream or None), "GPU transcript absorb failed")

    def squeeze(self, d_out: int, count: int = 1, stream: int = 0) -> None:
        """`count` challenges (canonical residues) to d_out; an Ext challenge is count = 4."""
        check(lib.toyni_transcript_squeeze_device(self.ptr, d_out, count, stream or None), "GPU transcript squeeze failed")

    def squeeze_indices(self, d_out: int, count: int, mx: int, stream: int = 0) -> None:
        """`count` distinct values below `mx`, in order of first appearance, to d_out."""
        check(lib.toyni_transcript_squeeze_indices_device(self.ptr, count, mx, d_out, stream or None), "GPU transcript index squeeze failed")

    def squeeze_ext_point(self, d_z: int, stream: int = 0) -> None:
        """The out-of-domain point (include/toyni_hip.h 3o): four challenges to d_z, squeezed again while z1 = z2 = z3 = 0."""
        check(lib.toyni_transcript_squeeze_ext_point_device(self.ptr, d_z or None, stream or None), "GPU transcript point squeeze failed")

    def squeeze_point(self, d_z: int, log_N: int, shift: int, stream: int = 0) -> None:
        """derive_z of the Fibonacci protocol (include/toyni_hip.h 3q): one challenge to d_z, squeezed again while z^N = 1 or
        (z / shift)^N = 1, N = 2^log_N."""
        check(lib.toyni_transcript_squeeze_point_device(self.ptr, log_N, shift, d_z or None, stream or None), "GPU transcript point squeeze failed")

    def absorb_fields(self, d_words: int, count: int, stream: int = 0) -> None:
        """absorb_field for `count` (<= 126) device-resident words: 8 little-endian bytes of the canonical residue each."""
        check(lib.toyni_transcript_absorb_fields_device(self.ptr, d_words or None, count, stream or None), "GPU transcript field absorb failed")

    def grind(self, d_nonce: int, bits: int, start: int = 0, log_tries: int = None, stream: int = 0) -> None:
        """Proof of work (include/toyni_hip.h 3n): the smallest nonce of [start, start + 2^log_tries) whose SHA256(state || LE64(nonce))
        has `bits` leading zero bits goes to the device word d_nonce (8-byte aligned) and its 8 bytes are absorbed.  A window without
        one sets the status and leaves the state as it is, with *d_nonce = 0 -- after the WHOLE window has been hashed: log_tries
        defaults to pow_default_log_tries(bits) = min(40, bits + 8); name a wider one only where the time of a failing call is
        acceptable."""
        if log_tries is None:
            log_tries = pow_default_log_tries(min(max(int(bits), 0), POW_MAX_BITS))
        check(lib.toyni_transcript_grind_device(self.ptr, bits, start, log_tries, d_nonce or None, stream or None), "GPU transcript grind failed")

    def download(self):
        """(state bytes, status) after a synchronous copy (the default stream: synchronise the stream that carries the work first)."""
        host = np.zeros(1024, dtype=np.uint8)
        check(lib.toyni_memcpy_d2h(host.ctypes.data, self.ptr, 1024), "download of a transcript failed")
        length, status = (int(v) for v in host[:8].view(np.uint32))
        return host[16:16 + min(length, TRANSCRIPT_CAPACITY)].tobytes(), status

    def status(self) -> int:
        return self.download()[1]

    def free(self) -> None:
        if self.ptr:
            lib.toyni_free(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def fri_query_positions_device(d_indices: int, count: int, m0: int, final_size: int, d_out: int, stream: int = 0) -> None:
    """The positions `count` queries open in every layer but the final one: per layer k (m0 >> k elements) the pairs
    [i mod half, i mod half + half], the layers back to back -- rounds x 2 count words."""
    check(lib.toyni_fri_query_positions_device(d_indices, count, m0, final_size, d_out, stream or None), "GPU query positions failed")


def fri_commit_phase_transcript_device(ctx, d_layer0: int, m0: int, x0: int, final_size: int, d_salts: int, transcript: DeviceTranscript,
                                       d_layers: int, d_levels: int, d_betas: int = 0, stream: int = 0) -> None:
    """fri_commit_phase_device with the transcript on the device: asynchronous, no callback; every beta is squeezed from
    `transcript` and every root absorbed into it by kernels.  d_betas (optional): one word per round."""
    check(lib.toyni_fri_commit_phase_transcript_device(ctx.handle, d_layer0, m0, x0, final_size, d_salts or None, transcript.ptr, d_layers,
                                                       d_levels, d_betas or None, stream or None), "GPU FRI commit phase (device transcript) failed")


def fri_commit_phase_transcript_ext_device(ctx, d_layer0: int, m0: int, x0: int, final_size: int, d_salts: int, transcript: DeviceTranscript,
                                           d_layers: int, d_levels: int, d_betas: int = 0, stream: int = 0) -> None:
    """The same over Ext-valued layers (four words per element, an Ext beta per round: d_betas takes four words per round)."""
    check(lib.toyni_fri_commit_phase_transcript_ext_device(ctx.handle, d_layer0, m0, x0, final_size, d_salts or None, transcript.ptr, d_layers,
                                                           d_levels, d_betas or None, stream or None),
          "GPU Ext FRI commit phase (device transcript) failed")


# ---- a batch dimension for the tail of a proof (include/toyni_hip.h 3r) ----
class DeviceTranscriptBatch:
    """toyni_transcript d_tr[batch]: one DeviceTranscript per proof in one allocation, 1 KiB apart, every operation one launch for
    all of them.  `status` is sticky per proof.  Every method but `download` and `status` only enqueues on `stream`."""

    def __init__(self, batch: int):
        if batch < 1:
            raise ValueError("a transcript batch holds at least one transcript")
        p = ctypes.c_void_p()
        check(lib.toyni_malloc(ctypes.byref(p), 1024 * batch), "device allocation of a transcript batch failed")
        self.ptr, self.batch = p.value, batch
        self._staged = []    # host copies that an enqueued upload may still read

    @classmethod
    def from_states(cls, states, stream: int = 0) -> "DeviceTranscriptBatch":
        """One state per proof; the lengths may differ."""
        tr = cls(len(states))
        tr.load(states, stream)
        return tr

    def load(self, states, stream: int = 0) -> None:
        if len(states) != self.batch:
            raise ValueError(f"{self.batch} states are needed")
        host = np.zeros((self.batch, 1024), dtype=np.uint8)
        for b, state in enumerate(states):
            if len(state) > TRANSCRIPT_CAPACITY:
                raise ValueError(f"a device transcript holds at most {TRANSCRIPT_CAPACITY} bytes")
            host[b, :4] = np.frombuffer(np.uint32(len(state)).tobytes(), dtype=np.uint8)
            host[b, 16:16 + len(state)] = np.frombuffer(bytes(state), dtype=np.uint8)
        self._staged = self._staged[-7:] + [host]
        check(lib.toyni_memcpy_h2d_async(self.ptr, host.ctypes.data, host.nbytes, stream or None), "upload of a transcript batch failed")

    def absorb_device(self, d_bytes: int, byte_stride: int, length: int, stream: int = 0) -> None:
        """Transcript b absorbs `length` bytes at d_bytes + b * byte_stride."""
        check(lib.toyni_transcript_absorb_batch_device(self.ptr, self.batch, d_bytes or None, byte_stride, length, stream or None),
              "GPU batched transcript absorb failed")

    def squeeze_indices(self, d_out: int, out_stride: int, count: int, mx: int, stream: int = 0) -> None:
        """Per proof `count` distinct values below `mx` to d_out + b * out_stride words."""
        check(lib.toyni_transcript_squeeze_indices_batch_device(self.ptr, self.batch, count, mx, d_out, out_stride, stream or None),
              "GPU batched transcript index squeeze failed")

    def squeeze_point(self, log_N: int, shift: int, d_z: int, z_stride: int = 1, stream: int = 0) -> None:
        """derive_z per proof (include/toyni_hip.h 3s): proof b's z to d_z + b * z_stride words."""
        check(lib.toyni_transcript_squeeze_point_batch_device(self.ptr, self.batch, log_N, shift, d_z, z_stride, stream or None),
              "GPU batched transcript point squeeze failed")

    def absorb_fields(self, d_words: int, word_stride: int, count: int, stream: int = 0) -> None:
        """Transcript b absorbs the `count` field words at d_words + b * word_stride (absorb_field, 8 bytes each)."""
        check(lib.toyni_transcript_absorb_fields_batch_device(self.ptr, self.batch, d_words or None, word_stride, count, stream or None),
              "GPU batched transcript field absorb failed")

    def download(self):
        """[(state bytes, status)] per proof after a synchronous copy (synchronise the stream that carries the work first)."""
        host = np.zeros((self.batch, 1024), dtype=np.uint8)
        check(lib.toyni_memcpy_d2h(host.ctypes.data, self.ptr, host.nbytes), "download of a transcript batch failed")
        out = []
        for b in range(self.batch):
            length, status = (int(v) for v in host[b, :8].view(np.uint32))
            out.append((host[b, 16:16 + min(length, TRANSCRIPT_CAPACITY)].tobytes(), status))
        return out

    def status(self):
        return [s for _, s in self.download()]

    def free(self) -> None:
        if self.ptr:
            lib.toyni_free(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def fri_query_positions_batch_device(d_indices: int, index_stride: int, count: int, m0: int, final_size: int, batch: int, d_out: int,
                                     out_stride: int, stream: int = 0) -> None:
    check(lib.toyni_fri_query_positions_batch_device(d_indices, index_stride, count, m0, final_size, batch, d_out, out_stride, stream or None),
          "GPU batched query positions failed")


# ---- the batch dimension of the first half of a Fibonacci proof (include/toyni_hip.h 3s): thin bindings, strides as the header counts them ----
def chacha20_fill_batch_device(d_out: int, out_stride: int, nbytes: int, d_keys: int, nonce: int, batch: int, stream: int = 0) -> None:
    """Per proof `nbytes` keystream bytes at d_out + b * out_stride under the key at d_keys + 32 b (device memory)."""
    check(lib.toyni_chacha20_fill_batch_device(d_out or None, out_stride, nbytes, d_keys or None, nonce, batch, stream or None),
          "GPU batched ChaCha20 fill failed")


def mask_poly_batch_device(d_coeffs: int, coeff_stride: int, n: int, mask_degree: int, d_keys: int, nonce: int, batch: int, stream: int = 0) -> None:
    check(lib.toyni_mask_poly_batch_device(d_coeffs or None, coeff_stride, n, mask_degree, d_keys or None, nonce, batch, stream or None),
          "GPU batched mask failed")


def fib_quotient_batch_device(ctx, d_trace_lde: int, trace_stride: int, d_c_evals: int, c_stride: int, d_q_evals: int, q_stride: int,
                              log_blowup: int, shift: int, batch: int, stream: int = 0) -> None:
    check(lib.toyni_fib_quotient_batch_device(ctx.handle, d_trace_lde or None, trace_stride, d_c_evals or None, c_stride, d_q_evals or None, q_stride,
                                              log_blowup, shift, batch, stream or None), "GPU batched constraint / quotient evaluation failed")


def poly_eval_dz_batch_device(ctx, d_coeffs: int, coeff_stride: int, ncoeffs: int, d_z: int, z_stride: int, mults, batch: int, d_out: int,
                              out_stride: int, stream: int = 0) -> None:
    m = np.ascontiguousarray(mults, dtype=np.uint32).ravel()
    check(lib.toyni_poly_eval_dz_batch_device(ctx.handle, d_coeffs or None, coeff_stride, ncoeffs, d_z or None, z_stride, m.ctypes.data, m.size, batch,
                                              d_out or None, out_stride, stream or None), "GPU batched polynomial evaluation (device point) failed")


def fib_deep_dz_batch_device(ctx, d_trace_lde: int, trace_stride: int, d_q_evals: int, q_stride: int, d_out: int, out_stride: int, log_blowup: int,
                             shift: int, d_z: int, z_stride: int, d_ood: int, ood_stride: int, trace_len: int, d_check: int, check_stride: int,
                             batch: int, stream: int = 0) -> None:
    check(lib.toyni_fib_deep_dz_batch_device(ctx.handle, d_trace_lde or None, trace_stride, d_q_evals or None, q_stride, d_out or None, out_stride,
                                             log_blowup, shift, d_z or None, z_stride, d_ood or None, ood_stride, trace_len, d_check or None,
                                             check_stride, batch, stream or None), "GPU batched DEEP evaluation (device point) failed")


def query_rows_batch_device(d_indices: int, index_stride: int, count: int, n: int, offsets, batch: int, d_out: int, out_stride: int,
                            stream: int = 0) -> None:
    off = np.ascontiguousarray(offsets, dtype=np.uint32).ravel()
    check(lib.toyni_query_rows_batch_device(d_indices or None, index_stride, count, n, off.ctypes.data, off.size, batch, d_out or None, out_stride,
                                            stream or None), "GPU batched query rows failed")


def fri_phase_roots_batch_device(d_levels: int, level_stride: int, m_first: int, rounds: int, batch: int, d_roots: int, root_stride: int,
                                 stream: int = 0) -> None:
    check(lib.toyni_fri_phase_roots_batch_device(d_levels or None, level_stride, m_first, rounds, batch, d_roots or None, root_stride, stream or None),
          "GPU batched phase roots failed")


def copy_rows_device(d_dst: int, dst_stride: int, d_src: int, src_stride: int, row_bytes: int, rows: int, stream: int = 0) -> None:
    """`rows` stream-ordered copies of row_bytes bytes in one launch; strides in bytes."""
    check(lib.toyni_copy_rows_device(d_dst or None, dst_stride, d_src or None, src_stride, row_bytes, rows, stream or None), "GPU row copy failed")


def _phase_batch(entry, what, ctx, d_layer0, layer0_stride, m0, x0, final_size, d_salts, salt_stride, transcripts, d_layers, layers_stride,
                 d_levels, level_stride, d_betas, beta_stride, stream):
    check(entry(ctx.handle, d_layer0, layer0_stride, m0, x0, final_size, d_salts or None, salt_stride, transcripts.ptr, transcripts.batch,
                d_layers, layers_stride, d_levels, level_stride, d_betas or None, beta_stride, stream or None), what)


def fri_commit_phase_transcript_batch_device(ctx, d_layer0: int, layer0_stride: int, m0: int, x0: int, final_size: int, d_salts: int,
                                             salt_stride: int, transcripts: DeviceTranscriptBatch, d_layers: int, layers_stride: int,
                                             d_levels: int, level_stride: int, d_betas: int = 0, beta_stride: int = 0, stream: int = 0) -> None:
    """fri_commit_phase_transcript_device for transcripts.batch proofs in one chain of launches; strides in words, bytes for the salts
    and the levels."""
    _phase_batch(lib.toyni_fri_commit_phase_transcript_batch_device, "GPU batched FRI commit phase failed", ctx, d_layer0, layer0_stride, m0, x0,
                 final_size, d_salts, salt_stride, transcripts, d_layers, layers_stride, d_levels, level_stride, d_betas, beta_stride, stream)


def fri_commit_phase_transcript_ext_batch_device(ctx, d_layer0: int, layer0_stride: int, m0: int, x0: int, final_size: int, d_salts: int,
                                                 salt_stride: int, transcripts: DeviceTranscriptBatch, d_layers: int, layers_stride: int,
                                                 d_levels: int, level_stride: int, d_betas: int = 0, beta_stride: int = 0,
                                                 stream: int = 0) -> None:
    """The same over Ext-valued layers."""
    _phase_batch(lib.toyni_fri_commit_phase_transcript_ext_batch_device, "GPU batched Ext FRI commit phase failed", ctx, d_layer0, layer0_stride,
                 m0, x0, final_size, d_salts, salt_stride, transcripts, d_layers, layers_stride, d_levels, level_stride, d_betas, beta_stride, stream)


# ---- four-to-one Ext FRI rounds under coset leaves (include/toyni_hip.h 3m) ----
def fri_fold4_commit_ext_device(ctx, d_evals: int, d_out: int, m: int, beta4, x0: int, d_salts: int, d_levels: int, stream: int = 0) -> None:
    """One four-to-one round: the m / 4 folded Ext elements to d_out (two pairwise folds, beta4 on x0 then beta4^2 on x0^2, in one
    sweep) and their coset tree (m / 16 leaves, every level) to d_levels."""
    b = np.ascontiguousarray(beta4, dtype=np.uint32)
    assert b.size == 4
    check(lib.toyni_fri_fold4_commit_ext_device(ctx.handle, d_evals, d_out, m, b.ctypes.data, x0, d_salts or None, d_levels, stream or None),
          "GPU four-to-one fold + commit (Ext) failed")


def fri4_query_positions_device(d_indices: int, count: int, m0: int, final_size: int, d_out: int, stream: int = 0) -> None:
    """The coset leaf `count` queries open in every layer but the final one: list k holds index mod (m0 >> (2 k + 2)), the lists back
    to back -- rounds x count words."""
    check(lib.toyni_fri4_query_positions_device(d_indices, count, m0, final_size, d_out, stream or None), "GPU four-to-one query positions failed")


def fri4_commit_phase_transcript_ext_device(ctx, d_layer0: int, m0: int, x0: int, final_size: int, d_salts: int, transcript: DeviceTranscript,
                                            d_layers: int, d_levels: int, d_betas: int = 0, stream: int = 0) -> None:
    """The Ext commit phase on a device transcript folding four to one per round under coset leaves: half the rounds of
    fri_commit_phase_transcript_ext_device, each tree two levels lower.  d_betas (optional): four words per round."""
    check(lib.toyni_fri4_commit_phase_transcript_ext_device(ctx.handle, d_layer0, m0, x0, final_size, d_salts or None, transcript.ptr, d_layers,
                                                            d_levels, d_betas or None, stream or None),
          "GPU four-to-one Ext FRI commit phase failed")


def merkle_open_record_bytes(n: int) -> int:
    return lib.toyni_merkle_open_record_bytes(n)


def merkle_open_device(d_levels: int, n: int, d_values: int, d_salts: int, d_indices: int, nidx: int, d_out: int, stream: int = 0) -> None:
    check(lib.toyni_merkle_open_device(d_levels, n, d_values, d_salts or None, d_indices, nidx, d_out, stream or None), "GPU Merkle opening failed")


class _OpenGroup(ctypes.Structure):   # toyni_merkle_open_group (include/toyni_hip.h 3c)
    _fields_ = [("d_levels", ctypes.c_void_p), ("n", ctypes.c_size_t), ("d_values", ctypes.c_void_p), ("d_salts", ctypes.c_void_p),
                ("d_indices", ctypes.c_void_p), ("nidx", ctypes.c_size_t), ("d_out", ctypes.c_void_p)]


def merkle_open_groups_device(groups, stream: int = 0) -> None:
    """The openings of several trees in one launch per 32 trees.  groups: iterable of (d_levels, n, d_values, d_salts, d_indices, nidx,
    d_out), every field as in merkle_open_device."""
    arr = (_OpenGroup * len(groups))(*[_OpenGroup(lv, n, v, s or None, ix, k, o) for lv, n, v, s, ix, k, o in groups])
    check(lib.toyni_merkle_open_groups_device(arr, len(groups), stream or None), "GPU Merkle openings failed")


def parse_openings(raw: np.ndarray, n: int, indices, salted: bool):
    """Records of toyni_merkle_open_device -> the fields of MerkleOpening (src/fibonacci.rs:366-375)."""
    depth = 0
    m = n
    while m > 1:
        m = (m + 1) // 2
        depth += 1
    rec = merkle_open_record_bytes(n)
    raw = np.asarray(raw, dtype=np.uint8).reshape(len(indices), rec)
    out = []
    for k, index in enumerate(indices):
        r = raw[k]
        path = [r[32 * l:32 * (l + 1)].tobytes() for l in range(depth)]
        salt = r[32 * depth:32 * depth + 16].tobytes() if salted else b""
        value = int.from_bytes(r[32 * depth + 16:32 * depth + 24].tobytes(), "little")
        position = [bool(b) for b in r[32 * depth + 24:32 * depth + 24 + depth]]
        out.append({"index": int(index), "value": value, "path": path, "position": position, "salt": salt})
    return out
