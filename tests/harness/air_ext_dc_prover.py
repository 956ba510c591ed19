"""air_ext_dz_prover.py with the transcript on the device from the FIRST root onward (include/toyni_hip.h 3p) -- TEST HARNESS.

The device transcript is loaded with its 14 initial bytes right after the trace upload, and from there the prover only ENQUEUES:

  main columns            as air_ext_prover.py; DeviceTranscript.absorb_device of the root where the commitment left it
  gamma                   one squeeze of 4 words
  accumulators            toyni_column_scan_ext_dc_device twice, gamma named by index 0 of the one challenge array; commit, absorb
  constraint weights      one squeeze of 4 x NUM_WEIGHTS words
  quotient                ONE toyni_air_quotient_ext_dc_device call (TOYNI_AIR_WEIGHTS_EMIT_EXT) on a program written with ext_param(0)
                          and created once per (context, process): gamma is its parameters 0..3; commit, absorb
  the rest                steps 4-7 of air_ext_dz_prover.py as they are

then ONE synchronisation and the downloads, the three roots among them.  The wire form is air_ext_ref_prover's.  EVENTS receives
"transcript loaded" and "final download" when those points are passed, as in the dz harness."""
import numpy as np
import torch

import toyni_amd
from toyni_amd._lib import lib as _lib

import ext_model as em

from .air_ext_prover import _root
from .air_ext_ref_prover import salt_pool
from .air_ext_verifier import ACC_WIDTH, DEEP_TERMS, MAIN_WIDTH, NUM_QUERIES, NUM_WEIGHTS, Q_WIDTH, from_columns, opening_plan
from .air_ref_prover import layer_sizes
from .fib_verifier import COSET_SHIFT, root_of_unity

EVENTS = []
CREATED = []          # one entry per constraint program created: a test counts them
_PROGRAMS = {}


def constraint_program_params():
    """air_ext_prover.constraint_program with gamma as the parameters 0..3 instead of four constants: the program of the AIR, not of
    one proof."""
    bld = toyni_amd.prover.AirBuilder()
    g = bld.ext_param(0)
    a, b, u, w = (bld.cell(0, c) for c in range(4))
    zc, zn, sc, sn = bld.ext_cell(1, 0, 0), bld.ext_cell(1, 0, 1), bld.ext_cell(1, 4, 0), bld.ext_cell(1, 4, 1)
    bld.emit_ext(0, zn * (g + b) - zc * (g + a))
    bld.emit_ext(1, (sn - sc) * (g + w) - u)
    bld.emit_ext(2, (zc - 1) * bld.xinv(1), divide=False)
    bld.emit_ext(3, sc * bld.xinv(1), divide=False)
    return bld.compile()


def program_for(ctx):
    """The AIR's program on ctx's device: created at the first proof, kept for every later one."""
    key = id(ctx)
    if key not in _PROGRAMS:
        _PROGRAMS[key] = (ctx, toyni_amd.prover.AirProgram(ctx, constraint_program_params(), params=True))
        CREATED.append(key)
    return _PROGRAMS[key][1]


def prove(main, log_blowup, seed, info=None):
    """The proof in wire form (air_ext_ref_prover.WIRE_FIELDS) of the 4 x n main trace (canonical residues).  info (optional dict)
    receives the device transcript's final status word as "transcript_status"."""
    pv = toyni_amd.prover
    COL, ROW = toyni_amd.ROWS_COLUMN_MAJOR, toyni_amd.ROWS_ROW_MAJOR
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    main = np.asarray(main, dtype=np.uint64)
    n = main.shape[1]
    assert main.shape == (MAIN_WIDTH, n) and n >= 2 and n & (n - 1) == 0 and log_blowup >= 1
    B, N = 1 << log_blowup, n << log_blowup
    g = root_of_unity(n.bit_length() - 1)
    ctx_n, ctx_N = toyni_amd.ntt.get_or_create_ctx(n), toyni_amd.ntt.get_or_create_ctx(N)
    prog = program_for(ctx_N)                    # (the first proof on a context creates it: blocking, before anything is enqueued)
    sizes = layer_sizes(n, N)
    pool = torch.from_numpy(salt_pool(n, N, seed)).to(dev)
    taken = [0]

    def take_salts(count):
        s = pool[taken[0]:taken[0] + count]
        taken[0] += count
        return s

    def words(count):
        return torch.empty(count, dtype=torch.int32, device=dev)

    def tree(leaves):
        return torch.empty((_lib.toyni_merkle_total_digests(leaves), 32), dtype=torch.uint8, device=dev)

    def committed_matrix(d_columns, width):
        """columns over H -> (coefficients, LDE, salts, tree levels); the root stays where the commitment wrote it"""
        coef, lde = words(width * n), words(width * N)
        ctx_n.run_device(d_columns, coef.data_ptr(), width, True, stream=stream)
        ctx_N.lde_device(coef.data_ptr(), lde.data_ptr(), width, log_blowup, COSET_SHIFT, stream=stream)
        salts, levels = take_salts(N), tree(N)
        toyni_amd.merkle_commit_rows_device(lde.data_ptr(), N, width, COL, N, salts.data_ptr(), levels.data_ptr(), stream=stream)
        return coef, lde, salts, levels

    # ---- the trace upload, every buffer of the proof, then the transcript goes to the device ----
    vals = torch.from_numpy(main.astype(np.uint32).view(np.int32).reshape(-1)).to(dev)
    nterms = len(DEEP_TERMS)
    challenges = words(4 + 4 * NUM_WEIGHTS)                                   # gamma, then the alphas
    d_gamma, d_alphas = challenges.data_ptr(), challenges.data_ptr() + 16
    acc, q = words(ACC_WIDTH * n), words(Q_WIDTH * N)
    q_coef, z, ood_dev, deep_w, deep = words(Q_WIDTH * N), words(4), words(4 * nterms), words(4 * nterms), words(4 * N)
    layers_all = words(4 * sum(sizes))
    digests = [_lib.toyni_merkle_total_digests(m) for m in sizes]
    levels_all = torch.empty((sum(digests), 32), dtype=torch.uint8, device=dev)
    qidx_dev, acc_rows = words(NUM_QUERIES), words(2 * NUM_QUERIES)
    rounds = len(sizes)
    positions = words(rounds * 2 * NUM_QUERIES)
    plan_shape = opening_plan(N, B, n, [0] * NUM_QUERIES)                     # names, sizes and widths: the indices are the device's
    rec_bytes = [len(ix) * _lib.toyni_merkle_open_rows_record_bytes(t, w) for _, t, w, ix in plan_shape]
    out = torch.empty(sum(rec_bytes), dtype=torch.uint8, device=dev)
    dtr = pv.DeviceTranscript.from_bytes(stream=stream)
    EVENTS.append("transcript loaded")

    # ---- 1. the main columns ----
    main_coef, main_lde, main_salts, main_levels = committed_matrix(vals.data_ptr(), MAIN_WIDTH)
    dtr.absorb_device(main_levels[-1].data_ptr(), 32, stream)

    # ---- 2. gamma and the accumulators under it: Z in columns 0..3, S in 4..7 of one buffer ----
    dtr.squeeze(d_gamma, 4, stream)
    col = lambda c: vals.data_ptr() + 4 * c * n
    pv.column_scan_ext_dc_device(ctx_n, pv.ExtOperandDc(col(0), n, 1, 0), pv.ExtOperandDc(col(1), n, 1, 0), d_gamma, acc.data_ptr(), n, n, 1,
                                 pv.SCAN_PRODUCT, [em.ONE], stream=stream)
    pv.column_scan_ext_dc_device(ctx_n, pv.ExtOperandDc(col(2), n, 1), pv.ExtOperandDc(col(3), n, 1, 0), d_gamma, acc.data_ptr() + 16 * n, n, n, 1,
                                 pv.SCAN_SUM, [em.ZERO], stream=stream)
    acc_coef, acc_lde, acc_salts, acc_levels = committed_matrix(acc.data_ptr(), ACC_WIDTH)
    dtr.absorb_device(acc_levels[-1].data_ptr(), 32, stream)

    # ---- 3. the constraint weights and the quotient: one call ----
    dtr.squeeze(d_alphas, 4 * NUM_WEIGHTS, stream)
    pv.air_quotient_ext_dc_device(ctx_N, prog, [(main_lde.data_ptr(), MAIN_WIDTH, N), (acc_lde.data_ptr(), ACC_WIDTH, N)], log_blowup, COSET_SHIFT,
                                  d_gamma, 4, d_alphas, NUM_WEIGHTS, pv.AIR_WEIGHTS_EMIT_EXT, q.data_ptr(), N, stream=stream)
    q_salts, q_levels = take_salts(N), tree(N)
    toyni_amd.merkle_commit_rows_device(q.data_ptr(), N, Q_WIDTH, COL, N, q_salts.data_ptr(), q_levels.data_ptr(), stream=stream)
    dtr.absorb_device(q_levels[-1].data_ptr(), 32, stream)
    deep_salts, deep_levels = take_salts(N), tree(N)
    salts_all = take_salts(sum(sizes[:-1])) if len(sizes) > 1 else None       # the last layer is committed unsalted

    # ---- 4. z and the out-of-domain values ----
    ctx_N.run_device(q.data_ptr(), q_coef.data_ptr(), Q_WIDTH, True, stream=stream, shift=COSET_SHIFT)
    dtr.squeeze_ext_point(z.data_ptr(), stream)
    pv.poly_eval_ext_batch_dz_device(ctx_n, main_coef.data_ptr(), n, n, MAIN_WIDTH, z.data_ptr(), [1], ood_dev.data_ptr(), stream=stream)
    pv.poly_eval_ext_batch_dz_device(ctx_n, acc_coef.data_ptr(), n, n, ACC_WIDTH, z.data_ptr(), [1, g], ood_dev.data_ptr() + 16 * MAIN_WIDTH, stream=stream)
    pv.poly_eval_ext_batch_dz_device(ctx_N, q_coef.data_ptr(), N, N, Q_WIDTH, z.data_ptr(), [1], ood_dev.data_ptr() + 16 * (MAIN_WIDTH + 2 * ACC_WIDTH),
                                     stream=stream)
    dtr.absorb_fields(ood_dev.data_ptr(), 4 * nterms, stream)

    # ---- 5. the DEEP layer: weight t and value t belong to DEEP_TERMS[t] ----
    dtr.squeeze(deep_w.data_ptr(), 4 * nterms, stream)
    mats = {"main": (main_lde, MAIN_WIDTH), "acc": (acc_lde, ACC_WIDTH), "quotient": (q, Q_WIDTH)}
    for k, (name, (values, width)) in enumerate(mats.items()):
        mine = [(c, r, t, t) for t, (mat, c, r) in enumerate(DEEP_TERMS) if mat == name]
        pv.deep_combine_ext_dz_device(ctx_N, values.data_ptr(), width, N, log_blowup, COSET_SHIFT, z.data_ptr(), deep_w.data_ptr(), ood_dev.data_ptr(),
                                      pv.deep_ext_slots(*zip(*mine)), deep.data_ptr(), accumulate=k > 0, stream=stream)
    toyni_amd.merkle_commit_rows_device(deep.data_ptr(), N, 4, ROW, 0, deep_salts.data_ptr(), deep_levels.data_ptr(), stream=stream)
    dtr.absorb_device(deep_levels[-1].data_ptr(), 32, stream)

    # ---- 6. the fold loop on the device transcript ----
    pv.fri_commit_phase_transcript_ext_device(ctx_N, deep.data_ptr(), N, COSET_SHIFT, B, salts_all.data_ptr() if salts_all is not None else 0, dtr,
                                              layers_all.data_ptr(), levels_all.data_ptr(), 0, stream)

    # ---- 7. queries ----
    dtr.squeeze_indices(qidx_dev.data_ptr(), NUM_QUERIES, N // 2, stream)
    pv.fri_query_positions_device(qidx_dev.data_ptr(), NUM_QUERIES, N, B, positions.data_ptr(), stream)
    pv.query_rows_device(qidx_dev.data_ptr(), NUM_QUERIES, N, [0, B], acc_rows.data_ptr(), stream)
    folded, lo, dlo, slo = {}, 0, 0, 0
    for k, (m, nd) in enumerate(zip(sizes, digests), start=1):
        folded[f"fri{k}"] = (levels_all[dlo:dlo + nd], layers_all[4 * lo:4 * (lo + m)], 4, ROW, salts_all[slo:slo + m] if m != B else None)
        lo, dlo, slo = lo + m, dlo + nd, slo + (m if m != B else 0)
    trees = {"main": (main_levels, main_lde, MAIN_WIDTH, COL, main_salts), "acc": (acc_levels, acc_lde, ACC_WIDTH, COL, acc_salts),
             "quotient": (q_levels, q, Q_WIDTH, COL, q_salts), "deep": (deep_levels, deep, 4, ROW, deep_salts), **folded}
    pair = 4 * 2 * NUM_QUERIES                                               # bytes of one layer's positions
    where = {"main": qidx_dev.data_ptr(), "acc": acc_rows.data_ptr(), "quotient": qidx_dev.data_ptr(), "deep": positions.data_ptr()}
    where.update({f"fri{k}": positions.data_ptr() + k * pair for k in range(1, rounds)})
    boff = 0
    for (name, t, w, ix), sz in zip(plan_shape, rec_bytes):
        levels, values, width, layout, salts = trees[name]
        assert width == w
        toyni_amd.merkle_open_rows_device(levels.data_ptr(), t, values.data_ptr(), w, layout, t if layout == COL else 0, salts.data_ptr(),
                                          where[name], len(ix), out.data_ptr() + boff, stream=stream)
        boff += sz

    # ---- the one synchronisation and the downloads ----
    EVENTS.append("final download")
    torch.cuda.synchronize()
    _, status = dtr.download()
    dtr.free()
    if info is not None:
        info["transcript_status"] = status
    ext_values = lambda t: [tuple(int(c) for c in v) for v in t.cpu().numpy().view(np.uint32).reshape(-1, 4)]
    ood = ext_values(ood_dev)
    ood_main, ood_acc, ood_q = ood[:MAIN_WIDTH], ood[MAIN_WIDTH:MAIN_WIDTH + 2 * ACC_WIDTH], ood[MAIN_WIDTH + 2 * ACC_WIDTH:]
    qidx = [int(v) for v in qidx_dev.cpu().numpy().view(np.uint32)]
    lv = levels_all.cpu().numpy()
    commitments, dlo = [_root(deep_levels)], 0
    for nd in digests:
        commitments.append(lv[dlo + nd - 1].tobytes())
        dlo += nd
    plan = opening_plan(N, B, n, qidx)
    got = np.concatenate([qidx_dev.cpu().numpy(), acc_rows.cpu().numpy(), positions.cpu().numpy()]).view(np.uint32)
    want = np.concatenate([np.asarray(ix, dtype=np.uint32) for name, _, _, ix in plan if name != "quotient"])
    assert (got == want).all(), "the device's opening rows are the protocol's"
    return {
        "trace_len": n, "lde_size": N, "main_commitment": _root(main_levels), "acc_commitment": _root(acc_levels),
        "quotient_commitment": _root(q_levels), "ood_main": ood_main, "ood_acc": ood_acc, "ood_q": ood_q, "q_z": from_columns(ood_q),
        "fri_commitments": commitments, "fri_final_layer": ext_values(layers_all[4 * (sum(sizes) - B):]), "query_indices": qidx,
        "opening_groups": [(t, w, True, ix) for _, t, w, ix in plan], "opening_records": out.cpu().numpy(),
    }
