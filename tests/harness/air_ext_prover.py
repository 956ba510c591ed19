"""Device prover of the staged AIR proof under Ext challenges -- TEST HARNESS: the caller of the sequence include/toyni_hip.h spells out
in 3h and 3i, not a product.  The protocol of air_ext_verifier.py; every heavy step is ONE library call on device pointers:

  main columns            batched inverse transform (batch 4), toyni_lde_device(batch = 4): the 4 x N column-major matrix;
                          toyni_merkle_commit_rows_device on it as it lies (col_stride = N)
  accumulators            toyni_column_scan_ext_device twice (PRODUCT, SUM) into one 8 x n buffer, Z in columns 0..3, S in 4..7; the same
                          inverse transform, LDE and row commitment with batch / width 8
  quotient                an AirBuilder program written with emit_ext (sixteen base constraints), run by FOUR toyni_air_quotient_device
                          calls over [main, accumulators], call c under coordinate c of the Ext weights: the 4 x N matrix q_0..q_3;
                          its row commitment
  out-of-domain values    inverse coset transform of the q columns (batch 4); toyni_poly_eval_ext_batch_device three times: the main
                          coefficients at [z], the accumulators' at [z, g z], q's N coefficients at [z]
  DEEP layer              toyni_deep_combine_ext_device once per matrix, the second and third call accumulating;
                          toyni_merkle_commit_rows_device on the N x 4 row-major result
  FRI                     toyni_fri_commit_phase_ext_device, the transcript behind its callback
  openings                toyni_merkle_open_rows_device, one call per tree (width 4 or 8 column-major; width 4 row-major for the Ext layers)

The host runs the transcript and the recombination q(z) = sum_j X^j q_j(z), nothing else: no field arithmetic on a column or a codeword.
It asserts nothing about the trace, so a false one runs to the end.  The salts are the pool of air_ext_ref_prover.salt_pool, uploaded as
it is, so that the proof can be compared with air_ext_ref_prover.prove byte for byte."""
import numpy as np
import torch

import ext_model as em
import toyni_amd
from toyni_amd._lib import lib as _lib

from .air_ext_ref_prover import salt_pool
from .air_ext_verifier import (ACC_WIDTH, BASIS, DEEP_TERMS, MAIN_WIDTH, NUM_WEIGHTS, NUM_QUERIES, Q_WIDTH, absorb_ext, derive_z, from_columns,
                               opening_plan, squeeze_ext)
from .air_ref_prover import layer_sizes
from .fib_verifier import COSET_SHIFT, P, Transcript, root_of_unity


def constraint_program(gamma):
    """The four Ext constraints of air_ext_verifier.py as AirBuilder expressions: matrix 0 the main columns, matrix 1 the accumulators."""
    bld = toyni_amd.prover.AirBuilder()
    g = bld.ext_const(gamma)
    a, b, u, w = (bld.cell(0, c) for c in range(4))
    zc, zn, sc, sn = bld.ext_cell(1, 0, 0), bld.ext_cell(1, 0, 1), bld.ext_cell(1, 4, 0), bld.ext_cell(1, 4, 1)
    bld.emit_ext(0, zn * (g + b) - zc * (g + a))
    bld.emit_ext(1, (sn - sc) * (g + w) - u)
    bld.emit_ext(2, (zc - 1) * bld.xinv(1), divide=False)
    bld.emit_ext(3, sc * bld.xinv(1), divide=False)
    return bld.compile()


def coordinate_weights(alphas):
    """The base weights of the four quotient calls: base constraint 4 k + j carries coordinate j of Ext constraint k, so call c weighs it
    by coordinate c of alphas[k] X^j."""
    return [[em.mul(a, BASIS[j])[c] for a in alphas for j in range(4)] for c in range(4)]


def _root(levels: torch.Tensor) -> bytes:
    return bytes(levels[-1].cpu().numpy().tobytes())       # 32 bytes D2H (synchronises the stream)


def prove(main, log_blowup, seed):
    """The proof in wire form (air_ext_ref_prover.WIRE_FIELDS) of the 4 x n main trace (canonical residues)."""
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

    def ext_values(t):
        return [tuple(int(c) for c in v) for v in t.cpu().numpy().view(np.uint32).reshape(-1, 4)]

    def committed_matrix(d_columns, width):
        """columns over H -> (coefficients, LDE, salts, tree levels, root) of the width x N column-major matrix."""
        coef, lde = words(width * n), words(width * N)
        ctx_n.run_device(d_columns, coef.data_ptr(), width, True, stream=stream)
        ctx_N.lde_device(coef.data_ptr(), lde.data_ptr(), width, log_blowup, COSET_SHIFT, stream=stream)
        salts, levels = take_salts(N), tree(N)
        toyni_amd.merkle_commit_rows_device(lde.data_ptr(), N, width, COL, N, salts.data_ptr(), levels.data_ptr(), stream=stream)
        return coef, lde, salts, levels, _root(levels)

    # 1. the main columns
    vals = torch.from_numpy(main.astype(np.uint32).view(np.int32).reshape(-1)).to(dev)
    main_coef, main_lde, main_salts, main_levels, main_commitment = committed_matrix(vals.data_ptr(), MAIN_WIDTH)
    tr = Transcript()
    tr.absorb(main_commitment)

    # 2. the accumulators under gamma: Z in columns 0..3, S in 4..7 of one buffer
    gamma = squeeze_ext(tr)
    col = lambda c: vals.data_ptr() + 4 * c * n
    acc = words(ACC_WIDTH * n)
    pv.column_scan_ext_device(ctx_n, pv.ExtOperand(col(0), n, 1, gamma), pv.ExtOperand(col(1), n, 1, gamma), acc.data_ptr(), n, n, 1, pv.SCAN_PRODUCT,
                              [em.ONE], stream=stream)
    pv.column_scan_ext_device(ctx_n, pv.ExtOperand(col(2), n, 1, em.ZERO), pv.ExtOperand(col(3), n, 1, gamma), acc.data_ptr() + 16 * n, n, n, 1,
                              pv.SCAN_SUM, [em.ZERO], stream=stream)
    acc_coef, acc_lde, acc_salts, acc_levels, acc_commitment = committed_matrix(acc.data_ptr(), ACC_WIDTH)
    tr.absorb(acc_commitment)

    # 3. the quotient under four Ext weights: four calls, four base columns
    alphas = [squeeze_ext(tr) for _ in range(NUM_WEIGHTS)]
    q = words(Q_WIDTH * N)
    with pv.AirProgram(ctx_N, constraint_program(gamma)) as prog:
        for c, wts in enumerate(coordinate_weights(alphas)):
            pv.air_quotient_device(ctx_N, prog, [(main_lde.data_ptr(), MAIN_WIDTH, N), (acc_lde.data_ptr(), ACC_WIDTH, N)], log_blowup, COSET_SHIFT, wts,
                                   q.data_ptr() + 4 * c * N, stream=stream)
        q_salts, q_levels = take_salts(N), tree(N)
        toyni_amd.merkle_commit_rows_device(q.data_ptr(), N, Q_WIDTH, COL, N, q_salts.data_ptr(), q_levels.data_ptr(), stream=stream)
        quotient_commitment = _root(q_levels)
    tr.absorb(quotient_commitment)

    # 4. z, the out-of-domain values
    q_coef = words(Q_WIDTH * N)
    ctx_N.run_device(q.data_ptr(), q_coef.data_ptr(), Q_WIDTH, True, stream=stream, shift=COSET_SHIFT)
    z = derive_z(tr)
    gz = tuple(c * g % P for c in z)
    ood_dev = words(4 * len(DEEP_TERMS))
    pv.poly_eval_ext_batch_device(ctx_n, main_coef.data_ptr(), n, n, MAIN_WIDTH, [z], ood_dev.data_ptr(), stream=stream)
    pv.poly_eval_ext_batch_device(ctx_n, acc_coef.data_ptr(), n, n, ACC_WIDTH, [z, gz], ood_dev.data_ptr() + 16 * MAIN_WIDTH, stream=stream)
    pv.poly_eval_ext_batch_device(ctx_N, q_coef.data_ptr(), N, N, Q_WIDTH, [z], ood_dev.data_ptr() + 16 * (MAIN_WIDTH + 2 * ACC_WIDTH), stream=stream)
    ood = ext_values(ood_dev)                                # main, accumulators (column by column: z, g z), q: the order of DEEP_TERMS
    for v in ood:
        absorb_ext(tr, v)
    ood_main, ood_acc, ood_q = ood[:MAIN_WIDTH], ood[MAIN_WIDTH:MAIN_WIDTH + 2 * ACC_WIDTH], ood[MAIN_WIDTH + 2 * ACC_WIDTH:]
    q_z = from_columns(ood_q)

    # 5. the DEEP layer: one call per matrix, the second and third on top of the first; its row commitment
    deep_w = [squeeze_ext(tr) for _ in DEEP_TERMS]
    deep = words(4 * N)
    mats = {"main": (main_lde, MAIN_WIDTH), "acc": (acc_lde, ACC_WIDTH), "quotient": (q, Q_WIDTH)}
    for k, (name, (values, width)) in enumerate(mats.items()):
        mine = [(c, r, wt, val) for (mat, c, r), wt, val in zip(DEEP_TERMS, deep_w, ood) if mat == name]
        terms = pv.deep_ext_terms(*zip(*mine))
        pv.deep_combine_ext_device(ctx_N, values.data_ptr(), width, N, log_blowup, COSET_SHIFT, z, terms, deep.data_ptr(), accumulate=k > 0, stream=stream)
    deep_salts, deep_levels = take_salts(N), tree(N)
    toyni_amd.merkle_commit_rows_device(deep.data_ptr(), N, 4, ROW, 0, deep_salts.data_ptr(), deep_levels.data_ptr(), stream=stream)
    commitments = [_root(deep_levels)]
    tr.absorb(commitments[0])

    # 6. the fold loop: one call, the transcript behind the callback
    layers_all = words(4 * sum(sizes))
    digests = [_lib.toyni_merkle_total_digests(m) for m in sizes]
    levels_all = torch.empty((sum(digests), 32), dtype=torch.uint8, device=dev)
    salts_all = take_salts(sum(sizes[:-1])) if len(sizes) > 1 else None       # the last layer is committed unsalted

    def challenge(_round, root, want_beta):
        if root is not None:
            commitments.append(root)
            tr.absorb(root)
        return squeeze_ext(tr) if want_beta else None

    pv.fri_commit_phase_ext_device(ctx_N, deep.data_ptr(), N, COSET_SHIFT, B, salts_all.data_ptr() if salts_all is not None else 0, challenge,
                                   layers_all.data_ptr(), levels_all.data_ptr(), stream=stream)
    folded, lo, dlo, slo = {}, 0, 0, 0
    for k, (m, nd) in enumerate(zip(sizes, digests), start=1):
        folded[f"fri{k}"] = (levels_all[dlo:dlo + nd], layers_all[4 * lo:4 * (lo + m)], 4, ROW, salts_all[slo:slo + m] if m != B else None)
        lo, dlo, slo = lo + m, dlo + nd, slo + (m if m != B else 0)
    final_layer = ext_values(layers_all[4 * (sum(sizes) - B):])

    # 7. queries: one opener call per tree, the records back to back
    qidx = tr.squeeze_indices(NUM_QUERIES, N // 2)
    plan = opening_plan(N, B, n, qidx)
    trees = {"main": (main_levels, main_lde, MAIN_WIDTH, COL, main_salts), "acc": (acc_levels, acc_lde, ACC_WIDTH, COL, acc_salts),
             "quotient": (q_levels, q, Q_WIDTH, COL, q_salts), "deep": (deep_levels, deep, 4, ROW, deep_salts), **folded}
    rec_bytes = [len(ix) * _lib.toyni_merkle_open_rows_record_bytes(t, w) for _, t, w, ix in plan]
    d_idx = torch.from_numpy(np.concatenate([np.asarray(ix, dtype=np.int32) for _, _, _, ix in plan])).to(dev)
    out = torch.empty(sum(rec_bytes), dtype=torch.uint8, device=dev)
    ioff = boff = 0
    for (name, t, w, ix), sz in zip(plan, rec_bytes):
        levels, values, width, layout, salts = trees[name]
        assert width == w
        toyni_amd.merkle_open_rows_device(levels.data_ptr(), t, values.data_ptr(), w, layout, t if layout == COL else 0, salts.data_ptr(),
                                          d_idx.data_ptr() + 4 * ioff, len(ix), out.data_ptr() + boff, stream=stream)
        ioff, boff = ioff + len(ix), boff + sz
    records = out.cpu().numpy()
    return {
        "trace_len": n, "lde_size": N, "main_commitment": main_commitment, "acc_commitment": acc_commitment, "quotient_commitment": quotient_commitment,
        "ood_main": ood_main, "ood_acc": ood_acc, "ood_q": ood_q, "q_z": q_z, "fri_commitments": commitments, "fri_final_layer": final_layer,
        "query_indices": qidx, "opening_groups": [(t, w, True, ix) for _, t, w, ix in plan], "opening_records": records,
    }
