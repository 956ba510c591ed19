"""Device prover of the two-column AIR proof -- TEST HARNESS: the caller of the multi-column steps of include/toyni_hip.h 3d / 3e / 3f,
not a product.  The protocol of air_verifier.py; every heavy step is ONE library call on device pointers:

  interpolate, extend     batched inverse transform, toyni_lde_device(batch = 2): the 2 x N column-major matrix
  trace commitment        toyni_merkle_commit_rows_device on that matrix as it lies (col_stride = N)
  quotient                an AirBuilder program run by toyni_air_quotient_device; toyni_merkle_commit_device
  out-of-domain values    inverse coset transform of q; toyni_poly_eval_batch_device (2 columns x 2 points), toyni_poly_eval_device for q(z)
  DEEP layer              toyni_deep_combine_device on the trace matrix, then a second call that accumulates q as a matrix of one column
  FRI                     toyni_fri_commit_phase_device, the transcript behind its callback
  openings                toyni_merkle_open_rows_device for the trace rows, toyni_merkle_open_groups_device for every other tree

The host runs the transcript and nothing else: no field arithmetic on a codeword.  The salts are the pool of air_ref_prover.salt_pool,
uploaded as it is, so that the proof can be compared with air_ref_prover.prove byte for byte."""
import numpy as np
import torch

import toyni_amd
from toyni_amd._lib import lib as _lib

from .air_ref_prover import DEEP_TERMS, layer_sizes, salt_pool
from .air_verifier import NUM_DEEP_WEIGHTS, NUM_QUERIES, NUM_WEIGHTS, opening_plan
from .fib_verifier import COSET_SHIFT, P, Transcript, derive_z, root_of_unity


def constraint_program(n, a_0, b_0):
    """The four constraints of air_verifier.py as AirBuilder expressions."""
    last = pow(root_of_unity(n.bit_length() - 1), n - 1, P)
    bld = toyni_amd.prover.AirBuilder()
    ax, bx, agx, bgx = bld.cell(0, 0, 0), bld.cell(0, 1, 0), bld.cell(0, 0, 1), bld.cell(0, 1, 1)
    bld.emit(0, (agx - bx) * (bld.x() - last))
    bld.emit(1, (bgx - ax * bx - 1) * (bld.x() - last))
    bld.emit(2, (ax - a_0) * bld.xinv(1), divide=False)
    bld.emit(3, (bx - b_0) * bld.xinv(1), divide=False)
    return bld.compile()


def _root(levels: torch.Tensor) -> bytes:
    return bytes(levels[-1].cpu().numpy().tobytes())       # 32 bytes D2H (synchronises the stream)


def prove(cols, log_blowup, seed):
    """The proof in wire form (air_ref_prover.WIRE_FIELDS) of the 2 x n trace `cols` (canonical residues)."""
    pv = toyni_amd.prover
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    cols = np.asarray(cols, dtype=np.uint64)
    n = cols.shape[1]
    assert cols.shape == (2, n) and n >= 2 and n & (n - 1) == 0 and log_blowup >= 1
    B, N = 1 << log_blowup, n << log_blowup
    g = root_of_unity(n.bit_length() - 1)
    a_0, b_0 = int(cols[0, 0]), int(cols[1, 0])
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

    # 1. coefficients of both columns, the column-major LDE, one tree over its rows
    vals = torch.from_numpy(cols.astype(np.uint32).view(np.int32).reshape(-1)).to(dev)
    coef, lde = words(2 * n), words(2 * N)
    ctx_n.run_device(vals.data_ptr(), coef.data_ptr(), 2, True, stream=stream)
    ctx_N.lde_device(coef.data_ptr(), lde.data_ptr(), 2, log_blowup, COSET_SHIFT, stream=stream)
    trace_salts, trace_levels = take_salts(N), tree(N)
    toyni_amd.merkle_commit_rows_device(lde.data_ptr(), N, 2, toyni_amd.ROWS_COLUMN_MAJOR, N, trace_salts.data_ptr(), trace_levels.data_ptr(), stream=stream)
    tr = Transcript()
    trace_commitment = _root(trace_levels)
    tr.absorb(trace_commitment)

    # 2. the quotient under the squeezed weights, its tree
    weights = [tr.squeeze_challenge() for _ in range(NUM_WEIGHTS)]
    q = words(N)
    with pv.AirProgram(ctx_N, constraint_program(n, a_0, b_0)) as prog:
        pv.air_quotient_device(ctx_N, prog, [(lde.data_ptr(), 2, N)], log_blowup, COSET_SHIFT, weights, q.data_ptr(), stream=stream)
        q_salts, q_levels = take_salts(N), tree(N)
        toyni_amd.merkle_commit_device(q.data_ptr(), q_salts.data_ptr(), N, q_levels.data_ptr(), stream=stream)
        quotient_commitment = _root(q_levels)
    tr.absorb(quotient_commitment)

    # 3. z, the out-of-domain values
    q_poly, ood_dev = words(N), words(5)
    ctx_N.run_device(q.data_ptr(), q_poly.data_ptr(), 1, True, stream=stream, shift=COSET_SHIFT)
    z = derive_z(tr, N)
    pv.poly_eval_batch_device(ctx_n, coef.data_ptr(), n, n, 2, [z, g * z % P], ood_dev.data_ptr(), stream=stream)
    pv.poly_eval_device(ctx_N, q_poly.data_ptr(), N, [z], ood_dev.data_ptr() + 16, stream=stream)
    ood = [int(v) for v in ood_dev.cpu().numpy().view(np.uint32)]          # a(z), a(gz), b(z), b(gz), q(z)
    for v in ood:
        tr.absorb_field(v)

    # 4. the DEEP layer: the trace matrix, then the quotient as a second matrix on top
    alphas = [tr.squeeze_challenge() for _ in range(NUM_DEEP_WEIGHTS)]
    deep = words(N)
    t_cols, t_rots = zip(*DEEP_TERMS)
    pv.deep_combine_device(ctx_N, lde.data_ptr(), 2, N, log_blowup, COSET_SHIFT, z, pv.deep_terms(t_cols, t_rots, alphas[:4], ood[:4]), deep.data_ptr(),
                           stream=stream)
    pv.deep_combine_device(ctx_N, q.data_ptr(), 1, N, log_blowup, COSET_SHIFT, z, pv.deep_terms([0], [0], alphas[4:], ood[4:]), deep.data_ptr(),
                           accumulate=True, stream=stream)
    deep_salts, deep_levels = take_salts(N), tree(N)
    toyni_amd.merkle_commit_device(deep.data_ptr(), deep_salts.data_ptr(), N, deep_levels.data_ptr(), stream=stream)
    commitments = [_root(deep_levels)]
    tr.absorb(commitments[0])

    # 5. the fold loop: one call, the transcript behind the callback
    layers_all = words(sum(sizes))
    digests = [_lib.toyni_merkle_total_digests(m) for m in sizes]
    levels_all = torch.empty((sum(digests), 32), dtype=torch.uint8, device=dev)
    salts_all = take_salts(sum(sizes[:-1])) if len(sizes) > 1 else None       # the last layer is committed unsalted

    def challenge(_round, root, want_beta):
        if root is not None:
            commitments.append(root)
            tr.absorb(root)
        return tr.squeeze_challenge() if want_beta else 0

    pv.fri_commit_phase_device(ctx_N, deep.data_ptr(), N, COSET_SHIFT, B, salts_all.data_ptr() if salts_all is not None else 0, challenge,
                               layers_all.data_ptr(), levels_all.data_ptr(), stream=stream)
    folded, lo, dlo, slo = {}, 0, 0, 0
    for k, (m, nd) in enumerate(zip(sizes, digests), start=1):
        folded[f"fri{k}"] = (levels_all[dlo:dlo + nd], m, layers_all[lo:lo + m], salts_all[slo:slo + m] if m != B else None)
        lo, dlo, slo = lo + m, dlo + nd, slo + (m if m != B else 0)
    final_layer = [int(v) for v in layers_all[sum(sizes) - B:].cpu().numpy().view(np.uint32)]

    # 6. queries: the trace rows by the row opener, every other tree's openings in one launch
    qidx = tr.squeeze_indices(NUM_QUERIES, N // 2)
    plan = opening_plan(N, B, n, qidx)
    single = {"quotient": (q_levels, N, q, q_salts), "deep": (deep_levels, N, deep, deep_salts), **folded}
    rec_bytes = [len(ix) * (_lib.toyni_merkle_open_rows_record_bytes(t, w) if name == "trace" else pv.merkle_open_record_bytes(t)) for name, t, w, ix in plan]
    d_idx = torch.from_numpy(np.concatenate([np.asarray(ix, dtype=np.int32) for _, _, _, ix in plan])).to(dev)
    out = torch.empty(sum(rec_bytes), dtype=torch.uint8, device=dev)
    toyni_amd.merkle_open_rows_device(trace_levels.data_ptr(), N, lde.data_ptr(), 2, toyni_amd.ROWS_COLUMN_MAJOR, N, trace_salts.data_ptr(), d_idx.data_ptr(),
                                      len(plan[0][3]), out.data_ptr(), stream=stream)
    ioff, boff, batch = len(plan[0][3]), rec_bytes[0], []
    for (name, t, _w, ix), sz in zip(plan[1:], rec_bytes[1:]):
        levels, leaves, values, salts = single[name]
        assert leaves == t
        batch.append((levels.data_ptr(), t, values.data_ptr(), salts.data_ptr(), d_idx.data_ptr() + 4 * ioff, len(ix), out.data_ptr() + boff))
        ioff, boff = ioff + len(ix), boff + sz
    pv.merkle_open_groups_device(batch, stream=stream)
    records = out.cpu().numpy()
    return {
        "trace_len": n, "lde_size": N, "a_0": a_0, "b_0": b_0, "trace_commitment": trace_commitment, "quotient_commitment": quotient_commitment,
        "a_z": ood[0], "a_gz": ood[1], "b_z": ood[2], "b_gz": ood[3], "q_z": ood[4], "fri_commitments": commitments, "fri_final_layer": final_layer,
        "query_indices": qidx, "opening_groups": [(t, w, True, ix) for _, t, w, ix in plan], "opening_records": records,
    }
