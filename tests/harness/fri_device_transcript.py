"""The FRI part of a Fibonacci proof with the Fiat-Shamir transcript on the device (include/toyni_hip.h 3l): from the DEEP codeword to
the opening records of every FRI layer without one synchronisation -- commit of layer 0, absorb of its root, the commit phase on the
device transcript, the query indices, their positions in every layer, and all openings in one launch.  The caller hands over what the
transcript has absorbed so far (the two commitments, derive_z's squeezes and the four out-of-domain values live in that state) and
reads everything back with one download at the end.  Test harness: tests/test_gpu_commit_phase_transcript.py holds its outputs to
tests/harness/fib_prover.py byte for byte."""
import numpy as np
import torch

import toyni_amd
from toyni_amd._lib import lib as _lib


def fri_on_device(ctx, deep_u32: np.ndarray, salts_deep: np.ndarray, salts_fri, state: bytes, x0: int, final_size: int, nqueries: int):
    """deep_u32: the DEEP layer (N canonical residues); salts_deep: (N, 16) bytes; salts_fri: (salted leaves, 16) bytes of the folded
    layers back to back, or None; state: the transcript's bytes before layer 0's root is absorbed.
    Returns {"commitments": [root of layer 0, of every folded layer], "final_layer", "indices", "records" (layer 0 first, the final
    layer excluded), "groups": [(n, salted, positions)], "betas", "state" (the transcript afterwards), "status"}."""
    pv = toyni_amd.prover
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    N = int(deep_u32.size)
    sizes, m = [], N
    while m > final_size:
        m //= 2
        sizes.append(m)
    rounds = len(sizes)
    ndig0 = _lib.toyni_merkle_total_digests(N)
    ndigs = [_lib.toyni_merkle_total_digests(h) for h in sizes]
    d_layer0 = torch.from_numpy(np.ascontiguousarray(deep_u32, dtype=np.uint32).view(np.int32)).to(dev)
    d_salts0 = torch.from_numpy(np.ascontiguousarray(salts_deep, dtype=np.uint8)).to(dev)
    d_salts = torch.from_numpy(np.ascontiguousarray(salts_fri, dtype=np.uint8)).to(dev) if salts_fri is not None and len(salts_fri) else None
    levels0 = torch.empty((ndig0, 32), dtype=torch.uint8, device=dev)
    layers = torch.empty(sum(sizes), dtype=torch.int32, device=dev)
    levels = torch.empty((sum(ndigs), 32), dtype=torch.uint8, device=dev)
    betas = torch.empty(rounds, dtype=torch.int32, device=dev)
    indices = torch.empty(nqueries, dtype=torch.int32, device=dev)
    positions = torch.empty(rounds * 2 * nqueries, dtype=torch.int32, device=dev)
    # (tree, n, values, salts) of every layer that is opened: layer 0, then the folded layers but the final one
    opened = [(levels0, N, d_layer0, d_salts0)]
    lo = dlo = slo = 0
    for k, h in enumerate(sizes[:-1]):
        opened.append((levels[dlo:], h, layers[lo:], d_salts[slo:] if d_salts is not None else None))
        lo, dlo, slo = lo + h, dlo + ndigs[k], slo + h
    rec_sizes = [2 * nqueries * pv.merkle_open_record_bytes(n) for _, n, _, _ in opened]
    records = torch.empty(sum(rec_sizes), dtype=torch.uint8, device=dev)
    tr = pv.DeviceTranscript.from_bytes(state, stream)
    # ---- everything below only enqueues ----
    toyni_amd.merkle_commit_device(d_layer0.data_ptr(), d_salts0.data_ptr(), N, levels0.data_ptr(), stream=stream)
    tr.absorb_device(levels0[-1].data_ptr(), 32, stream)
    pv.fri_commit_phase_transcript_device(ctx, d_layer0.data_ptr(), N, x0, final_size, d_salts.data_ptr() if d_salts is not None else 0, tr,
                                          layers.data_ptr(), levels.data_ptr(), betas.data_ptr(), stream)
    tr.squeeze_indices(indices.data_ptr(), nqueries, N // 2, stream)
    pv.fri_query_positions_device(indices.data_ptr(), nqueries, N, final_size, positions.data_ptr(), stream)
    batch, boff = [], 0
    for k, ((tree, n, values, salts), sz) in enumerate(zip(opened, rec_sizes)):
        batch.append((tree.data_ptr(), n, values.data_ptr(), salts.data_ptr() if salts is not None else 0,
                      positions.data_ptr() + 4 * k * 2 * nqueries, 2 * nqueries, records.data_ptr() + boff))
        boff += sz
    pv.merkle_open_groups_device(batch, stream=stream)
    # ---- the one synchronisation: the downloads ----
    torch.cuda.synchronize()
    state_after, status = tr.download()
    tr.free()
    lv = levels.cpu().numpy()
    commitments, dlo = [levels0[-1].cpu().numpy().tobytes()], 0
    for nd in ndigs:
        commitments.append(lv[dlo + nd - 1].tobytes())
        dlo += nd
    pos = positions.cpu().numpy().view(np.uint32).reshape(rounds, 2 * nqueries)
    return {
        "commitments": commitments,
        "final_layer": [int(v) for v in layers[sum(sizes) - final_size:].cpu().numpy().view(np.uint32)],
        "indices": [int(v) for v in indices.cpu().numpy().view(np.uint32)],
        "records": records.cpu().numpy(),
        "groups": [(n, salts is not None, pos[k].tolist()) for k, (_, n, _, salts) in enumerate(opened)],
        "betas": [int(v) for v in betas.cpu().numpy().view(np.uint32)],
        "state": state_after, "status": status,
    }
