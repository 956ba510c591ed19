"""The device prover of a low-degree proof under the four-to-one protocol of include/toyni_hip.h 3m, from Ext coefficients to the opening
records with ONE synchronisation: Ext LDE -> coset commitment of layer 0 -> absorb its root -> the commit phase on the device transcript
-> squeeze_indices(max = m0 / 4) -> the leaf every query opens in every layer -> one coset opening call per layer.  Everything up to the
downloads only enqueues.  Test harness: tests/test_gpu_fold4_commit_ext.py hands its proofs to tests/harness/fri4_ext_verifier.py."""
import numpy as np
import torch

import toyni_amd
from toyni_amd._lib import check, lib as _lib


def layer_sizes(m0: int, final_size: int):
    """elements of the folded layers 1 .. R"""
    out, m = [], m0
    while m > final_size:
        m //= 4
        out.append(m)
    return out


def prove(ctx, coeffs4: np.ndarray, log_blowup: int, shift: int, final_size: int, seed: bytes, nqueries: int, rng, bend=None):
    """coeffs4: (ncoeffs, 4) canonical residues, the Ext coefficients of the committed polynomial; bend(layer0 tensor), optional, changes
    the codeword on the device before it is committed (a prover that commits something else than a low-degree word).
    Returns (proof dict for fri4_ext_verifier.verify, {"betas", "indices", "status", "layer0"})."""
    pv, dev = toyni_amd.prover, torch.device("cuda", 0)
    ncoeffs = coeffs4.shape[0]
    m0 = ncoeffs << log_blowup
    sizes = layer_sizes(m0, final_size)
    rounds = len(sizes)
    ndigs = [_lib.toyni_merkle_total_digests(s // 4) for s in sizes]
    tc = torch.from_numpy(np.ascontiguousarray(coeffs4, dtype=np.uint32).reshape(-1).view(np.int32)).to(dev)
    layer0 = torch.empty(4 * m0, dtype=torch.int32, device=dev)
    salts0 = torch.from_numpy(rng.integers(0, 256, (m0 // 4, 16), dtype=np.uint8)).to(dev)
    levels0 = torch.zeros((_lib.toyni_merkle_total_digests(m0 // 4), 32), dtype=torch.uint8, device=dev)
    nsalted = sum(s // 4 for s in sizes[:-1])
    salts = torch.from_numpy(rng.integers(0, 256, (max(nsalted, 1), 16), dtype=np.uint8)).to(dev)
    layers = torch.empty(4 * sum(sizes), dtype=torch.int32, device=dev)
    levels = torch.zeros((sum(ndigs), 32), dtype=torch.uint8, device=dev)
    betas = torch.empty(4 * rounds, dtype=torch.int32, device=dev)
    idx = torch.empty(nqueries, dtype=torch.int32, device=dev)
    pos = torch.empty(rounds * nqueries, dtype=torch.int32, device=dev)
    tr = pv.DeviceTranscript.from_bytes(seed)
    # ---- enqueue everything ----
    check(_lib.toyni_lde_ext_device(ctx.handle, tc.data_ptr(), layer0.data_ptr(), log_blowup, shift, None), "lde ext")
    if bend is not None:
        bend(layer0)
    toyni_amd.merkle_commit_cosets_ext_device(layer0.data_ptr(), m0, salts0.data_ptr(), levels0.data_ptr())
    tr.absorb_device(levels0[-1].data_ptr(), 32)
    pv.fri4_commit_phase_transcript_ext_device(ctx, layer0.data_ptr(), m0, shift, final_size, salts.data_ptr() if nsalted else 0, tr,
                                               layers.data_ptr(), levels.data_ptr(), betas.data_ptr())
    tr.squeeze_indices(idx.data_ptr(), nqueries, m0 // 4)
    pv.fri4_query_positions_device(idx.data_ptr(), nqueries, m0, final_size, pos.data_ptr())
    # (values, tree, salts, elements) of every layer that is opened: layer 0, then the folded layers but the final one
    opened = [(layer0, levels0, salts0, m0)]
    lo = dlo = slo = 0
    for k, s in enumerate(sizes[:-1]):
        opened.append((layers[4 * lo:], levels[dlo:], salts[slo:], s))
        lo, dlo, slo = lo + s, dlo + ndigs[k], slo + s // 4
    outs = []
    for k, (values, tree, s, m) in enumerate(opened):
        rec = _lib.toyni_merkle_open_rows_record_bytes(m // 4, 16)
        out = torch.full((nqueries * rec,), 0xA5, dtype=torch.uint8, device=dev)
        toyni_amd.merkle_open_cosets_ext_device(tree.data_ptr(), m, values.data_ptr(), s.data_ptr(), pos.data_ptr() + 4 * k * nqueries, nqueries,
                                                out.data_ptr())
        outs.append((out, rec))
    torch.cuda.synchronize()                                                    # the one synchronisation
    status = tr.status()
    tr.free()
    openings = [[] for _ in range(nqueries)]
    for out, rec in outs:
        raw = out.cpu().numpy().tobytes()
        for q in range(nqueries):
            openings[q].append(raw[q * rec:(q + 1) * rec])
    lv = levels.cpu().numpy()
    roots, dlo = [], 0
    for nd in ndigs:
        roots.append(lv[dlo + nd - 1].tobytes())
        dlo += nd
    final = layers[4 * (sum(sizes) - final_size):].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(final_size, 4)
    proof = {"m0": m0, "x0": shift, "final_size": final_size, "root0": levels0[-1].cpu().numpy().tobytes(), "roots": roots,
             "final_layer": [tuple(int(v) for v in e) for e in final], "openings": openings}
    extras = {"betas": [tuple(int(v) for v in b) for b in betas.cpu().numpy().view(np.uint32).reshape(rounds, 4)],
              "indices": [int(v) for v in idx.cpu().numpy().view(np.uint32)], "status": status,
              "layer0": layer0.cpu().numpy().view(np.uint32).reshape(m0, 4)}
    return proof, extras
