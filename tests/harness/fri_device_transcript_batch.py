"""fri_device_transcript.fri_on_device for SEVERAL proofs in one chain of launches (include/toyni_hip.h 3r): the DEEP codewords of
`batch` proofs of one size go in, and the commit of every layer 0, the absorb of its root, the commit phase, the query indices, their
positions and ALL openings of ALL proofs (one toyni_merkle_open_groups_device call) are enqueued once, each launch working on every
proof; one synchronisation, then the downloads.  Every array holds the proofs a stride apart, the strides larger than the extents.
Test harness: tests/test_gpu_fri_batch.py holds each proof's outputs to fri_on_device byte for byte."""
import numpy as np
import torch

import toyni_amd
from toyni_amd._lib import lib as _lib


def fri_on_device_batch(ctx, deeps, salts_deep, salts_fri, states, x0: int, final_size: int, nqueries: int):
    """deeps: per proof the DEEP layer (N canonical residues, one N for all); salts_deep: per proof (N, 16) bytes; salts_fri: per proof
    (salted leaves, 16) bytes; states: per proof the transcript's bytes before layer 0's root is absorbed.
    Returns one dict per proof with the keys of fri_on_device."""
    pv = toyni_amd.prover
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    B, N = len(deeps), int(deeps[0].size)
    sizes, m = [], N
    while m > final_size:
        m //= 2
        sizes.append(m)
    rounds = len(sizes)
    ndig0 = _lib.toyni_merkle_total_digests(N)
    ndigs = [_lib.toyni_merkle_total_digests(h) for h in sizes]
    nsalt = sum(sizes[:-1])
    # strides: words for the u32 arrays, bytes for salts and levels; each leaves a gap behind the proof's extent
    st_l0, st_s0, st_lv0 = N + 8, 16 * N + 32, 32 * ndig0 + 48
    st_ly, st_s, st_lv, st_b = sum(sizes) + 4, 16 * nsalt + 16, 32 * sum(ndigs) + 16, rounds + 3
    st_i, st_p = nqueries + 1, rounds * 2 * nqueries + 2

    def words(stride):
        return torch.full((B * stride,), -1, dtype=torch.int32, device=dev)

    def raw(stride):
        return torch.full((B * stride,), 0xA5, dtype=torch.uint8, device=dev)

    d_layer0, d_salts0, levels0 = words(st_l0), raw(st_s0), raw(st_lv0)
    d_salts, layers, levels, betas = raw(st_s), words(st_ly), raw(st_lv), words(st_b)
    indices, positions = words(st_i), words(st_p)
    for b in range(B):
        d_layer0[b * st_l0:b * st_l0 + N] = torch.from_numpy(np.ascontiguousarray(deeps[b], dtype=np.uint32).view(np.int32)).to(dev)
        d_salts0[b * st_s0:b * st_s0 + 16 * N] = torch.from_numpy(np.ascontiguousarray(salts_deep[b], dtype=np.uint8).reshape(-1)).to(dev)
        d_salts[b * st_s:b * st_s + 16 * nsalt] = torch.from_numpy(np.ascontiguousarray(salts_fri[b], dtype=np.uint8).reshape(-1)).to(dev)
    # (tree offset in bytes, n, values offset in words, salts offset in bytes) inside a proof, per opened layer; layer 0 first
    rec_bytes = [2 * nqueries * pv.merkle_open_record_bytes(n) for n in [N] + sizes[:-1]]
    per_proof = sum(rec_bytes)
    records = torch.empty(B * per_proof, dtype=torch.uint8, device=dev)
    tr = pv.DeviceTranscriptBatch.from_states(states, stream)
    # ---- everything below only enqueues ----
    toyni_amd.merkle_commit_batch_device(d_layer0.data_ptr(), st_l0, d_salts0.data_ptr(), st_s0, N, B, levels0.data_ptr(), st_lv0, stream=stream)
    tr.absorb_device(levels0.data_ptr() + 32 * (ndig0 - 1), st_lv0, 32, stream)
    pv.fri_commit_phase_transcript_batch_device(ctx, d_layer0.data_ptr(), st_l0, N, x0, final_size, d_salts.data_ptr(), st_s, tr, layers.data_ptr(),
                                                st_ly, levels.data_ptr(), st_lv, betas.data_ptr(), st_b, stream)
    tr.squeeze_indices(indices.data_ptr(), st_i, nqueries, N // 2, stream)
    pv.fri_query_positions_batch_device(indices.data_ptr(), st_i, nqueries, N, final_size, B, positions.data_ptr(), st_p, stream)
    groups = []
    for b in range(B):
        off = b * per_proof
        pos_b = positions.data_ptr() + 4 * b * st_p
        groups.append((levels0.data_ptr() + b * st_lv0, N, d_layer0.data_ptr() + 4 * b * st_l0, d_salts0.data_ptr() + b * st_s0, pos_b, 2 * nqueries,
                       records.data_ptr() + off))
        off += rec_bytes[0]
        lo = dlo = slo = 0
        for k, h in enumerate(sizes[:-1]):
            groups.append((levels.data_ptr() + b * st_lv + 32 * dlo, h, layers.data_ptr() + 4 * (b * st_ly + lo), d_salts.data_ptr() + b * st_s + 16 * slo,
                           pos_b + 4 * (k + 1) * 2 * nqueries, 2 * nqueries, records.data_ptr() + off))
            off += rec_bytes[k + 1]
            lo, dlo, slo = lo + h, dlo + ndigs[k], slo + h
    pv.merkle_open_groups_device(groups, stream=stream)
    # ---- the one synchronisation: the downloads ----
    torch.cuda.synchronize()
    after = tr.download()
    tr.free()
    lv0, lv = levels0.cpu().numpy().reshape(B, st_lv0), levels.cpu().numpy().reshape(B, st_lv)
    ly = layers.cpu().numpy().view(np.uint32).reshape(B, st_ly)
    out = []
    for b in range(B):
        commitments, dlo = [lv0[b, 32 * (ndig0 - 1):32 * ndig0].tobytes()], 0
        for nd in ndigs:
            commitments.append(lv[b, 32 * (dlo + nd - 1):32 * (dlo + nd)].tobytes())
            dlo += nd
        pos = positions[b * st_p:b * st_p + rounds * 2 * nqueries].cpu().numpy().view(np.uint32).reshape(rounds, 2 * nqueries)
        out.append({
            "commitments": commitments,
            "final_layer": [int(v) for v in ly[b, sum(sizes) - final_size:sum(sizes)]],
            "indices": [int(v) for v in indices[b * st_i:b * st_i + nqueries].cpu().numpy().view(np.uint32)],
            "records": records[b * per_proof:(b + 1) * per_proof].cpu().numpy(),
            "groups": [(n, True, pos[k].tolist()) for k, n in enumerate([N] + sizes[:-1])],
            "betas": [int(v) for v in betas[b * st_b:b * st_b + rounds].cpu().numpy().view(np.uint32)],
            "state": after[b][0], "status": after[b][1],
        })
    return out
