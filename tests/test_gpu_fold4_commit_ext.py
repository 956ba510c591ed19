"""Four-to-one Ext FRI rounds under coset leaves, on the device transcript (include/toyni_hip.h 3m), on the GPU.

* One round (toyni_fri_fold4_commit_ext_device), salted and unsalted, at 1 leaf, 4 leaves, under / exactly / over one workgroup of
  leaves, 1024 leaves (past the 512-digest tail of the node levels) and 4096: against the oracle's pairwise fold applied twice and
  hashlib coset trees, AND against what the existing device calls write (toyni_fri_fold_ext_device twice, then
  toyni_merkle_commit_rows_device on a torch-gathered copy).  Field-edge layers and an edge beta at 2^6 and 2^12.  Input unchanged.
* The grid-stride case: 2^24 elements = 2^20 leaves against the 2^19 threads the launch is capped at, device calls only.
* commit_cosets / open_cosets against commit_rows / open_rows on the gathered copy, hashlib, and tests/rows_common.py's record reader.
* The leaf positions against numpy.
* The phase: byte for byte the per-round calls fed the betas of d_betas; d_betas and the final transcript against a hashlib replay of
  the reference transcript over the roots; a transcript whose status is set (beta = 0, the phase completes); a captured graph of
  absorb + phase + indices + positions replayed twice.
* A low-degree proof end to end at N = 2^8 (tests/harness/fri4_ext_prover.py, one synchronisation), accepted by
  tests/harness/fri4_ext_verifier.py and rejected with one deviation at a time.
Every output up to 2^16 elements lies in guard bands.  Nothing here provokes a fault: what is out of range is refused on the host."""
import numpy as np
import pytest

import ext_model as em
import oracle
import rows_common as rc
import test_emu_transcript as emu
from guarded import edge_residues
from oracle import P

pytestmark = pytest.mark.gpu

ROW = rc.ROW
E_INVALID_SIZE, E_RANGE = 10001, 10006
GRID_THREADS = 256 * 8 * 256          # the cap of the library's grid-stride launches: 8 workgroups of 256 per CU-slot, 256 slots


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build_hip()
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import toyni_amd
    return toyni_amd, torch, torch.device("cuda", 0)


def layer_sizes(m0, final_size):
    out, m = [], m0
    while m > final_size:
        m //= 4
        out.append(m)
    return out


def fold4_oracle(layer, x0, beta):
    """the oracle's pairwise fold twice: (beta, points x0 w_m^i), then (beta^2, points x0^2 w_(m/2)^i)"""
    e = np.asarray(layer, dtype=np.uint64).reshape(-1, 4)
    m = e.shape[0]
    beta2 = em.mul(tuple(int(b) for b in beta), tuple(int(b) for b in beta))
    first = oracle.fri_fold_ext(e, oracle.domain_elements(m, x0), np.array(beta, dtype=np.uint64))
    return oracle.fri_fold_ext(first, oracle.domain_elements(m // 2, x0 * x0 % P), np.array(beta2, dtype=np.uint64))


def to_dev(torch, dev, arr, dtype=np.uint32):
    a = np.ascontiguousarray(arr, dtype=dtype)
    return torch.from_numpy(a.view(np.int32) if dtype == np.uint32 else a).to(dev)


def gathered(t_layer, m):
    """the (m / 4, 16) row-major copy of a device layer whose row j is elements j, j + m/4, j + m/2, j + 3m/4"""
    return t_layer[:4 * m].view(4, m // 4, 4).permute(1, 0, 2).contiguous()


def composed_round(ta, torch, dev, ctx, t_e, m, beta, x0, t_salts):
    """(folded layer, tree) as the EXISTING device calls write them: two pairwise folds, a gather, a row commitment of width 16"""
    lib = ta._lib.lib
    beta2 = em.mul(tuple(int(b) for b in beta), tuple(int(b) for b in beta))
    mid = torch.empty(4 * (m // 2), dtype=torch.int32, device=dev)
    out = torch.empty(4 * (m // 4), dtype=torch.int32, device=dev)
    ta.fri_fold_ext_device(ctx, t_e.data_ptr(), mid.data_ptr(), m, beta, x0)
    ta.fri_fold_ext_device(ctx, mid.data_ptr(), out.data_ptr(), m // 2, beta2, x0 * x0 % P)
    rows = gathered(out, m // 4)
    levels = torch.zeros((lib.toyni_merkle_total_digests(m // 16), 32), dtype=torch.uint8, device=dev)
    ta.merkle_commit_rows_device(rows.data_ptr(), m // 16, 16, ROW, 0, t_salts.data_ptr() if t_salts is not None else 0, levels.data_ptr())
    torch.cuda.synchronize()
    return out, levels


# ---- one round ----
@pytest.mark.parametrize("salted", [True, False])
@pytest.mark.parametrize("log_m", [4, 6, 9, 12, 13, 14, 16])
def test_one_round_equals_the_oracle_hashlib_and_the_composed_device_calls(env, log_m, salted):
    ta, torch, dev = env
    lib, pv = ta._lib.lib, ta.prover
    m = 1 << log_m
    ctx = ta.ntt.get_or_create_ctx(m)
    rng = np.random.default_rng(100 * log_m + salted)
    edgy = log_m in (6, 12)
    e = (edge_residues(4 * m, 7 + log_m) if edgy else rng.integers(0, P, 4 * m)).astype(np.uint64).reshape(m, 4)
    beta = [P - 1, 0, 1, int(rng.integers(0, P))] if edgy else [int(v) for v in rng.integers(0, P, 4)]
    x0 = P - 1 if log_m == 6 else 7
    salts = rng.integers(0, 256, (m // 16, 16), dtype=np.uint8) if salted else None
    ndig = lib.toyni_merkle_total_digests(m // 16)
    with rc.Dev(ta) as d:
        g_e, g_s = d.put(e.astype(np.uint32)), d.put(salts, word=1) if salted else None
        g_out, g_lv = d.buf(16 * (m // 4)), d.buf(32 * ndig, word=1)
        pv.fri_fold4_commit_ext_device(ctx, g_e.ptr, g_out.ptr, m, beta, x0, g_s.ptr if g_s else 0, g_lv.ptr)
        ctx.synchronize()
        got, got_lv = g_out.download().reshape(m // 4, 4), g_lv.download().reshape(ndig, 32)
        assert (g_e.download() == e.astype(np.uint32).reshape(-1)).all()                  # the input layer is read only
    want = fold4_oracle(e, x0, beta)
    assert (got == want).all()
    assert (got_lv == ta.CosetExtMerkleTree(want, salts).flat()).all()
    t_e, t_s = to_dev(torch, dev, e), to_dev(torch, dev, salts, np.uint8) if salted else None
    out2, lv2 = composed_round(ta, torch, dev, ctx, t_e, m, beta, x0, t_s)
    assert (out2.cpu().numpy().view(np.uint32).reshape(m // 4, 4) == got).all()
    assert (lv2.cpu().numpy() == got_lv).all()


@pytest.mark.parametrize("salted", [True, False])
def test_a_thread_takes_a_second_leaf_under_the_launch_cap(env, salted):
    ta, torch, dev = env
    lib, pv = ta._lib.lib, ta.prover
    m = 1 << 24
    assert m // 16 > GRID_THREADS                                              # 2^20 leaves on 2^19 threads
    ctx = ta.ntt.get_or_create_ctx(m)
    gen = torch.Generator(device=dev).manual_seed(24 + salted)
    t_e = torch.randint(0, P, (4 * m,), dtype=torch.int32, device=dev, generator=gen)
    keep = t_e.clone()
    t_s = torch.randint(0, 256, (m // 16, 16), dtype=torch.uint8, device=dev, generator=gen) if salted else None
    beta, x0 = [5, P - 2, 123456789, 1 << 30], 7
    out = torch.full((4 * (m // 4),), -1, dtype=torch.int32, device=dev)
    levels = torch.zeros((lib.toyni_merkle_total_digests(m // 16), 32), dtype=torch.uint8, device=dev)
    pv.fri_fold4_commit_ext_device(ctx, t_e.data_ptr(), out.data_ptr(), m, beta, x0, t_s.data_ptr() if salted else 0, levels.data_ptr())
    out2, lv2 = composed_round(ta, torch, dev, ctx, t_e, m, beta, x0, t_s)
    assert torch.equal(out, out2) and torch.equal(levels, lv2) and torch.equal(t_e, keep)


def test_a_layer_larger_than_the_context_is_refused(env):
    ta, torch, dev = env
    lib = ta._lib.lib
    ctx = ta.NttContext(64, device=dev.index)
    try:
        with rc.Dev(ta) as d:
            g_e, g_out, g_lv, g_b = d.put(np.zeros(4 * 256, dtype=np.uint32)), d.buf(16 * 64), d.buf(32 * 31, word=1), d.buf(64)
            beta = np.array([1, 2, 3, 4], dtype=np.uint32)
            assert lib.toyni_fri_fold4_commit_ext_device(ctx.handle, g_e.ptr, g_out.ptr, 256, beta.ctypes.data, 7, None, g_lv.ptr, None) == E_RANGE
            tr = ta.prover.DeviceTranscript.from_bytes(b"state")
            assert lib.toyni_fri4_commit_phase_transcript_ext_device(ctx.handle, g_e.ptr, 256, 7, 4, None, tr.ptr, g_out.ptr, g_lv.ptr, g_b.ptr,
                                                                     None) == E_INVALID_SIZE
            ctx.synchronize()
            assert tr.download() == (b"state", 0)
            tr.free()
            for g in (g_out, g_lv, g_b):
                assert (g.download(np.uint8) == 0xA5).all()
    finally:
        ctx.destroy()


# ---- the coset tree of a layer as it lies, and its openings ----
@pytest.mark.parametrize("salted", [True, False])
@pytest.mark.parametrize("m", [4, 16, 1 << 10, 1 << 13])
def test_commit_and_open_cosets_equal_rows_on_the_gathered_copy(env, m, salted):
    ta, torch, dev = env
    lib = ta._lib.lib
    n = m // 4
    rng = np.random.default_rng(3 * m + salted)
    e = rng.integers(0, P, (m, 4), dtype=np.uint64)
    salts = rng.integers(0, 256, (n, 16), dtype=np.uint8) if salted else None
    ndig, rec = lib.toyni_merkle_total_digests(n), lib.toyni_merkle_open_rows_record_bytes(n, 16)
    idx33 = np.concatenate([[0, n - 1, 0, n - 1], rng.integers(0, n, 29)]).astype(np.uint32)
    t_rows = gathered(to_dev(torch, dev, e), m)
    t_s = to_dev(torch, dev, salts, np.uint8) if salted else None
    lv2 = torch.zeros((ndig, 32), dtype=torch.uint8, device=dev)
    ta.merkle_commit_rows_device(t_rows.data_ptr(), n, 16, ROW, 0, t_s.data_ptr() if salted else 0, lv2.data_ptr())
    tree = ta.CosetExtMerkleTree(e, salts)
    rows = ta.merkle.coset_rows(e)
    with rc.Dev(ta) as d:
        g_e, g_s = d.put(e.astype(np.uint32)), d.put(salts, word=1) if salted else None
        g_lv = d.buf(32 * ndig, word=1)
        ta.merkle_commit_cosets_ext_device(g_e.ptr, m, g_s.ptr if g_s else 0, g_lv.ptr)
        torch.cuda.synchronize()
        got_lv = g_lv.download().reshape(ndig, 32)
        assert (got_lv == lv2.cpu().numpy()).all() and (got_lv == tree.flat()).all()
        for idx in (idx33, np.array([n - 1], dtype=np.uint32)):
            g_idx, g_out = d.put(idx), d.buf(rec * len(idx), word=1)
            ta.merkle_open_cosets_ext_device(g_lv.ptr, m, g_e.ptr, g_s.ptr if g_s else 0, g_idx.ptr, len(idx), g_out.ptr)
            t_idx = to_dev(torch, dev, idx)
            out2 = torch.full((rec * len(idx),), 0xA5, dtype=torch.uint8, device=dev)
            ta.merkle_open_rows_device(lv2.data_ptr(), n, t_rows.data_ptr(), 16, ROW, 0, t_s.data_ptr() if salted else 0, t_idx.data_ptr(), len(idx),
                                       out2.data_ptr())
            torch.cuda.synchronize()
            raw = g_out.download().tobytes()
            assert raw == out2.cpu().numpy().tobytes()
            for k, index in enumerate(int(i) for i in idx):
                path, salt, vals, flags, pad = rc.split_record(raw[k * rec:(k + 1) * rec], n, 16)
                assert not any(pad) and salt == (salts[index].tobytes() if salted else bytes(16))
                assert vals == rows[index].astype("<u8").tobytes()
                assert flags == [bool((index >> l) & 1) for l in range(rc.depth_of(n))]
                assert rc.verify_merkle_proof(tree.leaf_bytes(index), path, flags, tree.root())
        assert (g_e.download() == e.astype(np.uint32).reshape(-1)).all()


# ---- positions ----
@pytest.mark.parametrize("count", [1, 44])
@pytest.mark.parametrize("m0,final_size", [(1 << 6, 4), (1 << 12, 16), (1 << 20, 1 << 4)])
def test_positions_against_numpy(env, m0, final_size, count):
    ta, torch, dev = env
    rng = np.random.default_rng(m0 + count)
    idx = rng.integers(0, m0 // 4, count).astype(np.uint32)
    idx[0] = m0 // 4 - 1
    rounds = len(layer_sizes(m0, final_size))
    want = np.concatenate([idx % (m0 >> (2 * k + 2)) for k in range(rounds)])
    with rc.Dev(ta) as d:
        g_idx, g_pos = d.put(idx), d.buf(4 * rounds * count)
        ta.prover.fri4_query_positions_device(g_idx.ptr, count, m0, final_size, g_pos.ptr)
        torch.cuda.synchronize()
        assert (g_pos.download() == want).all() and len(want) == rounds * count


# ---- the phase ----
PHASE_SHAPES = [(16, 4), (1 << 6, 4), (1 << 12, 16), (1 << 16, 16)]


def run_phase(ta, d, ctx, e, m0, x0, final_size, salts, tr):
    """the phase into guard-banded buffers; returns (layers words, levels, betas) after a synchronisation"""
    lib, pv = ta._lib.lib, ta.prover
    sizes = layer_sizes(m0, final_size)
    ndig = sum(lib.toyni_merkle_total_digests(s // 4) for s in sizes)
    g_e = d.put(np.ascontiguousarray(e, dtype=np.uint32))
    g_s = d.put(salts, word=1) if salts is not None and len(salts) else None
    g_layers, g_levels, g_betas = d.buf(16 * sum(sizes)), d.buf(32 * ndig, word=1), d.buf(16 * len(sizes))
    pv.fri4_commit_phase_transcript_ext_device(ctx, g_e.ptr, m0, x0, final_size, g_s.ptr if g_s else 0, tr, g_layers.ptr, g_levels.ptr, g_betas.ptr)
    ctx.synchronize()
    assert (g_e.download() == np.ascontiguousarray(e, dtype=np.uint32).reshape(-1)).all()      # layer 0 is read only
    return g_layers.download(), g_levels.download().reshape(ndig, 32), g_betas.download().reshape(len(sizes), 4)


def per_round_calls(ta, d, ctx, e, m0, x0, final_size, salts, betas):
    """the same layers and trees from one toyni_fri_fold4_commit_ext_device call per round, fed `betas`; also returns the roots"""
    lib, pv = ta._lib.lib, ta.prover
    sizes = layer_sizes(m0, final_size)
    layers, levels, roots = [], [], []
    g_cur, m, x, slo = d.put(np.ascontiguousarray(e, dtype=np.uint32)), m0, x0, 0
    for k, s in enumerate(sizes):
        last = k == len(sizes) - 1
        ndig = lib.toyni_merkle_total_digests(s // 4)
        g_s = d.put(salts[slo:slo + s // 4], word=1) if salts is not None and not last else None
        g_out, g_lv = d.buf(16 * s), d.buf(32 * ndig, word=1)
        pv.fri_fold4_commit_ext_device(ctx, g_cur.ptr, g_out.ptr, m, [int(b) for b in betas[k]], x, g_s.ptr if g_s else 0, g_lv.ptr)
        ctx.synchronize()
        layers.append(g_out.download())
        levels.append(g_lv.download().reshape(ndig, 32))
        roots.append(levels[-1][-1].tobytes())
        g_cur, m, x, slo = g_out, s, pow(x, 4, P), slo + (0 if last else s // 4)
    return np.concatenate(layers), np.concatenate(levels), roots


@pytest.mark.parametrize("salted", [True, False])
@pytest.mark.parametrize("m0,final_size", PHASE_SHAPES)
def test_phase_equals_the_per_round_calls_and_the_transcript_replay(env, m0, final_size, salted):
    ta, torch, dev = env
    pv = ta.prover
    ctx = ta.ntt.get_or_create_ctx(m0)
    case = PHASE_SHAPES.index((m0, final_size))
    rng = np.random.default_rng(40 + 2 * case + salted)
    edgy = m0 == 1 << 12
    e = (edge_residues(4 * m0, 60 + case) if edgy else rng.integers(0, P, 4 * m0)).astype(np.uint64).reshape(m0, 4)
    x0 = P - 1 if m0 == 64 else 7
    sizes = layer_sizes(m0, final_size)
    salts = rng.integers(0, 256, (sum(s // 4 for s in sizes[:-1]), 16), dtype=np.uint8) if salted else None
    state0 = emu.pattern([32, 96, 1008 - 32, 46][case], case)
    with rc.Dev(ta) as d:
        tr = pv.DeviceTranscript.from_bytes(state0)
        got_layers, got_levels, got_betas = run_phase(ta, d, ctx, e, m0, x0, final_size, salts, tr)
        state, status = tr.download()
        tr.free()
        want_layers, want_levels, roots = per_round_calls(ta, d, ctx, e, m0, x0, final_size, salts, got_betas)
    assert status == 0
    assert (got_layers == want_layers).all() and (got_levels == want_levels).all()
    # the reference transcript over the roots: four squeezes, then the absorb of the round's root
    t = emu.Model(state0)
    for k, root in enumerate(roots):
        assert got_betas[k].tolist() == t.squeeze(4), k
        t.absorb(root)
    assert state == t.state and len(roots) == len(sizes)
    if m0 <= 1 << 12:                                   # and the direct judge for the first round: the oracle and hashlib
        want = fold4_oracle(e, x0, got_betas[0].tolist())
        assert (got_layers[:4 * sizes[0]].reshape(-1, 4) == want).all()
        nd = ta._lib.lib.toyni_merkle_total_digests(sizes[0] // 4)
        first_salts = salts[:sizes[0] // 4] if salted and len(sizes) > 1 else None
        assert (got_levels[:nd] == ta.CosetExtMerkleTree(want, first_salts).flat()).all()


def test_nothing_to_fold_writes_nothing_and_leaves_the_transcript(env):
    ta, torch, dev = env
    pv = ta.prover
    ctx = ta.ntt.get_or_create_ctx(64)
    state0 = emu.pattern(50, 3)
    with rc.Dev(ta) as d:
        g_e, g_layers, g_levels, g_betas = d.put(np.arange(64 * 4, dtype=np.uint32)), d.buf(1024), d.buf(1024, word=1), d.buf(64)
        tr = pv.DeviceTranscript.from_bytes(state0)
        for m0, fin in ((16, 16), (8, 32), (4, 4)):
            pv.fri4_commit_phase_transcript_ext_device(ctx, g_e.ptr, m0, 7, fin, 0, tr, g_layers.ptr, g_levels.ptr, g_betas.ptr)
        ctx.synchronize()
        assert tr.download() == (state0, 0)
        tr.free()
        for g in (g_layers, g_levels, g_betas):
            assert (g.download(np.uint8) == 0xA5).all()


def test_a_transcript_whose_status_is_set_gives_zero_betas_and_the_phase_completes(env):
    ta, torch, dev = env
    pv = ta.prover
    m0, final_size, x0 = 1 << 6, 4, 7
    ctx = ta.ntt.get_or_create_ctx(m0)
    rng = np.random.default_rng(77)
    e = rng.integers(0, P, (m0, 4), dtype=np.uint64)
    sizes = layer_sizes(m0, final_size)
    salts = rng.integers(0, 256, (sum(s // 4 for s in sizes[:-1]), 16), dtype=np.uint8)
    state0 = emu.pattern(1000, 2)
    with rc.Dev(ta) as d:
        g_root = d.put(np.frombuffer(emu.pattern(32, 1), dtype=np.uint8), word=1)
        tr = pv.DeviceTranscript.from_bytes(state0)
        tr.absorb_device(g_root.ptr, 32)                                         # the caller's own absorb of layer 0's root: 1000 + 32 > 1008
        got_layers, got_levels, got_betas = run_phase(ta, d, ctx, e, m0, x0, final_size, salts, tr)
        assert tr.download() == (state0, E_RANGE)
        tr.free()
        assert (got_betas == 0).all()
        want_layers, want_levels, _ = per_round_calls(ta, d, ctx, e, m0, x0, final_size, salts, np.zeros((len(sizes), 4), dtype=np.uint32))
    assert (got_layers == want_layers).all() and (got_levels == want_levels).all()
    # beta = 0 folds a coset to the average of its four values
    n = m0 // 4
    avg = (e[:n] + e[n:2 * n] + e[2 * n:3 * n] + e[3 * n:]) * pow(4, -1, P) % P
    assert (got_layers[:4 * n].reshape(n, 4) == avg).all()


# ---- captured replay ----
def test_absorb_phase_indices_and_positions_replay_from_one_captured_graph(env):
    ta, torch, dev = env
    lib, pv = ta._lib.lib, ta.prover
    m0, final_size, x0, nq = 1 << 10, 4, 7, 8
    sizes = layer_sizes(m0, final_size)
    rounds = len(sizes)
    ndig = sum(lib.toyni_merkle_total_digests(s // 4) for s in sizes)
    nsalted = sum(s // 4 for s in sizes[:-1])
    ctx = ta.NttContext(m0, device=dev.index)
    rng = np.random.default_rng(9)
    try:
        te = torch.zeros(4 * m0, dtype=torch.int32, device=dev)
        ts = torch.zeros((nsalted, 16), dtype=torch.uint8, device=dev)
        root0 = torch.zeros(32, dtype=torch.uint8, device=dev)
        layers = torch.empty(4 * sum(sizes), dtype=torch.int32, device=dev)
        levels = torch.empty((ndig, 32), dtype=torch.uint8, device=dev)
        betas = torch.empty(4 * rounds, dtype=torch.int32, device=dev)
        idx = torch.empty(nq, dtype=torch.int32, device=dev)
        pos = torch.empty(rounds * nq, dtype=torch.int32, device=dev)
        outs = (layers, levels, betas, idx, pos)
        tr = pv.DeviceTranscript.from_bytes(b"warm")
        s = torch.cuda.Stream(device=dev)

        def call():
            tr.absorb_device(root0.data_ptr(), 32, s.cuda_stream)
            pv.fri4_commit_phase_transcript_ext_device(ctx, te.data_ptr(), m0, x0, final_size, ts.data_ptr(), tr, layers.data_ptr(), levels.data_ptr(),
                                                       betas.data_ptr(), s.cuda_stream)
            tr.squeeze_indices(idx.data_ptr(), nq, m0 // 4, s.cuda_stream)
            pv.fri4_query_positions_device(idx.data_ptr(), nq, m0, final_size, pos.data_ptr(), s.cuda_stream)

        def fresh(rep):
            e = rng.integers(0, P, (m0, 4), dtype=np.uint64)
            salts = rng.integers(0, 256, (nsalted, 16), dtype=np.uint8)
            r0, state0 = emu.pattern(32, 20 + rep), emu.pattern(14 + 40 * rep, rep)
            te.copy_(torch.from_numpy(e.astype(np.uint32).reshape(-1).view(np.int32)))
            ts.copy_(torch.from_numpy(salts)), root0.copy_(torch.from_numpy(np.frombuffer(r0, dtype=np.uint8).copy()))
            return r0, state0

        torch.cuda.synchronize()
        call()                                                                  # eager: the context's record buffer of this stream exists
        ctx.synchronize(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        for rep in range(2):
            r0, state0 = fresh(rep)
            for t in outs:
                t.fill_(-1 if t.dtype == torch.int32 else 0xA5)
            tr.load(state0)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            replayed = [t.clone() for t in outs]
            state_replayed = tr.download()
            # the same calls made eagerly on the same contents: identical bytes
            for t in outs:
                t.fill_(-1 if t.dtype == torch.int32 else 0xA5)
            tr.load(state0)
            torch.cuda.synchronize()
            call()
            ctx.synchronize(s.cuda_stream)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(replayed, outs)), rep
            assert tr.download() == state_replayed and state_replayed[1] == 0, rep
            # and what the reference transcript says about them
            host = emu.Model(state0)
            host.absorb(r0)
            lv = levels.cpu().numpy()
            got_betas, dlo = betas.cpu().numpy().view(np.uint32).reshape(rounds, 4), 0
            for k, sz in enumerate(sizes):
                assert got_betas[k].tolist() == host.squeeze(4), (rep, k)
                dlo += lib.toyni_merkle_total_digests(sz // 4)
                host.absorb(lv[dlo - 1].tobytes())
            want_idx = host.squeeze_indices(nq, m0 // 4)
            assert idx.cpu().numpy().view(np.uint32).tolist() == want_idx, rep
            assert pos.cpu().numpy().view(np.uint32).tolist() == [i % (m0 >> (2 * k + 2)) for k in range(rounds) for i in want_idx], rep
            assert state_replayed == (host.state, 0), rep
        del g
        tr.free()
    finally:
        ctx.destroy()


# ---- end to end: a low-degree proof ----
N_EXT, LOG_BLOWUP, SHIFT, FINAL = 1 << 8, 2, 7, 4


def test_a_low_degree_proof_end_to_end_is_accepted_and_each_deviation_rejected(env):
    ta, torch, dev = env
    from harness import fri4_ext_prover as fp, fri4_ext_verifier as fv
    ctx = ta.ntt.get_or_create_ctx(N_EXT)
    coeffs = np.random.default_rng(8).integers(0, P, (N_EXT >> LOG_BLOWUP, 4), dtype=np.uint64)
    proof, extras = fp.prove(ctx, coeffs, LOG_BLOWUP, SHIFT, FINAL, fv.SEED, fv.NQUERIES, np.random.default_rng(81))
    assert extras["status"] == 0
    # layer 0 is the codeword of the polynomial (tests/ext_model.py on integers, at a few points)
    xs = em.coset_points(N_EXT, SHIFT)
    for i in (0, 1, 77, N_EXT - 1):
        acc = em.ZERO
        for c in reversed(coeffs.tolist()):
            acc = em.add(tuple(a * xs[i] % P for a in acc), tuple(c))
        assert tuple(int(v) for v in extras["layer0"][i]) == acc
    # the device's challenges are the verifier's own: the reference transcript over the roots
    assert (extras["betas"], extras["indices"]) == fv.challenges(proof)
    assert fv.verify(proof) == (True, "accepted")
    assert len(set(proof["final_layer"])) == 1 and len(proof["roots"]) == 3 and len(proof["openings"][0]) == 3
    # ---- one deviation at a time ----
    # a layer-0 codeword of too high a degree: one more coefficient than the folds remove
    def bend(layer0):
        layer0[4 * 21 + 2] = (layer0[4 * 21 + 2] + 1) % P

    bent, _ = fp.prove(ctx, coeffs, LOG_BLOWUP, SHIFT, FINAL, fv.SEED, fv.NQUERIES, np.random.default_rng(81), bend=bend)
    assert fv.verify(bent) == (False, "the final layer is not constant")
    high = np.concatenate([coeffs, np.zeros((N_EXT // 2 - len(coeffs), 4), dtype=np.uint64)])
    high[len(coeffs)] = (1, 0, 0, 0)                                            # degree 64 at blowup 2: not below N / 4
    too_high, _ = fp.prove(ctx, high, LOG_BLOWUP - 1, SHIFT, FINAL, fv.SEED, fv.NQUERIES, np.random.default_rng(81))
    assert too_high["m0"] == N_EXT and fv.verify(too_high) == (False, "the final layer is not constant")
    # a byte of one record: a path digest, the salt, a value, a position flag, the padding
    rec = proof["openings"][3][1]
    depth = rc.depth_of((N_EXT >> 2) // 4)
    for at in (0, 32 * depth - 1, 32 * depth + 3, 32 * depth + 16 + 8 * 5, 32 * depth + 16 + 128, len(rec) - 1):
        bad = dict(proof, openings=[list(q) for q in proof["openings"]])
        bad["openings"][3][1] = rec[:at] + bytes([rec[at] ^ 0x40]) + rec[at + 1:]
        ok, why = fv.verify(bad)
        assert not ok and why.startswith("query 3, layer 1"), (at, why)
    # two records exchanged between queries; a root; the final layer
    bad = dict(proof, openings=[list(q) for q in proof["openings"]])
    bad["openings"][0][0], bad["openings"][1][0] = bad["openings"][1][0], bad["openings"][0][0]
    assert not fv.verify(bad)[0]
    for k in range(3):
        bad = dict(proof, roots=list(proof["roots"]))
        bad["roots"][k] = bytes([bad["roots"][k][0] ^ 2]) + bad["roots"][k][1:]
        assert not fv.verify(bad)[0], k
    assert not fv.verify(dict(proof, root0=bytes(32)))[0]
    assert not fv.verify(dict(proof, final_layer=[em.add(e, em.ONE) for e in proof["final_layer"]]))[0]
    assert not fv.verify(dict(proof, final_layer=proof["final_layer"][:3] + [em.add(proof["final_layer"][3], em.ONE)]))[0]
    # another seed: the challenges are not the device's
    assert not fv.verify(proof, seed=b"another seed")[0]
