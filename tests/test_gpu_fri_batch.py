"""The batch dimension of the tail (include/toyni_hip.h 3r) on the GPU.  The specification is one sentence -- every batched call
writes, for proof b, exactly the bytes the single call writes when given proof b's pointers -- and two judges hold every case to it:

  (i)  `batch` single calls of the existing entry points on the same inputs, byte for byte in layers, levels, betas, indices,
       positions and every final transcript and status;
  (ii) for the shapes up to 2^12, the oracle fold, hashlib trees and the Python transcript (tests/test_emu_transcript.Model).

Every array holds the proofs a stride apart in ONE guard-banded buffer (tests/guarded.py) with the strides larger than the extents,
so the gaps between the proofs are guard bands too: after a call every byte outside the proofs' extents is still the sentinel.
Trees at n = 1, 2, 3, 512, 513, 1025, 2^15 + 2; both phases at m0 -> final = 2 -> 1, 2^6 -> 4, 2^11 -> 16, 2^12 -> 1 with 1, 3 and 5
proofs, salted and unsalted, initial states of 32, 55, 96 and 976 bytes in one batch, field-edge layers at 2^6; the same with
TOYNI_FRI_TAIL_LOG=-1 in a child process; a transcript of the batch that overflowed before the phase; indices and positions; strides
beyond 2^32 bytes; a captured graph replayed twice; and the FRI part of three Fibonacci proofs in one chain, each accepted by the
verifier, a mixture of two of them rejected."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import rows_common as rc
import test_emu_transcript as emu
from guarded import edge_residues
from oracle import P

pytestmark = pytest.mark.gpu

E_RANGE = 10006
STATES = [32, 55, 96, 976]          # 55: the SHA-256 one-block / two-block seam; 976 = capacity - 32: room for exactly one more root
PHASES = [(1, 1), (6, 4), (11, 16), (12, 1)]      # (log2 m0, final_size): tail only; a launched round handing over to the fused rounds (2)


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build_hip()
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import toyni_amd
    return toyni_amd, torch, torch.device("cuda", 0)


def halves_of(m0, final_size):
    sizes, m = [], m0
    while m > final_size:
        m //= 2
        sizes.append(m)
    return sizes


def tree_of(layer, words, salts):
    levels = rc.hashlib_levels(rc.leaves_of(np.asarray(layer, dtype=np.uint64).reshape(-1, words), salts))
    return np.frombuffer(b"".join(d for level in levels for d in level), dtype=np.uint8).reshape(-1, 32)


class Arena:
    """`batch` regions of `extent` bytes, `stride` bytes apart, in one guard-banded buffer that starts as sentinel bytes throughout."""

    def __init__(self, d, batch, extent, stride):
        assert stride > extent or batch == 1 and stride >= extent
        self.batch, self.extent, self.stride = batch, extent, stride
        self.g = d.buf((batch - 1) * stride + extent, word=1)
        self.ptr = self.g.ptr

    def put(self, b, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == self.extent
        self.g.upload(arr.view(np.uint8).reshape(-1), offset=b * self.stride)

    def get(self, dtype=np.uint8):
        """the proofs' regions; everything between them must still be the sentinel"""
        raw = self.g.download(np.uint8)
        mask = np.ones(raw.size, dtype=bool)
        out = []
        for b in range(self.batch):
            lo = b * self.stride
            mask[lo:lo + self.extent] = False
            out.append(raw[lo:lo + self.extent].copy().view(dtype))
        assert (raw[mask] == 0xA5).all(), "a gap between two proofs was written"
        return out


# ---- trees ----
TREE_SIZES = [1, 2, 3, 512, 513, 1025, (1 << 15) + 2]


@pytest.mark.parametrize("salted", [True, False])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", TREE_SIZES)
def test_trees_equal_the_single_call_and_hashlib(env, n, batch, salted):
    ta, torch, dev = env
    lib = ta._lib.lib
    rng = np.random.default_rng(n * 10 + batch * 2 + salted)
    ndig = lib.toyni_merkle_total_digests(n)
    vals = [edge_residues(n, 7 + b) if n >= 16 else rng.integers(0, P, n, dtype=np.uint64).astype(np.uint32) for b in range(batch)]
    salts = [rng.integers(0, 256, (n, 16), dtype=np.uint8) for _ in range(batch)] if salted else None
    with rc.Dev(ta) as d:
        a_v, a_s, a_l = Arena(d, batch, 4 * n, 4 * (n + 5)), Arena(d, batch, 16 * n, 16 * n + 32), Arena(d, batch, 32 * ndig, 32 * ndig + 48)
        for b in range(batch):
            a_v.put(b, vals[b])
            if salted:
                a_s.put(b, salts[b])
        ta.merkle_commit_batch_device(a_v.ptr, n + 5, a_s.ptr if salted else 0, 16 * n + 32 if salted else 0, n, batch, a_l.ptr, 32 * ndig + 48)
        singles = []
        for b in range(batch):
            g_v, g_s, g_l = d.put(vals[b]), d.put(salts[b], word=1) if salted else None, d.buf(32 * ndig, word=1)
            ta.merkle_commit_device(g_v.ptr, g_s.ptr if salted else 0, n, g_l.ptr)
            singles.append(g_l)
        ta.ntt.get_or_create_ctx(16).synchronize()
        got = a_l.get()
        for b in range(batch):
            assert (got[b] == singles[b].download(np.uint8)).all(), b
            if n <= 1 << 12:
                assert (got[b].reshape(-1, 32) == tree_of(vals[b], 1, salts[b] if salted else None)).all(), b
        assert all((x == y.view(np.uint8).reshape(-1)).all() for x, y in zip(a_v.get(), vals))        # inputs are read only


# ---- the phases ----
def phase_inputs(words, log_m0, final_size, batch, salted, edgy=False):
    m0 = 1 << log_m0
    sizes = halves_of(m0, final_size)
    rng = np.random.default_rng(100000 * words + 1000 * log_m0 + 10 * batch + salted)
    es = [(edge_residues(words * m0, 40 + b) if edgy else rng.integers(0, P, words * m0)).astype(np.uint64).reshape(m0, words) for b in range(batch)]
    salts = [rng.integers(0, 256, (sum(sizes[:-1]), 16), dtype=np.uint8) for _ in range(batch)] if salted and sum(sizes[:-1]) else None
    states = [emu.pattern(STATES[b % 4], 3 * b + log_m0) for b in range(batch)]
    return es, salts, states


def batch_phase(ta, d, ctx, words, m0, x0, final_size, es, salts, states, pre_absorb=None):
    """The batched call on proofs a stride apart.  Returns per proof {"layers", "levels", "betas", "state", "status"}."""
    lib, pv = ta._lib.lib, ta.prover
    batch = len(es)
    sizes = halves_of(m0, final_size)
    ndig = sum(lib.toyni_merkle_total_digests(h) for h in sizes)
    nsalt = sum(sizes[:-1])
    gap_w = 4 if words == 4 else 5                   # the Ext call wants 16-byte layers; the base call takes any word stride
    x_l0, x_ly, x_s, x_lv, x_b = 4 * words * m0, 4 * words * sum(sizes), 16 * nsalt, 32 * ndig, 4 * words * len(sizes)
    a_e, a_ly = Arena(d, batch, x_l0, x_l0 + 4 * gap_w), Arena(d, batch, x_ly, x_ly + 4 * gap_w)
    a_s, a_lv, a_b = Arena(d, batch, x_s, x_s + 32), Arena(d, batch, x_lv, x_lv + 48), Arena(d, batch, x_b, x_b + 12)
    for b in range(batch):
        a_e.put(b, es[b].astype(np.uint32))
        if salts is not None:
            a_s.put(b, salts[b])
    tr = pv.DeviceTranscriptBatch.from_states(states)
    if pre_absorb is not None:
        a_r = Arena(d, batch, 32, 40)
        for b in range(batch):
            a_r.put(b, np.frombuffer(pre_absorb, dtype=np.uint8))
        tr.absorb_device(a_r.ptr, 40, 32)
    entry = pv.fri_commit_phase_transcript_ext_batch_device if words == 4 else pv.fri_commit_phase_transcript_batch_device
    entry(ctx, a_e.ptr, a_e.stride // 4, m0, x0, final_size, a_s.ptr if salts is not None else 0, a_s.stride if salts is not None else 0, tr,
          a_ly.ptr, a_ly.stride // 4, a_lv.ptr, a_lv.stride, a_b.ptr, a_b.stride // 4)
    ctx.synchronize()
    after = tr.download()
    tr.free()
    layers, levels, betas = a_ly.get(np.uint32), a_lv.get(), a_b.get(np.uint32)
    assert all((x == e.astype(np.uint32).reshape(-1)).all() for x, e in zip(a_e.get(np.uint32), es))     # layer 0 is read only
    return [{"layers": layers[b], "levels": levels[b].reshape(-1, 32), "betas": betas[b].tolist(), "state": after[b][0], "status": after[b][1]}
            for b in range(batch)]


def single_phase(ta, d, ctx, words, m0, x0, final_size, e, salts, state0, pre_absorb=None):
    lib, pv = ta._lib.lib, ta.prover
    sizes = halves_of(m0, final_size)
    ndig = sum(lib.toyni_merkle_total_digests(h) for h in sizes)
    g_e = d.put(e.astype(np.uint32))
    g_s = d.put(salts, word=1) if salts is not None else None
    g_layers, g_levels, g_betas = d.buf(4 * words * sum(sizes)), d.buf(32 * ndig, word=1), d.buf(4 * words * len(sizes))
    tr = pv.DeviceTranscript.from_bytes(state0)
    if pre_absorb is not None:
        tr.absorb_device(d.put(np.frombuffer(pre_absorb, dtype=np.uint8), word=1).ptr, 32)
    entry = pv.fri_commit_phase_transcript_ext_device if words == 4 else pv.fri_commit_phase_transcript_device
    entry(ctx, g_e.ptr, m0, x0, final_size, g_s.ptr if g_s else 0, tr, g_layers.ptr, g_levels.ptr, g_betas.ptr)
    ctx.synchronize()
    state, status = tr.download()
    tr.free()
    return {"layers": g_layers.download(), "levels": g_levels.download().reshape(-1, 32), "betas": g_betas.download().tolist(), "state": state,
            "status": status}


def same(a, b):
    return (a["betas"] == b["betas"] and a["state"] == b["state"] and a["status"] == b["status"] and (a["layers"] == b["layers"]).all() and
            (a["levels"] == b["levels"]).all())


def replay(lib, words, e, m0, x0, final_size, salts, state0, got):
    """judge (ii): the reference transcript, the oracle's fold on the squared domain, hashlib trees (the last one unsalted)"""
    t = emu.Model(state0)
    sizes = halves_of(m0, final_size)
    got_layers, got_levels = got["layers"].astype(np.uint64).reshape(-1, words), got["levels"]
    cur, x, lo, dlo, slo = e, x0, 0, 0, 0
    for k, h in enumerate(sizes):
        beta = t.squeeze(words)
        assert got["betas"][words * k:words * (k + 1)] == beta, k
        xs = oracle.domain_elements(2 * h, x)
        if words == 4:
            want = oracle.fri_fold_ext(cur, xs, np.array(beta, dtype=np.uint64))
        else:
            want = oracle.fri_fold(cur.reshape(-1), xs, beta[0]).reshape(-1, 1)
        assert (got_layers[lo:lo + h] == want).all(), k
        s = salts[slo:slo + h] if salts is not None and k < len(sizes) - 1 else None
        nd = lib.toyni_merkle_total_digests(h)
        tree = tree_of(want, words, s)
        assert (got_levels[dlo:dlo + nd] == tree).all(), k
        t.absorb(tree[-1].tobytes())
        cur, x, lo, dlo, slo = want, x * x % P, lo + h, dlo + nd, slo + (h if s is not None else 0)
    assert (got["state"], got["status"]) == (t.state, t.status)


@pytest.mark.parametrize("salted", [True, False])
@pytest.mark.parametrize("batch", [1, 3, 5])
@pytest.mark.parametrize("words", [1, 4])
@pytest.mark.parametrize("log_m0,final_size", PHASES)
def test_phases_equal_the_single_calls_and_the_cpu_replay(env, log_m0, final_size, words, batch, salted):
    ta, torch, dev = env
    m0 = 1 << log_m0
    ctx = ta.ntt.get_or_create_ctx(max(m0, 2))
    x0 = P - 1 if log_m0 == 6 else 7
    es, salts, states = phase_inputs(words, log_m0, final_size, batch, salted, edgy=log_m0 == 6)
    with rc.Dev(ta) as d:
        got = batch_phase(ta, d, ctx, words, m0, x0, final_size, es, salts, states)
        for b in range(batch):
            one = single_phase(ta, d, ctx, words, m0, x0, final_size, es[b], salts[b] if salts is not None else None, states[b])
            assert same(got[b], one), b
            assert len(got[b]["betas"]) == words * log_m0 - words * (final_size.bit_length() - 1)
    for b in range(batch):
        replay(ta._lib.lib, words, es[b], m0, x0, final_size, salts[b] if salts is not None else None, states[b], got[b])
        assert got[b]["status"] == 0, b           # (a squeeze leaves a 32-byte state: 976 bytes is the longest that starts a phase)


def phase_digests(ta):
    """sha256 over everything the batched phases leave for three proofs, per (shape, element type, salted)"""
    out = {}
    for log_m0, final_size in PHASES:
        m0 = 1 << log_m0
        ctx = ta.ntt.get_or_create_ctx(max(m0, 2))
        for words in (1, 4):
            for salted in (True, False):
                es, salts, states = phase_inputs(words, log_m0, final_size, 3, salted)
                with rc.Dev(ta) as d:
                    got = batch_phase(ta, d, ctx, words, m0, 7, final_size, es, salts, states)
                h = hashlib.sha256()
                for g in got:
                    for part in (g["layers"].tobytes(), g["levels"].tobytes(), np.array(g["betas"], dtype=np.uint32).tobytes(), g["state"],
                                 bytes([g["status"] & 0xFF])):
                        h.update(part)
                out["%d %d %d %d" % (log_m0, final_size, words, salted)] = h.hexdigest()
    return out


def test_the_launched_path_alone_gives_the_same_bytes(env):
    """A child process (the knob is read once per process) with TOYNI_FRI_TAIL_LOG=-1: no fused launch, every round a fold, the tree
    levels and a one-wave transcript step, each on all three proofs.  The fused default of this process must have written the same."""
    ta, torch, dev = env
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child_env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests"), os.path.join(root, "tests", "_hooks")]),
                     TOYNI_FRI_TAIL_LOG="-1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, env=child_env, cwd=root)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    lines = [l.split() for l in res.stdout.split("\n") if l.startswith("PHASE ")]
    tails = [l for l in res.stdout.split("\n") if l.startswith("TAIL ")]
    assert tails == ["TAIL 0"], res.stdout[-1500:]
    child = {" ".join(l[1:5]): l[5] for l in lines}
    want = phase_digests(ta)
    assert len(want) == 16 and child == want
    assert any("fri_tail_rounds_batch_kernel" in k for k in ta._lib.launched_kernels())          # this process took the fused launch


@pytest.mark.parametrize("words", [1, 4])
def test_a_transcript_that_overflowed_before_the_phase_does_not_touch_its_neighbours(env, words):
    """Proof 1's transcript holds 1000 bytes: the caller's absorb of layer 0's root overflows it.  Its beta is 0 in every round, its
    status set, its layers (the averages) and trees still written; proofs 0 and 2 equal their single calls."""
    ta, torch, dev = env
    lib = ta._lib.lib
    m0, final_size, x0 = 1 << 6, 4, 7
    ctx = ta.ntt.get_or_create_ctx(m0)
    es, salts, states = phase_inputs(words, 6, final_size, 3, True)
    states = [states[0], emu.pattern(1000, 2), states[2]]
    root = emu.pattern(32, 1)
    with rc.Dev(ta) as d:
        got = batch_phase(ta, d, ctx, words, m0, x0, final_size, es, salts, states, pre_absorb=root)
        ones = [single_phase(ta, d, ctx, words, m0, x0, final_size, es[b], salts[b], states[b], pre_absorb=root) for b in range(3)]
    assert all(same(g, o) for g, o in zip(got, ones))
    assert [g["status"] for g in got] == [0, E_RANGE, 0] and got[1]["state"] == states[1] and got[1]["betas"] == [0] * (4 * words)
    for b in (0, 2):                                 # the neighbours against the model, their transcripts having absorbed the root
        assert any(got[b]["betas"])
        replay(lib, words, es[b], m0, x0, final_size, salts[b], states[b] + root, got[b])
    sizes = halves_of(m0, final_size)
    cur, lo, dlo = es[1], 0, 0
    layers, levels = got[1]["layers"].astype(np.uint64).reshape(-1, words), got[1]["levels"]
    for k, h in enumerate(sizes):
        want = (cur[:h] + cur[h:]) * ((P + 1) // 2) % P
        nd = lib.toyni_merkle_total_digests(h)
        s = salts[1][sum(sizes[:k]):sum(sizes[:k]) + h] if k < len(sizes) - 1 else None
        assert (layers[lo:lo + h] == want).all() and (levels[dlo:dlo + nd] == tree_of(want, words, s)).all()
        cur, lo, dlo = want, lo + h, dlo + nd


# ---- indices and positions ----
@pytest.mark.parametrize("count,mx_is_count", [(1, True), (1, False), (80, True), (80, False)])
def test_indices_and_positions_equal_the_single_calls_and_the_model(env, count, mx_is_count):
    ta, torch, dev = env
    pv = ta.prover
    m0, final_size, batch = 1 << 10, 4, 3
    mx = count if mx_is_count else m0 // 2
    rounds = len(halves_of(m0, final_size))
    states = [emu.pattern(STATES[b], 11 + b) for b in range(batch)] + [emu.pattern(60, 9)]
    batch += 1
    with rc.Dev(ta) as d:
        a_i, a_p = Arena(d, batch, 4 * count, 4 * count + 4), Arena(d, batch, 4 * rounds * 2 * count, 4 * rounds * 2 * count + 8)
        tr = pv.DeviceTranscriptBatch.from_states(states)
        # the last transcript's status is set: zeros, the state as it was, and the neighbours as if it were not there
        host = np.zeros(1024, dtype=np.uint8)
        host[:8] = np.array([60, E_RANGE], dtype=np.uint32).view(np.uint8)
        host[16:76] = np.frombuffer(states[-1], dtype=np.uint8)
        ta._lib.check(ta._lib.lib.toyni_memcpy_h2d(tr.ptr + 1024 * (batch - 1), host.ctypes.data, 1024), "upload")
        tr.squeeze_indices(a_i.ptr, count + 1, count, mx)
        pv.fri_query_positions_batch_device(a_i.ptr, count + 1, count, m0, final_size, batch, a_p.ptr, rounds * 2 * count + 2)
        ones = []
        for b in range(batch - 1):
            t1 = pv.DeviceTranscript.from_bytes(states[b])
            g_i, g_p = d.buf(4 * count), d.buf(4 * rounds * 2 * count)
            t1.squeeze_indices(g_i.ptr, count, mx)
            pv.fri_query_positions_device(g_i.ptr, count, m0, final_size, g_p.ptr)
            ones.append((t1, g_i, g_p))
        ta.ntt.get_or_create_ctx(16).synchronize()
        after = tr.download()
        tr.free()
        idx, pos = a_i.get(np.uint32), a_p.get(np.uint32)
        for b, (t1, g_i, g_p) in enumerate(ones):
            assert (idx[b] == g_i.download()).all() and (pos[b] == g_p.download()).all() and after[b] == t1.download(), b
            t1.free()
            model = emu.Model(states[b])
            want = model.squeeze_indices(count, mx)
            assert idx[b].tolist() == want and pos[b].tolist() == emu.query_positions(want, m0, final_size) and after[b] == (model.state, 0)
        assert after[-1] == (states[-1], E_RANGE) and (idx[-1] == 0).all() and (pos[-1] == emu.query_positions([0] * count, m0, final_size)).all()


# ---- offsets beyond 2^32 ----
def test_strides_beyond_four_gibibytes(env):
    """Two proofs whose trees lie 2^32 + 64 bytes apart, in one uninitialised allocation with guard bands around the two regions
    only: every offset is formed in 64 bits."""
    ta, torch, dev = env
    lib, pv = ta._lib.lib, ta.prover
    m0, final_size, x0, G = 1 << 6, 4, 7, 1 << 16
    sizes = halves_of(m0, final_size)
    ndig = sum(lib.toyni_merkle_total_digests(h) for h in sizes)
    stride = (1 << 32) + 64
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > stride + (1 << 28), "the case needs 4 GiB of free device memory"
    ctx = ta.ntt.get_or_create_ctx(m0)
    es, salts, states = phase_inputs(1, 6, final_size, 2, True)
    big = torch.empty(G + stride + 32 * ndig + G, dtype=torch.uint8, device=dev)
    try:
        for b in range(2):
            big[b * stride:b * stride + 2 * G + 32 * ndig].fill_(0xA5)
        nsalt = sum(sizes[:-1])
        te = torch.full((2 * (m0 + 4),), -1, dtype=torch.int32, device=dev)
        ts = torch.full((2 * (16 * nsalt + 16),), 0xA5, dtype=torch.uint8, device=dev)
        for b in range(2):
            te[b * (m0 + 4):b * (m0 + 4) + m0] = torch.from_numpy(es[b].astype(np.uint32).reshape(-1).view(np.int32)).to(dev)
            ts[b * (16 * nsalt + 16):b * (16 * nsalt + 16) + 16 * nsalt] = torch.from_numpy(salts[b].reshape(-1)).to(dev)
        layers = torch.full((2 * (sum(sizes) + 1),), -1, dtype=torch.int32, device=dev)
        betas = torch.full((2 * (len(sizes) + 1),), -1, dtype=torch.int32, device=dev)
        tr = pv.DeviceTranscriptBatch.from_states(states)
        pv.fri_commit_phase_transcript_batch_device(ctx, te.data_ptr(), m0 + 4, m0, x0, final_size, ts.data_ptr(), 16 * nsalt + 16, tr, layers.data_ptr(),
                                                    sum(sizes) + 1, big.data_ptr() + G, stride, betas.data_ptr(), len(sizes) + 1)
        # the roots, through the same stride
        tr2 = pv.DeviceTranscriptBatch.from_states([b"", b""])
        tr2.absorb_device(big.data_ptr() + G + 32 * (ndig - 1), stride, 32)
        torch.cuda.synchronize()
        after, roots = tr.download(), tr2.download()
        tr.free(), tr2.free()
        with rc.Dev(ta) as d:
            for b in range(2):
                one = single_phase(ta, d, ctx, 1, m0, x0, final_size, es[b], salts[b], states[b])
                region = big[b * stride:b * stride + 2 * G + 32 * ndig].cpu().numpy()
                assert (region[:G] == 0xA5).all() and (region[G + 32 * ndig:] == 0xA5).all(), b
                assert (region[G:G + 32 * ndig].reshape(-1, 32) == one["levels"]).all(), b
                assert (layers[b * (sum(sizes) + 1):][:sum(sizes)].cpu().numpy().view(np.uint32) == one["layers"]).all(), b
                assert after[b] == (one["state"], 0) and roots[b] == (one["levels"][-1].tobytes(), 0), b
    finally:
        del big
        torch.cuda.empty_cache()


# ---- captured replay ----
def test_commit_absorb_phase_indices_and_positions_replay_from_one_captured_graph(env):
    ta, torch, dev = env
    lib, pv = ta._lib.lib, ta.prover
    m0, final_size, x0, nq, B = 1 << 10, 4, 7, 8, 3
    sizes = halves_of(m0, final_size)
    rounds = len(sizes)
    ndig0, ndig = lib.toyni_merkle_total_digests(m0), sum(lib.toyni_merkle_total_digests(h) for h in sizes)
    nsalt = sum(sizes[:-1])
    st_e, st_s0, st_lv0, st_s, st_ly, st_lv, st_b, st_i, st_p = (m0 + 4, 16 * m0 + 16, 32 * ndig0 + 32, 16 * nsalt + 16, sum(sizes) + 4, 32 * ndig + 16,
                                                                 rounds + 1, nq + 2, rounds * 2 * nq + 3)
    ctx = ta.NttContext(m0, device=dev.index)
    rng = np.random.default_rng(19)
    try:
        te = torch.zeros(B * st_e, dtype=torch.int32, device=dev)
        ts0, ts = torch.zeros(B * st_s0, dtype=torch.uint8, device=dev), torch.zeros(B * st_s, dtype=torch.uint8, device=dev)
        levels0, levels = torch.empty(B * st_lv0, dtype=torch.uint8, device=dev), torch.empty(B * st_lv, dtype=torch.uint8, device=dev)
        layers, betas = torch.empty(B * st_ly, dtype=torch.int32, device=dev), torch.empty(B * st_b, dtype=torch.int32, device=dev)
        idx, pos = torch.empty(B * st_i, dtype=torch.int32, device=dev), torch.empty(B * st_p, dtype=torch.int32, device=dev)
        tr = pv.DeviceTranscriptBatch.from_states([b"warm"] * B)
        s = torch.cuda.Stream(device=dev)

        def call():
            ta.merkle_commit_batch_device(te.data_ptr(), st_e, ts0.data_ptr(), st_s0, m0, B, levels0.data_ptr(), st_lv0, stream=s.cuda_stream)
            tr.absorb_device(levels0.data_ptr() + 32 * (ndig0 - 1), st_lv0, 32, s.cuda_stream)
            pv.fri_commit_phase_transcript_batch_device(ctx, te.data_ptr(), st_e, m0, x0, final_size, ts.data_ptr(), st_s, tr, layers.data_ptr(), st_ly,
                                                        levels.data_ptr(), st_lv, betas.data_ptr(), st_b, s.cuda_stream)
            tr.squeeze_indices(idx.data_ptr(), st_i, nq, m0 // 2, s.cuda_stream)
            pv.fri_query_positions_batch_device(idx.data_ptr(), st_i, nq, m0, final_size, B, pos.data_ptr(), st_p, s.cuda_stream)

        torch.cuda.synchronize()
        call()                                                       # eager: the context's record buffer of this stream holds B records per round
        ctx.synchronize(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        for rep in range(2):
            es = [rng.integers(0, P, m0, dtype=np.uint64) for _ in range(B)]
            salts0 = [rng.integers(0, 256, (m0, 16), dtype=np.uint8) for _ in range(B)]
            salts = [rng.integers(0, 256, (nsalt, 16), dtype=np.uint8) for _ in range(B)]
            states = [emu.pattern(14 + 41 * b + 7 * rep, rep + b) for b in range(B)]
            for b in range(B):
                te[b * st_e:b * st_e + m0] = torch.from_numpy(es[b].astype(np.uint32).view(np.int32)).to(dev)
                ts0[b * st_s0:b * st_s0 + 16 * m0] = torch.from_numpy(salts0[b].reshape(-1)).to(dev)
                ts[b * st_s:b * st_s + 16 * nsalt] = torch.from_numpy(salts[b].reshape(-1)).to(dev)
            for t in (layers, betas, idx, pos):
                t.fill_(-1)
            levels0.fill_(0xA5), levels.fill_(0xA5)
            tr.load(states)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            after = tr.download()
            for b in range(B):
                # the single calls on proof b
                t1 = pv.DeviceTranscript.from_bytes(states[b])
                e1, s01, s1 = te[b * st_e:b * st_e + m0].clone(), ts0[b * st_s0:b * st_s0 + 16 * m0].clone(), ts[b * st_s:b * st_s + 16 * nsalt].clone()
                lv01, lv1 = torch.empty(32 * ndig0, dtype=torch.uint8, device=dev), torch.empty(32 * ndig, dtype=torch.uint8, device=dev)
                ly1, b1 = torch.empty(sum(sizes), dtype=torch.int32, device=dev), torch.empty(rounds, dtype=torch.int32, device=dev)
                i1, p1 = torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(rounds * 2 * nq, dtype=torch.int32, device=dev)
                ta.merkle_commit_device(e1.data_ptr(), s01.data_ptr(), m0, lv01.data_ptr())
                t1.absorb_device(lv01.data_ptr() + 32 * (ndig0 - 1), 32)
                pv.fri_commit_phase_transcript_device(ctx, e1.data_ptr(), m0, x0, final_size, s1.data_ptr(), t1, ly1.data_ptr(), lv1.data_ptr(), b1.data_ptr())
                t1.squeeze_indices(i1.data_ptr(), nq, m0 // 2)
                pv.fri_query_positions_device(i1.data_ptr(), nq, m0, final_size, p1.data_ptr())
                torch.cuda.synchronize()
                assert torch.equal(levels0[b * st_lv0:][:32 * ndig0], lv01) and torch.equal(levels[b * st_lv:][:32 * ndig], lv1), (rep, b)
                assert torch.equal(layers[b * st_ly:][:sum(sizes)], ly1) and torch.equal(betas[b * st_b:][:rounds], b1), (rep, b)
                assert torch.equal(idx[b * st_i:][:nq], i1) and torch.equal(pos[b * st_p:][:rounds * 2 * nq], p1), (rep, b)
                assert after[b] == t1.download() and after[b][1] == 0, (rep, b)
                t1.free()
                # and the model
                model = emu.Model(states[b])
                model.absorb(tree_of(es[b].reshape(-1, 1), 1, salts0[b])[-1].tobytes())
                want_betas = []
                for k in range(rounds):
                    want_betas += model.squeeze(1)
                    model.absorb(lv1.cpu().numpy().reshape(-1, 32)[sum(lib.toyni_merkle_total_digests(h) for h in sizes[:k + 1]) - 1].tobytes())
                assert b1.cpu().numpy().view(np.uint32).tolist() == want_betas
                assert i1.cpu().numpy().view(np.uint32).tolist() == model.squeeze_indices(nq, m0 // 2) and after[b][0] == model.state
            # the gaps between the proofs were not written
            assert (levels0.reshape(B, st_lv0)[:, 32 * ndig0:] == 0xA5).all() and (levels.reshape(B, st_lv)[:, 32 * ndig:] == 0xA5).all()
            assert (layers.reshape(B, st_ly)[:, sum(sizes):] == -1).all() and (pos.reshape(B, st_p)[:, rounds * 2 * nq:] == -1).all()
        del g
        tr.free()
    finally:
        ctx.destroy()


# ---- end to end: the FRI part of three Fibonacci proofs in one chain ----
def test_the_fri_part_of_three_fibonacci_proofs_in_one_batched_chain(env):
    ta, torch, dev = env
    from harness import fib_prover as fp, fib_verifier as fvb
    from harness.fri_device_transcript import fri_on_device
    from harness.fri_device_transcript_batch import fri_on_device_batch
    n = 1 << 3
    proofs, caps, states = [], [], []
    for b in range(3):
        cap = {}
        proof = fp.generate_proof(fp.fibonacci_trace(n), seed=5 + b, raw=True, capture=cap)     # another seed: another mask, other salts
        t = fp.Transcript()
        t.absorb(proof["trace_commitment"]), t.absorb(proof["quotient_commitment"])
        assert fp.derive_z(t, proof["lde_size"]) == cap["z"]
        for v in (proof["t_z"], proof["t_gz"], proof["t_ggz"], proof["q_z"]):
            t.absorb_field(v)
        proofs.append(proof), caps.append(cap), states.append(t.state)
    N = proofs[0]["lde_size"]
    assert N == 1 << 8 and all(p["lde_size"] == N for p in proofs)
    final_size = len(proofs[0]["fri_final_layer"])
    assert len({p["trace_commitment"] for p in proofs}) == 3
    ctx = ta.ntt.get_or_create_ctx(N)
    deeps = [np.asarray(c["deep"], dtype=np.uint64).astype(np.uint32) for c in caps]
    pools = [c["salt_pool"] for c in caps]
    got = fri_on_device_batch(ctx, deeps, [p[2 * N:3 * N] for p in pools], [p[3 * N:] for p in pools], states, fp.COSET_SHIFT, final_size,
                              fp.NUM_QUERIES)
    rebuilt = []
    for b, proof in enumerate(proofs):
        one = fri_on_device(ctx, deeps[b], pools[b][2 * N:3 * N], pools[b][3 * N:], states[b], fp.COSET_SHIFT, final_size, fp.NUM_QUERIES)
        assert got[b]["status"] == 0
        for key in ("commitments", "final_layer", "indices", "groups", "betas", "state", "status"):
            assert got[b][key] == one[key], (b, key)
        assert got[b]["records"].tobytes() == one["records"].tobytes(), b
        assert got[b]["commitments"] == proof["fri_commitments"] and got[b]["indices"] == proof["query_indices"] and got[b]["betas"] == caps[b]["betas"]
        groups = proof["opening_groups"]
        head = sum(len(ix) * ta.prover.merkle_open_record_bytes(n_) for n_, _, ix in groups[:2])
        assert proof["opening_records"][head:].tobytes() == got[b]["records"].tobytes(), b
        rebuilt.append(dict(proof, fri_commitments=got[b]["commitments"], fri_final_layer=got[b]["final_layer"], query_indices=got[b]["indices"],
                            opening_records=np.concatenate([proof["opening_records"][:head], got[b]["records"]]),
                            opening_groups=groups[:2] + got[b]["groups"]))
        why = []
        assert fvb.verify(fp.expand_proof(rebuilt[-1]), why), (b, why)
    # proof 0's layers under proof 1's openings
    groups0 = proofs[0]["opening_groups"]
    head = sum(len(ix) * ta.prover.merkle_open_record_bytes(n_) for n_, _, ix in groups0[:2])
    mixed = dict(rebuilt[0], opening_records=np.concatenate([proofs[0]["opening_records"][:head], got[1]["records"]]),
                 opening_groups=groups0[:2] + got[1]["groups"])
    why = []
    assert not fvb.verify(fp.expand_proof(mixed), why)


if __name__ == "__main__":   # the child of test_the_launched_path_alone_gives_the_same_bytes
    import __graft_entry__ as _entry
    _entry.build_hip()
    import toyni_amd as _ta
    for _key, _digest in phase_digests(_ta).items():
        print("PHASE %s %s" % (_key, _digest))
    print("TAIL %d" % sum("fri_tail_rounds" in k for k in _ta._lib.launched_kernels()))
