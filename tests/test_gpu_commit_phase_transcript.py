"""The Fiat-Shamir transcript in device memory and the FRI commit phases on it (include/toyni_hip.h 3l), on the GPU.

* The four transcript calls against hashlib, at the vectors tests/test_emu_transcript.py steps on the CPU (the same script, run through
  the device calls).
* Both phases against two judges, byte for byte in layers, levels, roots, d_betas and the final transcript: the callback phase of the
  same library driven by the Python Transcript (every shape), and the oracle fold plus hashlib trees (the shapes up to 2^12).
  Salted and unsalted, field-edge layers at 2^5 and 2^12, initial states of 32, 96 and 1008 - 32 bytes, every buffer in guard bands.
* A transcript that overflowed before the phase: status set, the phase completes with beta = 0, guard bands intact.
* A captured graph of absorb + Ext phase + indices + positions, replayed twice on new contents.
* End to end: the FRI part of the Fibonacci proof of tests/harness/fib_prover.py rebuilt without a synchronisation
  (tests/harness/fri_device_transcript.py) and accepted by tests/harness/fib_verifier.py; the low-degree Ext proof of
  tests/test_gpu_fold_commit_ext.py with the device transcript, judged by tests/harness/fri_ext_verifier.py."""
import hashlib

import numpy as np
import pytest

import oracle
import rows_common as rc
import test_emu_transcript as emu
from guarded import edge_residues
from oracle import P

pytestmark = pytest.mark.gpu

ROW = rc.ROW
E_RANGE = 10006


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
    """every level of the commitment of a layer ((n, words) residues; a base leaf is the row leaf of width 1), hashlib only"""
    levels = rc.hashlib_levels(rc.leaves_of(np.asarray(layer, dtype=np.uint64).reshape(-1, words), salts))
    return np.frombuffer(b"".join(d for level in levels for d in level), dtype=np.uint8).reshape(-1, 32)


class HostTranscript(emu.Model):
    """the reference transcript (tests/test_emu_transcript.Model, which is tests/harness/fib_prover.Transcript below the capacity)"""

    def challenge_fn(self, words, betas):
        def challenge(_rnd, root, want_beta):
            if root is not None:
                self.absorb(root)
            if not want_beta:
                return 0
            b = self.squeeze(words)
            betas.extend(b)
            return b if words == 4 else b[0]
        return challenge


# ---- the transcript calls alone ----
def test_transcript_calls_match_hashlib_at_the_emu_vectors(env):
    ta, torch, dev = env
    pv = ta.prover
    lines, want = emu.script()
    expected_checks = sum(1 for kind, _ in want if kind != "R")
    want = iter(want)
    tr = pv.DeviceTranscript()
    checked = 0
    with rc.Dev(ta) as d:
        g_out = d.buf(4 * 256)
        for line in lines:
            f = line.split()
            if f[0] == "init":
                tr.load(b"" if f[1] == "-" else bytes.fromhex(f[1]))
            elif f[0] == "status":
                state, _ = tr.download()
                host = np.zeros(1024, dtype=np.uint8)
                host[:8] = np.array([len(state), int(f[1])], dtype=np.uint32).view(np.uint8)
                host[16:16 + len(state)] = np.frombuffer(state, dtype=np.uint8)
                ta._lib.check(ta._lib.lib.toyni_memcpy_h2d(tr.ptr, host.ctypes.data, 1024), "upload")
            elif f[0] == "absorb":
                data = b"" if f[1] == "-" else bytes.fromhex(f[1])
                g = d.put(np.frombuffer(data, dtype=np.uint8), word=1) if data else None
                tr.absorb_device(g.ptr if g else 0, len(data))
            elif f[0] == "squeeze":
                kind, exp = next(want)
                g_out.fill_sentinel()
                if int(f[1]):
                    tr.squeeze(g_out.ptr, int(f[1]))
                got = g_out.download()
                assert kind == "S" and got[:len(exp)].tolist() == exp and (got[len(exp):] == 0xA5A5A5A5).all(), line
                checked += 1
            elif f[0] == "indices":
                kind, exp = next(want)
                g_out.fill_sentinel()
                tr.squeeze_indices(g_out.ptr, int(f[1]), int(f[2]))
                got = g_out.download()
                assert kind == "I" and got[:len(exp)].tolist() == exp and (got[len(exp):] == 0xA5A5A5A5).all(), line
                checked += 1
            elif f[0] == "state":
                kind, exp = next(want)
                assert kind == "T" and tr.download() == (exp.state, exp.status), line
                checked += 1
            elif f[0] == "reduce":
                next(want)                                   # the reduction is reached through every squeeze; alone it is a CPU case
            elif f[0] == "positions":
                kind, exp = next(want)
                m0, fin, idx = int(f[1]), int(f[2]), [int(v) for v in f[3:]]
                g_idx, g_pos = d.put(np.array(idx, dtype=np.uint32)), d.buf(4 * max(len(exp), 1))
                pv.fri_query_positions_device(g_idx.ptr, len(idx), m0, fin, g_pos.ptr)
                got = g_pos.download()
                assert got[:len(exp)].tolist() == exp and (got[len(exp):] == 0xA5A5A5A5).all(), line
                checked += 1
    tr.free()
    assert checked == expected_checks and checked > 80


# ---- both phases against the callback phase and against the oracle + hashlib ----
SHAPES = [(1, 1), (4, 4), (5, 1), (10, 1), (11, 1 << 10), (12, 1), (12, 16), (16, 16), (21, 1 << 20)]   # (log2 m0, final_size)
INITIAL = [32, 96, 1008 - 32]


def run_both(ta, d, ctx, words, e, m0, x0, final_size, salts, state0):
    """The callback phase (Python transcript) and the device-transcript phase on the same inputs, each into its own guard-banded
    buffers.  Returns (callback outputs, device outputs) as dicts of layers, levels, betas, state, status."""
    lib, pv = ta._lib.lib, ta.prover
    sizes = halves_of(m0, final_size)
    ndig = sum(lib.toyni_merkle_total_digests(h) for h in sizes)
    g_e = d.put(np.ascontiguousarray(e, dtype=np.uint32))
    g_s = d.put(salts, word=1) if salts is not None and len(salts) else None
    sp = g_s.ptr if g_s else 0
    out = []
    for device in (False, True):
        g_layers, g_levels = d.buf(4 * words * sum(sizes)), d.buf(32 * ndig, word=1)
        if device:
            g_betas = d.buf(4 * words * len(sizes))
            tr = pv.DeviceTranscript.from_bytes(state0)
            entry = pv.fri_commit_phase_transcript_ext_device if words == 4 else pv.fri_commit_phase_transcript_device
            entry(ctx, g_e.ptr, m0, x0, final_size, sp, tr, g_layers.ptr, g_levels.ptr, g_betas.ptr)
            ctx.synchronize()
            state, status = tr.download()
            tr.free()
            betas = g_betas.download().tolist()
        else:
            host, betas = HostTranscript(state0), []
            entry = pv.fri_commit_phase_ext_device if words == 4 else pv.fri_commit_phase_device
            entry(ctx, g_e.ptr, m0, x0, final_size, sp, host.challenge_fn(words, betas), g_layers.ptr, g_levels.ptr)
            state, status = host.state, host.status
        out.append({"layers": g_layers.download(), "levels": g_levels.download().reshape(-1, 32), "betas": betas, "state": state, "status": status})
    assert (g_e.download() == np.ascontiguousarray(e, dtype=np.uint32).reshape(-1)).all()      # layer 0 is read only
    return out


@pytest.mark.parametrize("salted", [True, False])
@pytest.mark.parametrize("words", [1, 4])
@pytest.mark.parametrize("log_m0,final_size", SHAPES)
def test_phase_equals_the_callback_phase_and_the_cpu_replay(env, log_m0, final_size, words, salted):
    ta, torch, dev = env
    lib = ta._lib.lib
    m0 = 1 << log_m0
    ctx = ta.ntt.get_or_create_ctx(max(m0, 2))
    case = SHAPES.index((log_m0, final_size))
    rng = np.random.default_rng(1000 * words + 10 * case + salted)
    edgy = log_m0 in (5, 12) and final_size == 1
    e = (edge_residues(words * m0, 40 + case) if edgy else rng.integers(0, P, words * m0)).astype(np.uint64).reshape(m0, words)
    x0 = P - 1 if log_m0 == 5 else 7
    sizes = halves_of(m0, final_size)
    salts = rng.integers(0, 256, (sum(sizes[:-1]), 16), dtype=np.uint8) if salted else None
    state0 = emu.pattern(INITIAL[case % 3], case)
    with rc.Dev(ta) as d:
        cb, dv = run_both(ta, d, ctx, words, e, m0, x0, final_size, salts, state0)
    assert dv["status"] == 0 and cb["status"] == 0
    assert dv["betas"] == cb["betas"] and len(dv["betas"]) == words * len(sizes)
    assert dv["state"] == cb["state"]
    assert (dv["layers"] == cb["layers"]).all() and (dv["levels"] == cb["levels"]).all()
    if log_m0 > 12:
        return
    # the direct judge: the reference transcript, the oracle's fold on the squared domain, hashlib trees (the last one unsalted)
    t = emu.Model(state0)
    got_layers, got_levels = dv["layers"].astype(np.uint64).reshape(-1, words), dv["levels"]
    cur, x, lo, dlo, slo = e, x0, 0, 0, 0
    for k, h in enumerate(sizes):
        beta = t.squeeze(words)
        assert dv["betas"][words * k:words * (k + 1)] == beta, k
        xs = oracle.domain_elements(2 * h, x)
        if words == 4:
            want = oracle.fri_fold_ext(cur, xs, np.array(beta, dtype=np.uint64))
        else:
            want = oracle.fri_fold(cur.reshape(-1), xs, beta[0]).reshape(-1, 1)
        assert (got_layers[lo:lo + h] == want).all(), k
        s = salts[slo:slo + h] if salted and k < len(sizes) - 1 else None
        nd = lib.toyni_merkle_total_digests(h)
        tree = tree_of(want, words, s)
        assert (got_levels[dlo:dlo + nd] == tree).all(), k
        t.absorb(tree[-1].tobytes())
        cur, x, lo, dlo, slo = want, x * x % P, lo + h, dlo + nd, slo + (h if s is not None else 0)
    assert dv["state"] == t.state


# ---- TOYNI_FRI_TAIL_LOG=-1: every round on the launched path, the same bytes ----
def phase_digest(ta, log_m0, final_size, words):
    """sha256 over everything the device phase leaves (layers, levels, betas, transcript) for a fixed salted input"""
    m0 = 1 << log_m0
    ctx = ta.ntt.get_or_create_ctx(m0)
    rng = np.random.default_rng(5000 + 10 * log_m0 + words)
    e = rng.integers(0, P, (m0, words), dtype=np.uint64)
    sizes = halves_of(m0, final_size)
    salts = rng.integers(0, 256, (sum(sizes[:-1]), 16), dtype=np.uint8)
    ndig = sum(ta._lib.lib.toyni_merkle_total_digests(h) for h in sizes)
    with rc.Dev(ta) as d:
        g_e, g_s = d.put(e.astype(np.uint32)), d.put(salts, word=1)
        g_layers, g_levels, g_betas = d.buf(4 * words * sum(sizes)), d.buf(32 * ndig, word=1), d.buf(4 * words * len(sizes))
        tr = ta.prover.DeviceTranscript.from_bytes(emu.pattern(46, 7))
        entry = ta.prover.fri_commit_phase_transcript_ext_device if words == 4 else ta.prover.fri_commit_phase_transcript_device
        entry(ctx, g_e.ptr, m0, 7, final_size, g_s.ptr, tr, g_layers.ptr, g_levels.ptr, g_betas.ptr)
        ctx.synchronize()
        state, status = tr.download()
        tr.free()
        h = hashlib.sha256()
        for part in (g_layers.download().tobytes(), g_levels.download().tobytes(), g_betas.download().tobytes(), state, bytes([status & 0xFF])):
            h.update(part)
    return h.hexdigest()


@pytest.mark.parametrize("words", [1, 4])
@pytest.mark.parametrize("log_m0,final_size", [(12, 1), (16, 16)])
def test_the_launched_path_alone_gives_the_same_bytes(env, log_m0, final_size, words):
    """A child process (the knob is read once per process) with TOYNI_FRI_TAIL_LOG=-1: no fused launch, every round a fold, a tree
    and a one-wave transcript step.  The fused default of this process must have written the same bytes."""
    import os
    import subprocess
    import sys
    ta, torch, dev = env
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child_env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests"), os.path.join(root, "tests", "_hooks")]),
                     TOYNI_FRI_TAIL_LOG="-1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(log_m0), str(final_size), str(words)], capture_output=True, text=True,
                         timeout=300, env=child_env, cwd=root)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    m = [l for l in res.stdout.split("\n") if l.startswith("PHASE ")]
    assert len(m) == 1 and "tail=0" in m[0], res.stdout[-1500:]
    launched = ta._lib.launched_kernels()
    want = phase_digest(ta, log_m0, final_size, words)
    assert any("fri_tail_rounds_kernel" in k for k in ta._lib.launched_kernels()), launched     # this process took the fused launch
    assert m[0].split()[1] == want


@pytest.mark.parametrize("words", [1, 4])
def test_nothing_to_fold_writes_nothing_and_leaves_the_transcript(env, words):
    ta, torch, dev = env
    pv = ta.prover
    ctx = ta.ntt.get_or_create_ctx(64)
    state0 = emu.pattern(50, 3)
    with rc.Dev(ta) as d:
        g_e, g_layers, g_levels, g_betas = d.put(np.arange(64 * words, dtype=np.uint32)), d.buf(1024), d.buf(1024, word=1), d.buf(64)
        tr = pv.DeviceTranscript.from_bytes(state0)
        entry = pv.fri_commit_phase_transcript_ext_device if words == 4 else pv.fri_commit_phase_transcript_device
        for m0, fin in ((16, 16), (8, 32), (1, 1)):
            entry(ctx, g_e.ptr, m0, 7, fin, 0, tr, g_layers.ptr, g_levels.ptr, g_betas.ptr)
        ctx.synchronize()
        assert tr.download() == (state0, 0)
        tr.free()
        for g in (g_layers, g_levels, g_betas):
            assert (g.download(np.uint8) == 0xA5).all()


# ---- a transcript that overflowed before the phase ----
@pytest.mark.parametrize("words", [1, 4])
def test_an_overflowed_transcript_gives_zero_betas_and_the_phase_completes(env, words):
    ta, torch, dev = env
    lib, pv = ta._lib.lib, ta.prover
    m0, final_size, x0 = 1 << 6, 4, 7
    ctx = ta.ntt.get_or_create_ctx(m0)
    rng = np.random.default_rng(77 + words)
    e = rng.integers(0, P, (m0, words), dtype=np.uint64)
    sizes = halves_of(m0, final_size)
    ndig = sum(lib.toyni_merkle_total_digests(h) for h in sizes)
    state0 = emu.pattern(1000, 2)
    with rc.Dev(ta) as d:
        g_e, g_root = d.put(e.astype(np.uint32)), d.put(np.frombuffer(emu.pattern(32, 1), dtype=np.uint8), word=1)
        g_layers, g_levels, g_betas = d.buf(4 * words * sum(sizes)), d.buf(32 * ndig, word=1), d.buf(4 * words * len(sizes))
        tr = pv.DeviceTranscript.from_bytes(state0)
        tr.absorb_device(g_root.ptr, 32)                                         # the caller's own absorb of layer 0's root: 1000 + 32 > 1008
        entry = pv.fri_commit_phase_transcript_ext_device if words == 4 else pv.fri_commit_phase_transcript_device
        entry(ctx, g_e.ptr, m0, x0, final_size, 0, tr, g_layers.ptr, g_levels.ptr, g_betas.ptr)
        ctx.synchronize()
        assert tr.download() == (state0, E_RANGE)
        tr.free()
        assert (g_betas.download() == 0).all()
        # beta = 0 folds to the averages; the trees are those of these layers
        got_layers, got_levels = g_layers.download().astype(np.uint64).reshape(-1, words), g_levels.download().reshape(-1, 32)
        cur, lo, dlo = e, 0, 0
        for h in sizes:
            want = (cur[:h] + cur[h:]) * ((P + 1) // 2) % P
            nd = lib.toyni_merkle_total_digests(h)
            assert (got_layers[lo:lo + h] == want).all() and (got_levels[dlo:dlo + nd] == tree_of(want, words, None)).all()
            cur, lo, dlo = want, lo + h, dlo + nd


# ---- captured replay ----
def test_absorb_phase_indices_and_positions_replay_from_one_captured_graph(env):
    ta, torch, dev = env
    lib, pv = ta._lib.lib, ta.prover
    m0, final_size, x0, nq = 1 << 10, 4, 7, 8
    sizes = halves_of(m0, final_size)
    rounds = len(sizes)
    ndig = sum(lib.toyni_merkle_total_digests(h) for h in sizes)
    ctx = ta.NttContext(m0, device=dev.index)
    rng = np.random.default_rng(9)
    try:
        te = torch.zeros(4 * m0, dtype=torch.int32, device=dev)
        ts = torch.zeros((sum(sizes[:-1]), 16), dtype=torch.uint8, device=dev)
        root0 = torch.zeros(32, dtype=torch.uint8, device=dev)
        layers = torch.empty(4 * sum(sizes), dtype=torch.int32, device=dev)
        levels = torch.empty((ndig, 32), dtype=torch.uint8, device=dev)
        betas = torch.empty(4 * rounds, dtype=torch.int32, device=dev)
        idx = torch.empty(nq, dtype=torch.int32, device=dev)
        pos = torch.empty(rounds * 2 * nq, dtype=torch.int32, device=dev)
        tr = pv.DeviceTranscript.from_bytes(b"warm")
        s = torch.cuda.Stream(device=dev)

        def call():
            tr.absorb_device(root0.data_ptr(), 32, s.cuda_stream)
            pv.fri_commit_phase_transcript_ext_device(ctx, te.data_ptr(), m0, x0, final_size, ts.data_ptr(), tr, layers.data_ptr(), levels.data_ptr(),
                                                      betas.data_ptr(), s.cuda_stream)
            tr.squeeze_indices(idx.data_ptr(), nq, m0 // 2, s.cuda_stream)
            pv.fri_query_positions_device(idx.data_ptr(), nq, m0, final_size, pos.data_ptr(), s.cuda_stream)

        torch.cuda.synchronize()
        call()                                                                  # eager: the context's record buffer of this stream exists
        ctx.synchronize(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        for rep in range(2):
            e = rng.integers(0, P, (m0, 4), dtype=np.uint64)
            salts = rng.integers(0, 256, (sum(sizes[:-1]), 16), dtype=np.uint8)
            r0, state0 = emu.pattern(32, 20 + rep), emu.pattern(14 + 40 * rep, rep)
            te.copy_(torch.from_numpy(e.astype(np.uint32).reshape(-1).view(np.int32)))
            ts.copy_(torch.from_numpy(salts)), root0.copy_(torch.from_numpy(np.frombuffer(r0, dtype=np.uint8).copy()))
            layers.fill_(-1), levels.fill_(0xA5), betas.fill_(-1), idx.fill_(-1), pos.fill_(-1)
            tr.load(state0)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            # the callback phase on the same inputs, the Python transcript having absorbed the same root
            host, want_betas = HostTranscript(state0), []
            host.absorb(r0)
            layers2, levels2 = torch.empty_like(layers), torch.empty_like(levels)
            pv.fri_commit_phase_ext_device(ctx, te.data_ptr(), m0, x0, final_size, ts.data_ptr(), host.challenge_fn(4, want_betas), layers2.data_ptr(),
                                           levels2.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(layers, layers2) and torch.equal(levels, levels2), rep
            assert betas.cpu().numpy().view(np.uint32).tolist() == want_betas, rep
            want_idx = host.squeeze_indices(nq, m0 // 2)
            assert idx.cpu().numpy().view(np.uint32).tolist() == want_idx, rep
            assert pos.cpu().numpy().view(np.uint32).tolist() == emu.query_positions(want_idx, m0, final_size), rep
            assert tr.download() == (host.state, 0), rep
        del g
        tr.free()
    finally:
        ctx.destroy()


# ---- end to end, base field: the FRI part of the Fibonacci proof without a synchronisation ----
def test_the_fri_part_of_the_fibonacci_proof_on_the_device_transcript(env):
    ta, torch, dev = env
    from harness import fib_prover as fp, fib_verifier as fvb
    from harness.fri_device_transcript import fri_on_device
    n = 1 << 6
    cap = {}
    proof = fp.generate_proof(fp.fibonacci_trace(n), seed=5, raw=True, capture=cap)
    N = proof["lde_size"]
    final_size = len(proof["fri_final_layer"])
    # the transcript as the prover's stood before the DEEP layer's root: the two commitments, derive_z, the four OOD values
    t = fp.Transcript()
    t.absorb(proof["trace_commitment"]), t.absorb(proof["quotient_commitment"])
    assert fp.derive_z(t, N) == cap["z"]
    for v in (proof["t_z"], proof["t_gz"], proof["t_ggz"], proof["q_z"]):
        t.absorb_field(v)
    pool = cap["salt_pool"]
    got = fri_on_device(ta.ntt.get_or_create_ctx(N), np.asarray(cap["deep"], dtype=np.uint64).astype(np.uint32), pool[2 * N:3 * N], pool[3 * N:],
                        t.state, fp.COSET_SHIFT, final_size, fp.NUM_QUERIES)
    assert got["status"] == 0
    assert got["commitments"] == proof["fri_commitments"]
    assert got["final_layer"] == proof["fri_final_layer"]
    assert got["indices"] == proof["query_indices"] and len(got["indices"]) == 44
    assert got["betas"] == cap["betas"]
    # the opening records of the DEEP layer and of every FRI layer: the tail of the harness's records, byte for byte
    groups = proof["opening_groups"]
    assert [(n_, s_, list(ix)) for n_, s_, ix in groups[2:]] == got["groups"]
    head = sum(len(ix) * ta.prover.merkle_open_record_bytes(n_) for n_, _, ix in groups[:2])
    assert proof["opening_records"][head:].tobytes() == got["records"].tobytes()
    # and the proof assembled from the device's parts is accepted
    rebuilt = dict(proof, fri_commitments=got["commitments"], fri_final_layer=got["final_layer"], query_indices=got["indices"],
                   opening_records=np.concatenate([proof["opening_records"][:head], got["records"]]), opening_groups=groups[:2] + got["groups"])
    why = []
    assert fvb.verify(fp.expand_proof(rebuilt), why), why


# ---- end to end, Ext: the low-degree proof of tests/test_gpu_fold_commit_ext.py on the device transcript ----
N_EXT, LOG_BLOWUP, SHIFT, FINAL = 1 << 8, 2, 7, 4


def reference_challenges(seed, proof, nq):
    """What src/transcript.rs yields for the roots of the proof: four squeezes per round, then squeeze_indices."""
    t = emu.Model(seed)
    t.absorb(proof["root0"])
    betas = []
    for root in proof["roots"]:
        betas.append(tuple(t.squeeze(4)))
        t.absorb(root)
    return betas, t.squeeze_indices(nq, proof["m0"] // 2)


def test_the_ext_low_degree_proof_on_the_device_transcript(env, monkeypatch):
    """tests/harness/fri_ext_verifier.py judges paths, position flags, salts, the fold relation between every two layers and the
    final layer, unchanged.  Its own challenge derivation reduces all 32 bytes of a hash and draws indices without dropping repeats
    -- not the reference transcript that the device implements -- so verify() is handed the betas of d_betas and the indices the
    device squeezed (fv.challenges is what it calls for them), and those are held to the reference transcript here, separately."""
    ta, torch, dev = env
    from harness import fri_ext_verifier as fv
    lib, pv = ta._lib.lib, ta.prover
    nq = fv.NQUERIES
    ctx = ta.ntt.get_or_create_ctx(N_EXT)
    rng = np.random.default_rng(8)
    sizes = halves_of(N_EXT, FINAL)
    rounds = len(sizes)
    coeffs = rng.integers(0, P, (N_EXT >> LOG_BLOWUP, 4), dtype=np.uint64)
    tc = torch.from_numpy(coeffs.astype(np.uint32).reshape(-1).view(np.int32)).to(dev)
    layer0 = torch.empty(4 * N_EXT, dtype=torch.int32, device=dev)
    salts0 = torch.from_numpy(rng.integers(0, 256, (N_EXT, 16), dtype=np.uint8)).to(dev)
    levels0 = torch.zeros((lib.toyni_merkle_total_digests(N_EXT), 32), dtype=torch.uint8, device=dev)
    salts = torch.from_numpy(rng.integers(0, 256, (sum(sizes[:-1]), 16), dtype=np.uint8)).to(dev)
    layers = torch.empty(4 * sum(sizes), dtype=torch.int32, device=dev)
    ndigs = [lib.toyni_merkle_total_digests(h) for h in sizes]
    levels = torch.zeros((sum(ndigs), 32), dtype=torch.uint8, device=dev)
    betas = torch.empty(4 * rounds, dtype=torch.int32, device=dev)
    idx = torch.empty(nq, dtype=torch.int32, device=dev)
    pos = torch.empty((rounds + 1) * 2 * nq, dtype=torch.int32, device=dev)
    tr = pv.DeviceTranscript.from_bytes(fv.SEED)
    # ---- enqueue everything ----
    ta._lib.check(lib.toyni_lde_ext_device(ctx.handle, tc.data_ptr(), layer0.data_ptr(), LOG_BLOWUP, SHIFT, None), "lde ext")
    ta.merkle_commit_rows_device(layer0.data_ptr(), N_EXT, 4, ROW, 0, salts0.data_ptr(), levels0.data_ptr())
    tr.absorb_device(levels0[-1].data_ptr(), 32)
    pv.fri_commit_phase_transcript_ext_device(ctx, layer0.data_ptr(), N_EXT, SHIFT, FINAL, salts.data_ptr(), tr, layers.data_ptr(), levels.data_ptr(),
                                              betas.data_ptr())
    tr.squeeze_indices(idx.data_ptr(), nq, N_EXT // 2)
    # the verifier also wants the FINAL layer opened: positions down to one layer further than the phase folds
    pv.fri_query_positions_device(idx.data_ptr(), nq, N_EXT, FINAL // 2, pos.data_ptr())
    per_layer = [(layer0, levels0, salts0, N_EXT)]
    lo = dlo = slo = 0
    for k, h in enumerate(sizes):
        last = k == rounds - 1
        per_layer.append((layers[4 * lo:], levels[dlo:], None if last else salts[slo:], h))
        lo, dlo, slo = lo + h, dlo + ndigs[k], slo + (0 if last else h)
    outs = []
    for k, (values, tree, s, m) in enumerate(per_layer):
        rec = lib.toyni_merkle_open_rows_record_bytes(m, 4)
        out = torch.full((2 * nq * rec,), 0xA5, dtype=torch.uint8, device=dev)
        ta.merkle_open_rows_device(tree.data_ptr(), m, values.data_ptr(), 4, ROW, 0, s.data_ptr() if s is not None else 0,
                                   pos.data_ptr() + 4 * k * 2 * nq, 2 * nq, out.data_ptr())
        outs.append((out, rec))
    torch.cuda.synchronize()                                                    # the one synchronisation
    assert tr.status() == 0
    tr.free()
    openings = [[] for _ in range(nq)]
    for out, rec in outs:
        raw = out.cpu().numpy().tobytes()
        for q in range(nq):
            openings[q].append([raw[(2 * q + j) * rec:(2 * q + j + 1) * rec] for j in range(2)])
    lv = levels.cpu().numpy()
    roots, dlo = [], 0
    for nd in ndigs:
        roots.append(lv[dlo + nd - 1].tobytes())
        dlo += nd
    final = layers[4 * (sum(sizes) - FINAL):].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(FINAL, 4)
    proof = {"m0": N_EXT, "x0": SHIFT, "final_size": FINAL, "root0": levels0[-1].cpu().numpy().tobytes(), "roots": roots,
             "final_layer": [tuple(int(v) for v in e) for e in final], "openings": openings}
    got_betas = [tuple(int(v) for v in b) for b in betas.cpu().numpy().view(np.uint32).reshape(rounds, 4)]
    got_idx = [int(v) for v in idx.cpu().numpy().view(np.uint32)]
    assert (got_betas, got_idx) == reference_challenges(fv.SEED, proof, nq)
    monkeypatch.setattr(fv, "challenges", lambda _proof: (got_betas, got_idx))
    assert fv.verify(proof) == (True, "accepted")
    assert len(set(proof["final_layer"])) == 1
    # one changed beta of d_betas: the fold relation of that round no longer holds
    wrong = [b for b in got_betas]
    wrong[2] = (wrong[2][0], (wrong[2][1] + 1) % P, wrong[2][2], wrong[2][3])
    monkeypatch.setattr(fv, "challenges", lambda _proof: (wrong, got_idx))
    ok, why = fv.verify(proof)
    assert not ok and "fold relation between layers 2 and 3" in why, why


if __name__ == "__main__":   # the child of test_the_launched_path_alone_gives_the_same_bytes
    import sys
    import __graft_entry__ as _entry
    _entry.build_hip()
    import toyni_amd as _ta
    _digest = phase_digest(_ta, int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]))
    print("PHASE %s tail=%d" % (_digest, sum("fri_tail_rounds_kernel" in k for k in _ta._lib.launched_kernels())))
