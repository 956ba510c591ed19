"""The Ext fold-and-commit round and the Ext commit phase on the device (include/toyni_hip.h 3j), bit-exact against three references:
the oracle's fri_fold_ext for every layer, hashlib over the row leaves of tests/rows_common.py for every tree, and the two existing
calls a round replaces (toyni_fri_fold_ext_device, then toyni_merkle_commit_rows_device with width 4, row-major) for both.  Guard
bands around d_out and d_levels at every size up to 2^12, field-edge inputs at two of them, the grid-stride step at 2^21, the phase
with its transcript replayed on the CPU, the failure paths, a captured replay of one round, and a low-degree proof at N = 2^8 that
tests/harness/fri_ext_verifier.py accepts and, with one deviation at a time, rejects."""
import ctypes
import hashlib

import numpy as np
import pytest

import ext_model as em
import oracle
import rows_common as rc
from guarded import Guarded, HostMem, edge_residues
from harness import fri_ext_verifier as fv
from oracle import P

pytestmark = pytest.mark.gpu

ROW = rc.ROW
E_INVALID_SIZE, E_RANGE, E_REENTRANT = 10001, 10006, 10011


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build_hip()
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import toyni_amd
    return toyni_amd, torch, torch.device("cuda", 0)


def _dev(torch, dev, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).astype(np.uint32).reshape(-1).view(np.int32)).to(dev)


def _host(t):
    return t.cpu().numpy().view(np.uint32).astype(np.uint64)


def tree_of(layer, salts):
    """Every level of the row commitment of an Ext layer ((n, 4) residues), hashlib only: (digests, 32) uint8."""
    levels = rc.hashlib_levels(rc.leaves_of(np.asarray(layer, dtype=np.uint64).reshape(-1, 4), salts))
    return np.frombuffer(b"".join(d for level in levels for d in level), dtype=np.uint8).reshape(-1, 32)


def halves_of(m0, final_size):
    sizes, m = [], m0
    while m > final_size:
        m //= 2
        sizes.append(m)
    return sizes


# ---- one round ----
@pytest.mark.parametrize("salted", [False, True])
@pytest.mark.parametrize("log_m", [1, 2, 5, 8, 9, 10, 12, 16])
def test_one_round_is_the_oracles_fold_a_hashlib_tree_and_the_two_calls_it_replaces(env, log_m, salted):
    """m / 2 = 1 (the leaf is the root), below one workgroup, exactly one (2^9), two (2^10) and many; guard bands around every output
    up to 2^12; field-edge values in every coordinate at 2^5 and 2^12, and a beta with edge coordinates there."""
    ta, torch, dev = env
    lib = ta._lib.lib
    m = 1 << log_m
    half = m // 2
    ctx = ta.ntt.get_or_create_ctx(max(m, 2))
    rng = np.random.default_rng(100 + log_m)
    edgy = log_m in (5, 12)
    e = (edge_residues(4 * m, 300 + log_m) if edgy else rng.integers(0, P, 4 * m)).astype(np.uint64).reshape(m, 4)
    beta = [P - 1, 0, 1, int(rng.integers(0, P))] if edgy else [int(v) for v in rng.integers(0, P, 4)]
    x0 = P - 1 if log_m == 5 else 49
    want = oracle.fri_fold_ext(e, oracle.domain_elements(m, x0), np.array(beta, dtype=np.uint64))
    salts = rng.integers(0, 256, (half, 16), dtype=np.uint8) if salted else None
    levels_want = tree_of(want, salts)
    ndig = lib.toyni_merkle_total_digests(half)
    assert levels_want.shape[0] == ndig
    with rc.Dev(ta) as d:
        g_e = d.put(e.astype(np.uint32))
        g_s = d.put(salts, word=1) if salted else None
        sp = g_s.ptr if salted else 0
        g_out, g_lv = d.buf(16 * half), d.buf(32 * ndig, word=1)
        ta.prover.fri_fold_commit_ext_device(ctx, g_e.ptr, g_out.ptr, m, beta, x0, sp, g_lv.ptr)
        ctx.synchronize()
        got, got_lv = g_out.download().astype(np.uint64).reshape(half, 4), g_lv.download().reshape(ndig, 32)
        assert (got == want).all()
        assert (got_lv == levels_want).all()
        assert (g_e.download().astype(np.uint64).reshape(m, 4) == e).all()           # the input layer is read only
        # and identical to the two separate calls it replaces
        g_out2, g_lv2 = d.buf(16 * half), d.buf(32 * ndig, word=1)
        ta.fri_fold_ext_device(ctx, g_e.ptr, g_out2.ptr, m, beta, x0)
        ta.merkle_commit_rows_device(g_out2.ptr, half, 4, ROW, 0, sp, g_lv2.ptr)
        ctx.synchronize()
        assert (g_out2.download() == g_out.download()).all() and (g_lv2.download() == g_lv.download()).all()


def test_one_round_beyond_the_grid_cap_takes_the_grid_stride_step(env):
    """m / 2 = 2^20 outputs against the 2^19 threads a launch is capped at: every thread takes two.  The layer against the oracle, the
    levels against the two existing calls (which their own tests hold to hashlib), and the first, the middle and the last leaf of the
    download against hashlib directly."""
    ta, torch, dev = env
    lib = ta._lib.lib
    m = 1 << 21
    half = m // 2
    ctx = ta.ntt.get_or_create_ctx(m)
    rng = np.random.default_rng(21)
    e = rng.integers(0, P, (m, 4), dtype=np.uint64)
    beta, x0 = [int(v) for v in rng.integers(0, P, 4)], 7
    want = oracle.fri_fold_ext(e, oracle.domain_elements(m, x0), np.array(beta, dtype=np.uint64))
    salts = rng.integers(0, 256, (half, 16), dtype=np.uint8)
    ndig = lib.toyni_merkle_total_digests(half)
    te, ts = _dev(torch, dev, e), torch.from_numpy(salts).to(dev)
    out, out2 = torch.empty(4 * half, dtype=torch.int32, device=dev), torch.empty(4 * half, dtype=torch.int32, device=dev)
    lv, lv2 = torch.zeros((ndig, 32), dtype=torch.uint8, device=dev), torch.zeros((ndig, 32), dtype=torch.uint8, device=dev)
    ta.prover.fri_fold_commit_ext_device(ctx, te.data_ptr(), out.data_ptr(), m, beta, x0, ts.data_ptr(), lv.data_ptr())
    ta.fri_fold_ext_device(ctx, te.data_ptr(), out2.data_ptr(), m, beta, x0)
    ta.merkle_commit_rows_device(out2.data_ptr(), half, 4, ROW, 0, ts.data_ptr(), lv2.data_ptr())
    torch.cuda.synchronize()
    assert (_host(out).reshape(half, 4) == want).all()
    assert torch.equal(out, out2) and torch.equal(lv, lv2)
    got_lv = lv.cpu().numpy()
    for i in (0, 1, (1 << 19) - 1, 1 << 19, half - 1):                                 # both sides of the stride's seam
        assert got_lv[i].tobytes() == rc.hash_leaf(rc.leaves_of(want[i:i + 1], salts[i:i + 1])[0]), i


# ---- the phase ----
def chained_transcript(seed=b"toyni-test"):
    state = {"t": seed, "seen": [], "order": []}

    def squeeze():
        h = hashlib.sha256(state["t"]).digest()                  # squeeze_challenge: hash, feed back, reduce
        state["t"] = h
        return int.from_bytes(h, "little") % P

    def challenge(rnd, root, want_beta):
        state["order"].append((rnd, root is not None, want_beta))
        if root is not None:
            state["seen"].append(root)
            state["t"] = state["t"] + root                       # absorb_commitment
        return [squeeze() for _ in range(4)] if want_beta else None   # squeeze_ext_challenge: four squeezes

    return state, challenge


@pytest.mark.parametrize("log_m0,final_size,salted", [(1, 1, False), (6, 4, True), (10, 1, False), (14, 16, True)])
def test_commit_phase_in_one_call(env, log_m0, final_size, salted):
    """Every layer as the oracle's fri_fold_ext on the squared domain, every tree as hashlib builds it (the final layer unsalted),
    betas of four squeezes from a transcript that absorbed the previous root, and the callback sees exactly the committed roots, in
    order.  The salted phases launch both instantiations of the fused kernel."""
    ta, torch, dev = env
    lib = ta._lib.lib
    m0 = 1 << log_m0
    ctx = ta.ntt.get_or_create_ctx(max(m0, 2))
    rng = np.random.default_rng(log_m0)
    e = rng.integers(0, P, (m0, 4), dtype=np.uint64)
    x0 = 7
    sizes = halves_of(m0, final_size)
    salts = [rng.integers(0, 256, (h, 16), dtype=np.uint8) for h in sizes[:-1]] if salted else None
    state, challenge = chained_transcript()
    te = _dev(torch, dev, e)
    layers = torch.empty(4 * sum(sizes), dtype=torch.int32, device=dev)
    total = sum(lib.toyni_merkle_total_digests(h) for h in sizes)
    levels = torch.zeros((total, 32), dtype=torch.uint8, device=dev)
    d_salts = torch.from_numpy(np.concatenate(salts)).to(dev) if salted and salts else None
    roots = ta.prover.fri_commit_phase_ext_device(ctx, te.data_ptr(), m0, x0, final_size, d_salts.data_ptr() if d_salts is not None else 0,
                                                  challenge, layers.data_ptr(), levels.data_ptr())
    assert len(roots) == len(sizes) and state["seen"] == roots
    assert state["order"] == [(k, k > 0, True) for k in range(len(sizes))] + [(len(sizes), True, False)]
    launched = [k for k in ta._lib.launched_kernels() if "fri_fold_ext_commit_kernel" in k]
    assert any("ILb0E" in k for k in launched) and (not (salted and len(sizes) > 1) or any("ILb1E" in k for k in launched)), launched
    # replay on the CPU with the same transcript
    got_layers, got_levels = _host(layers).reshape(-1, 4), levels.cpu().numpy()
    t = b"toyni-test"
    cur, x, lo, dlo = e, x0, 0, 0
    for k, h in enumerate(sizes):
        if k:
            t = t + roots[k - 1]
        beta = []
        for _ in range(4):
            t = hashlib.sha256(t).digest()
            beta.append(int.from_bytes(t, "little") % P)
        want = oracle.fri_fold_ext(cur, oracle.domain_elements(2 * h, x), np.array(beta, dtype=np.uint64))
        assert (got_layers[lo:lo + h] == want).all(), k
        s = salts[k] if salted and k < len(sizes) - 1 else None
        tree = tree_of(want, s)
        nd = lib.toyni_merkle_total_digests(h)
        assert (got_levels[dlo:dlo + nd] == tree).all(), k
        assert got_levels[dlo + nd - 1].tobytes() == roots[k]
        cur, x, lo, dlo = want, x * x % P, lo + h, dlo + nd


# ---- failures ----
def test_phase_reports_a_failing_transcript_a_beta_outside_the_field_and_reentry(env):
    ta, torch, dev = env
    lib = ta._lib.lib
    ctx = ta.NttContext(64, device=dev.index)
    try:
        te = _dev(torch, dev, np.random.default_rng(1).integers(0, P, (64, 4)))
        layers = torch.empty(4 * 63, dtype=torch.int32, device=dev)
        levels = torch.zeros((200, 32), dtype=torch.uint8, device=dev)
        run = lambda cb: ta.prover.fri_commit_phase_ext_device(ctx, te.data_ptr(), 64, 7, 1, 0, cb, layers.data_ptr(), levels.data_ptr())

        def bad(rnd, root, want_beta):
            if rnd == 2:
                raise RuntimeError("transcript failure")
            return [5, 6, 7, 8]

        with pytest.raises(RuntimeError, match="transcript failure"):
            run(bad)
        assert torch.cuda.default_stream(dev).query()                            # the call has drained: nothing is still running
        # a beta coordinate outside the field is refused, not reduced silently -- whichever coordinate it is
        for k in range(4):
            with pytest.raises(ta._lib.ToyniError) as err:
                run(lambda r, root, w, k=k: [P if j == k else 1 for j in range(4)])
            assert err.value.status == E_RANGE
            assert torch.cuda.default_stream(dev).query()
        # an entry point on the same context from inside the callback
        scratch = torch.zeros(64, dtype=torch.int32, device=dev)
        seen = []

        def reenter(rnd, root, want_beta):
            seen.append(lib.toyni_ntt_device(ctx.handle, scratch.data_ptr(), scratch.data_ptr(), 1, 0, None))
            b = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
            seen.append(lib.toyni_fri_fold_commit_ext_device(ctx.handle, te.data_ptr(), layers.data_ptr(), 64, b, 7, None, levels.data_ptr(), None))
            return [1, 2, 3, 4]

        roots = run(reenter)
        assert len(roots) == 6 and len(seen) == 14 and all(st == E_REENTRANT for st in seen), seen
        assert lib.toyni_ntt_device(ctx.handle, scratch.data_ptr(), scratch.data_ptr(), 1, 0, None) == 0     # free again afterwards
        torch.cuda.synchronize()
    finally:
        ctx.destroy()


def test_the_refusals_that_need_a_context_leave_the_outputs_untouched(env):
    """What tests/test_fold_ext_commit_abi.py cannot ask without a device: a layer larger than the context's domain -- and, on real
    device memory, a sample of the refusals it does ask."""
    ta, torch, dev = env
    lib = ta._lib.lib
    ctx = ta.NttContext(64, device=dev.index)
    called = []
    cb = ta._lib.FRI_EXT_CHALLENGE_FN(lambda user, rnd, root, beta: called.append(rnd) or 1)
    try:
        with rc.Dev(ta) as d:
            g_e = d.put(np.random.default_rng(2).integers(0, P, 4 * 128).astype(np.uint32))
            g_out, g_lv = d.buf(16 * 64), d.buf(32 * 127, word=1)
            g_roots = Guarded(HostMem(), 32 * 8, word=1)
            beta = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
            bad_beta = (ctypes.c_uint32 * 4)(1, 2, P, 4)
            rounds = ctypes.c_uint(99)
            round_ = lambda m=64, b=beta, x0=7, o=g_out.ptr, lv=g_lv.ptr: \
                lib.toyni_fri_fold_commit_ext_device(ctx.handle, g_e.ptr, o, m, b, x0, None, lv, None)
            phase = lambda m0=64, x0=7, final=4, ls=g_out.ptr, lv=g_lv.ptr: \
                lib.toyni_fri_commit_phase_ext_device(ctx.handle, g_e.ptr, m0, x0, final, None, ctypes.cast(cb, ctypes.c_void_p), None, ls, lv,
                                                      g_roots.ptr, ctypes.byref(rounds), None)
            assert round_(m=128) == E_RANGE                                      # m > n
            assert round_(m=66) == E_RANGE and round_(b=bad_beta) == E_RANGE and round_(x0=P) == E_RANGE
            assert round_(o=g_out.ptr + 4) == E_RANGE and round_(lv=g_lv.ptr + 8) == E_RANGE
            assert round_(m=63) == 10003 and round_(x0=0) == 10005
            assert phase(m0=128) == E_INVALID_SIZE                               # m0 > n
            assert phase(m0=48) == E_INVALID_SIZE and phase(final=3) == E_INVALID_SIZE
            assert phase(x0=0) == 10005 and phase(x0=P) == E_RANGE and phase(ls=g_out.ptr + 8) == E_RANGE and phase(lv=g_lv.ptr + 4) == E_RANGE
            ctx.synchronize()
            assert not called and rounds.value == 99
            assert (g_out.download(np.uint8) == 0xA5).all() and (g_lv.download(np.uint8) == 0xA5).all()
            assert (g_roots.download(np.uint8) == 0xA5).all()
            g_roots.free()
            # nothing to fold is no refusal: rounds_out = 0, the transcript is not asked, nothing is written
            assert phase(m0=4, final=4) == 0 and rounds.value == 0 and not called
            assert round_(m=0) == 0
            ctx.synchronize()
            assert (g_out.download(np.uint8) == 0xA5).all() and (g_lv.download(np.uint8) == 0xA5).all()
    finally:
        ctx.destroy()


# ---- captured replay ----
def test_a_round_on_a_warm_context_can_be_captured_and_replayed(env):
    """One round = a single linear chain of launches (the fused sweep, then the node levels one after another): captured once,
    replayed on new contents.  The phase blocks on every root and cannot be captured."""
    ta, torch, dev = env
    lib = ta._lib.lib
    m = 1 << 10
    half = m // 2
    ndig = lib.toyni_merkle_total_digests(half)
    ctx = ta.NttContext(m, device=dev.index)
    rng = np.random.default_rng(5)
    beta, x0 = [3, 1, 4, 1], 7
    try:
        te = torch.zeros(4 * m, dtype=torch.int32, device=dev)
        ts = torch.zeros((half, 16), dtype=torch.uint8, device=dev)
        out, lv = torch.empty(4 * half, dtype=torch.int32, device=dev), torch.empty((ndig, 32), dtype=torch.uint8, device=dev)
        s = torch.cuda.Stream(device=dev)
        call = lambda: ta.prover.fri_fold_commit_ext_device(ctx, te.data_ptr(), out.data_ptr(), m, beta, x0, ts.data_ptr(), lv.data_ptr(),
                                                            stream=s.cuda_stream)
        call()                                                                  # eager, warm
        ctx.synchronize(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):                                     # kernel nodes in a line
            call()
        for rep in range(2):
            e = rng.integers(0, P, (m, 4), dtype=np.uint64)
            salts = rng.integers(0, 256, (half, 16), dtype=np.uint8)
            te.copy_(_dev(torch, dev, e)), ts.copy_(torch.from_numpy(salts))
            out.fill_(-1), lv.fill_(0xA5)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want = oracle.fri_fold_ext(e, oracle.domain_elements(m, x0), np.array(beta, dtype=np.uint64))
            assert (_host(out).reshape(half, 4) == want).all(), rep
            assert (lv.cpu().numpy() == tree_of(want, salts)).all(), rep
        del g
    finally:
        ctx.destroy()


# ---- a low-degree proof, end to end ----
N, LOG_BLOWUP, SHIFT, FINAL = 1 << 8, 2, 7, 4


def prove(env, coeffs, tamper_layer0=False, wrong_beta_round=None):
    """Ext coefficients -> LDE on the coset -> row commitment of layer 0 -> the Ext commit phase -> 8 queries -> every layer opened
    at lo and lo + m_k / 2.  tamper_layer0: one coordinate of layer 0 changes before it is committed.  wrong_beta_round: that round
    folds with a beta that is not the transcript's."""
    ta, torch, dev = env
    lib = ta._lib.lib
    ctx = ta.ntt.get_or_create_ctx(N)
    rng = np.random.default_rng(8)
    sizes = halves_of(N, FINAL)
    rounds = len(sizes)
    tc = _dev(torch, dev, coeffs)
    layer0 = torch.empty(4 * N, dtype=torch.int32, device=dev)
    ta._lib.check(lib.toyni_lde_ext_device(ctx.handle, tc.data_ptr(), layer0.data_ptr(), LOG_BLOWUP, SHIFT, None), "lde ext")
    if tamper_layer0:
        layer0[4 * 77 + 2] = (layer0[4 * 77 + 2] + 1) % P
    salts0 = torch.from_numpy(rng.integers(0, 256, (N, 16), dtype=np.uint8)).to(dev)
    levels0 = torch.zeros((lib.toyni_merkle_total_digests(N), 32), dtype=torch.uint8, device=dev)
    ta.merkle_commit_rows_device(layer0.data_ptr(), N, 4, ROW, 0, salts0.data_ptr(), levels0.data_ptr())
    torch.cuda.synchronize()
    root0 = levels0[-1].cpu().numpy().tobytes()
    tr = fv.Transcript()
    tr.absorb(root0)

    def challenge(rnd, root, want_beta):
        if root is not None:
            tr.absorb(root)
        if not want_beta:
            return None
        beta = tr.squeeze_ext()
        return em.add(beta, em.ONE) if rnd == wrong_beta_round else beta

    salts = torch.from_numpy(rng.integers(0, 256, (sum(sizes[:-1]), 16), dtype=np.uint8)).to(dev)
    layers = torch.empty(4 * sum(sizes), dtype=torch.int32, device=dev)
    ndigs = [lib.toyni_merkle_total_digests(h) for h in sizes]
    levels = torch.zeros((sum(ndigs), 32), dtype=torch.uint8, device=dev)
    roots = ta.prover.fri_commit_phase_ext_device(ctx, layer0.data_ptr(), N, SHIFT, FINAL, salts.data_ptr(), challenge, layers.data_ptr(),
                                                  levels.data_ptr())
    indices = [tr.squeeze() % N for _ in range(fv.NQUERIES)]
    # (values, tree, salts, size) of every layer, layer 0 first
    per_layer = [(layer0, levels0, salts0, N)]
    lo = dlo = slo = 0
    for k, h in enumerate(sizes):
        last = k == rounds - 1
        per_layer.append((layers[4 * lo:], levels[dlo:], None if last else salts[slo:], h))
        lo, dlo, slo = lo + h, dlo + ndigs[k], slo + (0 if last else h)
    openings = [[] for _ in indices]
    for values, tree, s, m in per_layer:
        pos = [p for i in indices for p in (i % (m // 2), i % (m // 2) + m // 2)]
        it = torch.tensor(pos, dtype=torch.int32, device=dev)
        rec = lib.toyni_merkle_open_rows_record_bytes(m, 4)
        out = torch.full((len(pos) * rec,), 0xA5, dtype=torch.uint8, device=dev)
        ta.merkle_open_rows_device(tree.data_ptr(), m, values.data_ptr(), 4, ROW, 0, s.data_ptr() if s is not None else 0, it.data_ptr(), len(pos),
                                   out.data_ptr())
        torch.cuda.synchronize()
        raw = out.cpu().numpy().tobytes()
        for q in range(len(indices)):
            openings[q].append([raw[(2 * q + j) * rec:(2 * q + j + 1) * rec] for j in range(2)])
    final = _host(layers[4 * (sum(sizes) - FINAL):]).reshape(FINAL, 4)
    return {"m0": N, "x0": SHIFT, "final_size": FINAL, "root0": root0, "roots": roots, "final_layer": [tuple(int(v) for v in e) for e in final],
            "openings": openings}


@pytest.fixture(scope="module")
def honest(env):
    coeffs = np.random.default_rng(64).integers(0, P, (N >> LOG_BLOWUP, 4), dtype=np.uint64)
    return coeffs, prove(env, coeffs)


def test_the_verifier_accepts_the_honest_low_degree_proof(honest):
    coeffs, proof = honest
    assert fv.verify(proof) == (True, "accepted")
    # the constant the folds arrive at is no accident of the verifier: the codeword had degree < 64 and six folds leave degree < 1
    assert len(proof["roots"]) == 6 and len(set(proof["final_layer"])) == 1


def test_the_verifier_rejects_a_layer_that_is_not_low_degree(env, honest):
    coeffs, _ = honest
    ok, why = fv.verify(prove(env, coeffs, tamper_layer0=True))                  # every fold and every path is honest; the word is not
    assert not ok and why == "the final layer is not constant", why


def test_the_verifier_rejects_one_changed_byte_of_an_opened_record(honest):
    _, proof = honest
    depth = rc.depth_of(N >> 2)
    for at in (5, 32 * depth + 16 + 9, 32 * depth + 3, 32 * depth + 48):        # a sibling, a value, the salt, a position flag
        bad = dict(proof, openings=[[list(layer) for layer in q] for q in proof["openings"]])
        rec = bytearray(bad["openings"][3][2][1])
        rec[at] ^= 0x40
        bad["openings"][3][2][1] = bytes(rec)
        ok, why = fv.verify(bad)
        assert not ok and why.startswith("query 3, layer 2"), why


def test_the_verifier_rejects_a_beta_that_is_not_the_transcripts(env, honest):
    coeffs, _ = honest
    ok, why = fv.verify(prove(env, coeffs, wrong_beta_round=2))
    assert not ok and "fold relation between layers 2 and 3" in why, why
