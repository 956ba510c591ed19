"""The calls of include/toyni_hip.h 3q on the device, each between guard bands (tests/guarded.py) against its host-argument
counterpart on the reduced values, and against Python integers where a model is a few lines:
  1. toyni_poly_eval_dz_device at ncoeffs in {0, 1, 4095, 4097, 64 + 140}, 1 and 3 points, z as it is and as z + p
  2. toyni_fib_deep_dz_device at log_N in {2, 3, 8, 11} (both paths of the kernel), d_check null and not, the check word on a tuple
     that satisfies the constraint and with each of the four values off by one, z on the coset
  3. toyni_mask_poly_device at n in {8, 128, 140, 141, 256} with mask_degree 140 and 1, against the ChaCha20 model of
     tests/harness/ref_prover.py
  4. toyni_transcript_squeeze_point_device on the six states "toyni-stark-v1" || LE64(i) that take 0 .. 5 rejections at log_N = 27
  5. toyni_fri_phase_roots_device on the trees of two commit phases (one wholly in the fused tail, one that ends in it)
  6. all five captured once into a graph and replayed after the transcript, z's source and the inputs were overwritten
Every comparison is exact."""
import hashlib
import os
import sys

import numpy as np
import pytest

from guarded import DevMem, Guarded
from test_emu_transcript import E_RANGE as TR_E_RANGE, Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

P = 2013265921
SHIFT = 7
POINT_STATES = [(0, 0), (3, 1), (92, 2), (19, 3), (8065, 4), (19425, 5)]   # i, rejections at log_N = 27, shift = 7


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


def root_of_unity(log_n):
    return pow(440564289, 1 << (27 - log_n), P)


def model_point(m, log_N, shift, tries=8):
    """derive_z_from_transcript on the transcript model: (z, rejections); after `tries` rejections the state stays and the status is set"""
    before, inv = m.state, pow(shift, P - 2, P)
    for k in range(tries):
        z = m.squeeze(1)[0]
        if pow(z, 1 << log_N, P) != 1 and pow(z * inv % P, 1 << log_N, P) != 1:
            return z, k
    m.state, m.status = before, TR_E_RANGE
    return 0, tries


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + int(c)) % P
    return acc


class Bufs:
    """Guarded buffers freed (and their bands checked) together."""

    def __init__(self, ta):
        self.mem = DevMem(ta)
        self.all = []

    def new(self, nbytes, word=4, arr=None):
        g = Guarded(self.mem, nbytes, seed=len(self.all) + 1, word=word)
        self.all.append(g)
        if arr is not None:
            g.upload(arr)
        return g

    def words(self, arr):
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.uint64).astype(np.uint32))
        return self.new(max(a.nbytes, 4), arr=a)

    def free(self):
        self.mem.sync()
        for k, g in enumerate(self.all):
            g.free()
        self.all = []


@pytest.fixture()
def bufs(ta):
    b = Bufs(ta)
    yield b
    b.free()


# ---- 1. the out-of-domain values ----
@pytest.mark.parametrize("ncoeffs", [0, 1, 4095, 4097, 64 + 140])
@pytest.mark.parametrize("npoints", [1, 3])
def test_evaluation_at_a_device_point_matches_the_host_point_call_and_horner(ta, bufs, ncoeffs, npoints):
    rng = np.random.default_rng(100 * ncoeffs + npoints)
    coeffs = rng.integers(0, P, ncoeffs, dtype=np.uint64)
    coeffs[:3] = [P - 1, 0, 1][:min(3, ncoeffs)]
    g = root_of_unity(6)
    mults = [1, g, g * g % P][:npoints]
    z = int(rng.integers(2, P))
    points = [m * z % P for m in mults]
    want = [horner(coeffs, x) for x in points]
    ctx = ta.NttContext(1 << 10)
    try:
        g_c, g_out, g_ref = bufs.words(coeffs), bufs.new(4 * npoints), bufs.new(4 * npoints)
        for lift in (0, P):                                  # z + p < 2^32: the same point as a word that needs the reduction
            g_z = bufs.words([z + lift])
            g_out.fill_sentinel()
            ta.prover.poly_eval_dz_device(ctx, g_c.ptr if ncoeffs else 0, ncoeffs, g_z.ptr, mults, g_out.ptr)
            bufs.mem.sync()
            assert g_out.download(np.uint32).tolist() == want, (ncoeffs, npoints, lift)
        ta.prover.poly_eval_device(ctx, g_c.ptr if ncoeffs else 0, ncoeffs, points, g_ref.ptr)
        bufs.mem.sync()
        assert g_ref.download(np.uint8).tobytes() == g_out.download(np.uint8).tobytes()
    finally:
        bufs.free()
        ctx.destroy()


# ---- 2. the DEEP layer and the constraint check ----
def fibonacci_tuple(rng, n, z):
    """(t_z, t_gz, t_ggz, q_z) with (t_ggz - t_gz - t_z)(z - g^(n-1))(z - g^(n-2)) == q_z (z^n - 1)"""
    g = root_of_unity(n.bit_length() - 1)
    t_z, t_gz, q_z = (int(v) for v in rng.integers(0, P, 3))
    den = (z - pow(g, n - 1, P)) * (z - pow(g, n - 2, P)) % P
    fib = q_z * (pow(z, n, P) - 1) % P * pow(den, P - 2, P) % P
    return [t_z, t_gz, (fib + t_gz + t_z) % P, q_z]


@pytest.mark.parametrize("log_N,log_b", [(2, 1), (3, 1), (8, 5), (11, 5)])
def test_deep_layer_from_device_values_matches_the_host_value_call(ta, bufs, log_N, log_b):
    N, n = 1 << log_N, 1 << (log_N - log_b)
    rng = np.random.default_rng(9000 + log_N)
    trace, quot = rng.integers(0, P, N, dtype=np.uint64), rng.integers(0, P, N, dtype=np.uint64)
    ctx = ta.NttContext(N)
    try:
        g_t, g_q, g_out, g_ref = bufs.words(trace), bufs.words(quot), bufs.new(4 * N), bufs.new(4 * N)
        on_coset = SHIFT * pow(root_of_unity(log_N), N - 1, P) % P               # x_i = z at the last point: that point alone is 0
        for z in (int(rng.integers(2, P)), on_coset):
            good = fibonacci_tuple(rng, n, z)
            cases = [(good, 1)] + [([(v + (k == j)) % P for k, v in enumerate(good)], 0) for j in range(4)]
            for ood, holds in cases:
                ta.prover.fib_deep_device(ctx, g_t.ptr, g_q.ptr, g_ref.ptr, log_b, SHIFT, z, ood)
                bufs.mem.sync()
                ref = g_ref.download(np.uint8).tobytes()
                for lift, with_check in ((0, True), (P, True), (0, False)):
                    g_z, g_o, g_c = bufs.words([z + lift]), bufs.words([v + lift for v in ood]), bufs.new(4)
                    g_out.fill_sentinel()
                    ta.prover.fib_deep_dz_device(ctx, g_t.ptr, g_q.ptr, g_out.ptr, log_b, SHIFT, g_z.ptr, g_o.ptr, n, g_c.ptr if with_check else 0)
                    bufs.mem.sync()
                    assert g_out.download(np.uint8).tobytes() == ref, (log_N, z, ood, lift)
                    assert g_c.download(np.uint32).tolist() == [holds if with_check else 0xA5A5A5A5], (log_N, z, ood, lift)
            if z == on_coset:
                assert g_out.download(np.uint32)[N - 1] == 0
    finally:
        bufs.free()
        ctx.destroy()


def test_the_refusal_that_reads_the_context_leaves_the_output_untouched(ta, bufs):
    N = 64
    ctx = ta.NttContext(N)
    try:
        g_t, g_out, g_z, g_o, g_c = bufs.words(np.arange(N)), bufs.new(4 * N), bufs.words([5]), bufs.words([1, 2, 3, 4]), bufs.new(4)
        rc = ta._lib.lib.toyni_fib_deep_dz_device(ctx.handle, g_t.ptr, g_t.ptr, g_out.ptr, 7, SHIFT, g_z.ptr, g_o.ptr, 1, g_c.ptr, None)   # 2^7 > N
        assert rc == 10006
        bufs.mem.sync()
        assert (g_out.download(np.uint8) == 0xA5).all() and (g_c.download(np.uint8) == 0xA5).all()
        ta.prover.fib_deep_dz_device(ctx, g_t.ptr, g_t.ptr, g_out.ptr, 6, SHIFT, g_z.ptr, g_o.ptr, 1, g_c.ptr)   # the largest blow-up is fine
        bufs.mem.sync()
        assert (g_out.download(np.uint32) < P).all()
    finally:
        bufs.free()
        ctx.destroy()


# ---- 3. the mask ----
@pytest.mark.parametrize("n", [8, 128, 140, 141, 256])
@pytest.mark.parametrize("mask_degree", [140, 1])
def test_mask_matches_the_keystream_model(ta, bufs, n, mask_degree):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from harness import ref_prover
    rng = np.random.default_rng(n * 1000 + mask_degree)
    key = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    total = n + mask_degree
    coeffs = np.zeros(total + 5, dtype=np.uint64)
    coeffs[:n] = rng.integers(0, P, n)
    coeffs[total:] = 0xFFFFFFF0                               # words behind the polynomial: not touched
    if n > mask_degree + 2:
        coeffs[mask_degree + 1] = P + 5                      # between the two ranges: not touched either, not even reduced
    r = ref_prover.ChaChaRandomness(key).mask(mask_degree)
    want = [int(v) for v in coeffs]
    for j in range(total):
        v = want[j]
        if j < mask_degree:
            v = (v - r[j]) % P
        if n <= j < n + mask_degree:
            v = (v + r[j - n]) % P
        want[j] = v
    g_c = bufs.words(coeffs)
    ta.prover.mask_poly_device(g_c.ptr, n, mask_degree, key, 1)
    bufs.mem.sync()
    assert g_c.download(np.uint32).tolist() == want, (n, mask_degree)
    # the host loop of csrc/host/fib_prover.hpp says the same: T_hat(x) = T(x) + (x^n - 1) R(x) at a point
    x = 123456789
    t = horner(coeffs[:n], x)
    assert horner(want[:total], x) == (t + (pow(x, n, P) - 1) * horner(r, x)) % P


# ---- 4. derive_z ----
@pytest.mark.parametrize("i,rejections", POINT_STATES)
def test_point_squeeze_on_the_states_that_take_0_to_5_rejections(ta, bufs, i, rejections):
    state = b"toyni-stark-v1" + i.to_bytes(8, "little")
    m = Model(state)
    z, k = model_point(m, 27, SHIFT)
    assert k == rejections                                   # the cases are what the docstring says they are
    tr = ta.prover.DeviceTranscript.from_bytes(state)
    try:
        g_z, g_c = bufs.new(4), bufs.new(12)
        tr.squeeze_point(g_z.ptr, 27, SHIFT)
        bufs.mem.sync()
        assert g_z.download(np.uint32).tolist() == [z] and tr.download() == (m.state, 0)
        tr.squeeze(g_c.ptr, 3)                               # the continuation
        bufs.mem.sync()
        assert g_c.download(np.uint32).tolist() == m.squeeze(3)
    finally:
        tr.free()


def test_point_squeeze_on_a_set_status_writes_zero(ta, bufs):
    tr = ta.prover.DeviceTranscript.from_bytes(b"x" * 1000)
    try:
        g_b, g_z = bufs.new(16, word=1, arr=np.zeros(16, dtype=np.uint8)), bufs.new(4)
        tr.absorb_device(g_b.ptr, 16)                        # 1016 > 1008: the status is set
        tr.squeeze_point(g_z.ptr, 10, SHIFT)
        bufs.mem.sync()
        assert g_z.download(np.uint32).tolist() == [0] and tr.download() == (b"x" * 1000, TR_E_RANGE)
    finally:
        tr.free()


# ---- 5. the roots of a phase ----
@pytest.mark.parametrize("log_m0,final_size", [(9, 4), (12, 8)])
def test_phase_roots_are_the_last_digest_of_every_tree(ta, bufs, log_m0, final_size):
    lib = ta._lib.lib
    m0 = 1 << log_m0
    rng = np.random.default_rng(log_m0)
    sizes, m = [], m0
    while m > final_size:
        m //= 2
        sizes.append(m)
    ndigs = [lib.toyni_merkle_total_digests(h) for h in sizes]
    ctx = ta.NttContext(m0)
    tr = ta.prover.DeviceTranscript.from_bytes(b"roots")
    try:
        g_l0 = bufs.words(rng.integers(0, P, m0))
        g_layers, g_levels, g_roots = bufs.new(4 * sum(sizes)), bufs.new(32 * sum(ndigs), word=1), bufs.new(32 * len(sizes), word=1)
        ta.prover.fri_commit_phase_transcript_device(ctx, g_l0.ptr, m0, SHIFT, final_size, 0, tr, g_layers.ptr, g_levels.ptr)
        ta.prover.fri_phase_roots_device(g_levels.ptr, m0 // 2, len(sizes), g_roots.ptr)
        bufs.mem.sync()
        levels = g_levels.download(np.uint8).reshape(-1, 32)
        ends = np.cumsum(ndigs) - 1
        got = g_roots.download(np.uint8).reshape(-1, 32)
        assert (got == levels[ends]).all()
        assert len({r.tobytes() for r in got}) == len(sizes)                      # real digests, all different
        g_roots.fill_sentinel()
        ta.prover.fri_phase_roots_device(g_levels.ptr, m0 // 2, 1, g_roots.ptr)   # fewer rounds: the rest stays
        bufs.mem.sync()
        got = g_roots.download(np.uint8).reshape(-1, 32)
        assert (got[0] == levels[ends[0]]).all() and (got[1:] == 0xA5).all()
    finally:
        tr.free()
        bufs.free()
        ctx.destroy()


# ---- 6. the calls in a graph ----
def test_the_calls_replay_from_a_graph_on_new_words(ta):
    """squeeze_point, the evaluations, their absorb, the DEEP layer with its check, the mask and the phase roots captured ONCE;
    replayed after the transcript, the coefficients and the trees were replaced: every output must be that of the NEW words."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from harness import ref_prover
    pv = ta.prover
    tdev = torch.device("cuda", 0)
    n, log_b, md = 64, 1, 5
    N, log_N = n << log_b, 7
    rng = np.random.default_rng(606)
    g_mult = root_of_unity(6)
    mults = [1, g_mult, g_mult * g_mult % P]
    key = bytes(range(32))
    ctx = ta.NttContext(N)
    tr = pv.DeviceTranscript()
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64).astype(np.uint32)).view(np.int32)).to(tdev)
    try:
        trace_h, quot_h = rng.integers(0, P, N, dtype=np.uint64), rng.integers(0, P, N, dtype=np.uint64)
        trace, quot = as_dev(trace_h), as_dev(quot_h)
        coef = torch.zeros(n + md, dtype=torch.int32, device=tdev)
        levels = torch.zeros((2 * 8 - 1) + (2 * 4 - 1), 8, dtype=torch.int32, device=tdev)       # trees of 8 and 4 leaves
        z, ood, chk, deep, ref, roots = (torch.empty(k, dtype=torch.int32, device=tdev) for k in (1, 4, 1, N, N, 16))
        s = torch.cuda.Stream(device=tdev)

        def segment():
            st = s.cuda_stream
            pv.mask_poly_device(coef.data_ptr(), n, md, key, 1, st)
            tr.squeeze_point(z.data_ptr(), log_N, SHIFT, st)
            pv.poly_eval_dz_device(ctx, coef.data_ptr(), n + md, z.data_ptr(), mults, ood.data_ptr(), stream=st)
            pv.poly_eval_dz_device(ctx, quot.data_ptr(), N, z.data_ptr(), mults[:1], ood.data_ptr() + 12, stream=st)
            tr.absorb_fields(ood.data_ptr(), 4, st)
            pv.fib_deep_dz_device(ctx, trace.data_ptr(), quot.data_ptr(), deep.data_ptr(), log_b, SHIFT, z.data_ptr(), ood.data_ptr(), n, chk.data_ptr(), st)
            pv.fri_phase_roots_device(levels.data_ptr(), 8, 2, roots.data_ptr(), st)

        r = ref_prover.ChaChaRandomness(key).mask(md)

        def load(seed, state):
            c = np.random.default_rng(seed).integers(0, P, n, dtype=np.uint64)
            lv = np.random.default_rng(seed + 1).integers(0, 1 << 32, levels.numel(), dtype=np.uint64)
            coef.copy_(as_dev(np.concatenate([c, np.zeros(md, dtype=np.uint64)])))
            levels.copy_(as_dev(lv).reshape(levels.shape))
            tr.load(state, s.cuda_stream)
            masked = [int(v) for v in c] + [0] * md
            for j in range(md):
                masked[j] = (masked[j] - r[j]) % P
                masked[n + j] = (masked[n + j] + r[j]) % P
            torch.cuda.synchronize()
            return masked, lv.reshape(-1, 8)

        load(1, b"warm")
        segment()                                            # eager first: code objects loaded, the context's buffer grown
        ctx.synchronize(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            segment()
        for seed, state in ((10, b"first state"), (20, hashlib.sha256(b"second").digest() + b"x" * 9)):
            masked, lv = load(seed, state)
            for t in (z, ood, chk, deep, roots):
                t.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            m = Model(state)
            zz, _ = model_point(m, log_N, SHIFT)
            vals = [horner(masked, mlt * zz % P) for mlt in mults] + [horner(quot_h, zz)]
            m.absorb(b"".join(v.to_bytes(8, "little") for v in vals))
            assert coef.cpu().numpy().view(np.uint32).tolist() == masked
            assert z.cpu().numpy().view(np.uint32).tolist() == [zz]
            assert ood.cpu().numpy().view(np.uint32).tolist() == vals
            assert tr.download() == (m.state, 0)
            gg = root_of_unity(6)
            holds = (vals[2] - vals[1] - vals[0]) * (zz - pow(gg, n - 1, P)) * (zz - pow(gg, n - 2, P)) % P == vals[3] * (pow(zz, n, P) - 1) % P
            assert chk.cpu().numpy().view(np.uint32).tolist() == [int(holds)]
            pv.fib_deep_device(ctx, trace.data_ptr(), quot.data_ptr(), ref.data_ptr(), log_b, SHIFT, zz, vals, s.cuda_stream)
            torch.cuda.synchronize()
            assert (deep.cpu().numpy() == ref.cpu().numpy()).all()
            assert (roots.cpu().numpy().view(np.uint32).reshape(2, 8) == lv[[14, 21]]).all()
        del g
    finally:
        tr.free()
        ctx.destroy()
