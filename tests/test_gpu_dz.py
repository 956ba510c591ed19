"""The calls of include/toyni_hip.h 3o on the device, each against Python integers (tests/ext_model.py), hashlib and the transcript model
of tests/test_emu_transcript.py; equality with the host-argument call of 3h is a second assertion, never the only one.
  1. squeeze_ext_point and absorb_fields: the words, the state afterwards and the continuation; a set status gives zeros; an overflow
     the host cannot see; the same calls on a second stream
  2. toyni_poly_eval_ext_batch_dz_device at ncoeffs in {1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 5}, 1..4 points, batch 1 and 3,
     guard bands round z and the output, device words that need the reduction
  3. toyni_deep_combine_ext_dz_device at N in {2, 4, 1024} with 1, 64 and 65 slots (the inline and the table form), accumulate on and
     off, aligned and misaligned columns, z on the coset; every refusal that needs a real context
  4. toyni_query_rows_device
  5. the whole segment from z to the DEEP layer captured into a graph and replayed on a different transcript state
The preparation record lives in the context's own per-stream buffer, which no caller can put guard bands round: what guards it here
is that the partial sums and the record share that buffer and every output is still the model's.  Every comparison is exact."""
import hashlib

import numpy as np
import pytest

import ext_model as em
from guarded import DevMem, Guarded
from test_emu_transcript import E_RANGE as TR_E_RANGE, Model, pattern
from test_gpu_deep_ext import Dev, ext_term_set, padded_words, rand_ext, rand_field

pytestmark = pytest.mark.gpu

P = em.P
E_NULL, E_RANGE = 10002, 10006
POLY_SHAPES = [(1, 1, 1), (15, 2, 3), (16, 3, 1), (17, 4, 3), (4095, 1, 3), (4096, 2, 1), (4097, 3, 3), (2 * 4096 + 5, 4, 1)]   # ncoeffs, npoints, batch


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


@pytest.fixture()
def dev(ta):
    d = Dev(ta)
    yield d
    d.free()


def field_bytes(words):
    return b"".join((int(w) % P).to_bytes(8, "little") for w in words)


def model_point(m):
    """derive_z on the model: four challenges, again while z1 = z2 = z3 = 0"""
    while True:
        z = m.squeeze(4)
        if any(z[1:]) or m.status:
            return z


# ---- 1. the transcript helpers ----
def test_point_and_field_absorb_match_the_model_and_continue_as_it_does(ta, dev):
    rng = np.random.default_rng(1)
    for count in (0, 1, 4, 96, 126):
        state0 = pattern(0 if count == 126 else 46, count)
        words = rng.integers(0, 1 << 32, size=count, dtype=np.uint64)
        if count >= 4:
            words[:4] = [0, P - 1, P, (1 << 32) - 1]
        m = Model(state0)
        tr = ta.prover.DeviceTranscript.from_bytes(state0)
        try:
            d_w, d_z, d_c = dev.up(words.astype(np.uint32)), dev.alloc(4), dev.alloc(3)
            dev.fill(d_z, 4)
            tr.absorb_fields(d_w, count)
            m.absorb(field_bytes(words))
            dev.mem.sync()
            assert tr.download() == (m.state, 0), count
            tr.squeeze_ext_point(d_z)
            assert dev.down(d_z, 4).tolist() == model_point(m) and tr.download() == (m.state, 0), count
            tr.squeeze(d_c, 3)                               # the continuation
            assert dev.down(d_c, 3).tolist() == m.squeeze(3), count
        finally:
            tr.free()
        dev.free()


def test_a_set_status_gives_zeros_and_an_unseen_overflow_sets_it(ta, dev):
    tr = ta.prover.DeviceTranscript.from_bytes(pattern(241, 3))
    try:
        d_w, d_z = dev.up(np.arange(96)), dev.alloc(4)
        dev.fill(d_z, 4)
        tr.absorb_fields(d_w, 96)                           # 241 + 768 = 1009
        dev.mem.sync()
        assert tr.download() == (pattern(241, 3), TR_E_RANGE)
        tr.squeeze_ext_point(d_z)
        assert dev.down(d_z, 4).tolist() == [0, 0, 0, 0] and tr.download() == (pattern(241, 3), TR_E_RANGE)
        tr.absorb_fields(d_w, 1)
        dev.mem.sync()
        assert tr.download() == (pattern(241, 3), TR_E_RANGE)
    finally:
        tr.free()


def test_the_transcript_helpers_twice_and_on_a_second_stream(ta, dev):
    lib = ta._lib.lib
    import ctypes
    s = ctypes.c_void_p()
    assert lib.toyni_stream_create(ctypes.byref(s), 0) == 0
    try:
        for stream in (0, s.value):
            m = Model(b"two streams")
            tr = ta.prover.DeviceTranscript.from_bytes(b"two streams", stream)
            d_w, d_z, want = dev.up([5, P + 5, 7]), dev.alloc(8), []
            for rep in range(2):
                tr.absorb_fields(d_w, 3, stream)
                m.absorb(field_bytes([5, 5, 7]))
                tr.squeeze_ext_point(d_z + 16 * rep, stream)
                want += model_point(m)
            assert lib.toyni_stream_synchronize(None, stream or None) == 0
            assert dev.down(d_z, 8).tolist() == want and tr.download() == (m.state, 0), stream
            tr.free()
    finally:
        assert lib.toyni_stream_destroy(s) == 0


# ---- 2. the out-of-domain values ----
@pytest.fixture(scope="module")
def poly_cases():
    """(shape, columns, z, multipliers, the integer model's values), computed once"""
    rng = np.random.default_rng(22)
    g = pow(31, (P - 1) >> 10, P)
    cases = []
    for ncoeffs, npoints, batch in POLY_SHAPES:
        cols = rand_field(rng, batch, ncoeffs)
        cols[0, :min(3, ncoeffs)] = [P - 1, 0, 1][:min(3, ncoeffs)]
        z = rand_ext(rng)
        mults = [1, g, P - 1, int(rng.integers(2, P))][:npoints]
        points = [tuple(c * mlt % P for c in z) for mlt in mults]
        want = np.array(em.poly_eval_ext_batch_model([[int(v) for v in col] for col in cols], points), dtype=np.uint32).reshape(batch, npoints, 4)
        cases.append(((ncoeffs, npoints, batch), cols, z, mults, points, want))
    return cases


@pytest.mark.parametrize("k", range(len(POLY_SHAPES)))
def test_evaluation_at_device_points_matches_the_model_and_the_host_point_call(ta, poly_cases, k):
    (ncoeffs, npoints, batch), cols, z, mults, points, want = poly_cases[k]
    mem = DevMem(ta)
    stride = ncoeffs + 3
    coeffs = np.full(batch * stride, 0xFFFFFFF0, dtype=np.uint32)
    for b in range(batch):
        coeffs[b * stride:b * stride + ncoeffs] = cols[b]
    ctx = ta.NttContext(1 << 10)
    g_c, g_z, g_out, g_ref = Guarded(mem, coeffs.nbytes, seed=1), Guarded(mem, 16, seed=2), Guarded(mem, 16 * batch * npoints, seed=3), Guarded(mem, 16 * batch * npoints, seed=4)
    try:
        g_c.upload(coeffs)
        for lift in (0, P):                                  # the same z as words that need the reduction (z_k + p < 2^32)
            g_z.upload(np.array([c + lift for c in z], dtype=np.uint32))
            ta.prover.poly_eval_ext_batch_dz_device(ctx, g_c.ptr, ncoeffs, stride, batch, g_z.ptr, mults, g_out.ptr)
            mem.sync()
            got = g_out.download(np.uint32).reshape(batch, npoints, 4)
            assert (got == want).all(), (ncoeffs, npoints, batch, lift)
        ta.prover.poly_eval_ext_batch_device(ctx, g_c.ptr, ncoeffs, stride, batch, points, g_ref.ptr)
        mem.sync()
        assert g_ref.download(np.uint8).tobytes() == g_out.download(np.uint8).tobytes()
        for name, g in (("coeffs", g_c), ("z", g_z), ("out", g_out), ("ref", g_ref)):
            g.check(name)
    finally:
        for g in (g_c, g_z, g_out, g_ref):
            g.free()
        ctx.destroy()


def test_evaluation_of_nothing(ta, dev):
    ctx = ta.NttContext(64)
    try:
        d_z, d_out = dev.up([1, 2, 3, 4]), dev.alloc(2 * 2 * 4)
        dev.fill(d_out, 16)
        ta.prover.poly_eval_ext_batch_dz_device(ctx, 0, 0, 0, 2, d_z, [1, 5], d_out)           # zero polynomials
        assert not dev.down(d_out, 16).any()
        dev.fill(d_out, 16)
        ta.prover.poly_eval_ext_batch_dz_device(ctx, d_z, 4, 4, 0, d_z, [1, 5], d_out)         # no columns: nothing written
        assert (dev.down(d_out, 16) == 0xA5A5A5A5).all()
    finally:
        ctx.destroy()


# ---- 3. the DEEP layer ----
def slots_of(ta, terms, rng, spare=3):
    """terms (column, rotation, alpha4, value4) -> (slot table, weights array, values array): the elements shuffled into arrays that
    hold `spare` more, so that an index is not its term's number"""
    n = len(terms)
    ai, vi = rng.permutation(n + spare)[:n], rng.permutation(n + spare)[:n]
    al, cl = rand_field(rng, n + spare, 4), rand_field(rng, n + spare, 4)
    for t, (_, _, a, v) in enumerate(terms):
        al[ai[t]], cl[vi[t]] = a, v
    return ta.prover.deep_ext_slots([t[0] for t in terms], [t[1] for t in terms], ai, vi), al.astype(np.uint32), cl.astype(np.uint32)


@pytest.mark.parametrize("log_n,log_b,nslots", [(1, 0, 1), (1, 1, 64), (2, 1, 65), (2, 0, 64), (10, 2, 1), (10, 2, 64), (10, 3, 65)])
def test_combination_from_device_values_matches_the_model_and_the_host_value_call(ta, dev, log_n, log_b, nslots):
    N, B, width = 1 << log_n, 1 << log_b, 5
    rng = np.random.default_rng(7000 + 100 * log_n + nslots)
    cs, shift = N + 20, 7
    xs = em.coset_points(N, shift)
    ctx = ta.NttContext(N)
    try:
        for off in (0, 4):                                   # aligned and misaligned columns: both load widths
            m = rand_field(rng, width, N)
            terms = ext_term_set(rng, width, nslots, N >> log_b)
            slots, al, cl = slots_of(ta, terms, rng)
            terms2 = ext_term_set(rng, width, 3, N >> log_b)
            slots2, al2, cl2 = slots_of(ta, terms2, rng)
            for z in (rand_ext(rng), em.embed(xs[N - 1])):   # the second: x_i = z at the last point of the last group
                lift = P if off else 0                       # misaligned pass: every device-resident challenge word needs the reduction
                d_m, d_out, d_ref = dev.up(padded_words(m, cs), off), dev.alloc(4 * N), dev.alloc(4 * N)
                d_z = dev.up(np.array([c + lift for c in z], dtype=np.uint64).astype(np.uint32))
                d_al, d_cl = dev.up((al.astype(np.uint64) + lift).astype(np.uint32)), dev.up((cl.astype(np.uint64) + lift).astype(np.uint32))
                d_al2, d_cl2 = dev.up(al2), dev.up(cl2)
                dev.fill(d_out, 4 * N)
                ta.prover.deep_combine_ext_dz_device(ctx, d_m, width, cs, log_b, shift, d_z, d_al, d_cl, slots, d_out)
                want = em.deep_ext_model(m, terms, B, shift, z)
                got = dev.down(d_out, 4 * N).reshape(N, 4)
                assert (got == want).all(), (log_n, nslots, off, z)
                if not any(z[1:]):
                    assert not got[N - 1].any()
                ta.prover.deep_combine_ext_dz_device(ctx, d_m, width, cs, log_b, shift, d_z, d_al2, d_cl2, slots2, d_out, accumulate=True)
                want2 = (want.astype(np.uint64) + em.deep_ext_model(m, terms2, B, shift, z)) % np.uint64(P)
                got2 = dev.down(d_out, 4 * N).reshape(N, 4)
                assert (got2 == want2).all(), (log_n, nslots, off, z)
                # the host-value call on the same values: the same bytes
                ta.prover.deep_combine_ext_device(ctx, d_m, width, cs, log_b, shift, z, ta.prover.deep_ext_terms(*zip(*terms)), d_ref)
                ta.prover.deep_combine_ext_device(ctx, d_m, width, cs, log_b, shift, z, ta.prover.deep_ext_terms(*zip(*terms2)), d_ref, accumulate=True)
                assert (dev.down(d_ref, 4 * N).reshape(N, 4) == got2).all()
                dev.free()
    finally:
        ctx.destroy()


def test_combination_guard_bands_and_no_slots(ta):
    mem = DevMem(ta)
    N, width, log_b = 64, 3, 1
    rng = np.random.default_rng(5)
    m = rand_field(rng, width, N)
    terms = ext_term_set(rng, width, 9, N >> log_b)
    slots, al, cl = slots_of(ta, terms, rng, spare=0)
    z = rand_ext(rng)
    ctx = ta.NttContext(N)
    bufs = [Guarded(mem, 4 * width * N, seed=1), Guarded(mem, 16, seed=2), Guarded(mem, al.nbytes, seed=3), Guarded(mem, cl.nbytes, seed=4), Guarded(mem, 16 * N, seed=5)]
    g_m, g_z, g_al, g_cl, g_out = bufs
    try:
        g_m.upload(m.astype(np.uint32).reshape(-1)), g_z.upload(np.array(z, dtype=np.uint32)), g_al.upload(al), g_cl.upload(cl)
        ta.prover.deep_combine_ext_dz_device(ctx, g_m.ptr, width, N, log_b, 7, g_z.ptr, g_al.ptr, g_cl.ptr, slots, g_out.ptr)
        mem.sync()
        want = em.deep_ext_model(m, terms, 1 << log_b, 7, z)
        assert (g_out.download(np.uint32).reshape(N, 4) == want).all()
        none = ta.prover.deep_ext_slots([], [], [], [])
        ta.prover.deep_combine_ext_dz_device(ctx, g_m.ptr, width, N, log_b, 7, g_z.ptr, g_al.ptr, g_cl.ptr, none, g_out.ptr, accumulate=True)
        mem.sync()
        assert (g_out.download(np.uint32).reshape(N, 4) == want).all()                          # left alone
        ta.prover.deep_combine_ext_dz_device(ctx, g_m.ptr, width, N, log_b, 7, g_z.ptr, g_al.ptr, g_cl.ptr, none, g_out.ptr)
        mem.sync()
        assert not g_out.download(np.uint32).any()                                              # zeros
        for k, g in enumerate(bufs):
            g.check(f"buffer {k}")
    finally:
        for g in bufs:
            g.free()
        ctx.destroy()


def test_every_refusal_of_the_combination_leaves_the_output_untouched(ta, dev):
    lib = ta._lib.lib
    N, width = 64, 3
    ctx = ta.NttContext(N)
    try:
        d_m, d_out, d_z, d_al, d_cl = dev.up(np.arange(width * N)), dev.alloc(4 * N), dev.up([9, 1, 2, 3]), dev.up(np.arange(8)), dev.up(np.arange(8))
        dev.fill(d_out, 4 * N)
        good = ta.prover.deep_ext_slots([0, 2], [0, 3], [0, 1], [1, 0])

        def deep(m=d_m, w=width, cs=N, lb=2, shift=7, z=d_z, a=d_al, c=d_cl, slots=good, n=2, acc=0, out=d_out, handle=ctx.handle):
            return lib.toyni_deep_combine_ext_dz_device(handle, m, w, cs, lb, shift, z, a, c, slots, n, acc, out, None)

        one = lambda c, r, ai, vi: ta.prover.deep_ext_slots([c], [r], [ai], [vi])
        nulls = [deep(handle=None), deep(m=None), deep(out=None), deep(slots=None), deep(z=None), deep(a=None), deep(c=None)]
        assert all(rc == E_NULL for rc in nulls), nulls
        cases = [deep(shift=0), deep(shift=P), deep(lb=7), deep(cs=N - 1), deep(w=0), deep(w=65537), deep(slots=one(3, 0, 0, 0), n=1),
                 deep(slots=one(0, 16, 0, 0), n=1), deep(slots=one(0, 0, 1 << 20, 0), n=1), deep(slots=one(0, 0, 0, 1 << 20), n=1), deep(m=d_m + 2),
                 deep(z=d_z + 2), deep(a=d_al + 1), deep(c=d_cl + 3), deep(out=d_out + 4), deep(out=d_out + 8), deep(out=d_out + 1)]
        assert all(rc == E_RANGE for rc in cases), cases
        big = (ta.prover.DeepExtSlot * ((1 << 20) + 1))()
        assert deep(slots=big, n=(1 << 20) + 1) == E_RANGE
        assert (dev.down(d_out, 4 * N) == 0xA5A5A5A5).all()
        assert deep(slots=one(0, 15, 1, 1), n=1) == 0                                            # the largest rotation is fine
    finally:
        ctx.destroy()


# ---- 4. the rows of a query ----
def test_query_rows(ta, dev):
    rng = np.random.default_rng(4)
    for n, offsets, idx in ((1, [0], [0, 5, (1 << 32) - 1]), (1 << 32, [0, (1 << 32) - 1], [0, 1, (1 << 32) - 1, 12345]),
                            (1 << 14, [0, 4], rng.integers(0, 1 << 13, size=8).tolist()), (96, [0, 95, 1, 2, 3, 5, 8, 13], [0, 95, 96, 4000000000]),
                            (1 << 20, [(1 << 20) - 1], rng.integers(0, 1 << 20, size=700).tolist())):
        d_i, d_o = dev.up(np.array(idx, dtype=np.uint64).astype(np.uint32)), dev.alloc(len(idx) * len(offsets) + 4)
        dev.fill(d_o, len(idx) * len(offsets) + 4)
        ta.prover.query_rows_device(d_i, len(idx), n, offsets, d_o)
        got = dev.down(d_o, len(idx) * len(offsets) + 4)
        assert got[:-4].tolist() == [(i + o) % n for i in idx for o in offsets] and (got[-4:] == 0xA5A5A5A5).all(), n


# ---- 5. the segment in a graph ----
def test_the_segment_replays_from_a_graph_on_another_transcript_state(ta):
    """z, the out-of-domain values, their absorb, the weights and the DEEP layer captured ONCE; replayed after the transcript's bytes
    were replaced: every output must be that of the NEW state -- nothing of z was baked in at capture."""
    import torch
    pv = ta.prover
    tdev = torch.device("cuda", 0)
    n, log_b, width = 64, 1, 2
    N = n << log_b
    rng = np.random.default_rng(77)
    g_mult = pow(31, (P - 1) // n, P)
    ctx_n, ctx_N = ta.NttContext(n), ta.NttContext(N)
    tr = pv.DeviceTranscript()
    try:
        coef_h = rand_field(rng, width, n)
        lde_h = rand_field(rng, width, N)
        coef = torch.from_numpy(coef_h.astype(np.uint32).view(np.int32).reshape(-1)).to(tdev)
        lde = torch.from_numpy(lde_h.astype(np.uint32).view(np.int32).reshape(-1)).to(tdev)
        nterms = 2 * width
        z, ood, w, deep = (torch.empty(k, dtype=torch.int32, device=tdev) for k in (4, 4 * nterms, 4 * nterms, 4 * N))
        slot_list = [(c, r, 2 * c + r, 2 * c + r) for c in range(width) for r in (0, 1)]
        slots = pv.deep_ext_slots(*zip(*slot_list))
        s = torch.cuda.Stream(device=tdev)

        def segment():
            st = s.cuda_stream
            tr.squeeze_ext_point(z.data_ptr(), st)
            pv.poly_eval_ext_batch_dz_device(ctx_n, coef.data_ptr(), n, n, width, z.data_ptr(), [1, g_mult], ood.data_ptr(), stream=st)
            tr.absorb_fields(ood.data_ptr(), 4 * nterms, st)
            tr.squeeze(w.data_ptr(), 4 * nterms, st)
            pv.deep_combine_ext_dz_device(ctx_N, lde.data_ptr(), width, N, log_b, 7, z.data_ptr(), w.data_ptr(), ood.data_ptr(), slots, deep.data_ptr(), stream=st)

        def model(state):
            m = Model(state)
            zz = tuple(model_point(m))
            pts = [zz, tuple(c * g_mult % P for c in zz)]
            vals = em.poly_eval_ext_batch_model([[int(v) for v in col] for col in coef_h], pts)
            vals = [tuple(int(c) for c in v) for v in np.array(vals).reshape(-1, 4)]
            m.absorb(field_bytes([c for v in vals for c in v]))
            ws = m.squeeze(4 * nterms)
            terms = [(c, r, tuple(ws[4 * a:4 * a + 4]), vals[v]) for c, r, a, v in slot_list]
            return zz, vals, em.deep_ext_model(lde_h, terms, 1 << log_b, 7, zz), m.state

        tr.load(b"warm", s.cuda_stream)
        segment()                                            # eager first: code objects loaded, the contexts' buffers grown
        ctx_N.synchronize(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            segment()
        for state in (b"first state", hashlib.sha256(b"second").digest() + b"x" * 9):
            tr.load(state, s.cuda_stream)
            for t in (z, ood, w, deep):
                t.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            zz, vals, want, after = model(state)
            assert tuple(int(v) for v in z.cpu().numpy().view(np.uint32)) == zz
            assert [tuple(int(c) for c in v) for v in ood.cpu().numpy().view(np.uint32).reshape(-1, 4)] == vals
            assert (deep.cpu().numpy().view(np.uint32).reshape(N, 4) == want).all()
            assert tr.download() == (after, 0)
        del g
    finally:
        tr.free()
        ctx_n.destroy()
        ctx_N.destroy()
