"""Out-of-domain values at Ext points and the DEEP codeword under Ext challenges (include/toyni_hip.h 3h) on the device:
  1. embedding: with z, weights, values and points embedded from the base field, coordinate 0 is the base call's word, 1..3 are zero
  2. random term sets against tests/ext_model.py (Python integers, inverse by a^(p^4 - 2)); long tables through the staging ring
  3. toyni_poly_eval_ext_batch_device against the model, and an Ext polynomial held as four base columns
  4. the pipeline property: the combination of true out-of-domain values has degree < n - 1, folds to a constant under Ext betas,
     and a folded layer's row commitment is the tree over Ext::to_bytes leaves
  5. guard bands around every buffer, two fillings, same outputs
  6. every refusal of the header, with d_out untouched; graph capture and replay of an inline-table call
Every comparison is exact."""
import numpy as np
import pytest

import ext_model as em
import oracle
from guarded import DevMem, Guarded

pytestmark = pytest.mark.gpu

P = em.P
E_NULL, E_RANGE = 10002, 10006
SENTINEL_WORD = 0xA5A5A5A5


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


class Dev:
    """Plain device buffers of u32 words (16-byte aligned base + a byte offset), freed together."""

    def __init__(self, ta):
        self.mem = DevMem(ta)
        self.ptrs = []

    def alloc(self, words, offset=0):
        base = self.mem.malloc(4 * words + 16 + offset)
        self.ptrs.append(base)
        return base + offset

    def up(self, arr, offset=0):
        a = np.ascontiguousarray(arr, dtype=np.uint32)
        p = self.alloc(max(a.size, 1), offset)
        if a.size:
            self.mem.h2d(p, a.ctypes.data, a.nbytes)
        return p

    def down(self, ptr, words):
        out = np.empty(words, dtype=np.uint32)
        self.mem.sync()
        if words:
            self.mem.d2h(out.ctypes.data, ptr, out.nbytes)
        return out

    def fill(self, ptr, words):
        self.mem.memset(ptr, 0xA5, 4 * words)

    def free(self):
        self.mem.sync()
        for p in self.ptrs:
            self.mem.free(p)
        self.ptrs = []


@pytest.fixture()
def dev(ta):
    d = Dev(ta)
    yield d
    d.free()


def rand_field(rng, *shape):
    return rng.integers(0, P, shape, dtype=np.uint64)


def rand_ext(rng):
    return tuple(int(v) for v in rng.integers(0, P, 4))


def combine_ext(ta, ctx, d_m, width, cs, log_b, shift, z, terms, d_out, accumulate=False, stream=0):
    """terms: (column, rotation, alpha4, value4)"""
    t = ta.prover.deep_ext_terms(*zip(*terms)) if terms else ta.prover.deep_ext_terms([], [], [], [])
    ta.prover.deep_combine_ext_device(ctx, d_m, width, cs, log_b, shift, z, t, d_out, accumulate=accumulate, stream=stream)


def ext_term_set(rng, width, nterms, rows):
    edge = [0, 1, P - 1]
    terms = []
    for t in range(nterms):
        alpha, value = list(rand_ext(rng)), list(rand_ext(rng))
        alpha[t % 4], value[(t + 1) % 4] = edge[t % 3], edge[(t + 1) % 3]
        terms.append((int(rng.integers(0, width)), (rows - 1) if t % 3 == 2 else int(rng.integers(0, rows)), tuple(alpha), tuple(value)))
    return terms


def padded_words(m, cs):
    width, N = m.shape
    words = np.full(width * cs, 0xFFFFFFF0, dtype=np.uint32)                   # the tails: a sentinel >= p that must never be read
    for c in range(width):
        words[c * cs:c * cs + N] = m[c]
    return words[: (width - 1) * cs + N]


# ---- 1. embedding ----
@pytest.mark.parametrize("log_n", [1, 3, 12])
def test_embedded_base_challenges_reproduce_the_base_calls(ta, dev, log_n):
    N, width, log_b = 1 << log_n, 3, min(1, log_n)
    rows = N >> log_b
    rng = np.random.default_rng(300 + log_n)
    m = rand_field(rng, width, N)
    z = int(rng.integers(1, P))
    base_terms = [(int(rng.integers(0, width)), int(rng.integers(0, rows)), int(rng.integers(0, P)), int(rng.integers(0, P))) for _ in range(7)]
    ctx = ta.NttContext(N)
    try:
        d_m, d_base, d_ext = dev.up(m.reshape(-1)), dev.alloc(N), dev.alloc(4 * N)
        ta.prover.deep_combine_device(ctx, d_m, width, N, log_b, 7, z, ta.prover.deep_terms(*zip(*base_terms)), d_base)
        combine_ext(ta, ctx, d_m, width, N, log_b, 7, em.embed(z), [(c, r, em.embed(a), em.embed(v)) for c, r, a, v in base_terms], d_ext)
        base, ext = dev.down(d_base, N), dev.down(d_ext, 4 * N).reshape(N, 4)
        assert (ext[:, 0] == base).all() and not ext[:, 1:].any()
        # the evaluation: the matrix's columns read as coefficient vectors
        pts = [int(v) for v in rng.integers(0, P, 3)]
        d_pb, d_pe = dev.alloc(width * 3), dev.alloc(width * 3 * 4)
        ta.prover.poly_eval_batch_device(ctx, d_m, N, N, width, pts, d_pb)
        ta.prover.poly_eval_ext_batch_device(ctx, d_m, N, N, width, [em.embed(v) for v in pts], d_pe)
        pb, pe = dev.down(d_pb, width * 3), dev.down(d_pe, width * 3 * 4).reshape(width * 3, 4)
        assert (pe[:, 0] == pb).all() and not pe[:, 1:].any()
    finally:
        ctx.destroy()


# ---- 2. the model ----
@pytest.mark.parametrize("log_n,log_b", [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (3, 3), (6, 0), (6, 1), (6, 3), (12, 0), (12, 1), (12, 3)])
def test_random_term_sets_match_the_integer_model(ta, dev, log_n, log_b):
    N, B = 1 << log_n, 1 << log_b
    rows = N >> log_b
    rng = np.random.default_rng(9000 + 16 * log_n + log_b)
    shift, cs = 7, N + 20
    xs = em.coset_points(N, shift)
    ctx = ta.NttContext(N)
    try:
        for off in (0, 4):
            width, width2 = 1 + (log_n + off) % 5, 2
            m, m2 = rand_field(rng, width, N), rand_field(rng, width2, N)
            m[0, : min(N, 3)] = [0, 1, P - 1][: min(N, 3)]
            terms = ext_term_set(rng, width, 5 + (log_n + log_b + off // 4) % 8, rows)      # 5..12 terms: every tail of the groups of four
            terms.append(terms[0][:2] + (rand_ext(rng), rand_ext(rng)))                      # a repeated (column, rotation)
            terms2 = ext_term_set(rng, width2, 3, rows)
            hit = (N // 2) | (3 if N >= 4 else 0)                                            # the last point of a group
            for z, at in ((rand_ext(rng), None), ((int(rng.integers(0, P)), 0, int(rng.integers(1, P)), 0), None), (em.embed(xs[hit]), hit)):
                d_m, d_m2, d_out = dev.up(padded_words(m, cs), off), dev.up(padded_words(m2, cs), 4 - off), dev.alloc(4 * N)
                dev.fill(d_out, 4 * N)
                combine_ext(ta, ctx, d_m, width, cs, log_b, shift, z, terms, d_out)
                got = dev.down(d_out, 4 * N).reshape(N, 4)
                want = em.deep_ext_model(m, terms, B, shift, z)
                bad = np.flatnonzero((got != want).any(axis=1))
                assert bad.size == 0, (log_n, log_b, off, z, bad[:8])
                if at is not None:
                    assert not got[at].any() and (N == 1 or got[np.arange(N) != at].any())
                # a second matrix accumulated on top
                combine_ext(ta, ctx, d_m2, width2, cs, log_b, shift, z, terms2, d_out, accumulate=True)
                want2 = (want.astype(np.uint64) + em.deep_ext_model(m2, terms2, B, shift, z)) % np.uint64(P)
                assert (dev.down(d_out, 4 * N).reshape(N, 4) == want2).all(), (log_n, log_b, off, z)
                dev.free()
    finally:
        ctx.destroy()


def test_long_tables_go_through_the_ring_and_do_not_overwrite_each_other(ta, dev):
    """Tables of more than 64 terms go through the context's pinned staging ring: 65 and 200 terms, 24 calls enqueued on one stream
    without a wait in between (the ring wraps on the way); every output must be the one of its own table."""
    N, width, log_b = 64, 5, 1
    rng = np.random.default_rng(199)
    m = rand_field(rng, width, N)
    ctx = ta.NttContext(N)
    try:
        d_m = dev.up(m.reshape(-1))
        calls = []
        for k in range(24):
            terms = ext_term_set(rng, width, 65 if k % 2 else 200, N >> log_b)
            z = rand_ext(rng)
            d_out = dev.alloc(4 * N)
            combine_ext(ta, ctx, d_m, width, N, log_b, 7, z, terms, d_out)
            calls.append((terms, z, d_out))
        for k, (terms, z, d_out) in enumerate(calls):
            assert (dev.down(d_out, 4 * N).reshape(N, 4) == em.deep_ext_model(m, terms, 1 << log_b, 7, z)).all(), k
    finally:
        ctx.destroy()


def test_no_terms_writes_zeros_or_leaves_the_output_alone(ta, dev):
    N = 64
    ctx = ta.NttContext(N)
    try:
        d_m, d_out = dev.up(np.arange(N)), dev.alloc(4 * N)
        dev.fill(d_out, 4 * N)
        combine_ext(ta, ctx, d_m, 1, N, 1, 7, (5, 1, 0, 0), [], d_out, accumulate=True)
        assert (dev.down(d_out, 4 * N) == SENTINEL_WORD).all()
        combine_ext(ta, ctx, d_m, 1, N, 1, 7, (5, 1, 0, 0), [], d_out)
        assert (dev.down(d_out, 4 * N) == 0).all()
    finally:
        ctx.destroy()


# ---- 3. evaluation at Ext points ----
@pytest.mark.parametrize("k,ncoeffs", list(enumerate([0, 1, 15, 16, 17, 4095, 4096, 4097])))
def test_ext_evaluation_matches_the_model(ta, dev, k, ncoeffs):
    ctx = ta.NttContext(16)
    lib = ta._lib.lib
    try:
        for batch, npoints in ((1, 1 + k % 4), (3, 1 + (k + 2) % 4)):
            rng = np.random.default_rng(50 * ncoeffs + batch)
            stride = ncoeffs + (5 if batch > 1 else 0)
            coeffs = rand_field(rng, batch, ncoeffs)
            words = np.full(batch * stride + 1, 0xFFFFFFF0, dtype=np.uint32)
            for b in range(batch):
                words[b * stride:b * stride + ncoeffs] = coeffs[b]
            points = [(P - 1,) * 4, (0, 1, 0, 0), rand_ext(rng), em.embed(int(rng.integers(0, P)))][:npoints]
            d_c, d_out = dev.up(words[: (batch - 1) * stride + ncoeffs], 4), dev.alloc(batch * npoints * 4, 8)
            dev.fill(d_out, batch * npoints * 4)
            ta.prover.poly_eval_ext_batch_device(ctx, d_c, ncoeffs, stride, batch, points, d_out)
            got = dev.down(d_out, batch * npoints * 4).reshape(batch, npoints, 4)
            assert (got == em.poly_eval_ext_batch_model(coeffs, points)).all(), (ncoeffs, batch, npoints)
            dev.free()
        assert lib.toyni_poly_eval_ext_batch_device(ctx.handle, 0x1000, 4, 4, 0, np.zeros(4, np.uint32).ctypes.data, 1, 0x2000, None) == 0   # batch 0
    finally:
        ctx.destroy()


def test_four_base_columns_are_an_ext_polynomial(ta, dev):
    """The header's note: an Ext-valued polynomial q held as four base columns q_0..q_3 is evaluated column by column and combined on
    the host, q(z) = sum_j X^j q_j(z).  At an Ext point this is checked against Horner with Ext coefficients; at a base point the four
    values are four base evaluations (toyni_poly_eval_batch_device)."""
    ncoeffs = 300
    rng = np.random.default_rng(4)
    q = rand_field(rng, 4, ncoeffs)
    z, zb = rand_ext(rng), int(rng.integers(0, P))
    ctx = ta.NttContext(16)
    try:
        d_q, d_out, d_base = dev.up(q.reshape(-1)), dev.alloc(4 * 2 * 4), dev.alloc(4)
        ta.prover.poly_eval_ext_batch_device(ctx, d_q, ncoeffs, ncoeffs, 4, [z, em.embed(zb)], d_out)
        ta.prover.poly_eval_batch_device(ctx, d_q, ncoeffs, ncoeffs, 4, [zb], d_base)
        got, base = dev.down(d_out, 32).reshape(4, 2, 4), dev.down(d_base, 4)
        assert (got[:, 1, 0] == base).all() and not got[:, 1, 1:].any()
        want = em.ZERO
        for i in reversed(range(ncoeffs)):
            want = em.add(em.mul(want, z), tuple(int(q[j, i]) for j in range(4)))
        combined, xj = em.ZERO, em.ONE
        for j in range(4):
            combined = em.add(combined, em.mul(xj, tuple(int(v) for v in got[j, 0])))
            xj = em.mul(xj, (0, 1, 0, 0))
        assert combined == want
    finally:
        ctx.destroy()


# ---- 4. the pipeline ----
@pytest.mark.parametrize("log_rows,log_b", [(6, 3), (12, 5)])
def test_pipeline_from_columns_to_folded_ext_layers_stays_on_the_device(ta, dev, log_rows, log_b):
    lib = ta._lib.lib
    w, n = 3, 1 << log_rows
    N, B = n << log_b, 1 << log_b
    rng = np.random.default_rng(20261019 + log_rows)
    shift = 7
    cols = rand_field(rng, w, n)
    small, big = ta.NttContext(n), ta.NttContext(N)
    try:
        d_vals = dev.up(cols.reshape(-1))
        d_coef, d_lde, d_ood = dev.alloc(w * n), dev.alloc(w * N), dev.alloc(w * 2 * 4)
        small.run_device(d_vals, d_coef, w, True)                                  # batched inverse transform: coefficients
        big.lde_device(d_coef, d_lde, w, log_b, shift)                              # batched LDE, column-major, col_stride = N
        d_levels = dev.alloc(8 * int(lib.toyni_merkle_total_digests(N)))
        ta.merkle_commit_rows_device(d_lde, N, w, ta.ROWS_COLUMN_MAJOR, N, 0, d_levels)
        g = pow(em.GEN_2_27, (1 << 27) // n, P)
        z = (int(rng.integers(0, P)), int(rng.integers(1, P)), int(rng.integers(0, P)), int(rng.integers(1, P)))
        gz = tuple(v * g % P for v in z)
        ta.prover.poly_eval_ext_batch_device(small, d_coef, n, n, w, [z, gz], d_ood)
        ood = dev.down(d_ood, w * 2 * 4).reshape(w, 2, 4)
        terms = [(c, r, rand_ext(rng), tuple(int(v) for v in ood[c, r])) for c in range(w) for r in range(2)]
        d_deep, d_poly = dev.alloc(4 * N), dev.alloc(4 * N)
        combine_ext(ta, big, d_lde, w, N, log_b, shift, z, terms, d_deep)
        dev.mem.sync()
        lib.toyni_memcpy_d2d_async(d_poly, d_deep, 16 * N, None)
        big.run_device_ext(d_poly, True, shift=shift)                               # inverse coset transform, in place
        coeffs = dev.down(d_poly, 4 * N).reshape(N, 4)
        assert not coeffs[n - 1:].any(), "the combination of true values has degree < n - 1 in every coordinate"
        assert coeffs[n - 2].any()
        # one claimed value off by one: the division leaves a remainder, the degree bound breaks
        c0, r0, a0, v0 = terms[3]
        wrong = terms[:3] + [(c0, r0, a0, ((v0[0] + 1) % P,) + v0[1:])] + terms[4:]
        d_bad = dev.alloc(4 * N)
        combine_ext(ta, big, d_lde, w, N, log_b, shift, z, wrong, d_bad)
        big.run_device_ext(d_bad, True, shift=shift)
        assert dev.down(d_bad, 4 * N).reshape(N, 4)[n - 1:].any()
        # Ext folds down to B values: a codeword of degree < n - 1 folds to a constant layer; the first folded layer's row commitment
        # (row-major, width 4) is the tree over the host's Ext::to_bytes leaves
        layers = [d_deep] + [dev.alloc(4 * (N >> k)) for k in range(1, log_rows + 1)]
        x0 = shift
        for k in range(log_rows):
            ta.fri_fold_ext_device(big, layers[k], layers[k + 1], N >> k, rand_ext(rng), x0)
            x0 = x0 * x0 % P
        last = dev.down(layers[-1], 4 * B).reshape(B, 4)
        assert (last == last[0]).all() and last[0].any(), last
        m1 = N // 2
        total = int(lib.toyni_merkle_total_digests(m1))
        d_tree = dev.alloc(8 * total)
        ta.merkle_commit_rows_device(layers[1], m1, 4, ta.ROWS_ROW_MAJOR, 0, 0, d_tree)
        root = dev.down(d_tree, 8 * total)[-8:].tobytes()
        layer1 = dev.down(layers[1], 4 * m1).reshape(m1, 4).astype("<u8")
        assert root == oracle.merkle_levels([row.tobytes() for row in layer1])[-1][0].tobytes()
    finally:
        small.destroy()
        big.destroy()


# ---- 5. guard bands ----
@pytest.mark.parametrize("log_n,width,off", [(1, 3, 8), (3, 2, 4), (6, 5, 12)])
def test_deep_combine_ext_between_guard_bands(ta, log_n, width, off):
    N = 1 << log_n
    cs = N + 20
    rng = np.random.default_rng(155 + log_n)
    m = rand_field(rng, width, N)
    terms = ext_term_set(rng, width, 7, N)
    z = rand_ext(rng)
    ctx = ta.NttContext(N)
    results = []
    try:
        for pattern in ("sentinel", "random"):
            slack = np.full(width * cs, 0xA5A5A5A5, dtype=np.uint32) if pattern == "sentinel" else rand_field(rng, width * cs).astype(np.uint32)
            for c in range(width):
                slack[c * cs:c * cs + N] = m[c]
            words = slack[: (width - 1) * cs + N]
            dm, do = Guarded(ta, words.nbytes, offset=off, seed=1), Guarded(ta, 16 * N, offset=0, seed=2)
            try:
                dm.refill(pattern)
                dm.upload(words)
                combine_ext(ta, ctx, dm.ptr, width, cs, 0, 7, z, terms, do.ptr)
                dm.mem.sync()
                dm.check("matrix"), do.check("d_out")
                assert (dm.download() == words).all(), "the matrix was changed"
                results.append(do.download())
            finally:
                dm.free(check=False), do.free(check=False)
        assert (results[0] == results[1]).all() and (results[0].reshape(N, 4) == em.deep_ext_model(m, terms, 1, 7, z)).all()
    finally:
        ctx.destroy()


@pytest.mark.parametrize("ncoeffs,batch,npoints,off", [(17, 3, 2, 4), (4097, 2, 4, 12), (100, 1, 1, 8)])
def test_poly_eval_ext_batch_between_guard_bands(ta, ncoeffs, batch, npoints, off):
    rng = np.random.default_rng(ncoeffs + 1)
    stride = ncoeffs + 7
    coeffs = rand_field(rng, batch, ncoeffs)
    points = [rand_ext(rng) for _ in range(npoints)]
    ctx = ta.NttContext(8)
    results = []
    try:
        for pattern in ("sentinel", "random"):
            slack = np.full(batch * stride, 0xA5A5A5A5, dtype=np.uint32) if pattern == "sentinel" else rand_field(rng, batch * stride).astype(np.uint32)
            for b in range(batch):
                slack[b * stride:b * stride + ncoeffs] = coeffs[b]
            words = slack[: (batch - 1) * stride + ncoeffs]
            dc, do = Guarded(ta, words.nbytes, offset=off, seed=3), Guarded(ta, 16 * batch * npoints, offset=(off + 4) % 16, seed=4)
            try:
                dc.refill(pattern)
                dc.upload(words)
                ta.prover.poly_eval_ext_batch_device(ctx, dc.ptr, ncoeffs, stride, batch, points, do.ptr)
                dc.mem.sync()
                dc.check("coefficients"), do.check("d_out")
                assert (dc.download() == words).all()
                results.append(do.download())
            finally:
                dc.free(check=False), do.free(check=False)
        assert (results[0] == results[1]).all()
        assert (results[0].reshape(batch, npoints, 4) == em.poly_eval_ext_batch_model(coeffs, points)).all()
    finally:
        ctx.destroy()


# ---- 6. refusals, graph capture ----
def test_every_refusal_leaves_the_output_untouched(ta, dev):
    lib = ta._lib.lib
    N, width = 64, 3
    ctx = ta.NttContext(N)
    try:
        d_m, d_out = dev.up(np.arange(width * N) % P), dev.alloc(4 * N)
        dev.fill(d_out, 4 * N)
        U4 = lambda v: np.array(v, dtype=np.uint32)
        good_z = U4([9, 1, 2, 3])
        good = ta.prover.deep_ext_terms([0, 2], [0, 3], [[1, 2, 3, 4]] * 2, [[5, 6, 7, 8]] * 2)

        def deep(m=d_m, w=width, cs=N, lb=2, shift=7, z=good_z, terms=good, nterms=2, acc=0, out=d_out, handle=ctx.handle):
            return lib.toyni_deep_combine_ext_device(handle, m, w, cs, lb, shift, z.ctypes.data if z is not None else None, terms, nterms, acc, out, None)

        one = lambda c, r, a, v: ta.prover.deep_ext_terms([c], [r], [a], [v])
        unit = [1, 0, 0, 0]
        assert deep(handle=None) == E_NULL and deep(m=None) == E_NULL and deep(out=None) == E_NULL and deep(terms=None) == E_NULL
        assert deep(z=None) == E_NULL
        cases = [deep(shift=0), deep(shift=P), deep(lb=7), deep(cs=N - 1), deep(w=0), deep(w=65537),
                 deep(terms=one(3, 0, unit, unit), nterms=1), deep(terms=one(0, 16, unit, unit), nterms=1), deep(m=d_m + 2),
                 deep(out=d_out + 4), deep(out=d_out + 8), deep(out=d_out + 1)]                    # d_out: 16-byte aligned
        for k in range(4):                                                                        # a coordinate >= p, one at a time
            bad = [1, 1, 1, 1]
            bad[k] = P
            cases += [deep(z=U4(bad)), deep(terms=one(0, 0, bad, unit), nterms=1), deep(terms=one(0, 0, unit, bad), nterms=1)]
        assert all(rc == E_RANGE for rc in cases), cases
        big = (ta.prover.DeepExtTerm * ((1 << 20) + 1))()
        assert deep(terms=big, nterms=(1 << 20) + 1) == E_RANGE
        assert deep(terms=one(0, 15, unit, unit), nterms=1, acc=1, out=dev.alloc(4 * N)) == 0     # the largest rotation is fine
        pts = U4([1, 2, 3, 4, 5, 6, 7, 8] + [0] * 12)

        def poly(c=d_m, nc=8, stride=8, batch=2, points=pts.ctypes.data, npts=2, out=d_out, handle=ctx.handle):
            return lib.toyni_poly_eval_ext_batch_device(handle, c, nc, stride, batch, points, npts, out, None)

        assert poly(handle=None) == E_NULL and poly(c=None) == E_NULL and poly(points=None) == E_NULL and poly(out=None) == E_NULL
        cases = [poly(npts=0), poly(npts=5), poly(stride=7), poly(batch=1 << 32, stride=8), poly(c=d_m + 2), poly(out=d_out + 2)]
        for k in range(8):                                                                        # a coordinate of either point >= p
            bad = U4([1, 2, 3, 4, 5, 6, 7, 8])
            bad[k] = P
            cases.append(poly(points=bad.ctypes.data))
        assert all(rc == E_RANGE for rc in cases), cases
        assert poly(stride=0, batch=1, out=dev.alloc(8)) == 0                                     # one column: the stride is not used
        assert (dev.down(d_out, 4 * N) == SENTINEL_WORD).all()
    finally:
        ctx.destroy()


def test_an_inline_table_call_can_be_captured_and_replayed(ta):
    import torch
    tdev = torch.device("cuda", 0)
    N, width, log_b = 1 << 10, 4, 2
    rng = np.random.default_rng(78)
    terms = ext_term_set(rng, width, 64, N >> log_b)                            # the longest table that rides in the arguments
    z = rand_ext(rng)
    ctx = ta.NttContext(N)
    try:
        m = torch.zeros(width * N, dtype=torch.int32, device=tdev)
        out = torch.empty(4 * N, dtype=torch.int32, device=tdev)
        s = torch.cuda.Stream(device=tdev)
        call = lambda: combine_ext(ta, ctx, m.data_ptr(), width, N, log_b, 7, z, terms, out.data_ptr(), stream=s.cuda_stream)
        call()                                                                  # eager first: the kernel's code is loaded from here on
        ctx.synchronize(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):                                     # one kernel node
            call()
        for rep in range(2):
            h_m = rand_field(rng, width, N)
            m.copy_(torch.from_numpy(h_m.astype(np.uint32).view(np.int32).reshape(-1)))
            out.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32).reshape(N, 4)
            assert (got == em.deep_ext_model(h_m, terms, 1 << log_b, 7, z)).all(), rep
        del g
    finally:
        ctx.destroy()
