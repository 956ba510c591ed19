"""Batched out-of-domain evaluation and the multi-column DEEP combination (include/toyni_hip.h 3e) on the device:
  1. the Fibonacci term set equals toyni_fib_deep_device and oracle.fib_deep word for word (one call, and trace + quotient as two calls)
  2. general term sets against a vectorised numpy model that imports nothing from the library
  3. toyni_poly_eval_batch_device equals oracle.poly_eval and toyni_poly_eval_device per column
  4. the pipeline property: the combination of true out-of-domain values is a polynomial of degree < n - 1, and folds to a constant
  5. guard bands around every buffer, two fillings, same outputs
  6. every refusal of the header, with d_out untouched"""
import ctypes

import numpy as np
import pytest

import oracle
from air_model import GEN_2_27, P, coset_points, deep_model
from guarded import DevMem, Guarded

pytestmark = pytest.mark.gpu

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


# the independent model (numpy only) is deep_model of tests/air_model.py, shared with the oracle-only prover of the two-column proof
def rand_field(rng, *shape):
    return rng.integers(0, P, shape, dtype=np.uint64)


def combine(ta, ctx, d_m, width, cs, log_b, shift, z, terms, d_out, accumulate=False):
    t = ta.prover.deep_terms(*zip(*terms)) if terms else ta.prover.deep_terms([], [], [], [])
    ta.prover.deep_combine_device(ctx, d_m, width, cs, log_b, shift, z, t, d_out, accumulate=accumulate)


# ---- 1. Fibonacci anchor ----
@pytest.mark.parametrize("log_n", [1, 2, 3, 6, 12, 16, 21])
def test_fibonacci_terms_equal_fib_deep_and_the_oracle(ta, dev, log_n):
    N = 1 << log_n
    ctx = ta.NttContext(N)
    try:
        for log_b in (0, 1, 3, 5):
            if log_b >= log_n:                                     # a trace of at least two rows
                continue
            rows = N >> log_b                                      # rotation 2 of a two-row trace is its row 0
            rng = np.random.default_rng(100 * log_n + log_b)
            tq = rand_field(rng, 2, N)
            shift, z = 7, int(rng.integers(1, P))
            ood = [int(v) for v in rand_field(rng, 4)]
            d_m, d_out, d_ref, d_two = dev.up(tq.reshape(-1)), dev.alloc(N), dev.alloc(N), dev.alloc(N)
            terms = [(0, 0, 1, ood[0]), (0, 1, 1, ood[1]), (0, 2 % rows, 1, ood[2]), (1, 0, 1, ood[3])]
            combine(ta, ctx, d_m, 2, N, log_b, shift, z, terms, d_out)
            ta.prover.fib_deep_device(ctx, d_m, d_m + 4 * N, d_ref, log_b, shift, z, ood)
            combine(ta, ctx, d_m, 1, N, log_b, shift, z, terms[:3], d_two)                       # trace matrix first,
            combine(ta, ctx, d_m + 4 * N, 1, N, log_b, shift, z, [(0, 0, 1, ood[3])], d_two, accumulate=True)   # then the quotient's
            got, ref, two = dev.down(d_out, N), dev.down(d_ref, N), dev.down(d_two, N)
            want = oracle.fib_deep(tq[0], tq[1], N >> log_b, shift, z, *ood).astype(np.uint32)
            assert (got == ref).all() and (got == want).all() and (two == want).all(), (log_n, log_b)
            dev.free()
    finally:
        ctx.destroy()


# ---- 2. general parity ----
def term_set(rng, width, rots_per_col, rows):
    terms = []
    for c in range(width):
        for r in range(rots_per_col):
            terms.append((c, r % rows, int(rng.integers(0, P)), int(rng.integers(0, P))))
    return terms


@pytest.mark.parametrize("log_n,log_b,width,rots,off", [
    (3, 0, 1, 1, 0), (3, 1, 2, 2, 4), (4, 1, 3, 3, 8), (6, 2, 8, 4, 12), (10, 3, 33, 3, 0), (12, 5, 64, 3, 4), (12, 1, 8, 2, 8),
    (16, 5, 8, 3, 12), (18, 5, 3, 4, 0), (18, 3, 2, 1, 4), (2, 0, 3, 2, 0), (0, 0, 2, 1, 4),
])
def test_general_term_sets_match_the_numpy_model(ta, dev, log_n, log_b, width, rots, off):
    N, B = 1 << log_n, 1 << log_b
    rows = N >> log_b
    rng = np.random.default_rng(7000 + 10 * log_n + width)
    cs = N + 20
    m = rand_field(rng, width, N)
    m[0, : min(N, 3)] = [0, 1, P - 1][: min(N, 3)]
    words = np.full(width * cs, 0xFFFFFFF0, dtype=np.uint32)                   # the tails: a sentinel >= p that must never be read
    for c in range(width):
        words[c * cs:c * cs + N] = m[c]
    words = words[: (width - 1) * cs + N]
    terms = term_set(rng, width, min(rots, rows), rows)
    terms.append(terms[0][:2] + (int(rng.integers(1, P)), 5))                  # a repeated (column, rotation)
    terms[len(terms) // 2] = terms[len(terms) // 2][:2] + (0, 77)              # weight 0
    rng.shuffle(terms)
    terms = [tuple(int(v) for v in t) for t in terms]
    ctx = ta.NttContext(N)
    try:
        shift = 7
        xs = coset_points(N, shift)
        for z, hit in ((int(rng.integers(1, P)), None), (int(xs[N - 1]), N - 1), (int(xs[(N // 2) & ~7]), (N // 2) & ~7)):
            d_m, d_out = dev.up(words, off), dev.alloc(N, (off + 4) % 16)
            combine(ta, ctx, d_m, width, cs, log_b, shift, z, terms, d_out)
            got = dev.down(d_out, N)
            want = deep_model(m, terms, B, shift, z)
            if hit is not None:
                assert got[hit] == 0 and want[hit] == 0
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (log_n, log_b, width, z, bad[:8])
            # accumulate on top of a known vector
            prev = rand_field(rng, N).astype(np.uint32)
            dev.mem.h2d(d_out, prev.ctypes.data, prev.nbytes)
            combine(ta, ctx, d_m, width, cs, log_b, shift, z, terms, d_out, accumulate=True)
            assert (dev.down(d_out, N) == ((prev.astype(np.uint64) + want) % P).astype(np.uint32)).all()
            dev.free()
    finally:
        ctx.destroy()


def test_long_tables_in_flight_do_not_overwrite_each_other(ta, dev):
    """Tables of more than 64 terms go through the context's pinned staging ring.  45 calls of 100 terms each are enqueued without a
    wait in between (the ring wraps once on the way); every output must be the one of its own table."""
    N, width, log_b = 64, 5, 1
    rng = np.random.default_rng(99)
    m = rand_field(rng, width, N)
    ctx = ta.NttContext(N)
    try:
        d_m = dev.up(m.reshape(-1))
        tables, outs = [], []
        for k in range(45):
            terms = [(int(rng.integers(0, width)), int(rng.integers(0, N >> log_b)), int(rng.integers(0, P)), int(rng.integers(0, P))) for _ in range(100)]
            d_out = dev.alloc(N)
            combine(ta, ctx, d_m, width, N, log_b, 7, 1000 + k, terms, d_out)
            tables.append(terms), outs.append(d_out)
        for k, (terms, d_out) in enumerate(zip(tables, outs)):
            assert (dev.down(d_out, N) == deep_model(m, terms, 1 << log_b, 7, 1000 + k)).all(), k
    finally:
        ctx.destroy()


def test_no_terms_writes_zeros_or_leaves_the_output_alone(ta, dev):
    N = 64
    ctx = ta.NttContext(N)
    try:
        d_m, d_out = dev.up(np.arange(N)), dev.alloc(N)
        dev.fill(d_out, N)
        combine(ta, ctx, d_m, 1, N, 1, 7, 5, [], d_out, accumulate=True)
        assert (dev.down(d_out, N) == SENTINEL_WORD).all()
        combine(ta, ctx, d_m, 1, N, 1, 7, 5, [], d_out)
        assert (dev.down(d_out, N) == 0).all()
    finally:
        ctx.destroy()


# ---- 3. batched polynomial evaluation ----
@pytest.mark.parametrize("ncoeffs", [0, 1, 15, 16, 17, 4095, 4096, 4097, (1 << 16) + 3])
def test_batched_poly_eval_equals_the_oracle_and_the_single_call(ta, dev, ncoeffs):
    ctx = ta.NttContext(16)
    lib = ta._lib.lib
    try:
        for batch, npoints in ((1, 1), (2, 2), (7, 3), (64, 4)):
            rng = np.random.default_rng(ncoeffs + batch)
            stride = ncoeffs + (5 if batch > 1 else 0)
            coeffs = rand_field(rng, batch, ncoeffs)
            words = np.full(batch * stride + 1, 0xFFFFFFF0, dtype=np.uint32)
            for b in range(batch):
                words[b * stride:b * stride + ncoeffs] = coeffs[b]
            points = [P - 1, 1, int(rng.integers(0, P)), 0][:npoints]
            d_c, d_out, d_one = dev.up(words[: (batch - 1) * stride + ncoeffs], 4), dev.alloc(batch * npoints, 8), dev.alloc(batch * npoints)
            dev.fill(d_out, batch * npoints)
            ta.prover.poly_eval_batch_device(ctx, d_c, ncoeffs, stride, batch, points, d_out)
            for b in range(batch):
                ta.prover.poly_eval_device(ctx, d_c + 4 * b * stride, ncoeffs, points, d_one + 4 * b * npoints)
            got, one = dev.down(d_out, batch * npoints), dev.down(d_one, batch * npoints)
            assert (got == one).all(), (ncoeffs, batch)
            for b in sorted({0, batch // 2, batch - 1}):
                for p, pt in enumerate(points):
                    assert got[b * npoints + p] == oracle.poly_eval(coeffs[b], pt), (ncoeffs, batch, b, p)
            dev.free()
        assert lib.toyni_poly_eval_batch_device(ctx.handle, 0x1000, 4, 4, 0, np.zeros(1, np.uint32).ctypes.data, 1, 0x2000, None) == 0   # batch 0
    finally:
        ctx.destroy()


# ---- 4. the pipeline ----
def test_pipeline_from_columns_to_openings_stays_on_the_device(ta, dev):
    lib = ta._lib.lib
    w, n, log_b = 8, 1 << 10, 3
    N, B = n << log_b, 1 << log_b
    rng = np.random.default_rng(424242)
    shift = 7
    cols = rand_field(rng, w, n)
    small, big = ta.NttContext(n), ta.NttContext(N)
    try:
        d_vals = dev.up(cols.reshape(-1))
        d_coef, d_lde, d_ood = dev.alloc(w * n), dev.alloc(w * N), dev.alloc(3 * w)
        small.run_device(d_vals, d_coef, w, True)                                  # batched inverse transform: coefficients
        big.lde_device(d_coef, d_lde, w, log_b, shift)                              # batched LDE, column-major, col_stride = N
        total = int(lib.toyni_merkle_total_digests(N))
        d_levels = dev.alloc(8 * total)
        ta.merkle_commit_rows_device(d_lde, N, w, ta.ROWS_COLUMN_MAJOR, N, 0, d_levels)
        g = pow(GEN_2_27, (1 << 27) // n, P)
        z = int(rng.integers(2, P))
        points = [z, g * z % P, g * g % P * z % P]
        ta.prover.poly_eval_batch_device(small, d_coef, n, n, w, points, d_ood)
        ood = dev.down(d_ood, 3 * w).reshape(w, 3)
        alphas = rng.integers(1, P, (w, 3))
        terms = [(c, r, int(alphas[c, r]), int(ood[c, r])) for c in range(w) for r in range(3)]
        d_deep, d_poly = dev.alloc(N), dev.alloc(N)
        combine(ta, big, d_lde, w, N, log_b, shift, z, terms, d_deep)
        big.run_device(d_deep, d_poly, 1, True, shift=shift)                        # inverse coset transform
        coeffs = dev.down(d_poly, N)
        assert (coeffs[n - 1:] == 0).all(), "the combination of true values has degree < n - 1"
        # one claimed value off by one: the division leaves a remainder, the degree bound breaks
        c0, r0, a0, v0 = terms[5]
        wrong = terms[:5] + [(c0, r0, a0, (v0 + 1) % P)] + terms[6:]
        d_bad = dev.alloc(N)
        combine(ta, big, d_lde, w, N, log_b, shift, z, wrong, d_bad)
        big.run_device(d_bad, d_poly, 1, True, shift=shift)
        assert dev.down(d_poly, N)[n - 1:].any()
        # FRI commit phase down to 8 values: a codeword of degree < n - 1 at blow-up 8 folds to a constant layer
        final = 8
        layer_words = N - final
        d_layers = dev.alloc(layer_words)
        tree_digests = sum(int(lib.toyni_merkle_total_digests(N >> k)) for k in range(1, (N // final).bit_length()))
        d_trees = dev.alloc(8 * tree_digests)
        betas = iter(int(v) for v in rng.integers(1, P, 64))
        roots = ta.prover.fri_commit_phase_device(big, d_deep, N, shift, final, 0, lambda rnd, root, want: next(betas) if want else 0, d_layers, d_trees)
        assert len(roots) == (N // final).bit_length() - 1
        last = dev.down(d_layers + 4 * (layer_words - final), final)
        assert (last == last[0]).all(), last
        # the rows the combination read are the rows the commitment opens
        idx = np.array([0, N // 3, N - 1], dtype=np.uint32)
        rec = int(lib.toyni_merkle_open_rows_record_bytes(N, w))
        d_idx, d_rec = dev.up(idx), dev.alloc(rec * idx.size // 4 + 2)
        ta.merkle_open_rows_device(d_levels, N, d_lde, w, ta.ROWS_COLUMN_MAJOR, N, 0, d_idx, idx.size, d_rec)
        raw = dev.down(d_rec, rec * idx.size // 4).view(np.uint8).reshape(idx.size, rec)
        lde = dev.down(d_lde, w * N).reshape(w, N)
        depth = N.bit_length() - 1
        for k, i in enumerate(idx):
            row = raw[k, 32 * depth + 16:32 * depth + 16 + 8 * w].view(np.uint64)
            assert (row == lde[:, i]).all()
        # and that row enters the combination: recompute d at those three points from the opened rows of i, i + B, i + 2B
        deep = dev.down(d_deep, N)
        assert (deep[idx] == deep_model(lde.astype(np.uint64), terms, B, shift, z)[idx]).all()
    finally:
        small.destroy()
        big.destroy()


# ---- 5. guard bands ----
@pytest.mark.parametrize("log_n,width,off", [(3, 2, 4), (6, 5, 12), (12, 9, 0), (1, 3, 8)])
def test_deep_combine_between_guard_bands(ta, log_n, width, off):
    N = 1 << log_n
    cs = N + 20
    rng = np.random.default_rng(55 + log_n)
    m = rand_field(rng, width, N)
    rows = N
    terms = [tuple(int(v) for v in t) for t in term_set(rng, width, min(3, rows), rows)]
    ctx = ta.NttContext(N)
    results = []
    try:
        for pattern in ("sentinel", "random"):
            slack = np.full(width * cs, 0xA5A5A5A5, dtype=np.uint32) if pattern == "sentinel" else rand_field(rng, width * cs).astype(np.uint32)
            for c in range(width):
                slack[c * cs:c * cs + N] = m[c]
            words = slack[: (width - 1) * cs + N]
            dm, do = Guarded(ta, words.nbytes, offset=off, seed=1), Guarded(ta, 4 * N, offset=(off + 8) % 16, seed=2)
            try:
                dm.refill(pattern)
                dm.upload(words)
                combine(ta, ctx, dm.ptr, width, cs, 0, 7, 12345, terms, do.ptr)
                dm.mem.sync()
                dm.check("matrix"), do.check("d_out")
                assert (dm.download() == words).all(), "the matrix was changed"
                results.append(do.download())
            finally:
                dm.free(check=False), do.free(check=False)
        assert (results[0] == results[1]).all() and (results[0] == deep_model(m, terms, 1, 7, 12345)).all()
    finally:
        ctx.destroy()


@pytest.mark.parametrize("ncoeffs,batch,npoints,off", [(17, 3, 2, 4), (4097, 5, 4, 12), (100, 1, 1, 8)])
def test_poly_eval_batch_between_guard_bands(ta, ncoeffs, batch, npoints, off):
    rng = np.random.default_rng(ncoeffs)
    stride = ncoeffs + 7
    coeffs = rand_field(rng, batch, ncoeffs)
    points = [int(v) for v in rng.integers(0, P, npoints)]
    ctx = ta.NttContext(8)
    results = []
    try:
        for pattern in ("sentinel", "random"):
            slack = np.full(batch * stride, 0xA5A5A5A5, dtype=np.uint32) if pattern == "sentinel" else rand_field(rng, batch * stride).astype(np.uint32)
            for b in range(batch):
                slack[b * stride:b * stride + ncoeffs] = coeffs[b]
            words = slack[: (batch - 1) * stride + ncoeffs]
            dc, do = Guarded(ta, words.nbytes, offset=off, seed=3), Guarded(ta, 4 * batch * npoints, offset=(off + 4) % 16, seed=4)
            try:
                dc.refill(pattern)
                dc.upload(words)
                ta.prover.poly_eval_batch_device(ctx, dc.ptr, ncoeffs, stride, batch, points, do.ptr)
                dc.mem.sync()
                dc.check("coefficients"), do.check("d_out")
                assert (dc.download() == words).all()
                results.append(do.download())
            finally:
                dc.free(check=False), do.free(check=False)
        assert (results[0] == results[1]).all()
        for b in range(batch):
            for p, pt in enumerate(points):
                assert results[0][b * npoints + p] == oracle.poly_eval(coeffs[b], pt)
    finally:
        ctx.destroy()


# ---- 6. refusals ----
def test_every_refusal_leaves_the_output_untouched(ta, dev):
    lib = ta._lib.lib
    N, width = 64, 3
    ctx = ta.NttContext(N)
    try:
        d_m, d_out = dev.up(np.arange(width * N) % P), dev.alloc(N)
        dev.fill(d_out, N)
        T = ta.prover.DeepTerm
        good = (T * 2)(T(0, 0, 1, 2), T(2, 3, 4, 5))

        def deep(m=d_m, w=width, cs=N, lb=2, shift=7, z=9, terms=good, nterms=2, acc=0, out=d_out, handle=ctx.handle):
            return lib.toyni_deep_combine_device(handle, m, w, cs, lb, shift, z, terms, nterms, acc, out, None)

        one = lambda *f: (T * 1)(T(*f))
        assert deep(handle=None) == E_NULL and deep(m=None) == E_NULL and deep(out=None) == E_NULL and deep(terms=None) == E_NULL
        cases = [deep(z=P), deep(shift=0), deep(shift=P), deep(lb=7), deep(cs=N - 1), deep(w=0), deep(w=65537),
                 deep(terms=one(3, 0, 1, 1), nterms=1), deep(terms=one(0, 16, 1, 1), nterms=1), deep(terms=one(0, 0, P, 1), nterms=1),
                 deep(terms=one(0, 0, 1, P), nterms=1), deep(m=d_m + 2), deep(out=d_out + 1)]
        assert all(rc == E_RANGE for rc in cases), cases
        big = (T * ((1 << 20) + 1))()
        assert deep(terms=big, nterms=(1 << 20) + 1) == E_RANGE
        assert deep(terms=one(0, 15, 1, 1), nterms=1, acc=1, out=dev.alloc(N)) == 0      # the largest rotation is fine
        pts = np.array([1, 2, 3, 4, 5], dtype=np.uint32)

        def poly(c=d_m, nc=8, stride=8, batch=2, points=pts.ctypes.data, npts=2, out=d_out, handle=ctx.handle):
            return lib.toyni_poly_eval_batch_device(handle, c, nc, stride, batch, points, npts, out, None)

        assert poly(handle=None) == E_NULL and poly(c=None) == E_NULL and poly(points=None) == E_NULL and poly(out=None) == E_NULL
        bad_pt = np.array([1, P], dtype=np.uint32)
        cases = [poly(npts=0), poly(npts=5), poly(points=bad_pt.ctypes.data), poly(stride=7), poly(batch=1 << 32, stride=8), poly(c=d_m + 2), poly(out=d_out + 2)]
        assert all(rc == E_RANGE for rc in cases), cases
        assert poly(stride=0, batch=1, out=dev.alloc(4)) == 0                           # one column: the stride is not used
        assert (dev.down(d_out, N) == SENTINEL_WORD).all()
    finally:
        ctx.destroy()
