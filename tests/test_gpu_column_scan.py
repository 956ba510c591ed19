"""Accumulator columns on the device (include/toyni_hip.h 3g): toyni_column_scan_device and toyni_batch_inverse_device.
  1. parity without an inversion on the host: where no denominator is zero the output is the unique solution of a recurrence, checked
     vectorised in uint64 -- every n from 1 to 2 T + 1, 2^19 + T + 1, and 2^22 + 3 (step 2 loops in rounds); both ops, the three
     operand forms, batch 1 and 3 with padded and distinct strides, columns 0 / 4 / 8 / 12 bytes off alignment
  2. zero denominators and field edges against a Python-integer model, with the zero counts
  3. the inversion alone
  4. in place on either operand
  5. guard bands around every operand, the words between n and the stride included
  6. two stages of a proof composed: a permutation product and a LogUp sum built from a main trace, committed to as a second matrix,
     and the quotient of the constraints that tie them to the main trace is a polynomial of the degree it must have
  7. a call captured into a graph and replayed"""
import numpy as np
import pytest

from guarded import DevMem, Guarded
from harness.fib_prover import COSET_SHIFT

pytestmark = pytest.mark.gpu

P = 2013265921
SUM, PRODUCT = 0, 1
FORMS = {"num/den": (True, True), "1/den": (False, True), "num": (True, False)}
SENTINEL_WORD = 0xA5A5A5A5
PU = np.uint64(P)


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


@pytest.fixture(scope="module")
def T(ta):
    return ta.prover.column_scan_tile()


@pytest.fixture(scope="module")
def ctx(ta):
    c = ta.NttContext(64)                                  # n is not tied to the context's size
    yield c
    c.destroy()


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
        self.mem.h2d(p, a.ctypes.data, a.nbytes)
        return p

    def down(self, ptr, words):
        out = np.empty(words, dtype=np.uint32)
        self.mem.sync()
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


# one pool of nonzero residues, shared and never changed: every parity case reads slices of it
POOL_WORDS = 3 * ((1 << 22) + 64)
_pool = {}


def pool():
    if "v" not in _pool:
        v = np.random.default_rng(0x5CA9).integers(1, P, POOL_WORDS, dtype=np.uint64)
        v.setflags(write=False)
        _pool["v"] = v
    return _pool["v"]


def recurrence_holds(op, out, total, num, den, init):
    """out (n), total: does out[0] = init and out[i+1] (x) den[i] = ... hold at every i, the wrap-around step included?  uint64
    throughout: operands < 2^31, products < 2^62.  num / den None: ones."""
    o = out.astype(np.uint64)
    nxt = np.append(o[1:], np.uint64(total))
    one = np.uint64(1)
    d = den if den is not None else one
    u = num if num is not None else one
    if op == SUM:
        ok = ((nxt + PU - o) % PU) * d % PU == u % PU
    else:
        ok = nxt * d % PU == o * u % PU
    return bool(o[0] == init and (o < PU).all() and total < P and np.all(ok))


# ---- 1. parity ----
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("op", [SUM, PRODUCT])
def test_every_n_up_to_two_tiles_and_one_solves_the_recurrence(ta, ctx, dev, T, op, form):
    has_num, has_den = FORMS[form]
    top = 2 * T + 1
    ns = np.arange(1, top + 1, dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(ns)))                         # call n writes at word offs[n - 1]: every alignment occurs
    num_h, den_h = pool()[:top + 4], pool()[top + 4:2 * (top + 4)]
    d_num, d_den = dev.up(num_h), dev.up(den_h)
    d_out, d_tot = dev.alloc(int(offs[-1])), dev.alloc(2 * top)
    dev.fill(d_out, int(offs[-1])), dev.fill(d_tot, 2 * top)
    init = 5 + op
    for n in range(top, 0, -1):                                         # downwards: an overrun would land in words already written
        sh = n % 4                                                      # the operands start 0 / 4 / 8 / 12 bytes off alignment
        ta.prover.column_scan_device(ctx, d_num + 4 * sh if has_num else 0, d_den + 4 * ((sh + 1) % 4) if has_den else 0, d_out + 4 * int(offs[n - 1]),
                                     n, 1, op, [init], d_tot + 8 * (n - 1))
    out, tot = dev.down(d_out, int(offs[-1])).astype(np.uint64), dev.down(d_tot, 2 * top).astype(np.uint64).reshape(top, 2)
    assert (tot[:, 1] == 0).all() and (tot[:, 0] < PU).all() and (out < PU).all()
    seg = np.repeat(ns, ns)
    pos = np.arange(offs[-1]) - np.repeat(offs[:-1], ns)
    nxt = np.append(out[1:], np.uint64(0))
    nxt[offs[1:] - 1] = tot[:, 0]
    u = num_h[pos + seg % 4] if has_num else np.uint64(1)
    d = den_h[pos + (seg + 1) % 4] if has_den else np.uint64(1)
    ok = ((nxt + PU - out) % PU) * d % PU == u % PU if op == SUM else nxt * d % PU == out * u % PU
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, ("first failure at n, i =", int(seg[bad[0]]), int(pos[bad[0]]))
    assert (out[offs[:-1]] == init).all()


def run_batch(ta, ctx, dev, op, form, n, batch, strides, offsets, init):
    """One call on slices of the pool; -> (list of (out, total, zeros, num, den) per column)."""
    has_num, has_den = FORMS[form]
    ns, ds, os_ = strides
    words = [(batch - 1) * s + n for s in strides]
    num_h, den_h = pool()[:words[0]], pool()[words[0]:words[0] + words[1]]
    d_num = dev.up(num_h, offsets[0]) if has_num else 0
    d_den = dev.up(den_h, offsets[1]) if has_den else 0
    d_out, d_tot = dev.alloc(words[2], offsets[2]), dev.alloc(2 * batch)
    dev.fill(d_out, words[2])
    ta.prover.column_scan_device(ctx, d_num, d_den, d_out, n, batch, op, init, d_tot, strides=strides)
    out, tot = dev.down(d_out, words[2]), dev.down(d_tot, 2 * batch)
    cols = []
    for b in range(batch):
        cols.append((out[b * os_:b * os_ + n], int(tot[2 * b]), int(tot[2 * b + 1]), num_h[b * ns:b * ns + n] if has_num else None,
                     den_h[b * ds:b * ds + n] if has_den else None))
        if b + 1 < batch:
            assert (out[b * os_ + n:(b + 1) * os_] == SENTINEL_WORD).all(), "the words between n and the stride were written"
    return cols


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("op", [SUM, PRODUCT])
def test_batches_with_padded_strides_solve_the_recurrence(ta, ctx, dev, T, op, form):
    k = 0
    for n in (1, 7, 8, 9, T - 1, T, T + 1, 2 * T + 1, (1 << 19) + T + 1):
        for batch in (1, 3):
            k += 1
            strides = (n + 3, n + 6, n + 1) if batch > 1 else (n, n, n)        # distinct: the columns of an operand differ in alignment
            offsets = (4 * (k % 4), 4 * ((k + 1) % 4), 4 * ((k + 3) % 4))
            init = [1, P - 1, 12345][:batch]
            for b, (out, total, zeros, num, den) in enumerate(run_batch(ta, ctx, dev, op, form, n, batch, strides, offsets, init)):
                assert zeros == 0 and recurrence_holds(op, out, total, num, den, init[b]), (n, batch, b)
            dev.free()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("op", [SUM, PRODUCT])
def test_a_column_whose_tile_prefixes_take_two_rounds(ta, ctx, dev, T, op, form):
    n = (1 << 22) + 3
    assert (n + T - 1) // T > T                                                 # more aggregates than one round of step 2 takes
    (out, total, zeros, num, den), = run_batch(ta, ctx, dev, op, form, n, 1, (n, n, n), (4 * op, 8, 12 if form == "num" else 0), [7])
    assert zeros == 0 and recurrence_holds(op, out, total, num, den, 7)


# ---- 2. zero denominators and field edges ----
def model(op, num, den, init):
    n = len(num if num is not None else den)
    acc, out, zeros = int(init), [], 0
    for i in range(n):
        out.append(acc)
        d = 1 if den is None else int(den[i])
        zeros += d == 0
        term = 0 if d == 0 else (1 if num is None else int(num[i])) * pow(d, -1, P) % P
        acc = (acc * term if op else acc + term) % P
    return np.array(out, dtype=np.uint32), acc, zeros


def edge_values(rng, n):
    v = rng.integers(0, P, n, dtype=np.uint64)
    pick = rng.integers(0, 8, n)
    v[pick == 0], v[pick == 1], v[pick == 2] = 0, 1, P - 1
    return v


@pytest.mark.parametrize("op", [SUM, PRODUCT])
def test_zero_denominators_and_field_edges_match_the_integer_model(ta, ctx, dev, T, op):
    G = 8                                                                       # a thread's group (the tile is 256 of them)
    rng = np.random.default_rng(40 + op)
    cases = []
    for n in (3 * T, 2 * T + 5, T - 1, 9):
        i = np.arange(n)
        num, den = edge_values(rng, n), rng.integers(1, P, n, dtype=np.uint64)
        den[(i % T == 0) | (i % T == T - 1) | (((i // G) % 3 == 1) & ((i % G == 0) | (i % G == G - 1))) | ((i // G) % 11 == 5)] = 0
        den[n - 1] = 0
        cases += [(num, den), (None, den), (edge_values(rng, n), edge_values(rng, n))]
    n = 2 * T + 5
    cases += [(edge_values(rng, n), np.zeros(n, dtype=np.uint64)), (None, np.zeros(n, dtype=np.uint64)),
              (np.full(n, P - 1, dtype=np.uint64), np.full(n, P - 1, dtype=np.uint64)), (np.full(n, P - 1, dtype=np.uint64), None),
              (None, np.full(n, P - 1, dtype=np.uint64)), (np.zeros(n, dtype=np.uint64), None)]
    met = 0
    for k, (num, den) in enumerate(cases):
        n = len(num if num is not None else den)
        init = [1, P - 1, 0, 77][k % 4] if op == SUM else [1, P - 1, 77][k % 3]
        d_num = dev.up(num, 4 * (k % 4)) if num is not None else 0
        d_den = dev.up(den, 4 * ((k + 2) % 4)) if den is not None else 0
        d_out, d_tot = dev.alloc(n, 4 * ((k + 1) % 4)), dev.alloc(2)
        ta.prover.column_scan_device(ctx, d_num, d_den, d_out, n, 1, op, [init], d_tot)
        got, tot = dev.down(d_out, n), dev.down(d_tot, 2)
        want, total, zeros = model(op, num, den, init)
        assert (got == want).all(), (k, n, int(np.flatnonzero(got != want)[0]))
        assert (int(tot[0]), int(tot[1])) == (total, zeros), (k, n)
        met += zeros
        dev.free()
    assert met > 3 * T


# ---- 3. the inversion alone ----
def test_batch_inverse(ta, dev, T):
    rng = np.random.default_rng(3)
    for k, count in enumerate((1, 7, 8, 9, T - 1, T + 1, (1 << 20) + 5)):
        for inplace in (False, True):
            v = edge_values(rng, count)
            if count > 24:
                v[8:16] = 0                                                     # a whole group
            d_in = dev.up(v, 4 * (k % 4))
            d_out = d_in if inplace else dev.alloc(count, 4 * ((k + 1 + inplace) % 4))
            d_zc = dev.alloc(1)
            dev.fill(d_zc, 1)
            ta.prover.batch_inverse_device(d_in, d_out, count, d_zc)
            got = dev.down(d_out, count).astype(np.uint64)
            assert (got < PU).all()
            assert np.all(np.where(v == 0, got == 0, got * v % PU == 1)), (count, inplace)
            assert int(dev.down(d_zc, 1)[0]) == int((v == 0).sum())
            ta.prover.batch_inverse_device(d_out, d_out, count)                 # without a counter, and back again
            assert (dev.down(d_out, count) == v).all()
            dev.free()


# ---- 4. in place ----
@pytest.mark.parametrize("op", [SUM, PRODUCT])
def test_in_place_on_either_operand_gives_the_same_words(ta, ctx, dev, T, op):
    rng = np.random.default_rng(50 + op)
    for n, batch in ((2 * T + 5, 3), ((1 << 19) + T + 1, 2), (5, 1)):
        stride = n + 2
        words = (batch - 1) * stride + n
        num, den = edge_values(rng, words), edge_values(rng, words)
        init = [3, 4, 5][:batch]
        d_out, d_tot = dev.alloc(words), dev.alloc(2 * batch)
        ta.prover.column_scan_device(ctx, dev.up(num), dev.up(den), d_out, n, batch, op, init, d_tot, strides=(stride,) * 3)
        want, want_tot = dev.down(d_out, words), dev.down(d_tot, 2 * batch)
        for which in (0, 1):
            d_num, d_den = dev.up(num, 4 * which), dev.up(den, 8 * which)
            dev.fill(d_tot, 2 * batch)
            ta.prover.column_scan_device(ctx, d_num, d_den, (d_num, d_den)[which], n, batch, op, init, d_tot, strides=(stride,) * 3)
            got, other = dev.down((d_num, d_den)[which], words), dev.down((d_den, d_num)[which], words)
            for b in range(batch):
                s = slice(b * stride, b * stride + n)
                assert (got[s] == want[s]).all(), (n, which, b)
                gap = slice(b * stride + n, min((b + 1) * stride, words))
                assert (got[gap] == (num, den)[which][gap]).all()               # the words up to the stride keep the operand's
            assert (other == (den, num)[which]).all() and (dev.down(d_tot, 2 * batch) == want_tot).all()
        dev.free()


# ---- 5. guard bands ----
@pytest.mark.parametrize("op", [SUM, PRODUCT])
@pytest.mark.parametrize("n,batch,off", [(5, 3, 4), (2049, 2, 12), (4101, 3, 0), (4096, 1, 8)])
def test_column_scan_between_guard_bands(ta, ctx, op, n, batch, off):
    rng = np.random.default_rng(60 + n)
    strides = (n + 3, n + 6, n + 1)
    words = [(batch - 1) * s + n for s in strides]
    num, den = edge_values(rng, words[0]), edge_values(rng, words[1])
    init = [1, 2, P - 1][:batch]
    results = []
    for pattern in ("sentinel", "random"):
        def between(v, s):                                                      # the words between n and the stride of every column
            v = v.astype(np.uint32)
            for b in range(batch - 1):
                v[b * s + n:(b + 1) * s] = SENTINEL_WORD if pattern == "sentinel" else rng.integers(0, 1 << 32, s - n, dtype=np.uint64)
            return v
        g_num, g_den = Guarded(ta, 4 * words[0], offset=off, seed=1), Guarded(ta, 4 * words[1], offset=(off + 4) % 16, seed=2)
        g_out, g_tot, g_zc = Guarded(ta, 4 * words[2], offset=(off + 8) % 16, seed=3), Guarded(ta, 8 * batch, seed=4), Guarded(ta, 4, seed=5)
        try:
            w_num, w_den = between(num, strides[0]), between(den, strides[1])
            for g_ in (g_num, g_den, g_out, g_tot, g_zc):
                g_.refill(pattern)
            g_num.upload(w_num), g_den.upload(w_den)
            ta.prover.column_scan_device(ctx, g_num.ptr, g_den.ptr, g_out.ptr, n, batch, op, init, g_tot.ptr, strides=strides)
            ta.prover.batch_inverse_device(g_den.ptr, g_den.ptr, n, g_zc.ptr)   # the first column of den, in place
            g_out.mem.sync()
            for g_, name in ((g_num, "num"), (g_den, "den"), (g_out, "out"), (g_tot, "totals"), (g_zc, "zero count")):
                g_.check(name)
            assert (g_num.download() == w_num).all() and (g_den.download()[n:] == w_den[n:]).all(), "an operand was changed"
            out = g_out.download()
            for b in range(batch - 1):
                assert (out[b * strides[2] + n:(b + 1) * strides[2]] == SENTINEL_WORD).all(), "written between n and the stride"
            results.append((np.concatenate([out[b * strides[2]:b * strides[2] + n] for b in range(batch)]), g_tot.download(), g_den.download()[:n],
                            g_zc.download()))
        finally:
            for g_ in (g_num, g_den, g_out, g_tot, g_zc):
                g_.free(check=False)
    for a, b in zip(*results):
        assert (a == b).all()
    out, tot = results[0][0], results[0][1]
    for b in range(batch):
        want, total, zeros = model(op, num[b * strides[0]:b * strides[0] + n], den[b * strides[1]:b * strides[1] + n], init[b])
        assert (out[b * n:(b + 1) * n] == want).all() and (int(tot[2 * b]), int(tot[2 * b + 1])) == (total, zeros)


# ---- 6. two stages of a proof ----
def tail_of_quotient(ta, dev, small, big, n, log_b, main_cols, term_of, op, init, constraints, first_zero):
    """Main columns -> per-row num and den through a program at log_blowup = 0 -> the accumulator column -> both matrices extended ->
    the quotient of `constraints` over the two matrices -> its coefficients from first_zero on, and the scan's total."""
    N = n << log_b
    pv = ta.prover
    width = len(main_cols)
    d_main = dev.up(np.array(main_cols, dtype=np.uint32).reshape(-1))
    d_num, d_den, d_acc, d_tot = dev.alloc(n), dev.alloc(n), dev.alloc(n), dev.alloc(2)
    bld = pv.AirBuilder()
    num, den = term_of(bld, lambda c: bld.cell(0, c, 0))
    bld.emit(0, num, divide=False), bld.emit(1, den, divide=False)
    with pv.AirProgram(small, bld.compile()) as terms:
        pv.air_quotient_device(small, terms, [(d_main, width, n)], 0, 1, [1, 0], d_num)
        pv.air_quotient_device(small, terms, [(d_main, width, n)], 0, 1, [0, 1], d_den)
    pv.column_scan_device(small, d_num, d_den, d_acc, n, 1, op, [init], d_tot)
    total, zeros = (int(v) for v in dev.down(d_tot, 2))
    assert zeros == 0
    d_coef, d_lde_main, d_lde_acc, d_q, d_poly = dev.alloc(width * n), dev.alloc(width * N), dev.alloc(N), dev.alloc(N), dev.alloc(N)
    small.run_device(d_main, d_coef, width, True)
    big.lde_device(d_coef, d_lde_main, width, log_b, COSET_SHIFT)
    small.run_device(d_acc, d_coef, 1, True)
    big.lde_device(d_coef, d_lde_acc, 1, log_b, COSET_SHIFT)
    bld = pv.AirBuilder()
    constraints(bld)
    rng = np.random.default_rng(n)
    with pv.AirProgram(big, bld.compile()) as prog:
        assert prog.info.nmatrices == 2 and prog.info.max_rotation == 1 and prog.info.divides_by_zh == 1
        pv.air_quotient_device(big, prog, [(d_lde_main, width, N), (d_lde_acc, 1, N)], log_b, COSET_SHIFT, [int(v) for v in rng.integers(1, P, 2)], d_q)
    big.run_device(d_q, d_poly, 1, True, shift=COSET_SHIFT)
    return dev.down(d_poly, N)[first_zero:], total


@pytest.mark.parametrize("n", [64, 1024])
def test_a_permutation_product_column_satisfies_its_constraints(ta, dev, n):
    log_b = 2
    rng = np.random.default_rng(700 + n)
    gamma = int(rng.integers(1, P))
    a = [int(v) for v in rng.integers(0, P, n)]
    b = [a[j] for j in rng.permutation(n)]
    term_of = lambda bld, cell: (cell(0) + gamma, cell(1) + gamma)

    def constraints(bld):
        ax, bx, zx, zgx = bld.cell(0, 0, 0), bld.cell(0, 1, 0), bld.cell(1, 0, 0), bld.cell(1, 0, 1)
        bld.emit(0, zgx * (bx + gamma) - zx * (ax + gamma))
        bld.emit(1, (zx - 1) * bld.xinv(1), divide=False)

    small, big = ta.NttContext(n), ta.NttContext(n << log_b)
    try:
        tail, total = tail_of_quotient(ta, dev, small, big, n, log_b, [a, b], term_of, PRODUCT, 1, constraints, n - 1)
        assert total == 1 and (tail == 0).all(), "a true permutation: the product closes and the quotient has degree n - 2"
        wrong = list(b)
        wrong[n // 3] = (wrong[n // 3] + 1) % P
        tail, total = tail_of_quotient(ta, dev, small, big, n, log_b, [a, wrong], term_of, PRODUCT, 1, constraints, n - 1)
        assert total != 1 and tail[-1] != 0
    finally:
        small.destroy()
        big.destroy()


@pytest.mark.parametrize("n", [64, 1024])
def test_a_logup_sum_column_satisfies_its_constraints(ta, dev, n):
    log_b = 2
    rng = np.random.default_rng(800 + n)
    gamma = int(rng.integers(1, P))
    t = [int(v) for v in rng.permutation(np.unique(rng.integers(0, P, 4 * n))[:n])]             # distinct table entries
    picks = rng.integers(0, n // 4, n)                                          # a quarter of the table is looked up, most rows more than once
    v = [t[j] for j in picks]
    m = [int(c) for c in np.bincount(picks, minlength=n)]
    # columns v, t, m:  term = 1 / (gamma + v) - m / (gamma + t) = ((gamma + t) - m (gamma + v)) / ((gamma + v)(gamma + t))
    term_of = lambda bld, cell: ((cell(1) + gamma) - cell(2) * (cell(0) + gamma), (cell(0) + gamma) * (cell(1) + gamma))

    def constraints(bld):
        vx, tx, mx, sx, sgx = bld.cell(0, 0, 0), bld.cell(0, 1, 0), bld.cell(0, 2, 0), bld.cell(1, 0, 0), bld.cell(1, 0, 1)
        bld.emit(0, (sgx - sx) * ((vx + gamma) * (tx + gamma)) - ((tx + gamma) - mx * (vx + gamma)))
        bld.emit(1, sx * bld.xinv(1), divide=False)

    small, big = ta.NttContext(n), ta.NttContext(n << log_b)
    try:
        tail, total = tail_of_quotient(ta, dev, small, big, n, log_b, [v, t, m], term_of, SUM, 0, constraints, 2 * n - 2)
        assert total == 0 and (tail == 0).all(), "a true lookup: the sum closes and the quotient has degree 2 n - 3"
        wrong = list(m)
        wrong[int(picks[0])] += 1
        tail, total = tail_of_quotient(ta, dev, small, big, n, log_b, [v, t, wrong], term_of, SUM, 0, constraints, 2 * n - 2)
        assert total != 0 and tail[-1] != 0
    finally:
        small.destroy()
        big.destroy()


# ---- 7. graph capture ----
def test_a_call_on_a_warm_context_can_be_captured_and_replayed(ta, T):
    import torch
    tdev = torch.device("cuda", 0)
    n, batch, stride = 8 * T + 5, 3, 8 * T + 8
    rng = np.random.default_rng(77)
    ctx = ta.NttContext(64)
    try:
        num, den = (torch.zeros(batch * stride, dtype=torch.int32, device=tdev) for _ in range(2))
        out, tot = torch.empty(batch * stride, dtype=torch.int32, device=tdev), torch.empty(2 * batch, dtype=torch.int32, device=tdev)
        s = torch.cuda.Stream(device=tdev)
        call = lambda: ta.prover.column_scan_device(ctx, num.data_ptr(), den.data_ptr(), out.data_ptr(), n, batch, PRODUCT, [1, 2, 3], tot.data_ptr(),
                                                    strides=(stride,) * 3, stream=s.cuda_stream)
        call()                                                                  # eager, warm: the intermediate buffer exists from here on
        ctx.synchronize(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):                                     # three kernel nodes in a line
            call()
        for rep in range(2):
            for buf in (num, den):
                buf.copy_(torch.from_numpy(edge_values(rng, batch * stride).astype(np.uint32).view(np.int32)))
            out.fill_(-1), tot.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got, got_tot = out.cpu().numpy().view(np.uint32).copy(), tot.cpu().numpy().view(np.uint32).copy()
            out.fill_(-1), tot.fill_(-1)
            call()                                                              # the direct call on the same contents
            torch.cuda.synchronize()
            assert (got == out.cpu().numpy().view(np.uint32)).all() and (got_tot == tot.cpu().numpy().view(np.uint32)).all(), rep
            h_num, h_den = num.cpu().numpy().view(np.uint32), den.cpu().numpy().view(np.uint32)
            want, total, zeros = model(PRODUCT, h_num[stride:stride + n], h_den[stride:stride + n], 2)
            assert (got[stride:stride + n] == want).all() and (int(got_tot[2]), int(got_tot[3])) == (total, zeros)
        del g
    finally:
        ctx.destroy()
