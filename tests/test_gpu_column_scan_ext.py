"""Accumulator columns under an Ext challenge on the device (include/toyni_hip.h 3i): toyni_column_scan_ext_device and
toyni_batch_inverse_ext_device.  T = the tile, G = 4 the elements of a thread.
  1. the recurrence without an inversion on the host: no denominator is zero (asserted), so the output is the unique solution of
         sum      (out[i+1] - out[i]) den_i = num_i          product   out[i+1] den_i = out[i] num_i          out[0] = init
     with the wrap-around step against d_totals, checked at EVERY point by vectorised uint64 Ext products -- every n in 1..2G+1,
     T-G-1..T+G+1, 2T-1..2T+G+1; both ops, the eight (numerator width, denominator width) forms, batch 1 and 3 with distinct padded
     strides, columns 0 / 4 / 8 / 12 bytes off alignment; and n = T T + T + 1 in the (4, 4) form, where step 2 loops
  2. zero denominators and field edges against the Python-integer model of tests/ext_model.py, with the zero counts
  3. embedded base field: coordinate 0 is toyni_column_scan_device's word, coordinates 1..3 are 0
  4. the inversion alone: a a^-1 = 1, zeros give 0 and are counted, in place
  5. in place on a width-4 numerator and on a width-4 denominator
  6. guard bands around every operand, the output, the totals and the words between n and each stride
  7. a call captured into a graph and replayed
  8. two stages of a proof composed under an Ext gamma"""
import hashlib

import numpy as np
import pytest

import ext_model as E
from guarded import DevMem, Guarded
from harness.fib_prover import COSET_SHIFT

pytestmark = pytest.mark.gpu

P = E.P
PU = np.uint64(P)
SUM, PRODUCT = 0, 1
G = 4
FORMS = [(1, 1), (4, 4), (1, 4), (4, 1), (0, 1), (0, 4), (1, 0), (4, 0)]
SENTINEL_WORD = 0xA5A5A5A5


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


@pytest.fixture(scope="module")
def T(ta):
    return ta.prover.column_scan_ext_tile()


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


_pool = {}


def pool(words):
    """Residues from a fixed seed, shared and never changed: every recurrence case reads slices of it."""
    if "v" not in _pool or _pool["v"].size < words:
        v = np.random.default_rng(0xE5CA).integers(0, P, max(words, 1 << 16), dtype=np.uint64)
        v.setflags(write=False)
        _pool["v"] = v
    return _pool["v"]


NSHIFT, DSHIFT = (11, 22, 33, 44), (1234567, 7654321, 99, 2013265920)


def words_of(width, batch, stride, n):
    return (width * batch - 1) * stride + n if width else 0


def elements(host, width, shift, b, stride, n):
    """Column b of an operand as an (n, 4) uint64 array of Ext elements, the shift added; width 0: ones."""
    e = np.zeros((n, 4), dtype=np.uint64)
    if width == 0:
        e[:, 0] = 1
        return e
    if width == 1:
        e[:, 0] = host[b * stride:b * stride + n]
    else:
        for k in range(4):
            e[:, k] = host[(4 * b + k) * stride:(4 * b + k) * stride + n]
    return (e + np.array(shift, dtype=np.uint64)) % PU


def ext_columns(out, b, stride, n):
    return np.stack([out[(4 * b + k) * stride:(4 * b + k) * stride + n] for k in range(4)], axis=-1).astype(np.uint64)


def recurrence_failures(op, out, total, num, den, init):
    """Indices at which the recurrence fails (the wrap-around step is index n - 1); -1 for a wrong out[0] or a non-canonical word."""
    nxt = np.concatenate([out[1:], np.asarray(total, dtype=np.uint64).reshape(1, 4)])
    if op == SUM:
        ok = (E.vmul((nxt + PU - out) % PU, den) == num).all(axis=-1)
    else:
        ok = (E.vmul(nxt, den) == E.vmul(out, num)).all(axis=-1)
    bad = list(np.flatnonzero(~ok))
    if not (out[0] == np.asarray(init, dtype=np.uint64)).all() or not (out < PU).all() or not (np.asarray(total, dtype=np.uint64) < PU).all():
        bad.insert(0, -1)
    return bad


def run_case(ta, ctx, dev, op, nw, dw, n, batch, strides, offsets, init, d_pool, host, shifts=(NSHIFT, DSHIFT)):
    """One call on slices of the device copy of the pool (numerators from word 0, denominators from word `half`); every point checked."""
    ns, ds, os_ = strides
    half = host.size // 2
    d_num, d_den = d_pool + 4 * offsets[0], d_pool + 4 * (half + offsets[1])
    h_num, h_den = host[offsets[0]:], host[half + offsets[1]:]
    num = ta.prover.ExtOperand(d_num, ns, nw, shifts[0]) if nw else None
    den = ta.prover.ExtOperand(d_den, ds, dw, shifts[1]) if dw else None
    ow = words_of(4, batch, os_, n)
    d_out, d_tot = dev.alloc(ow, 4 * offsets[2]), dev.alloc(8 * batch)
    dev.fill(d_out, ow), dev.fill(d_tot, 8 * batch)
    ta.prover.column_scan_ext_device(ctx, num, den, d_out, os_, n, batch, op, init, d_tot)
    out, tot = dev.down(d_out, ow), dev.down(d_tot, 8 * batch).reshape(batch, 8)
    for b in range(batch):
        en, ed = elements(h_num, nw, shifts[0], b, ns, n), elements(h_den, dw, shifts[1], b, ds, n)
        assert ed.any(axis=-1).all(), "the check needs every denominator non-zero: no point is exempt"
        bad = recurrence_failures(op, ext_columns(out, b, os_, n), tot[b, :4], en, ed, init[b])
        assert not bad, (op, nw, dw, n, batch, b, "first failure at", bad[0])
        assert list(tot[b, 4:]) == [0, 0, 0, 0]
    gaps = np.ones(ow, dtype=bool)
    for c in range(4 * batch):
        gaps[c * os_:c * os_ + n] = False
    assert (out[gaps] == SENTINEL_WORD).all(), "the words between n and the stride were written"


# ---- 1. the recurrence ----
@pytest.mark.parametrize("form", FORMS, ids=lambda f: "%d-%d" % f)
@pytest.mark.parametrize("op", [SUM, PRODUCT])
def test_every_n_around_the_group_and_the_tile_solves_the_recurrence(ta, ctx, dev, T, op, form):
    nw, dw = form
    sizes = list(range(1, 2 * G + 2)) + list(range(T - G - 1, T + G + 2)) + list(range(2 * T - 1, 2 * T + G + 2))
    top = max(sizes)
    half = 12 * (top + 8) + 8
    host = pool(2 * half)[:2 * half]
    d_pool = dev.up(host)
    k = 0
    for n in sizes:
        for batch in (1, 3):
            k += 1
            strides = (n + 3, n + 6, n + 1) if batch > 1 else (n, n, n)        # distinct: the coordinate columns differ in alignment
            offsets = (k % 4, (k + 1) % 4, (k + 3) % 4)                         # words: 0 / 4 / 8 / 12 bytes off alignment
            init = [E.ONE if op == PRODUCT else E.ZERO, (P - 1, 0, 5, P - 1), (12345, 1, 2, 3)][:batch]
            run_case(ta, ctx, dev, op, nw, dw, n, batch, strides, offsets, init, d_pool, host)
        ptrs, dev.ptrs = dev.ptrs[1:], dev.ptrs[:1]                             # keep the pool, free the outputs
        dev.mem.sync()
        for p in ptrs:
            dev.mem.free(p)


@pytest.mark.parametrize("op", [SUM, PRODUCT])
def test_a_column_whose_tile_prefixes_take_two_rounds(ta, ctx, dev, T, op):
    n = T * T + T + 1
    assert (n + T - 1) // T > T                                                 # more aggregates than one round of step 2 takes
    half = 4 * n + 8
    host = pool(2 * half)[:2 * half]
    run_case(ta, ctx, dev, op, 4, 4, n, 1, (n, n, n), (1 + op, 2, 3), [(7, 8, 9, 10)], dev.up(host), host)


# ---- 2. zero denominators and field edges ----
def model(op, n, num, nw, nshift, den, dw, dshift, init):
    """Python integers.  num / den: lists of stored coordinate columns.  -> (out (n, 4), total, zeros)"""
    def operand(cols, width, shift, i):
        if width == 0:
            return E.ONE
        return E.add(E.embed(cols[0][i]) if width == 1 else tuple(int(c[i]) for c in cols), shift)
    dens = [operand(den, dw, dshift, i) for i in range(n)]
    invs = E.batch_inverse(dens) if dw else [E.ONE] * n
    acc, out = tuple(int(v) for v in init), []
    for i in range(n):
        out.append(acc)
        term = E.mul(operand(num, nw, nshift, i), invs[i])
        acc = E.mul(acc, term) if op else E.add(acc, term)
    return np.array(out, dtype=np.uint32), acc, sum(1 for d in dens if not any(d))


def edge_values(rng, n):
    v = rng.integers(0, P, n, dtype=np.uint64)
    pick = rng.integers(0, 8, n)
    v[pick == 0], v[pick == 1], v[pick == 2] = 0, 1, P - 1
    return v


def zero_places(n, T, kind):
    i = np.arange(n)
    if kind == "edges":       # first / last slot of a group, first / last element of a tile, the last element
        return (i % T == 0) | (i % T == T - 1) | (((i // G) % 3 == 1) & ((i % G == 0) | (i % G == G - 1))) | (i == n - 1)
    if kind == "groups":      # whole groups
        return (i // G) % 2 == 1
    return np.ones(n, dtype=bool) if kind == "all" else np.zeros(n, dtype=bool)


@pytest.mark.parametrize("op", [SUM, PRODUCT])
def test_zero_denominators_and_field_edges_match_the_integer_model(ta, ctx, dev, T, op):
    rng = np.random.default_rng(140 + op)
    met, partial, k = 0, 0, 0
    for n in (2 * T + 5, T + 1, T - 1, G + 1):
        for nw, dw, kind in ((4, 4, "edges"), (1, 1, "edges"), (0, 4, "groups"), (4, 1, "groups"), (1, 4, "all"), (0, 1, "all"), (4, 4, "none"), (4, 0, "none")):
            if kind == "all" and n != T + 1:
                continue
            k += 1
            nshift = tuple(int(v) for v in rng.integers(1, P, 4)) if nw else (0, 0, 0, 0)
            # a width-1 denominator vanishes only under a base-field shift (s, 0, 0, 0), at v = p - s
            dshift = (int(rng.integers(1, P)), 0, 0, 0) if dw == 1 else tuple(int(v) for v in rng.integers(1, P, 4)) if dw else (0, 0, 0, 0)
            num = [edge_values(rng, n) for _ in range(nw)]
            zero = zero_places(n, T, kind)
            if dw == 1:
                v = edge_values(rng, n)
                v[v == P - dshift[0]] = 1
                v[zero] = P - dshift[0]
                den = [v]
            elif dw == 4:
                d = np.stack([edge_values(rng, n) for _ in range(4)])           # the VALUES shift + stored: coordinates from the edges ...
                i = np.arange(n)
                for r, count in ((3, 1), (4, 2), (5, 3)):                       # ... with one, two and three zero coordinates, the norm non-zero
                    for c in range(count):
                        d[(i // 7 + c) % 4, i] = np.where(i % 7 == r, 0, d[(i // 7 + c) % 4, i])
                d[3, ~d.any(axis=0)] = 5
                partial += int(((d == 0).sum(axis=0) > 0).sum())
                d[:, zero] = 0
                den = [(d[c] + PU - np.uint64(dshift[c])) % PU for c in range(4)]
            else:
                den = []
            init = [(1, 0, 0, 0), (P - 1, P - 1, 0, 1), (0, 0, 0, 0), (77, 0, 0, P - 1)][k % 4]
            if op == PRODUCT and not any(init):
                init = (0, 1, 0, 0)
            d_num = dev.up(np.concatenate(num), 4 * (k % 4)) if nw else 0
            d_den = dev.up(np.concatenate(den), 4 * ((k + 2) % 4)) if dw else 0
            d_out, d_tot = dev.alloc(4 * n, 4 * ((k + 1) % 4)), dev.alloc(8)
            Op = ta.prover.ExtOperand
            ta.prover.column_scan_ext_device(ctx, Op(d_num, n, nw, nshift) if nw else None, Op(d_den, n, dw, dshift) if dw else None, d_out, n, n, 1, op,
                                             [init], d_tot)
            got, tot = dev.down(d_out, 4 * n).reshape(4, n).T, dev.down(d_tot, 8)
            want, total, zeros = model(op, n, num, nw, nshift, den, dw, dshift, init)
            assert zeros == int(zero.sum()) if dw else zeros == 0
            assert (got == want).all(), (n, nw, dw, kind, int(np.flatnonzero((got != want).any(axis=1))[0]))
            assert list(tot) == list(total) + [zeros, 0, 0, 0], (n, nw, dw, kind)
            met += zeros
            dev.free()
    assert met > 2 * T and partial > T


# ---- 3. the embedded base field ----
@pytest.mark.parametrize("op", [SUM, PRODUCT])
def test_embedded_from_the_base_field_it_is_the_base_scan(ta, ctx, dev, T, op):
    rng = np.random.default_rng(150 + op)
    Op = ta.prover.ExtOperand
    for n, batch in ((2 * T + 5, 2), (9, 1), (3 * ta.prover.column_scan_tile() + 1, 1)):
        stride = n + 3
        words = (batch - 1) * stride + n
        sn, sd = int(rng.integers(1, P)), int(rng.integers(1, P))
        num, den = edge_values(rng, words), edge_values(rng, words)
        den[::97] = P - sd                                                      # zero denominators after the shift
        init = [int(v) for v in rng.integers(1, P, batch)]
        d_base, d_btot = dev.alloc(words), dev.alloc(2 * batch)
        ta.prover.column_scan_device(ctx, dev.up((num + np.uint64(sn)) % PU), dev.up((den + np.uint64(sd)) % PU), d_base, n, batch, op, init, d_btot,
                                     strides=(stride,) * 3)
        base, btot = dev.down(d_base, words), dev.down(d_btot, 2 * batch)
        wide = lambda v: np.concatenate([np.concatenate([v[b * stride:b * stride + n], np.zeros(stride - n, np.uint64)] + [np.zeros(stride, np.uint64)] * 3)
                                         for b in range(batch)])
        for width in (1, 4):                                                    # a base column, and an Ext column whose coordinates 1..3 are 0
            d_num, d_den = (dev.up(num), dev.up(den)) if width == 1 else (dev.up(wide(num)), dev.up(wide(den)))
            d_out, d_tot = dev.alloc(4 * batch * stride), dev.alloc(8 * batch)
            ta.prover.column_scan_ext_device(ctx, Op(d_num, stride, width, (sn, 0, 0, 0)), Op(d_den, stride, width, (sd, 0, 0, 0)), d_out, stride, n, batch, op,
                                             [(v, 0, 0, 0) for v in init], d_tot)
            out, tot = dev.down(d_out, 4 * batch * stride), dev.down(d_tot, 8 * batch).reshape(batch, 8)
            for b in range(batch):
                assert (out[4 * b * stride:4 * b * stride + n] == base[b * stride:b * stride + n]).all(), (n, width, b)
                for c in (1, 2, 3):
                    assert not out[(4 * b + c) * stride:(4 * b + c) * stride + n].any(), (n, width, b, c)
                assert list(tot[b]) == [btot[2 * b], 0, 0, 0, btot[2 * b + 1], 0, 0, 0] and btot[2 * b + 1] > 0
        dev.free()


# ---- 4. the inversion alone ----
def test_batch_inverse_ext(ta, dev, T):
    rng = np.random.default_rng(13)
    for k, count in enumerate((1, G - 1, G, G + 1, T - 1, T, T + 1, 2 * T + 5)):
        for inplace in (False, True):
            stride = count + (k % 3)
            v = np.stack([edge_values(rng, count) for _ in range(4)])
            v[:, ~v.any(axis=0)] = 3
            v[1:, ::5] = 0                                                      # three zero coordinates
            v[:, 2::7] = 0                                                      # zeros ...
            if count > 3 * G:
                v[:, G:2 * G] = 0                                               # ... and a whole group of them
            stored = np.full(3 * stride + count, 0xFFFFFFF0, dtype=np.uint64)
            for c in range(4):
                stored[c * stride:c * stride + count] = v[c]
            d_in = dev.up(stored, 4 * (k % 4))
            d_out = d_in if inplace else dev.alloc(3 * stride + count, 4 * ((k + 1) % 4))
            if not inplace:
                dev.fill(d_out, 3 * stride + count)
            d_zc = dev.alloc(1)
            dev.fill(d_zc, 1)
            ta.prover.batch_inverse_ext_device(d_in, stride, d_out, stride, count, d_zc)
            raw = dev.down(d_out, 3 * stride + count)
            got = np.stack([raw[c * stride:c * stride + count] for c in range(4)], axis=-1).astype(np.uint64)
            zero = ~v.any(axis=0)
            assert (got < PU).all() and not got[zero].any()
            one = np.zeros((count, 4), dtype=np.uint64)
            one[~zero, 0] = 1
            assert (E.vmul(got, v.T) == one).all(), (count, inplace)
            assert int(dev.down(d_zc, 1)[0]) == int(zero.sum())
            for c in range(3):                                                  # the words between count and the stride
                assert (raw[c * stride + count:(c + 1) * stride] == (0xFFFFFFF0 if inplace else SENTINEL_WORD)).all()
            ta.prover.batch_inverse_ext_device(d_out, stride, d_out, stride, count)     # without a counter, and back again
            back = dev.down(d_out, 3 * stride + count)
            assert all((back[c * stride:c * stride + count] == v[c]).all() for c in range(4))
            dev.free()


# ---- 5. in place ----
@pytest.mark.parametrize("op", [SUM, PRODUCT])
def test_in_place_on_a_width_4_operand_gives_the_same_words(ta, ctx, dev, T, op):
    rng = np.random.default_rng(160 + op)
    Op = ta.prover.ExtOperand
    for n, batch in ((2 * T + 5, 3), (5, 1), (T, 2)):
        stride = n + 2
        words = (4 * batch - 1) * stride + n
        num, den = edge_values(rng, words), edge_values(rng, words)
        init = [(3, 1, 4, 1), (5, 9, 2, 6), (5, 3, 5, 8)][:batch]
        d_out, d_tot = dev.alloc(words), dev.alloc(8 * batch)
        ta.prover.column_scan_ext_device(ctx, Op(dev.up(num), stride, 4, NSHIFT), Op(dev.up(den), stride, 4, DSHIFT), d_out, stride, n, batch, op, init, d_tot)
        want, want_tot = dev.down(d_out, words), dev.down(d_tot, 8 * batch)
        live = np.zeros(words, dtype=bool)
        for c in range(4 * batch):
            live[c * stride:c * stride + n] = True
        for which in (0, 1):
            d_num, d_den = dev.up(num, 4 * which), dev.up(den, 8 * which)
            dev.fill(d_tot, 8 * batch)
            ta.prover.column_scan_ext_device(ctx, Op(d_num, stride, 4, NSHIFT), Op(d_den, stride, 4, DSHIFT), (d_num, d_den)[which], stride, n, batch, op, init,
                                             d_tot)
            got, other = dev.down((d_num, d_den)[which], words), dev.down((d_den, d_num)[which], words)
            assert (got[live] == want[live]).all(), (n, which)
            assert (got[~live] == (num, den)[which][~live]).all()               # the words up to the stride keep the operand's
            assert (other == (den, num)[which]).all() and (dev.down(d_tot, 8 * batch) == want_tot).all()
        dev.free()


# ---- 6. guard bands ----
@pytest.mark.parametrize("op", [SUM, PRODUCT])
@pytest.mark.parametrize("form", [(4, 4), (1, 1), (4, 1)], ids=lambda f: "%d-%d" % f)
@pytest.mark.parametrize("n,batch,off", [(5, 3, 4), (1025, 2, 12), (2053, 1, 0)])
def test_ext_column_scan_between_guard_bands(ta, ctx, op, form, n, batch, off):
    nw, dw = form
    rng = np.random.default_rng(170 + n)
    strides = (n + 3, n + 6, n + 1)
    words = [words_of(nw, batch, strides[0], n), words_of(dw, batch, strides[1], n), words_of(4, batch, strides[2], n)]
    num, den = edge_values(rng, words[0]), edge_values(rng, words[1])
    dshift = (DSHIFT[0], 0, 0, 0) if dw == 1 else DSHIFT
    den[::53] = P - dshift[0]
    init = [(1, 2, 3, 4), (2, 0, 0, 0), (P - 1, 1, 1, 1)][:batch]
    Op = ta.prover.ExtOperand
    results = []
    for pattern in ("sentinel", "random"):
        def between(v, s, width):                                               # the words between n and the stride of every base column
            v = v.astype(np.uint32)
            for c in range(width * batch - 1):
                v[c * s + n:(c + 1) * s] = SENTINEL_WORD if pattern == "sentinel" else rng.integers(0, 1 << 32, s - n, dtype=np.uint64)
            return v
        g_num, g_den = Guarded(ta, 4 * words[0], offset=off, seed=1), Guarded(ta, 4 * words[1], offset=(off + 4) % 16, seed=2)
        g_out, g_tot, g_zc = Guarded(ta, 4 * words[2], offset=(off + 8) % 16, seed=3), Guarded(ta, 32 * batch, seed=4), Guarded(ta, 4, seed=5)
        g_inv = Guarded(ta, 4 * (3 * strides[2] + n), offset=(off + 12) % 16, seed=6)
        try:
            w_num, w_den = between(num, strides[0], nw), between(den, strides[1], dw)
            for g_ in (g_num, g_den, g_out, g_tot, g_zc, g_inv):
                g_.refill(pattern)
            g_num.upload(w_num), g_den.upload(w_den)
            ta.prover.column_scan_ext_device(ctx, Op(g_num.ptr, strides[0], nw, NSHIFT), Op(g_den.ptr, strides[1], dw, dshift), g_out.ptr, strides[2], n, batch,
                                             op, init, g_tot.ptr)
            ta.prover.batch_inverse_ext_device(g_out.ptr, strides[2], g_inv.ptr, strides[2], n, g_zc.ptr)   # the first Ext column of the output
            g_out.mem.sync()
            for g_, name in ((g_num, "num"), (g_den, "den"), (g_out, "out"), (g_tot, "totals"), (g_zc, "zero count"), (g_inv, "inverses")):
                g_.check(name)
            assert (g_num.download() == w_num).all() and (g_den.download() == w_den).all(), "an operand was changed"
            out, inv = g_out.download(), g_inv.download()
            for c in range(4 * batch - 1):
                assert (out[c * strides[2] + n:(c + 1) * strides[2]] == SENTINEL_WORD).all(), "written between n and the stride"
            for c in range(3):
                assert (inv[c * strides[2] + n:(c + 1) * strides[2]] == SENTINEL_WORD).all(), "the inversion wrote between count and the stride"
            results.append((np.stack([out[c * strides[2]:c * strides[2] + n] for c in range(4 * batch)]), g_tot.download(),
                            np.stack([inv[c * strides[2]:c * strides[2] + n] for c in range(4)]), g_zc.download()))
        finally:
            for g_ in (g_num, g_den, g_out, g_tot, g_zc, g_inv):
                g_.free(check=False)
    for a, b in zip(*results):
        assert (a == b).all()
    out, tot = results[0][0], results[0][1].reshape(batch, 8)
    met = 0
    for b in range(batch):
        cn = [num[(nw * b + c) * strides[0]:(nw * b + c) * strides[0] + n] for c in range(nw)]
        cd = [den[(dw * b + c) * strides[1]:(dw * b + c) * strides[1] + n] for c in range(dw)]
        want, total, zeros = model(op, n, cn, nw, NSHIFT, cd, dw, dshift, init[b])
        assert (out[4 * b:4 * b + 4].T == want).all() and list(tot[b]) == list(total) + [zeros, 0, 0, 0]
        met += zeros
    assert met > 0 or dw == 4
    first = out[:4].T.astype(np.uint64)
    one = np.zeros((n, 4), dtype=np.uint64)
    one[first.any(axis=1), 0] = 1
    assert (E.vmul(results[0][2].T, first) == one).all() and int(results[0][3][0]) == int((~first.any(axis=1)).sum())


# ---- 7. graph capture ----
def test_a_call_on_a_warm_context_can_be_captured_and_replayed(ta, T):
    import torch
    tdev = torch.device("cuda", 0)
    n, batch, stride = 4 * T + 5, 2, 4 * T + 8
    rng = np.random.default_rng(177)
    ctx = ta.NttContext(64)
    Op = ta.prover.ExtOperand
    try:
        num = torch.zeros(4 * batch * stride, dtype=torch.int32, device=tdev)
        den = torch.zeros(batch * stride, dtype=torch.int32, device=tdev)
        out, tot = torch.empty(4 * batch * stride, dtype=torch.int32, device=tdev), torch.empty(8 * batch, dtype=torch.int32, device=tdev)
        s = torch.cuda.Stream(device=tdev)
        init = [(1, 0, 0, 0), (2, 3, 4, 5)]
        call = lambda: ta.prover.column_scan_ext_device(ctx, Op(num.data_ptr(), stride, 4, NSHIFT), Op(den.data_ptr(), stride, 1, DSHIFT), out.data_ptr(), stride,
                                                        n, batch, PRODUCT, init, tot.data_ptr(), stream=s.cuda_stream)
        call()                                                                  # eager, warm: the intermediate buffer exists from here on
        ctx.synchronize(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):                                     # three kernel nodes in a line
            call()
        for rep in range(2):
            for buf in (num, den):
                buf.copy_(torch.from_numpy(edge_values(rng, buf.numel()).astype(np.uint32).view(np.int32)))
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
            cn = [h_num[(4 + c) * stride:(4 + c) * stride + n] for c in range(4)]
            want, total, zeros = model(PRODUCT, n, cn, 4, NSHIFT, [h_den[stride:stride + n]], 1, DSHIFT, init[1])
            assert (np.stack([got[(4 + c) * stride:(4 + c) * stride + n] for c in range(4)]).T == want).all()
            assert list(got_tot[8:]) == list(total) + [zeros, 0, 0, 0]
        del g
    finally:
        ctx.destroy()


# ---- 8. two stages of a proof ----
def ext_weights(alphas):
    """The weights of the four base-field calls that together weigh Ext constraint k by alphas[k]: base constraint 4 k + j carries
    coordinate j of the constraint's value, so call c weighs it by coordinate c of alphas[k] X^j."""
    basis = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
    return [[E.mul(a, basis[j])[c] for a in alphas for j in range(4)] for c in range(4)]


def merkle_root(leaves):
    level = [hashlib.sha256(b"\x00" + l).digest() for l in leaves]
    while len(level) > 1:
        level = [hashlib.sha256(b"\x01" + level[i] + level[min(i + 1, len(level) - 1)]).digest() for i in range(0, len(level), 2)]
    return level[0]


def staged_proof_tail(ta, dev, small, big, n, log_b, main, gamma, alphas, z):
    """main: columns a, b (the permutation), u, w (the lookup: numerators and denominators).  -> (the quotient's four coefficient
    columns, the two wrap-around totals, q(z) from the device, q(z) from the model)."""
    pv = ta.prover
    N = n << log_b
    d_main = dev.up(np.array(main, dtype=np.uint32).reshape(-1))
    col = lambda c: d_main + 4 * c * n
    d_acc, d_tot = dev.alloc(8 * n), dev.alloc(16)
    # stage 2: both accumulators from main-trace columns in the width-1 forms; together the second matrix, eight base columns
    pv.column_scan_ext_device(small, pv.ExtOperand(col(0), n, 1, gamma), pv.ExtOperand(col(1), n, 1, gamma), d_acc, n, n, 1, PRODUCT, [E.ONE], d_tot)
    pv.column_scan_ext_device(small, pv.ExtOperand(col(2), n, 1, E.ZERO), pv.ExtOperand(col(3), n, 1, gamma), d_acc + 16 * n, n, n, 1, SUM, [E.ZERO], d_tot + 32)
    tot = dev.down(d_tot, 16).reshape(2, 8)
    assert tot[0, 4] == 0 and tot[1, 4] == 0
    d_cm, d_ca, d_lm, d_la = dev.alloc(4 * n), dev.alloc(8 * n), dev.alloc(4 * N), dev.alloc(8 * N)
    small.run_device(d_main, d_cm, 4, True)
    big.lde_device(d_cm, d_lm, 4, log_b, COSET_SHIFT)
    small.run_device(d_acc, d_ca, 8, True)                                      # the batched inverse transform of the eight columns
    big.lde_device(d_ca, d_la, 8, log_b, COSET_SHIFT)
    total_digests = int(ta._lib.lib.toyni_merkle_total_digests(N))
    d_levels = dev.alloc(8 * total_digests)
    ta.merkle_commit_rows_device(d_la, N, 8, ta.ROWS_COLUMN_MAJOR, N, 0, d_levels)
    lde_acc = dev.down(d_la, 8 * N).reshape(8, N)
    leaves = [r.tobytes() for r in np.ascontiguousarray(lde_acc.T).astype("<u8")]
    assert dev.down(d_levels, 8 * total_digests)[-8:].tobytes() == merkle_root(leaves), "the commitment to the accumulator matrix"
    # the constraints that tie the accumulators to the main trace, written with the Ext helper; both transitions hold on every row,
    # the wrap-around included, exactly when the totals equal init
    bld = pv.AirBuilder()
    g = bld.ext_const(gamma)
    a, b, u, w = (bld.cell(0, c) for c in range(4))
    zc, zn, sc, sn = bld.ext_cell(1, 0, 0), bld.ext_cell(1, 0, 1), bld.ext_cell(1, 4, 0), bld.ext_cell(1, 4, 1)
    bld.emit_ext(0, zn * (g + b) - zc * (g + a))
    bld.emit_ext(1, (sn - sc) * (g + w) - u)
    bld.emit_ext(2, (zc - 1) * bld.xinv(1), divide=False)
    bld.emit_ext(3, sc * bld.xinv(1), divide=False)
    d_q, d_qc, d_qz = dev.alloc(4 * N), dev.alloc(4 * N), dev.alloc(16)
    with pv.AirProgram(big, bld.compile()) as prog:
        assert prog.info.nconstraints == 16 and prog.info.nmatrices == 2 and list(prog.info.min_width)[:2] == [4, 8]
        for c, wts in enumerate(ext_weights(alphas)):                           # the quotient under Ext weights: four calls, four base columns
            pv.air_quotient_device(big, prog, [(d_lm, 4, N), (d_la, 8, N)], log_b, COSET_SHIFT, wts, d_q + 4 * c * N)
    big.run_device(d_q, d_qc, 4, True, shift=COSET_SHIFT)
    coeffs = dev.down(d_qc, 4 * N).reshape(4, N)
    pv.poly_eval_ext_batch_device(big, d_qc, N, N, 4, [z], d_qz)
    qz = dev.down(d_qz, 16).reshape(4, 4)
    basis = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
    q_dev = E.ZERO
    for j in range(4):
        q_dev = E.add(q_dev, E.mul(basis[j], tuple(int(v) for v in qz[j])))     # q(z) = sum_j X^j q_j(z)
    # the model: the constraints evaluated at z from the columns' out-of-domain values
    gz = tuple(v * pow(E.GEN_2_27, (1 << 27) // n, P) % P for v in z)
    cm, ca = dev.down(d_cm, 4 * n).reshape(4, n), dev.down(d_ca, 8 * n).reshape(8, n)
    at = lambda coef, pt: E.poly_eval_ext(coef, pt)
    ext_at = lambda first, pt: tuple(sum(E.mul(basis[j], at(ca[first + j], pt))[c] for j in range(4)) % P for c in range(4))
    A, B, U, W = (at(cm[c], z) for c in range(4))
    Z, Zn, S, Sn = ext_at(0, z), ext_at(0, gz), ext_at(4, z), ext_at(4, gz)
    e0 = E.sub(E.mul(Zn, E.add(gamma, B)), E.mul(Z, E.add(gamma, A)))
    e1 = E.sub(E.mul(E.sub(Sn, S), E.add(gamma, W)), U)
    zh_inv, x1_inv = E.inverse(E.sub(E.power(z, n), E.ONE)), E.inverse(E.sub(z, E.ONE))
    q_model = E.add(E.mul(E.add(E.mul(alphas[0], e0), E.mul(alphas[1], e1)), zh_inv),
                    E.mul(E.add(E.mul(alphas[2], E.sub(Z, E.ONE)), E.mul(alphas[3], S)), x1_inv))
    return coeffs, tot[:, :4], q_dev, q_model


def test_two_stages_of_a_proof_under_an_ext_gamma(ta, dev):
    n, log_b = 1 << 8, 2
    rng = np.random.default_rng(900)
    rand_ext = lambda: tuple(int(v) for v in rng.integers(1, P, 4))
    gamma, z, alphas = rand_ext(), rand_ext(), [rand_ext() for _ in range(4)]
    a = [int(v) for v in rng.integers(0, P, n)]
    b = [a[j] for j in rng.permutation(n)]
    # the lookup in one pair of columns: rows 0 .. n/2 - 1 look values up (+1 / (gamma + v)), rows n/2 .. n - 1 hold the table with its
    # multiplicities (-m / (gamma + t)); the sum closes exactly when every looked-up value is in the table as often as it says
    t = [int(v) for v in np.unique(rng.integers(0, P, 4 * n))[:n // 2]]
    picks = rng.integers(0, n // 8, n // 2)
    m = np.bincount(picks, minlength=n // 2)
    u = [1] * (n // 2) + [int(-c % P) for c in m]
    w = [t[j] for j in picks] + t
    small, big = ta.NttContext(n), ta.NttContext(n << log_b)
    try:
        coeffs, totals, q_dev, q_model = staged_proof_tail(ta, dev, small, big, n, log_b, [a, b, u, w], gamma, alphas, z)
        assert tuple(totals[0]) == E.ONE and tuple(totals[1]) == E.ZERO, "a true permutation and a true lookup: both totals equal init"
        assert not coeffs[:, n - 1:].any(), "every constraint has degree 2 (n - 1): the quotient's is n - 2"
        assert coeffs[:, :n - 1].any(axis=1).all() and q_dev == q_model
        dev.free()
        wrong_b = list(b)
        wrong_b[n // 3] = (wrong_b[n // 3] + 1) % P
        coeffs, totals, q_dev, q_model = staged_proof_tail(ta, dev, small, big, n, log_b, [a, wrong_b, u, w], gamma, alphas, z)
        assert tuple(totals[0]) != E.ONE and tuple(totals[1]) == E.ZERO and coeffs[:, -1].any(), "one changed cell: the product is open"
        dev.free()
        wrong_u = list(u)
        wrong_u[n // 2 + int(picks[0])] = (wrong_u[n // 2 + int(picks[0])] + 1) % P
        coeffs, totals, _, _ = staged_proof_tail(ta, dev, small, big, n, log_b, [a, b, wrong_u, w], gamma, alphas, z)
        assert tuple(totals[0]) == E.ONE and tuple(totals[1]) != E.ZERO and coeffs[:, -1].any(), "one changed multiplicity: the sum is open"
    finally:
        small.destroy()
        big.destroy()
