"""Ext = F_p[X]/(X^4 - 11) on Python integers (src/ext.rs:178-192 the product, :122-128 the inverse a^(p^4 - 2)), and a model of the
two calls of include/toyni_hip.h 3h built on it.  A helper of the tests, not a test; imports nothing from the library.

An element is a tuple of four canonical residues (c0, c1, c2, c3).  The bulk forms take and return numpy arrays whose last axis is
the four coordinates."""
import numpy as np

P = 2013265921
W = 11
GEN_2_27 = 440564289
ZERO, ONE = (0, 0, 0, 0), (1, 0, 0, 0)


def embed(v):
    return (int(v) % P, 0, 0, 0)


def add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def sub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def neg(a):
    return tuple(-x % P for x in a)


def mul(a, b):
    r0 = a[0] * b[0] + W * (a[1] * b[3] + a[2] * b[2] + a[3] * b[1])
    r1 = a[0] * b[1] + a[1] * b[0] + W * (a[2] * b[3] + a[3] * b[2])
    r2 = a[0] * b[2] + a[1] * b[1] + a[2] * b[0] + W * (a[3] * b[3])
    r3 = a[0] * b[3] + a[1] * b[2] + a[2] * b[1] + a[3] * b[0]
    return (r0 % P, r1 % P, r2 % P, r3 % P)


def power(a, e):
    r = ONE
    while e:
        if e & 1:
            r = mul(r, a)
        a = mul(a, a)
        e >>= 1
    return r


def inverse(a):
    assert any(a), "Cannot invert zero"
    return power(a, P ** 4 - 2)


def batch_inverse(elems):
    """The inverses of a list of elements behind one `inverse` (prefix products); a zero element gives zero."""
    pre, acc = [], ONE
    for e in elems:
        pre.append(acc)
        if any(e):
            acc = mul(acc, e)
    inv = inverse(acc)
    out = [ZERO] * len(elems)
    for k in range(len(elems) - 1, -1, -1):
        if any(elems[k]):
            out[k] = mul(inv, pre[k])
            inv = mul(inv, elems[k])
    return out


def vmul(a, b):
    """Element-wise product of arrays (..., 4) of canonical residues (uint64), broadcasting."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    p, w = np.uint64(P), np.uint64(W)
    m = lambda i, j: a[..., i] * b[..., j] % p
    r0 = (m(0, 0) + w * ((m(1, 3) + m(2, 2) + m(3, 1)) % p)) % p
    r1 = (m(0, 1) + m(1, 0) + w * ((m(2, 3) + m(3, 2)) % p)) % p
    r2 = (m(0, 2) + m(1, 1) + m(2, 0) + w * m(3, 3)) % p
    r3 = (m(0, 3) + m(1, 2) + m(2, 1) + m(3, 0)) % p
    return np.stack([r0, r1, r2, r3], axis=-1)


def coset_points(n, shift):
    w = pow(GEN_2_27, (1 << 27) // n, P)
    xs, x = [], shift % P
    for _ in range(n):
        xs.append(x)
        x = x * w % P
    return xs


def poly_eval_ext(coeffs, point):
    """sum_i coeffs[i] * point^i by Horner: base coefficients, an Ext point."""
    acc = ZERO
    for c in reversed([int(v) for v in coeffs]):
        acc = mul(acc, point)
        acc = ((acc[0] + c) % P,) + acc[1:]
    return acc


def poly_eval_ext_batch_model(columns, points):
    """columns: (batch, ncoeffs); points: list of Ext points -> (batch, npoints, 4) uint32, the layout of the device call."""
    out = np.zeros((len(columns), len(points), 4), dtype=np.uint32)
    for b, col in enumerate(columns):
        for p, pt in enumerate(points):
            out[b, p] = poly_eval_ext(col, tuple(int(v) for v in pt))
    return out


def deep_denominators(n, shift, z):
    """(n, 4) uint64: 1 / (x_i - z) on the coset, 0 where x_i = z."""
    z = tuple(int(v) for v in z)
    return np.array(batch_inverse([sub(embed(x), z) for x in coset_points(n, shift)]), dtype=np.uint64)


def deep_ext_model(m, terms, blowup, shift, z, inv=None):
    """m: (width, N) canonical residues; terms: (column, rotation, alpha4, value4); z: Ext.  -> (N, 4) uint32:
    d_i = sum_t alpha_t (M(column_t, i + rotation_t * blowup) - value_t) / (x_i - z), and 0 where x_i = z.  inv: deep_denominators(N,
    shift, z) when the caller has them already (several matrices over one z)."""
    m = np.asarray(m, dtype=np.uint64)
    n = m.shape[1]
    p = np.uint64(P)
    num = np.zeros((n, 4), dtype=np.uint64)
    for c, rot, alpha, value in terms:
        diff = np.zeros((n, 4), dtype=np.uint64)
        diff[:, 0] = np.roll(m[c], -(rot * blowup) % n)
        diff = (diff + np.array(neg(tuple(int(v) for v in value)), dtype=np.uint64)) % p
        num = (num + vmul(diff, np.array([int(v) for v in alpha], dtype=np.uint64))) % p
    if inv is None:
        inv = deep_denominators(n, shift, z)
    return vmul(num, inv).astype(np.uint32)
