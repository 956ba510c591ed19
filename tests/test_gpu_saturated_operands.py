"""Saturated operands through the ABI: every data word p - 1 and every caller-supplied constant 1069547521, the plain value whose
Montgomery form is p - 1 (tests/guarded.py names it mont=p-1), so that every product a kernel forms between data and a constant is
(p - 1)^2 -- the bound the comments of toyni_amd/csrc/bb_field.hpp claim for mont_dot2, mont_dot_sub and the four-product groups of
mont_reduce_wide, which scattered edge values among random data never reach in every factor at once.  The smallest shapes that take
every loop form; expected values from Python integers (tests/air_model.py, tests/ext_model.py) or the oracle, exact.  Every buffer is
guard-banded (tests/rows_common.py Dev: the guards are checked when a case ends).  tests/test_field_contracts.py runs the same
cases on the CPU under operand-domain checks."""
import numpy as np
import pytest

import ext_model as E
import oracle
import rows_common as rc
from air_model import CELL, CONST, EMIT, MUL, P, air_model, deep_model

pytestmark = pytest.mark.gpu

SAT_X = 1069547521            # SAT_X * 2^32 = p - 1 (mod p)
SAT_X2 = 125829121            # its neighbour: Montgomery form p - 2
assert SAT_X * (1 << 32) % P == P - 1 and SAT_X2 * (1 << 32) % P == P - 2
TOP = P - 1
SAT4 = (SAT_X,) * 4


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


@pytest.fixture(scope="module")
def ctx64(ta):
    c = ta.NttContext(64)
    yield c
    c.destroy()


def words(g, count=None):
    g.mem.sync()
    return g.download(count=count)


# ---- DEEP combinations: 2^6 points, blow-up 4, width 8; whole groups of four, a remainder, the inline table (<= 64) and the staged one
N, LOG_B, WIDTH = 64, 2, 8
MATRIX = np.full((WIDTH, N), TOP, dtype=np.uint64)


@pytest.mark.parametrize("nterms", [3, 4, 5, 8, 64, 65])
def test_deep_combine_saturated(ta, ctx64, nterms):
    terms = [(t % WIDTH, t % 2, SAT_X, SAT_X) for t in range(nterms)]                    # rotations 0 and 1
    want = deep_model(MATRIX, terms, 1 << LOG_B, SAT_X, SAT_X2)
    table = ta.prover.deep_terms(*zip(*terms))
    with rc.Dev(ta) as d:
        g_m, g_out = d.put(MATRIX.astype(np.uint32)), d.put(np.full(N, TOP, dtype=np.uint32))
        ta.prover.deep_combine_device(ctx64, g_m.ptr, WIDTH, N, LOG_B, SAT_X, SAT_X2, table, g_out.ptr)
        assert (words(g_out) == want).all(), nterms
        g_out.upload(np.full(N, TOP, dtype=np.uint32))
        ta.prover.deep_combine_device(ctx64, g_m.ptr, WIDTH, N, LOG_B, SAT_X, SAT_X2, table, g_out.ptr, accumulate=True)
        assert (words(g_out) == (want.astype(np.uint64) + TOP) % P).all(), nterms
    assert want.any()


@pytest.mark.parametrize("nterms", [3, 4, 5, 8, 64, 65])
def test_deep_combine_ext_saturated(ta, ctx64, nterms):
    terms = [(t % WIDTH, t % 2, SAT4, SAT4) for t in range(nterms)]
    want = E.deep_ext_model(MATRIX, terms, 1 << LOG_B, SAT_X, SAT4)
    table = ta.prover.deep_ext_terms(*zip(*terms))
    with rc.Dev(ta) as d:
        g_m, g_out = d.put(MATRIX.astype(np.uint32)), d.put(np.full(4 * N, TOP, dtype=np.uint32))
        ta.prover.deep_combine_ext_device(ctx64, g_m.ptr, WIDTH, N, LOG_B, SAT_X, SAT4, table, g_out.ptr)
        assert (words(g_out).reshape(N, 4) == want).all(), nterms
        g_out.upload(np.full(4 * N, TOP, dtype=np.uint32))
        ta.prover.deep_combine_ext_device(ctx64, g_m.ptr, WIDTH, N, LOG_B, SAT_X, SAT4, table, g_out.ptr, accumulate=True)
        assert (words(g_out).reshape(N, 4) == (want.astype(np.uint64) + TOP) % P).all(), nterms
    assert want.any()


# ---- batched evaluation: below one thread's share + 1, and one chunk + 1
@pytest.mark.parametrize("ncoeffs", [17, 4097])
def test_poly_eval_batches_saturated(ta, ctx64, ncoeffs):
    batch, stride = 3, ncoeffs + 3
    points = [SAT_X, TOP]
    coeffs = np.full(batch * stride, 0xFFFFFFF0, dtype=np.uint32)                         # the slack: >= p, never read
    for b in range(batch):
        coeffs[b * stride:b * stride + ncoeffs] = TOP
    coeffs = coeffs[: (batch - 1) * stride + ncoeffs]
    base_want = [oracle.poly_eval(np.full(ncoeffs, TOP, dtype=np.uint64), pt) for pt in points]
    ext_points = [SAT4, (TOP,) * 4]
    ext_want = E.poly_eval_ext_batch_model([[TOP] * ncoeffs], ext_points)[0]
    with rc.Dev(ta) as d:
        g_c, g_out, g_ext = d.put(coeffs), d.buf(4 * batch * 2), d.buf(16 * batch * 2)
        ta.prover.poly_eval_batch_device(ctx64, g_c.ptr, ncoeffs, stride, batch, points, g_out.ptr)
        ta.prover.poly_eval_ext_batch_device(ctx64, g_c.ptr, ncoeffs, stride, batch, ext_points, g_ext.ptr)
        got, got_ext = words(g_out).reshape(batch, 2), words(g_ext).reshape(batch, 2, 4)
        for b in range(batch):
            assert list(got[b]) == base_want, (ncoeffs, b)
            assert (got_ext[b] == ext_want).all(), (ncoeffs, b)


# ---- a constraint program: cell * CONST SAT_X, that times the next row's cell, emitted under weight SAT_X (divided and undivided)
def test_air_quotient_saturated(ta, ctx64):
    insns = [(CELL, 0, 0, 0, 0), (CONST, 1, 0, 0, SAT_X), (MUL, 2, 0, 1, 0), (CELL, 0, 1, 0, 1), (MUL, 3, 2, 0, 0),
             (EMIT, 0, 2, 1, 0), (EMIT, 0, 3, 0, 1), (EMIT, 0, 3, 0, 0)]
    m = np.full((2, N), TOP, dtype=np.uint64)
    weights = [SAT_X, SAT_X]
    want_c, want_q = air_model(insns, [m], N, LOG_B, SAT_X, weights)
    assert want_c.any() and want_q.any()
    with rc.Dev(ta) as d, ta.prover.AirProgram(ctx64, insns) as prog:
        g_m, g_q, g_c = d.put(m.astype(np.uint32)), d.buf(4 * N), d.buf(4 * N)
        ta.prover.air_quotient_device(ctx64, prog, [(g_m.ptr, 2, N)], LOG_B, SAT_X, weights, g_q.ptr, d_c_out=g_c.ptr)
        assert (words(g_c) == want_c).all() and (words(g_q) == want_q).all()
        ta.prover.air_quotient_device(ctx64, prog, [(g_m.ptr, 2, N)], LOG_B, SAT_X, weights, g_q.ptr, d_c_out=g_c.ptr, accumulate=True)
        assert (words(g_c) == 2 * want_c.astype(np.uint64) % P).all() and (words(g_q) == 2 * want_q.astype(np.uint64) % P).all()


# ---- the Ext fold, alone and with the folded layer's commitment: beta = (SAT_X, SAT_X, SAT_X, SAT_X), the points from x0 = SAT_X
@pytest.mark.parametrize("m", [8, 1 << 10])
def test_ext_folds_saturated(ta, m):
    half = m // 2
    e = np.full((m, 4), TOP, dtype=np.uint64)
    e[half::2] = 0                                       # a - b = p - 1 at the even points, 0 at the odd ones
    want = oracle.fri_fold_ext(e, oracle.domain_elements(m, SAT_X), np.array(SAT4, dtype=np.uint64))
    levels = rc.hashlib_levels(rc.leaves_of(np.asarray(want, dtype=np.uint64).reshape(-1, 4), None))
    levels_want = np.frombuffer(b"".join(dg for level in levels for dg in level), dtype=np.uint8).reshape(-1, 32)
    ndig = int(ta._lib.lib.toyni_merkle_total_digests(half))
    assert levels_want.shape[0] == ndig
    ctx = ta.NttContext(m)
    try:
        with rc.Dev(ta) as d:
            g_e, g_out, g_out2, g_lv = d.put(e.astype(np.uint32)), d.buf(16 * half), d.buf(16 * half), d.buf(32 * ndig, word=1)
            ta.fri_fold_ext_device(ctx, g_e.ptr, g_out.ptr, m, SAT4, SAT_X)
            ta.prover.fri_fold_commit_ext_device(ctx, g_e.ptr, g_out2.ptr, m, SAT4, SAT_X, 0, g_lv.ptr)
            assert (words(g_out).reshape(half, 4) == want).all()
            assert (words(g_out2).reshape(half, 4) == want).all()
            assert (words(g_lv).reshape(ndig, 32) == levels_want).all()
    finally:
        ctx.destroy()


# ---- accumulator columns under gamma = (SAT_X, SAT_X, SAT_X, SAT_X): one element past a tile
@pytest.mark.parametrize("op", [0, 1], ids=["sum", "product"])
def test_column_scan_ext_saturated(ta, ctx64, op):
    n = ta.prover.column_scan_ext_tile() + 1
    num, den = E.add((TOP,) * 4, SAT4), E.add(E.embed(TOP), SAT4)                       # a width-4 numerator, a width-1 denominator
    term = E.mul(num, E.inverse(den))
    acc, want = SAT4, []
    for _ in range(n):
        want.append(acc)
        acc = E.mul(acc, term) if op else E.add(acc, term)
    want = np.array(want, dtype=np.uint32)
    with rc.Dev(ta) as d:
        g_num, g_den = d.put(np.full(4 * n, TOP, dtype=np.uint32)), d.put(np.full(n, TOP, dtype=np.uint32))
        g_out, g_tot = d.buf(16 * n), d.buf(32)
        ta.prover.column_scan_ext_device(ctx64, ta.prover.ExtOperand(g_num.ptr, n, 4, SAT4), ta.prover.ExtOperand(g_den.ptr, n, 1, SAT4), g_out.ptr, n, n,
                                         1, op, [SAT4], g_tot.ptr)
        assert (words(g_out).reshape(4, n).T == want).all()
        assert list(words(g_tot)) == list(acc) + [0, 0, 0, 0]


# ---- transforms: every word p - 1, and alternating 0 / p - 1; plain, the coset of SAT_X, and the LDE by 4 onto it
@pytest.mark.parametrize("log_n", [6, 12, 16])
def test_transforms_saturated(ta, log_n):
    n, log_b = 1 << log_n, 2
    vecs = np.full((2, n), TOP, dtype=np.uint64)
    vecs[1, 0::2] = 0
    compact = vecs[:, : n >> log_b]
    ctx = ta.NttContext(n)
    try:
        with rc.Dev(ta) as d:
            g_in, g_c, g_out = d.put(vecs.astype(np.uint32)), d.put(np.ascontiguousarray(compact).astype(np.uint32)), d.buf(8 * n)
            for inverse in (False, True):
                ctx.run_device(g_in.ptr, g_out.ptr, 2, inverse)
                got = words(g_out).reshape(2, n)
                for b in range(2):
                    assert (got[b] == (oracle.intt(vecs[b]) if inverse else oracle.ntt(vecs[b]))).all(), (log_n, inverse, b)
                ctx.run_device(g_in.ptr, g_out.ptr, 2, inverse, shift=SAT_X)
                got = words(g_out).reshape(2, n)
                for b in range(2):
                    assert (got[b] == (oracle.domain_ifft(vecs[b], SAT_X) if inverse else oracle.domain_fft(vecs[b], n, SAT_X))).all(), (log_n, inverse, b)
            ctx.lde_device(g_c.ptr, g_out.ptr, 2, log_b, SAT_X)
            got = words(g_out).reshape(2, n)
            for b in range(2):
                assert (got[b] == oracle.domain_fft(compact[b], n, SAT_X)).all(), (log_n, b)
            assert (words(g_in).reshape(2, n) == vecs).all()
    finally:
        ctx.destroy()
