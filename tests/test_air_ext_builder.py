"""prover.AirBuilder's Ext helper (include/toyni_hip.h 3i): Ext expressions as four base-field expressions, so that the constraints
tying an Ext accumulator to the trace compile to ordinary programs.  Programs built with it, interpreted by the numpy model of the
instruction set (tests/air_model.py, nothing from the library), equal tests/ext_model.py arithmetic coordinate by coordinate at every
point; a program that uses none of the helper compiles to exactly the instructions the builder gave before the helper existed."""
import numpy as np
import pytest

import ext_model as E
from air_model import P, air_model, coset_points


@pytest.fixture(scope="module")
def prover():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd.prover


def _coordinates(insns, mats, N, log_b, shift, nconstraints):
    """value_k(i) of every constraint number k: one model run per one-hot weight vector -> (c, q), each (nconstraints, N)."""
    cs, qs = [], []
    for k in range(nconstraints):
        w = [1 if j == k else 0 for j in range(nconstraints)]
        c, q = air_model(insns, mats, N, log_b, shift, w)
        cs.append([int(v) for v in c]), qs.append([int(v) for v in q])
    return cs, qs


def test_ext_programs_equal_ext_model_arithmetic(prover):
    N, log_b, shift = 32, 1, 7
    B = 1 << log_b
    rng = np.random.default_rng(11)
    mats = [rng.integers(0, P, (3, N), dtype=np.uint64), rng.integers(0, P, (9, N), dtype=np.uint64)]
    gamma, delta = tuple(int(v) for v in rng.integers(1, P, 4)), tuple(int(v) for v in rng.integers(1, P, 4))
    b = prover.AirBuilder()
    z, z_next = b.ext_cell(1, 0, 0), b.ext_cell(1, 0, 1)               # an Ext accumulator in columns 0..3 of matrix 1
    s, s_next = b.ext_cell(1, 5, 0), b.ext_cell(1, 5, 2)               # another in columns 5..8
    g = b.ext_const(gamma)
    a0, a1, m = b.cell(0, 0), b.cell(0, 1), b.cell(0, 2, 1)
    b.emit_ext(0, z_next * (g + a1) - z * (g + a0))                    # permutation transition: Ext x (Ext + base)
    b.emit_ext(1, (s_next - s) * (g + a0) - m)                         # LogUp transition: an Ext minus a base expression
    b.emit_ext(2, (z - 1) * b.xinv(9) + (3 - s) * 2, divide=False)     # boundaries: int on either side, Ext x base, undivided
    b.emit_ext(3, z * s * b.ext_const(delta) + a0 * z + 5 + s)         # Ext x Ext x Ext; base x Ext; + int; Ext x base from the left
    b.emit(16, a0 * a1)                                                # base-field constraints mix in
    b.emit_ext(5, b.ext(a1) - b.ext(4) + (g - z))                      # embeddings, Ext - Ext
    insns = b.compile()
    info = prover.air_program_check(insns)
    assert info.nconstraints == 24 and info.nmatrices == 2 and list(info.min_width) == [3, 9, 0, 0] and info.max_rotation == 2
    cs, qs = _coordinates(insns, mats, N, log_b, shift, 24)
    xs = [int(v) for v in coset_points(N, shift)]
    for i in range(N):
        cell = lambda mt, c, r=0: int(mats[mt][c][(i + r * B) % N])
        ext = lambda c0, r=0: tuple(cell(1, c0 + k, r) for k in range(4))
        zh_inv = pow(pow(xs[i], N // B, P) - 1, P - 2, P)
        ga0, ga1 = E.add(gamma, E.embed(cell(0, 0))), E.add(gamma, E.embed(cell(0, 1)))
        want = {
            0: E.sub(E.mul(ext(0, 1), ga1), E.mul(ext(0), ga0)),
            1: E.sub(E.mul(E.sub(ext(5, 2), ext(5)), ga0), E.embed(cell(0, 2, 1))),
            3: E.add(E.add(E.add(E.mul(E.mul(ext(0), ext(5)), delta), E.mul(E.embed(cell(0, 0)), ext(0))), E.embed(5)), ext(5)),
            5: E.add(E.sub(E.embed(cell(0, 1)), E.embed(4)), E.sub(gamma, ext(0))),
        }
        for k, w in want.items():
            for j in range(4):
                assert cs[4 * k + j][i] == w[j] and qs[4 * k + j][i] == w[j] * zh_inv % P, (k, j, i)
        w2 = E.add(E.mul(E.sub(ext(0), E.ONE), E.embed(pow(xs[i] - 9, P - 2, P))), E.mul(E.sub(E.embed(3), ext(5)), E.embed(2)))
        for j in range(4):
            assert cs[8 + j][i] == 0 and qs[8 + j][i] == w2[j], (2, j, i)
        assert cs[16][i] == cell(0, 0) * cell(0, 1) % P
        for k in (17, 18, 19):
            assert cs[k][i] == 0 and qs[k][i] == 0


def test_ext_products_fold_through_x4_equals_11(prover):
    """X * X^3 = 11: the product of two constants, compiled and run, against ext_model.mul -- and the shared subexpressions of the four
    coordinates are computed once."""
    b = prover.AirBuilder()
    u, v = b.ext_cell(0, 0), b.ext_cell(0, 4)
    b.emit_ext(0, u * v, divide=False)
    insns = b.compile()
    assert sum(1 for i in insns if i[0] == prover.AIR_CELL) == 8 and sum(1 for i in insns if i[0] == prover.AIR_MUL) == 16 + 3
    N = 8
    rng = np.random.default_rng(3)
    mat = rng.integers(0, P, (8, N), dtype=np.uint64)
    mat[:, 0] = [0, 1, 0, 0, 0, 0, 0, 1]                               # X * X^3
    _, qs = _coordinates(insns, [mat], N, 0, 1, 4)
    assert [qs[j][0] for j in range(4)] == [11, 0, 0, 0]
    for i in range(N):
        assert tuple(qs[j][i] for j in range(4)) == E.mul(tuple(int(x) for x in mat[:4, i]), tuple(int(x) for x in mat[4:, i]))


def test_a_program_without_the_helper_compiles_as_before(prover):
    b = prover.AirBuilder()
    assert all(hasattr(b, name) for name in ("ext_cell", "ext_const", "ext", "emit_ext"))   # the helper is there, and stays unused below
    a0, a1, a2 = b.cell(0, 0, 0), b.cell(0, 0, 1), b.cell(0, 0, 2)
    t = (a2 - (a1 + a0)) * (b.x() - 5)
    b.emit(0, t * (b.x() - 7))
    b.emit(1, (a0 - 3) * b.xinv(9) + t, divide=False)
    b.emit(2, 2 * b.cell(1, 3, 4) + t * t)
    # what the builder gave for these lines before the Ext helper was added, instruction for instruction
    assert b.compile() == [
        (0, 0, 2, 0, 0), (0, 1, 1, 0, 0), (0, 2, 0, 0, 0), (4, 1, 1, 2, 0), (5, 1, 0, 1, 0), (2, 0, 0, 0, 0), (1, 3, 0, 0, 5), (5, 3, 0, 3, 0),
        (6, 3, 1, 3, 0), (1, 1, 0, 0, 7), (5, 1, 0, 1, 0), (6, 1, 3, 1, 0), (7, 0, 1, 0, 0), (1, 1, 0, 0, 3), (5, 1, 2, 1, 0), (3, 2, 0, 0, 9),
        (6, 2, 1, 2, 0), (4, 2, 2, 3, 0), (7, 0, 2, 1, 1), (1, 2, 0, 0, 2), (0, 1, 4, 1, 3), (6, 1, 2, 1, 0), (6, 3, 3, 3, 0), (4, 3, 1, 3, 0),
        (7, 0, 3, 0, 2)]
