"""prover.AirBuilder: expressions -> a constraint program.  Its output passes toyni_air_program_check and, interpreted by the numpy
model of the instruction set (tests/air_model.py, nothing from the library), equals direct big-integer evaluation of the same
expressions at random points; shared subexpressions are computed once; 65 live registers are refused."""
import numpy as np
import pytest

from air_model import ADD, CELL, EMIT, MUL, P, XINV, air_model, coset_points


@pytest.fixture(scope="module")
def prover():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd.prover


def test_compiled_program_equals_direct_evaluation(prover):
    N, log_b, shift = 64, 2, 7
    B = 1 << log_b
    rng = np.random.default_rng(5)
    mats = [rng.integers(0, P, (3, N), dtype=np.uint64), rng.integers(0, P, (2, N), dtype=np.uint64)]
    weights = [int(v) for v in rng.integers(0, P, 3)]
    b = prover.AirBuilder()
    a0, a1, c2 = b.cell(0, 0, 0), b.cell(0, 0, 1), b.cell(0, 2, 5)
    d1 = b.cell(1, 1, 15)
    t = (a1 - a0 * c2 - 1) * (b.x() - 3)
    b.emit(0, t + 2 * d1 - (5 - a0))
    b.emit(1, (a0 - 11) * b.xinv(9), divide=False)
    b.emit(0, t * t, divide=False)
    b.emit(2, P + 4)                                                  # an int alone: a constant (reduced mod p)
    insns = b.compile()
    info = prover.air_program_check(insns)
    assert info.nconstraints == 3 and info.nmatrices == 2 and list(info.min_width) == [3, 2, 0, 0] and info.max_rotation == 15
    got_c, got_q = air_model(insns, mats, N, log_b, shift, weights)
    xs = [int(v) for v in coset_points(N, shift)]
    for i in range(N):
        cell = lambda m, c, r: int(mats[m][c][(i + r * B) % N])
        x = xs[i]
        tv = (cell(0, 0, 1) - cell(0, 0, 0) * cell(0, 2, 5) - 1) * (x - 3)
        e0 = tv + 2 * cell(1, 1, 15) - (5 - cell(0, 0, 0))
        e1 = (cell(0, 0, 0) - 11) * pow(x - 9, P - 2, P)
        c = (weights[0] * e0 + weights[2] * 4) % P
        q = (c * pow(pow(x, N // B, P) - 1, P - 2, P) + weights[1] * e1 + weights[0] * tv * tv) % P
        assert got_c[i] == c and got_q[i] == q, i


def test_shared_subexpressions_are_computed_once(prover):
    b = prover.AirBuilder()
    s1 = b.cell(0, 1, 2) * b.cell(0, 3, 0) + b.x()
    s2 = b.cell(0, 1, 2) * b.cell(0, 3, 0) + b.x()                    # built a second time
    assert s1 is s2
    b.emit(0, s1 * s2 + s1)
    b.emit(1, s2 * b.xinv(4) + b.xinv(4), divide=False)
    insns = b.compile()
    ops = [i[0] for i in insns]
    assert ops.count(CELL) == 2 and ops.count(XINV) == 1 and ops.count(EMIT) == 2
    assert ops.count(MUL) == 3 and ops.count(ADD) == 3                # c*c', s*s, s*xinv; +x, +s, +xinv
    assert prover.air_program_check(insns).nregs <= 4


def test_registers_are_reused_after_the_last_use(prover):
    b = prover.AirBuilder()
    acc = b.cell(0, 0, 0)
    for k in range(1, 500):                                           # a long chain of values used once needs three registers, not 500
        acc = acc * b.cell(0, k, k % 3) + k
    b.emit(0, acc)
    info = prover.air_program_check(b.compile())
    assert info.nregs <= 4 and info.ninsns > 1000


def test_sixty_five_live_registers_are_refused(prover):
    def balanced(b, leaves):
        # every leaf stays live to the end: after the sum, each is used once more
        total = leaves[0]
        for leaf in leaves[1:]:
            total = total + leaf
        for leaf in leaves:
            total = total * leaf
        return total

    b = prover.AirBuilder()
    b.emit(0, balanced(b, [b.cell(0, c, 0) for c in range(63)]))      # 63 leaves + the running value = 64 live: fits
    assert prover.air_program_check(b.compile()).nregs == 64
    b = prover.AirBuilder()
    b.emit(0, balanced(b, [b.cell(0, c, 0) for c in range(65)]))
    with pytest.raises(ValueError):
        b.compile()
