"""Constraint programs evaluated into the quotient codeword on the device (include/toyni_hip.h 3f):
  1. the 13-instruction Fibonacci program equals toyni_fib_quotient_device and oracle.fib_quotient word for word (c and q)
  2. random programs against the numpy model of the instruction set (tests/air_model.py, nothing from the library), and once more
     at every launch shape the sizing rule can pick: 256 / 128 / 64 threads x where 1 / Z_H comes from
  3. the pipeline property: the quotient of a true two-column trace is a polynomial of degree < n
  4. guard bands around every matrix and both outputs, two fillings, same outputs
  5. every refusal of the header, the outputs untouched
  6. a call whose weights ride in the kernel arguments, captured into a graph and replayed"""
import ctypes

import numpy as np
import pytest

import oracle
from air_model import CELL, CONST, EMIT, GEN_2_27, P, X, XINV, air_launch_shape, air_model, coset_points, fib_program, random_program
from guarded import DevMem, Guarded

pytestmark = pytest.mark.gpu

E_NULL, E_ZERO_INVERSE, E_RANGE = 10002, 10005, 10006
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


def rand_field(rng, *shape):
    return rng.integers(0, P, shape, dtype=np.uint64)


def layout(m, stride, fill=0xFFFFFFF0):
    """(width, N) values -> the words of a column-major matrix with `stride` words per column; the tails hold a value >= p."""
    width, n = m.shape
    words = np.full(width * stride, fill, dtype=np.uint32)
    for c in range(width):
        words[c * stride:c * stride + n] = m[c]
    return words[: (width - 1) * stride + n]


# ---- 1. Fibonacci anchor ----
@pytest.mark.parametrize("log_n", [1, 2, 3, 6, 12, 16])
def test_fibonacci_program_equals_fib_quotient_and_the_oracle(ta, dev, log_n):
    N = 1 << log_n
    ctx = ta.NttContext(N)
    try:
        for log_b in (0, 1, 3, 5):
            if log_b >= log_n:                                     # a trace of at least two rows
                continue
            rows = N >> log_b                                      # rotation 2 of a two-row trace is its row 0
            rng = np.random.default_rng(300 * log_n + log_b)
            trace = rand_field(rng, N)
            shift = 7
            d_t, d_c, d_q, d_cref, d_qref = dev.up(trace), dev.alloc(N), dev.alloc(N), dev.alloc(N), dev.alloc(N)
            with ta.prover.AirProgram(ctx, fib_program(rows)) as prog:
                assert prog.info.ninsns == 13 and prog.info.nregs == 3 and prog.info.max_rotation == max(1 % rows, 2 % rows)
                ta.prover.air_quotient_device(ctx, prog, [(d_t, 1, N)], log_b, shift, [1], d_q, d_c_out=d_c)
                ta.prover.fib_quotient_device(ctx, d_t, d_cref, d_qref, log_b, shift)
                c, q, cref, qref = dev.down(d_c, N), dev.down(d_q, N), dev.down(d_cref, N), dev.down(d_qref, N)
            want_c, want_q = oracle.fib_quotient(trace, rows, shift)
            assert (c == cref).all() and (q == qref).all(), (log_n, log_b)
            assert (c == want_c.astype(np.uint32)).all() and (q == want_q.astype(np.uint32)).all(), (log_n, log_b)
            dev.free()
    finally:
        ctx.destroy()


# ---- 2. general programs ----
# log_N, log_blowup, matrices, registers, program length (2: one CELL, one EMIT), weights, byte offset, shift 1 with an XINV on the coset
GENERAL = [
    (1, 0, 1, 1, 2, 3, 0, False), (1, 0, 2, 7, 40, 100, 4, False), (1, 1, 1, 7, 40, 3, 8, True), (2, 1, 1, 7, 40, 3, 8, False),
    (2, 0, 4, 64, 40, 100, 12, False), (3, 1, 2, 7, 40, 100, 12, False), (3, 0, 1, 7, 40, 3, 0, True), (6, 2, 4, 64, 3000, 3, 4, False),
    (6, 3, 2, 7, 40, 3, 8, True), (6, 6, 1, 1, 40, 3, 12, False), (12, 3, 4, 7, 3000, 100, 12, False), (12, 9, 1, 1, 2, 3, 0, False),
    (12, 9, 2, 7, 40, 3, 4, False), (12, 0, 2, 64, 40, 100, 0, True), (16, 5, 2, 64, 40, 100, 4, False), (16, 4, 4, 7, 40, 3, 8, False),
    (16, 2, 1, 1, 40, 3, 0, False),
]


def check_random_program(ta, dev, log_N, log_b, nmats, nregs, length, nweights, off, on_coset, seed, divides=True):
    """One random program: the first call, an accumulating second with other weights, a third that leaves c alone -- c and q word for
    word against the numpy model.  divides = False: every constraint is emitted undivided."""
    N = 1 << log_N
    rows = N >> log_b
    rng = np.random.default_rng(seed)
    widths = [[1, 3, 64][(m + log_N) % 3] for m in range(nmats)]
    strides = [N + 20 if m == nmats - 1 and (nmats > 1 or log_N % 2) else N for m in range(nmats)]
    mats = [rand_field(rng, w, N) for w in widths]
    mats[0][0, : min(N, 3)] = [0, 1, P - 1][: min(N, 3)]
    shift = 1 if on_coset else 7                                   # Z_H vanishes on the subgroup itself: nothing is divided there
    point = int(coset_points(N, shift)[N - 1]) if on_coset else int(rng.integers(0, P))
    if length == 2:
        insns = [(CELL, 0, 0, 0, 0), (EMIT, 0, 0, 0, 0)]
    else:
        ncons = 100 if (nweights, length) == (100, 3000) else 3    # 101 EMITs would leave a 40-instruction program no room for anything else
        insns = random_program(rng, nregs, length, widths, rows, ncons, point, may_divide=divides and not on_coset)
        assert len(insns) == max(length, nregs + ncons + 1)
    ops = {i[0] for i in insns}
    assert length == 2 or (ops == set(range(8)) if nregs > 1 else EMIT in ops)
    w1, w2 = ([int(v) for v in rng.integers(0, P, nweights)] for _ in range(2))
    w1[0] = P - 1
    ctx = ta.NttContext(N)
    try:
        d_mats = [(dev.up(layout(m, s), off), w, s) for m, w, s in zip(mats, widths, strides)]
        d_q, d_c = dev.alloc(N, (off + 4) % 16), dev.alloc(N, (off + 8) % 16)
        with ta.prover.AirProgram(ctx, insns) as prog:
            assert prog.info.nregs == (1 if length == 2 else nregs) and prog.info.ninsns == len(insns)
            assert length == 2 or prog.info.divides_by_zh == int(divides and not on_coset)
            ta.prover.air_quotient_device(ctx, prog, d_mats, log_b, shift, w1, d_q, d_c_out=d_c)
            c1, q1 = dev.down(d_c, N), dev.down(d_q, N)
            want_c1, want_q1 = air_model(insns, mats, N, log_b, shift, w1)
            if on_coset and XINV in ops:
                assert int(coset_points(N, shift)[N - 1]) == point   # the inverse at that point is 0: the model's Fermat power agrees
            bad = np.flatnonzero((c1 != want_c1) | (q1 != want_q1))
            assert bad.size == 0, (log_N, log_b, bad[:8])
            # accumulate: a second call with other weights on top, then a third that leaves c alone
            ta.prover.air_quotient_device(ctx, prog, d_mats, log_b, shift, w2, d_q, d_c_out=d_c, accumulate=True)
            ta.prover.air_quotient_device(ctx, prog, d_mats, log_b, shift, w1, d_q, accumulate=True)
            c2, q2 = dev.down(d_c, N), dev.down(d_q, N)
            want_c2, want_q2 = air_model(insns, mats, N, log_b, shift, w2)
            assert (c2 == ((want_c1.astype(np.uint64) + want_c2) % P).astype(np.uint32)).all()
            assert (q2 == ((2 * want_q1.astype(np.uint64) + want_q2) % P).astype(np.uint32)).all()
    finally:
        ctx.destroy()


@pytest.mark.parametrize("log_N,log_b,nmats,nregs,length,nweights,off,on_coset", GENERAL)
def test_random_programs_match_the_numpy_model(ta, dev, log_N, log_b, nmats, nregs, length, nweights, off, on_coset):
    check_random_program(ta, dev, log_N, log_b, nmats, nregs, length, nweights, off, on_coset, seed=9000 + 100 * log_N + 10 * nmats + nregs)


# ---- 2b. every launch shape ----
# air_launch_shape (toyni_amd/csrc/prover_kernels.hpp; restated in tests/air_model.py, held to the emulator's SHAPE lines by
# tests/test_emu_air.py) picks the workgroup from nregs and decides whether 1 / Z_H of the B residue classes sits in LDS behind the
# register file, where `for (t = threadIdx.x; t < B; t += blockDim.x)` fills it.  (nregs, log2 B, some constraint is divided), N = 2^12:
SHAPES = [
    (16, 3, 1),   # last size on 256 threads: 64 KiB of registers, no room for the table
    (17, 3, 1),   # first size on 128 threads
    (31, 8, 1),   # 128 threads, B = 256 > threads: the strided fill
    (32, 8, 1),   # 128 threads, 64 KiB full: per-group inversion
    (32, 3, 0),   # 128 threads, nothing divided
    (33, 7, 1),   # 64 threads, B = 128: the strided fill
    (63, 8, 1),   # 64 threads, 63 KiB + 1 KiB: exactly 64 KiB of dynamic LDS
    (63, 9, 1),   # B > 256: no table
    (64, 2, 1),   # the anchor GENERAL already has: 64 threads, no room
    # the combinations the nine above leave out
    (7, 3, 1), (7, 9, 1), (7, 3, 0),      # 256 threads: table in LDS, B > 256, nothing divided
    (17, 9, 1),                           # 128 threads, B > 256
    (33, 3, 1), (64, 3, 0),               # 64 threads: table in LDS with B <= threads, nothing divided
]
SHAPES_LOG_N = 12


def shape_class(nregs, log_b, divides):
    """(threads, where 1 / Z_H comes from) of a launch."""
    threads, _lds, zh = air_launch_shape(nregs, divides, log_b)
    if zh:
        return threads, "table in LDS, B <= threads" if (1 << log_b) <= threads else "table in LDS, B > threads: strided fill"
    return threads, "no table: nothing divides" if not divides else "no table: B > 256" if log_b > 8 else "no table: no room"


# 3 weights ride in the kernel arguments, 100 come from device memory: two kernels, each compiled with the fill loop of its own
@pytest.mark.parametrize("nweights", [3, 100])
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[f"nregs{r}-logb{b}-div{d}" for r, b, d in SHAPES])
def test_random_programs_match_the_numpy_model_at_every_launch_shape(ta, dev, k, nweights):
    nregs, log_b, divides = SHAPES[k]
    check_random_program(ta, dev, SHAPES_LOG_N, log_b, 2, nregs, 40, nweights, 4 * (k % 4), False, seed=12000 + k, divides=bool(divides))


# SHAPES hits every combination the rule can produce at this N -- 3 workgroup sizes x 5 sources of 1 / Z_H, less the one that cannot
# occur: a 256-thread workgroup never meets B > threads with the table in LDS, because the table is only kept for B <= 256
REACHABLE = {shape_class(r, b, d) for r in range(1, 65) for b in range(SHAPES_LOG_N + 1) for d in (0, 1)}
assert (256, "table in LDS, B > threads: strided fill") not in REACHABLE and len(REACHABLE) == 14
assert {t for t, _ in REACHABLE} == {256, 128, 64}
assert {shape_class(*s) for s in SHAPES} == REACHABLE
assert air_launch_shape(63, 1, 8) == (64, 65536, 1) and air_launch_shape(31, 1, 8) == (128, 64512, 1)     # the exact fit; B = 2 x threads


# the cases above cover what the module's docstring claims
assert {c[0] for c in GENERAL} == {1, 2, 3, 6, 12, 16} and {c[2] for c in GENERAL} == {1, 2, 4} and {c[3] for c in GENERAL} == {1, 7, 64}
assert {c[4] for c in GENERAL} == {2, 40, 3000} and {c[5] for c in GENERAL} == {3, 100} and {c[6] for c in GENERAL} == {0, 4, 8, 12}
assert all({c[5] for c in GENERAL if c[0] == log_N} == {3, 100} for log_N in (1, 12))   # single points and groups of four, both kinds of weights


# ---- 3. the pipeline ----
@pytest.mark.parametrize("n", [8, 64])
def test_quotient_of_a_true_trace_is_a_polynomial_of_degree_below_n(ta, dev, n):
    log_b, shift = 2, 7
    N = n << log_b
    rng = np.random.default_rng(n)
    a, b = [int(rng.integers(0, P))], [int(rng.integers(0, P))]
    for j in range(n - 1):
        a.append(b[j])
        b.append((a[j] * b[j] + 1) % P)
    g = pow(GEN_2_27, (1 << 27) // n, P)
    last = pow(g, n - 1, P)
    bld = ta.prover.AirBuilder()
    ax, bx, agx, bgx = bld.cell(0, 0, 0), bld.cell(0, 1, 0), bld.cell(0, 0, 1), bld.cell(0, 1, 1)
    bld.emit(0, (agx - bx) * (bld.x() - last))
    bld.emit(1, (bgx - ax * bx - 1) * (bld.x() - last))
    bld.emit(2, (ax - a[0]) * bld.xinv(1), divide=False)
    weights = [int(v) for v in rng.integers(1, P, 3)]
    small, big = ta.NttContext(n), ta.NttContext(N)
    try:
        with ta.prover.AirProgram(big, bld.compile()) as prog:
            assert prog.info.nconstraints == 3 and prog.info.divides_by_zh == 1 and prog.info.max_rotation == 1
            d_coef, d_lde, d_q, d_poly = dev.alloc(2 * n), dev.alloc(2 * N), dev.alloc(N), dev.alloc(N)

            def tail_of_quotient(cols):
                d_vals = dev.up(np.array(cols, dtype=np.uint32).reshape(-1))
                small.run_device(d_vals, d_coef, 2, True)                      # batched inverse transform: coefficients
                big.lde_device(d_coef, d_lde, 2, log_b, shift)                  # batched LDE, column-major, col_stride = N
                ta.prover.air_quotient_device(big, prog, [(d_lde, 2, N)], log_b, shift, weights, d_q)
                big.run_device(d_q, d_poly, 1, True, shift=shift)               # inverse coset transform
                return dev.down(d_poly, N)[n:]

            assert (tail_of_quotient([a, b]) == 0).all(), "the quotient of a true trace has degree < n"
            wrong = list(b)
            wrong[n // 2] = (wrong[n // 2] + 1) % P                            # one cell off: Z_H no longer divides the numerator
            assert tail_of_quotient([a, wrong]).any()
    finally:
        small.destroy()
        big.destroy()


# ---- 4. guard bands ----
@pytest.mark.parametrize("log_N,off", [(1, 4), (3, 12), (12, 0)])
def test_air_quotient_between_guard_bands(ta, log_N, off):
    N = 1 << log_N
    rng = np.random.default_rng(70 + log_N)
    widths, strides = [3, 1], [N + 20, N]
    mats = [rand_field(rng, w, N) for w in widths]
    insns = random_program(rng, 7, 40, widths, N, 3, int(rng.integers(0, P)))
    weights = [int(v) for v in rng.integers(0, P, 3)]
    ctx = ta.NttContext(N)
    results = []
    try:
        with ta.prover.AirProgram(ctx, insns) as prog:
            for pattern in ("sentinel", "random"):
                words = [layout(m, s, 0xA5A5A5A5) if pattern == "sentinel" else layout(m, s, int(rng.integers(0, 1 << 32))) for m, s in zip(mats, strides)]
                gm = [Guarded(ta, w.nbytes, offset=(off + 4 * k) % 16, seed=1 + k) for k, w in enumerate(words)]
                gc, gq = Guarded(ta, 4 * N, offset=(off + 8) % 16, seed=5), Guarded(ta, 4 * N, offset=(off + 12) % 16, seed=6)
                try:
                    for g_, w in zip(gm, words):
                        g_.refill(pattern)
                        g_.upload(w)
                    ta.prover.air_quotient_device(ctx, prog, [(g_.ptr, w, s) for g_, w, s in zip(gm, widths, strides)], 0, 7, weights, gq.ptr, d_c_out=gc.ptr)
                    gq.mem.sync()
                    for k, (g_, w) in enumerate(zip(gm, words)):
                        g_.check(f"matrix {k}")
                        assert (g_.download() == w).all(), "a matrix was changed"
                    gc.check("d_c_out"), gq.check("d_q_out")
                    results.append((gc.download(), gq.download()))
                finally:
                    for g_ in gm + [gc, gq]:
                        g_.free(check=False)
        want_c, want_q = air_model(insns, mats, N, 0, 7, weights)
        for c, q in results:
            assert (c == want_c).all() and (q == want_q).all()
    finally:
        ctx.destroy()


# ---- 5. refusals ----
def test_every_refusal_leaves_the_outputs_untouched(ta, dev):
    lib = ta._lib.lib
    N, lb = 64, 2
    ctx = ta.NttContext(N)
    progs = []
    try:
        d_m, d_c, d_q = dev.up(np.arange(3 * N) % P), dev.alloc(N), dev.alloc(N)
        dev.fill(d_c, N), dev.fill(d_q, N)
        M = ta.prover.AirMatrix
        make = lambda insns: progs.append(ta.prover.AirProgram(ctx, insns)) or progs[-1]
        # matrix 0 is not read, matrix 1 up to column 2 and rotation 15 (= N / B - 1), constraints 0 and 1, one of them divided
        prog = make([(CELL, 0, 15, 1, 2), (X, 1, 0, 0, 0), (EMIT, 0, 0, 0, 0), (EMIT, 0, 1, 1, 1)])
        far = make([(CELL, 0, 16, 1, 2), (EMIT, 0, 0, 1, 0)])                   # rotation N / B
        two = (M * 2)(M(None, 0, 0), M(d_m, 3, N))
        w2 = (ctypes.c_uint32 * 2)(5, 6)

        def run(handle=ctx.handle, p=prog, mats=two, nmats=2, log_b=lb, shift=7, w=w2, nw=2, c=d_c, q=d_q, acc=0):
            return lib.toyni_air_quotient_device(handle, p.handle if p else None, mats, nmats, log_b, shift, w, nw, c, q, acc, None)

        assert run(handle=None) == E_NULL and run(p=None) == E_NULL and run(mats=None) == E_NULL and run(w=None) == E_NULL and run(q=None) == E_NULL
        five = (M * 5)(*[M(d_m, 3, N)] * 5)
        big_w = (ctypes.c_uint32 * 65537)()
        cases = {
            "nmats < nmatrices": run(nmats=1), "nmats > 4": run(mats=five, nmats=5),
            "null d_values": run(mats=(M * 2)(M(None, 0, 0), M(None, 3, N))), "width < min_width": run(mats=(M * 2)(M(None, 0, 0), M(d_m, 2, N))),
            "width > 65536": run(mats=(M * 2)(M(None, 0, 0), M(d_m, 65537, N))), "col_stride < N": run(mats=(M * 2)(M(None, 0, 0), M(d_m, 3, N - 1))),
            "max_rotation >= N / B": run(p=far), "log_blowup > log2 N": run(log_b=7), "shift 0": run(shift=0), "shift p": run(shift=P),
            "nweights < nconstraints": run(nw=1), "nweights > 65536": run(w=big_w, nw=65537), "weight p": run(w=(ctypes.c_uint32 * 2)(5, P)),
            "matrix misaligned": run(mats=(M * 2)(M(None, 0, 0), M(d_m + 2, 3, N))), "d_c_out misaligned": run(c=d_c + 1), "d_q_out misaligned": run(q=d_q + 2),
        }
        assert all(rc == E_RANGE for rc in cases.values()), cases
        assert run(shift=1) == E_ZERO_INVERSE                                  # Z_H vanishes on the subgroup and constraint 0 is divided
        assert (dev.down(d_c, N) == SENTINEL_WORD).all() and (dev.down(d_q, N) == SENTINEL_WORD).all()
        # what sits next to the refusals is accepted: the largest rotation, the unread matrix left null, no c, weights to spare
        assert run(c=None, w=(ctypes.c_uint32 * 3)(5, 6, P - 1), nw=3) == 0
        undivided = make([(CELL, 0, 0, 0, 0), (EMIT, 0, 0, 1, 0)])
        assert run(p=undivided, mats=(M * 1)(M(d_m, 1, N)), nmats=1, shift=1, c=None) == 0    # nothing divided: shift 1 is fine
        dev.mem.sync()
    finally:
        for p in progs:
            p.destroy()
        ctx.destroy()


def test_a_program_created_on_another_device_is_refused(ta, dev):
    lib = ta._lib.lib
    ndev = ctypes.c_int(0)
    assert lib.toyni_device_count(ctypes.byref(ndev)) == 0
    if ndev.value < 2:
        pytest.skip("needs two devices")
    N = 64
    ctx, other = ta.NttContext(N), ta.NttContext(N, device=1)
    try:
        d_q = dev.alloc(N)
        dev.fill(d_q, N)
        w = (ctypes.c_uint32 * 1)(1)
        with ta.prover.AirProgram(other, [(X, 0, 0, 0, 0), (EMIT, 0, 0, 1, 0)]) as foreign:
            assert lib.toyni_air_quotient_device(ctx.handle, foreign.handle, None, 0, 2, 7, w, 1, None, d_q, 0, None) == E_RANGE
        assert (dev.down(d_q, N) == SENTINEL_WORD).all()
    finally:
        ctx.destroy()
        other.destroy()


# ---- 6. graph capture ----
def test_a_call_with_inline_weights_can_be_captured_and_replayed(ta):
    import torch
    tdev = torch.device("cuda", 0)
    N, log_b = 1 << 12, 3
    rng = np.random.default_rng(66)
    insns = random_program(rng, 7, 40, [3], N >> log_b, 3, int(rng.integers(0, P)))
    weights = [int(v) for v in rng.integers(0, P, 64)]                         # the most that ride in the kernel arguments
    ctx = ta.NttContext(N)
    try:
        with ta.prover.AirProgram(ctx, insns) as prog:
            buf = torch.zeros(3 * N, dtype=torch.int32, device=tdev)
            q, c = torch.empty(N, dtype=torch.int32, device=tdev), torch.empty(N, dtype=torch.int32, device=tdev)
            s = torch.cuda.Stream(device=tdev)
            call = lambda: ta.prover.air_quotient_device(ctx, prog, [(buf.data_ptr(), 3, N)], log_b, 7, weights, q.data_ptr(), d_c_out=c.data_ptr(),
                                                         stream=s.cuda_stream)
            call()                                                              # eager, warm
            ctx.synchronize(s.cuda_stream)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):                                 # one kernel node: a single-branch graph
                call()
            for rep in range(2):
                m = rand_field(rng, 3, N)
                buf.copy_(torch.from_numpy(m.astype(np.uint32).view(np.int32).reshape(-1)))
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                got_c, got_q = c.cpu().numpy().view(np.uint32).copy(), q.cpu().numpy().view(np.uint32).copy()
                call()                                                          # the eager call on the same contents
                torch.cuda.synchronize()
                assert (got_c == c.cpu().numpy().view(np.uint32)).all() and (got_q == q.cpu().numpy().view(np.uint32)).all()
                want_c, want_q = air_model(insns, [m], N, log_b, 7, weights)
                assert (got_c == want_c).all() and (got_q == want_q).all(), rep
            del g
    finally:
        ctx.destroy()
