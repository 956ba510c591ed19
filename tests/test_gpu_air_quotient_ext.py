"""The AIR quotient under Ext weights in one device call (include/toyni_hip.h 3k).  By definition column e of its output is, word for
word, what toyni_air_quotient_device writes under the base weights weights4[4 k + e]; the arithmetic is exact, so every comparison
here is equality -- with four air_quotient_device calls on the same device buffers and, up to N = 4096, with the numpy model of the
base instruction set (tests/air_model.py) run per coordinate.

  1. CASES: N = 1, 2, 4, 8; several workgroups at 256 and at 64 threads; every source of 1 / Z_H (class table in LDS, per-thread
     inversion for B = 512, no room beside 64 registers, nothing divided); output columns 16-byte aligned, out_stride = N + 1, the base
     pointer one word off, a matrix one word off, rotation 1 with B = 2; accumulate on and off; c written or not; the weights inside
     the kernel arguments (up to the limit) and one above it (the second kernel); saturated operands.  Matrices and outputs lie
     between guard bands (tests/guarded.py): nothing outside the 4 x N output words changes, the words N .. out_stride included.
  2. every refusal of the header leaves the outputs untouched
  3. a call at the inline limit captured into a graph (a single kernel node) and replayed
  4. the staged AIR of tests/harness/air_ext_prover.py: one call under air_ext_weights(alphas) gives the 4 x N matrix and the
     row-commitment root of the harness's four calls"""
import ctypes

import numpy as np
import pytest

from air_model import CELL, EMIT, MUL, P, SUB, X, air_launch_shape, air_model, random_program
from guarded import DevMem, Guarded

pytestmark = pytest.mark.gpu

E_NULL, E_ZERO_INVERSE, E_RANGE = 10002, 10005, 10006
SENTINEL_WORD = 0xA5A5A5A5
SAT_X = 1069547521                       # the plain value whose Montgomery form is p - 1
MODEL_MAX_N = 4096


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


def layout(m, stride, fill=SENTINEL_WORD):
    """(width, N) values -> the words of a column-major matrix with `stride` words per column; the tails hold a value >= p."""
    width, n = m.shape
    words = np.full((width - 1) * stride + n, fill, dtype=np.uint32)
    for c in range(width):
        words[c * stride:c * stride + n] = m[c]
    return words


def columns_of(words, stride, n):
    return np.stack([words[e * stride:e * stride + n] for e in range(4)])


def gaps_of(words, stride, n):
    return np.concatenate([words[e * stride + n:(e + 1) * stride] for e in range(3)])


# rotation 1 with B = 2: the next row's cell lies two words on, never a 16-byte load (the program of tests/emu/emu_air_ext.cpp)
ROT1 = [(CELL, 0, 0, 0, 0), (CELL, 1, 1, 0, 0), (CELL, 2, 1, 0, 1), (MUL, 3, 1, 2, 0), (SUB, 3, 3, 0, 0), (EMIT, 0, 3, 0, 0), (EMIT, 0, 1, 1, 1),
        (EMIT, 0, 2, 0, 0)]
# the saturated program of tests/emu: every product is (p - 1)^2
SAT = [(CELL, 0, 0, 0, 0), (1, 1, 0, 0, SAT_X), (MUL, 2, 0, 1, 0), (CELL, 0, 1, 0, 1), (MUL, 3, 2, 0, 0), (EMIT, 0, 2, 1, 0), (EMIT, 0, 3, 0, 1),
       (EMIT, 0, 3, 0, 0)]

# name -> log_N, log_b, nregs, nweights, and what differs from: something divided, out_stride = N, aligned pointers, no accumulation,
# c written, a random program of 40 instructions
CASES = {
    "N=1": dict(log_N=0, log_b=0, nregs=3, nweights=3),
    "N=2": dict(log_N=1, log_b=1, nregs=7, nweights=3, pad=1),
    "N=2 accumulate, no c": dict(log_N=1, log_b=0, nregs=7, nweights=3, acc=True, with_c=False),
    "N=4": dict(log_N=2, log_b=1, nregs=7, nweights=3, pad=1, acc=True),
    "N=8": dict(log_N=3, log_b=2, nregs=7, nweights=3, out_off=4),
    "N=2048 two workgroups of 256, Z_H table (B=8)": dict(log_N=11, log_b=3, nregs=7, nweights=3),
    "N=4096 sixteen workgroups of 64, no room for the table": dict(log_N=12, log_b=3, nregs=64, nweights=3, pad=1, with_c=False),
    "B=512 n=2 per-thread inversion": dict(log_N=10, log_b=9, nregs=7, nweights=3, acc=True),
    "nothing divided": dict(log_N=8, log_b=3, nregs=7, nweights=3, divides=False, pad=1, acc=True, with_c=False),
    "aligned columns": dict(log_N=8, log_b=2, nregs=17, nweights=3, pad=4),
    "out_stride N+1 behind an aligned base": dict(log_N=8, log_b=2, nregs=7, nweights=3, pad=1),
    "out_stride N+1, accumulate": dict(log_N=8, log_b=2, nregs=7, nweights=3, pad=1, acc=True),
    "base pointer one word off": dict(log_N=8, log_b=2, nregs=7, nweights=3, out_off=4, acc=True),
    "base pointer one word off, stride N+3": dict(log_N=8, log_b=2, nregs=7, nweights=3, out_off=4, pad=3),
    "matrix one word off": dict(log_N=8, log_b=2, nregs=7, nweights=3, mat_off=4),
    "rotation 1 with B=2": dict(log_N=6, log_b=1, nweights=2, insns=ROT1, widths=[2]),
    "rotation 1 with B=2, N=4": dict(log_N=2, log_b=1, nweights=2, insns=ROT1, widths=[2], pad=1),
    "weights at the inline limit": dict(log_N=8, log_b=3, nregs=7, nweights=64, ncons=64),
    "one weight above the inline limit": dict(log_N=8, log_b=3, nregs=7, nweights=65, ncons=65, pad=1),
    "one above the limit, N=2, accumulate": dict(log_N=1, log_b=0, nregs=7, nweights=65, acc=True),
    "saturated": dict(log_N=6, log_b=2, nweights=2, insns=SAT, widths=[2], saturated=True, shift=SAT_X),
    "saturated, accumulate, B=1": dict(log_N=6, log_b=0, nweights=2, insns=SAT, widths=[2], saturated=True, shift=SAT_X, acc=True, pad=1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_call_equals_four_base_calls_and_the_model(ta, name):
    case = CASES[name]
    log_N, log_b, nweights = case["log_N"], case["log_b"], case["nweights"]
    N, rows = 1 << log_N, (1 << log_N) >> log_b
    pad, out_off, mat_off = case.get("pad", 0), case.get("out_off", 0), case.get("mat_off", 0)
    acc, with_c, sat, shift = case.get("acc", False), case.get("with_c", True), case.get("saturated", False), case.get("shift", 7)
    stride = N + pad
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + log_N)
    widths = case.get("widths", [3, 8])
    mat_strides = [N + 20 if m else N for m in range(len(widths))]
    mats = [np.full((w, N), P - 1, dtype=np.uint64) if sat else rng.integers(0, P, (w, N), dtype=np.uint64) for w in widths]
    insns = case.get("insns") or random_program(rng, case["nregs"], 40, widths, rows, case.get("ncons", 3), int(rng.integers(0, P)),
                                                may_divide=case.get("divides", True))
    weights4 = np.full((nweights, 4), P - 1, dtype=np.uint32) if sat else rng.integers(0, P, (nweights, 4)).astype(np.uint32)
    if not sat:
        weights4[0] = [P - 1, 0, 1, P - 1]
    out_words = 3 * stride + N
    before = np.full(out_words, SENTINEL_WORD, dtype=np.uint32)
    if acc:
        for e in range(4):
            before[e * stride:e * stride + N] = P - 1 if sat else rng.integers(0, P, N)
    ctx = ta.NttContext(N)
    mem = DevMem(ta)
    guards = []
    try:
        gm = [Guarded(ta, 4 * ((w - 1) * s + N), offset=mat_off, seed=1 + k) for k, (w, s) in enumerate(zip(widths, mat_strides))]
        gq, gc = Guarded(ta, 4 * out_words, offset=out_off, seed=8), Guarded(ta, 4 * out_words, offset=out_off, seed=9)
        rq, rc = Guarded(ta, 4 * out_words, seed=10), Guarded(ta, 4 * out_words, seed=11)       # what the four base calls write
        guards = gm + [gq, gc, rq, rc]
        mat_words = [layout(m, s) for m, s in zip(mats, mat_strides)]
        for g_, w in zip(gm, mat_words):
            g_.upload(w)
        for g_ in (gq, gc, rq, rc):
            g_.upload(before)
        d_mats = [(g_.ptr, w, s) for g_, w, s in zip(gm, widths, mat_strides)]
        with ta.prover.AirProgram(ctx, insns) as prog:
            info = prog.info
            ta.air_quotient_ext_device(ctx, prog, d_mats, log_b, shift, weights4, gq.ptr, stride, d_c_out=gc.ptr if with_c else 0, accumulate=acc)
            for e in range(4):
                ta.air_quotient_device(ctx, prog, d_mats, log_b, shift, weights4[:, e], rq.ptr + 4 * e * stride, d_c_out=rc.ptr + 4 * e * stride if with_c else 0,
                                       accumulate=acc)
            mem.sync()
        for k, (g_, w) in enumerate(zip(gm, mat_words)):
            g_.check(f"matrix {k}")
            assert (g_.download() == w).all(), "a matrix was changed"
        for g_, what in ((gq, "d_q_out"), (gc, "d_c_out"), (rq, "base q"), (rc, "base c")):
            g_.check(what)
        q, c, want_q, want_c = gq.download(), gc.download(), rq.download(), rc.download()
        assert (q == want_q).all(), (name, np.flatnonzero(q != want_q)[:8])                      # the gaps included: both still hold the sentinel
        assert (c == want_c).all(), (name, np.flatnonzero(c != want_c)[:8])
        assert (gaps_of(q, stride, N) == SENTINEL_WORD).all() and (gaps_of(c, stride, N) == SENTINEL_WORD).all()
        if not with_c:
            assert (c == before).all(), "a null d_c_out: nothing is written"
        assert (columns_of(q, stride, N) < P).all()
        # which of the two kernels ran: the weights ride in the kernel arguments up to the limit (the launch registry of the library)
        kernel = "air_quotient_ext_inline_kernel" if nweights <= ta.prover.AIR_EXT_INLINE_WEIGHTS else "air_quotient_ext_kernel"
        assert any(kernel in k for k in ta._lib.launched_kernels()), kernel
        # the launch shape the case is named for
        threads, _lds, zh = air_launch_shape(info.nregs, info.divides_by_zh, log_b)
        if "workgroups of 256" in name:
            assert threads == 256 and zh == 1 and N // 4 > threads
        if "workgroups of 64" in name:
            assert threads == 64 and zh == 0 and info.divides_by_zh == 1 and N // 4 > threads
        if "per-thread" in name:
            assert zh == 0 and info.divides_by_zh == 1 and rows == 2
        if "nothing divided" in name:
            assert info.divides_by_zh == 0
        if N <= MODEL_MAX_N:
            p64 = np.uint64(P)
            for e in range(4):
                mc, mq = air_model(insns, mats, N, log_b, shift, [int(v) for v in weights4[:, e]])
                mc, mq = mc.astype(np.uint64), mq.astype(np.uint64)
                if acc:
                    pre = before[e * stride:e * stride + N].astype(np.uint64)
                    mc, mq = (mc + pre) % p64, (mq + pre) % p64
                assert (columns_of(q, stride, N)[e] == mq).all(), (name, e)
                if with_c:
                    assert (columns_of(c, stride, N)[e] == mc).all(), (name, e)
        if sat:
            assert columns_of(q, stride, N).any()
    finally:
        for g_ in guards:
            g_.free(check=False)
        ctx.destroy()


def test_the_cases_cover_what_the_docstring_claims(ta):
    limit = ta.prover.AIR_EXT_INLINE_WEIGHTS
    assert {c["nweights"] for c in CASES.values()} >= {limit, limit + 1}
    assert {c["log_N"] for c in CASES.values()} >= {0, 1, 2, 3}
    assert any(c.get("pad", 0) % 4 and not c.get("out_off") for c in CASES.values()) and any(c.get("out_off") for c in CASES.values())
    assert any(c.get("mat_off") for c in CASES.values())
    for acc in (False, True):
        for with_c in (False, True):
            assert any(c.get("acc", False) == acc and c.get("with_c", True) == with_c for c in CASES.values()), (acc, with_c)


# ---- 2. refusals ----
def test_every_refusal_leaves_the_outputs_untouched(ta):
    lib = ta._lib.lib
    N, lb, stride = 64, 2, 68
    out_words = 3 * stride + N
    ctx = ta.NttContext(N)
    progs, guards = [], []
    try:
        gm, gc, gq = Guarded(ta, 4 * 3 * N, seed=1), Guarded(ta, 4 * out_words, seed=2), Guarded(ta, 4 * out_words, seed=3)
        guards = [gm, gc, gq]
        gm.upload((np.arange(3 * N) % P).astype(np.uint32))
        d_m, d_c, d_q = gm.ptr, gc.ptr, gq.ptr
        M = ta.prover.AirMatrix
        make = lambda insns: progs.append(ta.prover.AirProgram(ctx, insns)) or progs[-1]
        # matrix 0 is not read, matrix 1 up to column 2 and rotation 15 (= N / B - 1), constraints 0 and 1, one of them divided
        prog = make([(CELL, 0, 15, 1, 2), (X, 1, 0, 0, 0), (EMIT, 0, 0, 0, 0), (EMIT, 0, 1, 1, 1)])
        far = make([(CELL, 0, 16, 1, 2), (EMIT, 0, 0, 1, 0)])                   # rotation N / B
        two = (M * 2)(M(None, 0, 0), M(d_m, 3, N))
        w2 = (ctypes.c_uint32 * 8)(5, 6, 7, 8, 9, 10, 11, 12)

        def run(handle=ctx.handle, p=prog, mats=two, nmats=2, log_b=lb, shift=7, w=w2, nw=2, c=d_c, q=d_q, os_=stride, acc=0):
            return lib.toyni_air_quotient_ext_device(handle, p.handle if p else None, mats, nmats, log_b, shift, w, nw, c, q, os_, acc, None)

        assert run(handle=None) == E_NULL and run(p=None) == E_NULL and run(mats=None) == E_NULL and run(w=None) == E_NULL and run(q=None) == E_NULL
        five = (M * 5)(*[M(d_m, 3, N)] * 5)
        big_w = (ctypes.c_uint32 * (4 * 65537))()
        bad_coordinate = lambda k: (ctypes.c_uint32 * 8)(*[P if i == k else 5 for i in range(8)])
        cases = {
            "nmats < nmatrices": run(nmats=1), "nmats > 4": run(mats=five, nmats=5),
            "null d_values": run(mats=(M * 2)(M(None, 0, 0), M(None, 3, N))), "width < min_width": run(mats=(M * 2)(M(None, 0, 0), M(d_m, 2, N))),
            "width > 65536": run(mats=(M * 2)(M(None, 0, 0), M(d_m, 65537, N))), "col_stride < N": run(mats=(M * 2)(M(None, 0, 0), M(d_m, 3, N - 1))),
            "max_rotation >= N / B": run(p=far), "log_blowup > log2 N": run(log_b=7), "shift 0": run(shift=0), "shift p": run(shift=P),
            "nweights < nconstraints": run(nw=1), "nweights > 65536": run(w=big_w, nw=65537),
            "coordinate 0 of weight 0 = p": run(w=bad_coordinate(0)), "coordinate 3 of weight 0 = p": run(w=bad_coordinate(3)),
            "coordinate 3 of weight 1 = p": run(w=bad_coordinate(7)),
            "out_stride < N": run(os_=N - 1), "out_stride 0": run(os_=0),
            "matrix misaligned": run(mats=(M * 2)(M(None, 0, 0), M(d_m + 2, 3, N))), "d_c_out misaligned": run(c=d_c + 1), "d_q_out misaligned": run(q=d_q + 2),
        }
        assert all(rc == E_RANGE for rc in cases.values()), cases
        assert run(shift=1) == E_ZERO_INVERSE                                  # Z_H vanishes on the subgroup and constraint 0 is divided
        gq.mem.sync()
        for g_, what in ((gc, "d_c_out"), (gq, "d_q_out")):
            g_.check(what)
            assert (g_.download() == SENTINEL_WORD).all(), what + " was written by a refused call"
        # what sits next to the refusals is accepted: out_stride = N, no c, weights to spare, p - 1 in every coordinate
        spare = (ctypes.c_uint32 * 12)(*[P - 1] * 12)
        assert run(c=None, w=spare, nw=3, os_=N) == 0
        undivided = make([(CELL, 0, 0, 0, 0), (EMIT, 0, 0, 1, 0)])
        assert run(p=undivided, mats=(M * 1)(M(d_m, 1, N)), nmats=1, shift=1, c=None) == 0    # nothing divided: shift 1 is fine
        gq.mem.sync()
        gq.check("d_q_out"), gc.check("d_c_out")
        assert (gc.download() == SENTINEL_WORD).all()
    finally:
        for p in progs:
            p.destroy()
        for g_ in guards:
            g_.free(check=False)
        ctx.destroy()


# ---- 3. graph capture ----
def test_a_call_at_the_inline_limit_can_be_captured_and_replayed(ta):
    import torch
    tdev = torch.device("cuda", 0)
    N, log_b = 1 << 12, 3
    rng = np.random.default_rng(67)
    insns = random_program(rng, 7, 40, [3], N >> log_b, 3, int(rng.integers(0, P)))
    limit = ta.prover.AIR_EXT_INLINE_WEIGHTS
    weights4 = rng.integers(0, P, (limit, 4)).astype(np.uint32)                 # the most that ride in the kernel arguments
    ctx = ta.NttContext(N)
    try:
        with ta.prover.AirProgram(ctx, insns) as prog:
            buf = torch.zeros(3 * N, dtype=torch.int32, device=tdev)
            q, c = torch.empty(4 * N, dtype=torch.int32, device=tdev), torch.empty(4 * N, dtype=torch.int32, device=tdev)
            s = torch.cuda.Stream(device=tdev)
            call = lambda: ta.air_quotient_ext_device(ctx, prog, [(buf.data_ptr(), 3, N)], log_b, 7, weights4, q.data_ptr(), N, d_c_out=c.data_ptr(),
                                                      stream=s.cuda_stream)
            call()                                                              # eager, warm
            ctx.synchronize(s.cuda_stream)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):                                 # one kernel node: a single-branch graph
                call()
            for rep in range(2):
                m = rng.integers(0, P, (3, N), dtype=np.uint64)
                buf.copy_(torch.from_numpy(m.astype(np.uint32).view(np.int32).reshape(-1)))
                q.fill_(-1), c.fill_(-1)
                torch.cuda.synchronize()
                g.replay()
                torch.cuda.synchronize()
                got_c, got_q = c.cpu().numpy().view(np.uint32).copy(), q.cpu().numpy().view(np.uint32).copy()
                call()                                                          # the eager call on the same contents
                torch.cuda.synchronize()
                assert (got_c == c.cpu().numpy().view(np.uint32)).all() and (got_q == q.cpu().numpy().view(np.uint32)).all()
                for e in range(4):
                    want_c, want_q = air_model(insns, [m], N, log_b, 7, [int(v) for v in weights4[:, e]])
                    assert (got_c[e * N:(e + 1) * N] == want_c).all() and (got_q[e * N:(e + 1) * N] == want_q).all(), (rep, e)
            del g
    finally:
        ctx.destroy()


# ---- 4. the staged AIR ----
def test_the_staged_air_quotient_in_one_call_equals_the_harness_four(ta):
    """Steps 1-3 of tests/harness/air_ext_prover.py on random main columns (n = 16, B = 4): everything downstream in the proof is a
    function of the 4 x N quotient matrix and its commitment, so the matrix and the root are what is compared."""
    import torch
    import ext_model as em
    from harness import air_ext_prover as hp
    from harness.air_ext_verifier import ACC_WIDTH, MAIN_WIDTH, NUM_WEIGHTS, Q_WIDTH
    from harness.fib_verifier import COSET_SHIFT
    pv, lib = ta.prover, ta._lib.lib
    n, log_blowup = 16, 2
    N = n << log_blowup
    rng = np.random.default_rng(0x57A6ED)
    tdev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    words = lambda count: torch.empty(count, dtype=torch.int32, device=tdev)
    ext = lambda: tuple(int(v) for v in rng.integers(0, P, 4))
    main = rng.integers(0, P, (MAIN_WIDTH, n), dtype=np.uint64)
    gamma, alphas = ext(), [ext() for _ in range(NUM_WEIGHTS)]
    ctx_n, ctx_N = ta.ntt.get_or_create_ctx(n), ta.ntt.get_or_create_ctx(N)

    def lde_of(d_columns, width):
        coef, lde = words(width * n), words(width * N)
        ctx_n.run_device(d_columns, coef.data_ptr(), width, True, stream=stream)
        ctx_N.lde_device(coef.data_ptr(), lde.data_ptr(), width, log_blowup, COSET_SHIFT, stream=stream)
        return lde

    vals = torch.from_numpy(main.astype(np.uint32).view(np.int32).reshape(-1)).to(tdev)
    main_lde = lde_of(vals.data_ptr(), MAIN_WIDTH)
    col = lambda c: vals.data_ptr() + 4 * c * n
    acc = words(ACC_WIDTH * n)
    pv.column_scan_ext_device(ctx_n, pv.ExtOperand(col(0), n, 1, gamma), pv.ExtOperand(col(1), n, 1, gamma), acc.data_ptr(), n, n, 1, pv.SCAN_PRODUCT,
                              [em.ONE], stream=stream)
    pv.column_scan_ext_device(ctx_n, pv.ExtOperand(col(2), n, 1, em.ZERO), pv.ExtOperand(col(3), n, 1, gamma), acc.data_ptr() + 16 * n, n, n, 1,
                              pv.SCAN_SUM, [em.ZERO], stream=stream)
    acc_lde = lde_of(acc.data_ptr(), ACC_WIDTH)
    mats = [(main_lde.data_ptr(), MAIN_WIDTH, N), (acc_lde.data_ptr(), ACC_WIDTH, N)]
    salts = torch.from_numpy(rng.integers(0, 256, (N, 16), dtype=np.uint8)).to(tdev)

    def root_of(q):
        levels = torch.empty((lib.toyni_merkle_total_digests(N), 32), dtype=torch.uint8, device=tdev)
        ta.merkle_commit_rows_device(q.data_ptr(), N, Q_WIDTH, ta.ROWS_COLUMN_MAJOR, N, salts.data_ptr(), levels.data_ptr(), stream=stream)
        return bytes(levels[-1].cpu().numpy().tobytes())

    four, one = words(Q_WIDTH * N), words(Q_WIDTH * N)
    four.fill_(-1), one.fill_(-1)
    with pv.AirProgram(ctx_N, hp.constraint_program(gamma)) as prog:
        assert prog.info.nconstraints == 4 * NUM_WEIGHTS == 16
        for e, wts in enumerate(hp.coordinate_weights(alphas)):                 # step 3 of the harness, as it stands
            pv.air_quotient_device(ctx_N, prog, mats, log_blowup, COSET_SHIFT, wts, four.data_ptr() + 4 * e * N, stream=stream)
        ta.air_quotient_ext_device(ctx_N, prog, mats, log_blowup, COSET_SHIFT, ta.air_ext_weights(alphas), one.data_ptr(), N, stream=stream)
        root_four, root_one = root_of(four), root_of(one)
    got, want = one.cpu().numpy().view(np.uint32), four.cpu().numpy().view(np.uint32)
    assert (want < P).all() and want.any()
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    assert root_one == root_four
