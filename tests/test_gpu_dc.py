"""The two calls of include/toyni_hip.h 3p -- the quotient with its parameters and weights in device memory, the Ext accumulators with
gamma in device memory -- against the host-argument calls they are defined by.  Everything is exact, so every comparison is equality.

  1. Quotient: each call against toyni_air_quotient_ext_device on the program with every PARAM j replaced by CONST (params[j] mod p)
     (the substitution is made HERE: the PARAM program is derived from the CONST program of tests/air_model.py, whose model is not
     touched) under the host-expanded weights of the reduced alphas, and up to N = 4096 against the numpy model per coordinate.  The
     shapes are those of tests/test_gpu_air_quotient_ext.py's CASES that select different code; both weight forms with 1, 16 and 17
     alphas (4 x 16 weights is the old inline limit); 0, 1, 4 and 256 parameters; parameter and alpha words >= p (0xFFFFFFFF, p,
     p + 1 among them); the saturated program.  Everything lies between guard bands (tests/guarded.py).
  2. Scan: each call against toyni_column_scan_ext_device under the reduced shifts: n = 1, 5, tile, tile + 1, 3 tile + 7; batch 1 and
     17; both ops; the operand forms 1/1 (one index), 1 (no shift)/1, 4/4, 0/1, 4/0; a column one word off; in place; a gamma in the base
     field that makes one width-1 denominator zero (counted); shift words >= p; d_totals null and not.
  3. every refusal leaves the outputs untouched
  4. each call captured into a graph (a linear chain), the challenge words OVERWRITTEN, the graph replayed: the result is that of the
     host-argument call under the new values -- the values are read at run time
  5. each call twice, and on a second stream of the same context"""
import ctypes

import numpy as np
import pytest

from air_model import CELL, CONST, EMIT, P, X, air_model, random_program
from guarded import DevMem, Guarded
from test_gpu_air_quotient_ext import CASES, SENTINEL_WORD, columns_of, gaps_of, layout

pytestmark = pytest.mark.gpu

E_NULL, E_ZERO_INVERSE, E_RANGE = 10002, 10005, 10006
PARAM = 8
EXT, EMIT_EXT = 0, 1
NONE = 0xFFFFFFFF
MODEL_MAX_N = 4096
EDGE_WORDS = [0xFFFFFFFF, P, P + 1, 0]


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


def parametrise(insns, nparams, rng):
    """-> (the program with its first CONSTs turned into PARAMs, the nparams raw words).  The first CONST becomes parameter
    nparams - 1, the next ones 0, 1, ...; a parameter's word is the constant plus p (so it needs the reduction), the words no PARAM
    names are any u32.  Substituting CONST (word mod p) back gives `insns`."""
    words = rng.integers(0, 1 << 32, nparams, dtype=np.uint64)
    if nparams >= 4:
        words[1:4] = EDGE_WORDS[:3]
    order = [nparams - 1] + list(range(nparams - 1))
    out, used = [], 0
    for op, dst, a, b, imm in insns:
        if op == CONST and used < nparams:
            j = order[used]
            used += 1
            words[j] = imm + P                                       # < 2^32 for every canonical imm
            out.append((PARAM, dst, 0, 0, j))
        else:
            out.append((op, dst, a, b, imm))
    return out, words.astype(np.uint32), used


def raw_alphas(rng, nalphas, saturated=False):
    """nalphas x 4 raw u32 words, most of them >= p; saturated: every word reduces to p - 1"""
    if saturated:
        return np.full((nalphas, 4), 2 * P - 1, dtype=np.uint32)
    al = rng.integers(0, 1 << 32, (nalphas, 4), dtype=np.uint64).astype(np.uint32)
    al[0] = EDGE_WORDS
    return al


def host_weights(ta, alphas_raw, form):
    red = (alphas_raw.astype(np.uint64) % P).astype(np.uint32)
    return red if form == EXT else ta.air_ext_weights([tuple(int(c) for c in a) for a in red])


# case of tests/test_gpu_air_quotient_ext.py -> nparams, nalphas, form, constraints (None: the case's own)
DC_CASES = {
    "N=1": (0, 1, EMIT_EXT, None),
    "N=2": (1, 16, EXT, None),
    "N=2 accumulate, no c": (4, 17, EXT, 17),
    "N=4": (256, 1, EMIT_EXT, 4),
    "N=8": (1, 17, EMIT_EXT, 68),
    "N=2048 two workgroups of 256, Z_H table (B=8)": (4, 16, EMIT_EXT, 64),
    "N=4096 sixteen workgroups of 64, no room for the table": (256, 16, EXT, 16),
    "B=512 n=2 per-thread inversion": (1, 1, EMIT_EXT, None),
    "nothing divided": (0, 17, EXT, None),
    "aligned columns": (0, 1, EXT, 1),
    "out_stride N+1 behind an aligned base": (4, 16, EXT, None),
    "out_stride N+1, accumulate": (1, 1, EMIT_EXT, None),
    "base pointer one word off": (256, 17, EMIT_EXT, None),
    "matrix one word off": (4, 16, EMIT_EXT, None),
    "rotation 1 with B=2": (1, 1, EMIT_EXT, None),                   # (a program without a PARAM under a spare parameter)
    "saturated": (1, 1, EMIT_EXT, None),
    "saturated, accumulate, B=1": (4, 16, EXT, None),
}


def test_the_cases_cover_what_the_docstring_claims():
    assert {c[0] for c in DC_CASES.values()} == {0, 1, 4, 256}
    assert {(c[1], c[2]) for c in DC_CASES.values()} == {(k, f) for k in (1, 16, 17) for f in (EXT, EMIT_EXT)}
    cs = [CASES[k] for k in DC_CASES]
    assert {c["log_N"] for c in cs} >= {0, 1, 2, 3, 11, 12} and any(c.get("nregs") == 64 for c in cs) and any(c["log_b"] == 9 for c in cs)
    assert any(c.get("divides", True) is False for c in cs) and any(c.get("mat_off") for c in cs) and any(c.get("out_off") for c in cs)
    assert any(c.get("pad", 0) % 4 for c in cs) and any(c.get("insns") for c in cs) and any(c.get("saturated") for c in cs)
    for acc in (False, True):
        assert any(c.get("acc", False) == acc for c in cs)
    assert any(c.get("with_c", True) is False for c in cs)


@pytest.mark.parametrize("name", list(DC_CASES))
def test_quotient_equals_the_host_argument_call_on_the_substituted_program_and_the_model(ta, name):
    case = CASES[name]
    nparams, nalphas, form, ncons = DC_CASES[name]
    log_N, log_b = case["log_N"], case["log_b"]
    N, rows = 1 << log_N, (1 << log_N) >> log_b
    pad, out_off, mat_off = case.get("pad", 0), case.get("out_off", 0), case.get("mat_off", 0)
    acc, with_c, sat, shift = case.get("acc", False), case.get("with_c", True), case.get("saturated", False), case.get("shift", 7)
    stride = N + pad
    rng = np.random.default_rng(sum(map(ord, name)) * 7907 + log_N)
    widths = case.get("widths", [3, 8])
    mat_strides = [N + 20 if m else N for m in range(len(widths))]
    mats = [np.full((w, N), P - 1, dtype=np.uint64) if sat else rng.integers(0, P, (w, N), dtype=np.uint64) for w in widths]
    const_insns = case.get("insns") or random_program(rng, case["nregs"], 40, widths, rows, ncons or case.get("ncons", 3), int(rng.integers(0, P)),
                                                      may_divide=case.get("divides", True))
    param_insns, params_raw, used = parametrise(const_insns, nparams, rng)
    alphas_raw = raw_alphas(rng, nalphas, sat)
    weights4 = host_weights(ta, alphas_raw, form)
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
        rq, rc = Guarded(ta, 4 * out_words, offset=out_off, seed=10), Guarded(ta, 4 * out_words, offset=out_off, seed=11)   # the host-argument call
        gp, ga = Guarded(ta, 4 * max(nparams, 1), offset=4, seed=12), Guarded(ta, 16 * nalphas, offset=4, seed=13)          # one word off
        guards = gm + [gq, gc, rq, rc, gp, ga]
        mat_words = [layout(m, s) for m, s in zip(mats, mat_strides)]
        for g_, w in zip(gm, mat_words):
            g_.upload(w)
        for g_ in (gq, gc, rq, rc):
            g_.upload(before)
        gp.upload(params_raw), ga.upload(alphas_raw)
        d_mats = [(g_.ptr, w, s) for g_, w, s in zip(gm, widths, mat_strides)]
        with ta.prover.AirProgram(ctx, param_insns, params=True) as prog, ta.prover.AirProgram(ctx, const_insns) as ref:
            info = prog.info
            assert prog.nparams == (nparams if used else 0) and bytes(info) == bytes(ref.info)
            ta.prover.air_quotient_ext_dc_device(ctx, prog, d_mats, log_b, shift, gp.ptr if nparams else 0, nparams, ga.ptr, nalphas, form, gq.ptr, stride,
                                                 d_c_out=gc.ptr if with_c else 0, accumulate=acc)
            ta.air_quotient_ext_device(ctx, ref, d_mats, log_b, shift, weights4, rq.ptr, stride, d_c_out=rc.ptr if with_c else 0, accumulate=acc)
            mem.sync()
        for k, (g_, w) in enumerate(zip(gm, mat_words)):
            g_.check(f"matrix {k}")
            assert (g_.download() == w).all(), "a matrix was changed"
        for g_, what in ((gq, "d_q_out"), (gc, "d_c_out"), (rq, "host-argument q"), (rc, "host-argument c"), (gp, "d_params"), (ga, "d_alphas")):
            g_.check(what)
        assert (gp.download()[:nparams] == params_raw).all() and (ga.download().reshape(-1, 4) == alphas_raw).all(), "an input was changed"
        q, c, want_q, want_c = gq.download(), gc.download(), rq.download(), rc.download()
        assert (q == want_q).all(), (name, np.flatnonzero(q != want_q)[:8])                      # the gaps included: both still hold the sentinel
        assert (c == want_c).all(), (name, np.flatnonzero(c != want_c)[:8])
        assert (gaps_of(q, stride, N) == SENTINEL_WORD).all() and (gaps_of(c, stride, N) == SENTINEL_WORD).all()
        if not with_c:
            assert (c == before).all(), "a null d_c_out: nothing is written"
        assert (columns_of(q, stride, N) < P).all()
        launched = ta._lib.launched_kernels()
        assert any("air_dc_prepare_kernel" in k for k in launched) and any("air_quotient_ext_dc_kernel" in k for k in launched)
        if N <= MODEL_MAX_N:
            p64 = np.uint64(P)
            for e in range(4):
                mc, mq = air_model(const_insns, mats, N, log_b, shift, [int(v) for v in weights4[:, e]])
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


# ---- 2. the scan ----
FORMS = {            # name -> (num width, num index, den width, den index); index None: TOYNI_EXT_SHIFT_NONE
    "1/1 one index": (1, 0, 1, 0),
    "1 (no shift)/1": (1, None, 1, 0),
    "4/4": (4, 1, 4, 0),
    "0/1": (0, None, 1, 2),                # challenge 2 lies in the base field and makes one denominator zero
    "4/0": (4, 0, 0, None),
}


def scan_sizes(ta):
    tile = ta.prover.column_scan_ext_tile()
    return [1, 5, tile, tile + 1, 3 * tile + 7]


def operand_words(rng, width, n, batch, stride):
    """the words of an operand of `batch` columns (width base columns each) `stride` apart; the tails hold a value >= p"""
    cols = width * batch
    words = np.full((cols - 1) * stride + n, SENTINEL_WORD, dtype=np.uint32)
    for c in range(cols):
        words[c * stride:c * stride + n] = rng.integers(0, P, n)
    return words


@pytest.mark.parametrize("form", list(FORMS))
def test_scan_equals_the_host_argument_call_under_the_reduced_shifts(ta, form):
    pv = ta.prover
    nw, ni, dw, di = FORMS[form]
    rng = np.random.default_rng(sum(map(ord, form)) * 104729)
    mem = DevMem(ta)
    ctx = ta.NttContext(1 << 10)           # n is not tied to the context's size
    seen_zero = 0
    try:
        for n in scan_sizes(ta):
            for batch in (1, 17):
                stride = n + (3 if batch == 17 else 0)               # columns that start one, two, three words off
                off = 4 if n in (5, scan_sizes(ta)[3]) else 0        # ... and a column one word off behind an aligned stride
                hit = min(3, n - 1)
                num_w = operand_words(rng, nw, n, batch, stride) if nw else None
                den_w = operand_words(rng, dw, n, batch, stride) if dw else None
                chal = rng.integers(0, 1 << 32, (3, 4), dtype=np.uint64)
                chal[1] = EDGE_WORDS
                if dw == 1:
                    chal[2] = [(P - int(den_w[hit])) % P + P, P, P, P]                # gamma = p - v_hit in the base field, every word >= p
                shift = lambda i: (0, 0, 0, 0) if i is None else tuple(int(w) % P for w in chal[i])
                out_words = (4 * batch - 1) * stride + n
                guards = []
                try:
                    gn = Guarded(ta, 4 * num_w.size, offset=off, seed=1) if nw else None
                    gd = Guarded(ta, 4 * den_w.size, offset=off, seed=2) if dw else None
                    gch = Guarded(ta, 48, offset=4, seed=3)
                    guards = [g_ for g_ in (gn, gd, gch) if g_]
                    gch.upload(chal.astype(np.uint32))
                    for op in (pv.SCAN_SUM, pv.SCAN_PRODUCT):
                        for with_totals in (True, False):
                            if not with_totals and (batch == 17 or op == pv.SCAN_SUM):
                                continue
                            for in_place in ((False, True) if nw == 4 and batch == 1 else (False,)):
                                if nw:
                                    gn.upload(num_w)
                                if dw:
                                    gd.upload(den_w)
                                init = rng.integers(0, P, (batch, 4)).astype(np.uint32)
                                go, ro = Guarded(ta, 4 * out_words, offset=off, seed=4), Guarded(ta, 4 * out_words, offset=off, seed=5)
                                gt, rt = Guarded(ta, 32 * batch, seed=6), Guarded(ta, 32 * batch, seed=7)
                                guards += [go, ro, gt, rt]
                                # the host-argument call first: an in-place call overwrites the numerator
                                pv.column_scan_ext_device(ctx, pv.ExtOperand(gn.ptr, stride, nw, shift(ni)) if nw else None,
                                                          pv.ExtOperand(gd.ptr, stride, dw, shift(di)) if dw else None, ro.ptr, stride, n, batch, op, init,
                                                          totals=rt.ptr if with_totals else 0)
                                d_out = gn.ptr if in_place else go.ptr
                                pv.column_scan_ext_dc_device(ctx, pv.ExtOperandDc(gn.ptr, stride, nw, NONE if ni is None else ni) if nw else None,
                                                             pv.ExtOperandDc(gd.ptr, stride, dw, NONE if di is None else di) if dw else None, gch.ptr,
                                                             d_out, stride, n, batch, op, init, totals=gt.ptr if with_totals else 0)
                                mem.sync()
                                what = (form, n, batch, op, with_totals, in_place)
                                for g_ in guards:
                                    g_.check(str(what))
                                want = ro.download()
                                got = (gn if in_place else go).download()
                                assert (got == want).all(), (what, np.flatnonzero(got != want)[:8])
                                cols = np.stack([want[c * stride:c * stride + n] for c in range(4 * batch)])
                                assert (cols < P).all() and (in_place or (np.concatenate([got[c * stride + n:(c + 1) * stride] for c in range(4 * batch - 1)])
                                                                          == SENTINEL_WORD).all())
                                if in_place:
                                    assert (go.download() == SENTINEL_WORD).all()
                                elif nw:
                                    assert (gn.download() == num_w).all(), "the numerator was changed"
                                if dw:
                                    assert (gd.download() == den_w).all(), "the denominator was changed"
                                tot, want_tot = gt.download(), rt.download()
                                assert (tot == want_tot).all(), what
                                if with_totals:
                                    assert (tot.reshape(batch, 8)[:, 5:] == 0).all()
                                    if di == 2:
                                        assert tot[4] >= 1, "the zero denominator of column 0 is counted"
                                        seen_zero += 1
                                else:
                                    assert (tot == SENTINEL_WORD).all()
                                for g_ in (go, ro, gt, rt):
                                    guards.remove(g_)
                                    g_.free(check=False)
                finally:
                    for g_ in guards:
                        g_.free(check=False)
        assert seen_zero > 0 or di != 2
        launched = ta._lib.launched_kernels()
        for k in ("extcol_dc_prepare_kernel", "extcol_aggregate_dc_kernel", "extcol_apply_dc_kernel"):
            assert any(k in s for s in launched), k
    finally:
        ctx.destroy()


# ---- 3. refusals ----
def test_every_quotient_refusal_leaves_the_outputs_untouched(ta):
    lib = ta._lib.lib
    N, lb, stride = 64, 2, 68
    out_words = 3 * stride + N
    ctx = ta.NttContext(N)
    progs, guards = [], []
    try:
        gm, gc, gq, gp = Guarded(ta, 4 * 3 * N, seed=1), Guarded(ta, 4 * out_words, seed=2), Guarded(ta, 4 * out_words, seed=3), Guarded(ta, 4 * 256, seed=4)
        guards = [gm, gc, gq, gp]
        gm.upload((np.arange(3 * N) % P).astype(np.uint32))
        gp.upload(np.arange(256, dtype=np.uint32))
        d_m, d_c, d_q, d_p = gm.ptr, gc.ptr, gq.ptr, gp.ptr
        M = ta.prover.AirMatrix
        make = lambda insns, params=True: progs.append(ta.prover.AirProgram(ctx, insns, params=params)) or progs[-1]
        # matrix 0 is not read, matrix 1 up to column 2 and rotation 15 (= N / B - 1), parameters up to 2, constraints 0 and 1, one divided
        prog = make([(CELL, 0, 15, 1, 2), (PARAM, 1, 0, 0, 2), (EMIT, 0, 0, 0, 0), (EMIT, 0, 1, 1, 1)])
        far = make([(CELL, 0, 16, 1, 2), (EMIT, 0, 0, 1, 0)])
        two = (M * 2)(M(None, 0, 0), M(d_m, 3, N))

        def run(handle=ctx.handle, p=prog, mats=two, nmats=2, log_b=lb, shift=7, par=d_p, npar=3, al=d_p, nal=2, form=EXT, c=d_c, q=d_q, os_=stride, acc=0):
            return lib.toyni_air_quotient_ext_dc_device(handle, p.handle if p else None, mats, nmats, log_b, shift, par, npar, al, nal, form, c, q, os_, acc, None)

        assert run(handle=None) == E_NULL and run(p=None) == E_NULL and run(mats=None) == E_NULL and run(al=None) == E_NULL and run(q=None) == E_NULL
        assert run(par=None) == E_NULL
        five = (M * 5)(*[M(d_m, 3, N)] * 5)
        cases = {
            "nparams < the program's": run(npar=2), "nparams > 256": run(npar=257), "nweights < nconstraints": run(nal=1),
            "nweights < nconstraints (emit_ext form, no alpha)": run(nal=0, form=EMIT_EXT), "nweights > 65536": run(nal=65537),
            "nweights > 65536 (emit_ext form)": run(nal=16385, form=EMIT_EXT), "unknown form": run(form=2), "d_params misaligned": run(par=d_p + 2),
            "d_alphas misaligned": run(al=d_p + 1),
            "nmats < nmatrices": run(nmats=1), "nmats > 4": run(mats=five, nmats=5),
            "null d_values": run(mats=(M * 2)(M(None, 0, 0), M(None, 3, N))), "width < min_width": run(mats=(M * 2)(M(None, 0, 0), M(d_m, 2, N))),
            "width > 65536": run(mats=(M * 2)(M(None, 0, 0), M(d_m, 65537, N))), "col_stride < N": run(mats=(M * 2)(M(None, 0, 0), M(d_m, 3, N - 1))),
            "max_rotation >= N / B": run(p=far), "log_blowup > log2 N": run(log_b=7), "shift 0": run(shift=0), "shift p": run(shift=P),
            "out_stride < N": run(os_=N - 1), "matrix misaligned": run(mats=(M * 2)(M(None, 0, 0), M(d_m + 2, 3, N))),
            "d_c_out misaligned": run(c=d_c + 1), "d_q_out misaligned": run(q=d_q + 2),
        }
        assert all(rc == E_RANGE for rc in cases.values()), cases
        assert run(shift=1) == E_ZERO_INVERSE
        # a program with a PARAM has no place under the calls without a parameter array
        w2 = (ctypes.c_uint32 * 8)(5, 6, 7, 8, 9, 10, 11, 12)
        assert lib.toyni_air_quotient_ext_device(ctx.handle, prog.handle, two, 2, lb, 7, w2, 2, d_c, d_q, stride, 0, None) == E_RANGE
        assert lib.toyni_air_quotient_device(ctx.handle, prog.handle, two, 2, lb, 7, w2, 2, d_c, d_q, 0, None) == E_RANGE
        with pytest.raises(RuntimeError):
            make([(PARAM, 0, 0, 0, 0), (EMIT, 0, 0, 1, 0)], params=False)      # toyni_air_program_create keeps refusing op 8
        gq.mem.sync()
        for g_, what in ((gc, "d_c_out"), (gq, "d_q_out")):
            g_.check(what)
            assert (g_.download() == SENTINEL_WORD).all(), what + " was written by a refused call"
        # what sits next to the refusals is accepted: parameters to spare, out_stride = N, no c, a null d_params under a program without PARAM
        assert run(npar=256, c=None, os_=N) == 0
        plain = make([(CELL, 0, 0, 0, 0), (EMIT, 0, 0, 1, 0)])                 # created with _create_params, no PARAM: accepted everywhere
        assert plain.nparams == 0
        one = (M * 1)(M(d_m, 1, N))
        assert run(p=plain, mats=one, nmats=1, shift=1, par=None, npar=0, nal=1, c=None) == 0
        assert lib.toyni_air_quotient_ext_device(ctx.handle, plain.handle, one, 1, lb, 1, w2, 1, None, d_q, stride, 0, None) == 0
        assert lib.toyni_air_quotient_device(ctx.handle, plain.handle, one, 1, lb, 1, w2, 1, None, d_q, 0, None) == 0
        gq.mem.sync()
        gq.check("d_q_out"), gc.check("d_c_out")
        assert (gc.download() == SENTINEL_WORD).all()
    finally:
        for p in progs:
            p.destroy()
        for g_ in guards:
            g_.free(check=False)
        ctx.destroy()


def test_every_scan_refusal_leaves_the_outputs_untouched(ta):
    pv, lib = ta.prover, ta._lib.lib
    n, batch = 40, 2
    ctx = ta.NttContext(64)
    guards = []
    try:
        gv, go, gt, gch = Guarded(ta, 4 * 8 * n, seed=1), Guarded(ta, 4 * 8 * n, seed=2), Guarded(ta, 64, seed=3), Guarded(ta, 16, seed=4)
        guards = [gv, go, gt, gch]
        gv.upload(np.arange(8 * n, dtype=np.uint32))
        gch.upload(np.array([1, 2, 3, 4], dtype=np.uint32))
        init = (ctypes.c_uint32 * 8)(1, 0, 0, 0, 1, 0, 0, 0)
        good = pv.ExtOperandDc(gv.ptr, n, 1, 0)

        def rc(num=good, den=good, c=ctx.handle, chal=gch.ptr, o=go.ptr, stride=n, n_=n, b=batch, op=0, ini=init, totals=gt.ptr):
            return lib.toyni_column_scan_ext_dc_device(c, ctypes.byref(num) if num is not None else None, ctypes.byref(den) if den is not None else None,
                                                       chal, o, stride, n_, b, op, ini, totals, None)

        assert rc(c=None) == E_NULL and rc(o=None) == E_NULL and rc(ini=None) == E_NULL and rc(chal=None) == E_NULL
        cases = {
            "both operands absent": rc(num=None, den=None), "width 2": rc(num=pv.ExtOperandDc(gv.ptr, n, 2, 0)),
            "width 1 with null d_values": rc(num=pv.ExtOperandDc(0, n, 1, 0)), "operand stride < n, batch 2": rc(num=pv.ExtOperandDc(gv.ptr, n - 1, 1, 0)),
            "width 4 stride < n": rc(num=pv.ExtOperandDc(gv.ptr, n - 1, 4, 0), b=1), "index 2^20": rc(den=pv.ExtOperandDc(gv.ptr, n, 1, 1 << 20)),
            "unknown op": rc(op=2), "n > 2^27": rc(n_=(1 << 27) + 1, stride=1 << 28, num=pv.ExtOperandDc(gv.ptr, 1 << 28, 1, 0), den=None),
            "out_stride < n": rc(stride=n - 1), "batch 2^14": rc(b=1 << 14), "init >= p": rc(ini=(ctypes.c_uint32 * 8)(1, 0, 0, 0, 1, P, 0, 0)),
            "d_challenges misaligned": rc(chal=gch.ptr + 2), "d_out misaligned": rc(o=go.ptr + 1), "d_totals misaligned": rc(totals=gt.ptr + 2),
            "operand misaligned": rc(den=pv.ExtOperandDc(gv.ptr + 2, n, 1, 0)),
        }
        assert all(v == E_RANGE for v in cases.values()), cases
        go.mem.sync()
        for g_, what in ((go, "d_out"), (gt, "d_totals")):
            g_.check(what)
            assert (g_.download() == SENTINEL_WORD).all(), what + " was written by a refused call"
        assert rc(num=pv.ExtOperandDc(gv.ptr, n, 1), den=None, chal=None) == 0          # no index named: no challenge array needed
        go.mem.sync()
        assert (go.download() < P).all()
    finally:
        for g_ in guards:
            g_.free(check=False)
        ctx.destroy()


# ---- 4, 5. capture, a second run, a second stream ----
def _u32(t):
    return t.cpu().numpy().view(np.uint32).copy()


def _dev(arr, tdev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32).reshape(-1)).to(tdev)


def test_quotient_graph_reads_the_challenges_at_replay_and_the_call_repeats_on_a_second_stream(ta):
    import torch
    tdev = torch.device("cuda", 0)
    N, log_b, nparams, nalphas = 1 << 12, 3, 4, 17                              # 68 weights: beyond what ever rode in kernel arguments
    rng = np.random.default_rng(71)
    const_insns = random_program(rng, 7, 40, [3], N >> log_b, 5, int(rng.integers(0, P)))
    param_insns, _, used = parametrise(const_insns, nparams, rng)
    slots = [i for i, ins in enumerate(param_insns) if ins[0] == PARAM]
    assert used >= 1

    def substituted(params_raw):
        out = list(const_insns)
        for i in slots:
            op, dst, a, b, j = param_insns[i]
            out[i] = (CONST, dst, 0, 0, int(params_raw[j]) % P)
        return out

    ctx = ta.NttContext(N)
    try:
        with ta.prover.AirProgram(ctx, param_insns, params=True) as prog:
            m = rng.integers(0, P, (3, N), dtype=np.uint64)
            buf = _dev(m, tdev)
            q, c, wq, wc = (torch.empty(4 * N, dtype=torch.int32, device=tdev) for _ in range(4))
            d_par, d_al = torch.zeros(nparams, dtype=torch.int32, device=tdev), torch.zeros(4 * nalphas, dtype=torch.int32, device=tdev)
            s, s2 = torch.cuda.Stream(device=tdev), torch.cuda.Stream(device=tdev)
            call = lambda st: ta.prover.air_quotient_ext_dc_device(ctx, prog, [(buf.data_ptr(), 3, N)], log_b, 7, d_par.data_ptr(), nparams, d_al.data_ptr(),
                                                                   nalphas, EMIT_EXT, q.data_ptr(), N, d_c_out=c.data_ptr(), stream=st.cuda_stream)

            def want(params_raw, alphas_raw):
                with ta.prover.AirProgram(ctx, substituted(params_raw)) as ref:
                    ta.air_quotient_ext_device(ctx, ref, [(buf.data_ptr(), 3, N)], log_b, 7, host_weights(ta, alphas_raw, EMIT_EXT), wq.data_ptr(), N,
                                               d_c_out=wc.data_ptr())
                    torch.cuda.synchronize()
                return _u32(wq), _u32(wc)

            def load():
                pr, al = rng.integers(0, 1 << 32, nparams, dtype=np.uint64).astype(np.uint32), raw_alphas(rng, nalphas)
                d_par.copy_(_dev(pr, tdev)), d_al.copy_(_dev(al, tdev))
                q.fill_(-1), c.fill_(-1)
                torch.cuda.synchronize()
                return pr, al

            pr, al = load()
            wq0, wc0 = want(pr, al)
            for st in (s, s, s2):                                                # twice on one stream (the second call warm), once on another
                q.fill_(-1), c.fill_(-1)
                torch.cuda.synchronize()
                call(st)
                torch.cuda.synchronize()
                assert (_u32(q) == wq0).all() and (_u32(c) == wc0).all()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):                                 # two kernel nodes, one after the other
                call(s)
            for _ in range(2):
                pr, al = load()                                                 # the challenge words are OVERWRITTEN, then the graph replayed
                g.replay()
                torch.cuda.synchronize()
                got_q, got_c = _u32(q), _u32(c)
                wq1, wc1 = want(pr, al)
                assert (got_q == wq1).all() and (got_c == wc1).all()
                assert (wq1 != wq0).any()
                for e in (0, 3):
                    mc, mq = air_model(substituted(pr), [m], N, log_b, 7, [int(v) for v in host_weights(ta, al, EMIT_EXT)[:, e]])
                    assert (got_c[e * N:(e + 1) * N] == mc).all() and (got_q[e * N:(e + 1) * N] == mq).all(), e
            del g
    finally:
        ctx.destroy()


def test_scan_graph_reads_gamma_at_replay_and_the_call_repeats_on_a_second_stream(ta):
    import torch
    pv = ta.prover
    tdev = torch.device("cuda", 0)
    tile = pv.column_scan_ext_tile()
    rng = np.random.default_rng(73)
    ctx = ta.NttContext(1 << 10)
    try:
        for n, op in ((tile, pv.SCAN_SUM), (3 * tile + 7, pv.SCAN_PRODUCT)):     # one launch behind the preparation, and three
            a, b = _dev(rng.integers(0, P, n), tdev), _dev(rng.integers(0, P, n), tdev)
            out, ref, tot, rtot = (torch.empty(k, dtype=torch.int32, device=tdev) for k in (4 * n, 4 * n, 8, 8))
            d_g = torch.zeros(8, dtype=torch.int32, device=tdev)
            s, s2 = torch.cuda.Stream(device=tdev), torch.cuda.Stream(device=tdev)
            init = [(5, 6, 7, 8)]
            call = lambda st: pv.column_scan_ext_dc_device(ctx, pv.ExtOperandDc(a.data_ptr(), n, 1, 1), pv.ExtOperandDc(b.data_ptr(), n, 1, 1), d_g.data_ptr(),
                                                           out.data_ptr(), n, n, 1, op, init, totals=tot.data_ptr(), stream=st.cuda_stream)

            def want(words):
                gamma = tuple(int(w) % P for w in words[4:])
                pv.column_scan_ext_device(ctx, pv.ExtOperand(a.data_ptr(), n, 1, gamma), pv.ExtOperand(b.data_ptr(), n, 1, gamma), ref.data_ptr(), n, n, 1, op,
                                          init, totals=rtot.data_ptr())
                torch.cuda.synchronize()
                return _u32(ref), _u32(rtot)

            def load():
                words = rng.integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32)
                d_g.copy_(_dev(words, tdev))
                out.fill_(-1), tot.fill_(-1)
                torch.cuda.synchronize()
                return words

            words = load()
            w0, t0 = want(words)
            for st in (s, s, s2):
                out.fill_(-1), tot.fill_(-1)
                torch.cuda.synchronize()
                call(st)
                torch.cuda.synchronize()
                assert (_u32(out) == w0).all() and (_u32(tot) == t0).all()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):                                 # a linear chain: the preparation, then one or three launches
                call(s)
            for _ in range(2):
                words = load()
                g.replay()
                torch.cuda.synchronize()
                w1, t1 = want(words)
                assert (_u32(out) == w1).all() and (_u32(tot) == t1).all() and (w1 != w0).any()
            del g
    finally:
        ctx.destroy()
