"""The batch dimension of the first half of a Fibonacci proof (include/toyni_hip.h 3s): the ten entry points are exported with the
header's parameter counts and bound in the Python package, and every refusal the host decides before anything is enqueued comes from
an otherwise valid call with the outputs untouched.  The pointers are host stand-in memory (tests/guarded.py HostMem), the context a
block of it that a call which passed its checks would misread -- none does (a call on it is refused when the context is first read:
the stride refusals of the two calls that read it before their strides are held on a real context by
tests/test_gpu_fib_batch_calls.py).  The order of the refusals is 3r's: null pointers, batch, the single call's own in the single
call's order (held here against the single call itself on the same bad arguments), the strides.  No compute."""
import ctypes
import os

import numpy as np
import pytest

from guarded import Guarded, HostMem, P

E_INVALID_SIZE, E_NULL, E_ZERO_INVERSE, E_RANGE = 10001, 10002, 10005, 10006
COUNTS = {"toyni_chacha20_fill_batch_device": 7, "toyni_mask_poly_batch_device": 8, "toyni_fib_quotient_batch_device": 11,
          "toyni_transcript_squeeze_point_batch_device": 7, "toyni_poly_eval_dz_batch_device": 12, "toyni_transcript_absorb_fields_batch_device": 6,
          "toyni_fib_deep_dz_batch_device": 18, "toyni_query_rows_batch_device": 10, "toyni_fri_phase_roots_batch_device": 8,
          "toyni_copy_rows_device": 7}
BAD_BATCHES = (0, 65536, 1 << 40)


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def test_symbols_are_exported_and_bound_with_the_headers_parameter_counts(ta):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "toyni_hip.h")).read()
    assert " * 3s. " in header and header.index(" * 3r. ") < header.index(" * 3s. ") < header.index(" * 3c. ")
    for name, nargs in COUNTS.items():
        assert name in ta._lib.SIGNATURES and hasattr(ta._lib.lib, name), name
        f = getattr(ta._lib.lib, name)
        assert f.argtypes == ta._lib.SIGNATURES[name][1] and len(f.argtypes) == nargs and f.restype is ctypes.c_int
        decl = header.split("int " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == nargs, (name, decl)
    c_size, c_void = ctypes.c_size_t, ctypes.c_void_p
    # every stride is a size_t
    assert ta._lib.SIGNATURES["toyni_copy_rows_device"][1] == [c_void, c_size, c_void, c_size, c_size, c_size, c_void]
    assert ta._lib.SIGNATURES["toyni_fri_phase_roots_batch_device"][1] == [c_void, c_size, c_size, ctypes.c_uint, c_size, c_void, c_size, c_void]
    for name in ("chacha20_fill_batch_device", "mask_poly_batch_device", "fib_quotient_batch_device", "poly_eval_dz_batch_device",
                 "fib_deep_dz_batch_device", "query_rows_batch_device", "fri_phase_roots_batch_device", "copy_rows_device"):
        assert hasattr(ta.prover, name), name
    for method in ("squeeze_point", "absorb_fields"):
        assert hasattr(ta.prover.DeviceTranscriptBatch, method)


def _untouched(buffers):
    for name, g in buffers:
        g.check(name)
        assert (g.download(np.uint8) == 0xA5).all(), name


def test_every_refusal_of_the_calls_without_a_context_leaves_everything_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    B = 3
    out, keys, tr, wordsb, idx = (Guarded(mem, 1 << 16, word=1, seed=1), Guarded(mem, 32 * B, word=1, seed=2), Guarded(mem, 1024 * B, seed=3),
                                  Guarded(mem, 4096, seed=4), Guarded(mem, 4096, seed=5))
    key = (ctypes.c_uint8 * 32)(*range(32))
    offs = (ctypes.c_uint32 * 3)(0, 32, 64)
    big_off = (ctypes.c_uint32 * 3)(0, 32, 256)
    try:
        def fill(o=out.ptr, st=128 + 16, n=128, k=keys.ptr, b=B):
            return lib.toyni_chacha20_fill_batch_device(o, st, n, k, 0, b, None)

        def mask(c=out.ptr, st=8 + 140, n=8, md=140, k=keys.ptr, b=B):
            return lib.toyni_mask_poly_batch_device(c, st, n, md, k, 1, b, None)

        def point(t=tr.ptr, b=B, log_N=10, shift=7, z=out.ptr, st=1):
            return lib.toyni_transcript_squeeze_point_batch_device(t, b, log_N, shift, z, st, None)

        def fields(t=tr.ptr, b=B, w=wordsb.ptr, st=4, n=4):
            return lib.toyni_transcript_absorb_fields_batch_device(t, b, w, st, n, None)

        def rows(i=idx.ptr, ist=8, n=8, size=256, off=offs, noff=3, b=B, o=out.ptr, ost=24):
            return lib.toyni_query_rows_batch_device(i, ist, n, size, off, noff, b, o, ost, None)

        def roots(lv=wordsb.ptr, ls=32 * (15 + 7), m=8, r=2, b=B, o=out.ptr, rs=64):
            return lib.toyni_fri_phase_roots_batch_device(lv, ls, m, r, b, o, rs, None)

        def copy(dst=out.ptr, ds=48, src=wordsb.ptr, ss=40, n=36, r=B):
            return lib.toyni_copy_rows_device(dst, ds, src, ss, n, r, None)

        nulls = {"fill out": fill(o=None), "fill keys": fill(k=None), "mask coeffs": mask(c=None), "mask keys": mask(k=None), "point tr": point(t=None),
                 "point z": point(z=None), "fields tr": fields(t=None), "fields words": fields(w=None), "rows idx": rows(i=None), "rows out": rows(o=None),
                 "rows offsets": rows(off=None), "roots levels": roots(lv=None), "roots out": roots(o=None), "copy dst": copy(dst=None),
                 "copy src": copy(src=None),
                 # a null pointer is named before a bad batch
                 "fill, batch 0": fill(o=None, b=0), "mask, batch 2^16": mask(k=None, b=1 << 16), "point, batch 0": point(z=None, b=0),
                 "fields, batch 0": fields(t=None, b=0), "rows, batch 0": rows(off=None, b=0), "roots, batch 0": roots(o=None, b=0),
                 "copy, rows 2^16": copy(src=None, r=1 << 16)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        ranges = {}
        for b in BAD_BATCHES:
            ranges.update({f"fill batch {b}": fill(b=b), f"mask batch {b}": mask(b=b), f"point batch {b}": point(b=b), f"fields batch {b}": fields(b=b),
                           f"rows batch {b}": rows(b=b), f"roots batch {b}": roots(b=b)})
        ranges.update({
            # batch before the single call's own: the code would be the same, so the pair is held where the codes differ (roots, below)
            "copy rows 65536": copy(r=65536),
            # the single calls' own
            "fill out + 8": fill(o=out.ptr + 8), "fill bytes 100": fill(n=100, st=256), "fill bytes 2^38 + 64": fill(n=(1 << 38) + 64, st=1 << 39),
            "mask degree 0": mask(md=0), "mask degree 4097": mask(md=4097, st=8192), "mask n 0": mask(n=0), "mask coeffs + 2": mask(c=out.ptr + 2),
            "point tr + 4": point(t=tr.ptr + 4), "point z + 1": point(z=out.ptr + 1), "point log_N 28": point(log_N=28), "point shift 0": point(shift=0),
            "point shift p": point(shift=P),
            "fields tr + 8": fields(t=tr.ptr + 8), "fields words + 2": fields(w=wordsb.ptr + 2), "fields 127": fields(n=127, st=200),
            "rows idx + 2": rows(i=idx.ptr + 2), "rows out + 1": rows(o=out.ptr + 1), "rows noffsets 0": rows(noff=0), "rows noffsets 9": rows(noff=9),
            "rows n 0": rows(size=0), "rows n 2^33": rows(size=1 << 33), "rows count 65537": rows(n=65537, ist=1 << 20, ost=1 << 30),
            "rows offset >= n": rows(off=big_off),
            "roots rounds 65": roots(r=65, ls=1 << 20, rs=1 << 20), "roots too many rounds": roots(r=5, ls=1 << 20, rs=1 << 20),
            "roots levels + 8": roots(lv=wordsb.ptr + 8), "roots out + 2": roots(o=out.ptr + 2),
            "copy dst + 2": copy(dst=out.ptr + 2), "copy src + 1": copy(src=wordsb.ptr + 1), "copy row_bytes 34": copy(n=34),
            "copy dst_stride 50": copy(ds=50), "copy src_stride 38": copy(ss=38),
            # a stride one element short of the extent, and one that breaks the alignment rule
            "fill stride 112": fill(st=112), "fill stride 127": fill(st=127), "fill stride + 8": fill(st=128 + 8), "fill stride 0": fill(st=0),
            "fill keys + 2": fill(k=keys.ptr + 2),
            "mask stride n + d - 1": mask(st=8 + 140 - 1), "mask stride 0": mask(st=0), "mask keys + 1": mask(k=keys.ptr + 1),
            "point z_stride 0": point(st=0), "fields word_stride 3": fields(st=3), "fields word_stride 0": fields(st=0),
            "rows index_stride 7": rows(ist=7), "rows out_stride 23": rows(ost=23),
            "roots level_stride - 16": roots(ls=32 * 22 - 16), "roots level_stride + 8": roots(ls=32 * 22 + 8), "roots level_stride 0": roots(ls=0),
            "roots root_stride 60": roots(rs=60), "roots root_stride 66": roots(rs=66),
            "copy dst_stride 32": copy(ds=32), "copy src_stride 32": copy(ss=32),
        })
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        # the single calls' refusals arrive through the batch call in the single call's order, with its codes
        assert roots(m=12) == E_INVALID_SIZE == lib.toyni_fri_phase_roots_device(wordsb.ptr, 12, 2, out.ptr, None)
        assert roots(m=1 << 33, ls=1 << 40) == E_INVALID_SIZE and roots(m=12, r=65) == E_INVALID_SIZE and roots(m=12, lv=wordsb.ptr + 8) == E_INVALID_SIZE
        assert roots(m=12, b=0) == E_RANGE and roots(m=12, ls=0) == E_INVALID_SIZE          # batch before, the strides after the single call's own
        pairs = [
            (fill(o=out.ptr + 8, st=0), lib.toyni_chacha20_fill_device(out.ptr + 8, 128, key, 0, None)),
            (fill(n=100), lib.toyni_chacha20_fill_device(out.ptr, 100, key, 0, None)),
            (mask(md=0, st=0), lib.toyni_mask_poly_device(out.ptr, 8, 0, key, 1, None)),
            (mask(n=0), lib.toyni_mask_poly_device(out.ptr, 0, 140, key, 1, None)),
            (point(log_N=28, st=0), lib.toyni_transcript_squeeze_point_device(tr.ptr, 28, 7, out.ptr, None)),
            (point(shift=P), lib.toyni_transcript_squeeze_point_device(tr.ptr, 10, P, out.ptr, None)),
            (fields(n=127), lib.toyni_transcript_absorb_fields_device(tr.ptr, wordsb.ptr, 127, None)),
            (rows(noff=9, ist=0), lib.toyni_query_rows_device(idx.ptr, 8, 256, offs, 9, out.ptr, None)),
            (rows(off=big_off, ost=0), lib.toyni_query_rows_device(idx.ptr, 8, 256, big_off, 3, out.ptr, None)),
        ]
        assert all(got == want != 0 for got, want in pairs), pairs
        # nothing to do is no refusal and enqueues nothing (no device is needed to say so); there batch = 65535 passes and 65536 does not
        assert fill(n=0, st=0, b=65535) == 0 and fill(n=0, st=0, b=65536) == E_RANGE
        assert fields(n=0, st=0, b=65535) == 0 and fields(w=None, n=0, st=0, b=65535) == 0 and fields(n=0, st=0, b=65536) == E_RANGE
        assert rows(n=0, ist=0, ost=0, b=65535) == 0 and rows(n=0, ist=0, ost=0, b=65536) == E_RANGE
        assert roots(r=0, ls=0, rs=0, b=65535) == 0 and roots(r=0, ls=0, rs=0, b=65536) == E_RANGE
        assert copy(r=0) == 0 and copy(n=0, ds=0, ss=0, r=65535) == 0 and copy(n=0, ds=0, ss=0, r=65536) == E_RANGE
        _untouched((("out", out), ("keys", keys), ("tr", tr), ("words", wordsb), ("idx", idx)))
    finally:
        for g in (out, keys, tr, wordsb, idx):
            g.free()


def test_every_refusal_of_the_calls_with_a_context_leaves_everything_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    B, N = 3, 256
    fake_ctx, trace, quot, out, small = (Guarded(mem, 4096, seed=1), Guarded(mem, 4 * (N + 4) * B, seed=2), Guarded(mem, 4 * (N + 4) * B, seed=3),
                                         Guarded(mem, 4 * (N + 4) * B, seed=4), Guarded(mem, 4096, seed=5))
    mults = (ctypes.c_uint32 * 3)(1, 5, 25)
    bad_mults = (ctypes.c_uint32 * 3)(1, P, 25)
    try:
        def quotient(ctx=fake_ctx.ptr, t=trace.ptr, ts=N + 4, c=out.ptr, cs=N + 4, q=quot.ptr, qs=N + 4, lb=5, shift=7, b=B):
            return lib.toyni_fib_quotient_batch_device(ctx, t, ts, c, cs, q, qs, lb, shift, b, None)

        def deep(ctx=fake_ctx.ptr, t=trace.ptr, ts=N + 4, q=quot.ptr, qs=N + 4, o=out.ptr, os_=N + 4, lb=5, shift=7, z=small.ptr, zs=8, ood=small.ptr + 4,
                 ods=8, n=8, chk=small.ptr + 20, cs=8, b=B):
            return lib.toyni_fib_deep_dz_batch_device(ctx, t, ts, q, qs, o, os_, lb, shift, z, zs, ood, ods, n, chk, cs, b, None)

        def evaluate(ctx=fake_ctx.ptr, c=trace.ptr, cs=N + 4, nc=N, z=small.ptr, zs=8, m=mults, np_=3, b=B, o=out.ptr, os_=4):
            return lib.toyni_poly_eval_dz_batch_device(ctx, c, cs, nc, z, zs, m, np_, b, o, os_, None)

        nulls = {"quotient ctx": quotient(ctx=None), "quotient trace": quotient(t=None), "quotient q": quotient(q=None),
                 "deep ctx": deep(ctx=None), "deep trace": deep(t=None), "deep quot": deep(q=None), "deep out": deep(o=None), "deep z": deep(z=None),
                 "deep ood": deep(ood=None), "eval ctx": evaluate(ctx=None), "eval z": evaluate(z=None), "eval mults": evaluate(m=None),
                 "eval out": evaluate(o=None), "eval coeffs": evaluate(c=None),
                 "quotient, batch 0": quotient(q=None, b=0), "deep, batch 0": deep(ood=None, b=0), "eval, batch 2^16": evaluate(o=None, b=1 << 16)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        ranges = {}
        for b in BAD_BATCHES:
            ranges.update({f"quotient batch {b}": quotient(b=b), f"deep batch {b}": deep(b=b), f"eval batch {b}": evaluate(b=b)})
        ranges.update({
            # the single calls' own that are decided on the arguments alone
            "deep shift 0": deep(shift=0), "deep shift p": deep(shift=P), "deep trace_len 12": deep(n=12), "deep trace_len 2^28": deep(n=1 << 28),
            "deep z + 2": deep(z=small.ptr + 2), "deep ood + 1": deep(ood=small.ptr + 5), "deep check + 3": deep(chk=small.ptr + 23),
            "eval npoints 0": evaluate(np_=0), "eval npoints 5": evaluate(np_=5, os_=8), "eval mult p": evaluate(m=bad_mults),
            "eval coeffs + 2": evaluate(c=trace.ptr + 2), "eval z + 1": evaluate(z=small.ptr + 1), "eval out + 2": evaluate(o=out.ptr + 2),
            # the strides of the evaluation are judged before its context is read
            "eval coeff_stride - 1": evaluate(cs=N - 1), "eval z_stride 0": evaluate(zs=0), "eval out_stride 2": evaluate(os_=2),
            "eval all strides 0": evaluate(cs=0, zs=0, os_=0),
            # ... and a context that says log_N < log_blowup is the single call's refusal
            "quotient on the stand-in context": quotient(), "deep on the stand-in context": deep(),
        })
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        pairs = [
            (deep(shift=0, ts=0), lib.toyni_fib_deep_dz_device(fake_ctx.ptr, trace.ptr, quot.ptr, out.ptr, 5, 0, small.ptr, small.ptr + 4, 8, None, None)),
            (deep(n=12), lib.toyni_fib_deep_dz_device(fake_ctx.ptr, trace.ptr, quot.ptr, out.ptr, 5, 7, small.ptr, small.ptr + 4, 12, None, None)),
            (evaluate(np_=5, cs=0), lib.toyni_poly_eval_dz_device(fake_ctx.ptr, trace.ptr, N, small.ptr, mults, 5, out.ptr, None)),
            (evaluate(m=bad_mults, os_=0), lib.toyni_poly_eval_dz_device(fake_ctx.ptr, trace.ptr, N, small.ptr, bad_mults, 3, out.ptr, None)),
            (quotient(shift=0, ts=0), lib.toyni_fib_quotient_device(fake_ctx.ptr, trace.ptr, out.ptr, quot.ptr, 5, 0, None)),
        ]
        assert all(got == want != 0 for got, want in pairs), pairs
        # batch = 65535 passes the batch check (the next refusal is the single call's): 65536 is named first
        assert deep(b=65535, n=12) == E_RANGE and evaluate(b=65535, np_=0) == E_RANGE
        _untouched((("ctx", fake_ctx), ("trace", trace), ("quot", quot), ("out", out), ("small", small)))
    finally:
        for g in (fake_ctx, trace, quot, out, small):
            g.free()
