"""The Ext accumulator-column calls (include/toyni_hip.h 3i): exported, bound, and every refusal of the header from an otherwise valid
call with the outputs untouched.  The refusals are decided on the arguments alone, before the context is touched and before anything is
enqueued, so they can be asked for without a device: the pointers are host stand-in memory (tests/guarded.py HostMem), the context a
block of it that a call which passed its checks would misread -- none does.  No compute (no GPU here)."""
import ctypes

import numpy as np
import pytest

from guarded import Guarded, HostMem, P

E_NULL, E_RANGE = 10002, 10006
SUM, PRODUCT = 0, 1


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def test_symbols_are_exported_and_bound(ta):
    for name in ("toyni_column_scan_ext_tile", "toyni_batch_inverse_ext_device", "toyni_column_scan_ext_device"):
        assert name in ta._lib.SIGNATURES and hasattr(ta._lib.lib, name)
        assert getattr(ta._lib.lib, name).argtypes == ta._lib.SIGNATURES[name][1]
    for name in ("ExtOperand", "batch_inverse_ext_device", "column_scan_ext_device", "column_scan_ext_tile"):
        assert hasattr(ta.prover, name)
    op = ta.prover.ExtOperand(0x1000, 7, 4, (1, 2, 3, 4))
    assert (op.d_values, op.stride, op.width, list(op.shift)) == (0x1000, 7, 4, [1, 2, 3, 4])
    assert ctypes.sizeof(op) == 40                                             # pointer, size_t, five words and the tail padding of the C struct


def test_the_tile_is_a_power_of_two(ta):
    t = ta.prover.column_scan_ext_tile()
    assert t >= 64 and t & (t - 1) == 0


def test_every_refusal_leaves_the_outputs_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    n, batch, stride = 100, 3, 104
    words = 4 * batch * stride
    bufs = {k: Guarded(mem, 4 * words, seed=i) for i, k in enumerate(("num", "den", "out"))}
    totals, zc, fake_ctx = Guarded(mem, 32 * batch, seed=7), Guarded(mem, 4, seed=8), Guarded(mem, 4096, seed=9)
    filling = (np.arange(words, dtype=np.uint32) * 7919 + 1) % P
    bufs["num"].upload(filling), bufs["den"].upload(filling[::-1].copy())
    before = {k: g.download() for k, g in bufs.items()}
    init = (ctypes.c_uint32 * (4 * batch))(1, 2, 3, 4, 5, 6, 7, 8, P - 1, 0, 0, 1)
    Op = ta.prover.ExtOperand
    try:
        def run(ctx=fake_ctx.ptr, num=Op(bufs["num"].ptr, stride, 4, (1, 2, 3, 4)), den=Op(bufs["den"].ptr, stride, 1, (5, 6, 7, 8)), out=bufs["out"].ptr,
                os_=stride, n=n, batch=batch, op=SUM, init=init, tot=totals.ptr):
            return lib.toyni_column_scan_ext_device(ctx, ctypes.byref(num) if num is not None else None, ctypes.byref(den) if den is not None else None,
                                                    out, os_, n, batch, op, init, tot, None)

        nulls = {"ctx": run(ctx=None), "d_out": run(out=None), "init": run(init=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        big = 1 << 28
        bad_init = lambda k, v: (ctypes.c_uint32 * (4 * batch))(*[v if j == k else 1 for j in range(4 * batch)])
        ranges = {
            "both operands absent": run(num=None, den=None), "both of width 0": run(num=Op(), den=Op(bufs["den"].ptr, stride, 0)),
            "one null, one of width 0": run(num=None, den=Op()),
            "num width 2": run(num=Op(bufs["num"].ptr, stride, 2)), "den width 3": run(den=Op(bufs["den"].ptr, stride, 3)),
            "num width 5": run(num=Op(bufs["num"].ptr, stride, 5)),
            "num null values": run(num=Op(0, stride, 4)), "den null values": run(den=Op(0, stride, 1)),
            "op 2": run(op=2), "op -1": run(op=-1),
            "n > 2^27": run(n=(1 << 27) + 1, os_=big, num=Op(bufs["num"].ptr, big, 4), den=Op(bufs["den"].ptr, big, 1)),
            "width-4 stride < n": run(num=Op(bufs["num"].ptr, n - 1, 4)), "width-4 stride < n at batch 1": run(num=Op(bufs["num"].ptr, n - 1, 4), batch=1),
            "width-1 stride < n at batch 3": run(den=Op(bufs["den"].ptr, n - 1, 1)),
            "out stride < n": run(os_=n - 1), "out stride < n at batch 1": run(os_=n - 1, batch=1),
            "batch 2^14": run(batch=1 << 14, init=(ctypes.c_uint32 * (4 << 14))()),
            "init p": run(init=bad_init(11, P)), "init 2^32 - 1": run(init=bad_init(0, 0xFFFFFFFF)), "init coordinate 2 = p": run(init=bad_init(6, P)),
            "num shift p": run(num=Op(bufs["num"].ptr, stride, 4, (0, 0, P, 0))), "den shift 2^32 - 1": run(den=Op(bufs["den"].ptr, stride, 1, (0, 0, 0, 0xFFFFFFFF))),
            "num misaligned": run(num=Op(bufs["num"].ptr + 2, stride, 4)), "den misaligned": run(den=Op(bufs["den"].ptr + 1, stride, 1)),
            "out misaligned": run(out=bufs["out"].ptr + 3), "totals misaligned": run(tot=totals.ptr + 2),
        }
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        # nothing to do is no refusal, and writes nothing; the stride of a single base column is not looked at; an absent operand's other
        # fields are ignored
        assert run(n=0) == 0 and run(batch=0) == 0 and run(batch=0, init=(ctypes.c_uint32 * 1)(P)) == 0
        assert run(n=0, batch=1, den=Op(bufs["den"].ptr, 0, 1)) == 0 and run(n=0, den=Op(0, 0, 0, (P, P, P, P))) == 0
        # the inversion: null and misaligned pointers, a count past 2^32, strides below the count
        inv = lambda src=bufs["num"].ptr, ss=stride, dst=bufs["out"].ptr, ds=stride, count=n, z=zc.ptr: \
            lib.toyni_batch_inverse_ext_device(src, ss, dst, ds, count, z, None)
        assert inv(src=None) == E_NULL and inv(dst=None) == E_NULL
        assert inv(src=bufs["num"].ptr + 2) == E_RANGE and inv(dst=bufs["out"].ptr + 1) == E_RANGE and inv(z=zc.ptr + 2) == E_RANGE
        assert inv(count=(1 << 32) + 1, ss=1 << 33, ds=1 << 33) == E_RANGE and inv(ss=n - 1) == E_RANGE and inv(ds=n - 1) == E_RANGE
        for k, g in bufs.items():
            g.check(k)
            assert (g.download() == before[k]).all(), k
        assert (totals.download() == 0xA5A5A5A5).all() and (zc.download() == 0xA5A5A5A5).all() and (bufs["out"].download() == 0xA5A5A5A5).all()
        assert (fake_ctx.download(np.uint8) == 0xA5).all()                     # the stand-in context was not written either
    finally:
        for g in list(bufs.values()) + [totals, zc, fake_ctx]:
            g.free()
