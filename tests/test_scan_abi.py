"""The accumulator-column calls (include/toyni_hip.h 3g): exported, bound, and every refusal of the header from an otherwise valid
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
    for name in ("toyni_column_scan_tile", "toyni_batch_inverse_device", "toyni_column_scan_device"):
        assert name in ta._lib.SIGNATURES and hasattr(ta._lib.lib, name)
        assert getattr(ta._lib.lib, name).argtypes == ta._lib.SIGNATURES[name][1]
    for name in ("batch_inverse_device", "column_scan_device", "column_scan_tile", "SCAN_SUM", "SCAN_PRODUCT"):
        assert hasattr(ta.prover, name)
    assert (ta.prover.SCAN_SUM, ta.prover.SCAN_PRODUCT) == (SUM, PRODUCT)


def test_the_tile_is_a_power_of_two(ta):
    t = ta.prover.column_scan_tile()
    assert t >= 64 and t & (t - 1) == 0


def test_every_refusal_leaves_the_outputs_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    n, batch, stride = 100, 3, 104
    words = batch * stride
    bufs = {k: Guarded(mem, 4 * words, seed=i) for i, k in enumerate(("num", "den", "out"))}
    totals, zc, fake_ctx = Guarded(mem, 8 * batch, seed=7), Guarded(mem, 4, seed=8), Guarded(mem, 4096, seed=9)
    filling = (np.arange(words, dtype=np.uint32) * 7919 + 1) % P
    bufs["num"].upload(filling), bufs["den"].upload(filling[::-1].copy())
    before = {k: g.download() for k, g in bufs.items()}
    init = (ctypes.c_uint32 * batch)(1, 2, P - 1)
    try:
        def run(ctx=fake_ctx.ptr, num=bufs["num"].ptr, ns=stride, den=bufs["den"].ptr, ds=stride, out=bufs["out"].ptr, os_=stride, n=n, batch=batch,
                op=SUM, init=init, tot=totals.ptr):
            return lib.toyni_column_scan_device(ctx, num, ns, den, ds, out, os_, n, batch, op, init, tot, None)

        nulls = {"ctx": run(ctx=None), "d_out": run(out=None), "init": run(init=None), "both operands": run(num=None, den=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        ranges = {
            "op 2": run(op=2), "op -1": run(op=-1), "n > 2^27": run(n=(1 << 27) + 1, ns=1 << 28, ds=1 << 28, os_=1 << 28),
            "num stride < n": run(ns=n - 1), "den stride < n": run(ds=n - 1), "out stride < n": run(os_=n - 1),
            "batch 2^16": run(batch=1 << 16, init=(ctypes.c_uint32 * (1 << 16))()),
            "init p": run(init=(ctypes.c_uint32 * batch)(1, 2, P)), "init 2^32 - 1": run(init=(ctypes.c_uint32 * batch)(0xFFFFFFFF, 0, 0)),
            "num misaligned": run(num=bufs["num"].ptr + 2), "den misaligned": run(den=bufs["den"].ptr + 1), "out misaligned": run(out=bufs["out"].ptr + 3),
            "totals misaligned": run(tot=totals.ptr + 2),
        }
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        # nothing to do is no refusal, and writes nothing; the stride of a single column is not looked at
        assert run(n=0) == 0 and run(batch=0) == 0 and run(batch=0, init=(ctypes.c_uint32 * 1)(P)) == 0
        # the inversion: null and misaligned pointers, a count past 2^32
        inv = lambda src=bufs["num"].ptr, dst=bufs["out"].ptr, count=n, z=zc.ptr: lib.toyni_batch_inverse_device(src, dst, count, z, None)
        assert inv(src=None) == E_NULL and inv(dst=None) == E_NULL
        assert inv(src=bufs["num"].ptr + 2) == E_RANGE and inv(dst=bufs["out"].ptr + 1) == E_RANGE and inv(z=zc.ptr + 2) == E_RANGE
        assert inv(count=(1 << 32) + 1) == E_RANGE
        for k, g in bufs.items():
            g.check(k)
            assert (g.download() == before[k]).all(), k
        assert (totals.download() == 0xA5A5A5A5).all() and (zc.download() == 0xA5A5A5A5).all() and (bufs["out"].download() == 0xA5A5A5A5).all()
        assert (fake_ctx.download(np.uint8) == 0xA5).all()                     # the stand-in context was not written either
    finally:
        for g in list(bufs.values()) + [totals, zc, fake_ctx]:
            g.free()
