"""The calls of include/toyni_hip.h 3q: exported with the header's parameter counts, bound in the Python package, and every refusal
the host decides before anything is enqueued, from an otherwise valid call with the outputs and a stand-in transcript untouched.
The pointers are host stand-in memory (tests/guarded.py HostMem), the context a block of it that a call which passed its checks
would misread -- none does.  The one refusal of toyni_fib_deep_dz_device that reads the context's size (log_blowup > log N) needs a
real context and is in tests/test_gpu_fib_dz.py.  No compute (no GPU here)."""
import ctypes
import os

import numpy as np
import pytest

from guarded import Guarded, HostMem, P

E_NULL, E_INVALID_SIZE, E_RANGE = 10002, 10001, 10006
COUNTS = {"toyni_mask_poly_device": 6, "toyni_transcript_squeeze_point_device": 5, "toyni_poly_eval_dz_device": 8, "toyni_fib_deep_dz_device": 11,
          "toyni_fri_phase_roots_device": 5}


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def test_symbols_are_exported_and_bound_with_the_headers_parameter_counts(ta):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "toyni_hip.h")).read()
    for name, nargs in COUNTS.items():
        assert name in ta._lib.SIGNATURES and hasattr(ta._lib.lib, name)
        f = getattr(ta._lib.lib, name)
        assert f.argtypes == ta._lib.SIGNATURES[name][1] and len(f.argtypes) == nargs and f.restype is ctypes.c_int
        decl = header.split("int " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == nargs, (name, decl)
    assert ta._lib.error_string(E_INVALID_SIZE) and ta._lib.lib.toyni_fri_phase_roots_device(0x1000, 3, 1, 0x1000, None) == E_INVALID_SIZE
    for name in ("mask_poly_device", "poly_eval_dz_device", "fib_deep_dz_device", "fri_phase_roots_device"):
        assert hasattr(ta.prover, name)
    assert hasattr(ta.prover.DeviceTranscript, "squeeze_point")


def _untouched(buffers):
    for name, g in buffers:
        g.check(name)
        assert (g.download(np.uint8) == 0xA5).all(), name


def test_every_refusal_of_the_mask_the_point_and_the_roots_leaves_everything_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    tr, coeffs, out, levels = Guarded(mem, 1024, seed=1), Guarded(mem, 4 * 512, seed=2), Guarded(mem, 4 * 64, seed=3), Guarded(mem, 32 * 31, seed=4)
    key = (ctypes.c_uint8 * 32)(*range(32))
    try:
        mask = lambda c=coeffs.ptr, n=256, d=140, k=key, nonce=1: lib.toyni_mask_poly_device(c, n, d, k, nonce, None)
        point = lambda t=tr.ptr, log_n=11, shift=7, z=out.ptr: lib.toyni_transcript_squeeze_point_device(t, log_n, shift, z, None)
        roots = lambda lv=levels.ptr, m=16, rounds=4, o=out.ptr: lib.toyni_fri_phase_roots_device(lv, m, rounds, o, None)
        nulls = {"mask coeffs": mask(c=None), "mask key": mask(k=None), "point tr": point(t=None), "point z": point(z=None),
                 "roots levels": roots(lv=None), "roots out": roots(o=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        ranges = {"mask degree 0": mask(d=0), "mask degree 4097": mask(d=4097), "mask n 0": mask(n=0), "mask coeffs + 2": mask(c=coeffs.ptr + 2),
                  "point log_N 28": point(log_n=28), "point shift 0": point(shift=0), "point shift p": point(shift=P), "point shift 2^32 - 1": point(shift=0xFFFFFFFF),
                  "point tr + 4": point(t=tr.ptr + 4), "point tr + 8": point(t=tr.ptr + 8), "point z + 2": point(z=out.ptr + 2),
                  "roots rounds 65": roots(m=1 << 32, rounds=65), "roots rounds beyond one leaf": roots(m=16, rounds=6),
                  "roots levels + 8": roots(lv=levels.ptr + 8), "roots out + 2": roots(o=out.ptr + 2)}
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        sizes = {"roots m 0": roots(m=0), "roots m 24": roots(m=24), "roots m 2^33": roots(m=1 << 33)}
        assert all(rc == E_INVALID_SIZE for rc in sizes.values()), sizes
        assert roots(rounds=0) == 0                       # nothing to do: no refusal, nothing enqueued
        _untouched((("tr", tr), ("coeffs", coeffs), ("out", out), ("levels", levels)))
    finally:
        for g in (tr, coeffs, out, levels):
            g.free()


def test_every_refusal_of_the_evaluation_leaves_everything_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    coeffs, z, out, fake_ctx = Guarded(mem, 4 * 64, seed=1), Guarded(mem, 4, seed=2), Guarded(mem, 16, seed=3), Guarded(mem, 4096, seed=4)
    try:
        def run(ctx=fake_ctx.ptr, c=coeffs.ptr, ncoeffs=64, dz=z.ptr, mults=(1, 5), npoints=None, o=out.ptr, null_mults=False):
            m = np.array(mults, dtype=np.uint32)
            return lib.toyni_poly_eval_dz_device(ctx, c, ncoeffs, dz, None if null_mults else m.ctypes.data, len(mults) if npoints is None else npoints, o, None)

        nulls = {"ctx": run(ctx=None), "d_coeffs": run(c=None), "d_z": run(dz=None), "mults": run(null_mults=True), "d_out": run(o=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        ranges = {"npoints 0": run(npoints=0), "npoints 5": run(mults=(1,) * 5), "multiplier p": run(mults=(1, P)), "multiplier 2^32 - 1": run(mults=(0xFFFFFFFF,)),
                  "d_coeffs + 2": run(c=coeffs.ptr + 2), "d_out + 1": run(o=out.ptr + 1), "d_z + 2": run(dz=z.ptr + 2)}
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        _untouched((("coeffs", coeffs), ("z", z), ("out", out), ("ctx", fake_ctx)))
    finally:
        for g in (coeffs, z, out, fake_ctx):
            g.free()


def test_every_refusal_of_the_deep_layer_that_needs_no_context_leaves_everything_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    trace, quot, out, z, ood, chk, fake_ctx = (Guarded(mem, nbytes, seed=k) for k, nbytes in enumerate((4 * 64, 4 * 64, 4 * 64, 4, 16, 4, 4096), start=1))
    try:
        def run(ctx=fake_ctx.ptr, t=trace.ptr, q=quot.ptr, o=out.ptr, shift=7, dz=z.ptr, dood=ood.ptr, n=32, c=chk.ptr):
            return lib.toyni_fib_deep_dz_device(ctx, t, q, o, 1, shift, dz, dood, n, c, None)

        nulls = {"ctx": run(ctx=None), "d_trace_lde": run(t=None), "d_q_evals": run(q=None), "d_out": run(o=None), "d_z": run(dz=None), "d_ood": run(dood=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        ranges = {"shift 0": run(shift=0), "shift p": run(shift=P), "trace_len 0": run(n=0), "trace_len 24": run(n=24), "trace_len 2^28": run(n=1 << 28),
                  "d_z + 2": run(dz=z.ptr + 2), "d_ood + 1": run(dood=ood.ptr + 1), "d_check + 2": run(c=chk.ptr + 2)}
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        _untouched((("trace", trace), ("quot", quot), ("out", out), ("z", z), ("ood", ood), ("check", chk), ("ctx", fake_ctx)))
    finally:
        for g in (trace, quot, out, z, ood, chk, fake_ctx):
            g.free()


def test_the_wrappers_hand_refusals_through_as_toyni_errors(ta):
    fake = ta.prover.DeviceTranscript.__new__(ta.prover.DeviceTranscript)
    fake.ptr, fake._staged = 0, []
    for call in (lambda: fake.squeeze_point(0x1000, 11, 7), lambda: ta.prover.mask_poly_device(0, 64, 140, bytes(32)),
                 lambda: ta.prover.fri_phase_roots_device(0, 16, 2, 0x1000)):
        with pytest.raises(ta._lib.ToyniError) as e:
            call()
        assert e.value.status == E_NULL
    fake.ptr = 0x1000
    for call in (lambda: fake.squeeze_point(0x2000, 28, 7), lambda: ta.prover.mask_poly_device(0x1000, 64, 0, bytes(32))):
        with pytest.raises(ta._lib.ToyniError) as e:
            call()
        assert e.value.status == E_RANGE
    fake.ptr = 0
