"""The device transcript and the commit phases on it (include/toyni_hip.h 3l): exported with the header's parameter counts, bound in the
Python package, and every refusal the host decides before anything is enqueued, from an otherwise valid call with the outputs
untouched.  The pointers are host stand-in memory (tests/guarded.py HostMem), the context a block of it that a call which passed its
checks would misread -- none does.  "m0 exceeds the context's n" needs a real context and a device.  No compute (no GPU here)."""
import ctypes
import os

import numpy as np
import pytest

from guarded import Guarded, HostMem, P

E_INVALID_SIZE, E_NULL, E_ZERO_INVERSE, E_RANGE = 10001, 10002, 10005, 10006
COUNTS = {"toyni_transcript_absorb_device": 4, "toyni_transcript_squeeze_device": 4, "toyni_transcript_squeeze_indices_device": 5,
          "toyni_fri_query_positions_device": 6, "toyni_fri_commit_phase_transcript_device": 11, "toyni_fri_commit_phase_transcript_ext_device": 11}


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
    assert ta._lib.SIGNATURES["toyni_fri_commit_phase_transcript_device"][1] == ta._lib.SIGNATURES["toyni_fri_commit_phase_transcript_ext_device"][1]
    assert "#define TOYNI_TRANSCRIPT_CAPACITY 1008" in header
    assert "typedef struct { uint32_t len, status, reserved[2]; uint8_t bytes[TOYNI_TRANSCRIPT_CAPACITY]; } toyni_transcript;" in header
    for name in ("DeviceTranscript", "fri_commit_phase_transcript_device", "fri_commit_phase_transcript_ext_device", "fri_query_positions_device"):
        assert hasattr(ta.prover, name)
    for method in ("from_bytes", "absorb_device", "squeeze", "squeeze_indices", "status", "download"):
        assert hasattr(ta.prover.DeviceTranscript, method)
    assert ta.prover.TRANSCRIPT_CAPACITY == 1008


def _untouched(buffers):
    for name, g in buffers:
        g.check(name)
        assert (g.download(np.uint8) == 0xA5).all(), name


def test_every_refusal_of_the_transcript_calls_leaves_everything_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    tr, data, out, idx = Guarded(mem, 1024, seed=1), Guarded(mem, 1024, word=1, seed=2), Guarded(mem, 4 * 65536, seed=3), Guarded(mem, 4 * 64, seed=4)
    try:
        absorb = lambda t=tr.ptr, d=data.ptr, n=32: lib.toyni_transcript_absorb_device(t, d, n, None)
        squeeze = lambda t=tr.ptr, o=out.ptr, n=4: lib.toyni_transcript_squeeze_device(t, o, n, None)
        indices = lambda t=tr.ptr, n=8, mx=64, o=out.ptr: lib.toyni_transcript_squeeze_indices_device(t, n, mx, o, None)
        positions = lambda i=idx.ptr, n=8, m0=64, fin=4, o=out.ptr: lib.toyni_fri_query_positions_device(i, n, m0, fin, o, None)
        nulls = {"absorb tr": absorb(t=None), "absorb bytes": absorb(d=None), "squeeze tr": squeeze(t=None), "squeeze out": squeeze(o=None),
                 "indices tr": indices(t=None), "indices out": indices(o=None), "positions idx": positions(i=None), "positions out": positions(o=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        ranges = {
            "absorb tr + 4": absorb(t=tr.ptr + 4), "absorb tr + 8": absorb(t=tr.ptr + 8), "absorb 1009": absorb(n=1009), "absorb 2^40": absorb(n=1 << 40),
            "squeeze tr + 4": squeeze(t=tr.ptr + 4), "squeeze out + 2": squeeze(o=out.ptr + 2), "squeeze 65537": squeeze(n=65537),
            "indices tr + 12": indices(t=tr.ptr + 12), "indices out + 1": indices(o=out.ptr + 1), "indices count 0": indices(n=0),
            "indices count 257": indices(n=257, mx=1 << 20), "indices max 0": indices(mx=0), "indices count > max": indices(n=9, mx=8),
            "positions idx + 2": positions(i=idx.ptr + 2), "positions out + 3": positions(o=out.ptr + 3), "positions m0 48": positions(m0=48),
            "positions m0 0": positions(m0=0), "positions final 3": positions(fin=3), "positions final 0": positions(fin=0),
            "positions m0 2^33": positions(m0=1 << 33), "positions count 65537": positions(n=65537),
        }
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        # nothing to do is no refusal and enqueues nothing (no device is needed to say so)
        assert absorb(n=0) == 0 and absorb(d=None, n=0) == 0 and squeeze(n=0) == 0 and positions(n=0) == 0 and positions(m0=4, fin=4) == 0
        assert positions(m0=4, fin=16) == 0
        _untouched((("tr", tr), ("data", data), ("out", out), ("idx", idx)))
    finally:
        for g in (tr, data, out, idx):
            g.free()


@pytest.mark.parametrize("ext", [False, True])
def test_every_refusal_of_the_phases_leaves_everything_untouched(ta, ext):
    lib = ta._lib.lib
    mem = HostMem()
    m0 = 64
    layer0, layers, salts = Guarded(mem, 16 * m0, seed=1), Guarded(mem, 16 * m0, seed=2), Guarded(mem, 16 * m0, seed=3)
    levels, fake_ctx = Guarded(mem, 32 * 2 * m0, word=1, seed=4), Guarded(mem, 4096, seed=5)
    tr, betas = Guarded(mem, 1024, seed=6), Guarded(mem, 4 * 4 * 8, seed=7)
    entry = lib.toyni_fri_commit_phase_transcript_ext_device if ext else lib.toyni_fri_commit_phase_transcript_device
    try:
        def run(ctx=fake_ctx.ptr, l0=layer0.ptr, m0=m0, x0=7, final=4, s=salts.ptr, t=tr.ptr, ls=layers.ptr, lv=levels.ptr, b=betas.ptr):
            return entry(ctx, l0, m0, x0, final, s, t, ls, lv, b, None)

        nulls = {"ctx": run(ctx=None), "d_layer0": run(l0=None), "d_tr": run(t=None), "d_layers": run(ls=None), "d_levels": run(lv=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        sizes = {"m0 48": run(m0=48), "m0 0": run(m0=0), "final 3": run(final=3), "final 0": run(final=0), "m0 63": run(m0=63)}
        assert all(rc == E_INVALID_SIZE for rc in sizes.values()), sizes
        assert run(x0=0) == (E_ZERO_INVERSE if ext else E_RANGE)              # as the callback call of the same element type
        ranges = {"x0 p": run(x0=P), "x0 2^32 - 1": run(x0=0xFFFFFFFF), "d_levels + 8": run(lv=levels.ptr + 8), "d_salts + 12": run(s=salts.ptr + 12),
                  "d_tr + 4": run(t=tr.ptr + 4), "d_tr + 8": run(t=tr.ptr + 8), "d_betas + 2": run(b=betas.ptr + 2)}
        if ext:
            ranges.update({"d_layer0 + 4": run(l0=layer0.ptr + 4), "d_layers + 8": run(ls=layers.ptr + 8)})
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        _untouched((("layer0", layer0), ("layers", layers), ("salts", salts), ("levels", levels), ("ctx", fake_ctx), ("tr", tr), ("betas", betas)))
    finally:
        for g in (layer0, layers, salts, levels, fake_ctx, tr, betas):
            g.free()
