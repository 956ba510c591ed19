"""The calls of include/toyni_hip.h 3o: exported with the header's parameter counts, bound in the Python package, the slot struct in
the header's order, and every refusal the host decides before anything is enqueued, from an otherwise valid call with the outputs and
a stand-in transcript untouched.  The pointers are host stand-in memory (tests/guarded.py HostMem), the context a block of it that a
call which passed its checks would misread -- none does.  The range refusals of toyni_deep_combine_ext_dz_device read the context's
size first, as those of toyni_deep_combine_ext_device do: they need a real context and are in tests/test_gpu_dz.py.  No compute (no
GPU here)."""
import ctypes
import os

import numpy as np
import pytest

from guarded import Guarded, HostMem, P

E_NULL, E_RANGE = 10002, 10006
COUNTS = {"toyni_transcript_squeeze_ext_point_device": 3, "toyni_transcript_absorb_fields_device": 4, "toyni_poly_eval_ext_batch_dz_device": 10,
          "toyni_deep_combine_ext_dz_device": 14, "toyni_query_rows_device": 7}


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
    assert "typedef struct { uint32_t column, rotation, alpha_index, value_index; } toyni_deep_ext_slot;" in header
    for name in ("poly_eval_ext_batch_dz_device", "deep_combine_ext_dz_device", "deep_ext_slots", "DeepExtSlot", "query_rows_device"):
        assert hasattr(ta.prover, name)
    for method in ("squeeze_ext_point", "absorb_fields"):
        assert hasattr(ta.prover.DeviceTranscript, method)


def test_slot_struct_is_four_words_in_the_headers_order(ta):
    assert ctypes.sizeof(ta.prover.DeepExtSlot) == 16
    assert [f[0] for f in ta.prover.DeepExtSlot._fields_] == ["column", "rotation", "alpha_index", "value_index"]
    s = ta.prover.deep_ext_slots([3, 0], [2, 1], [5, 6], [7, 8])
    assert len(s) == 2 and np.frombuffer(s, dtype=np.uint32).tolist() == [3, 2, 5, 7, 0, 1, 6, 8]
    assert len(ta.prover.deep_ext_slots([], [], [], [])) == 0


def _untouched(buffers):
    for name, g in buffers:
        g.check(name)
        assert (g.download(np.uint8) == 0xA5).all(), name


def test_every_refusal_of_the_transcript_and_row_calls_leaves_everything_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    tr, words, out, idx = Guarded(mem, 1024, seed=1), Guarded(mem, 4 * 128, seed=2), Guarded(mem, 4 * 8 * 64, seed=3), Guarded(mem, 4 * 64, seed=4)
    try:
        point = lambda t=tr.ptr, z=out.ptr: lib.toyni_transcript_squeeze_ext_point_device(t, z, None)
        fields = lambda t=tr.ptr, w=words.ptr, n=24: lib.toyni_transcript_absorb_fields_device(t, w, n, None)

        def rows(i=idx.ptr, count=8, n=64, offsets=(0, 4), noffsets=None, o=out.ptr, null_offsets=False):
            off = np.array(offsets, dtype=np.uint32)
            return lib.toyni_query_rows_device(i, count, n, None if null_offsets else off.ctypes.data, len(offsets) if noffsets is None else noffsets, o, None)

        nulls = {"point tr": point(t=None), "point z": point(z=None), "fields tr": fields(t=None), "fields words": fields(w=None),
                 "rows idx": rows(i=None), "rows out": rows(o=None), "rows offsets": rows(null_offsets=True)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        ranges = {
            "point tr + 4": point(t=tr.ptr + 4), "point tr + 8": point(t=tr.ptr + 8), "point z + 2": point(z=out.ptr + 2),
            "fields tr + 4": fields(t=tr.ptr + 4), "fields words + 1": fields(w=words.ptr + 1), "fields 127": fields(n=127), "fields 2^40": fields(n=1 << 40),
            "rows idx + 2": rows(i=idx.ptr + 2), "rows out + 3": rows(o=out.ptr + 3), "rows noffsets 0": rows(noffsets=0),
            "rows noffsets 9": rows(offsets=(0,) * 9), "rows n 0": rows(n=0, offsets=(0,)), "rows n 2^32 + 1": rows(n=(1 << 32) + 1),
            "rows offset n": rows(offsets=(0, 64)), "rows offset 2^32 - 1": rows(offsets=(0xFFFFFFFF,)), "rows count 65537": rows(count=65537),
        }
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        # nothing to do is no refusal and enqueues nothing (no device is needed to say so)
        assert fields(n=0) == 0 and fields(w=None, n=0) == 0 and rows(count=0) == 0 and rows(count=0, n=1 << 32, offsets=((1 << 32) - 1,)) == 0
        _untouched((("tr", tr), ("words", words), ("out", out), ("idx", idx)))
    finally:
        for g in (tr, words, out, idx):
            g.free()


def test_every_refusal_of_the_evaluation_leaves_everything_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    coeffs, z, out, fake_ctx = Guarded(mem, 4 * 3 * 64, seed=1), Guarded(mem, 16, seed=2), Guarded(mem, 4 * 4 * 3 * 4, seed=3), Guarded(mem, 4096, seed=4)
    try:
        def run(ctx=fake_ctx.ptr, c=coeffs.ptr, ncoeffs=64, stride=64, batch=3, dz=z.ptr, mults=(1, 5), npoints=None, o=out.ptr, null_mults=False):
            m = np.array(mults, dtype=np.uint32)
            return lib.toyni_poly_eval_ext_batch_dz_device(ctx, c, ncoeffs, stride, batch, dz, None if null_mults else m.ctypes.data,
                                                           len(mults) if npoints is None else npoints, o, None)

        nulls = {"ctx": run(ctx=None), "d_coeffs": run(c=None), "d_z": run(dz=None), "mults": run(null_mults=True), "d_out": run(o=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        ranges = {"npoints 0": run(npoints=0), "npoints 5": run(mults=(1,) * 5), "multiplier p": run(mults=(1, P)), "multiplier 2^32 - 1": run(mults=(0xFFFFFFFF,)),
                  "stride < ncoeffs": run(stride=63), "batch 2^32": run(batch=1 << 32), "d_coeffs + 2": run(c=coeffs.ptr + 2), "d_out + 1": run(o=out.ptr + 1),
                  "d_z + 2": run(dz=z.ptr + 2)}
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        assert run(batch=0) == 0                          # nothing to do: no refusal, nothing enqueued, the context not touched
        _untouched((("coeffs", coeffs), ("z", z), ("out", out), ("ctx", fake_ctx)))
    finally:
        for g in (coeffs, z, out, fake_ctx):
            g.free()


def test_null_pointers_of_the_combination_are_refused_without_a_device(ta):
    lib = ta._lib.lib
    mem = HostMem()
    values, z, al, cl, out, fake_ctx = (Guarded(mem, nbytes, seed=k) for k, nbytes in enumerate((4 * 64, 16, 64, 64, 16 * 64, 4096), start=1))
    try:
        slots = ta.prover.deep_ext_slots([0, 0], [0, 1], [0, 1], [1, 0])

        def run(ctx=fake_ctx.ptr, v=values.ptr, dz=z.ptr, a=al.ptr, c=cl.ptr, s=slots, n=2, o=out.ptr):
            return lib.toyni_deep_combine_ext_dz_device(ctx, v, 1, 64, 1, 7, dz, a, c, s, n, 0, o, None)

        nulls = {"ctx": run(ctx=None), "d_values": run(v=None), "d_z": run(dz=None), "d_alphas": run(a=None), "d_claims": run(c=None),
                 "slots": run(s=None), "d_out": run(o=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        _untouched((("values", values), ("z", z), ("alphas", al), ("claims", cl), ("out", out), ("ctx", fake_ctx)))
    finally:
        for g in (values, z, al, cl, out, fake_ctx):
            g.free()


def test_the_wrappers_hand_refusals_through_as_toyni_errors(ta):
    fake = ta.prover.DeviceTranscript.__new__(ta.prover.DeviceTranscript)
    fake.ptr, fake._staged = 0, []
    for call in (lambda: fake.squeeze_ext_point(0x1000), lambda: fake.absorb_fields(0x1000, 4),
                 lambda: ta.prover.query_rows_device(0, 4, 64, [0, 1], 0x1000)):
        with pytest.raises(ta._lib.ToyniError) as e:
            call()
        assert e.value.status == E_NULL
    fake.ptr = 0x1000
    with pytest.raises(ta._lib.ToyniError) as e:
        fake.absorb_fields(0x2000, 127)
    assert e.value.status == E_RANGE
    with pytest.raises(ta._lib.ToyniError) as e:
        ta.prover.query_rows_device(0x1000, 4, 64, [64], 0x2000)
    assert e.value.status == E_RANGE
    fake.ptr = 0
