"""The proof-of-work calls (include/toyni_hip.h 3n): exported with the header's parameter counts and bound in the Python package;
toyni_pow_check_host -- plain host code, what a verifier calls -- against tests/pow_model.py (hashlib) on the checked table of the
issue, on nonce +- 1 and on long states; every refusal either call decides on the host, with the outputs and a stand-in transcript
(tests/guarded.py HostMem) untouched; the Python wrappers.  No device is needed, and none is used."""
import ctypes
import os

import numpy as np
import pytest

import pow_model as pm
from guarded import Guarded, HostMem

E_NULL, E_RANGE = 10002, 10006
COUNTS = {"toyni_transcript_grind_device": 6, "toyni_pow_check_host": 5}
# the table of the issue: recomputed with the model below, never used as the expectation
TABLE = {"n=0": (1, 477, 11961, 31429), "toyni-stark-v1": (0, 153, 439, 16322), "n=32": (0, 403, 2983, 55645), "n=47": (4, 36, 855, 279941),
         "n=48": (0, 691, 2997, 43596), "n=55": (1, 517, 9790, 9790), "n=56": (0, 19, 201, 16475), "n=63": (1, 185, 5878, 23712),
         "n=64": (0, 46, 34895, 52126), "n=96": (3, 36, 7238, 11004), "n=119": (1, 143, 4263, 98510), "n=120": (1, 175, 2375, 9581),
         "n=1000": (0, 800, 7286, 260843)}


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def host_check(lib, state, nonce, bits):
    out = ctypes.c_int(-7)
    buf = (ctypes.c_uint8 * len(state)).from_buffer_copy(state) if state else None
    rc = lib.toyni_pow_check_host(buf, len(state), nonce, bits, ctypes.byref(out))
    return rc, out.value


def test_symbols_are_exported_and_bound_with_the_headers_parameter_counts(ta):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "toyni_hip.h")).read()
    for name, nargs in COUNTS.items():
        assert name in ta._lib.SIGNATURES and hasattr(ta._lib.lib, name)
        f = getattr(ta._lib.lib, name)
        assert f.argtypes == ta._lib.SIGNATURES[name][1] and len(f.argtypes) == nargs and f.restype is ctypes.c_int
        decl = header.split("int " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == nargs, (name, decl)
    assert "#define TOYNI_POW_MAX_BITS 32" in header and "#define TOYNI_POW_MAX_LOG_TRIES 40" in header
    assert header.index(" 3m. ") < header.index(" 3n. ") < header.index("int toyni_transcript_grind_device(")
    assert ta._lib.SIGNATURES["toyni_transcript_grind_device"][1][2] is ctypes.c_uint64          # start: 64 bits, whatever size_t is
    assert hasattr(ta.prover.DeviceTranscript, "grind") and ta.pow_check is ta.prover.pow_check
    assert (ta.prover.POW_MAX_BITS, ta.prover.POW_MAX_LOG_TRIES) == (32, 40)
    # the window a Python caller gets without naming one is tied to the bits: a failing call must not hash 2^40 candidates by default
    assert [ta.prover.pow_default_log_tries(b) for b in (0, 8, 16, 20, 28, 31, 32)] == [8, 16, 24, 28, 36, 39, 40]


def test_the_models_answers_are_the_checked_table():
    # the model, not the library: the numbers the issue records came from hashlib, and the model must still say so
    for name, state in pm.table_states():
        assert tuple(pm.must_grind(state, bits) for bits in (1, 8, 12, 16)) == TABLE[name], name
    start = (1 << 32) - 100
    assert pm.must_grind(pm.pattern(64, 3), 8, start) == start + 232 and pm.must_grind(pm.pattern(64, 3), 12, start) == start + 3345
    assert pm.grind(pm.pattern(64, 9), 32, 0, 1 << 10) is None and pm.grind(pm.pattern(64, 9), 24, 0, 1 << 12) is None


def test_the_host_check_is_the_models_accept(ta):
    lib = ta._lib.lib
    seen = {0: 0, 1: 0}
    for name, state in pm.table_states():
        for bits in (1, 8, 12, 16):
            hit = pm.must_grind(state, bits)
            for nonce in sorted({hit, hit + 1, max(hit - 1, 0)}):
                for b in sorted({0, bits - 1, bits, bits + 1}):
                    want = pm.accept(state, nonce, b)
                    assert host_check(lib, state, nonce, b) == (0, int(want)), (name, nonce, b)
                    assert ta.pow_check(state, nonce, b) is want
                    seen[int(want)] += 1
            assert host_check(lib, state, hit, bits) == (0, 1)
    assert seen[0] > 100 and seen[1] > 100
    # nonces whose eight bytes all differ, the top of the range, and every bit count on one state
    s = pm.pattern(119, 7)
    for nonce in (0x0807060504030201, 0xF1E2D3C4B5A69788, (1 << 64) - 1, 1 << 63, (1 << 32) - 1, 1 << 32):
        for bits in range(0, 33):
            assert host_check(lib, s, nonce, bits) == (0, int(pm.accept(s, nonce, bits))), (nonce, bits)
    # the call is not bound to the transcript's capacity, nor to a tail of any particular length
    for n in (1009, 4096, 4096 + 47, 4096 + 48, 4096 + 55, 4096 + 56, 4096 + 63, 70001):
        s = pm.pattern(n, n)
        hit = pm.must_grind(s, 8)
        assert host_check(lib, s, hit, 8) == (0, 1) and host_check(lib, s, hit + 1, 8) == (0, int(pm.accept(s, hit + 1, 8))), n
    # 32 bits: a digest that starts with four zero bytes is out of a test's reach; what can be said is that near misses are refused
    hit = pm.must_grind(pm.START_STATE, 16)
    assert host_check(lib, pm.START_STATE, hit, 32) == (0, 0) and host_check(lib, pm.START_STATE, hit, 16) == (0, 1)


def test_every_host_side_refusal_leaves_everything_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    tr, nonce = Guarded(mem, 1024, seed=1), Guarded(mem, 64, seed=2)
    try:
        grind = lambda t=tr.ptr, bits=8, start=0, lt=20, n=nonce.ptr: lib.toyni_transcript_grind_device(t, bits, start, lt, n, None)
        nulls = {"d_tr": grind(t=None), "d_nonce": grind(n=None), "both": grind(t=None, n=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        top = (1 << 64) - 1
        ranges = {"d_tr + 4": grind(t=tr.ptr + 4), "d_tr + 8": grind(t=tr.ptr + 8), "d_nonce + 4": grind(n=nonce.ptr + 4), "d_nonce + 1": grind(n=nonce.ptr + 1),
                  "bits 33": grind(bits=33), "bits 2^31": grind(bits=1 << 31), "log_tries 41": grind(lt=41), "log_tries 64": grind(lt=64),
                  "log_tries 2^31": grind(lt=1 << 31),
                  "start 2^64 - 1, 2 tries": grind(start=top, lt=1), "start 2^64 - 2^20 + 1": grind(start=top - (1 << 20) + 2, lt=20),
                  "start 2^64 - 2^40 + 1": grind(start=(1 << 64) - (1 << 40) + 1, lt=40)}
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        for g, name in ((tr, "tr"), (nonce, "nonce")):
            g.check(name)
            assert (g.download(np.uint8) == 0xA5).all(), name
        # the host check: null arguments, bits out of range -- `accepted` keeps what it held
        out = ctypes.c_int(-7)
        buf = (ctypes.c_uint8 * 4)(1, 2, 3, 4)
        assert lib.toyni_pow_check_host(buf, 4, 0, 8, None) == E_NULL
        assert lib.toyni_pow_check_host(None, 4, 0, 8, ctypes.byref(out)) == E_NULL and out.value == -7
        assert lib.toyni_pow_check_host(buf, 4, 0, 33, ctypes.byref(out)) == E_RANGE and out.value == -7
        assert lib.toyni_pow_check_host(buf, 4, 0, 1 << 31, ctypes.byref(out)) == E_RANGE and out.value == -7
        assert lib.toyni_pow_check_host(None, 0, 5, 0, ctypes.byref(out)) == 0 and out.value == 1            # a null state of length 0 is the empty state
        assert lib.toyni_pow_check_host(None, 0, 477, 8, ctypes.byref(out)) == 0 and out.value == int(pm.accept(b"", 477, 8)) == 1
        assert bytes(buf) == b"\x01\x02\x03\x04"
    finally:
        tr.free()
        nonce.free()


def test_the_python_wrappers_refuse_what_the_header_refuses(ta):
    with pytest.raises(ValueError):
        ta.pow_check(b"abc", 0, 33)
    with pytest.raises(ValueError):
        ta.pow_check(b"abc", 1 << 64, 8)
    with pytest.raises(ValueError):
        ta.pow_check(b"abc", -1, 8)
    assert ta.pow_check(b"", 477, 8) is True and ta.pow_check(bytearray(b""), 476, 8) is pm.accept(b"", 476, 8)
    # DeviceTranscript.grind hands the arguments through: the host refusals surface as ToyniError with the header's code, before a
    # device is touched (an object with a stand-in pointer; no allocation is made)
    mem = HostMem()
    tr, nonce = Guarded(mem, 1024, seed=3), Guarded(mem, 8, seed=4)
    try:
        fake = ta.prover.DeviceTranscript.__new__(ta.prover.DeviceTranscript)
        fake.ptr, fake._staged = tr.ptr, []
        for kwargs in ({"bits": 33}, {"bits": 8, "log_tries": 41}, {"bits": 8, "start": (1 << 64) - 1, "log_tries": 1}):
            with pytest.raises(ta._lib.ToyniError) as e:
                fake.grind(nonce.ptr, **kwargs)
            assert e.value.status == E_RANGE
        with pytest.raises(ta._lib.ToyniError) as e:
            fake.grind(0, 8)
        assert e.value.status == E_NULL
        fake.ptr = 0                                       # nothing of the stand-in is the object's to free
        assert (tr.download(np.uint8) == 0xA5).all() and (nonce.download(np.uint8) == 0xA5).all()
    finally:
        tr.free()
        nonce.free()
