"""The Ext fold-and-commit round and the Ext commit phase (include/toyni_hip.h 3j): exported with the header's parameter counts,
bound in the Python package, and every refusal of the header that the arguments alone decide, from an otherwise valid call with the
outputs untouched.  Those refusals come before the context is read, so they can be asked for without a device: the pointers are host
stand-in memory (tests/guarded.py HostMem), the context a block of it that a call which passed its checks would misread -- none
does.  "m exceeds the context's n" needs a real context and belongs to tests/test_gpu_fold_commit_ext.py.  No compute (no GPU here)."""
import ctypes
import os

import numpy as np
import pytest

from guarded import Guarded, HostMem, P

E_INVALID_SIZE, E_NULL, E_ODD, E_ZERO_INVERSE, E_RANGE = 10001, 10002, 10003, 10005, 10006


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def test_symbols_are_exported_and_bound_with_the_headers_parameter_counts(ta):
    counts = {"toyni_fri_fold_commit_ext_device": 9, "toyni_fri_commit_phase_ext_device": 13}
    for name, nargs in counts.items():
        assert name in ta._lib.SIGNATURES and hasattr(ta._lib.lib, name)
        f = getattr(ta._lib.lib, name)
        assert f.argtypes == ta._lib.SIGNATURES[name][1] and len(f.argtypes) == nargs and f.restype is ctypes.c_int
    # the same shapes as the base-field calls they mirror (beta by pointer instead of by value)
    assert len(ta._lib.SIGNATURES["toyni_fri_fold_commit_device"][1]) == 9
    assert ta._lib.SIGNATURES["toyni_fri_commit_phase_ext_device"][1] == ta._lib.SIGNATURES["toyni_fri_commit_phase_device"][1]
    for name in ("fri_fold_commit_ext_device", "fri_commit_phase_ext_device"):
        assert hasattr(ta.prover, name)
    # and the header declares them with exactly these parameter lists
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "toyni_hip.h")).read()
    for name, nargs in counts.items():
        decl = header.split("int " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == nargs, (name, decl)
    assert "typedef int (*toyni_fri_ext_challenge_fn)(void* user, unsigned round, const uint8_t* prev_root32, uint32_t beta_out[4]);" in header


def test_every_refusal_of_the_round_leaves_the_outputs_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    m = 64
    evals, out, salts = Guarded(mem, 16 * m, seed=1), Guarded(mem, 8 * m, seed=2), Guarded(mem, 16 * (m // 2), seed=3)
    levels, fake_ctx = Guarded(mem, 32 * (m - 1), word=1, seed=4), Guarded(mem, 4096, seed=5)
    beta_ok = (ctypes.c_uint32 * 4)(1, 2, 3, P - 1)
    try:
        def run(ctx=fake_ctx.ptr, e=evals.ptr, o=out.ptr, m=m, beta=beta_ok, x0=7, s=salts.ptr, lv=levels.ptr):
            return lib.toyni_fri_fold_commit_ext_device(ctx, e, o, m, beta, x0, s, lv, None)

        nulls = {"ctx": run(ctx=None), "d_evals": run(e=None), "d_out": run(o=None), "beta": run(beta=None), "d_levels": run(lv=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        assert run(m=63) == E_ODD and run(m=1) == E_ODD
        assert run(x0=0) == E_ZERO_INVERSE
        bad_beta = lambda k, v: (ctypes.c_uint32 * 4)(*[v if j == k else 5 for j in range(4)])
        ranges = {
            "m 6": run(m=6), "m 48": run(m=48), "m 2^40 + 2": run(m=(1 << 40) + 2),
            "x0 p": run(x0=P), "x0 2^32 - 1": run(x0=0xFFFFFFFF),
            **{f"beta[{k}] p": run(beta=bad_beta(k, P)) for k in range(4)}, "beta[2] 2^32 - 1": run(beta=bad_beta(2, 0xFFFFFFFF)),
            "d_evals + 4": run(e=evals.ptr + 4), "d_evals + 8": run(e=evals.ptr + 8), "d_out + 4": run(o=out.ptr + 4), "d_out + 12": run(o=out.ptr + 12),
            "d_levels + 8": run(lv=levels.ptr + 8), "d_salts + 4": run(s=salts.ptr + 4),
        }
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        # nothing to do is no refusal, and writes nothing; NULL salts are the unsalted tree, no refusal either
        assert run(m=0) == 0 and run(m=0, s=None) == 0
        for name, g in (("evals", evals), ("out", out), ("salts", salts), ("levels", levels), ("ctx", fake_ctx)):
            g.check(name)
            assert (g.download(np.uint8) == 0xA5).all(), name
    finally:
        for g in (evals, out, salts, levels, fake_ctx):
            g.free()


def test_every_refusal_of_the_phase_leaves_the_outputs_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    m0 = 64
    layer0, layers, salts = Guarded(mem, 16 * m0, seed=1), Guarded(mem, 16 * m0, seed=2), Guarded(mem, 16 * m0, seed=3)
    levels, fake_ctx = Guarded(mem, 32 * 2 * m0, word=1, seed=4), Guarded(mem, 4096, seed=5)
    roots, rounds = Guarded(mem, 32 * 8, word=1, seed=6), Guarded(mem, 4, seed=7)
    calls = []

    def _cb(user, rnd, root, beta):
        calls.append(rnd)
        return 77

    cb = ctypes.cast(ta._lib.FRI_EXT_CHALLENGE_FN(_cb), ctypes.c_void_p)
    try:
        def run(ctx=fake_ctx.ptr, l0=layer0.ptr, m0=m0, x0=7, final=4, s=salts.ptr, ch=cb, ls=layers.ptr, lv=levels.ptr):
            return lib.toyni_fri_commit_phase_ext_device(ctx, l0, m0, x0, final, s, ch, None, ls, lv, roots.ptr,
                                                         ctypes.cast(rounds.ptr, ctypes.POINTER(ctypes.c_uint)), None)

        nulls = {"ctx": run(ctx=None), "d_layer0": run(l0=None), "callback": run(ch=None), "d_layers": run(ls=None), "d_levels": run(lv=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        sizes = {"m0 48": run(m0=48), "m0 0": run(m0=0), "final 3": run(final=3), "final 0": run(final=0), "m0 63": run(m0=63)}
        assert all(rc == E_INVALID_SIZE for rc in sizes.values()), sizes
        assert run(x0=0) == E_ZERO_INVERSE
        ranges = {"x0 p": run(x0=P), "x0 2^32 - 1": run(x0=0xFFFFFFFF), "d_layer0 + 4": run(l0=layer0.ptr + 4), "d_layers + 8": run(ls=layers.ptr + 8),
                  "d_levels + 8": run(lv=levels.ptr + 8), "d_salts + 12": run(s=salts.ptr + 12)}
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        assert not calls                                                       # a refused call never reaches the transcript
        for name, g in (("layer0", layer0), ("layers", layers), ("salts", salts), ("levels", levels), ("ctx", fake_ctx), ("roots", roots),
                        ("rounds", rounds)):
            g.check(name)
            assert (g.download(np.uint8) == 0xA5).all(), name
    finally:
        for g in (layer0, layers, salts, levels, fake_ctx, roots, rounds):
            g.free()
