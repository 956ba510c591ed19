"""toyni_air_quotient_ext_device (include/toyni_hip.h 3k): exported and bound, the refusals that need no device, and the helper that
turns the Ext challenges of emit_ext constraints into the call's weight table.  CPU only."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import ext_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2013265921
E_NULL = 10002
NAME = "toyni_air_quotient_ext_device"


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def test_symbol_is_exported_and_bound_as_the_header_declares(ta):
    f = getattr(ta._lib.lib, NAME)
    assert NAME in ta._lib.SIGNATURES and f.argtypes == ta._lib.SIGNATURES[NAME][1] and f.restype is ctypes.c_int
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "toyni_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % NAME, header, flags=re.S)
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["toyni_ntt_ctx* ctx", "const toyni_air_program* prog", "const toyni_air_matrix* mats", "size_t nmats", "unsigned log_blowup",
                      "uint32_t shift", "const uint32_t* weights4", "size_t nweights", "uint32_t* d_c_out", "uint32_t* d_q_out", "size_t out_stride",
                      "int accumulate", "void* stream"]
    assert len(f.argtypes) == len(params)
    assert f.argtypes[10] is ctypes.c_size_t and f.argtypes[11] is ctypes.c_int            # out_stride, accumulate
    limit = int(re.search(r"#define TOYNI_AIR_EXT_INLINE_WEIGHTS (\d+)", header).group(1))
    assert limit == ta.prover.AIR_EXT_INLINE_WEIGHTS and 1 <= limit <= 64                  # at most 1 KiB of kernel arguments
    kernels = open(os.path.join(ROOT, "toyni_amd", "csrc", "prover_kernels.hpp")).read()
    assert int(re.search(r"AIR_EXT_INLINE_WEIGHTS = (\d+);", kernels).group(1)) == limit


def test_the_binding_and_its_exports(ta):
    sig = inspect.signature(ta.prover.air_quotient_ext_device)
    assert list(sig.parameters) == ["ctx", "prog", "mats", "log_blowup", "shift", "weights4", "d_q_out", "out_stride", "d_c_out", "accumulate", "stream"]
    assert sig.parameters["d_c_out"].default == 0 and sig.parameters["accumulate"].default is False and sig.parameters["stream"].default is None
    assert ta.air_quotient_ext_device is ta.prover.air_quotient_ext_device and ta.air_ext_weights is ta.prover.air_ext_weights


def test_null_arguments_are_refused_before_a_device_is_looked_for(ta):
    lib = ta._lib.lib
    w = (ctypes.c_uint32 * 4)(1, 0, 0, 0)
    ctx, prog, q = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)      # never dereferenced: a null sibling refuses first
    assert lib.toyni_air_quotient_ext_device(None, None, None, 0, 0, 7, w, 1, None, None, 8, 0, None) == E_NULL
    assert lib.toyni_air_quotient_ext_device(None, prog, None, 0, 0, 7, w, 1, None, q, 8, 0, None) == E_NULL       # context
    assert lib.toyni_air_quotient_ext_device(ctx, None, None, 0, 0, 7, w, 1, None, q, 8, 0, None) == E_NULL        # program
    assert lib.toyni_air_quotient_ext_device(ctx, prog, None, 0, 0, 7, None, 1, None, q, 8, 0, None) == E_NULL     # weights4
    assert lib.toyni_air_quotient_ext_device(ctx, prog, None, 0, 0, 7, w, 1, None, None, 8, 0, None) == E_NULL     # d_q_out
    assert lib.toyni_air_quotient_ext_device(ctx, prog, None, 1, 0, 7, w, 1, None, q, 8, 0, None) == E_NULL        # mats with nmats > 0


def test_weight_helper_equals_the_coordinate_weights_of_the_harness(ta):
    from harness.air_ext_prover import coordinate_weights
    rng = np.random.default_rng(0xA1FA)
    for count in (1, 4, 7):
        alphas = [tuple(int(v) for v in rng.integers(0, P, 4)) for _ in range(count)]
        alphas[0] = (P - 1, 0, 1, P - 1)
        table = ta.air_ext_weights(alphas)
        assert table.shape == (4 * count, 4) and table.dtype == np.uint32
        want = coordinate_weights(alphas)                                   # [coordinate][base constraint]
        for e in range(4):
            assert [int(v) for v in table[:, e]] == [int(v) for v in want[e]], e
        for k, a in enumerate(alphas):                                      # the definition: alpha_k * X^j
            for j in range(4):
                xj = tuple(int(i == j) for i in range(4))
                assert tuple(int(v) for v in table[4 * k + j]) == tuple(em.mul(a, xj))
    with pytest.raises(ValueError):
        ta.air_ext_weights([(1, 2, 3)])
