"""The out-of-domain evaluation at Ext points and the Ext DEEP combination (include/toyni_hip.h 3h): exported, bound, the term struct
has the header's size and field order, and a null context is refused before any device is touched.  No compute (no GPU here)."""
import ctypes

import numpy as np
import pytest

E_NULL = 10002


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def test_symbols_are_exported_and_bound(ta):
    for name in ("toyni_poly_eval_ext_batch_device", "toyni_deep_combine_ext_device"):
        assert name in ta._lib.SIGNATURES and hasattr(ta._lib.lib, name)
        assert getattr(ta._lib.lib, name).argtypes == ta._lib.SIGNATURES[name][1]
    for name in ("poly_eval_ext_batch_device", "deep_combine_ext_device", "deep_ext_terms", "DeepExtTerm"):
        assert hasattr(ta.prover, name)


def test_term_struct_is_ten_words_in_the_headers_order(ta):
    assert ctypes.sizeof(ta.prover.DeepExtTerm) == 40
    assert [f[0] for f in ta.prover.DeepExtTerm._fields_] == ["column", "rotation", "alpha", "value"]
    t = ta.prover.deep_ext_terms([3, 0], [2, 1], [[5, 6, 7, 8], [9, 10, 11, 12]], [[13, 14, 15, 16], [17, 18, 19, 20]])
    assert len(t) == 2 and ctypes.sizeof(t) == 80
    assert np.frombuffer(t, dtype=np.uint32).tolist() == [3, 2, 5, 6, 7, 8, 13, 14, 15, 16, 0, 1, 9, 10, 11, 12, 17, 18, 19, 20]
    assert len(ta.prover.deep_ext_terms([], [], [], [])) == 0


def test_null_context_is_refused_without_a_device(ta):
    lib = ta._lib.lib
    pts = np.array([1, 2, 3, 4, 5, 6, 7, 8], dtype=np.uint32)
    assert lib.toyni_poly_eval_ext_batch_device(None, 0x1000, 4, 4, 2, pts.ctypes.data, 2, 0x2000, None) == E_NULL
    t = ta.prover.deep_ext_terms([0], [0], [[1, 0, 0, 0]], [[1, 0, 0, 0]])
    z = np.array([3, 1, 0, 0], dtype=np.uint32)
    assert lib.toyni_deep_combine_ext_device(None, 0x1000, 1, 8, 0, 7, z.ctypes.data, t, 1, 0, 0x2000, None) == E_NULL
