"""The row-leaf Merkle entry points (include/toyni_hip.h 3d) refuse bad arguments before they touch a device, and their size
functions equal the formats.  No compute (no GPU here): the pointers handed over are never dereferenced by a refused call."""
import numpy as np
import pytest

E_NULL, E_RANGE = 10002, 10006
COL, ROW = 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build_hip()
    from toyni_amd import _lib
    return _lib.lib


def depth(n):
    d = 0
    while n > 1:
        n, d = (n + 1) // 2, d + 1
    return d


def test_leaf_and_record_sizes_equal_the_formats(lib):
    for width in (1, 2, 3, 4, 5, 7, 8, 13, 64, 100, 65536):
        assert lib.toyni_merkle_row_leaf_bytes(width, 1) == 16 + 8 * width
        assert lib.toyni_merkle_row_leaf_bytes(width, 0) == 8 * width
        for n in (1, 2, 3, 5, 33, 1000, 4096, 1 << 16, (1 << 21) + 1):
            d = depth(n)
            assert lib.toyni_merkle_open_rows_record_bytes(n, width) == 32 * d + 16 + 8 * width + (d + 7) // 8 * 8
    assert lib.toyni_merkle_row_leaf_bytes(1, 1) == 24 and lib.toyni_merkle_row_leaf_bytes(1, 0) == 8
    for n in (1, 2, 3, 5, 33, 1000, 4096, 1 << 16, 1 << 21):
        assert lib.toyni_merkle_open_rows_record_bytes(n, 1) == lib.toyni_merkle_open_record_bytes(n)
    assert lib.toyni_merkle_open_rows_record_bytes(0, 4) == 0


def test_layout_codes_of_the_python_package_match_the_header():
    import toyni_amd
    assert (toyni_amd.ROWS_COLUMN_MAJOR, toyni_amd.ROWS_ROW_MAJOR) == (COL, ROW)
    for name in ("RowMerkleTree", "merkle_commit_rows_device", "merkle_open_rows_device"):
        assert hasattr(toyni_amd, name)


def test_commit_rows_device_refusals_need_no_device(lib):
    # addresses that are never dereferenced: a refusal comes before anything is enqueued
    vals, salts, levels = 0x10000, 0x20000, 0x30000
    commit = lib.toyni_merkle_commit_rows_device
    assert commit(None, 8, 2, COL, 8, salts, levels, None) == E_NULL
    assert commit(vals, 8, 2, COL, 8, salts, None, None) == E_NULL
    assert commit(vals, 8, 0, COL, 8, salts, levels, None) == E_RANGE            # width 0
    assert commit(vals, 8, 65537, COL, 8, salts, levels, None) == E_RANGE        # width too large
    assert commit(vals, 8, 2, 2, 8, salts, levels, None) == E_RANGE              # unknown layout
    assert commit(vals, 8, 2, -1, 8, salts, levels, None) == E_RANGE
    assert commit(vals, 8, 2, COL, 7, salts, levels, None) == E_RANGE            # col_stride < n
    assert commit(vals, 8, 2, COL, 8, salts, levels + 8, None) == E_RANGE        # d_levels not 16-byte aligned
    assert commit(vals, 8, 2, COL, 8, salts + 4, levels, None) == E_RANGE        # d_salts not 16-byte aligned
    assert commit(vals + 2, 8, 2, COL, 8, salts, levels, None) == E_RANGE        # d_values not 4-byte aligned
    assert commit(vals + 1, 8, 2, ROW, 0, None, levels, None) == E_RANGE
    # n == 0: success, nothing to do (col_stride is ignored in row-major layout, NULL salts are the unsalted tree)
    assert commit(vals, 0, 2, COL, 0, None, levels, None) == 0
    assert commit(vals, 0, 2, ROW, 0, salts, levels, None) == 0


def test_open_rows_device_refusals_need_no_device(lib):
    levels, vals, salts, idx, out = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    op = lib.toyni_merkle_open_rows_device
    assert op(None, 8, vals, 2, COL, 8, salts, idx, 1, out, None) == E_NULL
    assert op(levels, 8, None, 2, COL, 8, salts, idx, 1, out, None) == E_NULL
    assert op(levels, 8, vals, 2, COL, 8, salts, None, 1, out, None) == E_NULL
    assert op(levels, 8, vals, 2, COL, 8, salts, idx, 1, None, None) == E_NULL
    assert op(levels, 8, vals, 0, COL, 8, salts, idx, 1, out, None) == E_RANGE
    assert op(levels, 8, vals, 65537, ROW, 0, salts, idx, 1, out, None) == E_RANGE
    assert op(levels, 8, vals, 2, 7, 8, salts, idx, 1, out, None) == E_RANGE
    assert op(levels, 8, vals, 2, COL, 7, salts, idx, 1, out, None) == E_RANGE
    assert op(levels + 8, 8, vals, 2, COL, 8, salts, idx, 1, out, None) == E_RANGE
    assert op(levels, 8, vals, 2, COL, 8, salts + 8, idx, 1, out, None) == E_RANGE
    assert op(levels, 8, vals + 2, 2, COL, 8, salts, idx, 1, out, None) == E_RANGE
    assert op(levels, 8, vals, 2, COL, 8, salts, idx + 2, 1, out, None) == E_RANGE
    assert op(levels, 8, vals, 2, COL, 8, salts, idx, 1, out + 4, None) == E_RANGE
    assert op(levels, 0, vals, 2, COL, 0, None, idx, 1, out, None) == 0
    assert op(levels, 8, vals, 2, ROW, 0, None, idx, 0, out, None) == 0


def test_commit_rows_host_refusals_need_no_device(lib):
    v = np.zeros(16, dtype=np.uint64)
    lv = np.full(32 * 15, 0xA5, dtype=np.uint8)
    host = lib.toyni_merkle_commit_rows_host
    assert host(None, 8, 2, None, lv.ctypes.data) == E_NULL
    assert host(v.ctypes.data, 8, 2, None, None) == E_NULL
    assert host(v.ctypes.data, 8, 0, None, lv.ctypes.data) == E_RANGE
    assert host(v.ctypes.data, 1, 65537, None, lv.ctypes.data) == E_RANGE
    assert host(v.ctypes.data, 0, 2, None, lv.ctypes.data) == 0
    assert (lv == 0xA5).all()
