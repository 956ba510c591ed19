"""The row-leaf Merkle entry points (include/toyni_hip.h 3d) between guard bands (tests/guarded.py): d_levels and d_out sit between
guards that stay intact, inputs are unchanged by the call, the words between n and col_stride of a padded column and beyond the
matrix never influence the result (the case runs with two different fillings of them and of the guards around every input), and
refused arguments and n = 0 write nothing."""
import numpy as np
import pytest

import oracle
from guarded import Guarded, edge_residues
from rows_common import COL, ROW, POISON, leaves_of

pytestmark = pytest.mark.gpu

E_NULL, E_RANGE = 10002, 10006


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


def lay_out(m, layout, cs, slack):
    """The matrix as device words, `slack` (an array generator) in every word the library must not read."""
    n, width = m.shape
    if layout == ROW:
        return m.reshape(-1).copy()
    out = slack(width * cs)
    for c in range(width):
        out[c * cs:c * cs + n] = m[:, c]
    return out[:(width - 1) * cs + n]             # the matrix ends with its last element: what follows is the guard


@pytest.mark.parametrize("n,width,layout,salted,off", [
    (5, 3, COL, 1, 4), (33, 7, COL, 0, 12), (1000, 13, COL, 1, 0), (4096, 64, COL, 0, 8), (1000, 8, COL, 1, 4),
    (5, 4, ROW, 0, 0), (33, 5, ROW, 1, 8), (1000, 15, ROW, 0, 4), (4096, 4, ROW, 1, 0), (1000, 100, ROW, 1, 0), (1000, 16, ROW, 0, 12),
])
def test_commit_and_open_between_guard_bands(ta, n, width, layout, salted, off):
    lib = ta._lib.lib
    m = edge_residues(n * width, 31000 + n + width).reshape(n, width)
    salts = np.random.default_rng(n + width).integers(0, 256, (n, 16), dtype=np.uint8) if salted else None
    cs = n + 40 if layout == COL else 0
    idx = np.array([0, n - 1, n // 2, n // 3], dtype=np.uint32)
    total = int(lib.toyni_merkle_total_digests(n))
    rec = int(lib.toyni_merkle_open_rows_record_bytes(n, width))
    rng = np.random.default_rng(5)
    fillings = {"sentinel": lambda k: np.full(k, POISON, dtype=np.uint32),
                "random": lambda k: rng.integers(0, oracle.P, k, dtype=np.uint64).astype(np.uint32)}
    results = []
    for pattern, slack in fillings.items():
        words = lay_out(m, layout, cs, slack)
        bufs = []
        try:
            dv = Guarded(ta, words.nbytes, offset=off, seed=1); bufs.append(dv)
            ds = None
            if salted:
                ds = Guarded(ta, salts.nbytes, word=1, seed=2); bufs.append(ds)
            ix = Guarded(ta, idx.nbytes, offset=12, seed=3); bufs.append(ix)
            dl = Guarded(ta, 32 * total, word=1, seed=4); bufs.append(dl)
            do = Guarded(ta, rec * idx.size, offset=8, word=1, seed=5); bufs.append(do)
            for g, host in ((dv, words), (ds, salts), (ix, idx)):
                if g is not None:
                    g.refill(pattern)                 # the guards around every input: 0xA5 bytes, then random canonical words
                    g.upload(host)
            sp = ds.ptr if ds else None
            assert lib.toyni_merkle_commit_rows_device(dv.ptr, n, width, layout, cs, sp, dl.ptr, None) == 0
            assert lib.toyni_merkle_open_rows_device(dl.ptr, n, dv.ptr, width, layout, cs, sp, ix.ptr, idx.size, do.ptr, None) == 0
            dv.mem.sync()
            for g in bufs:
                g.check(f"{pattern}: n={n} width={width}")
            assert (dv.download() == words).all() and (ix.download() == idx).all(), "an input was changed"
            if salted:
                assert (ds.download(np.uint8) == salts.reshape(-1)).all(), "the salts were changed"
            results.append((dl.download(np.uint8), do.download(np.uint8)))
        finally:
            for g in bufs:
                g.free(check=False)
    assert (results[0][0] == results[1][0]).all(), "the tree depends on words outside the matrix"
    assert (results[0][1] == results[1][1]).all(), "the openings depend on words outside the matrix"
    want = np.concatenate(oracle.merkle_levels(leaves_of(m, salts))).reshape(-1)
    assert (results[0][0] == want).all()
    # every byte of a record is written (the fields are compared one by one in tests/test_gpu_merkle_rows.py): the output was
    # pre-filled with 0xA5, so the zero padding after the position bytes and the upper halves of the values show a skipped byte
    assert rec % 8 == 0
    records = results[0][1].reshape(idx.size, rec)
    d = len(oracle.merkle_level_sizes(n)) - 1
    assert (records[:, 32 * d + 16 + 8 * width + d:] == 0).all()
    assert (records[:, 32 * d + 16:32 * d + 16 + 8 * width].reshape(idx.size, width, 8)[:, :, 4:] == 0).all()
    if not salted:
        assert (records[:, 32 * d:32 * d + 16] == 0).all()


def test_refused_arguments_and_zero_rows_write_nothing(ta):
    lib = ta._lib.lib
    n, width = 64, 4
    m = edge_residues(n * width, 99).reshape(n, width)
    idx = np.array([0, 63], dtype=np.uint32)
    total = int(lib.toyni_merkle_total_digests(n))
    rec = int(lib.toyni_merkle_open_rows_record_bytes(n, width))
    bufs = [Guarded(ta, m.nbytes), Guarded(ta, 16 * n, word=1), Guarded(ta, idx.nbytes), Guarded(ta, 32 * total + 16, word=1),
            Guarded(ta, 2 * rec + 8, word=1)]
    dv, ds, ix, dl, do = bufs
    try:
        dv.upload(m.reshape(-1))
        ix.upload(idx)
        commit, op = lib.toyni_merkle_commit_rows_device, lib.toyni_merkle_open_rows_device
        calls = {
            "commit null values": (lambda: commit(None, n, width, ROW, 0, ds.ptr, dl.ptr, None), E_NULL),
            "commit null levels": (lambda: commit(dv.ptr, n, width, ROW, 0, ds.ptr, None, None), E_NULL),
            "commit width 0": (lambda: commit(dv.ptr, n, 0, ROW, 0, ds.ptr, dl.ptr, None), E_RANGE),
            "commit width 65537": (lambda: commit(dv.ptr, n, 65537, COL, n, ds.ptr, dl.ptr, None), E_RANGE),
            "commit layout 2": (lambda: commit(dv.ptr, n, width, 2, n, ds.ptr, dl.ptr, None), E_RANGE),
            "commit stride < n": (lambda: commit(dv.ptr, n, width, COL, n - 1, ds.ptr, dl.ptr, None), E_RANGE),
            "commit levels misaligned": (lambda: commit(dv.ptr, n, width, ROW, 0, ds.ptr, dl.ptr + 8, None), E_RANGE),
            "commit salts misaligned": (lambda: commit(dv.ptr, n, width, ROW, 0, ds.ptr + 4, dl.ptr, None), E_RANGE),
            "commit values misaligned": (lambda: commit(dv.ptr + 2, n, width, ROW, 0, ds.ptr, dl.ptr, None), E_RANGE),
            "commit n 0": (lambda: commit(dv.ptr, 0, width, COL, 0, ds.ptr, dl.ptr, None), 0),
            "open null out": (lambda: op(dl.ptr, n, dv.ptr, width, ROW, 0, ds.ptr, ix.ptr, 2, None, None), E_NULL),
            "open width 0": (lambda: op(dl.ptr, n, dv.ptr, 0, ROW, 0, ds.ptr, ix.ptr, 2, do.ptr, None), E_RANGE),
            "open layout -1": (lambda: op(dl.ptr, n, dv.ptr, width, -1, 0, ds.ptr, ix.ptr, 2, do.ptr, None), E_RANGE),
            "open stride < n": (lambda: op(dl.ptr, n, dv.ptr, width, COL, n - 1, ds.ptr, ix.ptr, 2, do.ptr, None), E_RANGE),
            "open out misaligned": (lambda: op(dl.ptr, n, dv.ptr, width, ROW, 0, ds.ptr, ix.ptr, 2, do.ptr + 4, None), E_RANGE),
            "open indices misaligned": (lambda: op(dl.ptr, n, dv.ptr, width, ROW, 0, ds.ptr, ix.ptr + 2, 2, do.ptr, None), E_RANGE),
            "open levels misaligned": (lambda: op(dl.ptr + 8, n, dv.ptr, width, ROW, 0, ds.ptr, ix.ptr, 2, do.ptr, None), E_RANGE),
            "open n 0": (lambda: op(dl.ptr, 0, dv.ptr, width, ROW, 0, ds.ptr, ix.ptr, 2, do.ptr, None), 0),
            "open nidx 0": (lambda: op(dl.ptr, n, dv.ptr, width, ROW, 0, ds.ptr, ix.ptr, 0, do.ptr, None), 0),
        }
        for what, (call, expect) in calls.items():
            rc = call()
            assert rc == expect, f"{what}: status {rc}, expected {expect}"
            dv.mem.sync()
            for g in (dl, do):
                assert (g.download(np.uint8) == 0xA5).all(), f"{what}: wrote to an output"
                g.check(what)
        assert (dv.download() == m.reshape(-1)).all()
    finally:
        for g in bufs:
            g.free(check=False)
