"""Merkle commitment and openings of the ROWS of a device-resident matrix (include/toyni_hip.h 3d) against things that are not the
code under test: oracle.merkle_levels / oracle.merkle_get_proofs over leaves built in numpy, a few lines of hashlib
(tests/rows_common.py), and the single-column entry points for width = 1.  Equality is byte for byte everywhere.  Every matrix is
uploaded with poison (0xDEADBEEF >= p) between n and col_stride of its columns and past its end."""
import time

import numpy as np
import pytest

import oracle
from guarded import edge_residues, edge_u64, reduce_u64
from rows_common import COL, ROW, Dev, depth_of, device_words, hashlib_levels, leaves_of, level_sizes, split_record, verify_merkle_proof

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 5, 33, 1000, 4096, 1 << 16)
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 13, 15, 16, 31, 64, 100)
# (layout, extra column stride, byte offset of d_values): column-major tight and inside a larger allocation, row-major 16-byte
# aligned (16-byte loads when width % 4 == 0) and 4 bytes off (word loads whatever the width)
MODES = ((COL, 0, 0), (COL, 24, 0), (ROW, 0, 0), (ROW, 0, 4))


def padding_block_width(width, salted):
    """L mod 64 = 57: the SHA-256 padding takes a block of its own."""
    return (1 + 16 * salted + 8 * width) % 64 == 57


def parity_cases():
    """A sample of n x width x salt x mode in which every width meets every mode and both salt modes, every n occurs, and the
    padding-block widths (5, 13 salted; 7, 15 unsalted) run at n >= 1000."""
    cases = []
    for wi, width in enumerate(WIDTHS):
        for salted in (0, 1):
            for mi, (layout, extra, off) in enumerate(MODES):
                if off and width % 4:
                    continue                      # word loads already: the aligned case covers it
                k = 3 * wi + 5 * salted + 2 * mi
                n = NS[5 + k % 3] if padding_block_width(width, salted) else NS[k % len(NS)]
                cases.append((n, width, salted, layout, extra, off))
    return cases


def test_the_sample_covers_what_it_must():
    cases = parity_cases()
    assert {c[0] for c in cases} == set(NS) and {c[1] for c in cases} == set(WIDTHS)
    assert {c[2] for c in cases} == {0, 1} and {c[3] for c in cases} == {COL, ROW}
    assert any(c[3] == COL and c[4] == 24 for c in cases)
    for width, salted in ((5, 1), (13, 1), (7, 0), (15, 0)):
        assert padding_block_width(width, salted)
        hit = [c for c in cases if c[1] == width and c[2] == salted]
        assert hit and all(c[0] >= 1000 for c in hit) and {c[3] for c in hit} == {COL, ROW}


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


def matrix_of(n, width, seed):
    return edge_residues(n * width, seed).reshape(n, width)


def salts_of(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 16), dtype=np.uint8)


def commit_rows(ta, dev, m, layout, salts=None, extra=0, off=0):
    """Upload m (n, width) in `layout`, commit, return (flat levels (total, 32) uint8, d_values, d_salts, d_levels, col_stride)."""
    lib = ta._lib.lib
    n, width = m.shape
    cs = n + extra if layout == COL else 0
    words = device_words(m, layout, cs or None)
    dv = dev.put(words, off)
    ds = dev.put(salts.reshape(-1), word=1) if salts is not None else None
    total = int(lib.toyni_merkle_total_digests(n))
    dl = dev.buf(32 * total, word=1)
    rc = lib.toyni_merkle_commit_rows_device(dv.ptr, n, width, layout, cs, ds.ptr if ds else None, dl.ptr, None)
    assert rc == 0, f"status {rc}"
    dv.mem.sync()
    assert (dv.download() == words).all(), "the matrix was changed by the commit"
    return dl.download(np.uint8).reshape(total, 32), dv, ds, dl, cs


def same_levels(got_flat, want_levels, what):
    want = np.concatenate(want_levels)
    assert got_flat.shape == want.shape, what
    bad = np.flatnonzero((got_flat != want).any(axis=1))
    assert not bad.size, f"{what}: {bad.size} digests differ from the oracle, first at {bad[0]}"


# ---------------------------------------------------------------- 1. tree parity
@pytest.mark.parametrize("n,width,salted,layout,extra,off", parity_cases())
def test_tree_parity(ta, n, width, salted, layout, extra, off):
    m = matrix_of(n, width, 7000 + 131 * width + n)
    salts = salts_of(n, n + width) if salted else None
    with Dev(ta) as dev:
        got = commit_rows(ta, dev, m, layout, salts, extra, off)[0]
    leaves = leaves_of(m, salts)
    same_levels(got, oracle.merkle_levels(leaves), f"n={n} width={width} salted={salted} layout={layout} stride+{extra} off={off}")
    if n <= 33:                                     # and hashlib alone, where that is cheap
        want = hashlib_levels(leaves)
        assert [d.tobytes() for d in got] == [d for level in want for d in level]


# ---------------------------------------------------------------- 2. width 1 is today's tree
@pytest.mark.parametrize("n", [1, 5, 1000, 1 << 16])
@pytest.mark.parametrize("salted", [0, 1])
def test_width_one_is_the_single_column_tree(ta, n, salted):
    lib = ta._lib.lib
    vals = edge_residues(n, 4200 + n)
    salts = salts_of(n, 77 + n) if salted else None
    idx = np.array(sorted({0, n // 2, n - 1, (n - 1) // 2}), dtype=np.uint32)
    rec = int(lib.toyni_merkle_open_record_bytes(n))
    assert rec == int(lib.toyni_merkle_open_rows_record_bytes(n, 1))
    with Dev(ta) as dev:
        outs = []
        for layout in (COL, ROW):
            got, dv, ds, dl, cs = commit_rows(ta, dev, vals.reshape(n, 1), layout, salts)
            ix, o = dev.put(idx), dev.buf(idx.size * rec, word=1)
            assert lib.toyni_merkle_open_rows_device(dl.ptr, n, dv.ptr, 1, layout, cs, ds.ptr if ds else None, ix.ptr, idx.size, o.ptr, None) == 0
            dv.mem.sync()
            outs.append((got, o.download(np.uint8)))
        # the parent's entry points on the same values and salts
        total = got.shape[0]
        dl1, o1 = dev.buf(32 * total, word=1), dev.buf(idx.size * rec, word=1)
        assert lib.toyni_merkle_commit_device(dv.ptr, ds.ptr if ds else None, n, dl1.ptr, None) == 0
        assert lib.toyni_merkle_open_device(dl1.ptr, n, dv.ptr, ds.ptr if ds else None, ix.ptr, idx.size, o1.ptr, None) == 0
        dv.mem.sync()
        single, single_open = dl1.download(np.uint8).reshape(total, 32), o1.download(np.uint8)
    for got, opened in outs:
        assert (got == single).all(), "levels differ from toyni_merkle_commit_device"
        assert (opened == single_open).all(), "records differ from toyni_merkle_open_device"
    same_levels(single, oracle.merkle_commit_values(vals.astype(np.uint64), salts), f"width 1, n={n}")


# ---------------------------------------------------------------- 3. a prover-sized case
def test_prover_sized_commitment(ta):
    lib = ta._lib.lib
    n, width = 1 << 21, 8
    m = matrix_of(n, width, 2021)
    key = np.arange(32, dtype=np.uint8)
    with Dev(ta) as dev:
        dv = dev.put(device_words(m, COL, n))
        ds = dev.buf(16 * n, word=1)
        assert lib.toyni_chacha20_fill_device(ds.ptr, 16 * n, key.ctypes.data, 21, None) == 0
        total = int(lib.toyni_merkle_total_digests(n))
        dl = dev.buf(32 * total, word=1)
        assert lib.toyni_merkle_commit_rows_device(dv.ptr, n, width, COL, n, ds.ptr, dl.ptr, None) == 0
        dv.mem.sync()
        salts = ds.download(np.uint8).reshape(n, 16)
        got = dl.download(np.uint8).reshape(total, 32)
    assert len(np.unique(salts[:4096], axis=0)) == 4096          # a keystream, not a constant
    t0 = time.time()
    want = oracle.merkle_levels(leaves_of(m, salts))
    print(f"oracle tree over 2^21 leaves of {16 + 8 * width} bytes: {time.time() - t0:.1f} s")
    same_levels(got, want, "n=2^21 width=8 column-major salted")


# ---------------------------------------------------------------- 4. the pipeline
def test_lde_then_commit_rows_without_a_transpose(ta):
    lib = ta._lib.lib
    log_n, log_blowup, width, shift = 16, 4, 8, 7
    n, nc = 1 << log_n, 1 << (log_n - log_blowup)
    ctx = ta.ntt.get_or_create_ctx(n)
    coeffs = edge_residues(width * nc, 5150).reshape(width, nc)
    salts = salts_of(n, 5151)
    with Dev(ta) as dev:
        dc, dx = dev.put(coeffs.reshape(-1)), dev.buf(4 * width * n)
        ds = dev.put(salts.reshape(-1), word=1)
        total = int(lib.toyni_merkle_total_digests(n))
        dl = dev.buf(32 * total, word=1)
        assert lib.toyni_lde_device(ctx.handle, dc.ptr, dx.ptr, width, log_blowup, shift, None) == 0
        assert lib.toyni_merkle_commit_rows_device(dx.ptr, n, width, COL, n, ds.ptr, dl.ptr, None) == 0   # the LDE's output as it lies
        dx.mem.sync()
        got = dl.download(np.uint8).reshape(total, 32)
    m = np.stack([oracle.domain_fft(coeffs[c].astype(np.uint64), n, shift) for c in range(width)], axis=1)
    same_levels(got, oracle.merkle_levels(leaves_of(m, salts)), "LDE -> commit rows")


def test_ext_vector_commits_as_row_major_width_four(ta):
    lib = ta._lib.lib
    log_n, shift = 14, 7
    n = 1 << log_n
    ctx = ta.ntt.get_or_create_ctx(n)
    x = edge_residues(4 * n, 5160)
    with Dev(ta) as dev:
        dx = dev.put(x)
        total = int(lib.toyni_merkle_total_digests(n))
        dl = dev.buf(32 * total, word=1)
        assert lib.toyni_ntt_ext_device(ctx.handle, dx.ptr, shift, 0, None) == 0
        assert lib.toyni_merkle_commit_rows_device(dx.ptr, n, 4, ROW, 0, None, dl.ptr, None) == 0
        dx.mem.sync()
        got = dl.download(np.uint8).reshape(total, 32)
    xx = x.reshape(n, 4).astype(np.uint64)
    y = np.stack([oracle.domain_fft(xx[:, q], n, shift) for q in range(4)], axis=1)
    leaves = [b"".join(int(v).to_bytes(8, "little") for v in row) for row in y]      # Ext::to_bytes: the four limbs back to back
    assert leaves == leaves_of(y)
    same_levels(got, oracle.merkle_levels(leaves), "Ext vector, row-major width 4")


# ---------------------------------------------------------------- 5. openings
def last_node_of_an_odd_level(n):
    """A leaf whose path runs through the last node of an odd level (paired with itself), if the tree has one."""
    for lvl, m in enumerate(level_sizes(n)[:-1]):
        if m % 2:
            return min(n - 1, (m - 1) << lvl)
    return n - 1


@pytest.mark.parametrize("n", [5, 33, 1000, 1 << 16])
@pytest.mark.parametrize("width", [1, 4, 7, 64])
def test_openings(ta, n, width):
    lib = ta._lib.lib
    case = NS.index(n) + WIDTHS.index(width)
    layout, salted = (COL, ROW)[case % 2], (case // 2) % 2 == 0
    m = matrix_of(n, width, 9000 + n + width)
    salts = salts_of(n, 9 + n) if salted else None
    rng = np.random.default_rng(n * width)
    idx = np.array([0, n - 1, last_node_of_an_odd_level(n), n // 2] + rng.integers(0, n, 12).tolist(), dtype=np.uint32)
    rec = int(lib.toyni_merkle_open_rows_record_bytes(n, width))
    with Dev(ta) as dev:
        got, dv, ds, dl, cs = commit_rows(ta, dev, m, layout, salts, extra=24 if layout == COL else 0)
        ix, o = dev.put(idx, 12), dev.buf(idx.size * rec, 8, word=1)
        assert lib.toyni_merkle_open_rows_device(dl.ptr, n, dv.ptr, width, layout, cs, ds.ptr if ds else None, ix.ptr, idx.size, o.ptr, None) == 0
        dv.mem.sync()
        records = o.download(np.uint8).tobytes()
    leaves = leaves_of(m, salts)
    levels = oracle.merkle_levels(leaves)
    same_levels(got, levels, f"openings: tree n={n} width={width}")
    root = levels[-1][0].tobytes()
    proofs = oracle.merkle_get_proofs(levels, idx.tolist())
    d = depth_of(n)
    assert rec == 32 * d + 16 + 8 * width + (d + 7) // 8 * 8 and len(records) == rec * idx.size
    for k, index in enumerate(idx.tolist()):
        path, salt, vals, flags, pad = split_record(records[k * rec:(k + 1) * rec], n, width)
        want_path, want_flags = proofs[k]
        assert path == want_path and flags == want_flags, f"index {index}"
        assert salt == (salts[index].tobytes() if salted else bytes(16))
        assert vals == m[index].astype("<u8").tobytes() and pad == bytes(len(pad))
        leaf = (salt if salted else b"") + vals
        assert leaf == leaves[index]
        assert verify_merkle_proof(leaf, path, flags, root), f"index {index}: the opening does not verify"
        flipped = bytearray(leaf)
        flipped[-8] ^= 1                           # a value byte
        assert not verify_merkle_proof(bytes(flipped), path, flags, root), "the restatement accepts anything"


# ---------------------------------------------------------------- 7. host form and Python class
def test_row_merkle_tree_class(ta):
    n, width = 1000, 5
    raw = edge_u64(n * width, 606).reshape(n, width)               # non-canonical u64 inputs among them
    assert (raw >= np.uint64(oracle.P)).any()
    m = reduce_u64(raw).reshape(n, width)
    salts = salts_of(n, 607)
    for s in (salts, None):
        tree = ta.RowMerkleTree(raw, s)
        leaves = leaves_of(m, s)
        want = oracle.merkle_levels(leaves)
        assert len(tree.levels) == len(want)
        for a, b in zip(tree.levels, want):
            assert (a == b).all()
        assert tree.root() == want[-1][0].tobytes()
        for index in (0, 1, 499, 998, 999):
            assert tree.leaf_bytes(index) == leaves[index]
            path, position = tree.get_proof(index)
            assert (path, position) == oracle.merkle_get_proof(want, index)
            assert verify_merkle_proof(tree.leaf_bytes(index), path, position, tree.root())
        assert tree.get_proof(n) is None
    one = ta.RowMerkleTree(raw[:, :1], salts)                       # width 1 = MerkleTree
    assert one.root() == ta.MerkleTree(raw[:, 0], salts).root()


def test_python_device_wrappers(ta):
    lib = ta._lib.lib
    n, width = 33, 3
    m = matrix_of(n, width, 808)
    idx = np.array([0, 32, 16], dtype=np.uint32)
    rec = int(lib.toyni_merkle_open_rows_record_bytes(n, width))
    with Dev(ta) as dev:
        dv = dev.put(device_words(m, ROW))
        total = int(lib.toyni_merkle_total_digests(n))
        dl, ix, o = dev.buf(32 * total, word=1), dev.put(idx), dev.buf(rec * idx.size, word=1)
        ta.merkle_commit_rows_device(dv.ptr, n, width, ta.ROWS_ROW_MAJOR, 0, 0, dl.ptr)
        ta.merkle_open_rows_device(dl.ptr, n, dv.ptr, width, ta.ROWS_ROW_MAJOR, 0, 0, ix.ptr, idx.size, o.ptr)
        dv.mem.sync()
        got, records = dl.download(np.uint8).reshape(total, 32), o.download(np.uint8).tobytes()
        with pytest.raises(Exception):
            ta.merkle_commit_rows_device(dv.ptr, n, 0, ta.ROWS_ROW_MAJOR, 0, 0, dl.ptr)
    leaves = leaves_of(m)
    levels = hashlib_levels(leaves)
    assert [d.tobytes() for d in got] == [d for level in levels for d in level]
    for k, index in enumerate(idx.tolist()):
        path, salt, vals, flags, _ = split_record(records[k * rec:(k + 1) * rec], n, width)
        assert salt == bytes(16) and vals == leaves[index]
        assert verify_merkle_proof(vals, path, flags, levels[-1][0])
