"""Merkle commitment of a layer of field elements on the GPU.

Mirrors `MerkleTree` (src/merkle.rs:9-85) as the prover uses it through build_merkle_tree / build_unsalted_tree
(src/fibonacci.rs:340-361): the tree is built on the device; `levels`, `root()` and `get_proof()` expose the same data the
reference holds.  Verification (src/merkle.rs:87-101) is CPU-only in the reference (the verifier never uses the GPU) and is
not part of this package."""
import numpy as np

from ._lib import check, lib


def level_sizes(n: int):
    sizes = []
    while n >= 1:
        sizes.append(n)
        if n == 1:
            break
        n = (n + 1) // 2
    return sizes


class MerkleTree:
    """Tree over leaves salt(16) || value(8, LE) (salts given) or value(8, LE) (salts None)."""

    def __init__(self, values, salts=None):
        v = np.ascontiguousarray(values, dtype=np.uint64)
        n = v.size
        assert n > 0
        s = None
        if salts is not None:
            s = np.ascontiguousarray(salts, dtype=np.uint8).reshape(n, 16)
        flat = np.empty((lib.toyni_merkle_total_digests(n), 32), dtype=np.uint8)
        check(lib.toyni_merkle_commit_host(v.ctypes.data, s.ctypes.data if s is not None else None, n, flat.ctypes.data), "GPU Merkle commit failed")
        self.n = n
        self.levels, off = [], 0
        for m in level_sizes(n):
            self.levels.append(flat[off:off + m])
            off += m

    def root(self) -> bytes:  # src/merkle.rs:82-84
        return self.levels[-1][0].tobytes()

    def get_proof(self, index: int):
        """src/merkle.rs:50-80: (path, position) with position[i] = True when the sibling is on the LEFT of the running hash."""
        if index >= self.n:
            return None
        path, position, cur = [], [], index
        for level in self.levels[:-1]:
            sib = cur + 1 if cur % 2 == 0 else cur - 1
            if sib >= len(level):  # last node of an odd level: paired with itself, treated as right sibling
                path.append(level[cur].tobytes())
                position.append(True)
            else:
                path.append(level[sib].tobytes())
                position.append(cur % 2 == 1)
            cur //= 2
        return path, position


def merkle_commit_device(d_values: int, d_salts: int, n: int, d_levels: int, stream: int = 0) -> None:
    """Device-resident form: packed u32 values, optional 16-byte salts, all levels written to d_levels."""
    check(lib.toyni_merkle_commit_device(d_values, d_salts or None, n, d_levels, stream or None), "GPU Merkle commit failed")


def merkle_commit_batch_device(d_values: int, value_stride: int, d_salts: int, salt_stride: int, n: int, batch: int, d_levels: int,
                               level_stride: int, stream: int = 0) -> None:
    """`batch` trees of merkle_commit_device in one chain of launches (include/toyni_hip.h 3r): tree b's arrays lie b strides behind the
    base pointers; value_stride in words, salt_stride and level_stride in bytes."""
    check(lib.toyni_merkle_commit_batch_device(d_values, value_stride, d_salts or None, salt_stride, n, batch, d_levels, level_stride,
                                               stream or None), "GPU batched Merkle commit failed")


ROWS_COLUMN_MAJOR = 0   # TOYNI_ROWS_COLUMN_MAJOR: element (i, c) at values[c * col_stride + i]
ROWS_ROW_MAJOR = 1      # TOYNI_ROWS_ROW_MAJOR:    element (i, c) at values[i * width + c]


class RowMerkleTree(MerkleTree):
    """Tree whose leaf is one ROW of an (n, width) matrix: [salt(16)] || v(i,0) (8, LE) || ... || v(i,width-1) (8, LE).
    MerkleTree::new (src/merkle.rs:16-48) over such leaves; width = 1 is MerkleTree.  u64 inputs are reduced mod p like
    BabyBear::new."""

    def __init__(self, matrix, salts=None):
        m = np.ascontiguousarray(matrix, dtype=np.uint64)
        assert m.ndim == 2 and m.shape[0] > 0 and m.shape[1] > 0, "an (n, width) matrix"
        n, width = m.shape
        s = None
        if salts is not None:
            s = np.ascontiguousarray(salts, dtype=np.uint8).reshape(n, 16)
        flat = np.empty((lib.toyni_merkle_total_digests(n), 32), dtype=np.uint8)
        check(lib.toyni_merkle_commit_rows_host(m.ctypes.data, n, width, s.ctypes.data if s is not None else None, flat.ctypes.data),
              "GPU Merkle row commit failed")
        self.n, self.width = n, width
        self._values = m % np.uint64(2013265921)
        self._salts = s
        self.levels, off = [], 0
        for k in level_sizes(n):
            self.levels.append(flat[off:off + k])
            off += k

    def leaf_bytes(self, index: int) -> bytes:
        """The leaf the tree hashed for row `index` (what verify_merkle_proof, src/merkle.rs:87-101, is given)."""
        salt = self._salts[index].tobytes() if self._salts is not None else b""
        return salt + self._values[index].astype("<u8").tobytes()


def merkle_commit_rows_device(d_values: int, n: int, width: int, layout: int, col_stride: int, d_salts: int, d_levels: int,
                              stream: int = 0) -> None:
    """Device-resident row commitment: packed u32 matrix in either layout, optional 16-byte salts, all levels to d_levels."""
    check(lib.toyni_merkle_commit_rows_device(d_values, n, width, layout, col_stride, d_salts or None, d_levels, stream or None),
          "GPU Merkle row commit failed")


def merkle_open_rows_device(d_levels: int, n: int, d_values: int, width: int, layout: int, col_stride: int, d_salts: int,
                            d_indices: int, nidx: int, d_out: int, stream: int = 0) -> None:
    """nidx opening records of toyni_merkle_open_rows_record_bytes(n, width) bytes each, gathered on the device into d_out."""
    check(lib.toyni_merkle_open_rows_device(d_levels, n, d_values, width, layout, col_stride, d_salts or None, d_indices, nidx, d_out,
                                            stream or None), "GPU Merkle row opening failed")


# ---- coset leaves of an Ext FRI layer (include/toyni_hip.h 3m) ----
def coset_rows(layer4) -> np.ndarray:
    """(m, 4) Ext elements -> the (m / 4, 16) matrix whose row j is elements j, j + m/4, j + m/2, j + 3m/4: the rows the coset
    tree commits."""
    e = np.ascontiguousarray(layer4).reshape(-1, 4)
    m = e.shape[0]
    assert m >= 4 and m & (m - 1) == 0, "a layer of a power of two >= 4 Ext elements"
    return np.ascontiguousarray(e.reshape(4, m // 4, 4).transpose(1, 0, 2)).reshape(m // 4, 16)


class CosetExtMerkleTree:
    """The coset tree of an Ext layer in hashlib, no device: leaf j = [salt_j (16)] || to_bytes of elements j, j + m/4, j + m/2,
    j + 3m/4; node = sha256(01 || left || right), an odd level pairs its last node with itself (src/merkle.rs:25-48).  What
    merkle_commit_cosets_ext_device writes, as `levels` (lists of 32-byte digests), `flat()` (the device layout) and `root()`."""

    def __init__(self, layer4, salts=None):
        import hashlib
        rows = coset_rows(np.ascontiguousarray(layer4, dtype=np.uint64) % np.uint64(2013265921))
        n = rows.shape[0]
        body = rows.astype("<u8").view(np.uint8).reshape(n, 128)
        if salts is not None:
            body = np.concatenate([np.ascontiguousarray(salts, dtype=np.uint8).reshape(n, 16), body], axis=1)
        self.n = n
        self._leaves = [r.tobytes() for r in body]
        level = [hashlib.sha256(b"\x00" + l).digest() for l in self._leaves]
        self.levels = [level]
        while len(level) > 1:
            level = [hashlib.sha256(b"\x01" + level[i] + level[i + 1 if i + 1 < len(level) else i]).digest() for i in range(0, len(level), 2)]
            self.levels.append(level)

    def root(self) -> bytes:
        return self.levels[-1][0]

    def leaf_bytes(self, index: int) -> bytes:
        return self._leaves[index]

    def flat(self) -> np.ndarray:
        return np.frombuffer(b"".join(d for level in self.levels for d in level), dtype=np.uint8).reshape(-1, 32)


def merkle_commit_cosets_ext_device(d_layer: int, m: int, d_salts: int, d_levels: int, stream: int = 0) -> None:
    """The coset tree (m / 4 leaves) of a device-resident layer of m Ext elements, read as it lies; all levels to d_levels."""
    check(lib.toyni_merkle_commit_cosets_ext_device(d_layer, m, d_salts or None, d_levels, stream or None), "GPU coset commit failed")


def merkle_open_cosets_ext_device(d_levels: int, m: int, d_layer: int, d_salts: int, d_indices: int, nidx: int, d_out: int,
                                  stream: int = 0) -> None:
    """nidx opening records of toyni_merkle_open_rows_record_bytes(m / 4, 16) bytes each, of the coset leaves d_indices names."""
    check(lib.toyni_merkle_open_cosets_ext_device(d_levels, m, d_layer, d_salts or None, d_indices, nidx, d_out, stream or None),
          "GPU coset opening failed")
