"""Helpers of the row-leaf Merkle tests (a plain module, imported like tests/guarded.py): leaves built in numpy from a matrix, the
matrix laid out for the device in either layout with poison wherever the library must not read, a hashlib restatement of
verify_merkle_proof (src/merkle.rs:87-101), and the opening record taken apart."""
import hashlib

import numpy as np

from guarded import Guarded, P

COL, ROW = 0, 1
POISON = 0xDEADBEEF                   # >= p: no canonical residue; a leaf that absorbs it differs from the oracle's


def depth_of(n):
    d = 0
    while n > 1:
        n, d = (n + 1) // 2, d + 1
    return d


def level_sizes(n):
    out = [n]
    while n > 1:
        n = (n + 1) // 2
        out.append(n)
    return out


def leaf_array(matrix, salts=None):
    """(n, L) uint8: row i = [salt_i] || v(i,0) as 8 LE bytes || ... -- the leaves MerkleTree::new is given."""
    m = np.ascontiguousarray(matrix, dtype=np.uint64)
    n, width = m.shape
    body = m.astype("<u8").view(np.uint8).reshape(n, 8 * width)
    if salts is None:
        return body
    return np.concatenate([np.ascontiguousarray(salts, dtype=np.uint8).reshape(n, 16), body], axis=1)


def leaves_of(matrix, salts=None):
    return [r.tobytes() for r in leaf_array(matrix, salts)]


def device_words(matrix, layout, col_stride=None, tail=64):
    """The uint32 words handed to the device: the matrix in `layout`, POISON between n and col_stride of every column and in `tail`
    words past the matrix."""
    m = np.ascontiguousarray(matrix, dtype=np.uint32)
    n, width = m.shape
    if layout == ROW:
        return np.concatenate([m.reshape(-1), np.full(tail, POISON, dtype=np.uint32)])
    cs = col_stride or n
    out = np.full(width * cs + tail, POISON, dtype=np.uint32)
    for c in range(width):
        out[c * cs:c * cs + n] = m[:, c]
    return out


def hash_leaf(leaf: bytes) -> bytes:
    return hashlib.sha256(b"\x00" + leaf).digest()


def hash_node(left: bytes, right: bytes) -> bytes:
    return hashlib.sha256(b"\x01" + left + right).digest()


def verify_merkle_proof(leaf: bytes, path, position, root: bytes) -> bool:
    """src/merkle.rs:87-101: position[i] true = the sibling is the LEFT input."""
    cur = hash_leaf(leaf)
    for sibling, is_right in zip(path, position):
        cur = hash_node(sibling, cur) if is_right else hash_node(cur, sibling)
    return cur == root


def hashlib_levels(leaves):
    """MerkleTree::build_tree (src/merkle.rs:25-48) in hashlib, for small n."""
    level = [hash_leaf(l) for l in leaves]
    levels = [level]
    while len(level) > 1:
        level = [hash_node(level[i], level[i + 1] if i + 1 < len(level) else level[i]) for i in range(0, len(level), 2)]
        levels.append(level)
    return levels


def split_record(rec: bytes, n, width):
    """(path digests, salt, value bytes, position flags, padding) of one opening record."""
    d = depth_of(n)
    path = [rec[32 * l:32 * l + 32] for l in range(d)]
    salt = rec[32 * d:32 * d + 16]
    vals = rec[32 * d + 16:32 * d + 16 + 8 * width]
    flags = rec[32 * d + 16 + 8 * width:32 * d + 16 + 8 * width + d]
    pad = rec[32 * d + 16 + 8 * width + d:]
    return path, salt, vals, [bool(b) for b in flags], pad


class Dev:
    """Guard-banded device buffers of one test, freed (and their guards checked) on exit."""

    def __init__(self, ta):
        self.ta, self.bufs = ta, []

    def buf(self, nbytes, offset=0, word=4):
        g = Guarded(self.ta, nbytes, offset=offset, word=word, guard=min(max(nbytes, 64 << 10), 4 << 20))
        self.bufs.append(g)
        return g

    def put(self, arr, offset=0, word=4):
        arr = np.ascontiguousarray(arr)
        g = self.buf(arr.nbytes, offset, word)
        g.upload(arr)
        return g

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        err = None
        for g in self.bufs:
            try:
                g.free(check=exc[0] is None)
            except AssertionError as e:
                err = err or e
        if err:
            raise err
        return False


assert POISON >= P
