"""Reference prover -- TEST INFRASTRUCTURE.  The protocol both provers of this repository follow (the Python harness in this
directory and the compiled C++ prover of the library's host directory), restated with nothing but the C oracle (oracle/, the
CPU restatement of every kernel), Python integers, hashlib and the transcript of fib_verifier.py.  No device code is involved: a
proof computed here is what a prover must emit on the same trace and randomness, byte for byte -- the serialized opening
records included, padding zero.

    proof, components = prove(trace, randomness)

  proof       the StarkProof fields the verifier reads (the shape the harness' expand_proof returns), plus the wire form of
              the openings: "query_indices", "opening_groups" [(tree leaves, salted, indices)] and "opening_records" (uint8:
              the records of include/toyni_hip.h section 3c back to back, in group order)
  components  every intermediate value, keyed as the harness' `capture` dict keys them (COMPONENTS, in protocol order)

Randomness comes in two interchangeable forms: HarnessRandomness (the salt pool and mask values the Python harness drew) and
ChaChaRandomness (the keystreams the compiled prover derives from its 32-byte key).  Both hand out salts 16 bytes per leaf in
the order trace tree, quotient tree, DEEP tree, then every salted FRI layer from the largest down.
"""
import hashlib

import numpy as np

import oracle

from .fib_verifier import BLOWUP, COSET_SHIFT, MASK_DEGREE, NUM_QUERIES, P, Transcript, derive_z, root_of_unity

COMPONENTS = ("mask", "masked_coeffs", "trace_lde", "c_evals", "q_evals", "c_poly", "q_poly", "z", "ood", "deep", "betas", "fri_layers")
WIRE_FIELDS = ("trace_len", "lde_size", "trace_commitment", "quotient_commitment", "t_z", "t_gz", "t_ggz", "q_z", "fri_commitments",
               "fri_final_layer", "query_indices", "opening_groups", "opening_records")


# ---- ChaCha20 (RFC 8439 section 2.3), vectorised over the block counter ----
_SIGMA = np.array([0x61707865, 0x3320646E, 0x79622D32, 0x6B206574], dtype=np.uint32)
_CHUNK = 1 << 16          # blocks per sweep: 16 rows of 256 KiB


def _rotl(v, n, tmp):
    np.left_shift(v, np.uint32(n), out=tmp)
    v >>= np.uint32(32 - n)
    v |= tmp


def _quarter_round(x, a, b, c, d, tmp):
    xa, xb, xc, xd = x[a], x[b], x[c], x[d]
    xa += xb; xd ^= xa; _rotl(xd, 16, tmp)
    xc += xd; xb ^= xc; _rotl(xb, 12, tmp)
    xa += xb; xd ^= xa; _rotl(xd, 8, tmp)
    xc += xd; xb ^= xc; _rotl(xb, 7, tmp)


def chacha20_blocks(key: bytes, nonce, counter0: int, nblocks: int) -> np.ndarray:
    """The keystream of blocks counter0 ... counter0 + nblocks - 1 (32-bit counter) under a 256-bit key and the nonce given as
    three 32-bit words: nblocks * 64 bytes."""
    kw = np.frombuffer(bytes(key), dtype="<u4").astype(np.uint32)
    assert kw.size == 8 and len(nonce) == 3
    out = np.empty((nblocks, 16), dtype=np.uint32)
    for b0 in range(0, nblocks, _CHUNK):
        m = min(_CHUNK, nblocks - b0)
        s = np.empty((16, m), dtype=np.uint32)
        s[0:4] = _SIGMA[:, None]
        s[4:12] = kw[:, None]
        s[12] = (np.arange(counter0 + b0, counter0 + b0 + m, dtype=np.uint64) & 0xFFFFFFFF).astype(np.uint32)
        s[13:16] = np.asarray(nonce, dtype=np.uint32)[:, None]
        x = s.copy()
        tmp = np.empty(m, dtype=np.uint32)
        for _ in range(10):
            _quarter_round(x, 0, 4, 8, 12, tmp); _quarter_round(x, 1, 5, 9, 13, tmp)
            _quarter_round(x, 2, 6, 10, 14, tmp); _quarter_round(x, 3, 7, 11, 15, tmp)
            _quarter_round(x, 0, 5, 10, 15, tmp); _quarter_round(x, 1, 6, 11, 12, tmp)
            _quarter_round(x, 2, 7, 8, 13, tmp); _quarter_round(x, 3, 4, 9, 14, tmp)
        x += s
        out[b0:b0 + m] = x.T
    return out.astype("<u4", copy=False).view(np.uint8).reshape(nblocks * 64)


def chacha20_keystream(key: bytes, nonce, nbytes: int, counter0: int = 0) -> np.ndarray:
    return chacha20_blocks(key, nonce, counter0, -(-nbytes // 64))[:nbytes]


# ---- the two forms of the prover's randomness ----
class HarnessRandomness:
    """What the Python harness drew: its salt pool (leaves x 16 bytes) and the MASK_DEGREE mask values."""

    def __init__(self, salt_pool, mask):
        self.pool = np.ascontiguousarray(salt_pool, dtype=np.uint8).reshape(-1, 16)
        self.mask_values = [int(v) for v in mask]

    def salts(self, leaves: int) -> np.ndarray:
        assert leaves <= len(self.pool), "salt pool too short"
        return self.pool[:leaves]

    def mask(self, count: int):
        assert len(self.mask_values) == count
        return list(self.mask_values)


class ChaChaRandomness:
    """The compiled prover's randomness from its key: the salts are the keystream with nonce words (0, 0, 0) from counter 0 (the
    trees' salts at byte offsets 0, 16N, 32N and 48N on); mask value i is bytes [8i, 8i + 8) of the keystream with nonce words
    (0, 1, 0), little-endian, mod p."""
    SALT_NONCE = (0, 0, 0)
    MASK_NONCE = (0, 1, 0)

    def __init__(self, key: bytes):
        self.key = bytes(key)
        assert len(self.key) == 32

    def salts(self, leaves: int) -> np.ndarray:
        return chacha20_keystream(self.key, self.SALT_NONCE, 16 * leaves).reshape(leaves, 16)

    def mask(self, count: int):
        ks = chacha20_keystream(self.key, self.MASK_NONCE, 8 * count).tobytes()
        return [int.from_bytes(ks[8 * i:8 * i + 8], "little") % P for i in range(count)]


# ---- protocol sizes ----
def fri_layer_sizes(n: int):
    """(final layer size, sizes of the folded layers N/2 ... final size) for a trace of n rows."""
    N = n * BLOWUP
    final_size = N // (1 << (n + MASK_DEGREE - 1).bit_length())        # fri_degree_bound = next power of two of n + MASK_DEGREE
    sizes, m = [], N
    while m > final_size:
        m //= 2
        sizes.append(m)
    return final_size, sizes


def salt_leaves(n: int) -> int:
    """Salted leaves of one proof: three LDE-size trees and every FRI layer but the final one."""
    final_size, sizes = fri_layer_sizes(n)
    return 3 * n * BLOWUP + sum(m for m in sizes if m != final_size)


# ---- Merkle trees and opening records ----
def merkle_record_bytes(n: int) -> int:
    """Bytes of one opening record of a tree of n leaves (include/toyni_hip.h section 3c)."""
    d = len(oracle.merkle_level_sizes(n)) - 1
    return 32 * d + 24 + ((d + 7) & ~7)


def _leaf_digest(salt: bytes, value: int) -> bytes:
    return hashlib.sha256(b"\x00" + salt + int(value).to_bytes(8, "little")).digest()


def _levels_above(leaves: np.ndarray):
    levels, cur = [leaves], leaves
    while len(cur) > 1:
        nxt = np.empty(((len(cur) + 1) // 2, 32), dtype=np.uint8)
        for i in range(len(nxt)):
            left = cur[2 * i].tobytes()
            right = cur[2 * i + 1].tobytes() if 2 * i + 1 < len(cur) else left     # odd level: the last node pairs with itself
            nxt[i] = np.frombuffer(hashlib.sha256(b"\x01" + left + right).digest(), dtype=np.uint8)
        levels.append(nxt)
        cur = nxt
    return levels


def serialize_openings(levels, values, salts, indices):
    """Openings of `indices` in the tree `levels` (oracle.merkle_commit_values over values / salts): (the MerkleOpening fields
    as dicts, the records as the device writes them: path | salt (zero if unsalted) | value, 8 LE bytes | position flags |
    zero padding to a multiple of 8)."""
    n = len(levels[0])
    d = len(levels) - 1
    rec = merkle_record_bytes(n)
    raw = np.zeros((len(indices), rec), dtype=np.uint8)
    ops = []
    for k, (i, pp) in enumerate(zip(indices, oracle.merkle_get_proofs(levels, indices))):
        assert pp is not None, f"index {i} outside a tree of {n} leaves"
        path, pos = pp
        i = int(i)
        salt = salts[i].tobytes() if salts is not None else b""
        value = int(values[i])
        r = raw[k]
        if d:
            r[:32 * d] = np.frombuffer(b"".join(path), dtype=np.uint8)
        if salts is not None:
            r[32 * d:32 * d + 16] = salts[i]
        r[32 * d + 16:32 * d + 24] = np.frombuffer(value.to_bytes(8, "little"), dtype=np.uint8)
        r[32 * d + 24:32 * d + 24 + d] = pos
        ops.append({"index": i, "value": value, "path": path, "position": pos, "salt": salt})
    return ops, raw.reshape(-1)


class _Tree:
    """A committed layer.  `hook(name, salts, leaf_digests)` (tests only) may alter the salts or the leaf digests in place before
    the upper levels are built; a leaf whose salt it changed is re-hashed, every other digest is taken as the hook left it."""

    def __init__(self, name, values, salts, hook):
        self.n = len(values)
        self.values = np.asarray(values, dtype=np.uint64)
        self.salts = None if salts is None else np.array(salts, dtype=np.uint8)
        if hook is None:
            self.levels = oracle.merkle_commit_values(self.values, self.salts)
        else:
            leaves = oracle.merkle_commit_values(self.values, self.salts)[0].copy()
            before = None if self.salts is None else self.salts.copy()
            hook(name, self.salts, leaves)
            if before is not None:
                for i in np.nonzero((self.salts != before).any(axis=1))[0]:
                    leaves[i] = np.frombuffer(_leaf_digest(self.salts[i].tobytes(), self.values[i]), dtype=np.uint8)
            self.levels = _levels_above(leaves)
        self.root = self.levels[-1][0].tobytes()

    def open(self, indices):
        return serialize_openings(self.levels, self.values, self.salts, indices)


# ---- the prover ----
def prove(trace, randomness, tree_hook=None):
    """The proof of a trace column (n canonical residues, n a power of two) and every component on the way.  tree_hook: see
    _Tree; its names are "trace", "quotient", "deep", "fri1", "fri2", ... (fri_k = the layer after k folds)."""
    trace = np.asarray(trace, dtype=np.uint64)
    n = int(trace.size)
    assert n >= 2 and n & (n - 1) == 0
    N = n * BLOWUP
    g = root_of_unity(n.bit_length() - 1)
    final_size, sizes = fri_layer_sizes(n)
    pool = randomness.salts(salt_leaves(n))
    taken = [0]

    def take_salts(count):
        s = pool[taken[0]:taken[0] + count]
        taken[0] += count
        return s

    # 1. interpolate, mask (T - R + x^n R; the two ranges overlap when n < MASK_DEGREE), LDE on the coset, commit
    mask = randomness.mask(MASK_DEGREE)
    masked = [int(c) for c in oracle.intt(trace)] + [0] * MASK_DEGREE
    for i, r in enumerate(mask):
        masked[i] = (masked[i] - r) % P
        masked[n + i] = (masked[n + i] + r) % P
    masked = np.array(masked, dtype=np.uint64)
    trace_lde = oracle.domain_fft(masked, N, COSET_SHIFT)
    trace_tree = _Tree("trace", trace_lde, take_salts(N), tree_hook)

    # 2. constraint and quotient evaluations, the two inverse transforms, commit the quotient
    c_evals, q_evals = oracle.fib_quotient(trace_lde, n, COSET_SHIFT)
    c_poly = oracle.domain_ifft(c_evals, COSET_SHIFT)
    q_poly = oracle.domain_ifft(q_evals, COSET_SHIFT)
    quotient_tree = _Tree("quotient", q_evals, take_salts(N), tree_hook)

    # 3./4. transcript, z, out-of-domain values
    tr = Transcript()
    tr.absorb(trace_tree.root)
    tr.absorb(quotient_tree.root)
    z = derive_z(tr, N)
    t_z, t_gz, t_ggz = (oracle.poly_eval(masked, x) for x in (z, g * z % P, g * g % P * z % P))
    q_z = oracle.poly_eval(q_poly, z)
    c_z = (t_ggz - t_gz - t_z) % P * ((z - pow(g, n - 1, P)) % P) % P * ((z - pow(g, n - 2, P)) % P) % P
    assert c_z == q_z * ((pow(z, n, P) - 1) % P) % P, "Constraint check at z failed"
    for v in (t_z, t_gz, t_ggz, q_z):
        tr.absorb_field(v)

    # 5. DEEP layer; 6. FRI: layer k lives on 7^(2^k) <w_(N / 2^k)>; beta_k is squeezed before the next root is absorbed
    deep = oracle.fib_deep(trace_lde, q_evals, n, COSET_SHIFT, z, t_z, t_gz, t_ggz, q_z)
    layers = [deep]
    trees = [_Tree("deep", deep, take_salts(N), tree_hook)]
    commitments = [trees[0].root]
    tr.absorb(commitments[0])
    betas = []
    shift = COSET_SHIFT
    for k, m in enumerate(sizes):
        beta = tr.squeeze_challenge()
        betas.append(beta)
        layers.append(oracle.fri_fold(layers[-1], oracle.domain_elements(2 * m, shift), beta))
        shift = shift * shift % P
        trees.append(_Tree(f"fri{k + 1}", layers[-1], take_salts(m) if m != final_size else None, tree_hook))   # final layer: unsalted
        commitments.append(trees[-1].root)
        tr.absorb(commitments[-1])

    # 7. queries: trace q, q + B, q + 2B; quotient q; DEEP q, q + N/2; FRI layers 1 ... L-1 at their folded positions
    half0 = N // 2
    qidx = tr.squeeze_indices(NUM_QUERIES, half0)
    groups = [(trace_tree, [i for q in qidx for i in (q, (q + BLOWUP) % N, (q + 2 * BLOWUP) % N)]),
              (quotient_tree, list(qidx)),
              (trees[0], [i for q in qidx for i in (q, q + half0)])]
    cur = list(qidx)
    for li in range(1, len(layers) - 1):
        half = len(layers[li]) // 2
        cur = [c % half for c in cur]
        groups.append((trees[li], [i for c in cur for i in (c, c + half)]))
    opened = [t.open(idx) for t, idx in groups]
    t_open, q_open, d_open = (ops for ops, _ in opened[:3])
    fri_open = [ops for ops, _ in opened[3:]]
    query_proofs = []
    for k, qi in enumerate(qidx):
        query_proofs.append({
            "index": qi,
            "trace_opening": t_open[3 * k], "trace_opening_g": t_open[3 * k + 1], "trace_opening_gg": t_open[3 * k + 2],
            "quotient_opening": q_open[k],
            "deep_opening": d_open[2 * k], "deep_opening_pair": d_open[2 * k + 1],
            "fri_openings": [(lo[2 * k], lo[2 * k + 1]) for lo in fri_open],
        })
    proof = {
        "trace_len": n, "lde_size": N, "trace_commitment": trace_tree.root, "quotient_commitment": quotient_tree.root,
        "t_z": t_z, "t_gz": t_gz, "t_ggz": t_ggz, "q_z": q_z, "fri_commitments": commitments,
        "fri_final_layer": [int(v) for v in layers[-1]], "query_proofs": query_proofs,
        "query_indices": qidx,
        "opening_groups": [(t.n, t.salts is not None, idx) for t, idx in groups],
        "opening_records": np.concatenate([raw for _, raw in opened]),
    }
    components = {
        "mask": mask, "masked_coeffs": masked, "trace_lde": trace_lde, "c_evals": c_evals, "q_evals": q_evals, "c_poly": c_poly,
        "q_poly": q_poly, "z": z, "ood": (t_z, t_gz, t_ggz, q_z), "deep": deep, "betas": betas, "fri_layers": layers[1:],
    }
    return proof, components


# ---- comparisons: "" when equal, else the first difference in protocol order ----
def _first_index(name, got, want):
    if isinstance(got, (bytes, bytearray)) or isinstance(want, (bytes, bytearray)):
        got, want = np.frombuffer(bytes(got), dtype=np.uint8), np.frombuffer(bytes(want), dtype=np.uint8)
    a = np.asarray(got, dtype=np.uint64).reshape(-1)
    b = np.asarray(want, dtype=np.uint64).reshape(-1)
    if a.size != b.size:
        return f"{name}: length {a.size}, want {b.size}"
    bad = np.nonzero(a != b)[0]
    if bad.size:
        i = int(bad[0])
        return f"{name}: first difference at index {i} ({int(a[i])} != {int(b[i])}; {bad.size} differ)"
    return ""


def first_component_difference(got: dict, want: dict) -> str:
    """got: a harness capture; want: the components of prove() on the same randomness."""
    for key in COMPONENTS:
        if key not in got:
            return f"{key}: not captured"
        if key == "fri_layers":
            if len(got[key]) != len(want[key]):
                return f"fri_layers: {len(got[key])} layers, want {len(want[key])}"
            for k, (a, b) in enumerate(zip(got[key], want[key])):
                msg = _first_index(f"fri_layers[{k}] (after {k + 1} folds)", a, b)
                if msg:
                    return msg
        else:
            msg = _first_index(key, got[key], want[key])
            if msg:
                return msg
    return ""


def _record_field(byte, d):
    if byte < 32 * d:
        return f"path level {byte // 32}"
    return "salt" if byte < 32 * d + 16 else "value" if byte < 32 * d + 24 else "position" if byte < 33 * d + 24 else "padding"


def first_proof_difference(got: dict, want: dict) -> str:
    """Byte-exact comparison of two proofs in wire form (WIRE_FIELDS), field by field in protocol order: commitments and OOD
    values, every FRI commitment, the final layer, the query indices, the opening groups, then the raw records of each group
    (the first differing byte is named by record, leaf and field).  The roots cover every element of every committed layer."""
    for key in WIRE_FIELDS[:8]:
        if key.endswith("commitment"):
            if bytes(got[key]) != bytes(want[key]):
                return f"{key}: {bytes(got[key]).hex()} != {bytes(want[key]).hex()}"
        elif int(got[key]) != int(want[key]):
            return f"{key}: {int(got[key])} != {int(want[key])}"
    gc, wc = got["fri_commitments"], want["fri_commitments"]
    if len(gc) != len(wc):
        return f"fri_commitments: {len(gc)} roots, want {len(wc)}"
    for k, (a, b) in enumerate(zip(gc, wc)):
        if bytes(a) != bytes(b):
            return f"fri_commitments[{k}]: {bytes(a).hex()} != {bytes(b).hex()}"
    for key in ("fri_final_layer", "query_indices"):
        msg = _first_index(key, got[key], want[key])
        if msg:
            return msg
    gg = [(int(t), bool(s), [int(i) for i in ix]) for t, s, ix in got["opening_groups"]]
    wg = [(int(t), bool(s), [int(i) for i in ix]) for t, s, ix in want["opening_groups"]]
    if gg != wg:
        k = next((k for k, (a, b) in enumerate(zip(gg, wg)) if a != b), min(len(gg), len(wg)))
        return f"opening_groups[{k}] differ ({len(gg)} groups, want {len(wg)})"
    graw = np.asarray(got["opening_records"], dtype=np.uint8).reshape(-1)
    wraw = np.asarray(want["opening_records"], dtype=np.uint8).reshape(-1)
    if graw.size != wraw.size:
        return f"opening_records: {graw.size} bytes, want {wraw.size}"
    off = 0
    for k, (tn, _salted, ix) in enumerate(wg):
        rec = merkle_record_bytes(tn)
        d = len(oracle.merkle_level_sizes(tn)) - 1
        a, b = graw[off:off + rec * len(ix)], wraw[off:off + rec * len(ix)]
        bad = np.nonzero(a != b)[0]
        if bad.size:
            r, byte = divmod(int(bad[0]), rec)
            return (f"opening_records of group {k} (tree of {tn} leaves): record {r} (leaf {ix[r]}), byte {byte} of {rec} "
                    f"({_record_field(byte, d)}; {int(a[bad[0]])} != {int(b[bad[0]])}; {bad.size} bytes differ in the group)")
        off += rec * len(ix)
    return ""
