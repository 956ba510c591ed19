"""Oracle-only prover of the two-column AIR proof -- TEST INFRASTRUCTURE.  The protocol of air_verifier.py, computed with nothing but the
C oracle (oracle/), the numpy models of the constraint program and of the DEEP combination (tests/air_model.py), hashlib trees and the
transcript of fib_verifier.py.  No device code is involved: a proof computed here is what the device prover (air_prover.py) must emit on
the same trace and seed, byte for byte -- the serialized opening records included, padding zero.

    proof, components = prove(cols, log_blowup, seed)

  proof       the fields air_verifier.verify reads (WIRE_FIELDS): sizes, the public first row, roots, out-of-domain values, the final
              layer, "query_indices", "opening_groups" [(tree leaves, leaf width, salted, indices)] and "opening_records" (uint8: the
              records of include/toyni_hip.h 3c / 3d back to back, in group order)
  components  the intermediate values, for a test that wants to say where two provers part

The salts are numpy's default_rng(seed) bytes, 16 per leaf, in the order trace tree, quotient tree, DEEP tree, then every salted folded
layer from the largest down (salt_pool); the device prover uploads the same pool as it is.

`cheat` (tests only) makes a dishonest prover, one deviation per key, everything after it computed as the protocol says:
  "weights_order": a permutation    the constraint weights enter the quotient in that order
  "forge_q_z": True                 q(z) is not evaluated but solved from the constraints at z, whatever the quotient codeword holds
  "drop_quotient_term": True        the DEEP sum leaves the quotient's term out
  "rotation_rows": r                the second row of a query is opened at i + r instead of i + B
  "tamper": f(name, layer)          may change a layer ("deep", "fri1", ...) in place before it is committed"""
import hashlib

import numpy as np

import oracle
from air_model import CELL, CONST, EMIT, MUL, SUB, X, XINV, air_model, deep_model

from . import air_verifier
from .air_verifier import NUM_DEEP_WEIGHTS, NUM_QUERIES, NUM_WEIGHTS, OOD_KEYS, depth_of, opening_plan, record_bytes
from .fib_verifier import COSET_SHIFT, P, Transcript, derive_z, root_of_unity
from .ref_prover import _first_index

WIRE_FIELDS = ("trace_len", "lde_size", "a_0", "b_0", "trace_commitment", "quotient_commitment") + OOD_KEYS + (
    "fri_commitments", "fri_final_layer", "query_indices", "opening_groups", "opening_records")
DEEP_TERMS = ((0, 0), (0, 1), (1, 0), (1, 1))       # (column, rotation) of the four trace terms, in the order of their weights


def true_trace(n, a_0, b_0):
    """a(j + 1) = b(j), b(j + 1) = a(j) b(j) + 1."""
    a, b = [a_0 % P], [b_0 % P]
    for j in range(n - 1):
        a.append(b[j])
        b.append((a[j] * b[j] + 1) % P)
    return np.array([a, b], dtype=np.uint64)


def program(n, a_0, b_0):
    """The four constraints as (op, dst, a, b, imm) tuples, written by hand (the device prover compiles its own with AirBuilder)."""
    last = pow(root_of_unity(n.bit_length() - 1), n - 1, P)
    return [(CELL, 0, 0, 0, 0), (CELL, 1, 0, 0, 1), (CELL, 2, 1, 0, 0), (CELL, 3, 1, 0, 1),          # a(x), b(x), a(gx), b(gx)
            (X, 4, 0, 0, 0), (CONST, 5, 0, 0, last), (SUB, 4, 4, 5, 0),                               # x - last
            (SUB, 2, 2, 1, 0), (MUL, 2, 2, 4, 0), (EMIT, 0, 2, 0, 0),
            (MUL, 5, 0, 1, 0), (SUB, 3, 3, 5, 0), (CONST, 5, 0, 0, 1), (SUB, 3, 3, 5, 0), (MUL, 3, 3, 4, 0), (EMIT, 0, 3, 0, 1),
            (XINV, 4, 0, 0, 1),                                                                       # 1 / (x - 1)
            (CONST, 5, 0, 0, a_0), (SUB, 0, 0, 5, 0), (MUL, 0, 0, 4, 0), (EMIT, 0, 0, 1, 2),
            (CONST, 5, 0, 0, b_0), (SUB, 1, 1, 5, 0), (MUL, 1, 1, 4, 0), (EMIT, 0, 1, 1, 3)]


def layer_sizes(n, N):
    """Sizes of the folded layers N / 2 ... B."""
    return [N >> k for k in range(1, n.bit_length())]


def salt_pool(n, N, seed):
    leaves = 3 * N + sum(layer_sizes(n, N)[:-1])
    return np.random.default_rng(seed).integers(0, 256, (leaves, 16), dtype=np.uint8)


# ---- hashlib trees ----
class Tree:
    """MerkleTree::new over leaf = [salt] || the row's values as 8 LE bytes each; rows: (leaves, width) values."""

    def __init__(self, rows, salts):
        self.rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(len(rows), -1)
        self.n, self.width = self.rows.shape
        self.salts = None if salts is None else np.ascontiguousarray(salts, dtype=np.uint8).reshape(self.n, 16)
        body = self.rows.astype("<u8").view(np.uint8).reshape(self.n, 8 * self.width)
        data = body if self.salts is None else np.concatenate([self.salts, body], axis=1)
        level = [hashlib.sha256(b"\x00" + r.tobytes()).digest() for r in data]
        self.levels = [level]
        while len(level) > 1:
            level = [hashlib.sha256(b"\x01" + level[i] + (level[i + 1] if i + 1 < len(level) else level[i])).digest()
                     for i in range(0, len(level), 2)]
            self.levels.append(level)
        self.root = level[0]

    def records(self, indices):
        """The opening records of `indices` as the device writes them."""
        d = depth_of(self.n)
        rec = record_bytes(self.n, self.width)
        out = np.zeros((len(indices), rec), dtype=np.uint8)
        for k, index in enumerate(indices):
            cur = int(index)
            assert 0 <= cur < self.n
            for l in range(d):
                sib = cur ^ 1
                lvl = self.levels[l]
                out[k, 32 * l:32 * l + 32] = np.frombuffer(lvl[sib] if sib < len(lvl) else lvl[cur], dtype=np.uint8)
                out[k, 32 * d + 16 + 8 * self.width + l] = 1 if (cur & 1 or sib >= len(lvl)) else 0
                cur >>= 1
            if self.salts is not None:
                out[k, 32 * d:32 * d + 16] = self.salts[int(index)]
            out[k, 32 * d + 16:32 * d + 16 + 8 * self.width] = self.rows[int(index)].astype("<u8").view(np.uint8)
        return out.reshape(-1)


# ---- the prover ----
def prove(cols, log_blowup, seed, cheat=None):
    cheat = cheat or {}
    cols = np.asarray(cols, dtype=np.uint64)
    assert cols.ndim == 2 and cols.shape[0] == 2
    n = cols.shape[1]
    assert n >= 2 and n & (n - 1) == 0 and log_blowup >= 1
    B, N = 1 << log_blowup, n << log_blowup
    g = root_of_unity(n.bit_length() - 1)
    a_0, b_0 = int(cols[0, 0]), int(cols[1, 0])
    sizes = layer_sizes(n, N)
    pool = salt_pool(n, N, seed)
    taken = [0]

    def take_salts(count):
        s = pool[taken[0]:taken[0] + count]
        taken[0] += count
        return s

    tamper = cheat.get("tamper", lambda name, layer: None)

    # 1. interpolate both columns, extend to the coset, one row tree
    coeffs = np.stack([oracle.intt(c) for c in cols])
    lde = np.stack([oracle.domain_fft(c, N, COSET_SHIFT) for c in coeffs])
    trace_tree = Tree(lde.T, take_salts(N))
    tr = Transcript()
    tr.absorb(trace_tree.root)

    # 2. the quotient under the squeezed weights
    weights = [tr.squeeze_challenge() for _ in range(NUM_WEIGHTS)]
    used = [weights[k] for k in cheat.get("weights_order", range(NUM_WEIGHTS))]
    insns = program(n, a_0, b_0)
    c_evals, q_evals = (v.astype(np.uint64) for v in air_model(insns, [lde], N, log_blowup, COSET_SHIFT, used))
    quotient_tree = Tree(q_evals, take_salts(N))
    tr.absorb(quotient_tree.root)

    # 3. z and the out-of-domain values
    q_poly = oracle.domain_ifft(q_evals, COSET_SHIFT)
    z = derive_z(tr, N)
    gz = g * z % P
    a_z, a_gz, b_z, b_gz = (oracle.poly_eval(coeffs[c], x) for c in (0, 1) for x in (z, gz))
    q_z = oracle.poly_eval(q_poly, z)
    if cheat.get("forge_q_z"):
        cz = air_verifier.constraints_at(z, n, a_0, b_0, a_z, a_gz, b_z, b_gz)
        q_z = ((weights[0] * cz[0] + weights[1] * cz[1]) * pow((pow(z, n, P) - 1) % P, P - 2, P) + weights[2] * cz[2] + weights[3] * cz[3]) % P
    ood = (a_z, a_gz, b_z, b_gz, q_z)
    for v in ood:
        tr.absorb_field(v)

    # 4. the DEEP layer: the trace matrix, then the quotient as a second matrix of one column on top
    alphas = [tr.squeeze_challenge() for _ in range(NUM_DEEP_WEIGHTS)]
    terms = [(c, r, alphas[t], ood[t]) for t, (c, r) in enumerate(DEEP_TERMS)]
    deep = deep_model(lde, terms, B, COSET_SHIFT, z).astype(np.uint64)
    if not cheat.get("drop_quotient_term"):
        deep = (deep + deep_model(q_evals[None, :], [(0, 0, alphas[4], q_z)], B, COSET_SHIFT, z)) % np.uint64(P)
    tamper("deep", deep)

    # 5. FRI: layer k lives on 7^(2^k) <w_(N / 2^k)>; beta_k is squeezed before the next root is absorbed; the last layer is unsalted
    layers = [deep]
    trees = [Tree(deep, take_salts(N))]
    tr.absorb(trees[0].root)
    betas = []
    shift = COSET_SHIFT
    for k, m in enumerate(sizes):
        betas.append(tr.squeeze_challenge())
        folded = oracle.fri_fold(layers[-1], oracle.domain_elements(2 * m, shift), betas[-1])
        tamper(f"fri{k + 1}", folded)
        layers.append(folded)
        shift = shift * shift % P
        trees.append(Tree(folded, take_salts(m) if m != B else None))
        tr.absorb(trees[-1].root)

    # 6. queries
    qidx = tr.squeeze_indices(NUM_QUERIES, N // 2)
    plan = opening_plan(N, B, n, qidx)
    if "rotation_rows" in cheat:
        plan[0] = ("trace", N, 2, [i for q in qidx for i in (q, (q + cheat["rotation_rows"]) % N)])
    by_name = {"trace": trace_tree, "quotient": quotient_tree, "deep": trees[0]}
    by_name.update({f"fri{k}": trees[k] for k in range(1, len(sizes))})
    records = np.concatenate([by_name[name].records(ix) for name, _, _, ix in plan])
    honest_plan = opening_plan(N, B, n, qidx)        # a cheating prover still claims the indices the verifier expects
    proof = {
        "trace_len": n, "lde_size": N, "a_0": a_0, "b_0": b_0, "trace_commitment": trace_tree.root, "quotient_commitment": quotient_tree.root,
        "a_z": a_z, "a_gz": a_gz, "b_z": b_z, "b_gz": b_gz, "q_z": q_z,
        "fri_commitments": [t.root for t in trees], "fri_final_layer": [int(v) for v in layers[-1]],
        "query_indices": qidx, "opening_groups": [(t, w, True, ix) for _, t, w, ix in honest_plan], "opening_records": records,
    }
    components = {"coeffs": coeffs, "trace_lde": lde, "weights": weights, "c_evals": c_evals, "q_evals": q_evals, "q_poly": q_poly, "z": z,
                  "ood": ood, "alphas": alphas, "deep": deep, "betas": betas, "fri_layers": layers[1:]}
    return proof, components


# ---- comparison: "" when equal, else the first difference in protocol order ----
def _record_field(byte, d, width):
    if byte < 32 * d:
        return f"path level {byte // 32}"
    if byte < 32 * d + 16:
        return "salt"
    if byte < 32 * d + 16 + 8 * width:
        return f"value of column {(byte - 32 * d - 16) // 8}"
    return "position" if byte < 33 * d + 16 + 8 * width else "padding"


def first_proof_difference(got: dict, want: dict) -> str:
    """Byte-exact comparison of two proofs in wire form (WIRE_FIELDS), field by field in protocol order; inside the opening records the
    first differing byte is named by group, record, leaf and field."""
    for key in WIRE_FIELDS[:11]:
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
            return f"fri_commitments[{k}] ({'DEEP layer' if k == 0 else f'after {k} folds'}): {bytes(a).hex()} != {bytes(b).hex()}"
    for key in ("fri_final_layer", "query_indices"):
        msg = _first_index(key, got[key], want[key])
        if msg:
            return msg
    gg = [(int(t), int(w), bool(s), [int(i) for i in ix]) for t, w, s, ix in got["opening_groups"]]
    wg = [(int(t), int(w), bool(s), [int(i) for i in ix]) for t, w, s, ix in want["opening_groups"]]
    if gg != wg:
        k = next((k for k, (a, b) in enumerate(zip(gg, wg)) if a != b), min(len(gg), len(wg)))
        return f"opening_groups[{k}] differ ({len(gg)} groups, want {len(wg)})"
    graw = np.asarray(got["opening_records"], dtype=np.uint8).reshape(-1)
    wraw = np.asarray(want["opening_records"], dtype=np.uint8).reshape(-1)
    if graw.size != wraw.size:
        return f"opening_records: {graw.size} bytes, want {wraw.size}"
    off = 0
    for k, (tn, width, _salted, ix) in enumerate(wg):
        rec, d = record_bytes(tn, width), depth_of(tn)
        a, b = graw[off:off + rec * len(ix)], wraw[off:off + rec * len(ix)]
        bad = np.nonzero(a != b)[0]
        if bad.size:
            r, byte = divmod(int(bad[0]), rec)
            return (f"opening_records of group {k} (tree of {tn} leaves, {width} per leaf): record {r} (leaf {ix[r]}), byte {byte} of {rec} "
                    f"({_record_field(byte, d, width)}; {int(a[bad[0]])} != {int(b[bad[0]])}; {bad.size} bytes differ in the group)")
        off += rec * len(ix)
    return ""
