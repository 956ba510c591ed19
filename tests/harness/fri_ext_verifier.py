"""A FRI verifier for an Ext-valued codeword committed by the Ext commit phase (include/toyni_hip.h 3j), on Python integers: Ext from
tests/ext_model.py, paths through tests/rows_common.py's restatement of verify_merkle_proof.  Imports nothing from the library.

The proof it checks (a dict; the test's prover fills it from device buffers):
    m0, x0, final_size          layer 0 has m0 Ext elements on the points x0 w_m0^i; folding stops at final_size
    root0                       the row commitment (width 4, salted) of layer 0
    roots[k]                    the commitment of folded layer k + 1, k < R = log2(m0 / final_size); the last one unsalted
    final_layer                 the final_size Ext elements of layer R
    openings[q][k]              for query q and every layer k <= R: the two opening records (bytes, the format of 3d) at
                                lo = index_q mod (m_k / 2) and lo + m_k / 2

The transcript chains SHA-256 as tests/test_gpu_prover.py does: absorb = append the root, squeeze = hash, feed the hash back, reduce
it little-endian mod p; an Ext challenge is four squeezes; a query index one squeeze mod m0.  Layer 0's root is absorbed before the
first beta, every later root before the next one, the last root before the indices.

verify(proof) replays the transcript from the roots the proof carries and returns (accepted, reason).  Per query and layer it checks
both Merkle paths against the layer's root, that the position flags spell the index asked for, that the record's salt and padding have
the form of the layer (zero salt on the unsalted final layer), and the fold relation
    layer_{k+1}[lo] = (a + b) / 2 + ((a - b) / 2 * beta_k) / x,     a = layer_k[lo], b = layer_k[lo + m_k / 2], x = x0^(2^k) w_{m_k}^lo
between consecutive layers; then that the final layer is constant, hashes to the last root, and holds the opened values."""
import hashlib

import ext_model as em
import rows_common as rc

P = em.P
SEED = b"toyni-fri-ext"
NQUERIES = 8
INV2 = (P + 1) // 2


class Transcript:
    def __init__(self, seed=SEED):
        self.t = seed

    def absorb(self, root: bytes):
        self.t = self.t + root

    def squeeze(self) -> int:
        h = hashlib.sha256(self.t).digest()
        self.t = h
        return int.from_bytes(h, "little")

    def squeeze_ext(self):
        return tuple(self.squeeze() % P for _ in range(4))


def fold_pair(a, b, x, beta):
    """fri_fold_ext (src/math/fri.rs:7-25) of one pair: (a + b) / 2 + ((a - b) / 2 * beta) * x^-1."""
    avg = tuple((u + v) * INV2 % P for u, v in zip(a, b))
    half_diff = tuple((u - v) * INV2 % P for u, v in zip(a, b))
    t, xinv = em.mul(half_diff, beta), pow(x, -1, P)
    return tuple((s + c * xinv) % P for s, c in zip(avg, t))


def challenges(proof):
    """(betas, query indices) the transcript yields for the roots in the proof."""
    tr = Transcript()
    tr.absorb(proof["root0"])
    betas = []
    for k, root in enumerate(proof["roots"]):
        betas.append(tr.squeeze_ext())
        tr.absorb(root)
    return betas, [tr.squeeze() % proof["m0"] for _ in range(NQUERIES)]


def _open(record: bytes, n, salted):
    """(Ext value, leaf bytes, path, flags) of one record, or a string naming what is malformed."""
    if len(record) != 32 * rc.depth_of(n) + 16 + 32 + (rc.depth_of(n) + 7) // 8 * 8:
        return "record length"
    path, salt, vals, flags, pad = rc.split_record(record, n, 4)
    if any(pad) or (not salted and any(salt)) or any(b > 1 for b in record[len(record) - len(pad) - len(flags):len(record) - len(pad)]):
        return "padding, salt or position bytes of the record"
    words = [int.from_bytes(vals[8 * c:8 * c + 8], "little") for c in range(4)]
    if any(w >= P for w in words):
        return "non-canonical value"
    return tuple(words), (salt if salted else b"") + vals, path, flags


def verify(proof):
    m0, x0, final_size = proof["m0"], proof["x0"], proof["final_size"]
    rounds = len(proof["roots"])
    if m0 >> rounds != final_size or len(proof["final_layer"]) != final_size or len(proof["openings"]) != NQUERIES:
        return False, "shape of the proof"
    roots = [proof["root0"]] + list(proof["roots"])
    betas, indices = challenges(proof)
    w0 = pow(em.GEN_2_27, (1 << 27) // m0, P)
    final = [tuple(int(v) for v in e) for e in proof["final_layer"]]
    for q, index in enumerate(indices):
        if len(proof["openings"][q]) != rounds + 1:
            return False, "shape of the proof"
        carried = None                                   # (position, value) the fold of the layer below demands of this layer
        for k in range(rounds + 1):
            m = m0 >> k
            half = max(m // 2, 1)
            lo = index % half
            salted = k < rounds
            got = []
            for pos, record in zip((lo, lo + m // 2), proof["openings"][q][k]):
                o = _open(record, m, salted)
                if isinstance(o, str):
                    return False, f"query {q}, layer {k}: {o}"
                value, leaf, path, flags = o
                if [bool((pos >> l) & 1) for l in range(len(flags))] != flags:
                    return False, f"query {q}, layer {k}: the record is not at position {pos}"
                if not rc.verify_merkle_proof(leaf, path, flags, roots[k]):
                    return False, f"query {q}, layer {k}: Merkle path"
                got.append(value)
            if carried is not None:
                pos, value = carried
                if got[0 if pos == lo else 1] != value:
                    return False, f"query {q}: fold relation between layers {k - 1} and {k}"
            if k < rounds:
                x = pow(x0, 1 << k, P) * pow(w0, (lo << k) % m0, P) % P          # w_{m_k} = w_m0^(2^k)
                carried = (lo, fold_pair(got[0], got[1], x, betas[k]))
            elif got != [final[lo], final[lo + m // 2]] if m > 1 else got[0] != final[0]:
                return False, f"query {q}: the opened final values are not the final layer's"
    if any(e != final[0] for e in final):
        return False, "the final layer is not constant"
    tree = rc.hashlib_levels(rc.leaves_of([list(e) for e in final]))
    if tree[-1][0] != roots[-1]:
        return False, "the final layer does not hash to the last root"
    return True, "accepted"
