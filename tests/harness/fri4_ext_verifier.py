"""A FRI verifier for an Ext-valued codeword committed by the four-to-one commit phase under coset leaves (include/toyni_hip.h 3m), on
Python integers: Ext from tests/ext_model.py, paths through tests/rows_common.py's restatement of verify_merkle_proof, hashlib.  Imports
nothing from the library.

The proof it checks (a dict; a test's prover fills it):
    m0, x0, final_size          layer 0 has m0 Ext elements on the points x0 w_m0^i; folding four to one stops at final_size >= 4;
                                log2(m0 / final_size) = 2 R
    root0                       the coset commitment (salted) of layer 0
    roots[k]                    the coset commitment of layer k + 1, k < R; the last one (the final layer's) unsalted
    final_layer                 the final_size Ext elements of layer R
    openings[q][k]              for query q and every layer k < R: ONE opening record (bytes, the format of 3d with width 16 over
                                m_k / 4 leaves, m_k = m0 >> 2k) at leaf index_q mod (m_k / 4)

The transcript is the reference's (src/transcript.rs, what the device transcript of 3l implements): absorb = append; squeeze = hash the
state, the hash becomes the state, its first 8 bytes little-endian mod p; an Ext challenge is four squeezes; squeeze_indices(count,
max) takes the value mod max and drops repeats.  Layer 0's root is absorbed before the first beta, every later root before the next
one, the last root before the NQUERIES indices, which are drawn below m0 / 4.

verify(proof) replays that transcript from the roots the proof carries and returns (accepted, reason).  Per query and layer k < R, with
j = index mod (m_k / 4): the record's shape, salt and padding; that the position flags spell j; the path against roots[k]; and the fold
relation
    fold(fold(v0, v2; x, beta), fold(v1, v3; x I, beta); x^2, beta^2),   x = x0^(4^k) w_(m_k)^j,  I = w_(m_k)^(m_k / 4),
of the record's four values, which must equal slot j div (m_(k+1) / 4) of the NEXT layer's record (its leaf is j mod (m_(k+1) / 4)),
or final_layer[j] in the last round.  Then: the final layer is constant and hashes, as an unsalted coset tree, to the last root."""
import hashlib

import ext_model as em
import rows_common as rc

P = em.P
SEED = b"toyni-fri4-ext"
NQUERIES = 8
INV2 = (P + 1) // 2
WIDTH = 16


class Transcript:
    """src/transcript.rs:12-72"""

    def __init__(self, seed=SEED):
        self.t = bytes(seed)

    def absorb(self, data: bytes):
        self.t = self.t + data

    def squeeze(self) -> int:
        self.t = hashlib.sha256(self.t).digest()
        return int.from_bytes(self.t[:8], "little") % P

    def squeeze_ext(self):
        return tuple(self.squeeze() for _ in range(4))

    def squeeze_indices(self, count, mx):
        out = []
        while len(out) < count:
            self.t = hashlib.sha256(self.t).digest()
            idx = int.from_bytes(self.t[:8], "little") % mx
            if idx not in out:
                out.append(idx)
        return out


def fold_pair(a, b, x, beta):
    """fri_fold_ext (src/math/fri.rs:7-25) of one pair: (a + b) / 2 + ((a - b) / 2 * beta) * x^-1."""
    avg = tuple((u + v) * INV2 % P for u, v in zip(a, b))
    half_diff = tuple((u - v) * INV2 % P for u, v in zip(a, b))
    t, xinv = em.mul(half_diff, beta), pow(x, -1, P)
    return tuple((s + c * xinv) % P for s, c in zip(avg, t))


def fold_quad(v, x, i_unit, beta):
    """The four values of a coset {x, I x, -x, -I x} (in that order) -> the value at x^4: two pairwise rounds."""
    beta2 = em.mul(beta, beta)
    return fold_pair(fold_pair(v[0], v[2], x, beta), fold_pair(v[1], v[3], x * i_unit % P, beta), x * x % P, beta2)


def rounds_of(m0, final_size):
    """R, or None for sizes the protocol does not allow"""
    if m0 < 1 or final_size < 4 or m0 & (m0 - 1) or final_size & (final_size - 1) or m0 < final_size:
        return None
    d = (m0 // final_size).bit_length() - 1
    return None if d % 2 else d // 2


def coset_leaves(layer, salts=None):
    """the m / 4 leaves (bytes) of a layer given as a list of m Ext tuples; salts: m / 4 items of 16 bytes, or None"""
    n = len(layer) // 4
    out = []
    for j in range(n):
        body = b"".join(int(c).to_bytes(8, "little") for s in range(4) for c in layer[j + s * n])
        out.append((bytes(salts[j]) if salts is not None else b"") + body)
    return out


def challenges(proof, seed=SEED):
    """(betas, query indices) the transcript yields for the roots in the proof."""
    tr = Transcript(seed)
    tr.absorb(proof["root0"])
    betas = []
    for root in proof["roots"]:
        betas.append(tr.squeeze_ext())
        tr.absorb(root)
    return betas, tr.squeeze_indices(NQUERIES, proof["m0"] // 4)


def _open(record: bytes, n):
    """(four Ext values, leaf bytes, path, flags) of one record of a salted layer of n leaves, or a string naming what is malformed."""
    d = rc.depth_of(n)
    if len(record) != 32 * d + 16 + 8 * WIDTH + (d + 7) // 8 * 8:
        return "record length"
    path, salt, vals, flags, pad = rc.split_record(record, n, WIDTH)
    raw_flags = record[32 * d + 16 + 8 * WIDTH:32 * d + 16 + 8 * WIDTH + d]
    if any(pad) or any(b > 1 for b in raw_flags):
        return "padding or position bytes of the record"
    words = [int.from_bytes(vals[8 * c:8 * c + 8], "little") for c in range(WIDTH)]
    if any(w >= P for w in words):
        return "non-canonical value"
    return [tuple(words[4 * s:4 * s + 4]) for s in range(4)], salt + vals, path, flags


def verify(proof, seed=SEED):
    m0, x0, final_size = proof["m0"], proof["x0"], proof["final_size"]
    rounds = rounds_of(m0, final_size)
    if rounds is None or rounds != len(proof["roots"]) or len(proof["final_layer"]) != final_size or len(proof["openings"]) != NQUERIES:
        return False, "shape of the proof"
    roots = [proof["root0"]] + list(proof["roots"])
    betas, indices = challenges(proof, seed)
    final = [tuple(int(v) for v in e) for e in proof["final_layer"]]
    for q, index in enumerate(indices):
        if len(proof["openings"][q]) != rounds:
            return False, "shape of the proof"
        carried = None                                   # the value the fold of the layer below demands, and where
        for k in range(rounds):
            m = m0 >> (2 * k)
            n = m // 4
            j = index % n
            o = _open(proof["openings"][q][k], n)
            if isinstance(o, str):
                return False, f"query {q}, layer {k}: {o}"
            values, leaf, path, flags = o
            if [bool((j >> l) & 1) for l in range(len(flags))] != flags:
                return False, f"query {q}, layer {k}: the record is not at leaf {j}"
            if not rc.verify_merkle_proof(leaf, path, flags, roots[k]):
                return False, f"query {q}, layer {k}: Merkle path"
            if carried is not None:
                slot, value = carried
                if values[slot] != value:
                    return False, f"query {q}: fold relation between layers {k - 1} and {k}"
            w = pow(em.GEN_2_27, (1 << 27) // m, P)
            x = pow(x0, 4 ** k, P) * pow(w, j, P) % P
            folded = fold_quad(values, x, pow(w, m // 4, P), betas[k])
            if k + 1 < rounds:
                carried = (j // (n // 4), folded)         # layer k + 1 has n elements, n / 4 leaves
            elif final[j] != folded:
                return False, f"query {q}: fold relation between layer {k} and the final layer"
    if any(e != final[0] for e in final):
        return False, "the final layer is not constant"
    tree = rc.hashlib_levels(coset_leaves(final))
    if tree[-1][0] != roots[-1]:
        return False, "the final layer does not hash to the last root"
    return True, "accepted"
