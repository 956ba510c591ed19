"""tests/harness/fri_ext_verifier.py against a prover written in Python integers and hashlib alone (no library, no device): the verifier
must accept what the protocol produces and reject each deviation the GPU test feeds it, so that a rejection there speaks about the
device and an acceptance is not a verifier that accepts everything.  The fold is pinned to the oracle's fri_fold_ext first."""
import numpy as np

import ext_model as em
import oracle
import rows_common as rc
from harness import fri_ext_verifier as fv

P = em.P
N, NCOEFFS, SHIFT, FINAL = 1 << 6, 1 << 4, 7, 4


def test_the_verifiers_fold_is_the_oracles():
    rng = np.random.default_rng(3)
    for x in (1, P - 1, 7, 123456789):
        for _ in range(4):
            a, b, beta = (tuple(int(v) for v in rng.integers(0, P, 4)) for _ in range(3))
            want = oracle.fri_fold_ext(np.array([a, b], dtype=np.uint64), np.array([x], dtype=np.uint64), np.array(beta, dtype=np.uint64))
            assert fv.fold_pair(a, b, x, beta) == tuple(int(v) for v in want[0])


def record(levels, layer, salts, pos):
    """One opening record in the format of include/toyni_hip.h 3d, from hashlib levels."""
    n, d = len(layer), rc.depth_of(len(layer))
    path, flags, cur = [], [], pos
    for l in range(d):
        sib = cur ^ 1
        path.append(levels[l][sib if sib < len(levels[l]) else cur])
        flags.append(cur & 1)
        cur >>= 1
    body = b"".join(path) + (salts[pos].tobytes() if salts is not None else bytes(16))
    body += b"".join(int(v).to_bytes(8, "little") for v in layer[pos]) + bytes(flags)
    return body + bytes(-d % 8)


def prove(layer0, wrong_beta_round=None):
    rng = np.random.default_rng(9)
    layers, all_salts, trees = [list(layer0)], [], []
    m, rounds = N, (N // FINAL).bit_length() - 1
    salts = rng.integers(0, 256, (N, 16), dtype=np.uint8)
    all_salts.append(salts)
    trees.append(rc.hashlib_levels(rc.leaves_of([list(e) for e in layer0], salts)))
    tr = fv.Transcript()
    tr.absorb(trees[0][-1][0])
    roots = []
    xs = em.coset_points(N, SHIFT)
    for k in range(rounds):
        beta = tr.squeeze_ext()
        if k == wrong_beta_round:
            beta = em.add(beta, em.ONE)
        cur, half = layers[-1], len(layers[-1]) // 2
        pts = [pow(x, 1 << k, P) for x in xs[:half]]                                # (x0 w^i)^(2^k), i < m_k / 2
        layers.append([fv.fold_pair(cur[i], cur[i + half], pts[i], beta) for i in range(half)])
        salts = rng.integers(0, 256, (half, 16), dtype=np.uint8) if k < rounds - 1 else None
        all_salts.append(salts)
        trees.append(rc.hashlib_levels(rc.leaves_of([list(e) for e in layers[-1]], salts)))
        roots.append(trees[-1][-1][0])
        tr.absorb(roots[-1])
    indices = [tr.squeeze() % N for _ in range(fv.NQUERIES)]
    openings = [[[record(trees[k], layers[k], all_salts[k], p) for p in (i % (len(layers[k]) // 2), i % (len(layers[k]) // 2) + len(layers[k]) // 2)]
                 for k in range(rounds + 1)] for i in indices]
    return {"m0": N, "x0": SHIFT, "final_size": FINAL, "root0": trees[0][-1][0], "roots": roots, "final_layer": layers[-1], "openings": openings}


def codeword(coeffs):
    return [_eval(coeffs, x) for x in em.coset_points(N, SHIFT)]


def _eval(coeffs, x):
    """sum_i coeffs[i] x^i: Ext coefficients at a base-field point."""
    acc = em.ZERO
    for c in reversed(coeffs):
        acc = tuple((a * x + b) % P for a, b in zip(acc, c))
    return acc


def test_the_verifier_accepts_the_protocol_and_rejects_each_deviation():
    rng = np.random.default_rng(12)
    coeffs = [tuple(int(v) for v in rng.integers(0, P, 4)) for _ in range(NCOEFFS)]
    layer0 = codeword(coeffs)
    proof = prove(layer0)
    assert fv.verify(proof) == (True, "accepted")
    assert len(set(proof["final_layer"])) == 1 and len(proof["roots"]) == 4
    # a word that is not low degree: honest folds, honest paths, no constant at the end
    bent = list(layer0)
    bent[21] = em.add(bent[21], (0, 0, 1, 0))
    assert fv.verify(prove(bent)) == (False, "the final layer is not constant")
    # a beta that is not the transcript's
    ok, why = fv.verify(prove(layer0, wrong_beta_round=1))
    assert not ok and "fold relation between layers 1 and 2" in why, why
    # one changed byte anywhere in one record: path, salt, values, position flags, padding
    rec_len = len(proof["openings"][2][1][0])
    for at in range(rec_len):
        bad = dict(proof, openings=[[list(layer) for layer in q] for q in proof["openings"]])
        rec = bytearray(bad["openings"][2][1][0])
        rec[at] ^= 0x40
        bad["openings"][2][1][0] = bytes(rec)
        ok, why = fv.verify(bad)
        assert not ok and why.startswith("query 2, layer 1"), (at, why)
    # a final layer that is not the committed one
    bad = dict(proof, final_layer=[em.add(e, em.ONE) for e in proof["final_layer"]])
    assert not fv.verify(bad)[0]
