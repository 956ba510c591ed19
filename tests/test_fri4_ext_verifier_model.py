"""tests/harness/fri4_ext_verifier.py against a prover written in Python integers and hashlib alone (no library, no device), modelled on
tests/test_fri_ext_verifier_model.py: the verifier must accept what the four-to-one protocol of include/toyni_hip.h 3m produces and
reject each deviation, so that a rejection in the GPU test speaks about the device and an acceptance is not a verifier that accepts
everything.  The quad fold is pinned to the oracle's pairwise fri_fold_ext first."""
import numpy as np

import ext_model as em
import oracle
import rows_common as rc
from harness import fri4_ext_verifier as fv

P = em.P
N, NCOEFFS, SHIFT, FINAL = 1 << 6, 1 << 4, 7, 4
ROUNDS = 2


def test_the_verifiers_quad_fold_is_the_oracles_pairwise_fold_twice():
    rng = np.random.default_rng(3)
    for m, x0 in ((16, 7), (16, P - 1), (64, 123456789)):
        layer = rng.integers(0, P, (m, 4), dtype=np.uint64)
        beta = tuple(int(v) for v in rng.integers(0, P, 4))
        first = oracle.fri_fold_ext(layer, oracle.domain_elements(m, x0), np.array(beta, dtype=np.uint64))
        want = oracle.fri_fold_ext(first, oracle.domain_elements(m // 2, x0 * x0 % P), np.array(em.mul(beta, beta), dtype=np.uint64))
        w, n = pow(em.GEN_2_27, (1 << 27) // m, P), m // 4
        for j in range(n):
            v = [tuple(int(c) for c in layer[j + s * n]) for s in range(4)]
            assert fv.fold_quad(v, x0 * pow(w, j, P) % P, pow(w, n, P), beta) == tuple(int(c) for c in want[j]), (m, j)
    assert fv.rounds_of(64, 4) == 2 and fv.rounds_of(1 << 20, 16) == 8 and fv.rounds_of(16, 4) == 1
    assert fv.rounds_of(32, 4) is None and fv.rounds_of(64, 2) is None and fv.rounds_of(48, 4) is None


def record(levels, leaf_values, salt, pos):
    """One opening record in the format of include/toyni_hip.h 3d (width 16), from hashlib levels."""
    d = len(levels) - 1
    path, flags, cur = [], [], pos
    for l in range(d):
        sib = cur ^ 1
        path.append(levels[l][sib if sib < len(levels[l]) else cur])
        flags.append(cur & 1)
        cur >>= 1
    body = b"".join(path) + (bytes(salt) if salt is not None else bytes(16))
    body += b"".join(int(c).to_bytes(8, "little") for e in leaf_values for c in e) + bytes(flags)
    return body + bytes(-d % 8)


def quad(v, x, i_unit, beta, deviate):
    """fv.fold_quad with the prover's deviations: beta instead of beta^2 in the second fold, the I twist dropped"""
    beta2 = beta if deviate == "beta2 is beta" else em.mul(beta, beta)
    twist = 1 if deviate == "no twist" else i_unit
    return fv.fold_pair(fv.fold_pair(v[0], v[2], x, beta), fv.fold_pair(v[1], v[3], x * twist % P, beta), x * x % P, beta2)


def prove(layer0, deviate=None, at=1):
    """deviate (in round `at`, or in the layer that round commits): "beta", "beta2 is beta", "no twist", "swapped slot",
    "salted final"."""
    rng = np.random.default_rng(9)
    layers, all_salts, trees = [list(layer0)], [], []
    salts = rng.integers(0, 256, (N // 4, 16), dtype=np.uint8)
    all_salts.append(salts)
    trees.append(rc.hashlib_levels(fv.coset_leaves(layer0, salts)))
    tr = fv.Transcript()
    tr.absorb(trees[0][-1][0])
    roots, committed = [], [list(layer0)]          # committed[k]: the layer as the prover laid it under its leaves
    for k in range(ROUNDS):
        beta = tr.squeeze_ext()
        if deviate == "beta" and k == at:
            beta = em.add(beta, em.ONE)
        cur, m = layers[-1], len(layers[-1])
        n, w = m // 4, pow(em.GEN_2_27, (1 << 27) // m, P)
        xk = pow(SHIFT, 4 ** k, P)
        dev = deviate if k == at else None
        layers.append([quad([cur[j + s * n] for s in range(4)], xk * pow(w, j, P) % P, pow(w, n, P), beta, dev) for j in range(n)])
        laid = list(layers[-1])
        if deviate == "swapped slot" and k + 1 == at:      # quarters 1 and 2 of the committed layer change places
            q = len(laid) // 4
            laid = laid[:q] + laid[2 * q:3 * q] + laid[q:2 * q] + laid[3 * q:]
        committed.append(laid)
        last = k == ROUNDS - 1
        salts = rng.integers(0, 256, (n // 4, 16), dtype=np.uint8) if (not last or deviate == "salted final") else None
        all_salts.append(salts)
        trees.append(rc.hashlib_levels(fv.coset_leaves(laid, salts)))
        roots.append(trees[-1][-1][0])
        tr.absorb(roots[-1])
    indices = tr.squeeze_indices(fv.NQUERIES, N // 4)
    openings = []
    for i in indices:
        per_layer = []
        for k in range(ROUNDS):
            n = len(committed[k]) // 4
            j = i % n
            per_layer.append(record(trees[k], [committed[k][j + s * n] for s in range(4)], all_salts[k][j], j))
        openings.append(per_layer)
    return {"m0": N, "x0": SHIFT, "final_size": FINAL, "root0": trees[0][-1][0], "roots": roots, "final_layer": layers[-1], "openings": openings}


def _eval(coeffs, x):
    """sum_i coeffs[i] x^i: Ext coefficients at a base-field point."""
    acc = em.ZERO
    for c in reversed(coeffs):
        acc = tuple((a * x + b) % P for a, b in zip(acc, c))
    return acc


def codeword(coeffs):
    return [_eval(coeffs, x) for x in em.coset_points(N, SHIFT)]


def test_the_verifier_accepts_the_protocol_and_rejects_each_deviation():
    rng = np.random.default_rng(12)
    coeffs = [tuple(int(v) for v in rng.integers(0, P, 4)) for _ in range(NCOEFFS)]
    layer0 = codeword(coeffs)
    proof = prove(layer0)
    assert fv.verify(proof) == (True, "accepted")
    assert len(set(proof["final_layer"])) == 1 and len(proof["roots"]) == ROUNDS and len(proof["final_layer"]) == FINAL
    assert len(set(fv.challenges(proof)[1])) == fv.NQUERIES and all(i < N // 4 for i in fv.challenges(proof)[1])
    # a word that is not low degree: honest folds, honest paths, no constant at the end
    bent = list(layer0)
    bent[21] = em.add(bent[21], (0, 0, 1, 0))
    assert fv.verify(prove(bent)) == (False, "the final layer is not constant")
    # a beta that is not the transcript's, in either round
    ok, why = fv.verify(prove(layer0, "beta", at=0))
    assert not ok and "fold relation between layers 0 and 1" in why, why
    ok, why = fv.verify(prove(layer0, "beta", at=1))
    assert not ok and "fold relation between layer 1 and the final layer" in why, why
    # beta in place of beta^2 in the second fold; the twist by I dropped from the second pair
    for deviate in ("beta2 is beta", "no twist"):
        for at, where in ((0, "between layers 0 and 1"), (1, "between layer 1 and the final layer")):
            ok, why = fv.verify(prove(layer0, deviate, at=at))
            assert not ok and "fold relation " + where in why, (deviate, at, why)
    # two slots of layer 1's leaves exchanged: honest values, honest paths, the wrong place
    ok, why = fv.verify(prove(layer0, "swapped slot", at=1))
    assert not ok and "fold relation" in why, why
    # a final layer committed with salts
    assert fv.verify(prove(layer0, "salted final")) == (False, "the final layer does not hash to the last root")
    # one changed byte anywhere in one record: path, salt, values, position flags, padding
    for layer in range(ROUNDS):
        rec_len = len(proof["openings"][2][layer])
        for at in range(rec_len):
            bad = dict(proof, openings=[list(q) for q in proof["openings"]])
            rec = bytearray(bad["openings"][2][layer])
            rec[at] ^= 0x40
            bad["openings"][2][layer] = bytes(rec)
            ok, why = fv.verify(bad)
            assert not ok and why.startswith(f"query 2, layer {layer}"), (layer, at, why)
    # a tampered root: the transcript moves, and with it every challenge
    for which in ("root0", 0, 1):
        bad = dict(proof, roots=list(proof["roots"]))
        if which == "root0":
            bad["root0"] = bytes([proof["root0"][0] ^ 1]) + proof["root0"][1:]
        else:
            bad["roots"][which] = bytes([proof["roots"][which][0] ^ 1]) + proof["roots"][which][1:]
        assert not fv.verify(bad)[0], which
    # a final layer that is not the committed one
    bad = dict(proof, final_layer=[em.add(e, em.ONE) for e in proof["final_layer"]])
    assert not fv.verify(bad)[0]
    # shapes the protocol does not allow
    assert fv.verify(dict(proof, final_size=2)) == (False, "shape of the proof")
    assert fv.verify(dict(proof, roots=proof["roots"][:1])) == (False, "shape of the proof")
