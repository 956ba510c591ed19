"""tests/harness/fri4_pow_verifier.py against a prover in Python integers and hashlib alone (no library, no device): the model prover of
tests/test_fri4_ext_verifier_model.py with the grinding step of include/toyni_hip.h 3n hooked in front of its index squeeze, the same
way the verifier hooks it.  The verifier must accept the protocol and reject each deviation of the proof-of-work step, one at a time,
so that a rejection in the GPU test speaks about the device and an acceptance is not a verifier that accepts everything.  Every nonce
comes from tests/pow_model.py."""
import numpy as np

import pow_model as pm
import test_fri4_ext_verifier_model as base
from harness import fri4_ext_verifier as fv, fri4_pow_verifier as pv

BITS = pv.POW_BITS


def prove(layer0, nonce_for, bits=BITS, absorb=True):
    """the model prover's proof with pow_bits / pow_nonce; nonce_for(state) picks the nonce, absorb=False leaves it out of the transcript"""
    used = []

    def pick(state):
        used.append((state, nonce_for(state)))
        return used[-1][1]

    with pv.grinding(pick, absorb=absorb):
        proof = base.prove(layer0)
    assert len(used) == 1 and fv.Transcript.__name__ == "Transcript"          # one grind per proof; the hook is gone again
    proof["pow_bits"], proof["pow_nonce"] = bits, used[0][1]
    return proof, used[0][0]


def _layer0():
    rng = np.random.default_rng(12)
    return base.codeword([tuple(int(v) for v in rng.integers(0, base.P, 4)) for _ in range(base.NCOEFFS)])


def test_the_verifier_accepts_a_ground_proof_and_rejects_each_deviation_of_the_grinding_step():
    layer0 = _layer0()
    proof, state = prove(layer0, lambda s: pm.must_grind(s, BITS))
    nonce = proof["pow_nonce"]
    assert state == pv.state_before_queries(proof) and len(state) == 32 + 32 and pm.accept(state, nonce, BITS)
    assert pv.verify(proof) == (True, "accepted")
    # the nonce moves the indices, and nothing else: the betas are the ungrinded protocol's
    betas, indices = pv.challenges(proof)
    plain_betas, plain_indices = fv.challenges(proof)
    assert betas == plain_betas and indices != plain_indices
    assert fv.verify(proof)[0] is False                                         # the verifier without the step reads other leaves
    # nonce + 1: the hash no longer has the zero bits
    assert not pm.accept(state, nonce + 1, BITS)
    ok, why = pv.verify(dict(proof, pow_nonce=nonce + 1))
    assert not ok and why.startswith("proof of work"), why
    # a nonce that is good for BITS - 1 only, absorbed honestly, presented for BITS
    def weak(s):
        n = 0
        while True:
            n = pm.must_grind(s, BITS - 1, n)
            if not pm.accept(s, n, BITS):
                return n
            n += 1
    cheap, _ = prove(layer0, weak)
    assert pm.accept(state, cheap["pow_nonce"], BITS - 1)
    ok, why = pv.verify(cheap)
    assert not ok and why.startswith("proof of work: the hash"), why
    assert pv.verify(cheap, pow_bits=BITS - 1) == (False, "proof of work: bits or nonce field")      # the proof claims BITS
    assert pv.verify(dict(cheap, pow_bits=BITS - 1), pow_bits=BITS - 1) == (True, "accepted")        # it IS a proof for one bit less
    assert pv.verify(dict(proof, pow_bits=BITS - 1)) == (False, "proof of work: bits or nonce field")  # a prover does not choose the bits
    # a valid nonce that the prover's transcript never absorbed: its indices are the ungrinded ones, its openings at other leaves
    skipped, _ = prove(layer0, lambda s: pm.must_grind(s, BITS), absorb=False)
    assert skipped["pow_nonce"] == nonce
    ok, why = pv.verify(skipped)
    assert not ok and why.startswith("query 0, layer 0"), why
    # a LARGER accepted nonce is still accepted: minimality makes the device prover a function of its inputs; it is not a rule a
    # verifier could check without redoing the search, and it buys no soundness
    second = pm.must_grind(state, BITS, nonce + 1)
    later, _ = prove(layer0, lambda s: pm.must_grind(s, BITS, pm.must_grind(s, BITS) + 1))
    assert later["pow_nonce"] == second > nonce
    assert pv.verify(later) == (True, "accepted")
    # malformed fields
    for bad in (dict(proof, pow_nonce=-1), dict(proof, pow_nonce=1 << 64), dict(proof, pow_nonce=None), {k: v for k, v in proof.items() if k != "pow_bits"}):
        assert pv.verify(bad) == (False, "proof of work: bits or nonce field")


def test_bits_zero_still_absorbs_a_nonce():
    # bits = 0 accepts nonce 0, and the 8 zero bytes ARE absorbed: the proof is not the ungrinded protocol's proof
    layer0 = _layer0()
    proof, state = prove(layer0, lambda s: pm.must_grind(s, 0), bits=0)
    assert proof["pow_nonce"] == 0 and pv.verify(proof, pow_bits=0) == (True, "accepted")
    plain = base.prove(layer0)
    assert fv.verify(plain) == (True, "accepted") and plain["roots"] == proof["roots"]
    assert fv.challenges(plain)[1] != pv.challenges(proof)[1]
    tr = pm.Transcript(state + pm.le64(0))
    assert pv.challenges(proof)[1] == tr.squeeze_indices(fv.NQUERIES, plain["m0"] // 4)
