"""tests/harness/fri4_ext_verifier.py with the proof-of-work step of include/toyni_hip.h 3n between the last absorbed root and the query
indices.  On Python integers and hashlib (tests/pow_model.py); imports nothing from the library; fri4_ext_verifier.py itself is not
edited.

The proof is fri4_ext_verifier's with two more fields:
    pow_bits      the number of leading zero bits the prover claims; must equal what the verifier demands (a prover does not choose it)
    pow_nonce     a 64-bit integer
With S = the transcript's state after the last root: accept(S, pow_nonce, pow_bits) -- ONE hash -- then the transcript absorbs
LE64(pow_nonce), and the indices are squeezed from that.  Everything else is fri4_ext_verifier.verify.

A verifier does NOT ask for the smallest nonce: minimality is what makes the device prover a function of its inputs, not a soundness
rule; any accepted nonce costs the same expected work to find.

How the step gets into the existing verifier without a copy of it: that module builds its transcript through its global name
`Transcript`, so for the length of one call the name is bound to a subclass whose squeeze_indices absorbs the nonce first (`grinding`
below).  The model prover of tests/test_fri4_pow_verifier_model.py uses the same hook."""
import contextlib

import pow_model as pm
from harness import fri4_ext_verifier as fv

SEED = fv.SEED
NQUERIES = fv.NQUERIES
POW_BITS = 8


@contextlib.contextmanager
def grinding(nonce_for, absorb=True):
    """Inside the block every transcript fri4_ext_verifier creates calls nonce_for(state) right before its index squeeze and, unless
    absorb is False, absorbs the 8 bytes of what it returns."""
    base = fv.Transcript

    class GrindingTranscript(base):
        def squeeze_indices(self, count, mx):
            nonce = nonce_for(self.t)
            if absorb:
                self.absorb(pm.le64(nonce))
            return base.squeeze_indices(self, count, mx)

    fv.Transcript = GrindingTranscript
    try:
        yield
    finally:
        fv.Transcript = base


def state_before_queries(proof, seed=SEED):
    """the transcript's bytes after the last root: what the nonce is ground against"""
    tr = fv.Transcript(seed)
    tr.absorb(proof["root0"])
    for root in proof["roots"]:
        tr.squeeze_ext()
        tr.absorb(root)
    return tr.t


def challenges(proof, seed=SEED):
    """(betas, query indices) for the roots and the nonce in the proof"""
    with grinding(lambda _state: proof["pow_nonce"]):
        return fv.challenges(proof, seed)


def verify(proof, seed=SEED, pow_bits=POW_BITS):
    nonce = proof.get("pow_nonce")
    if proof.get("pow_bits") != pow_bits or not isinstance(nonce, int) or not 0 <= nonce < 1 << 64:
        return False, "proof of work: bits or nonce field"
    if not isinstance(proof.get("root0"), bytes) or not all(isinstance(r, bytes) for r in proof.get("roots", [None])):
        return False, "shape of the proof"
    if not pm.accept(state_before_queries(proof, seed), nonce, pow_bits):
        return False, "proof of work: the hash does not have the leading zero bits"
    with grinding(lambda _state: nonce):
        return fv.verify(proof, seed)
