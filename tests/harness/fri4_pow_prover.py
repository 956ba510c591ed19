"""tests/harness/fri4_ext_prover.py with the proof-of-work step of include/toyni_hip.h 3n: between the commit phase and squeeze_indices
the device transcript grinds a nonce (DeviceTranscript.grind: three more launches, nothing else) and absorbs it.  Still ONE
synchronisation from the Ext coefficients to the opening records; the nonce is downloaded with everything else after it.

fri4_ext_prover.py is not edited: its prove() creates its transcript through toyni_amd.prover.DeviceTranscript, so for the length of
that call the name is bound to a subclass whose squeeze_indices enqueues the grind first.  Test harness: tests/test_gpu_pow_grind.py
hands the proofs to tests/harness/fri4_pow_verifier.py."""
import numpy as np
import torch

import toyni_amd
from harness import fri4_ext_prover as base

layer_sizes = base.layer_sizes


def prove(ctx, coeffs4, log_blowup, shift, final_size, seed, nqueries, rng, bits, bend=None, start=0, log_tries=22, absorb=True):
    """base.prove with a `bits`-bit nonce ground on the device, from `start` on, before the indices.  absorb=False is the deviating
    prover whose indices ignore the nonce (it grinds on a copy of the transcript).  Returns (proof with pow_bits / pow_nonce,
    extras)."""
    pv, dev = toyni_amd.prover, torch.device("cuda", 0)
    d_nonce = torch.full((1,), -1, dtype=torch.int64, device=dev)
    real = pv.DeviceTranscript
    grinds = []                                        # one entry per grind the hook enqueued

    class GrindingTranscript(real):
        def squeeze_indices(self, d_out, count, mx, stream=0):
            grinds.append(bits)
            if absorb:
                self.grind(d_nonce.data_ptr(), bits, start, log_tries, stream)
            else:
                copy = real()
                toyni_amd._lib.check(toyni_amd._lib.lib.toyni_memcpy_d2d_async(copy.ptr, self.ptr, 1024, stream or None), "copy of a transcript")
                copy.grind(d_nonce.data_ptr(), bits, start, log_tries, stream)
                self._copy = copy                      # freed with the tensor's owner, after the synchronisation
            real.squeeze_indices(self, d_out, count, mx, stream)

    pv.DeviceTranscript = GrindingTranscript
    try:
        proof, extras = base.prove(ctx, coeffs4, log_blowup, shift, final_size, seed, nqueries, rng, bend=bend)
    finally:
        pv.DeviceTranscript = real
    # the hook holds only while base.prove looks the class up as toyni_amd.prover.DeviceTranscript at call time: had it bound the
    # name some other way, no grind would have been enqueued and the nonce word would still hold what it was filled with
    assert grinds == [bits], f"the base prover made {len(grinds)} index squeezes through the grinding transcript, not one"
    proof["pow_bits"] = bits
    proof["pow_nonce"] = int(d_nonce.cpu().numpy().view(np.uint64)[0])
    return proof, extras
