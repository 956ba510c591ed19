"""A two-column AIR proof end to end on the device (tests/harness/air_prover.py: row commitment, constraint program, batched
out-of-domain evaluation, DEEP combination over two matrices, the FRI commit phase, row and group openings -- include/toyni_hip.h
3d / 3e / 3f composed) against two judges that never saw the device:
  1. the oracle-only prover (tests/harness/air_ref_prover.py): the same proof byte for byte, the first differing component named
  2. the verifier (tests/harness/air_verifier.py, Python integers and hashlib): accepts it -- and rejects the device's proof of a
     false trace.
Each device step is pinned on its own model elsewhere; here a wrong rotation direction, c taken for q, weights in another order, a
second matrix that overwrites instead of accumulating or a row leaf laid out differently from what a verifier hashes fails.

Sizes (n rows, blow-up B, N = n B).  (8, 2) and (64, 8): every tree is the single-workgroup tail (N <= 512 = MERKLE_TAIL of
toyni_hip.hip), every fold one workgroup.  (1024, 8), N = 8192: the row tree and the DEEP / quotient trees run 32 leaf workgroups and
four levels of the two-wave node hash (up <= 2^TOYNI_MERKLE_COOP_LOG = 2^14) before the tail, the commit phase folds layers of 16 ... 2
workgroups with trees of their own above the tail, and the openings read paths of 13 levels.  Two gates sit higher, and (8192, 8),
N = 2^16, is there for them: the group opener stays at one workgroup per tree while 16 openings x (depth + 1) <= 256, i.e. up to
depth 15, and a level of more than 2^14 nodes leaves the two-wave node hash for the one-thread-per-node kernel (the first level above
2^16 leaves has 2^15 nodes).  (The commit phase has no single-launch form for small rounds: the one that was measured was not kept.)"""
import numpy as np
import pytest

from harness import air_ref_prover, air_verifier
from harness.fib_verifier import P

pytestmark = pytest.mark.gpu

CASES = [(8, 1, 0), (8, 1, 1), (64, 3, 0), (64, 3, 1), (1024, 3, 0), (1024, 3, 1), (8192, 3, 0)]      # n, log2 B, seed


@pytest.fixture(scope="module")
def prover():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    from harness import air_prover
    return air_prover


def trace_of(n, seed):
    rng = np.random.default_rng(77 + seed)
    return air_ref_prover.true_trace(n, int(rng.integers(0, P)), int(rng.integers(0, P)))


@pytest.mark.parametrize("n,log_b,seed", CASES)
def test_device_proof_equals_the_reference_proof_and_verifies(prover, n, log_b, seed):
    cols = trace_of(n, seed)
    got = prover.prove(cols, log_b, seed)
    want, _ = air_ref_prover.prove(cols, log_b, seed)
    assert set(got) == set(air_ref_prover.WIRE_FIELDS)
    assert air_ref_prover.first_proof_difference(got, want) == ""
    why = []
    assert air_verifier.verify(got, why), why


def test_the_device_proof_of_a_false_trace_is_rejected(prover):
    """One cell off: the device prover asserts nothing on the way and runs to the end; its proof is still the reference prover's, and
    the verifier stops at z (Z_H does not divide the constraints, so the quotient codeword's interpolant is not their quotient)."""
    n, log_b, seed = 64, 3, 2
    cols = trace_of(n, seed)
    cols[1, n // 2] = (cols[1, n // 2] + 1) % P
    got = prover.prove(cols, log_b, seed)
    assert air_ref_prover.first_proof_difference(got, air_ref_prover.prove(cols, log_b, seed)[0]) == ""
    why = []
    assert air_verifier.verify(got, why) is False and why == ["ood"]
