"""A staged AIR proof under Ext challenges end to end on the device (tests/harness/air_ext_prover.py: the sequence include/toyni_hip.h
spells out in 3h and 3i -- row commitments, toyni_column_scan_ext_device, an emit_ext program under the coordinates of Ext weights,
toyni_poly_eval_ext_batch_device, toyni_deep_combine_ext_device over three matrices, toyni_fri_commit_phase_ext_device, row openings of
width 4 and 8) against two judges that never saw the device:
  1. the oracle-only prover (tests/harness/air_ext_ref_prover.py): the same proof byte for byte, the first differing component named
  2. the verifier (tests/harness/air_ext_verifier.py, Python integers and hashlib): accepts it -- and rejects the device's proofs of a
     false permutation and of a false multiplicity.
The challenges come from one transcript across all stages.  Each device step is pinned on its own model elsewhere; here the 4 x 4
coordinate matrix of a weight used transposed, q(z) recombined without the powers of X, the accumulator columns committed
coordinate-minor, the values at z and g z swapped, a third accumulating DEEP call that overwrites, an Ext beta written in another
order by the phase's callback or a layer opened at a wrong offset inside d_layers fails.

Sizes (n rows, blow-up B, N = n B), each the smallest at which a launch form is met; the boundaries are read from the library and its
source and asserted below.  (16, 2): everything single-workgroup (N = 32 <= MERKLE_TAIL = 512).  (256, 4), N = 1024: still the scan's
single launch (n <= column_scan_ext_tile() = 1024), trees with a level above the tail.  (4096, 4), N = 2^14: four scan tiles, so the
three-launch form; folded layers of several workgroups with trees of their own above the tail.  (8192, 8), N = 2^16: a tree level of
2^15 nodes, past the two-wave node hash (2^TOYNI_MERKLE_COOP_LOG = 2^14), paths of 16 levels.

What a case costs is the reference prover, in Python (the device prover takes milliseconds): air_ext_ref_prover.prove measured on one
CPU core takes 0.01 s at (16, 1), 0.06 s at (256, 2), 0.6 s at (4096, 2) and 2.3 s at (8192, 3), where the base proof's reference
(air_ref_prover.prove) takes 0.8 s at its largest case, (8192, 3), on the same core.  Of the 2.3 s about 1 s is hashlib (five trees of
2^16 leaves against three), 0.8 s the N Ext inversions of the DEEP denominators (ext_model.batch_inverse, shared by the three
matrices) and 0.2 s the two scans; before the out-of-domain evaluations, the base-field inversions and the shared denominators were
taken off the per-element path it was 4.6 s.  A whole case, reference included, ran in under a second on the GPU host."""
import functools
import os
import re

import pytest

from harness import air_ext_ref_prover as ref
from harness import air_ext_verifier as av
from harness.fib_verifier import P

pytestmark = pytest.mark.gpu

SINGLE, TREE_LEVEL, SCAN_TILES, NODE_KERNEL = (16, 1), (256, 2), (4096, 2), (8192, 3)              # (n, log2 B)
CASES = [SINGLE + (0,), SINGLE + (1,), TREE_LEVEL + (0,), TREE_LEVEL + (1,), SCAN_TILES + (0,), NODE_KERNEL + (0,)]   # n, log2 B, seed
FALSE_AT = (64, 2, 2)


@pytest.fixture(scope="module")
def prover():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    from harness import air_ext_prover
    return air_ext_prover


@functools.lru_cache(maxsize=None)
def reference(n, log_b, seed, wrong=None):
    """(main trace, the reference prover's proof), computed once.  wrong: "b" changes one cell of b, "u" one multiplicity."""
    main = ref.true_main(n, seed)
    if wrong == "b":
        main[1, n // 3] = (main[1, n // 3] + 1) % P
    if wrong == "u":
        main[2, n // 2] = (main[2, n // 2] + 1) % P
    main.setflags(write=False)
    return main, ref.prove(main, log_b, seed)[0]


def test_the_cases_straddle_the_launch_boundaries():
    """A changed tile size or threshold fails here instead of silently narrowing what the cases reach."""
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    src = open(os.path.join(os.path.dirname(os.path.abspath(toyni_amd.__file__)), "csrc", "toyni_hip.hip")).read()
    tail = int(re.search(r"constexpr uint32_t MERKLE_TAIL = (\d+);", src).group(1))
    coop = 1 << int(re.search(r'env_int\("TOYNI_MERKLE_COOP_LOG", (\d+)\)', src).group(1))
    assert "TOYNI_MERKLE_COOP_LOG" not in os.environ
    tile = toyni_amd.prover.column_scan_ext_tile()
    size = lambda case: case[0] << case[1]
    assert size(SINGLE) <= tail and SINGLE[0] <= tile                       # one workgroup for every tree, fold and scan
    assert TREE_LEVEL[0] <= tile < SCAN_TILES[0] and SCAN_TILES[0] // tile == 4
    assert size(TREE_LEVEL) > tail                                            # a tree level above the tail
    assert size(SCAN_TILES) // 2 > tail and size(SCAN_TILES) // 2 <= coop     # folded layers with trees above the tail; two-wave node hash
    assert size(NODE_KERNEL) // 2 > coop and av.rc.depth_of(size(NODE_KERNEL)) == 16
    assert {c[:2] for c in CASES} == {SINGLE, TREE_LEVEL, SCAN_TILES, NODE_KERNEL}


@pytest.mark.parametrize("n,log_b,seed", CASES)
def test_device_proof_equals_the_reference_proof_and_verifies(prover, n, log_b, seed):
    main, want = reference(n, log_b, seed)
    got = prover.prove(main, log_b, seed)
    assert ref.first_proof_difference(got, want) == ""
    assert set(got) == set(ref.WIRE_FIELDS)
    why = []
    assert av.verify(got, why), why


@pytest.mark.parametrize("wrong", ["b", "u"])
def test_the_device_proof_of_a_false_trace_is_the_reference_proof_of_it(prover, wrong):
    """One cell of b off, or one multiplicity: the device prover asserts nothing on the way and runs to the end; byte for byte what
    the reference prover makes of the same trace."""
    n, log_b, seed = FALSE_AT
    main, want = reference(n, log_b, seed, wrong)
    got = prover.prove(main, log_b, seed)
    assert ref.first_proof_difference(got, want) == ""
    assert bytes(got["opening_records"]) == bytes(want["opening_records"])


@pytest.mark.parametrize("wrong", ["b", "u"])
def test_the_device_proof_of_a_false_trace_is_rejected(prover, wrong):
    """The verifier stops at z: Z_H does not divide the open transition, so the quotient codeword's interpolant is not its quotient."""
    n, log_b, seed = FALSE_AT
    main, _ = reference(n, log_b, seed, wrong)
    why = []
    assert av.verify(prover.prove(main, log_b, seed), why) is False and why == ["ood"]
