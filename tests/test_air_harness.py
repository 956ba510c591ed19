"""The verifier of the two-column AIR proof (tests/harness/air_verifier.py: Python integers and hashlib) against the oracle-only prover
(tests/harness/air_ref_prover.py) on the CPU.  The GPU test holds the device prover to that prover byte for byte and to this verifier, so
the pair is checked here first: the verifier accepts an honest proof, and rejects every single deviation below for the reason named --
a verifier that accepted one of them could not tell a wrong rotation, a swapped weight or a missing term on the device either."""
import numpy as np
import pytest

from harness import air_ref_prover, air_verifier
from harness.air_verifier import depth_of, record_bytes
from harness.fib_verifier import P

CASES = [(8, 1), (64, 3)]            # (n, log2 B): (8, 2) and (64, 8)
SEED = 5


def honest_trace(n, seed=SEED):
    rng = np.random.default_rng(1000 + seed)
    return air_ref_prover.true_trace(n, int(rng.integers(0, P)), int(rng.integers(0, P)))


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"n{c[0]}-B{1 << c[1]}")
def honest(request):
    n, log_b = request.param
    cols = honest_trace(n)
    proof, comp = air_ref_prover.prove(cols, log_b, SEED)
    return n, log_b, cols, proof, comp


def rejected_for(proof):
    why = []
    assert air_verifier.verify(proof, why) is False, "the verifier accepted a proof it must reject"
    assert len(why) == 1
    return why[0]


def group_offset(proof, k):
    """(byte offset of group k in the records, its record size, tree leaves, leaf width, indices)."""
    off = 0
    for j, (t, w, _s, ix) in enumerate(proof["opening_groups"]):
        if j == k:
            return off, record_bytes(t, w), t, w, ix
        off += len(ix) * record_bytes(t, w)
    raise IndexError(k)


def with_byte_flipped(proof, group, record, byte_of):
    """A copy of the proof with one byte of one record changed; byte_of(depth, width) -> offset inside the record."""
    bad = dict(proof)
    off, rec, t, w, _ = group_offset(proof, group)
    bad["opening_records"] = proof["opening_records"].copy()
    bad["opening_records"][off + record * rec + byte_of(depth_of(t), w)] ^= 1
    return bad


def test_the_verifier_accepts_the_reference_proof(honest):
    n, log_b, cols, proof, comp = honest
    why = []
    assert air_verifier.verify(proof, why), why
    assert set(proof) == set(air_ref_prover.WIRE_FIELDS)
    assert air_ref_prover.first_proof_difference(proof, air_ref_prover.prove(cols, log_b, SEED)[0]) == ""
    assert air_ref_prover.first_proof_difference(proof, air_ref_prover.prove(cols, log_b, SEED + 1)[0]).startswith("trace_commitment")
    # what the proof of a true trace is made of: a quotient and a DEEP layer of degree < n, B equal values at the end
    assert not comp["q_poly"][n:].any()
    assert len(set(proof["fri_final_layer"])) == 1 and len(proof["fri_final_layer"]) == 1 << log_b
    assert len(proof["fri_commitments"]) == n.bit_length()


def test_the_row_records_are_the_layout_of_the_header(honest):
    """depth x 32 path | 16 salt | width x 8 values | depth flags | zero padding to 8: the first trace record, taken apart by hand."""
    n, log_b, cols, proof, comp = honest
    N = n << log_b
    d = depth_of(N)
    rec = record_bytes(N, 2)
    assert rec == 32 * d + 16 + 16 + ((d + 7) & ~7) and rec % 8 == 0
    r = bytes(proof["opening_records"][:rec])
    i = proof["query_indices"][0]
    assert r[32 * d:32 * d + 16] == air_ref_prover.salt_pool(n, N, SEED)[i].tobytes()
    assert int.from_bytes(r[32 * d + 16:32 * d + 24], "little") == int(comp["trace_lde"][0, i])
    assert int.from_bytes(r[32 * d + 24:32 * d + 32], "little") == int(comp["trace_lde"][1, i])
    assert list(r[32 * d + 32:33 * d + 32]) == [i >> l & 1 for l in range(d)] and not any(r[33 * d + 32:])


def test_one_trace_cell_changed(honest):
    """An honest prover on a false trace is stopped at z: Z_H does not divide the constraints, so the interpolant of the quotient codeword
    is not their quotient.  A prover that forges q(z) to get past that carries a DEEP layer that is no low-degree codeword to the end."""
    n, log_b, cols, _, _ = honest
    wrong = cols.copy()
    wrong[1, n // 2] = (wrong[1, n // 2] + 1) % P
    proof, comp = air_ref_prover.prove(wrong, log_b, SEED)
    assert comp["q_poly"][n:].any()
    assert rejected_for(proof) == "ood"
    forged, _ = air_ref_prover.prove(wrong, log_b, SEED, cheat={"forge_q_z": True})
    assert rejected_for(forged) == "final_not_constant"


@pytest.mark.parametrize("key", air_verifier.OOD_KEYS)
def test_one_out_of_domain_value_off_by_one(honest, key):
    bad = dict(honest[3])
    bad[key] = (bad[key] + 1) % P
    assert rejected_for(bad) == "ood"


@pytest.mark.parametrize("order", [(1, 0, 2, 3), (0, 1, 3, 2), (2, 1, 0, 3)])
def test_constraint_weights_in_another_order(honest, order):
    n, log_b, cols, _, _ = honest
    proof, _ = air_ref_prover.prove(cols, log_b, SEED, cheat={"weights_order": order})
    assert rejected_for(proof) == "ood"


def test_rotated_rows_opened_one_leaf_on(honest):
    n, log_b, cols, _, _ = honest
    proof, _ = air_ref_prover.prove(cols, log_b, SEED, cheat={"rotation_rows": 1})
    assert rejected_for(proof) == "trace_index"


def test_rotated_rows_opened_backwards(honest):
    """i - B for i + B: the other direction of the rotation."""
    n, log_b, cols, _, _ = honest
    proof, _ = air_ref_prover.prove(cols, log_b, SEED, cheat={"rotation_rows": -(1 << log_b)})
    assert rejected_for(proof) == "trace_index"


@pytest.mark.parametrize("record,column", [(0, 0), (1, 1), (15, 0)])
def test_one_byte_of_an_opened_row_flipped(honest, record, column):
    bad = with_byte_flipped(honest[3], 0, record, lambda d, w: 32 * d + 16 + 8 * column)
    assert rejected_for(bad) == "trace_merkle"


@pytest.mark.parametrize("group,name", [(0, "trace_merkle"), (1, "quotient_merkle"), (2, "deep_merkle"), (3, "fri_merkle")])
def test_one_path_byte_flipped(honest, group, name):
    bad = with_byte_flipped(honest[3], group, 3, lambda d, w: 32 * (d - 1) + 7)
    assert rejected_for(bad) == name


def test_one_salt_or_position_or_padding_byte_flipped(honest):
    proof = honest[3]
    assert rejected_for(with_byte_flipped(proof, 0, 2, lambda d, w: 32 * d + 5)) == "trace_merkle"
    assert rejected_for(with_byte_flipped(proof, 1, 2, lambda d, w: 32 * d + 16 + 8 * w)) == "quotient_merkle"
    assert rejected_for(with_byte_flipped(proof, 2, 2, lambda d, w: record_bytes(1 << d, w) - 1)) == "deep_padding"


def test_one_deep_opening_changed(honest):
    """In the record, the path no longer leads to the root."""
    bad = with_byte_flipped(honest[3], 2, 0, lambda d, w: 32 * d + 16)
    assert rejected_for(bad) == "deep_merkle"


def test_one_fold_layer_value_changed(honest):
    bad = with_byte_flipped(honest[3], 3, 1, lambda d, w: 32 * d + 16)
    assert rejected_for(bad) == "fri_merkle"


def tampered_at_a_queried_index(cols, log_b, name, hit):
    """A proof whose prover changed ONE value of the layer `name` before committing it, at an index a query then asks for (the queries
    follow from the commitment, so candidates are tried in turn until one is hit)."""
    N = cols.shape[1] << log_b
    for j in range(N // 2):
        def tamper(layer_name, layer, j=j):
            if layer_name == name:
                layer[j] = (layer[j] + np.uint64(1)) % np.uint64(P)
        proof, _ = air_ref_prover.prove(cols, log_b, SEED, cheat={"tamper": tamper})
        if hit(j, proof["query_indices"]):
            return proof
    raise AssertionError("no candidate index was queried")


def test_one_committed_deep_value_changed(honest):
    """Committed as changed, so every path holds: the recomputation from the opened rows rejects."""
    n, log_b, cols, _, _ = honest
    proof = tampered_at_a_queried_index(cols, log_b, "deep", lambda j, q: j in q)
    assert rejected_for(proof) == "deep_value"


def test_one_committed_fold_value_changed(honest):
    n, log_b, cols, _, _ = honest
    proof = tampered_at_a_queried_index(cols, log_b, "fri1", lambda j, q: j in q)
    assert rejected_for(proof) == "fri_consistency"


def test_one_final_layer_value_changed(honest):
    n, log_b, cols, proof, _ = honest
    bad = dict(proof)
    bad["fri_final_layer"] = list(proof["fri_final_layer"])
    bad["fri_final_layer"][-1] = (bad["fri_final_layer"][-1] + 1) % P
    assert rejected_for(bad) == "final_not_constant"
    # every value changed alike: constant, but not what was committed
    bad["fri_final_layer"] = [(v + 1) % P for v in proof["fri_final_layer"]]
    assert rejected_for(bad) == "final_commitment"
    # committed as changed too: the last fold says otherwise
    def tamper(name, layer):
        if name == f"fri{n.bit_length() - 1}":
            layer[:] = (layer + np.uint64(1)) % np.uint64(P)

    tampered, _ = air_ref_prover.prove(cols, log_b, SEED, cheat={"tamper": tamper})
    assert rejected_for(tampered) == "final_value"


def test_quotient_term_left_out_of_the_deep_sum(honest):
    n, log_b, cols, _, _ = honest
    proof, _ = air_ref_prover.prove(cols, log_b, SEED, cheat={"drop_quotient_term": True})
    assert rejected_for(proof) == "deep_value"


def test_a_wrong_public_first_row_is_rejected(honest):
    bad = dict(honest[3])
    bad["b_0"] = (bad["b_0"] + 1) % P
    assert rejected_for(bad) == "ood"
