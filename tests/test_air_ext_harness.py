"""The verifier of the staged AIR proof under Ext challenges (tests/harness/air_ext_verifier.py: Python integers, ext_model's scalar
functions and hashlib) against the oracle-only prover (tests/harness/air_ext_ref_prover.py) on the CPU.  The GPU test holds the device
prover to that prover byte for byte and to this verifier, so the pair is checked here first: the verifier accepts an honest proof, and
rejects every single deviation below for the reason named -- a verifier that accepted one of them could not tell a transposed weight
matrix, an accumulator committed coordinate-minor, swapped values at z and g z or a lost DEEP matrix on the device either."""
import numpy as np
import pytest

import ext_model as em
import oracle
from harness import air_ext_ref_prover as ref
from harness import air_ext_verifier as av
from harness.air_ext_verifier import record_bytes
from harness.fib_verifier import COSET_SHIFT, P
from rows_common import depth_of

CASES = [(8, 1), (64, 2)]            # (n, log2 B)
SEED = 5
GROUPS = {"main": 0, "acc": 1, "quotient": 2, "deep": 3, "fri": 4}      # the first group of every tree kind in wire order


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"n{c[0]}-B{1 << c[1]}")
def honest(request):
    n, log_b = request.param
    main = ref.true_main(n, SEED)
    proof, comp = ref.prove(main, log_b, SEED)
    return n, log_b, main, proof, comp


def rejected_for(proof):
    why = []
    assert av.verify(proof, why) is False, "the verifier accepted a proof it must reject"
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


def with_byte_changed(proof, group, record, byte_of, xor=1):
    """A copy of the proof with one byte of one record changed; byte_of(depth, width) -> offset inside the record."""
    bad = dict(proof)
    off, rec, t, w, _ = group_offset(proof, group)
    bad["opening_records"] = proof["opening_records"].copy()
    bad["opening_records"][off + record * rec + byte_of(depth_of(t), w)] ^= xor
    return bad


def test_the_verifier_accepts_the_reference_proof(honest):
    n, log_b, main, proof, comp = honest
    why = []
    assert av.verify(proof, why), why
    assert set(proof) == set(ref.WIRE_FIELDS)
    # what the proof of a true trace is made of: both accumulators return to where they began, a quotient of degree < n in every
    # coordinate, B equal elements at the end
    assert comp["totals"] == (em.ONE, em.ZERO)
    assert not comp["q_coeffs"][:, n - 1:].any() and comp["q_coeffs"][:, :n - 1].any(axis=1).all()
    assert len(set(proof["fri_final_layer"])) == 1 and len(proof["fri_final_layer"]) == 1 << log_b
    assert len(proof["fri_commitments"]) == n.bit_length()
    assert any(comp["z"][1:]) and all(any(c[1:]) for c in [comp["gamma"]] + comp["alphas"] + comp["betas"])


def test_proving_twice_gives_equal_bytes_and_another_seed_parts_at_the_main_root(honest):
    n, log_b, main, proof, _ = honest
    again, _ = ref.prove(main, log_b, SEED)
    assert ref.first_proof_difference(again, proof) == ""
    assert bytes(again["opening_records"]) == bytes(proof["opening_records"]) and again["fri_commitments"] == proof["fri_commitments"]
    assert ref.first_proof_difference(ref.prove(main, log_b, SEED + 1)[0], proof).startswith("main_commitment")


def test_the_vectorised_prover_equals_the_scalar_one():
    """The default path inverts the scans' denominators behind one inversion and evaluates through tables of powers; scalar=True does one
    Ext inversion per term and Horner in Python.  Equal proofs, and equal intermediate values."""
    main = ref.true_main(64, SEED)
    fast, cf = ref.prove(main, 2, SEED)
    slow, cs = ref.prove(main, 2, SEED, scalar=True)
    assert ref.first_proof_difference(fast, slow) == ""
    assert (cf["acc"] == cs["acc"]).all() and cf["ood"] == cs["ood"] and cf["totals"] == cs["totals"]
    z = cf["z"]
    table = ref.powers_of(z, 67)
    assert tuple(int(v) for v in table[66]) == em.power(z, 66) and tuple(int(v) for v in table[1]) == z


def test_a_width_8_record_taken_apart_shows_the_coordinate_major_layout(honest):
    """depth x 32 path | 16 salt | 8 x 8 values | depth flags | zero padding to 8: the first accumulator record, by hand.  Its values are
    the LDE of Z's four coordinate columns, then of S's; row 1 of those columns is the first step of each scan, computed here in Ext."""
    n, log_b, main, proof, comp = honest
    N = n << log_b
    d = depth_of(N)
    off, rec, t, w, ix = group_offset(proof, GROUPS["acc"])
    assert (t, w) == (N, 8) and rec == 32 * d + 16 + 64 + ((d + 7) & ~7) and rec % 8 == 0
    assert ix[0] == proof["query_indices"][0] and ix[1] == (ix[0] + (1 << log_b)) % N
    r = bytes(proof["opening_records"][off:off + rec])
    i = ix[0]
    assert r[32 * d:32 * d + 16] == ref.salt_pool(n, N, SEED)[N + i].tobytes()                 # the second tree's salts
    values = [int.from_bytes(r[32 * d + 16 + 8 * c:32 * d + 24 + 8 * c], "little") for c in range(8)]
    assert list(r[32 * d + 80:33 * d + 80]) == [i >> l & 1 for l in range(d)] and not any(r[33 * d + 80:])
    gamma = comp["gamma"]
    a, b, u, w_ = (int(col[0]) for col in main)
    z1 = em.mul(em.add(gamma, em.embed(a)), em.inverse(em.add(gamma, em.embed(b))))
    s1 = em.mul(em.embed(u), em.inverse(em.add(gamma, em.embed(w_))))
    acc = comp["acc"]
    assert tuple(int(v) for v in acc[0:4, 0]) == em.ONE and tuple(int(v) for v in acc[4:8, 0]) == em.ZERO
    assert tuple(int(v) for v in acc[0:4, 1]) == z1 and tuple(int(v) for v in acc[4:8, 1]) == s1
    lde = [oracle.domain_fft(oracle.intt(acc[c]), N, COSET_SHIFT) for c in range(8)]
    assert values == [int(lde[c][i]) for c in range(8)]


CHEATS = [("weight_coordinates_transposed", True, "ood"), ("gamma_reversed", True, "ood"), ("acc_coordinate_minor", True, "ood"),
          ("q_z_without_powers", True, "q_recombination"), ("swap_z_gz", True, "ood"), ("drop_q_terms", True, "deep_value"),
          ("overwrite_second_matrix", True, "deep_value"), ("rotation_rows", 1, "acc_index"), ("rotation_rows", "backwards", "acc_index"),
          ("beta_reversed", True, "fri_consistency")]


@pytest.mark.parametrize("key,value,reason", CHEATS, ids=[f"{k}-{v}" for k, v, _ in CHEATS])
def test_every_cheat_is_rejected_for_its_reason(honest, key, value, reason):
    n, log_b, main, honest_proof, _ = honest
    if value == "backwards":
        value = -(1 << log_b)                     # i - B for i + B: the other direction of the rotation
    proof, _ = ref.prove(main, log_b, SEED, cheat={key: value})
    assert ref.first_proof_difference(proof, honest_proof) != ""
    assert rejected_for(proof) == reason


def test_one_changed_cell_of_b_is_rejected_at_z(honest):
    """An honest prover on a false permutation: the product does not return to 1, Z_H does not divide constraint 0, and the interpolant
    of the quotient codeword is not the constraints' quotient."""
    n, log_b, main, _, _ = honest
    wrong = main.copy()
    wrong[1, n // 3] = (wrong[1, n // 3] + 1) % P
    proof, comp = ref.prove(wrong, log_b, SEED)
    assert comp["totals"][0] != em.ONE and comp["totals"][1] == em.ZERO and comp["q_coeffs"][:, n:].any()
    assert rejected_for(proof) == "ood"


def test_one_changed_multiplicity_is_rejected_at_z(honest):
    n, log_b, main, _, _ = honest
    wrong = main.copy()
    wrong[2, n // 2] = (wrong[2, n // 2] + 1) % P
    proof, comp = ref.prove(wrong, log_b, SEED)
    assert comp["totals"][0] == em.ONE and comp["totals"][1] != em.ZERO and comp["q_coeffs"][:, n:].any()
    assert rejected_for(proof) == "ood"


@pytest.mark.parametrize("field,entry,coordinate", [("ood_main", 0, 0), ("ood_main", 3, 2), ("ood_acc", 0, 0), ("ood_acc", 1, 3), ("ood_acc", 9, 1),
                                                    ("ood_acc", 14, 0), ("ood_q", 0, 0), ("ood_q", 3, 3)])
def test_one_out_of_domain_word_off_by_one(honest, field, entry, coordinate):
    bad = dict(honest[3])
    vals = [list(v) for v in bad[field]]
    vals[entry][coordinate] = (vals[entry][coordinate] + 1) % P
    bad[field] = [tuple(v) for v in vals]
    assert rejected_for(bad) == ("q_recombination" if field == "ood_q" else "ood")


def test_a_q_z_that_is_not_the_recombination(honest):
    bad = dict(honest[3])
    bad["q_z"] = em.add(bad["q_z"], em.ONE)
    assert rejected_for(bad) == "q_recombination"
    bad["q_z"] = (P,) + tuple(bad["q_z"][1:])
    assert rejected_for(bad) == "value_range"


@pytest.mark.parametrize("kind", list(GROUPS))
def test_one_byte_of_a_record_of_each_tree_kind(honest, kind):
    """A path byte, a salt byte, a value byte, a position flag (to the other side, and to a value that is no flag) and a padding byte."""
    n, log_b, main, proof, _ = honest
    group = GROUPS[kind]
    last = len(group_offset(proof, group)[4]) - 1
    assert rejected_for(with_byte_changed(proof, group, 3, lambda d, w: 32 * (d - 1) + 7)) == kind + "_merkle"
    assert rejected_for(with_byte_changed(proof, group, 0, lambda d, w: 7)) == kind + "_merkle"
    assert rejected_for(with_byte_changed(proof, group, 2, lambda d, w: 32 * d + 5)) == kind + "_merkle"
    assert rejected_for(with_byte_changed(proof, group, 1, lambda d, w: 32 * d + 16)) == kind + "_merkle"
    assert rejected_for(with_byte_changed(proof, group, last, lambda d, w: 32 * d + 16 + 8 * (w - 1) + 1)) == kind + "_merkle"
    assert rejected_for(with_byte_changed(proof, group, 2, lambda d, w: 32 * d + 16 + 8 * w)) == kind + "_merkle"
    assert rejected_for(with_byte_changed(proof, group, 2, lambda d, w: 32 * d + 16 + 8 * w + d - 1, xor=2)) == kind + "_position"
    assert rejected_for(with_byte_changed(proof, group, 5, lambda d, w: 32 * d + 16 + 8 * (w - 1) + 7, xor=0x80)) == "value_range"
    _, rec, t, w, _ = group_offset(proof, group)
    padding = rec - (33 * depth_of(t) + 16 + 8 * w)
    assert padding > 0 or n != 8, "at n = 8 every opened tree has a depth that is no multiple of 8"
    if padding:
        assert rejected_for(with_byte_changed(proof, group, last, lambda d, w: record_bytes(1 << d, w) - 1)) == kind + "_padding"
        assert rejected_for(with_byte_changed(proof, group, 0, lambda d, w: 33 * d + 16 + 8 * w, xor=0x10)) == kind + "_padding"


def test_the_claimed_indices_and_groups_are_held_to_the_transcript(honest):
    proof = honest[3]
    bad = dict(proof, query_indices=[proof["query_indices"][1], proof["query_indices"][0]] + proof["query_indices"][2:])
    assert rejected_for(bad) == "query_index"
    groups = list(proof["opening_groups"])
    t, w, s, ix = groups[1]
    groups[1] = (t, w, s, [ix[1], ix[0]] + ix[2:])
    assert rejected_for(dict(proof, opening_groups=groups)) == "opening_groups"
    assert rejected_for(dict(proof, opening_records=proof["opening_records"][:-8])) == "record_length"
    assert rejected_for(dict(proof, fri_commitments=proof["fri_commitments"][:-1])) == "fold_count"
    assert rejected_for(dict(proof, fri_final_layer=proof["fri_final_layer"][:-1])) == "final_size"
    assert rejected_for(dict(proof, ood_acc=proof["ood_acc"][:-1])) == "ood_shape"


def tampered_at_a_queried_index(main, log_b, name, hit):
    """A proof whose prover changed ONE word of the layer `name` before committing it, at an index a query then asks for (the queries
    follow from the commitment, so candidates are tried in turn until one is hit)."""
    N = main.shape[1] << log_b
    for j in range(N // 2):
        def tamper(layer_name, layer, j=j):
            if layer_name == name:
                layer[j, 2] = (layer[j, 2] + np.uint64(1)) % np.uint64(P)
        proof, _ = ref.prove(main, log_b, SEED, cheat={"tamper": tamper})
        if hit(j, proof["query_indices"]):
            return proof
    raise AssertionError("no candidate index was queried")


def test_one_committed_deep_word_changed(honest):
    """Committed as changed, so every path holds: the recomputation from the opened rows rejects."""
    n, log_b, main, _, _ = honest
    assert rejected_for(tampered_at_a_queried_index(main, log_b, "deep", lambda j, q: j in q)) == "deep_value"


def test_one_committed_fold_word_changed(honest):
    n, log_b, main, _, _ = honest
    N = n << log_b
    assert rejected_for(tampered_at_a_queried_index(main, log_b, "fri1", lambda j, q: j in [i % (N // 2) for i in q])) == "fri_consistency"


def test_one_final_layer_word_changed(honest):
    n, log_b, main, proof, _ = honest
    bad = dict(proof)
    bad["fri_final_layer"] = list(proof["fri_final_layer"])
    bad["fri_final_layer"][-1] = em.add(bad["fri_final_layer"][-1], (0, 0, 1, 0))
    assert rejected_for(bad) == "final_not_constant"
    # every element changed alike: constant, but not what was committed
    bad["fri_final_layer"] = [em.add(v, (0, 0, 1, 0)) for v in proof["fri_final_layer"]]
    assert rejected_for(bad) == "final_commitment"
    # committed as changed too: the last fold says otherwise
    def tamper(name, layer):
        if name == f"fri{n.bit_length() - 1}":
            layer[:, 2] = (layer[:, 2] + np.uint64(1)) % np.uint64(P)

    tampered, _ = ref.prove(main, log_b, SEED, cheat={"tamper": tamper})
    assert rejected_for(tampered) == "final_value"


def test_first_proof_difference_names_the_component():
    main = ref.true_main(8, SEED)
    want, _ = ref.prove(main, 1, SEED)
    for cheat, head in [({"gamma_reversed": True}, "acc_commitment"), ({"weight_coordinates_transposed": True}, "quotient_commitment"),
                        ({"swap_z_gz": True}, "ood_acc"), ({"q_z_without_powers": True}, "q_z"), ({"drop_q_terms": True}, "fri_commitments[0]"),
                        ({"beta_reversed": True}, "fri_commitments[1]"), ({"rotation_rows": 1}, "opening_records of group 1")]:
        assert ref.first_proof_difference(ref.prove(main, 1, SEED, cheat=cheat)[0], want).startswith(head), cheat
