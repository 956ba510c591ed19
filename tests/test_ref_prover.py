"""The reference prover (tests/harness/ref_prover.py) on the CPU.  The GPU tests hold both provers' proofs to it byte for byte, so it
is checked here first: its ChaCha20 against RFC 8439 and against the host chacha20_block of toyni_amd/csrc/prover_kernels.hpp, its
proofs against the verifier restatement, and what a byte comparison sees that the verifier cannot (a committed but unopened leaf)."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from harness import fib_verifier, ref_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fibonacci_trace(n):
    out, a, b = [], 1, 1
    for _ in range(n):
        out.append(a)
        a, b = b, (a + b) % fib_verifier.P
    return out


def harness_randomness(n, seed):
    rng = np.random.default_rng(seed)
    return ref_prover.HarnessRandomness(rng.integers(0, 256, (ref_prover.salt_leaves(n), 16), dtype=np.uint8),
                                        rng.integers(0, fib_verifier.P, fib_verifier.MASK_DEGREE))


def test_chacha20_rfc8439_block_function_vector():
    # RFC 8439 section 2.3.2: key 00 01 .. 1f, nonce 00 00 00 09 00 00 00 4a 00 00 00 00 (non-zero first word), block counter 1
    got = ref_prover.chacha20_blocks(bytes(range(32)), (0x09000000, 0x4A000000, 0), 1, 1).tobytes().hex()
    assert got == ("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                   "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")


def test_chacha20_rfc8439_appendix_a1_vectors_1_and_2():
    # key 0, nonce 0, block counters 0 and 1
    got = ref_prover.chacha20_keystream(bytes(32), (0, 0, 0), 128).tobytes().hex()
    assert got == ("76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7"
                   "da41597c5157488d7724e03fb8d84a376a43b8f41518a11cc387b669b2ee6586"
                   "9f07e7be5551387a98ba977c732d080dcb0f29a048e3656912c6533e32ee7aed"
                   "29b721769ce64e43d57133b074d839d531ed1f28510afb45ace10a1f4b794d6f")


def test_chacha20_matches_the_host_block_function_of_the_prover(tmp_path):
    """The prover's own chacha20_block (compiled for the host): the mask's nonce (0, 1, 0) at counters 0 .. 17, the salts' nonce
    (0, 0, 0) at counters past 2^16, where the numpy keystream crosses from one sweep of blocks to the next."""
    src = tmp_path / "c.cpp"
    src.write_text('''#include <cstdio>
#include <cstring>
#include "prover_kernels.hpp"
static void block(const uint32_t* kw, uint32_t ctr, const uint32_t* nonce) {
    uint32_t o[16];
    toyni::chacha20_block(kw, ctr, nonce, o);
    unsigned char b[64];
    std::memcpy(b, o, 64);
    for (int i = 0; i < 64; ++i) std::printf("%02x", b[i]);
    std::printf("\\n");
}
int main() {
    uint8_t key[32];
    for (int i = 0; i < 32; ++i) key[i] = (uint8_t)(i * 37 + 11);
    uint32_t kw[8];
    std::memcpy(kw, key, 32);
    const uint32_t mask_nonce[3] = {0u, 1u, 0u}, salt_nonce[3] = {0u, 0u, 0u};
    for (uint32_t c = 0; c < 18; ++c) block(kw, c, mask_nonce);
    const uint32_t past[4] = {65535u, 65536u, 65537u, 70001u};
    for (uint32_t c : past) block(kw, c, salt_nonce);
    return 0;
}''')
    exe = tmp_path / "c"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "toyni_amd", "csrc"),
                           "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    key = bytes((i * 37 + 11) & 255 for i in range(32))
    mask_ks = ref_prover.chacha20_blocks(key, (0, 1, 0), 0, 18).reshape(18, 64)
    assert [r.tobytes().hex() for r in mask_ks] == out[:18]
    salt_ks = ref_prover.chacha20_blocks(key, (0, 0, 0), 0, 70002).reshape(-1, 64)
    assert [salt_ks[c].tobytes().hex() for c in (65535, 65536, 65537, 70001)] == out[18:]
    # and the mask values the compiled prover derives from that keystream: 8 bytes little-endian per value, mod p
    mask = ref_prover.ChaChaRandomness(key).mask(fib_verifier.MASK_DEGREE)
    ks = bytes.fromhex("".join(out[:18]))
    assert mask == [int.from_bytes(ks[8 * i:8 * i + 8], "little") % fib_verifier.P for i in range(fib_verifier.MASK_DEGREE)]


def test_merkle_get_proofs_matches_the_single_index_form():
    for n in (1, 2, 13, 1000):
        levels = oracle.merkle_commit_values(oracle.splitmix(n, n), np.random.default_rng(n).integers(0, 256, (n, 16), dtype=np.uint8))
        idx = sorted({0, n - 1, n // 2, (7 * n) // 11})
        assert oracle.merkle_get_proofs(levels, idx + [n]) == [oracle.merkle_get_proof(levels, i) for i in idx] + [None]


@pytest.mark.parametrize("n,depth,pad", [(1, 0, 0), (2, 1, 7), (13, 4, 4), (1000, 10, 6), (1 << 16, 16, 0), (1 << 21, 21, 3)])
def test_opening_record_layout_and_zero_padding(n, depth, pad):
    assert ref_prover.merkle_record_bytes(n) == 33 * depth + 24 + pad
    if n > 1 << 12:
        return
    vals = oracle.splitmix(n, 5 + n)
    salts = np.random.default_rng(n).integers(0, 256, (n, 16), dtype=np.uint8)
    levels = oracle.merkle_commit_values(vals, salts)
    idx = [0, n - 1, n // 2]
    ops, raw = ref_prover.serialize_openings(levels, vals, salts, idx)
    rec = raw.reshape(len(idx), -1)
    for o, r in zip(ops, rec):
        assert fib_verifier.verify_opening(o, levels[-1][0].tobytes())
        assert r[32 * depth:32 * depth + 16].tobytes() == o["salt"]
        assert int.from_bytes(r[32 * depth + 16:32 * depth + 24].tobytes(), "little") == o["value"]
        assert [bool(b) for b in r[32 * depth + 24:33 * depth + 24]] == o["position"]
        assert not r[33 * depth + 24:].any()


@pytest.mark.parametrize("n", [8, 16, 64, 256])
@pytest.mark.parametrize("form", ["harness", "chacha"])
def test_reference_proofs_are_accepted_and_tampering_is_not(n, form):
    rnd = harness_randomness(n, 100 + n) if form == "harness" else ref_prover.ChaChaRandomness(bytes(range(7, 39)))
    proof, comp = ref_prover.prove(fibonacci_trace(n), rnd)
    why = []
    assert fib_verifier.verify(proof, why), why
    final_size, sizes = ref_prover.fri_layer_sizes(n)
    assert len(proof["fri_commitments"]) == len(sizes) + 1 and len(proof["fri_final_layer"]) == final_size
    assert len(comp["betas"]) == len(sizes) and [len(l) for l in comp["fri_layers"]] == sizes
    bad = dict(proof, t_z=(proof["t_z"] + 1) % fib_verifier.P)
    why = []
    assert not fib_verifier.verify(bad, why) and why == ["ood"]
    # the two forms are interchangeable sources: the same pool handed over as harness randomness gives the same proof
    if form == "chacha":
        again, _ = ref_prover.prove(fibonacci_trace(n), ref_prover.HarnessRandomness(rnd.salts(ref_prover.salt_leaves(n)),
                                                                                       rnd.mask(fib_verifier.MASK_DEGREE)))
        assert ref_prover.first_proof_difference(again, proof) == ""


def test_a_committed_but_unopened_leaf_passes_the_verifier_and_fails_the_byte_comparison():
    """The blind spot the byte-exact comparisons close.  A Merkle proof checks out against a root built from the same wrong
    digests, so a wrong salt or digest at a leaf no query opens is accepted by the verifier; a comparison with the reference's
    proof names the commitment.  The quotient tree opens only q < N/2, so leaf N - 1 is never opened; leaf 30 of the first FRI
    layer is not opened under this seed (checked below)."""
    n = 8
    rnd = harness_randomness(n, 2024)
    base, _ = ref_prover.prove(fibonacci_trace(n), rnd)
    N = base["lde_size"]

    def bad_salt(name, salts, leaves):
        if name == "quotient":
            salts[N - 1, 0] ^= 1

    def bad_digest(name, salts, leaves):
        if name == "fri1":
            leaves[30, 5] ^= 0x40

    for hook, group, leaf, where in [(bad_salt, 1, N - 1, "quotient_commitment"), (bad_digest, 3, 30, "fri_commitments[1]")]:
        alt, _ = ref_prover.prove(fibonacci_trace(n), rnd, tree_hook=hook)
        assert leaf not in alt["opening_groups"][group][2], "the altered leaf was opened: pick another"
        why = []
        assert fib_verifier.verify(alt, why), why
        assert ref_prover.first_proof_difference(alt, base).startswith(where + ":")
    assert ref_prover.first_proof_difference(base, ref_prover.prove(fibonacci_trace(n), rnd)[0]) == ""
