"""The stream-ordered compiled prover (toyni_amd/csrc/host/fib_prover_dt.hpp, toyni::fib::StreamProver) run as the program
tests/cpp/fib_prove_dt.cpp: the whole Fibonacci proof as one chain of enqueues on the device transcript and ONE synchronisation.
Its proof is, byte for byte, the reference prover's under the key the file names (tests/harness/ref_prover.py, the oracle alone),
is accepted by the CPU restatement of src/verifier.rs, and its forgery is refused; the counts it reports for a warm proof show one
synchronisation, one device-to-host copy and no pinned root write; several proofs in flight from one thread are the same proofs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu


def _exe():
    import __graft_entry__ as entry
    entry.build_hip()
    return entry.build_fib_prove_dt()


def _run(args, timeout=600):
    res = subprocess.run([_exe()] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert lines, res.stdout[-2000:] + res.stderr[-2000:]
    return res.returncode, json.loads(lines[-1])


@pytest.mark.parametrize("n,lde,folds,final", [(8, 256, 8, 1), (16, 512, 8, 2), (64, 2048, 8, 8), (128, 4096, 9, 8), (256, 8192, 9, 16),
                                               (1024, 1 << 15, 11, 16), (1 << 14, 1 << 19, 15, 16), (1 << 16, 1 << 21, 17, 16)])
def test_stream_proof_is_the_reference_proof_and_synchronises_once(tmp_path, n, lde, folds, final):
    from harness import fib_prover, fib_verifier, ref_prover
    from test_fib_prover_cpp import _load_proof
    path = tmp_path / "proof.json"
    rc, out = _run([n, 5, 1, path])
    assert rc == 0 and out["gpu"], out
    assert (out["trace_len"], out["lde_size"], out["folds"], out["final_layer_size"], out["in_flight"]) == (n, lde, folds, final, 1)
    # the counted traffic of the warm proof: the trace and the 32 bytes of the initial transcript up, the tail down, one synchronisation
    pcie = out["pcie"]
    assert (pcie["synchronisations"], pcie["d2h_copies"], pcie["pinned_root_writes"], pcie["h2d_copies"]) == (1, 1, 0, 2), pcie
    assert pcie["h2d_bytes"] == 4 * n + 32
    raw = _load_proof(path)
    proof = fib_prover.expand_proof(raw)
    why = []
    assert fib_verifier.verify(proof, why), why
    assert len(proof["query_proofs"]) == 44 and len(proof["fri_commitments"]) == folds + 1
    want, _ = ref_prover.prove(fib_prover.fibonacci_trace(n), ref_prover.ChaChaRandomness(bytes.fromhex(raw["key"])))
    diff = ref_prover.first_proof_difference(raw, want)
    assert not diff, diff
    bad = dict(proof, t_z=(proof["t_z"] + 1) % fib_verifier.P)
    why = []
    assert not fib_verifier.verify(bad, why) and why == ["ood"]


def test_stream_prover_refuses_a_non_fibonacci_trace():
    rc, out = _run([64, 3, 1, "--corrupt-row", 10])
    assert rc == 1 and out["error"] == "Constraint check at z failed"        # src/fibonacci.rs:430-442


def test_three_proofs_in_flight_are_the_proof_of_one(tmp_path):
    one, three = tmp_path / "one.json", tmp_path / "three.json"
    rc, out1 = _run([256, 7, 2, one])
    assert rc == 0 and out1["in_flight"] == 1
    rc, out3 = _run([256, 7, 2, three, "--in-flight", 3])
    assert rc == 0 and out3["in_flight"] == 3 and len(out3["ms_per_proof"]) == 2
    pcie = out3["pcie"]
    assert (pcie["synchronisations"], pcie["d2h_copies"], pcie["pinned_root_writes"]) == (1, 1, 0), pcie
    want = json.load(open(one))
    for path in (three, str(three) + ".1", str(three) + ".2"):
        assert json.load(open(path)) == want, path
