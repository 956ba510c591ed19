"""The batched stream-ordered prover (toyni_amd/csrc/host/fib_prover_batch.hpp, toyni::fib::BatchStreamProver) run as the program
tests/cpp/fib_prove_batch.cpp: `batch` Fibonacci proofs of one trace length as ONE chain of launches (include/toyni_hip.h 3r, 3s), one
upload phase, one download, one synchronisation.  Every proof is, byte for byte, the reference prover's for its own trace under its
own key (tests/harness/ref_prover.py, the oracle alone), is accepted by the CPU restatement of src/verifier.rs, and its forgery is
refused; batch = 1 writes fib_prove_dt's proof file; the counted traffic of a warm call does not depend on the batch; a proof whose
trace breaks the AIR fails alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu

P = 2013265921


def _exe(dt=False):
    import __graft_entry__ as entry
    entry.build_hip()
    return entry.build_fib_prove_dt() if dt else entry.build_fib_prove_batch()


def _run(args, timeout=600, dt=False):
    res = subprocess.run([_exe(dt)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert lines, res.stdout[-2000:] + res.stderr[-2000:]
    return res.returncode, json.loads(lines[-1])


def trace_of(n, b):
    """the Fibonacci column started at (1 + b, 1 + b)"""
    out, x, y = np.empty(n, dtype=np.uint64), 1 + b, 1 + b
    for i in range(n):
        out[i] = x
        x, y = y, (x + y) % P
    return out


def check_proof(path, n, b, folds):
    from harness import fib_prover, fib_verifier, ref_prover
    from test_fib_prover_cpp import _load_proof
    raw = _load_proof(path)
    proof = fib_prover.expand_proof(raw)
    why = []
    assert fib_verifier.verify(proof, why), (b, why)
    assert len(proof["query_proofs"]) == 44 and len(proof["fri_commitments"]) == folds + 1
    want, _ = ref_prover.prove(trace_of(n, b), ref_prover.ChaChaRandomness(bytes.fromhex(raw["key"])))
    diff = ref_prover.first_proof_difference(raw, want)
    assert not diff, (b, diff)
    bad = dict(proof, t_z=(proof["t_z"] + 1) % fib_verifier.P)
    why = []
    assert not fib_verifier.verify(bad, why) and why == ["ood"], b
    return raw


@pytest.mark.parametrize("n,batch,lde,folds,final", [(8, 3, 256, 8, 1), (16, 3, 512, 8, 2), (64, 3, 2048, 8, 8), (256, 3, 8192, 9, 16),
                                                     (1024, 5, 1 << 15, 11, 16)])
def test_every_proof_of_a_batch_is_the_reference_proof_of_its_trace_under_its_key(tmp_path, n, batch, lde, folds, final):
    path = tmp_path / "proof.json"
    rc, out = _run([n, 5, 1, batch, path])
    assert rc == 0 and out["gpu"], out
    assert (out["trace_len"], out["lde_size"], out["folds"], out["final_layer_size"], out["batch"]) == (n, lde, folds, final, batch)
    assert out["errors"] == [""] * batch
    pcie = out["pcie"]
    assert (pcie["synchronisations"], pcie["d2h_copies"], pcie["pinned_root_writes"], pcie["h2d_copies"]) == (1, 1, 0, 3), pcie
    assert pcie["h2d_bytes"] == batch * (4 * n + 32 + 32)
    keys = set()
    for b in range(batch):
        raw = check_proof(str(path) + "." + str(b), n, b, folds)
        keys.add(raw["key"])
    assert len(keys) == batch                                                   # seed + b: every proof has its own key
    assert json.load(open(path)) == json.load(open(str(path) + ".0"))


def test_a_batch_of_one_writes_the_stream_provers_proof_file(tmp_path):
    one, dt = tmp_path / "batch.json", tmp_path / "dt.json"
    rc, out = _run([256, 7, 2, 1, one])
    assert rc == 0 and out["batch"] == 1 and out["errors"] == [""] and len(out["ms_per_proof"]) == 2
    rc, out_dt = _run([256, 7, 2, dt], dt=True)
    assert rc == 0
    assert json.load(open(one)) == json.load(open(dt))
    assert out["proof_bytes"] == out_dt["proof_bytes"]


def test_the_counted_traffic_does_not_depend_on_the_batch():
    counts = {}
    for batch in (1, 5):
        rc, out = _run([64, 3, 1, batch])
        assert rc == 0 and out["errors"] == [""] * batch
        pcie = out["pcie"]
        counts[batch] = (pcie["synchronisations"], pcie["d2h_copies"], pcie["h2d_copies"], pcie["pinned_root_writes"])
        assert pcie["h2d_bytes"] == batch * (4 * 64 + 64)
    assert counts[1] == counts[5] == (1, 1, 3, 0)


def test_a_proof_whose_trace_breaks_the_air_fails_alone(tmp_path):
    path = tmp_path / "proof.json"
    rc, out = _run([64, 3, 1, 3, path, "--corrupt-proof", 1, "--corrupt-row", 10])
    assert rc == 0 and out["errors"] == ["", "Constraint check at z failed", ""], out     # src/fibonacci.rs:430-442
    assert not os.path.exists(str(path) + ".1")
    for b in (0, 2):
        check_proof(str(path) + "." + str(b), 64, b, 8)
