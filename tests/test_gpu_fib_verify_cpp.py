"""The device verifier's C++ caller (toyni_amd/csrc/host/fib_verifier.hpp, toyni::fib::BatchVerifier) as the program
tests/cpp/fib_verify_batch.cpp: proofs of the batched device prover (BatchStreamProver) are packed, uploaded once, verified in one
chain of launches (include/toyni_hip.h 3t), and the verdicts come back in one download behind one synchronisation.  Every proof the
program verified is also judged by the restated reference verifier (tests/harness/fib_verifier.py)."""
import json
import os
import subprocess

import pytest

from test_fib_prover_cpp import _load_proof

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exe():
    import __graft_entry__ as entry
    entry.build_hip()
    return entry.build_fib_verify_batch()


def _run(args, timeout=300):
    res = subprocess.run([_exe()] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert lines, res.stdout[-2000:] + res.stderr[-2000:]
    return res.returncode, json.loads(lines[-1])


def test_cpp_verifier_builds_and_self_skips_without_gpu():
    import toyni_amd
    if toyni_amd.gpu_available():
        return                                            # the gpu-marked tests below run the program
    rc, out = _run([64, 3, 1, 3])
    assert rc == 0 and out == {"gpu": False}              # no device, no verdict, no CPU fallback


@pytest.mark.gpu
def test_three_proofs_of_the_device_prover_are_accepted_with_one_upload_one_download_one_synchronisation():
    rc, out = _run([64, 3, 1, 3])
    assert rc == 0 and out["verdicts"] == [0, 0, 0] and out["names"] == ["accept"] * 3, out
    t = out["traffic"]
    assert (t["synchronisations"], t["d2h_copies"], t["h2d_copies"]) == (1, 1, 1) and t["d2h_bytes"] == 4 * 3 and t["h2d_bytes"] == 3 * out["image_bytes"], out


@pytest.mark.gpu
def test_a_tampered_proof_fails_alone():
    rc, out = _run([64, 3, 1, 3, "--tamper", 1, "t_z"])
    assert rc == 0 and out["verdicts"] == [0, 2, 0] and out["names"] == ["accept", "ood", "accept"], out
    rc, out = _run([64, 3, 1, 3, "--tamper", 1, "path"])
    assert rc == 0 and out["verdicts"] == [0, 1 << 8 | 6, 0] and out["names"][1] == "trace_merkle", out


@pytest.mark.gpu
def test_five_proofs_of_1024_rows_agree_with_the_restated_reference_verifier(tmp_path):
    from harness import fib_prover, fib_verifier
    path = tmp_path / "proof.json"
    rc, out = _run([1024, 11, 1, 5, str(path), "--tamper", 3, "index"])
    assert rc == 0 and out["folds"] == 11 and out["final_layer_size"] == 16, out
    assert out["verdicts"] == [0, 0, 0, 4 << 8 | 5, 0] and out["names"][3] == "query_index", out
    for b in range(5):
        why = []
        ok = fib_verifier.verify(fib_prover.expand_proof(_load_proof(f"{path}.{b}")), why)
        assert (ok, why) == ((True, []) if b != 3 else (False, ["query_index"])), (b, why)
