"""Steps the per-element body of the Ext fold-and-commit round (fold_ext_commit_one, toyni_amd/csrc/prover_kernels.hpp: the text
fri_fold_ext_commit_kernel runs per thread; include/toyni_hip.h 3j) on the CPU under AddressSanitizer + UBSan.  Every folded element
is compared with the oracle's fri_fold_ext, every digest with hashlib over the row leaf tests/rows_common.py builds:
sha256(00 || [salt (16)] || Ext::to_bytes (32)).  Salted and unsalted; 0, 1 and p - 1 in every coordinate of a, b and beta; beta
embedded from the base field; x in {1, p - 1, 7, random}.  CPU only; the shipped library contains none of tests/emu."""
import os
import subprocess

import numpy as np

import oracle
import rows_common as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = 2013265921


def build_emu_fold_ext_commit() -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_fold_ext_commit.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_fold_ext_commit_asan")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-I", CSRC, "-o", out, src])
    return out


def test_fold_ext_commit_body_matches_the_oracle_and_hashlib_on_cpu():
    res = subprocess.run([build_emu_fold_ext_commit()], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.split("\n")
    assert lines[-2] == "DONE"
    seen_salted = {0: 0, 1: 0}
    coords = {"a": [set() for _ in range(4)], "b": [set() for _ in range(4)], "beta": [set() for _ in range(4)]}
    base_betas, xs_seen = set(), set()
    for line in lines[:-2]:
        f = line.split()
        assert len(f) == 20, line
        salted = int(f[0])
        a, b = [int(v) for v in f[1:5]], [int(v) for v in f[5:9]]
        x, beta = int(f[9]), [int(v) for v in f[10:14]]
        salt, folded, digest_hex = bytes.fromhex(f[14]), [int(v) for v in f[15:19]], f[19]
        assert all(0 <= v < P for v in a + b + beta + folded) and 0 < x < P and len(salt) == 16
        # the reference's fold of the pair (a, b) = (f(x), f(-x)) at the point x
        want = oracle.fri_fold_ext(np.array([a, b], dtype=np.uint64), np.array([x], dtype=np.uint64), np.array(beta, dtype=np.uint64))
        assert folded == [int(v) for v in want[0]], line
        leaf = rc.leaves_of(np.array([folded], dtype=np.uint64), np.frombuffer(salt, dtype=np.uint8).reshape(1, 16) if salted else None)[0]
        assert len(leaf) == 32 + 16 * salted
        assert rc.hash_leaf(leaf).hex() == digest_hex, line
        seen_salted[salted] += 1
        for k in range(4):
            coords["a"][k].add(a[k]), coords["b"][k].add(b[k]), coords["beta"][k].add(beta[k])
        if not any(beta[1:]):
            base_betas.add(beta[0])
        xs_seen.add(x)
    assert seen_salted[0] == seen_salted[1] and seen_salted[0] >= 48           # "a few dozen" cases, each in both forms
    for name, per_coord in coords.items():
        for k, s in enumerate(per_coord):
            assert {0, 1, P - 1} <= s and len(s) > 10, (name, k)
    assert {0, 1, P - 1} <= base_betas and len(base_betas) >= 5
    assert {1, P - 1, 7} <= xs_seen and len(xs_seen) > 10
