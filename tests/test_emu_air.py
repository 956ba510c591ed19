"""Steps the interpreter of constraint programs (air_eval_group and its helpers, toyni_amd/csrc/prover_kernels.hpp) on the CPU under
AddressSanitizer + UBSan, with the host-side preparation of toyni_air_quotient_device, and checks every printed word against the
numpy model of the instruction set (tests/air_model.py):
    c_i = sum_{EMIT k, b = 0} w_k value_k(i),   q_i = c_i / (x_i^n - 1) + sum_{EMIT k, b = 1} w_k value_k(i)
N in {2, 4, 8, 64}, every blow-up below N; the Fibonacci program (aligned and 4 bytes off, 1 / Z_H per class and per thread); random
programs over 1, 7 and all 64 registers and 1, 2 and 4 matrices with padded strides, misaligned matrices, rotations that wrap, and an
XINV at a point of the coset.  CPU only; the shipped library contains none of tests/emu."""
import os
import subprocess

import numpy as np

from air_model import EMIT, XINV, P, air_launch_shape, air_model, coset_points, fib_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")


def build_emu_air() -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_air.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_air_asan")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-I", CSRC, "-o", out, src])
    return out


def _records():
    res = subprocess.run([build_emu_air()], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.split("\n")
    assert lines[-2] == "DONE"
    return [l.split() for l in lines[:-2]]


def test_interpreter_body_matches_the_model_on_cpu():
    recs = _records()
    k = 0
    seen_n, seen_regs, seen_mats, fib_cases, zero_inverse, wrapped, padded, offset = set(), set(), set(), 0, 0, 0, 0, 0
    shapes_seen = [tuple(map(int, r[1:])) for r in recs if r[0] == "SHAPE"]
    recs = [r for r in recs if r[0] != "SHAPE"]
    assert len(shapes_seen) == 64 * 2 * 5
    for nregs, divides, log_b, threads, lds, zh in shapes_seen:       # the launcher's sizing rule, restated
        want_threads, want_lds, want_zh = air_launch_shape(nregs, divides, log_b)            # tests/air_model.py
        assert (threads, zh, lds) == (want_threads, want_zh, want_lds), (nregs, divides, log_b)
        assert 0 < lds <= 65536 and threads % 64 == 0
    assert (16, 1, 5, 256, 65536, 0) in shapes_seen and (15, 1, 5, 256, 61568, 1) in shapes_seen and (64, 1, 0, 64, 65536, 0) in shapes_seen
    while k < len(recs):
        r = recs[k]
        assert r[0] == "AIR"
        n, log_b, shift, nmats, ninsns, nweights, nregs = map(int, r[1:])
        k += 1
        shapes = []
        for m in range(nmats):
            assert recs[k][0] == "MAT" and int(recs[k][1]) == m
            shapes.append(tuple(map(int, recs[k][2:])))
            k += 1
        mats = []
        for m, (width, stride, off) in enumerate(shapes):
            cols = []
            for c in range(width):
                assert recs[k][:3] == ["COL", str(m), str(c)] and len(recs[k]) == n + 3
                cols.append(np.array(recs[k][3:], dtype=np.uint64))
                k += 1
            mats.append(np.stack(cols))
            padded += stride > n
            offset += off > 0
        insns = [tuple(map(int, recs[k + t][1:])) for t in range(ninsns)]
        assert all(recs[k + t][0] == "INSN" for t in range(ninsns))
        k += ninsns
        weights = list(map(int, recs[k][1:]))
        got_c, got_q = np.array(recs[k + 1][1:], dtype=np.uint32), np.array(recs[k + 2][1:], dtype=np.uint32)
        assert recs[k][0] == "W" and len(weights) == nweights and recs[k + 1][0] == "C" and recs[k + 2][0] == "Q"
        k += 3
        want_c, want_q = air_model(insns, mats, n, log_b, shift, weights)
        assert (got_c == want_c).all() and (got_q == want_q).all(), (n, log_b, nregs, ninsns)
        seen_n.add(n), seen_regs.add(nregs), seen_mats.add(nmats)
        fib_cases += insns == fib_program(n >> log_b)
        xs = set(int(v) for v in coset_points(n, shift))
        zero_inverse += any(op == XINV and imm in xs for op, _, _, _, imm in insns)
        wrapped += any(op == 0 and a and (n - 1 + a * (1 << log_b)) >= n for op, _, a, _, _ in insns)
        assert insns[-1][0] == EMIT
    assert seen_n == {2, 4, 8, 64} and {1, 7, 64} <= seen_regs and seen_mats == {1, 2, 4}
    assert fib_cases >= 20 and zero_inverse >= 5 and wrapped >= 20 and padded >= 10 and offset >= 10
