"""Steps the interpreter of constraint programs under Ext weights (air_eval_group_ext and air_ext_store, toyni_amd/csrc/prover_kernels.hpp;
include/toyni_hip.h 3k) on the CPU under AddressSanitizer + UBSan, with the host-side preparation of toyni_air_quotient_ext_device, and
checks every printed word against the numpy model of the BASE instruction set (tests/air_model.py) run four times, run e under the
base weights weights4[4 k + e] -- the definition of 3k.

N in {1, 2, 4, 8} with every blow-up in {1, 2, 4} that fits; rotation 1 with B = 2 (word loads); out_stride = N, N + 1 and N + 4; an
output base one word off a 16-byte boundary; accumulate; a null c output; a coset Z_H vanishes on (no divided constraint, an XINV at a
point of the coset); constraint number 0 emitted twice; and N = 2048 with 16, 32 and 64 registers, the three thread counts of
air_launch_shape, in the device's register-file layout.  A second run on saturated operands (every data word and every weight
coordinate p - 1).  CPU only, a stand-alone program with its own main; the shipped library contains none of tests/emu."""
import os
import subprocess
from functools import lru_cache

import numpy as np

from air_model import EMIT, XINV, P, air_launch_shape, air_model, coset_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
SAT_X = 1069547521                       # the plain value whose Montgomery form is p - 1


def build_emu_air_ext() -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_air_ext.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_air_ext_asan")
    deps = [src, os.path.join(ROOT, "tests", "emu", "contract_case.hpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-I", CSRC, "-o", out, src])
    return out


def parse_cases(stdout):
    """-> one dict per AIRX record of emu_air_ext's output (shared with tests/test_field_contracts_air_ext.py)."""
    lines = stdout.split("\n")
    assert lines[-2] == "DONE", lines[-3:]
    assert not any(l.startswith("FAIL") for l in lines), [l for l in lines if l.startswith("FAIL")][:5]
    recs = [l.split() for l in lines[:-2]]
    cases, k = [], 0
    while k < len(recs):
        assert recs[k][0] == "AIRX", recs[k][:3]
        n, log_b, shift, nmats, ninsns, nweights, nregs, stride, acc, has_c, threads, off = map(int, recs[k][1:])
        k += 1
        shapes = []
        for m in range(nmats):
            assert recs[k][0] == "MAT" and int(recs[k][1]) == m
            shapes.append(tuple(map(int, recs[k][2:])))
            k += 1
        mats = []
        for m, (width, _, _) in enumerate(shapes):
            cols = []
            for c in range(width):
                assert recs[k][:3] == ["COL", str(m), str(c)] and len(recs[k]) == n + 3
                cols.append(np.array(recs[k][3:], dtype=np.uint64))
                k += 1
            mats.append(np.stack(cols))
        assert all(recs[k + t][0] == "INSN" for t in range(ninsns))
        insns = [tuple(map(int, recs[k + t][1:])) for t in range(ninsns)]
        k += ninsns
        assert recs[k][0] == "W" and len(recs[k]) == 4 * nweights + 1
        weights4 = np.array(recs[k][1:], dtype=np.uint64).reshape(nweights, 4)
        k += 1

        def columns(tag):
            nonlocal k
            out = []
            for e in range(4):
                assert recs[k][:2] == [tag, str(e)] and len(recs[k]) == n + 2, (tag, e, recs[k][:2])
                out.append(np.array(recs[k][2:], dtype=np.uint64))
                k += 1
            return np.stack(out)

        pre_c = columns("PREC") if acc and has_c else None
        pre_q = columns("PREQ") if acc else None
        got_c = columns("C") if has_c else None
        got_q = columns("Q")
        cases.append(dict(n=n, log_b=log_b, shift=shift, mat_shapes=shapes, mats=mats, insns=insns, weights4=weights4, nregs=nregs, stride=stride, acc=acc,
                          has_c=has_c, threads=threads, off=off, pre_c=pre_c, pre_q=pre_q, got_c=got_c, got_q=got_q))
    return cases


def check_against_the_model(case):
    """Column e is the base model's output under the weights weights4[:, e], on top of what the column held when accumulating."""
    p = np.uint64(P)
    for e in range(4):
        want_c, want_q = air_model(case["insns"], case["mats"], case["n"], case["log_b"], case["shift"], [int(w) for w in case["weights4"][:, e]])
        want_c, want_q = want_c.astype(np.uint64), want_q.astype(np.uint64)
        if case["acc"]:
            want_q = (want_q + case["pre_q"][e]) % p
            if case["has_c"]:
                want_c = (want_c + case["pre_c"][e]) % p
        assert (case["got_q"][e] == want_q).all(), ("q", e, case["n"], case["log_b"], case["nregs"], case["stride"])
        if case["has_c"]:
            assert (case["got_c"][e] == want_c).all(), ("c", e, case["n"], case["log_b"], case["nregs"], case["stride"])


@lru_cache(maxsize=None)
def _run(*args):
    res = subprocess.run([build_emu_air_ext(), *args], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return res.stdout


def test_ext_interpreter_body_matches_the_base_model_per_coordinate():
    cases = parse_cases(_run())
    for case in cases:
        check_against_the_model(case)
        assert case["threads"] == air_launch_shape(case["nregs"], any(op == EMIT and b == 0 for op, _, _, b, _ in case["insns"]), case["log_b"])[0]
    seen = {(c["n"], 1 << c["log_b"]) for c in cases}
    assert {(n, b) for n in (1, 2, 4, 8) for b in (1, 2, 4) if b <= n} <= seen
    assert {(16, 256), (32, 128), (64, 64)} <= {(c["nregs"], c["threads"]) for c in cases if c["n"] == 2048}, "the three thread counts"
    for n in (1, 2, 4, 8):
        mine = [c for c in cases if c["n"] == n]
        assert any(c["stride"] == n + 1 for c in mine) and any(c["stride"] == n for c in mine)
        assert any(c["acc"] for c in mine) and any(not c["acc"] for c in mine)
        assert any(not c["has_c"] for c in mine) and any(c["off"] for c in mine)
        assert any(not any(op == EMIT and b == 0 for op, _, _, b, _ in c["insns"]) for c in mine), "no divided constraint"
        assert any(any(off for _, _, off in c["mat_shapes"]) for c in mine), "a matrix one word off"
    for c in cases:
        numbers = [imm for op, _, _, _, imm in c["insns"] if op == EMIT]
        assert len(numbers) > len(set(numbers)), "a constraint number is emitted twice"
    rot1 = [c for c in cases if c["log_b"] == 1 and any(op == 0 and a == 1 for op, _, a, _, _ in c["insns"]) and len(c["insns"]) == 8]
    assert {c["n"] for c in rot1} == {2, 4, 8, 64}, "rotation 1 with B = 2"
    on_coset = 0
    for c in cases:
        xs = set(int(v) for v in coset_points(c["n"], c["shift"]))
        on_coset += any(op == XINV and imm in xs for op, _, _, _, imm in c["insns"])
    assert on_coset >= 4
    # with out_stride = N + 1 the columns 1..3 start off a 16-byte boundary although the base pointer is on one: every coordinate
    # having matched the model above, the per-column store decision is right (UBSan aborts on a misaligned 16-byte access)
    assert any(c["stride"] % 4 and not c["off"] and c["n"] >= 4 for c in cases)


def test_ext_interpreter_on_saturated_operands():
    cases = parse_cases(_run("saturated"))
    assert len(cases) == 4 and {c["log_b"] for c in cases} == {0, 2} and {c["acc"] for c in cases} == {0, 1}
    for case in cases:
        assert all((m == P - 1).all() for m in case["mats"]) and (case["weights4"] == P - 1).all()
        assert (1, 1, 0, 0, SAT_X) in case["insns"]
        if case["acc"]:
            assert (case["pre_q"] == P - 1).all() and (case["pre_c"] == P - 1).all()
        check_against_the_model(case)
        assert case["got_q"].any() and case["got_c"].any()
