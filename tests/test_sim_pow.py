"""The three kernels of a grind chain (include/toyni_hip.h 3n) -- pow_arm_kernel, pow_search_kernel, pow_finish_kernel themselves, every
GPU thread a fiber -- run on the CPU through tests/sim/hip_sim.hpp (unchanged) by their own driver, tests/sim/sim_pow.cpp.

The search waits for nothing, so ANY order of its threads is a legal execution, and the answer must be the smallest accepted nonce
under every one of them.  The driver runs four grid shapes (1 x 64, 3 x 64, 4 x 256, 2 x 192) under the header's eight wave / lane
schedules, each with the workgroups ascending and descending -- descending waves and lanes with descending workgroups runs the highest
thread of the grid first, whose first hit lies far above the minimum.  Cases: bits 1, 6 and 10, states on both sides of the
one-block | two-block edge and with the nonce across three message words, the start 2^32 - 100 (at 8 and 12 bits, whose answers lie
beyond 2^32), other nonzero starts, a window without a hit and a transcript that cannot take a nonce.  Every expected value comes from tests/pow_model.py.

Teeth: the same driver built with the stop rule of pow_kernels.hpp replaced by "stop as soon as anything has been found" must return,
under some order, a nonce that is accepted but NOT the minimum.  CPU only, stand-alone programs, no sanitizer."""
import os
import re
import subprocess
from functools import lru_cache

import __graft_entry__ as entry
import pow_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
SHAPES = ["1x64", "3x64", "4x256", "2x192"]
START = (1 << 32) - 100
# (state, bits, start, log_tries)
CASES = [(pm.START_STATE, 1, 0, 12), (pm.START_STATE, 6, 0, 12), (pm.START_STATE, 10, 0, 14),
         (pm.pattern(47, 47), 6, 0, 12), (pm.pattern(48, 48), 10, 0, 14), (pm.pattern(63, 63), 6, 0, 12),
         (pm.pattern(64, 3), 8, START, 12), (pm.pattern(64, 3), 12, START, 12), (pm.pattern(1000, 1000), 6, 17, 12),
         (pm.pattern(0, 0), 10, 5, 14),
         (pm.pattern(64, 9), 24, 0, 10),                   # no hit in the window
         (pm.pattern(1001, 5), 1, 0, 10)]                  # cannot take the 8 bytes


def build_sim_pow(wrong_rule: bool = False) -> str:
    sim = os.path.join(ROOT, "tests", "sim")
    src, out = os.path.join(sim, "sim_pow.cpp"), os.path.join(sim, "build", "sim_pow" + ("_wrong_rule" if wrong_rule else ""))
    deps = [src, os.path.join(sim, "hip_sim.hpp"), os.path.join(ROOT, "include", "toyni_hip.h")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include")] + (["-DSIM_POW_WRONG_RULE"] if wrong_rule else []) + ["-o", out, src])
    return out


@lru_cache(maxsize=None)
def _run(wrong_rule: bool):
    text = "".join(f"{s.hex() or '-'} {bits} {start} {lt}\n" for s, bits, start, lt in CASES)
    res = subprocess.run([build_sim_pow(wrong_rule)], input=text, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("DONE"), res.stdout[-2000:] + res.stderr[-3000:]
    assert "LAUNCH-FAILED" not in res.stdout and re.search(r"hard failures=0$", res.stdout, re.M), res.stdout[-2000:]
    rows = []
    for m in re.finditer(r"^RESULT (\d+) (\S+) (\S+) (\S+) nonce=(\d+) status=(\d+) len=(\d+) state=(\S*)$", res.stdout, re.M):
        rows.append((int(m.group(1)), m.group(2), m.group(3), m.group(4), int(m.group(5)), int(m.group(6)), int(m.group(7)), bytes.fromhex(m.group(8))))
    assert len(rows) == len(CASES) * len(SHAPES) * 8 * 2
    return rows, res.stdout


@lru_cache(maxsize=None)
def _expected():
    out = []
    for s, bits, start, lt in CASES:
        m = pm.Transcript(s)
        out.append((m.grind(bits, start, 1 << lt), m))
    return out


def test_every_order_of_every_grid_leaves_the_models_minimum():
    rows, text = _run(False)
    want = _expected()
    assert [n for n, _ in want][6:8] == [START + 232, START + 3345]           # beyond 2^32: a nonce kept in 32 bits fails here
    assert sum(1 for _, m in want if m.status) == 2 and sum(1 for n, m in want if n > 64) >= 6
    seen = set()
    for case, shape, sched, blocks, nonce, status, length, state in rows:
        exp, m = want[case]
        assert (nonce, status, length, state) == (exp, m.status, len(m.state), m.state), (case, shape, sched, blocks, nonce, exp)
        seen.add((shape, sched, blocks))
    assert len(seen) == len(SHAPES) * 16 and {s for s, _, _ in seen} == set(SHAPES)
    assert ("4x256", "waves-desc/lanes-desc", "blocks-desc") in seen          # the highest workgroup and thread first
    # the search kernel's one barrier (behind the shared midstate) was reached, and is the only synchronisation site of the chain
    sites = re.findall(r"^SITE (\w+):\d+ (\S+) arrivals=(\d+)$", text, re.M)
    assert [k for k, _, _ in sites] == ["pow_search_kernel"] and sites[0][1].startswith("syncthreads@toyni_hip.hip"), sites


def test_stop_when_anything_is_found_returns_a_nonce_that_is_not_the_minimum():
    rows, _ = _run(True)
    want = _expected()
    worse = 0
    for case, shape, sched, blocks, nonce, status, length, state in rows:
        exp, m = want[case]
        s, bits, start, lt = CASES[case]
        if m.status:
            assert (nonce, status, state) == (0, m.status, m.state)           # the refusals do not depend on the rule
            continue
        assert status == 0 and start <= nonce < start + (1 << lt) and pm.accept(s, nonce, bits) and state == s + pm.le64(nonce)
        assert nonce >= exp
        worse += nonce > exp
    assert worse > 0, "the wrong stop rule went unnoticed under every order: the sim test cannot tell the rules apart"
