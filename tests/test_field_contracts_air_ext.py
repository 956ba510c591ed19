"""The operand domains of the lazy field arithmetic (toyni_amd/csrc/bb_field.hpp) in the AIR quotient under Ext
weights (include/toyni_hip.h 3k): the two CPU programs that run its text -- tests/emu/emu_air_ext.cpp (the body, plain and saturated
cases) and tests/sim/sim_air_ext.cpp (the two __global__ functions) -- rebuilt with tests/emu/field_contracts.hpp in front, as
tests/test_field_contracts.py rebuilds the others; its helpers are used by import.

An EMIT multiplies a Montgomery value by the four plain coordinates of its weight (mont_mul: canonical factors) and adds into
canonical accumulators (bb_add); the closing step is a mont_mul with 1 / Z_H and a bb_add.  Zero violations, with every weight
coordinate and data word at p - 1 as well, and the primitives the body is made of must have been reached.

CPU only, stand-alone programs, no sanitizer; built into the existing build/ folders with a _contracts suffix."""
import os
import subprocess
from functools import lru_cache

import __graft_entry__ as entry
import test_emu_air_ext
import test_sim_air_ext
from test_field_contracts import CSRC, EMU, HEADER, PRIMITIVES, ROOT, SIM, _stale, _sum_contracts

REACH = {"bb_add", "bb_sub", "bb_reduce_2p", "mont_mul_lazy", "mont_mul"}


@lru_cache(maxsize=None)
def build_contracts(program):
    sim = program.startswith("sim_")
    folder = SIM if sim else EMU
    src, out = os.path.join(folder, program + ".cpp"), os.path.join(folder, "build", program + "_contracts")
    deps = [src, HEADER, os.path.join(EMU, "contract_case.hpp"), os.path.join(SIM, "hip_sim.hpp"), os.path.join(ROOT, "include", "toyni_hip.h")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))]
    if _stale(out, deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        if sim:   # hip_sim.hpp first: it defines the host forms of the synchronisation macros, which bb_field.hpp keeps when it finds them
            cmd = [entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable", "-I", CSRC,
                   "-I", os.path.join(ROOT, "include"), "-include", os.path.join(SIM, "hip_sim.hpp"), "-include", HEADER, "-o", out, src]
        else:
            cmd = ["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-include", HEADER, "-o", out, src]
        subprocess.check_call(cmd)
    return out


def _run(program, *args):
    res = subprocess.run([build_contracts(program), *args], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, program + ":\n" + res.stdout[-2000:] + res.stderr[-3000:]
    assert "CONTRACT" not in res.stdout, "the contract lines belong on stderr"
    return res.stdout, res.stderr


def _judge(program, errs):
    total = _sum_contracts(errs)
    assert sorted(total) == sorted(PRIMITIVES)
    bad = ["%s: %d violations in %d calls, %s" % (p, v, c, rest) for p, (c, v, rest) in total.items() if v]
    assert not bad, program + " left an operand domain:\n" + "\n".join(bad)
    reached = {p for p, (c, _, _) in total.items() if c}
    assert REACH <= reached, "%s never called %s" % (program, sorted(REACH - reached))
    return total


def test_the_ext_body_keeps_every_operand_domain():
    out, err = _run("emu_air_ext")
    cases = test_emu_air_ext.parse_cases(out)                       # the contract build prints what the sanitized build prints ...
    for case in cases:
        test_emu_air_ext.check_against_the_model(case)              # ... and it is still the model's
    total = _judge("emu_air_ext", [err])
    emits = sum(sum(1 for op, *_ in c["insns"] if op == test_emu_air_ext.EMIT) * c["n"] for c in cases)
    assert total["mont_mul"][0] >= 4 * emits, "four products per EMIT and point"


def test_the_ext_body_keeps_every_operand_domain_on_saturated_operands():
    out, err = _run("emu_air_ext", "saturated")
    cases = test_emu_air_ext.parse_cases(out)
    assert len(cases) == 4
    for case in cases:
        assert (case["weights4"] == test_emu_air_ext.P - 1).all() and all((m == test_emu_air_ext.P - 1).all() for m in case["mats"])
        test_emu_air_ext.check_against_the_model(case)
    _judge("emu_air_ext", [err])


def test_both_ext_kernels_keep_every_operand_domain():
    errs = []
    for kernel in test_sim_air_ext.SITES:
        out, err = _run("sim_air_ext", "--only", kernel)
        assert "ALL OK" in out and "hard failures=0" in out, out[-2000:]
        errs.append(err)
    _judge("sim_air_ext", errs)
