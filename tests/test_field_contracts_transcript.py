"""The operand domains of the lazy field arithmetic (toyni_amd/csrc/bb_field.hpp) in the device transcript and the
fused rounds of its commit phase (include/toyni_hip.h 3l): the two CPU programs that run their text -- tests/emu/emu_transcript.cpp (the
transcript functions and the u64 reduction at its edges) and tests/sim/sim_fri_tail.cpp (the two instantiations of
fri_tail_rounds_kernel) -- rebuilt with tests/emu/field_contracts.hpp in front, as tests/test_field_contracts_air_ext.py rebuilds the
programs of the AIR quotient.

bb_reduce_u64 takes any u64: it is two Montgomery products with any u32 on the left and a canonical constant on the right, then a
bb_add of two canonical values, and each of those reports itself.  The fused rounds turn a plain beta into the factors of a fold
(mont_mul with host constants) and fold with fold_one / fold_ext_one.  Zero violations, the outputs still the models', and the
primitives the text is made of must have been reached.

CPU only, stand-alone programs, no sanitizer; built into the existing build/ folders with a _contracts suffix."""
import os
import subprocess
from functools import lru_cache

import __graft_entry__ as entry
import test_emu_transcript
import test_sim_fri_tail
from test_field_contracts import CSRC, EMU, HEADER, PRIMITIVES, ROOT, SIM, _stale, _sum_contracts


@lru_cache(maxsize=None)
def build_sim_contracts():
    src, out = os.path.join(SIM, "sim_fri_tail.cpp"), os.path.join(SIM, "build", "sim_fri_tail_contracts")
    deps = [src, HEADER, os.path.join(EMU, "contract_case.hpp"), os.path.join(SIM, "hip_sim.hpp"), os.path.join(ROOT, "include", "toyni_hip.h")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))]
    if _stale(out, deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        # hip_sim.hpp first: it defines the host forms of the synchronisation macros, which bb_field.hpp keeps when it finds them
        subprocess.check_call([entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-include", os.path.join(SIM, "hip_sim.hpp"), "-include", HEADER,
                               "-o", out, src])
    return out


def _judge(program, errs, reach):
    total = _sum_contracts(errs)
    assert sorted(total) == sorted(PRIMITIVES)
    bad = ["%s: %d violations in %d calls, %s" % (p, v, c, rest) for p, (c, v, rest) in total.items() if v]
    assert not bad, program + " left an operand domain:\n" + "\n".join(bad)
    reached = {p for p, (c, _, _) in total.items() if c}
    assert reach <= reached, "%s never called %s" % (program, sorted(reach - reached))
    return total


def test_the_transcript_functions_keep_every_operand_domain():
    lines, want = test_emu_transcript.script()
    res = test_emu_transcript.run(test_emu_transcript.build_emu_transcript(HEADER), lines)
    assert "CONTRACT" not in res.stdout, "the contract lines belong on stderr"
    test_emu_transcript.judge(res.stdout, want)                      # the contract build prints what the sanitized build prints
    total = _judge("emu_transcript", [res.stderr], {"bb_add", "bb_reduce_2p", "mont_mul_lazy", "mont_mul"})
    # (a squeeze of a transcript whose status is set writes zeros and reduces nothing)
    reductions = sum(len(exp) for kind, exp in want if kind == "R" or (kind == "S" and any(exp)))
    assert total["mont_mul"][0] >= 2 * reductions and total["bb_add"][0] >= reductions, "two products and one add per reduction"


def test_both_fused_rounds_kernels_keep_every_operand_domain():
    errs = []
    for kernel in test_sim_fri_tail.SITES:
        res = subprocess.run([build_sim_contracts(), "--only", kernel], capture_output=True, text=True, timeout=900)
        assert res.returncode == 0 and "ALL OK" in res.stdout and "hard failures=0" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
        assert "CONTRACT" not in res.stdout
        errs.append(res.stderr)
    _judge("sim_fri_tail", errs, {"bb_add", "bb_sub_lazy", "bb_halve", "bb_reduce_2p", "mont_mul_lazy", "mont_mul", "mont_dot2"})
