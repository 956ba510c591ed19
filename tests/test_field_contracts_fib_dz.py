"""The operand domains of the lazy field arithmetic (toyni_amd/csrc/bb_field.hpp) in the text of
include/toyni_hip.h 3q: tests/emu/emu_fib_dz.cpp and tests/sim/sim_fib_dz.cpp rebuilt with tests/emu/field_contracts.hpp in front, as
tests/test_field_contracts_dz.py rebuilds the programs of 3o.  Every word the new kernels read from device memory as a challenge or a
claimed value is reduced first (dz_reduce: a Montgomery product with any u32 on the left), so the domains must hold on the programs'
own cases (0, p - 1, p, p + 1 and 0xFFFFFFFF as z and as claimed values) AND on the saturated ones, where every such word and every
data word is p - 1.  Zero violations, the outputs still the models', and the primitives the text is made of must have been reached.

CPU only, stand-alone programs, no sanitizer; built into the existing build/ folders with a _contracts suffix."""
import test_emu_fib_dz
import test_sim_fib_dz
from test_field_contracts import HEADER
from test_field_contracts_transcript import _judge

REACH = {"bb_add", "bb_sub", "mont_mul"}


def test_the_bodies_keep_every_operand_domain_on_their_own_and_on_saturated_cases():
    program = test_emu_fib_dz.build_emu_fib_dz(HEADER)
    errs = []
    for mode, saturated in (("records", False), ("saturated", True)):
        res = test_emu_fib_dz.run(program, mode)
        assert "CONTRACT" not in res.stdout, "the contract lines belong on stderr"
        test_emu_fib_dz.judge_records(res.stdout, saturated)         # the contract build prints what the sanitized build prints
        errs.append(res.stderr)
    lines, _ = test_emu_fib_dz.script()
    res = test_emu_fib_dz.run(program, "script", lines)
    assert "CONTRACT" not in res.stdout and res.stdout.rstrip().endswith("DONE")
    errs.append(res.stderr)
    _judge("emu_fib_dz", errs, REACH)


def test_the_kernels_themselves_keep_every_operand_domain_on_their_own_and_on_saturated_cases():
    errs = []
    for args in ((), ("--saturated",)):
        rc, out, err = test_sim_fib_dz._sim(*args, contracts_header=HEADER)
        assert rc == 0 and "ALL OK" in out and "hard failures=0" in out, out[-2000:] + err[-2000:]
        assert "CONTRACT" not in out
        errs.append(err)
    _judge("sim_fib_dz", errs, REACH)
