"""The operand domains of the lazy field arithmetic (toyni_amd/csrc/bb_field.hpp) in the z-dependent preparation of
include/toyni_hip.h 3o: tests/emu/emu_dz.cpp rebuilt with tests/emu/field_contracts.hpp in front, as tests/test_field_contracts_transcript.py
rebuilds the transcript's program.  Everything the preparation reads from device memory is reduced first (dz_reduce: a Montgomery
product with any u32 on the left), so the domains must hold on the program's own cases (random z, a zero coordinate, the base field,
0, every word p - 1; absorbed words up to 2^32 - 1) AND on the saturated ones, where every device-resident challenge word -- z, every
weight, every claimed value -- and the multiplier are p - 1.  Zero violations, the outputs still the models', and the primitives the
text is made of must have been reached.

CPU only, a stand-alone program, no sanitizer; built into tests/emu/build with a _contracts suffix."""
import test_emu_dz
from test_field_contracts import HEADER
from test_field_contracts_transcript import _judge

REACH = {"bb_add", "bb_sub", "bb_reduce_2p", "mont_mul_lazy", "mont_mul", "mont_dot2"}


def test_the_preparation_keeps_every_operand_domain_on_its_own_and_on_saturated_cases():
    program = test_emu_dz.build_emu_dz(HEADER)
    errs = []
    for mode, saturated in (("prepare", False), ("saturated", True)):
        res = test_emu_dz.run(program, mode)
        assert "CONTRACT" not in res.stdout, "the contract lines belong on stderr"
        test_emu_dz.judge_prepare(res.stdout, saturated)             # the contract build prints what the sanitized build prints
        errs.append(res.stderr)
    _judge("emu_dz", errs, REACH)


def test_the_kernels_themselves_keep_every_operand_domain_on_their_own_and_on_saturated_cases():
    """tests/sim/sim_dz.cpp: the preparation kernels AND the device-record twins of the hot kernels, every data word p - 1 in the
    saturated run"""
    import test_sim_dz
    errs = []
    for saturated in (False, True):
        stdout, stderr = test_sim_dz.run(saturated, HEADER)
        assert "CONTRACT" not in stdout
        test_sim_dz.judge(stdout, saturated)
        errs.append(stderr)
    _judge("sim_dz", errs, REACH | {"mont_reduce_wide", "wide_acc"})


def test_the_transcript_helpers_keep_every_operand_domain():
    lines, want = test_emu_dz.transcript_script()
    res = test_emu_dz.run(test_emu_dz.build_emu_dz(HEADER), "transcript", lines)
    assert "CONTRACT" not in res.stdout
    test_emu_dz.judge_transcript(res.stdout, want)
    _judge("emu_dz", [res.stderr], {"bb_add", "bb_reduce_2p", "mont_mul_lazy", "mont_mul"})
