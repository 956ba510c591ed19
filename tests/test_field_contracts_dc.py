"""The operand domains of the lazy field arithmetic (toyni_amd/csrc/bb_field.hpp) in the challenge-dependent text
of include/toyni_hip.h 3p: tests/emu/emu_dc.cpp rebuilt with tests/emu/field_contracts.hpp in front, as
tests/test_field_contracts_air_ext.py and tests/test_field_contracts_dz.py rebuild theirs.  Every word the preparation reads from
device memory is reduced first (dz_reduce: a Montgomery product with any u32 on the left), so the domains must hold on the program's
own cases (any u32 as a parameter, an alpha coordinate or a shift word: 0xFFFFFFFF, p, p + 1 among them) AND on the saturated ones,
where every such word is 2^32 - 1 or reduces to p - 1 and every data word is p - 1 -- in the two preparations, in the PARAM
interpreter and in the record-fed scan bodies.  Zero violations, the outputs still the models', and the primitives the text is made
of must have been reached.

CPU only, a stand-alone program, no sanitizer; built into tests/emu/build with a _contracts suffix."""
import test_emu_dc
from test_field_contracts import HEADER
from test_field_contracts_transcript import _judge

REACH = {"bb_add", "bb_sub", "bb_reduce_2p", "mont_mul_lazy", "mont_mul", "mont_dot2"}


def test_the_device_challenge_text_keeps_every_operand_domain_on_its_own_and_on_saturated_cases():
    program = test_emu_dc.build_emu_dc(HEADER)
    errs = []
    for mode, saturated in (("cases", False), ("saturated", True)):
        res = test_emu_dc.run(program, mode)
        assert "CONTRACT" not in res.stdout, "the contract lines belong on stderr"
        test_emu_dc.judge(res.stdout, saturated)                     # the contract build prints what the sanitized build prints
        errs.append(res.stderr)
    _judge("emu_dc", errs, REACH)
