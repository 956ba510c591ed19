"""The operand domains of the lazy field arithmetic (toyni_amd/csrc/bb_field.hpp) in the four-to-one Ext FRI round
(include/toyni_hip.h 3m): tests/emu/emu_fold4_ext_commit.cpp -- the leaf body fold4_ext_commit_leaf with its 12 pairwise folds and the
products s / I and s^2 of the point inverses, and the record fri4_round_record with its Ext square -- rebuilt with
tests/emu/field_contracts.hpp in front, as tests/test_field_contracts_transcript.py rebuilds the transcript's program.

Zero violations on the program's own cases and on the saturated ones (every data word p - 1, every challenge coordinate and x0^-1 the
value whose Montgomery form is p - 1), the outputs still the oracle's and hashlib's, and the primitives the text is made of reached.

CPU only, a stand-alone program, no sanitizer; built into tests/emu/build with a _contracts suffix."""
import subprocess

import test_emu_fold4_ext_commit as emu4
from test_field_contracts import HEADER, PRIMITIVES, _sum_contracts

REACH = {"bb_add", "bb_sub_lazy", "bb_halve", "bb_reduce_2p", "mont_mul_lazy", "mont_mul", "mont_dot2"}


def _run(*args):
    res = subprocess.run([emu4.build_emu_fold4(HEADER), *args], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "CONTRACT" not in res.stdout, "the contract lines belong on stderr"
    return res


def _judge(errs):
    total = _sum_contracts(errs)
    assert sorted(total) == sorted(PRIMITIVES)
    bad = ["%s: %d violations in %d calls, %s" % (p, v, c, rest) for p, (c, v, rest) in total.items() if v]
    assert not bad, "emu_fold4_ext_commit left an operand domain:\n" + "\n".join(bad)
    reached = {p for p, (c, _, _) in total.items() if c}
    assert REACH <= reached, "emu_fold4_ext_commit never called %s" % sorted(REACH - reached)
    return total


def test_the_fold4_round_keeps_every_operand_domain():
    res = _run()
    seen = emu4.judge(res.stdout)                      # the contract build prints what the sanitized build prints
    total = _judge([res.stderr])
    # 12 pairwise folds per leaf, each with four 2-term dot products per coordinate pair: 8 mont_dot2 per fold, plus one Ext square
    leaves = sum(m // 16 for m, *_ in seen)
    assert total["mont_dot2"][0] >= 8 * 12 * leaves + 8 * len(seen)


def test_the_fold4_round_keeps_every_operand_domain_on_saturated_operands():
    res = _run("saturated")
    assert len(emu4.judge(res.stdout)) == 12
    _judge([res.stderr])
