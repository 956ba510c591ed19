"""The operand domains of the lazy field arithmetic (toyni_amd/csrc/bb_field.hpp) in the text of
include/toyni_hip.h 3t: tests/sim/sim_fib_verify.cpp rebuilt with tests/emu/field_contracts.hpp in front, as
tests/test_field_contracts_fib_batch.py rebuilds the driver of 3s.  Every word the verifier reads from an image or from its work buffer
as a field element is reduced first, so the domains must hold on the tamper matrix's images (among them words no BabyBear can hold)
AND on a saturated proof: t_z ... q_z, every opened value and the whole final layer at p - 1, whose verdict is whatever the restated
reference verifier says of it.  Zero violations, the verdicts still the judge's, and the primitives the text is made of reached.

CPU only, a stand-alone program, no sanitizer; built into the existing build/ folder with a _contracts suffix."""
import re

import numpy as np

import fib_verify_cases as cases
import test_sim_fib_verify as sim
from test_field_contracts import HEADER
from test_field_contracts_transcript import _judge

REACH = {"bb_add", "bb_sub", "mont_mul"}
P = cases.P


def _saturate(raw):
    for k in ("t_z", "t_gz", "t_ggz", "q_z"):
        raw[k] = P - 1
    raw["fri_final_layer"] = [P - 1] * len(raw["fri_final_layer"])
    for g, (_tn, _s, idx) in enumerate(raw["opening_groups"]):
        for j in range(len(idx)):
            cases._set_value_words(raw, g, j, P - 1, 0)


def test_the_kernels_keep_every_operand_domain_on_the_matrix_and_on_a_saturated_proof(tmp_path):
    from toyni_amd import verifier
    errs = []
    raws, where = sim.batch_of(16)
    rc, out, err = sim.run_driver(sim.write_images(raws, str(tmp_path / "matrix.bin")), contracts_header=HEADER)
    assert rc == 0 and "ALL OK" in out and "hard failures=0" in out and "CONTRACT" not in out, out[-2000:] + err[-2000:]
    sim.judge(raws, where, out)
    errs.append(err)
    valid = cases.proofs(16)
    sat = cases.tampered(valid[1], _saturate)
    ok, want = cases.expected_of(sat)
    assert not ok
    rc, out, err = sim.run_driver(sim.write_images([valid[0], sat, valid[2]], str(tmp_path / "saturated.bin")), contracts_header=HEADER)
    assert rc == 0 and "ALL OK" in out and "hard failures=0" in out and "CONTRACT" not in out, out[-2000:] + err[-2000:]
    words = [int(w) for w in re.search(r"^VERDICTS (.*)$", out, re.M).group(1).split()]
    assert words[0] == 0 and words[2] == 0 and verifier.decode_verdict(words[1])[1] == want, (words, want)
    errs.append(err)
    _judge("sim_fib_verify", errs, REACH)
