"""The operand domains of the lazy field arithmetic (toyni_amd/csrc/bb_field.hpp) in the text of
include/toyni_hip.h 3s: tests/sim/sim_fib_batch.cpp rebuilt with tests/emu/field_contracts.hpp in front, as
tests/test_field_contracts_fib_dz.py rebuilds the driver of 3q.  The batch twins share the bodies of their originals, so every word
they read from device memory as a challenge or a claimed value is reduced first; the domains must hold on the driver's own cases AND on
the saturated ones, where every such word and every data word is p - 1.  Zero violations, the outputs still those of the single
kernels and of host arithmetic, and the primitives the text is made of must have been reached.

CPU only, a stand-alone program, no sanitizer; built into the existing build/ folder with a _contracts suffix."""
import test_sim_fib_batch
from test_field_contracts import HEADER
from test_field_contracts_transcript import _judge

REACH = {"bb_add", "bb_sub", "mont_mul"}


def test_the_kernels_themselves_keep_every_operand_domain_on_their_own_and_on_saturated_cases():
    errs = []
    for args in ((), ("--saturated",)):
        rc, out, err = test_sim_fib_batch._sim(*args, contracts_header=HEADER)
        assert rc == 0 and "ALL OK" in out and "hard failures=0" in out, out[-2000:] + err[-2000:]
        assert "CONTRACT" not in out
        errs.append(err)
    _judge("sim_fib_batch", errs, REACH)
