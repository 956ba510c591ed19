"""The constraint-program entry points of include/toyni_hip.h 3f: exported and bound; toyni_air_program_check validates on the host
alone (no device here), refuses each malformed program for its one defect, and reports exactly what a call must supply."""
import ctypes

import pytest

P = 2013265921
E_NULL, E_RANGE = 10002, 10006
CELL, CONST, X, XINV, ADD, SUB, MUL, EMIT = range(8)
NAMES = ["toyni_air_program_check", "toyni_air_program_create", "toyni_air_program_destroy", "toyni_air_program_info", "toyni_air_quotient_device"]


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def check(ta, insns, n=None):
    arr = ta.prover.air_insns(insns)
    info = ta.prover.AirInfo()
    rc = ta._lib.lib.toyni_air_program_check(arr if len(insns) else None, len(insns) if n is None else n, ctypes.byref(info))
    return rc, info


# an otherwise valid program: every refusal below changes one thing in it
GOOD = [(CELL, 0, 0, 0, 0), (CONST, 1, 0, 0, P - 1), (X, 2, 0, 0, 0), (XINV, 3, 0, 0, 5), (ADD, 4, 0, 1, 0), (SUB, 5, 4, 2, 0), (MUL, 63, 5, 3, 0),
        (EMIT, 0, 63, 0, 0)]


def changed(index, **fields):
    names = ("op", "dst", "a", "b", "imm")
    out = list(GOOD)
    ins = dict(zip(names, out[index]))
    ins.update(fields)
    out[index] = tuple(ins[k] for k in names)
    return out


def test_symbols_are_exported_and_bound(ta):
    for name in NAMES:
        f = getattr(ta._lib.lib, name)
        assert name in ta._lib.SIGNATURES and f.argtypes == ta._lib.SIGNATURES[name][1] and f.restype is ctypes.c_int
    assert ctypes.sizeof(ta.prover.AirInsn) == 8 and ctypes.sizeof(ta.prover.AirInfo) == 40
    for name in ("air_insns", "AirProgram", "air_quotient_device", "AirBuilder"):
        assert hasattr(ta.prover, name)


def test_the_valid_program_passes(ta):
    rc, _ = check(ta, GOOD)
    assert rc == 0


@pytest.mark.parametrize("what,insns", [
    ("unknown op", changed(4, op=8)),
    ("unknown op 255", changed(4, op=255)),
    ("dst is register 64", changed(4, dst=64)),
    ("a is register 64", changed(4, a=64)),
    ("b is register 64", changed(4, b=64)),
    ("a read before it is written", changed(4, a=7)),
    ("b read before it is written", changed(4, b=5)),
    ("an operand written only later", changed(4, a=63)),
    ("EMIT of a register never written", changed(7, a=9)),
    ("EMIT of register 64", changed(7, a=64)),
    ("CONST = p", changed(1, imm=P)),
    ("XINV = p", changed(3, imm=P)),
    ("CELL matrix 4", changed(0, b=4)),
    ("CELL column 65536", changed(0, imm=65536)),
    ("EMIT number 65536", changed(7, imm=65536)),
    ("EMIT b = 2", changed(7, b=2)),
    ("no EMIT", GOOD[:7]),
    ("no EMIT, though the last instruction is fine", changed(7, op=ADD, dst=6, a=0, b=0, imm=0)),
])
def test_each_malformed_program_is_refused(ta, what, insns):
    rc, _ = check(ta, insns)
    assert rc == E_RANGE, what


def test_length_limits_and_null_arguments(ta):
    lib = ta._lib.lib
    info = ta.prover.AirInfo()
    arr = ta.prover.air_insns(GOOD)
    assert lib.toyni_air_program_check(arr, 0, ctypes.byref(info)) == E_RANGE
    long = [(X, 0, 0, 0, 0)] * 65535 + [(EMIT, 0, 0, 1, 0)]
    assert check(ta, long)[0] == 0
    assert check(ta, [(X, 0, 0, 0, 0)] + long)[0] == E_RANGE                     # 65537 instructions
    assert lib.toyni_air_program_check(None, 8, ctypes.byref(info)) == E_NULL
    assert lib.toyni_air_program_check(arr, 8, None) == E_NULL
    # the other entry points refuse null arguments before they look for a device
    h = ctypes.c_void_p()
    assert lib.toyni_air_program_create(None, arr, 8, ctypes.byref(h)) == E_NULL
    assert lib.toyni_air_program_info(None, ctypes.byref(info)) == E_NULL
    assert lib.toyni_air_program_destroy(None) == 0                               # null-safe
    w = (ctypes.c_uint32 * 1)(1)
    assert lib.toyni_air_quotient_device(None, None, None, 0, 0, 7, w, 1, None, None, 0, None) == E_NULL


def test_info_reports_exactly_what_a_call_must_supply(ta):
    rc, info = check(ta, GOOD)
    assert rc == 0
    assert (info.ninsns, info.nregs, info.nconstraints, info.nmatrices, info.max_rotation, info.divides_by_zh) == (8, 64, 1, 1, 0, 1)
    assert list(info.min_width) == [1, 0, 0, 0]
    prog = [(CELL, 0, 3, 2, 40), (CELL, 1, 200, 0, 6), (CELL, 2, 1, 2, 7), (ADD, 3, 0, 1, 0), (EMIT, 0, 3, 1, 9), (EMIT, 0, 2, 1, 2), (EMIT, 0, 2, 1, 9)]
    rc, info = check(ta, prog)
    assert rc == 0
    assert (info.ninsns, info.nregs, info.nconstraints, info.nmatrices, info.max_rotation, info.divides_by_zh) == (7, 4, 10, 3, 200, 0)
    assert list(info.min_width) == [7, 0, 41, 0]
    # operand fields that an instruction does not use are not registers: CONST / X / XINV ignore a and b, EMIT ignores dst
    rc, info = check(ta, [(CONST, 0, 200, 200, 1), (X, 1, 99, 99, 0), (XINV, 2, 77, 77, 0), (EMIT, 255, 2, 0, 0)])
    assert rc == 0 and info.nregs == 3 and info.nmatrices == 0 and info.divides_by_zh == 1
    assert ta.prover.air_program_check(prog).nconstraints == 10
