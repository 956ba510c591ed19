"""Section 3p of include/toyni_hip.h (gamma and the constraint weights in device memory): the symbols are exported and bound as the
header declares them, toyni_air_program_check_params accepts TOYNI_AIR_PARAM and reports nparams while toyni_air_program_check keeps
refusing op 8, every refusal that is decided on the arguments alone, and the Python side (AirBuilder.param / ext_param,
ExtOperandDc).  CPU only: no call here reaches a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2013265921
E_NULL, E_RANGE = 10002, 10006
CELL, CONST, X, XINV, ADD, SUB, MUL, EMIT, PARAM = range(9)
NAMES = ["toyni_air_program_check_params", "toyni_air_program_create_params", "toyni_air_program_nparams", "toyni_air_quotient_ext_dc_device",
         "toyni_column_scan_ext_dc_device"]
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def check_params(ta, insns):
    arr = ta.prover.air_insns(insns)
    info, nparams = ta.prover.AirInfo(), ctypes.c_uint32(77)
    rc = ta._lib.lib.toyni_air_program_check_params(arr, len(arr), ctypes.byref(info), ctypes.byref(nparams))
    return rc, info, nparams.value


def test_symbols_are_exported_and_bound_as_the_header_declares(ta):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "toyni_hip.h")).read(), flags=re.S)
    for name in NAMES:
        f = getattr(ta._lib.lib, name)
        assert name in ta._lib.SIGNATURES and f.argtypes == ta._lib.SIGNATURES[name][1] and f.restype is ctypes.c_int
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert m and len(m.group(1).split(",")) == len(f.argtypes), name
    m = re.search(r"\bint\s+toyni_air_quotient_ext_dc_device\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == [
        "toyni_ntt_ctx* ctx", "const toyni_air_program* prog", "const toyni_air_matrix* mats", "size_t nmats", "unsigned log_blowup", "uint32_t shift",
        "const uint32_t* d_params", "size_t nparams", "const uint32_t* d_alphas", "size_t nalphas", "int weights_form", "uint32_t* d_c_out",
        "uint32_t* d_q_out", "size_t out_stride", "int accumulate", "void* stream"]
    m = re.search(r"\bint\s+toyni_column_scan_ext_dc_device\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == [
        "toyni_ntt_ctx* ctx", "const toyni_ext_operand_dc* num", "const toyni_ext_operand_dc* den", "const uint32_t* d_challenges", "uint32_t* d_out",
        "size_t out_stride", "size_t n", "size_t batch", "int op", "const uint32_t* init", "uint32_t* d_totals", "void* stream"]
    defines = dict(re.findall(r"#define (TOYNI_\w+) (\w+)", header))
    assert (defines["TOYNI_AIR_PARAM"], defines["TOYNI_AIR_MAX_PARAMS"]) == ("8", "256")
    assert (defines["TOYNI_AIR_WEIGHTS_EXT"], defines["TOYNI_AIR_WEIGHTS_EMIT_EXT"], defines["TOYNI_EXT_SHIFT_NONE"]) == ("0", "1", "0xffffffffu")
    pv = ta.prover
    assert (pv.AIR_PARAM, pv.AIR_MAX_PARAMS, pv.AIR_WEIGHTS_EXT, pv.AIR_WEIGHTS_EMIT_EXT, pv.EXT_SHIFT_NONE) == (8, 256, 0, 1, NONE)
    assert ctypes.sizeof(pv._ExtOperandDc) == 24 and ctypes.sizeof(pv.AirInfo) == 40            # toyni_air_info stays 40 bytes


def test_check_params_accepts_op_8_and_reports_nparams_and_check_still_refuses_it(ta):
    lib = ta._lib.lib
    prog = [(PARAM, 0, 0, 0, 3), (CELL, 1, 0, 0, 0), (MUL, 2, 0, 1, 0), (PARAM, 3, 9, 9, 255), (ADD, 2, 2, 3, 0), (EMIT, 0, 2, 0, 1)]
    rc, info, nparams = check_params(ta, prog)                       # (a and b of PARAM are unused and not checked)
    assert (rc, nparams) == (0, 256)
    assert (info.ninsns, info.nregs, info.nconstraints, info.nmatrices, info.divides_by_zh) == (6, 4, 2, 1, 1)
    rc, _, nparams = check_params(ta, [(PARAM, 5, 0, 0, 0), (EMIT, 0, 5, 1, 0)])
    assert (rc, nparams) == (0, 1)
    rc, _, nparams = check_params(ta, [(X, 0, 0, 0, 0), (EMIT, 0, 0, 1, 0)])    # no PARAM: 0, and everything else as toyni_air_program_check
    assert (rc, nparams) == (0, 0)
    for what, bad in [("imm 256", [(PARAM, 0, 0, 0, 256), (EMIT, 0, 0, 1, 0)]), ("op 9", [(9, 0, 0, 0, 0), (EMIT, 0, 0, 1, 0)]),
                      ("op 255", [(255, 0, 0, 0, 0), (EMIT, 0, 0, 1, 0)]), ("dst 64", [(PARAM, 64, 0, 0, 0), (X, 0, 0, 0, 0), (EMIT, 0, 0, 1, 0)]),
                      ("a register no PARAM wrote", [(PARAM, 1, 0, 0, 0), (EMIT, 0, 0, 1, 0)]), ("no EMIT", [(PARAM, 0, 0, 0, 0)]),
                      ("CONST = p", [(CONST, 0, 0, 0, P), (EMIT, 0, 0, 1, 0)])]:
        rc, _, nparams = check_params(ta, bad)
        assert rc == E_RANGE and nparams == 77, what                 # a refusal leaves *nparams alone
    arr = ta.prover.air_insns(prog)
    info = ta.prover.AirInfo()
    assert lib.toyni_air_program_check(arr, len(arr), ctypes.byref(info)) == E_RANGE
    with pytest.raises(RuntimeError):
        ta.prover.air_program_check(prog)
    got_info, got_n = ta.prover.air_program_check_params(prog)
    assert got_n == 256 and got_info.nregs == 4
    n = ctypes.c_uint32()
    assert lib.toyni_air_program_check_params(None, 6, ctypes.byref(info), ctypes.byref(n)) == E_NULL
    assert lib.toyni_air_program_check_params(arr, 6, None, ctypes.byref(n)) == E_NULL
    assert lib.toyni_air_program_check_params(arr, 6, ctypes.byref(info), None) == E_NULL
    assert lib.toyni_air_program_check_params(arr, 0, ctypes.byref(info), ctypes.byref(n)) == E_RANGE
    h = ctypes.c_void_p()
    assert lib.toyni_air_program_create_params(None, arr, 6, ctypes.byref(h)) == E_NULL
    assert lib.toyni_air_program_create_params(ctypes.c_void_p(0x1000), None, 6, ctypes.byref(h)) == E_NULL
    assert lib.toyni_air_program_create_params(ctypes.c_void_p(0x1000), arr, 6, None) == E_NULL
    bad = ta.prover.air_insns([(PARAM, 0, 0, 0, 256), (EMIT, 0, 0, 1, 0)])
    assert lib.toyni_air_program_create_params(ctypes.c_void_p(0x1000), bad, 2, ctypes.byref(h)) == E_RANGE      # refused before the context is read
    assert lib.toyni_air_program_create(ctypes.c_void_p(0x1000), arr, 6, ctypes.byref(h)) == E_RANGE             # op 8 under the check of 3f
    assert lib.toyni_air_program_nparams(None, ctypes.byref(n)) == E_NULL
    assert lib.toyni_air_program_nparams(ctypes.c_void_p(0x1000), None) == E_NULL


def test_quotient_refusals_that_need_no_device(ta):
    call = ta._lib.lib.toyni_air_quotient_ext_dc_device
    ctx, prog, q, al, pa = (ctypes.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000))   # never dereferenced: the refusal comes first
    assert call(None, prog, None, 0, 0, 7, pa, 4, al, 4, 1, None, q, 8, 0, None) == E_NULL          # context
    assert call(ctx, None, None, 0, 0, 7, pa, 4, al, 4, 1, None, q, 8, 0, None) == E_NULL           # program
    assert call(ctx, prog, None, 0, 0, 7, pa, 4, None, 4, 1, None, q, 8, 0, None) == E_NULL         # d_alphas
    assert call(ctx, prog, None, 0, 0, 7, None, 4, al, 4, 1, None, q, 8, 0, None) == E_NULL         # d_params with nparams > 0
    assert call(ctx, prog, None, 0, 0, 7, pa, 4, al, 4, 1, None, None, 8, 0, None) == E_NULL        # d_q_out
    assert call(ctx, prog, None, 1, 0, 7, pa, 4, al, 4, 1, None, q, 8, 0, None) == E_NULL           # mats with nmats > 0
    for form in (2, -1):
        assert call(ctx, prog, None, 0, 0, 7, pa, 4, al, 4, form, None, q, 8, 0, None) == E_RANGE   # an unknown form
    assert call(ctx, prog, None, 0, 0, 7, pa, 257, al, 4, 1, None, q, 8, 0, None) == E_RANGE        # nparams > TOYNI_AIR_MAX_PARAMS
    assert call(ctx, prog, None, 0, 0, 7, pa, 4, al, 65537, 0, None, q, 8, 0, None) == E_RANGE      # nweights > 65536 whatever the form
    assert call(ctx, prog, None, 0, 0, 7, ctypes.c_void_p(0x5002), 4, al, 4, 1, None, q, 8, 0, None) == E_RANGE   # misaligned d_params
    assert call(ctx, prog, None, 0, 0, 7, pa, 4, ctypes.c_void_p(0x4001), 4, 1, None, q, 8, 0, None) == E_RANGE   # misaligned d_alphas


def test_scan_refusals_that_need_no_device(ta):
    pv = ta.prover
    call = ta._lib.lib.toyni_column_scan_ext_dc_device
    ctx, out, ch, col = (ctypes.c_void_p(v) for v in (0x1000, 0x2000, 0x3000, 0x4000))
    init = (ctypes.c_uint32 * 8)(1, 0, 0, 0, 1, 0, 0, 0)
    good = pv.ExtOperandDc(0x4000, 16, 1, 0)
    ref = ctypes.byref

    def rc(num=good, den=good, c=ctx, chal=ch, o=out, stride=16, n=16, batch=1, op=0, ini=init, totals=None):
        return call(c, ref(num) if num is not None else None, ref(den) if den is not None else None, chal, o, stride, n, batch, op, ini, totals, None)

    assert rc(c=None) == E_NULL and rc(o=None) == E_NULL and rc(ini=None) == E_NULL
    assert rc(chal=None) == E_NULL                                                   # an operand names an index
    assert rc(num=pv.ExtOperandDc(0x4000, 16, 1), den=None, chal=None, n=0) == 0     # no index named: d_challenges may be null (n == 0: nothing runs)
    assert rc(num=None, den=None) == E_RANGE                                         # both operands absent
    assert rc(num=pv.ExtOperandDc(0, 0, 0), den=pv.ExtOperandDc(0, 0, 0)) == E_RANGE
    assert rc(num=pv.ExtOperandDc(0x4000, 16, 2, 0)) == E_RANGE                      # a width not in {0, 1, 4}
    assert rc(num=pv.ExtOperandDc(0, 16, 1, 0)) == E_RANGE                           # width > 0 with null d_values
    assert rc(num=pv.ExtOperandDc(0x4002, 16, 1, 0)) == E_RANGE                      # misaligned column
    assert rc(num=pv.ExtOperandDc(0x4000, 15, 4, 0)) == E_RANGE                      # width 4: stride < n
    assert rc(num=pv.ExtOperandDc(0x4000, 15, 1, 0), batch=2) == E_RANGE             # batch > 1: stride < n
    assert rc(num=pv.ExtOperandDc(0x4000, 15, 1, 0), n=0) == 0                       # ... a single base column may be short (3i)
    assert rc(den=pv.ExtOperandDc(0x4000, 16, 1, 1 << 20)) == E_RANGE                # index >= 2^20
    assert rc(den=pv.ExtOperandDc(0x4000, 16, 1, NONE - 1)) == E_RANGE
    assert rc(den=pv.ExtOperandDc(0x4000, 16, 1, (1 << 20) - 1), n=0) == 0
    assert rc(op=2) == E_RANGE and rc(op=-1) == E_RANGE
    assert rc(n=(1 << 27) + 1, stride=1 << 28, num=pv.ExtOperandDc(0x4000, 1 << 28, 1, 0), den=None) == E_RANGE
    assert rc(stride=15) == E_RANGE                                                  # out_stride < n
    assert rc(batch=1 << 14, n=0) == E_RANGE
    assert rc(chal=ctypes.c_void_p(0x3002)) == E_RANGE                               # misaligned d_challenges
    assert rc(o=ctypes.c_void_p(0x2001)) == E_RANGE and rc(totals=ctypes.c_void_p(0x6002)) == E_RANGE
    assert rc(ini=(ctypes.c_uint32 * 4)(0, 0, P, 0)) == E_RANGE                      # init stays a host array of canonical residues
    assert rc(n=0) == 0 and rc(batch=0) == 0                                         # nothing to do: succeeds, the context not touched


def test_builder_parameters_compile_to_param_instructions(ta):
    pv = ta.prover
    bld = pv.AirBuilder()
    g = bld.ext_param(4)
    assert bld.param(5) is g.c[1]                                    # equal nodes are one object, as constants are
    bld.emit_ext(0, (g + bld.cell(0, 0)) * bld.ext_cell(1, 0), divide=False)
    insns = bld.compile()
    params = [i for i in insns if i[0] == PARAM]
    assert sorted(i[4] for i in params) == [4, 5, 6, 7] and all(i[2] == 0 and i[3] == 0 for i in params)
    info, nparams = pv.air_program_check_params(insns)
    assert nparams == 8 and info.nconstraints == 4
    with pytest.raises(RuntimeError):
        pv.air_program_check(insns)
    # the same expression over constants compiles to the same program with CONST in PARAM's places
    bld2 = pv.AirBuilder()
    g2 = bld2.ext_const((14, 15, 16, 17))
    bld2.emit_ext(0, (g2 + bld2.cell(0, 0)) * bld2.ext_cell(1, 0), divide=False)
    subst = [(CONST, d, 0, 0, 10 + imm) if op == PARAM else (op, d, a, b, imm) for op, d, a, b, imm in insns]
    assert subst == bld2.compile()
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            bld.param(bad)
    with pytest.raises(ValueError):
        bld.ext_param(253)
