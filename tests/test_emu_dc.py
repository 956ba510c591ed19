"""Steps the challenge-dependent preparation of include/toyni_hip.h 3p (toyni_amd/csrc/dc_kernels.hpp: the text the two one-wave
kernels and the record-fed twins run) on the CPU under AddressSanitizer + UBSan, as a stand-alone program (tests/emu/emu_dc.cpp).

Two judges, as in tests/test_emu_dz.py.  The program compares every record with memcmp against what the HOST code of the
host-argument entry points builds for the same values (to_mont_host, the rule of air_ext_weights, ext_shift_host), runs the PARAM
interpreter against the CONST one and the record-fed scan bodies against the argument-fed ones on the same inputs, and counts the
mismatches; this file recomputes every printed record from Python integers (tests/ext_model.py, toyni_amd.prover.air_ext_weights'
rule restated), so that a mistake shared by both sides of a memcmp would still show.  Raw words >= p (0xFFFFFFFF, p, p + 1) are among
the inputs of every record.  CPU only."""
import os
import subprocess

import ext_model as em
from test_emu_dz import shift_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = em.P
R = 1 << 32
NONE = 0xFFFFFFFF
EXT, EMIT_EXT = 0, 1
X_POWERS = ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1))


def build_emu_dc(contracts_header=None) -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_dc.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_dc" + ("_contracts" if contracts_header else "_asan"))
    deps = [src, os.path.join(ROOT, "tests", "emu", "contract_case.hpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if contracts_header:
        deps.append(contracts_header)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = ["-O2", "-include", contracts_header] if contracts_header else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "emu")] + flags + ["-o", out, src])
    return out


def run(program, mode):
    res = subprocess.run([program, mode], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return res


def judge(stdout, saturated):
    lines = stdout.split("\n")
    assert lines[-2] == "DONE" and lines[-3] == "BAD 0", lines[-3:]
    recs = [l.split() for l in lines[:-3]]
    assert not any(r[0] == "MISMATCH" for r in recs)
    ints = lambda f: [int(v) for v in f]
    k, quotients, scans, evals, terms, raw = 0, set(), set(), set(), [], set()
    while k < len(recs):
        r = recs[k]
        if r[0] == "QPREP":
            nparams, nalphas, form = ints(r[1:])
            par, al, rec = ints(recs[k + 1][1:]), ints(recs[k + 2][1:]), ints(recs[k + 3][1:])
            assert [recs[k + j][0] for j in (1, 2, 3)] == ["PAR", "AL", "REC"] and len(par) == nparams and len(al) == 4 * nalphas
            want = [w % P * R % P for w in par]                      # the Montgomery forms of the reduced parameters
            for a in range(nalphas):
                alpha = tuple(w % P for w in al[4 * a:4 * a + 4])
                want += list(alpha) if form == EXT else [c for j in range(4) for c in em.mul(alpha, X_POWERS[j])]   # alpha * X^j, plain
            assert rec == want, (nparams, nalphas, form)
            if form == EMIT_EXT and nalphas:
                a = [w % P for w in al[:4]]
                assert rec[nparams + 4:nparams + 8] == [11 * a[3] % P, a[0], a[1], a[2]]      # alpha * X as the header spells it
            quotients.add((nparams, nalphas, form))
            raw.update(par + al)
            k += 4
        elif r[0] == "SPREP":
            ni, di, norm = ints(r[1:])
            ch, rec = ints(recs[k + 1][1:]), ints(recs[k + 2][1:])
            assert recs[k + 1][0] == "CH" and recs[k + 2][0] == "SREC" and len(ch) == 12 and len(rec) == 24
            shift = lambda i: [0] * 4 if i == NONE else [w % P for w in ch[4 * i:4 * i + 4]]
            assert rec[:4] == shift(ni) and rec[4:8] == shift(di), (ni, di)
            assert rec[8:] == (shift_model([(P - c) % P for c in shift(di)]) if norm else [0] * 16), (ni, di, norm)   # adj_z, m_z of z = -shift
            scans.add((ni, di, norm))
            raw.update(ch)
            k += 3
        elif r[0] == "EVAL":
            evals.add(tuple(ints(r[1:])))
            k += 1
        else:
            assert r[0] == "TERMS", r[:3]
            terms.append(tuple(ints(r[1:])))
            k += 1
    assert quotients == {(p_, a, f) for p_ in (0, 1, 4, 256) for a in (1, 16, 17, 70) for f in (EXT, EMIT_EXT)}
    assert scans == {(ni, di, norm) for ni in (NONE, 0, 2) for di in (NONE, 0, 1) for norm in (0, 1)} | {(2, 2, 1)}
    assert {e[0] for e in evals} == {1, 2, 4, 8, 64} and {e[2] for e in evals} == {4, 256} and {e[4] for e in evals} == {EXT, EMIT_EXT}
    forms = {(1, 0, 1, 0), (1, NONE, 1, 0), (4, 1, 4, 0), (0, NONE, 1, 2), (4, 0, 0, NONE)}
    assert {t[1:5] for t in terms} == forms and {t[0] for t in terms} == {0, 1} and {t[5] for t in terms} == {1, 5, 8, 13}
    if saturated:
        assert raw == {0xFFFFFFFF, 2 * P - 1} or raw == {0xFFFFFFFF, 2 * P - 1, P + 5, P, 0}
    else:
        assert {0xFFFFFFFF, P, P + 1, 0} <= raw and sum(w >= P for w in raw) > 100
        assert all(t[6] >= 1 for t in terms if t[1:5] == (0, NONE, 1, 2)), "the gamma that makes a width-1 denominator zero is counted"


def test_records_and_twins_match_the_host_code_and_the_model():
    judge(run(build_emu_dc(), "cases").stdout, False)


def test_records_and_twins_with_every_word_saturated():
    judge(run(build_emu_dc(), "saturated").stdout, True)
