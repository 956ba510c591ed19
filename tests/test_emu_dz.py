"""Steps the z-dependent preparation of include/toyni_hip.h 3o (toyni_amd/csrc/dz_kernels.hpp: the text the one-wave kernels run) on
the CPU under AddressSanitizer + UBSan, as a stand-alone program (tests/emu/emu_dz.cpp).

Two judges.  The program itself compares every record with memcmp against what the HOST code of the host-argument entry points
builds for the same values (ext_pow_host, poly_ext_powers_host, ext_shift_host, the table loop) and counts the mismatches; this file
recomputes every printed word from Python integers (tests/ext_model.py) and hashlib, so that a mistake shared by both sides of the
memcmp would still show.  z: random, one with a zero coordinate, one in the base field, 0, every word p - 1, 1.

absorb_fields against written-out bytes at counts 0, 1, 4, 96 and 126 (one lane and a wave of 64), on the overflow into the status and
on a status already set; the point rule through its loop with the accept predicate replaced (the rejection branch, the bound of 8
tries); the query rows at n = 1, n = 2^32, an offset of n - 1, 1 and 8 offsets.  CPU only."""
import os
import subprocess

import numpy as np

import ext_model as em
from test_emu_transcript import CAPACITY, E_RANGE, Model, pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = em.P
R = 1 << 32
ZETA = pow(11, (P - 1) // 4, P)
LOG_PER_THREAD, LOG_CHUNK, BITS = 4, 12, 8
FIELD_COUNTS = [0, 1, 4, 96, 126]


def build_emu_dz(contracts_header=None) -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_dz.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_dz" + ("_contracts" if contracts_header else "_asan"))
    deps = [src, os.path.join(ROOT, "tests", "emu", "contract_case.hpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if contracts_header:
        deps.append(contracts_header)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = ["-O2", "-include", contracts_header] if contracts_header else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "emu")] + flags + ["-o", out, src])
    return out


def run(program, mode, lines=()):
    res = subprocess.run([program, mode], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return res


def factor(v):
    """ExtFactor of a plain Ext value: the Montgomery forms of its coordinates, then of 11 times them"""
    return [c * R % P for c in v] + [11 * c * R % P for c in v]


def powers_model(point):
    sq = [tuple(point)]
    for _ in range(LOG_CHUNK + BITS):
        sq.append(em.mul(sq[-1], sq[-1]))
    assert sq[LOG_CHUNK] == em.power(tuple(point), 4096)
    thread = factor(sq[0]) + [w for i in range(BITS) for w in factor(sq[LOG_PER_THREAD + i])]
    chunk = factor(sq[LOG_CHUNK + BITS]) + [w for i in range(BITS) for w in factor(sq[LOG_CHUNK + i])]
    return thread + chunk


def shift_model(z):
    """adj_z(x) = prod_{j=1..3} (x - phi^j(z)) and m_z(x) = (x - z) adj_z(x), coefficient i of x^i, in Montgomery form"""
    c = [tuple(z[k] * pow(ZETA, j * k, P) % P for k in range(4)) for j in (1, 2, 3)]
    a2 = em.neg(em.add(em.add(c[0], c[1]), c[2]))
    a1 = em.add(em.add(em.mul(c[0], c[1]), em.mul(c[0], c[2])), em.mul(c[1], c[2]))
    a0 = em.neg(em.mul(em.mul(c[0], c[1]), c[2]))
    z = tuple(z)
    m = [em.neg(em.mul(z, a0)), em.sub(a0, em.mul(z, a1)), em.sub(a1, em.mul(z, a2)), em.sub(a2, z)]
    assert all(not any(v[1:]) for v in m), "the norm has base-field coefficients"
    return [w * R % P for a in (a0, a1, a2) for w in a] + [v[0] * R % P for v in m]


def judge_prepare(stdout, saturated):
    lines = stdout.split("\n")
    assert lines[-2] == "DONE" and lines[-3] == "BAD 0", lines[-3:]
    recs = [l.split() for l in lines[:-3]]
    assert not any(r[0] == "MISMATCH" for r in recs)
    k, zs, mults, deep_shapes = 0, set(), set(), set()
    while k < len(recs):
        r = recs[k]
        if r[0] == "PREP":
            z, mult = tuple(map(int, r[1:5])), int(r[5])
            got = list(map(int, recs[k + 1][1:]))
            assert recs[k + 1][0] == "PW" and got == powers_model(tuple(c * mult % P for c in z)), (z, mult)
            zs.add(z), mults.add(mult)
            k += 2
        elif r[0] == "SHIFT":
            z = tuple(map(int, r[1:5]))
            assert recs[k + 1][0] == "SH" and list(map(int, recs[k + 1][1:])) == shift_model(z), z
            k += 2
        else:
            assert r[0] == "DEEP"
            nslots = int(r[1])
            slots = [tuple(map(int, recs[k + 1 + t][1:])) for t in range(nslots)]
            assert all(recs[k + 1 + t][0] == "SLOT" for t in range(nslots))
            al, cl, rec, tab = (np.array(list(map(int, recs[k + 1 + nslots + j][1:])), dtype=np.uint64) for j in range(4))
            assert [recs[k + 1 + nslots + j][0] for j in range(4)] == ["AL", "CL", "REC", "TAB"]
            al, cl, tab = al.reshape(-1, 4), cl.reshape(-1, 4), tab.reshape(nslots, 8)
            claim = em.ZERO
            assert slots == sorted(slots, key=lambda s: (s[0], s[1]))
            for t, (column, rot, ai, vi) in enumerate(slots):
                a, v = tuple(int(w) for w in al[ai]), tuple(int(w) for w in cl[vi])
                claim = em.add(claim, em.mul(a, v))
                assert [int(w) for w in tab[t]] == [column, rot] + [w * R % P for w in a] + [0, 0], (nslots, t)
            assert tuple(int(w) for w in rec) == claim, nslots
            deep_shapes.add(nslots)
            k += 5 + nslots
    assert deep_shapes == {1, 5, 64, 65, 130}
    if saturated:
        assert zs == {(P - 1,) * 4} and mults == {1, P - 1}
    else:
        assert {(0, 0, 0, 0), (P - 1,) * 4, (1, 0, 0, 0)} <= zs and len(mults) == 2 and 1 in mults
        assert any(z[0] and not any(z[1:]) and z[0] != 1 for z in zs) and any(z[1] == 0 and z[2] and z[3] for z in zs)
        assert sum(all(z) for z in zs) >= 6


def test_preparation_records_match_the_host_code_and_the_model():
    judge_prepare(run(build_emu_dz(), "prepare").stdout, False)


def test_preparation_records_with_every_word_saturated():
    judge_prepare(run(build_emu_dz(), "saturated").stdout, True)


def field_bytes(words):
    return b"".join((w % P).to_bytes(8, "little") for w in words)


def transcript_script():
    """(lines for the program, expected answers in order): ("T", Model) | ("Z", [z]) | ("W", [rows])"""
    lines, want = [], []
    rng = np.random.default_rng(0xD2)

    def start(state, status=0):
        lines.append("init " + (state.hex() or "-"))
        if status:
            lines.append(f"status {status}")
        return Model(state, status)

    def state_line(m):
        lines.append("state")
        want.append(("T", Model(m.state, m.status)))

    def fields(m, words, lanes):
        lines.append(f"fields {lanes} " + " ".join(str(w) for w in words))
        m.absorb(field_bytes(words))

    def point(m, reject=0):
        if reject:
            lines.append(f"reject {reject}")
        lines.append("point")
        if m.status:
            want.append(("Z", [0] * 4))
            return
        trial = Model(m.state)
        for tries in range(8):
            z = trial.squeeze(4)
            if tries >= reject and any(z[1:]):
                m.state = trial.state
                want.append(("Z", z))
                return
        m.status = E_RANGE
        want.append(("Z", [0] * 4))

    # absorb_fields: every count, one lane and a whole wave, words that need the reduction (p, 2^32 - 1) among them
    for count in FIELD_COUNTS:
        for lanes in (1, 64):
            words = [int(w) for w in rng.integers(0, 1 << 32, size=count)]
            if count >= 4:
                words[:4] = [0, P - 1, P, (1 << 32) - 1]
            m = start(pattern(7 if count < 126 else 0, count))
            fields(m, words, lanes)
            state_line(m)
            lines.append("point")
            m2 = Model(m.state)
            z = m2.squeeze(4)
            assert any(z[1:])
            m.state = m2.state
            want.append(("Z", z))
            state_line(m)
    m = start(pattern(241, 3))                       # 241 + 8 * 96 = 1009: the overflow the host cannot see
    fields(m, list(range(96)), 64)
    assert m.status == E_RANGE and len(m.state) == 241
    state_line(m)
    point(m)
    state_line(m)
    m = start(pattern(50, 4), status=9)              # a status already set: nothing moves
    fields(m, [1, 2, 3], 64)
    point(m)
    state_line(m)
    # the point rule: accepted at once, after 1, 3 and 7 rejections, and refused after 8
    for reject in (0, 1, 3, 7, 8, 11):
        m = start(pattern(40 + reject, 5))
        point(m, reject)
        state_line(m)
        lines.append("reject 0")
    # query rows
    for n, offsets, idx in ((1, [0], [0, 5, (1 << 32) - 1]), (1 << 32, [0, (1 << 32) - 1], [0, 1, (1 << 32) - 1, 12345]),
                            (1 << 14, [0, 4], [int(v) for v in rng.integers(0, 1 << 13, size=8)]),
                            (96, [0, 95, 1, 2, 3, 5, 8, 13], [0, 95, 96, 4000000000]), (1 << 20, [(1 << 20) - 1], [0, 1, (1 << 20) - 1])):
        lines.append(f"rows {n} {len(offsets)} " + " ".join(map(str, offsets)) + " : " + " ".join(map(str, idx)))
        want.append(("W", [(i + o) % n for i in idx for o in offsets]))
    return lines, want


def judge_transcript(stdout, want):
    got = stdout.split("\n")
    assert got[-2] == "DONE" and len(got) == len(want) + 2, (len(got), len(want))
    for n, (line, (kind, exp)) in enumerate(zip(got, want)):
        f = line.split()
        assert f[0] == kind, (n, line[:80])
        if kind == "T":
            length, status, raw = int(f[1]), int(f[2]), bytes.fromhex(f[3])
            assert (length, status) == (len(exp.state), exp.status), (n, length, status)
            assert len(raw) == CAPACITY and raw[:length] == exp.state, n
        else:
            assert [int(v) for v in f[1:]] == exp, (n, kind, line[:200])


def test_absorb_fields_point_rule_and_query_rows_match_hashlib_on_cpu():
    lines, want = transcript_script()
    judge_transcript(run(build_emu_dz(), "transcript", lines).stdout, want)
    kinds = [k for k, _ in want]
    assert kinds.count("Z") >= 2 * len(FIELD_COUNTS) + 8 and kinds.count("W") == 5
    refused = [exp for k, exp in want if k == "T" and exp.status == E_RANGE]
    assert len(refused) >= 4, "the overflow and the bound of 8 tries both end in the status"


def test_a_refused_field_absorb_leaves_every_byte_of_the_array_alone():
    lines = ["init " + pattern(241, 3).hex(), "state", "fields 64 " + " ".join(str(w) for w in range(96)), "state"]
    got = run(build_emu_dz(), "transcript", lines).stdout.split("\n")
    b, a = got[0].split(), got[1].split()
    assert b[1] == a[1] == "241" and (b[2], a[2]) == ("0", str(E_RANGE)) and b[3] == a[3]
