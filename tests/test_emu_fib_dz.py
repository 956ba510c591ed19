"""Steps the bodies of include/toyni_hip.h 3q (toyni_amd/csrc/fib_dz_kernels.hpp: the text the new kernels run) on the CPU under
AddressSanitizer + UBSan, as a stand-alone program (tests/emu/emu_fib_dz.cpp).

Two judges.  The program compares both records with memcmp against what the HOST code of toyni_poly_eval_device and
toyni_fib_deep_device builds for the reduced values, and the mask against the loop of csrc/host/fib_prover.hpp; this file recomputes
every printed word from Python integers, hashlib and the Python ChaCha20 of tests/harness/ref_prover.py.
  mask: n = 8, 128 (both overlap, n < 140), 140, 141, 256 with mask_degree 140 and 1, one thread per output word
  rejection rule: w_N^k and 7 w_N^k for k = 0, 1, N - 1 (rejected); 0, 1 + w_N, p - 1; log_N = 0 -- each judged by pow
  the loop: the states "toyni-stark-v1" || LE64(i), log_N = 27, shift = 7, where 2/15 of the field is rejected (p - 1 = 15 * 2^27 and 7
  lies outside the subgroup): i = 0 / 3 / 92 / 19 / 8065 / 19425 take exactly 0 / 1 / 2 / 3 / 4 / 5 rejections; the try limit
  records: z and the values among 0, p - 1, p, p + 1, 0xFFFFFFFF; the check word on a true tuple and with each value off by one
CPU only."""
import os
import subprocess
import sys

import numpy as np

from test_emu_transcript import CAPACITY, E_RANGE, Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = 2013265921
R = 1 << 32
MASK_SIZES = [8, 128, 140, 141, 256]
POINT_STATES = [(0, 0), (3, 1), (92, 2), (19, 3), (8065, 4), (19425, 5)]


def build_emu_fib_dz(contracts_header=None) -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_fib_dz.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_fib_dz" + ("_contracts" if contracts_header else "_asan"))
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


def root_of_unity(log_n):
    return pow(440564289, 1 << (27 - log_n), P)


def rejected(z, log_N, shift):
    return pow(z, 1 << log_N, P) == 1 or pow(z * pow(shift, P - 2, P) % P, 1 << log_N, P) == 1


# ---- the records ----
def judge_records(stdout, saturated):
    lines = stdout.split("\n")
    assert lines[-2] == "DONE" and lines[-3] == "BAD 0", lines[-3:]
    recs = [l.split() for l in lines[:-3]]
    assert not any(r[0] == "MISMATCH" for r in recs)
    k, zs, checks = 0, set(), []
    while k < len(recs):
        r = [int(v) for v in recs[k][1:]]
        if recs[k][0] == "POLY":
            z, mult = r
            point = z % P * mult % P
            assert recs[k + 1][0] == "PR" and [int(v) for v in recs[k + 1][1:]] == [point * R % P, pow(point, 16, P) * R % P, pow(point, 4096, P) * R % P], (z, mult)
            zs.add(z)
            k += 2
        elif recs[k][0] == "DEEP":
            assert recs[k + 1][0] == "DR" and [int(v) for v in recs[k + 1][1:]] == [r[0] % P * R % P] + [v % P for v in r[1:]], r
            zs.add(r[0])
            k += 2
        else:
            assert recs[k][0] == "CHECK"
            n, z, t_z, t_gz, t_ggz, q_z, got = r
            g = root_of_unity(n.bit_length() - 1)
            holds = (t_ggz - t_gz - t_z) * (z - pow(g, n - 1, P)) * (z - pow(g, (n - 2) % n, P)) % P == q_z * (pow(z, n, P) - 1) % P
            assert got == int(holds), r
            checks.append((n, got))
            k += 1
    if saturated:
        assert zs == {P - 1}
    else:
        assert {0, P - 1, P, P + 1, 0xFFFFFFFF} <= zs
        for n in (1, 2, 8, 64, 1 << 16):                     # per size: tuples that hold, and every value off by one refused
            got = [g for m, g in checks if m == n]
            assert got.count(1) >= 2 and got.count(0) == 4 * got.count(1), (n, got)


def test_records_match_the_host_code_and_python_integers():
    judge_records(run(build_emu_fib_dz(), "records").stdout, False)


def test_records_with_every_word_saturated():
    judge_records(run(build_emu_fib_dz(), "saturated").stdout, True)


# ---- the mask, the rule and the loop ----
def script():
    """(lines for the program, expected answers in order): ("M", words) | ("HOSTLOOP", [1]) | ("R", [0|1]) | ("Z", [z]) | ("T", Model)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from harness import ref_prover
    lines, want = [], []
    rng = np.random.default_rng(0xF1B)
    for n in MASK_SIZES:
        for d in (140, 1):
            key = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
            words = [int(v) for v in rng.integers(0, P, n)] + [0] * d + [0xFFFFFFF0, 0xFFFFFFF1]
            words[0] = P + 3                                 # a word the mask touches and has to reduce (T is canonical in a proof)
            if n > d + 2:
                words[d + 1] = P + 5                         # between the ranges: not touched, not reduced
            r = ref_prover.ChaChaRandomness(key).mask(d)
            out = list(words)
            for j in range(n + d):
                v = out[j]
                if j < d:
                    v = (v - r[j]) % P
                if n <= j < n + d:
                    v = (v + r[j - n]) % P
                out[j] = v
            lines.append(f"mask {n} {d} {key.hex()} : " + " ".join(map(str, words)))
            want += [("M", out), ("HOSTLOOP", [1])]
    # the rejection rule
    for log_N in (0, 1, 5, 27):
        N, w = 1 << log_N, root_of_unity(log_N)
        zs = [pow(w, k, P) for k in (0, 1, N - 1)] + [7 * pow(w, k, P) % P for k in (0, 1, N - 1)] + [0, (1 + w) % P, P - 1, 5, 123456789]
        for z in zs:
            lines.append(f"rule {z} {log_N} 7")
            want.append(("R", [int(rejected(z, log_N, 7))]))
        assert all(rejected(z, log_N, 7) for z in zs[:6])
    assert not rejected(0, 0, 7) and not rejected(P - 1, 0, 7) and rejected(P - 1, 1, 7)
    # the loop
    def point(m, log_N, shift, tries):
        lines.append(f"point {log_N} {shift} {tries}")
        if m.status:
            want.append(("Z", [0]))
            return None
        trial = Model(m.state)
        for k in range(tries):
            z = trial.squeeze(1)[0]
            if not rejected(z, log_N, shift):
                m.state = trial.state
                want.append(("Z", [z]))
                return k
        m.status = E_RANGE
        want.append(("Z", [0]))
        return tries

    def start(state, status=0):
        lines.append("init " + (state.hex() or "-"))
        if status:
            lines.append(f"status {status}")
        return Model(state, status)

    def state_line(m):
        lines.append("state")
        want.append(("T", Model(m.state, m.status)))

    for i, rejections in POINT_STATES:
        m = start(b"toyni-stark-v1" + i.to_bytes(8, "little"))
        assert point(m, 27, 7, 8) == rejections, i
        state_line(m)
        assert point(m, 27, 7, 8) is not None                # and on: the state is one digest now
        state_line(m)
    m = start(b"toyni-stark-v1" + (3).to_bytes(8, "little"))   # one rejection, a limit of one try: zero, the state as it was, the status
    assert point(m, 27, 7, 1) == 1 and m.status == E_RANGE and len(m.state) == 22
    state_line(m)
    point(m, 27, 7, 8)                                       # sticky: zero again
    state_line(m)
    m = start(b"toyni-stark-v1" + (19425).to_bytes(8, "little"))
    assert point(m, 27, 7, 5) == 5 and m.status == E_RANGE   # five rejections: a limit of five is one short
    state_line(m)
    m = start(b"abc", status=9)
    point(m, 3, 7, 8)
    state_line(m)
    return lines, want


def test_mask_rule_and_point_loop_match_python_on_cpu():
    lines, want = script()
    got = run(build_emu_fib_dz(), "script", lines).stdout.split("\n")
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
    kinds = [k for k, _ in want]
    assert kinds.count("M") == 2 * len(MASK_SIZES) and kinds.count("R") == 44
