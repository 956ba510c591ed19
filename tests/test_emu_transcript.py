"""Steps the device transcript (toyni_amd/csrc/transcript_kernels.hpp: the text the one-wave kernels of include/toyni_hip.h 3l run) on
the CPU under AddressSanitizer + UBSan, as a stand-alone program (tests/emu/emu_transcript.cpp), and judges every line it prints
against hashlib: the model below is src/transcript.rs with a 1008-byte state and a sticky status word.

Cases: a state at every padding edge of SHA-256 (0, 1, 31, 32, 55, 56, 63, 64, 119, 120, 976, 1008 bytes), each followed by a
32-byte absorb and a squeeze; the two overflows (977 + 32, 1008 + 1: status set, every byte unchanged); an Ext squeeze; the index
squeezes (44, 2^11), (8, 8), (256, 256) -- which force many repeats -- and (1, 1); status stickiness; the u64 reduction at its edges;
the query positions against the numpy expression of tests/harness/fib_prover.py.  CPU only."""
import hashlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = 2013265921
CAPACITY = 1008
E_RANGE = 10006
EDGES = [0, 1, 31, 32, 55, 56, 63, 64, 119, 120, 976, 1008]
INDEX_CASES = [(44, 1 << 11), (8, 8), (256, 256), (1, 1)]
REDUCE = sorted({0, P - 1, P, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1} |
                {k * P + d for k in (1, 2, 3, 2 ** 31, 2 ** 33 - 1, (2 ** 64 - 1) // P) for d in (-1, 1) if 0 <= k * P + d < 2 ** 64})


class Model:
    """src/transcript.rs:12-72 behind the capacity and the status word of include/toyni_hip.h 3l"""

    def __init__(self, state=b"", status=0):
        self.state, self.status = bytes(state), status

    def absorb(self, data):
        if self.status:
            return
        if len(self.state) + len(data) > CAPACITY:
            self.status = E_RANGE
            return
        self.state += data

    def squeeze(self, count):
        if self.status:
            return [0] * count
        out = []
        for _ in range(count):
            self.state = hashlib.sha256(self.state).digest()
            out.append(int.from_bytes(self.state[:8], "little") % P)
        return out

    def squeeze_indices(self, count, mx):
        if self.status:
            return [0] * count
        out, state = [], self.state
        for _ in range(64 * count + 64):
            state = hashlib.sha256(state).digest()
            idx = int.from_bytes(state[:8], "little") % mx
            if idx not in out:
                out.append(idx)
                if len(out) == count:
                    self.state = state
                    return out
        self.status = E_RANGE
        return [0] * count


def pattern(n, seed):
    return bytes((seed * 131 + 7 * i + (i >> 8)) & 0xFF for i in range(n))


def query_positions(indices, m0, final_size):
    """step 7 of tests/harness/fib_prover.py: per layer the pairs [i mod half, i mod half + half], the final layer excluded"""
    out, cur, m = [], np.asarray(indices, dtype=np.int64), m0
    while m > final_size:
        half = m // 2
        cur = cur % half
        out.append(np.stack([cur, cur + half], axis=1).reshape(-1))
        m //= 2
    return np.concatenate(out).tolist() if out else []


def script():
    """(lines for the program, expected answers in order)"""
    lines, want = [], []

    def state_line(m):
        lines.append("state")
        want.append(("T", Model(m.state, m.status)))

    def start(state, status=0):
        m = Model(state, status)
        lines.append("init " + (state.hex() or "-"))
        if status:
            lines.append(f"status {status}")
        return m

    def absorb(m, data):
        before = (m.state, m.status)
        m.absorb(data)
        lines.append("absorb " + (data.hex() or "-"))
        return before

    def squeeze(m, count):
        lines.append(f"squeeze {count}")
        want.append(("S", m.squeeze(count)))

    def indices(m, count, mx):
        lines.append(f"indices {count} {mx}")
        want.append(("I", m.squeeze_indices(count, mx)))

    for n in EDGES:                                    # every padding edge, squeezed as it lies ...
        m = start(pattern(n, n))
        squeeze(m, 1)
        state_line(m)
        m = start(pattern(n, n + 1))                   # ... and after a 32-byte absorb (which 1008 and 977.. cannot take)
        absorb(m, pattern(32, 99))
        state_line(m)
        squeeze(m, 2)
        state_line(m)
    for n, extra in ((977, 32), (1008, 1)):            # the overflows: status set, the bytes unchanged, zeros from then on
        m = start(pattern(n, 5))
        absorb(m, pattern(extra, 6))
        assert m.status == E_RANGE and len(m.state) == n
        state_line(m)
        squeeze(m, 4)
        indices(m, 3, 16)
        absorb(m, b"\x01")
        state_line(m)
    m = start(b"toyni-stark-v1")                       # the reference's start, an Ext challenge, roots, indices
    squeeze(m, 4)
    absorb(m, pattern(32, 1))
    squeeze(m, 1)
    absorb(m, pattern(32, 2))
    absorb(m, pattern(8, 3))
    state_line(m)
    for count, mx in INDEX_CASES:
        indices(m, count, mx)
        state_line(m)
    m = start(pattern(40, 8))                          # an index squeeze straight from a long state
    indices(m, 44, 1 << 11)
    state_line(m)
    m = start(pattern(64, 9), status=7)                # any status is sticky: nothing moves, zeros come out
    absorb(m, pattern(4, 1))
    squeeze(m, 2)
    indices(m, 2, 5)
    state_line(m)
    m = start(pattern(10, 4))                          # squeeze 0: nothing happens
    squeeze(m, 0)
    state_line(m)
    for x in REDUCE:
        lines.append(f"reduce {x}")
        want.append(("R", [x % P]))
    rng = np.random.default_rng(0x7A)
    for count, m0, fin in ((44, 1 << 11, 1), (8, 1 << 8, 4), (1, 2, 1), (5, 1 << 4, 1 << 4), (3, 1 << 20, 1 << 19)):
        idx = rng.integers(0, max(m0 // 2, 1), size=count).tolist()
        lines.append(f"positions {m0} {fin} " + " ".join(str(i) for i in idx))
        want.append(("P", query_positions(idx, m0, fin)))
    return lines, want


def build_emu_transcript(contracts_header=None) -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_transcript.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_transcript" + ("_contracts" if contracts_header else "_asan"))
    deps = [src, os.path.join(ROOT, "tests", "emu", "contract_case.hpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if contracts_header:
        deps.append(contracts_header)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = ["-O2", "-include", contracts_header] if contracts_header else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "emu")] + flags + ["-o", out, src])
    return out


def judge(stdout, want):
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


def run(program, lines, *args):
    res = subprocess.run([program, *args], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return res


def test_the_model_is_the_reference_transcript():
    # the harness's Transcript (held to the reference prover by the harness's own tests) and the model above agree where neither
    # meets the capacity
    from harness.fib_prover import Transcript
    t, m = Transcript(), Model(b"toyni-stark-v1")
    t.absorb(pattern(32, 1)), m.absorb(pattern(32, 1))
    assert [t.squeeze_challenge() for _ in range(3)] == m.squeeze(3)
    t.absorb(pattern(40, 2)), m.absorb(pattern(40, 2))
    assert t.squeeze_indices(44, 1 << 11) == m.squeeze_indices(44, 1 << 11) and t.state == m.state
    assert t.squeeze_indices(8, 8) == m.squeeze_indices(8, 8) and t.state == m.state


def test_transcript_functions_match_hashlib_on_cpu():
    lines, want = script()
    judge(run(build_emu_transcript(), lines).stdout, want)
    judge(run(build_emu_transcript(), lines, "wave").stdout, want)      # the lane-spread form of absorb
    kinds = [k for k, _ in want]
    assert kinds.count("S") >= 2 * len(EDGES) and kinds.count("I") >= len(INDEX_CASES) + 3 and kinds.count("R") == len(REDUCE)


def test_overflow_leaves_every_byte_of_the_array_alone():
    # judge() compares the live prefix; here the WHOLE array, stale bytes included, before and after the refused absorb
    lines = []
    for n, extra in ((977, 32), (1008, 1)):
        lines += ["init " + pattern(n, 5).hex(), "state", "absorb " + pattern(extra, 6).hex(), "state"]
    got = run(build_emu_transcript(), lines).stdout.split("\n")
    for before, after in ((got[0], got[1]), (got[2], got[3])):
        b, a = before.split(), after.split()
        assert b[3] == a[3] and b[1] == a[1] and (int(b[2]), int(a[2])) == (0, E_RANGE)
