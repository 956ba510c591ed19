"""Steps the proof-of-work bodies (toyni_amd/csrc/pow_kernels.hpp: the text the three kernels of a grind chain run, include/toyni_hip.h
3n) on the CPU under AddressSanitizer + UBSan, as a stand-alone program (tests/emu/emu_pow.cpp), and judges every line it prints
against tests/pow_model.py -- hashlib alone.

What is stepped: the midstate (against a SHA-256 compression written out below: hashlib does not show its state); the candidate
digest in its one-block and two-block form, over every state length of the checked table -- 47 | 48 is where the second block
begins, 0, 14, 55, 63 and 119 put the nonce across three message words -- and over nonces whose 8 bytes all differ; the acceptance
test at bits 0, 1, 7, 8, 9, 31, 32; the host check; the two ends of a chain, with the lengths 1001..1008 that cannot take a nonce and
a transcript whose status is set; the candidate whose value is the armed word itself (2^64 - 1); and a serial run of the search body
over every table case with bits <= 12.  CPU only."""
import hashlib
import os
import subprocess
from functools import lru_cache

import pow_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
NONE = (1 << 64) - 1
BITS_EDGES = [0, 1, 7, 8, 9, 31, 32]
NONCES = [0, 1, 0x0807060504030201, 0xF1E2D3C4B5A69788, (1 << 32) - 1, 1 << 32, NONE]

_K = [int(x, 16) for x in """428a2f98 71374491 b5c0fbcf e9b5dba5 3956c25b 59f111f1 923f82a4 ab1c5ed5 d807aa98 12835b01 243185be 550c7dc3 72be5d74
80deb1fe 9bdc06a7 c19bf174 e49b69c1 efbe4786 0fc19dc6 240ca1cc 2de92c6f 4a7484aa 5cb0a9dc 76f988da 983e5152 a831c66d b00327c8 bf597fc7 c6e00bf3
d5a79147 06ca6351 14292967 27b70a85 2e1b2138 4d2c6dfc 53380d13 650a7354 766a0abb 81c2c92e 92722c85 a2bfe8a1 a81a664b c24b8b70 c76c51a3 d192e819
d6990624 f40e3585 106aa070 19a4c116 1e376c08 2748774c 34b0bcb5 391c0cb3 4ed8aa4a 5b9cca4f 682e6ff3 748f82ee 78a5636f 84c87814 8cc70208 90befffa
a4506ceb bef9a3f7 c67178f2""".split()]
_IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def _compress(h, block):
    """FIPS 180-4, one block"""
    m, rotr = 0xFFFFFFFF, lambda x, n: ((x >> n) | (x << (32 - n))) & 0xFFFFFFFF
    w = [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(16)]
    for i in range(16, 64):
        s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & m)
    a, b, c, d, e, f, g, hh = h
    for i in range(64):
        t1 = (hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g & m)) + _K[i] + w[i]) & m
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & m
        hh, g, f, e, d, c, b, a = g, f, e, (d + t1) & m, c, b, a, (t1 + t2) & m
    return [(x + y) & m for x, y in zip(h, [a, b, c, d, e, f, g, hh])]


def midstate(state):
    h = list(_IV)
    for b in range(len(state) // 64):
        h = _compress(h, state[64 * b:64 * b + 64])
    return h


def test_the_written_out_compression_is_sha256():
    # one padded block by hand against hashlib: the midstate check below rests on this function
    msg = pm.pattern(55, 3)
    block = msg + b"\x80" + (8 * len(msg)).to_bytes(8, "big")
    assert b"".join(x.to_bytes(4, "big") for x in _compress(list(_IV), block)) == hashlib.sha256(msg).digest()


def build_emu_pow() -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_pow.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_pow_asan")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", out, src])
    return out


def run(lines):
    res = subprocess.run([build_emu_pow()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    got = res.stdout.split("\n")
    assert got[-2] == "DONE", got[-3:]
    return got[:-2]


def init(state):
    return "init " + (state.hex() or "-")


def parse_state(line):
    f = line.split()
    assert f[0] == "T"
    return int(f[1]), int(f[2]), bytes.fromhex(f[3])


@lru_cache(maxsize=None)
def states():
    return pm.table_states() + [("n=14+50", pm.pattern(64, 3))]


def test_midstate_and_candidate_digests_in_both_forms():
    lines, want = [], []
    for name, s in states():
        lines += [init(s), "mid"]
        want.append("M %d %s" % (len(s) // 64, " ".join(str(x) for x in midstate(s))))
        for nonce in NONCES:
            lines.append(f"digest {nonce}")
            form = 2 if len(s) % 64 + 8 + 9 > 64 else 1
            want.append("D %d %s" % (form, hashlib.sha256(s + pm.le64(nonce)).hexdigest()))
    got = run(lines)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    forms = {len(s): w.split()[1] for (_, s), w in zip(states(), [w for w in want if w[0] == "D"][::len(NONCES)])}
    assert forms[47] == "1" and forms[48] == "2" and forms[63] == "2" and forms[64] == "1" and forms[1000] == "1"


def test_acceptance_at_the_bit_edges():
    words = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x01000000, 0x00FFFFFF, 0x00800000, 0x007FFFFF, 0x02000000, 0x01FFFFFF, 2, 3]
    lines = [f"accept {h0} {bits}" for h0 in words for bits in BITS_EDGES]
    want = ["A %d" % (bits == 0 or h0 >> (32 - bits) == 0) for h0 in words for bits in BITS_EDGES]
    assert run(lines) == want
    assert "A 1" in want and "A 0" in want


def test_the_host_check_is_the_models_accept():
    lines, want = [], []
    for name, s in states():
        lines.append(init(s))
        for bits in (1, 8, 12):
            hit = pm.must_grind(s, bits)
            for nonce in sorted({hit, hit + 1, max(hit - 1, 0)}):
                for b in sorted({bits, bits - 1, min(bits + 1, 32)}):
                    lines.append(f"check {nonce} {b}")
                    want.append("C %d" % pm.accept(s, nonce, b))
        for bits in BITS_EDGES:
            lines.append(f"check {NONE} {bits}")
            want.append("C %d" % pm.accept(s, NONE, bits))
    assert run(lines) == want
    assert want.count("C 0") > 20 and want.count("C 1") > 20


def test_serial_search_gives_the_models_minimum_and_absorbs_it():
    lines, want = [], []
    cases = [(s, bits, 0, 1 << 16) for _, s in states() for bits in (0, 1, 8, 12)]
    s3 = pm.pattern(64, 3)
    cases += [(s3, 8, (1 << 32) - 100, 1 << 12), (s3, 12, (1 << 32) - 100, 1 << 12)]           # the answers lie beyond 2^32
    hit = pm.must_grind(pm.START_STATE, 8)
    cases += [(pm.START_STATE, 8, hit, 1 << 12), (pm.START_STATE, 8, hit + 1, 1 << 12)]        # at a hit, and just past it
    cases += [(pm.pattern(64, 9), 32, 0, 1 << 10), (pm.pattern(64, 9), 24, 0, 1 << 12)]        # windows without a hit
    cases += [(pm.pattern(32, 1), 0, (1 << 64) - 4, 4), (pm.pattern(32, 1), 0, NONE, 1)]       # the top of the range
    for s, bits, start, tries in cases:
        m = pm.Transcript(s)
        nonce = m.grind(bits, start, tries)
        lines += [init(s), f"search {bits} {start} {tries}", "state"]
        want.append((nonce, m))
    got = run(lines)
    assert len(got) == 2 * len(want)
    for k, (nonce, m) in enumerate(want):
        assert got[2 * k] == f"N {nonce}", (k, got[2 * k], nonce)
        length, status, raw = parse_state(got[2 * k + 1])
        assert (length, status) == (len(m.state), m.status) and raw[:length] == m.state, k
        if m.status:
            assert nonce == 0 and status == pm.E_RANGE and raw[length:] == b"\xA5" * (pm.CAPACITY - length)
    assert sum(1 for _, m in want if m.status) == 2
    s3_hits = [n for (s, b, st, _), (n, _) in zip(cases, want) if st == (1 << 32) - 100]
    assert s3_hits == [(1 << 32) - 100 + 232, (1 << 32) - 100 + 3345]


def test_the_ends_of_a_chain_refuse_what_cannot_take_a_nonce():
    lines, want = [], []
    for n in list(range(1001, 1009)) + [1000]:                     # 1001..1008 + 8 bytes pass the capacity; 1000 just fits
        s = pm.pattern(n, 5)
        lines += [init(s), "nonce 77", "arm", "state", "finish 0 0", "state"]
        want.append((s, 0 if n > 1000 else NONE, pm.E_RANGE if n > 1000 else 0))
    got = run(lines)
    for k, (s, armed, status) in enumerate(want):
        a, t1, f, t2 = got[4 * k:4 * k + 4]
        assert a == f"N {armed}"
        assert parse_state(t1) == (len(s), status, s + b"\xA5" * (pm.CAPACITY - len(s)))
        # finish: a set status leaves everything alone; an armed word that nothing lowered is "no hit"
        assert f == "N 0" and parse_state(t2) == (len(s), pm.E_RANGE, s + b"\xA5" * (pm.CAPACITY - len(s)))
    # a status set by anyone is sticky: nothing moves, zero comes out
    s = pm.pattern(64, 9)
    got = run([init(s), "status 7", "nonce 5", "arm", "state", "search 0 0 16", "state", "nonce 9", "finish 0 1", "state"])
    assert got[0] == "N 0" and got[2] == "N 0" and got[4] == "N 0"
    for t in (got[1], got[3], got[5]):
        assert parse_state(t) == (64, 7, s + b"\xA5" * (pm.CAPACITY - 64))


def test_finish_absorbs_a_hit_and_tests_the_candidate_that_equals_the_armed_word():
    s = pm.pattern(47, 47)
    got = run([init(s), "nonce 855", "finish 12 0", "state"])
    assert got[0] == "N 855" and parse_state(got[1])[:2] == (55, 0) and parse_state(got[1])[2][:55] == s + pm.le64(855)
    # nothing lowered the word and the window reaches 2^64 - 1: that candidate is judged here, by one hash
    for name, s in states():
        for bits in (0, 1, 2):
            m = pm.Transcript(s)
            ok = pm.accept(s, NONE, bits)
            got = run([init(s), f"nonce {NONE}", f"finish {bits} 1", "state", init(s), f"nonce {NONE}", f"finish {bits} 0", "state"])
            length, status, raw = parse_state(got[1])
            if ok:
                assert got[0] == f"N {NONE}" and (length, status) == (len(s) + 8, 0) and raw[:length] == s + b"\xFF" * 8
            else:
                assert got[0] == "N 0" and (length, status) == (len(s), pm.E_RANGE) and raw[:length] == s
            assert got[2] == "N 0" and parse_state(got[3])[:2] == (len(s), pm.E_RANGE)         # not in the window: no hit


def test_the_grid_is_small_for_few_bits_and_fills_the_chip_for_many():
    cases = [(b, t) for b in range(0, 33) for t in (0, 1, 8, 9, 12, 20, 32, 40)]
    got = run([f"grid {b} {t}" for b, t in cases])
    for (b, t), g in zip(cases, got):
        blocks = int(g.split()[1])
        assert 1 <= blocks <= 768 and (blocks <= 256 or blocks % 256 == 0)
        assert blocks * 256 <= max(256, min(1 << t, 1 << (b + 2)))
        if b <= 12:
            assert blocks * 256 <= 1 << 14                          # not half a million candidates for a dozen bits
        if b >= 16 and t >= 18:
            assert blocks == 768                                    # three workgroups on each of 256 CUs: the chip is full
