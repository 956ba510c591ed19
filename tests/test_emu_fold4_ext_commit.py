"""Steps the per-thread text of the four-to-one Ext FRI round under coset leaves (include/toyni_hip.h 3m) on the CPU under
AddressSanitizer + UBSan: the leaf body fold4_ext_commit_leaf (what fri_fold4_ext_commit_kernel runs per leaf of the folded layer),
the two-factor record fri4_round_record, the coset leaf merkle_row_leaf_at<ROWS_EXT_QUARTERS> and the opening's gather
coset_value_word (tests/emu/emu_fold4_ext_commit.cpp, a stand-alone program).  The program restates the sweep's index arithmetic
on the host; the kernel's own indexing (fold4_ext_commit_sweep is device-only text) is held by tests/test_gpu_fold4_commit_ext.py.

Judges: the oracle's fri_fold_ext applied twice -- (beta, x0), then (beta^2, x0^2) with beta^2 from tests/ext_model.py -- for every
folded element; hashlib over the coset leaves tests/rows_common.py builds from a numpy gather for every digest of both trees; Python
integers for the record.  m = 16 (one leaf, which is the root), 64, 256; salted and unsalted; saturated data (every word p - 1,
beta = (p - 1, 0, 1, r), x0 = p - 1).  CPU only; the shipped library contains none of tests/emu."""
import os
import subprocess

import numpy as np

import ext_model as em
import oracle
import rows_common as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = 2013265921
R = (1 << 32) % P
INV2 = (P + 1) // 2


def build_emu_fold4(contracts_header=None) -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_fold4_ext_commit.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_fold4_ext_commit" + ("_contracts" if contracts_header else "_asan"))
    deps = [src, os.path.join(ROOT, "tests", "emu", "contract_case.hpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if contracts_header:
        deps.append(contracts_header)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        flags = ["-O2", "-include", contracts_header] if contracts_header else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "emu")] + flags + ["-o", out, src])
    return out


def coset_rows(layer):
    """(m, 4) -> (m / 4, 16): row j = elements j, j + m/4, j + m/2, j + 3m/4"""
    e = np.asarray(layer).reshape(-1, 4)
    m = e.shape[0]
    return np.ascontiguousarray(e.reshape(4, m // 4, 4).transpose(1, 0, 2)).reshape(m // 4, 16)


def coset_tree(layer, salts):
    """every level of the coset tree of a layer, hashlib only, as one hex string"""
    levels = rc.hashlib_levels(rc.leaves_of(coset_rows(np.asarray(layer, dtype=np.uint64)), salts))
    return b"".join(d for level in levels for d in level).hex()


def fold4_oracle(layer, x0, beta):
    """the oracle's pairwise fold twice: (beta, points x0 w_m^i), then (beta^2, points x0^2 w_(m/2)^i)"""
    e = np.asarray(layer, dtype=np.uint64).reshape(-1, 4)
    m = e.shape[0]
    beta2 = em.mul(tuple(beta), tuple(beta))
    first = oracle.fri_fold_ext(e, oracle.domain_elements(m, x0), np.array(beta, dtype=np.uint64))
    return oracle.fri_fold_ext(first, oracle.domain_elements(m // 2, x0 * x0 % P), np.array(beta2, dtype=np.uint64))


KEYS = ["CASE", "REC", "IN", "SALTS_IN", "SALTS_OUT", "OUT", "TREE_OUT", "TREE_IN", "GATHER"]


def judge(stdout):
    """Checks every block of the program's output; returns the list of (m, salted, x0, beta, layer words) it saw."""
    lines = stdout.split("\n")
    assert lines[-2] == "DONE" and lines[-1] == "" and (len(lines) - 2) % len(KEYS) == 0
    seen = []
    for at in range(0, len(lines) - 2, len(KEYS)):
        f = [l.split() for l in lines[at:at + len(KEYS)]]
        assert [x[0] for x in f] == KEYS, lines[at][:80]
        m, salted, x0 = int(f[0][1]), int(f[0][2]), int(f[0][3])
        beta = [int(v) for v in f[0][4:8]]
        tag = (m, salted, x0, beta)
        assert 0 < x0 < P and all(0 <= b < P for b in beta)
        # the record: Montgomery forms of beta / 2, 11 beta / 2, beta^2 / 2, 11 beta^2 / 2
        beta2 = em.mul(tuple(beta), tuple(beta))
        want_rec = [c * k * INV2 % P * R % P for src in (beta, beta2) for k in (1, 11) for c in src]
        assert [int(v) for v in f[1][1:]] == want_rec, tag
        layer = np.array([int(v) for v in f[2][1:]], dtype=np.uint64)
        assert layer.size == 4 * m and (layer < P).all()
        salts_in = np.frombuffer(bytes.fromhex(f[3][1]), dtype=np.uint8).reshape(m // 4, 16) if salted else None
        salts_out = np.frombuffer(bytes.fromhex(f[4][1]), dtype=np.uint8).reshape(m // 16, 16) if salted else None
        assert salted or (f[3][1] == "-" and f[4][1] == "-")
        # the folds
        want = fold4_oracle(layer, x0, beta)
        got = np.array([int(v) for v in f[5][1:]], dtype=np.uint64).reshape(m // 4, 4)
        assert (got == want).all(), tag
        # both trees, every level
        assert f[6][1] == coset_tree(want, salts_out), tag
        assert f[7][1] == coset_tree(layer, salts_in), tag
        assert len(f[6][1]) == 64 * sum(rc.level_sizes(m // 16)) and len(f[7][1]) == 64 * sum(rc.level_sizes(m // 4))
        # the gather of the open kernel: the rows the leaves were hashed from
        assert [int(v) for v in f[8][1:]] == coset_rows(layer).reshape(-1).tolist(), tag
        seen.append((m, salted, x0, beta, layer))
    return seen


def test_the_model_fold_is_the_cubic_through_the_coset():
    """What the two pairwise folds compute, stated independently: f0 + beta f1 + beta^2 f2 + beta^3 f3 at y = x^4 for the cubic
    f0(y) + x f1(y) + x^2 f2(y) + x^3 f3(y) -- a codeword of degree < 4 folds to the constant that combination names."""
    rng = np.random.default_rng(4)
    m, x0 = 16, 7
    coeffs = [tuple(int(v) for v in rng.integers(0, P, 4)) for _ in range(4)]
    beta = tuple(int(v) for v in rng.integers(0, P, 4))
    xs = [int(v) for v in oracle.domain_elements(m, x0)]
    layer = []
    for x in xs:
        acc = em.ZERO
        for c in reversed(coeffs):
            acc = em.add(tuple(a * x % P for a in acc), c)
        layer.append(acc)
    want, bk = em.ZERO, em.ONE
    for c in coeffs:
        want = em.add(want, em.mul(c, bk))
        bk = em.mul(bk, beta)
    got = fold4_oracle(np.array(layer, dtype=np.uint64), x0, beta)
    assert got.shape == (4, 4) and all(tuple(int(v) for v in row) == want for row in got)


def test_fold4_leaf_body_record_coset_leaf_and_gather_match_the_oracle_and_hashlib_on_cpu():
    res = subprocess.run([build_emu_fold4()], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    seen = judge(res.stdout)
    assert {(m, s) for m, s, _, _, _ in seen} == {(m, s) for m in (16, 64, 256) for s in (0, 1)}
    for m in (16, 64, 256):
        for salted in (0, 1):      # saturated data in both forms: every word p - 1, beta = (p - 1, 0, 1, r), x0 = p - 1
            assert any(mm == m and s == salted and x0 == P - 1 and b[:3] == [P - 1, 0, 1] and (layer == P - 1).all()
                       for mm, s, x0, b, layer in seen), (m, salted)
        assert any(mm == m and not any(b) for mm, _, _, b, _ in seen)             # beta = 0: a transcript whose status is set
        assert any(mm == m and b[0] and not any(b[1:]) for mm, _, _, b, _ in seen)  # beta embedded from the base field


def test_fold4_saturated_operands_on_cpu():
    res = subprocess.run([build_emu_fold4(), "saturated"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    seen = judge(res.stdout)
    assert len(seen) == 12 and all((layer == P - 1).all() for *_, layer in seen)
