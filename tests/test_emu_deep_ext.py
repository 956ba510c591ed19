"""Steps the bodies of the Ext DEEP combination and of the batched evaluation at Ext points (deep_combine_ext_group with
ext_shifted_inverses, poly_ext_*; toyni_amd/csrc/prover_kernels.hpp, include/toyni_hip.h 3h) on the CPU under AddressSanitizer + UBSan
and checks every printed word against tests/ext_model.py, which inverts by a^(p^4 - 2) as src/ext.rs does:
    d_i = sum_t alpha_t (M(column_t, (i + rotation_t B) mod N) - value_t) / (x_i - z)  in Ext,  0 where x_i = z
N in {1, 2, 4, 8, 64, 1024}, widths 1..9, 1..12 terms (every tail length of the four-term groups), rotations that wrap past N,
padded column strides, matrices 4 bytes off alignment, coordinates from {0, 1, p - 1, random}, z in the base field off and on the
coset (at the first and at the last point of a group), z with one, two and three non-zero upper coordinates.  The model itself is
pinned to the oracle first.  CPU only; the shipped library contains none of tests/emu."""
import os
import subprocess

import numpy as np

import ext_model as em
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = em.P


def test_the_model_is_the_oracles_ext():
    rng = np.random.default_rng(11)
    edge = [em.ZERO, em.ONE, (P - 1,) * 4, (0, 1, 0, 0), (0, 0, 0, P - 1)]
    elems = edge + [tuple(int(v) for v in rng.integers(0, P, 4)) for _ in range(20)]
    for e in elems:
        for beta in elems[::3]:
            want = oracle.fri_fold_ext(np.array([e, em.neg(e)], dtype=np.uint64), np.array([1], dtype=np.uint64), np.array(beta, dtype=np.uint64))
            assert tuple(int(v) for v in want[0]) == em.mul(e, beta), (e, beta)
            assert tuple(int(v) for v in em.vmul(np.array(e), np.array(beta))) == em.mul(e, beta)
    for a in elems[1:]:
        assert em.mul(a, em.inverse(a)) == em.ONE, a
    inv = em.batch_inverse(elems)
    assert inv[0] == em.ZERO and all(em.mul(a, b) == em.ONE for a, b in zip(elems[1:], inv[1:]))
    assert em.sub(em.add(elems[7], elems[8]), elems[8]) == elems[7] and em.add(elems[9], em.neg(elems[9])) == em.ZERO


def build_emu_deep_ext() -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_deep_ext.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_deep_ext_asan")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-I", CSRC, "-o", out, src])
    return out


def _records():
    res = subprocess.run([build_emu_deep_ext()], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.split("\n")
    assert lines[-2] == "DONE"
    return [l.split() for l in lines[:-2]]


def test_ext_deep_combination_and_ext_evaluation_bodies_match_the_model_on_cpu():
    recs = _records()
    k = 0
    seen_n, seen_w, seen_t, tails, upper = set(), set(), set(), set(), set()
    wrapped, padded, offset, on_coset, base_off_coset = 0, 0, 0, {"first": 0, "last": 0}, 0
    matrix_values, weights, claims = set(), set(), set()
    poly_shapes, long_second_stage = set(), 0
    while k < len(recs):
        r = recs[k]
        if r[0] == "DEEPX":
            n, log_b, shift, z0, z1, z2, z3, width, stride, nterms, off = map(int, r[1:])
            z = (z0, z1, z2, z3)
            terms = []
            for t in range(nterms):
                row = recs[k + 1 + t]
                assert row[0] == "TERM" and len(row) == 11
                v = list(map(int, row[1:]))
                terms.append((v[0], v[1], tuple(v[2:6]), tuple(v[6:10])))
            cols = []
            for c in range(width):
                row = recs[k + 1 + nterms + c]
                assert row[0] == "COL" and int(row[1]) == c and len(row) == n + 2
                cols.append(list(map(int, row[2:])))
            out_row = recs[k + 1 + nterms + width]
            assert out_row[0] == "OUT" and len(out_row) == 4 * n + 1
            out = np.array(list(map(int, out_row[1:])), dtype=np.uint32).reshape(n, 4)
            k += 2 + nterms + width
            b = 1 << log_b
            want = em.deep_ext_model(np.array(cols, dtype=np.uint64), terms, b, shift, z)
            bad = np.flatnonzero((out != want).any(axis=1))
            assert bad.size == 0, (n, log_b, width, nterms, z, bad[:8])
            nz_upper = sum(1 for v in z[1:] if v)
            upper.add(nz_upper)
            if nz_upper == 0:
                xs = em.coset_points(n, shift)
                if z0 in xs:
                    i = xs.index(z0)
                    assert not out[i].any()
                    if n >= 4:
                        on_coset["first" if i % 4 == 0 else "last"] += i % 4 in (0, 3)
                else:
                    base_off_coset += 1
            seen_n.add(n), seen_w.add(width), seen_t.add(nterms), tails.add(nterms % 4)
            wrapped += any((n - 1 + rot * b) >= n and rot for _, rot, _, _ in terms)
            padded += stride > n
            offset += off
            matrix_values.update(v for col in cols for v in col)
            for _, _, a, v in terms:
                weights.update(a), claims.update(v)
        else:
            assert r[0] == "POLYX"
            ncoeffs, stride, batch, npoints = map(int, r[1:5])
            pts = list(map(int, r[5:]))
            assert len(pts) == 4 * npoints and stride >= ncoeffs
            points = [tuple(pts[4 * p:4 * p + 4]) for p in range(npoints)]
            got_row = recs[k + 1 + batch]
            assert got_row[0] == "POUT" and len(got_row) == batch * npoints * 4 + 1
            got = np.array(list(map(int, got_row[1:])), dtype=np.uint32).reshape(batch, npoints, 4)
            columns = []
            for bb in range(batch):
                row = recs[k + 1 + bb]
                assert row[0] == "COEF" and int(row[1]) == bb and len(row) == ncoeffs + 2
                columns.append(list(map(int, row[2:])))
            want = em.poly_eval_ext_batch_model(columns, points)
            assert (got == want).all(), (ncoeffs, batch, npoints)
            k += 2 + batch
            poly_shapes.add((ncoeffs, batch, npoints))
            long_second_stage += ncoeffs > 4096 * 256
    assert seen_n == {1, 2, 4, 8, 64, 1024} and seen_w == set(range(1, 10)) and seen_t == set(range(1, 13)) and tails == {0, 1, 2, 3}
    assert upper == {0, 1, 2, 3}
    assert wrapped > 50 and padded > 50 and offset > 20 and on_coset["first"] > 10 and on_coset["last"] > 10 and base_off_coset > 10
    for s in (matrix_values, weights, claims):
        assert {0, 1, P - 1} <= s and len(s) > 20
    assert {nc for nc, _, _ in poly_shapes} >= {1, 15, 16, 17, 4095, 4096, 4097}
    assert {b for _, b, _ in poly_shapes} == {1, 2, 3} and {p for _, _, p in poly_shapes} == {1, 2, 3, 4}
    assert len(poly_shapes) == 23 and long_second_stage == 1
