"""Steps the bodies of the DEEP combination and of the batched polynomial evaluation (deep_combine_group, poly_batch_*,
toyni_amd/csrc/prover_kernels.hpp) on the CPU under AddressSanitizer + UBSan and checks every printed word with Python integers:
    d_i = sum_t alpha_t (M(column_t, (i + rotation_t B) mod N) - value_t) / (x_i - z),  0 where x_i = z
N in {1, 2, 4, 8, 64, 1024}, widths 1..9, 1..12 terms (every tail length of the four-term groups), rotations that wrap past N,
padded column strides, matrices 4 bytes off alignment, values / weights / claims from {0, 1, p - 1, random}, z on the coset at the
first and at the last point of a group.  CPU only; the shipped library contains none of tests/emu."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = 2013265921
GEN_2_27 = 440564289


def build_emu_deep() -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_deep.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_deep_asan")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-I", CSRC, "-o", out, src])
    return out


def _records():
    res = subprocess.run([build_emu_deep()], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.split("\n")
    assert lines[-2] == "DONE"
    return [l.split() for l in lines[:-2]]


def test_deep_combination_and_batched_evaluation_bodies_match_integer_arithmetic_on_cpu():
    recs = _records()
    k = 0
    seen_n, seen_w, seen_t, wrapped, padded, offset, on_coset, tails = set(), set(), set(), 0, 0, 0, {"first": 0, "last": 0}, set()
    matrix_values, weights, claims = set(), set(), set()
    poly_cases = 0
    while k < len(recs):
        r = recs[k]
        if r[0] == "DEEP":
            n, log_b, shift, z, width, stride, nterms, off = map(int, r[1:])
            terms = [tuple(map(int, recs[k + 1 + t][1:])) for t in range(nterms)]
            assert all(recs[k + 1 + t][0] == "TERM" for t in range(nterms))
            cols = []
            for c in range(width):
                row = recs[k + 1 + nterms + c]
                assert row[0] == "COL" and int(row[1]) == c and len(row) == n + 2
                cols.append(list(map(int, row[2:])))
            out_row = recs[k + 1 + nterms + width]
            assert out_row[0] == "OUT" and len(out_row) == n + 1
            out = list(map(int, out_row[1:]))
            k += 2 + nterms + width
            b = 1 << log_b
            w_n = pow(GEN_2_27, (1 << 27) // n, P)
            x = shift
            zeros = 0
            for i in range(n):
                num = sum(a * (cols[c][(i + rot * b) % n] - v) for c, rot, a, v in terms) % P
                if x == z:
                    want, zeros = 0, zeros + 1
                    on_coset["first" if i % 8 == 0 else "last"] += (n >= 8 and i % 8 in (0, 7))
                else:
                    want = num * pow(x - z, -1, P) % P
                assert out[i] == want, (n, log_b, width, nterms, i)
                x = x * w_n % P
            assert zeros <= 1
            seen_n.add(n), seen_w.add(width), seen_t.add(nterms), tails.add(nterms % 4)
            wrapped += any((n - 1 + rot * b) >= n and rot for _, rot, _, _ in terms)
            padded += stride > n
            offset += off
            matrix_values.update(v for col in cols for v in col)
            weights.update(a for _, _, a, _ in terms), claims.update(v for _, _, _, v in terms)
        else:
            assert r[0] == "POLY"
            ncoeffs, stride, batch, npoints = map(int, r[1:5])
            points = list(map(int, r[5:]))
            assert len(points) == npoints and stride >= ncoeffs
            got = list(map(int, recs[k + 1 + batch][1:]))
            assert recs[k + 1 + batch][0] == "POUT" and len(got) == batch * npoints
            for bb in range(batch):
                row = recs[k + 1 + bb]
                assert row[0] == "COEF" and int(row[1]) == bb and len(row) == ncoeffs + 2
                coeffs = list(map(int, row[2:]))
                for p, pt in enumerate(points):
                    acc = 0
                    for c in reversed(coeffs):
                        acc = (acc * pt + c) % P
                    assert got[bb * npoints + p] == acc, (ncoeffs, batch, bb, p)
            k += 2 + batch
            poly_cases += 1
    assert seen_n == {1, 2, 4, 8, 64, 1024} and seen_w == set(range(1, 10)) and seen_t == set(range(1, 13)) and tails == {0, 1, 2, 3}
    assert wrapped > 50 and padded > 50 and offset > 20 and on_coset["first"] > 10 and on_coset["last"] > 10
    for s in (matrix_values, weights, claims):
        assert {0, 1, P - 1} <= s and len(s) > 20
    assert poly_cases == 17
