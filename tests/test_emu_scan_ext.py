"""Steps the bodies of the Ext accumulator-column kernels (include/toyni_hip.h 3i; ext_accum_* / ext_tower_inverses of
toyni_amd/csrc/prover_kernels.hpp) on the CPU under AddressSanitizer + UBSan, as a stand-alone program, and checks every printed word
against tests/ext_model.py in Python integers:
    term_i = num_i / den_i (0 where den_i = 0),  out[0] = init,  out[i] = out[i-1] (+ or *) term_{i-1},  total = out[n-1] (+ or *) term_{n-1}
On a reduced tile (groups of 4, two waves: 512 elements): n = 1, 2, 3, group - 1, group, group + 1, tile - 1, tile, tile + 1,
2 tile + 5 and more tiles than one round of step 2 takes; both ops; the eight (numerator width, denominator width) forms with non-zero
shifts; batch 1 and 3 with padded strides; values from {0, 1, p - 1, random}; in place on either width-4 operand; columns 0, 4, 8 and 12
bytes off 16-byte alignment; zero denominators at the first and the last slot of a group, at the first and the last element of a tile,
over a whole group and over a whole column; a width-1 denominator under a base-field shift (s, 0, 0, 0) with v = p - s, the only way
gamma + v = 0; denominators with one, two and three zero coordinates, whose norm must still be non-zero; the inversion alone.
CPU only; the shipped library contains none of tests/emu."""
import os
import subprocess

import ext_model as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = E.P
G, TILE = 4, 512


def build_emu_scan_ext() -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_scan_ext.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_scan_ext_asan")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-I", CSRC, "-o", out, src])
    return out


def _records():
    res = subprocess.run([build_emu_scan_ext()], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.split("\n")
    assert lines[-2] == "DONE" and lines[-3] == "BAD 0", lines[-3:]
    return [l.split() for l in lines[:-3]]


def operand(cols, width, shift, i):
    """Element i of an operand given its stored coordinate columns."""
    if width == 0:
        return E.ONE
    if width == 1:
        return E.add(E.embed(cols[0][i]), shift)
    return E.add(tuple(c[i] for c in cols), shift)


def model(op, n, num, nw, nshift, den, dw, dshift, init):
    """-> (out: list of Ext, total, zeros) in Python integers; the n inversions behind one (ext_model.batch_inverse)."""
    dens = [operand(den, dw, dshift, i) for i in range(n)]
    invs = E.batch_inverse(dens) if dw else [E.ONE] * n
    acc, out = tuple(init), []
    for i in range(n):
        out.append(acc)
        term = E.mul(operand(num, nw, nshift, i), invs[i])
        acc = E.mul(acc, term) if op else E.add(acc, term)
    return out, acc, sum(1 for d in dens if not any(d)), dens


def test_ext_scan_bodies_match_integer_arithmetic_on_cpu():
    recs = _records()
    k = 0
    seen = {"n": set(), "op": set(), "form": set(), "batch": set(), "inplace": set(), "off": set()}
    values = set()
    zero_first = zero_last = tile_first = tile_last = whole_group = whole_column = many_tiles = inverses = 0
    base_shift_zeros, partial = 0, {1: 0, 2: 0, 3: 0}
    assert E.inverse((3, 0, 5, 0)) == E.power((3, 0, 5, 0), P ** 4 - 2)
    while k < len(recs):
        r = recs[k]
        if r[0] == "SCAN":
            op, n, batch, nw, dw, inplace, off, ns, ds, os_ = map(int, r[1:])
            init = list(map(int, recs[k + 1][1:]))
            nshift, dshift = tuple(map(int, recs[k + 2][1:])), tuple(map(int, recs[k + 3][1:]))
            assert recs[k + 1][0] == "INIT" and len(init) == 4 * batch and recs[k + 2][0] == "NSHIFT" and recs[k + 3][0] == "DSHIFT"
            assert (not nw or all(nshift)) and (not dw or dshift[0])             # non-zero shifts
            assert batch == 1 or (ns > n and ds > n and os_ >= n)
            k += 4
            cols = []
            for b in range(batch):
                num, den = [], []
                for c in range(nw):
                    assert recs[k][:3] == ["NUM", str(b), str(c)] and len(recs[k]) == n + 3
                    num.append(list(map(int, recs[k][3:])))
                    k += 1
                for c in range(dw):
                    assert recs[k][:3] == ["DEN", str(b), str(c)] and len(recs[k]) == n + 3
                    den.append(list(map(int, recs[k][3:])))
                    k += 1
                cols.append((num, den))
            for b, (num, den) in enumerate(cols):
                got = []
                for c in range(4):
                    assert recs[k][:3] == ["OUT", str(b), str(c)] and len(recs[k]) == n + 3
                    got.append(list(map(int, recs[k][3:])))
                    k += 1
                assert recs[k][0] == "TOT" and int(recs[k][1]) == b and len(recs[k]) == 10
                tot = list(map(int, recs[k][2:]))
                k += 1
                want, total, zeros, dens = model(op, n, num, nw, nshift, den, dw, dshift, init[4 * b:4 * b + 4])
                for c in range(4):
                    assert got[c] == [w[c] for w in want], (op, n, batch, nw, dw, inplace, off, b, c,
                                                            next(i for i in range(n) if got[c][i] != want[i][c]))
                assert tot == list(total) + [zeros, 0, 0, 0], (op, n, batch, nw, dw, b)
                if n <= 3 * TILE:
                    for col in num + den:
                        values.update(col)
                if dw:
                    z = [i for i in range(n) if not any(dens[i])]
                    zero_first += any(i % G == 0 for i in z)
                    zero_last += any(i % G == G - 1 for i in z)
                    tile_first += any(i % TILE == 0 for i in z)
                    tile_last += any(i % TILE == TILE - 1 for i in z)
                    whole_group += any(all(not any(dens[i]) for i in range(g0, g0 + G)) for g0 in range(0, n - G + 1, G))
                    whole_column += len(z) == n and n > TILE
                    if dw == 1 and z:
                        assert dshift[1:] == (0, 0, 0) and all(den[0][i] == P - dshift[0] for i in z)
                        base_shift_zeros += 1
                    if dw == 4:
                        for d in dens:
                            nz = sum(1 for c in d if c == 0)
                            if 0 < nz < 4:
                                partial[nz] += 1
            many_tiles += n > TILE * TILE
            seen["n"].add(n), seen["op"].add(op), seen["form"].add((nw, dw)), seen["batch"].add(batch)
            seen["inplace"].add((inplace, nw if inplace == 1 else dw if inplace == 2 else 0)), seen["off"].add(off)
        else:
            assert r[0] == "BINV"
            count, off, inplace = map(int, r[1:])
            vin = [list(map(int, recs[k + 1 + c][3:])) for c in range(4)]
            vout = [list(map(int, recs[k + 5 + c][3:])) for c in range(4)]
            assert all(recs[k + 1 + c][:3] == ["IN", "0", str(c)] and recs[k + 5 + c][:3] == ["INV", "0", str(c)] for c in range(4))
            assert recs[k + 9][0] == "ZEROS" and all(len(v) == count for v in vin + vout)
            elems = [tuple(v[i] for v in vin) for i in range(count)]
            assert [tuple(v[i] for v in vout) for i in range(count)] == [E.inverse(e) if any(e) else E.ZERO for e in elems], (count, off)
            assert int(recs[k + 9][1]) == sum(1 for e in elems if not any(e))
            inverses += 1
            k += 10
    assert {1, 2, 3, G - 1, G, G + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 5} <= seen["n"] and many_tiles == 2
    assert seen["op"] == {0, 1} and seen["batch"] == {1, 3}
    assert seen["form"] == {(1, 1), (4, 4), (1, 4), (4, 1), (0, 1), (0, 4), (1, 0), (4, 0)}
    assert seen["inplace"] == {(0, 0), (1, 4), (2, 4)} and seen["off"] == {0, 1, 2, 3}
    assert {0, 1, P - 1} <= values and len(values) > 1000
    assert min(zero_first, zero_last, tile_first, tile_last, whole_group) > 10 and whole_column == 4
    assert base_shift_zeros > 10 and min(partial.values()) > 100
    assert inverses == 24
