"""Steps the bodies of the accumulator-column kernels (include/toyni_hip.h 3g; scan_* of toyni_amd/csrc/prover_kernels.hpp) on the CPU
under AddressSanitizer + UBSan -- workgroup by workgroup, wave by wave, the cross-lane steps lane by lane -- and checks every printed
word with Python integers:
    term_i = num_i / den_i (0 where den_i = 0),  out[0] = init,  out[i] = out[i-1] (+ or *) term_{i-1},  total = out[n-1] (+ or *) term_{n-1}
On a reduced tile (groups of 4, two waves: 512 elements): n = 1, 2, 3, group - 1, group, group + 1, tile - 1, tile, tile + 1,
2 tile + 5 and more tiles than one round of step 2 takes; both ops; each operand absent in turn; batch 1 and 3 with padded strides;
values from {0, 1, p - 1, random}; zero denominators at the first and the last slot of a group, at the first and the last element of a
tile, in every element of a group and in every element of a column; in place on either operand; columns 0, 4, 8 and 12 bytes off
16-byte alignment.  CPU only; the shipped library contains none of tests/emu."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = 2013265921
G, TILE = 4, 512


def build_emu_scan() -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_scan.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_scan_asan")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-I", CSRC, "-o", out, src])
    return out


def _records():
    res = subprocess.run([build_emu_scan()], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.split("\n")
    assert lines[-2] == "DONE" and lines[-3] == "BAD 0", lines[-3:]
    return [l.split() for l in lines[:-3]]


def model(op, num, den, init):
    """-> (out, total, zeros) in Python integers."""
    n = len(num if num is not None else den)
    acc, out, zeros = init, [], 0
    for i in range(n):
        out.append(acc)
        d = 1 if den is None else den[i]
        zeros += d == 0
        term = 0 if d == 0 else (1 if num is None else num[i]) * pow(d, -1, P) % P
        acc = (acc * term if op else acc + term) % P
    return out, acc, zeros


def test_scan_bodies_match_integer_arithmetic_on_cpu():
    recs = _records()
    k = 0
    seen = {"n": set(), "op": set(), "form": set(), "batch": set(), "inplace": set(), "off": set()}
    values, zero_first, zero_last, tile_first, tile_last, whole_group, whole_column, many_tiles, inverses = set(), 0, 0, 0, 0, 0, 0, 0, 0
    while k < len(recs):
        r = recs[k]
        if r[0] == "SCAN":
            op, n, batch, has_num, has_den, inplace, off, ns, ds, os_ = map(int, r[1:])
            init = list(map(int, recs[k + 1][1:]))
            assert recs[k + 1][0] == "INIT" and len(init) == batch
            assert batch == 1 or (ns >= n and ds >= n and os_ >= n and (ns > n or ds > n))
            k += 2
            cols = []
            for b in range(batch):
                num = den = None
                if has_num:
                    assert recs[k][0] == "NUM" and int(recs[k][1]) == b and len(recs[k]) == n + 2
                    num, k = list(map(int, recs[k][2:])), k + 1
                if has_den:
                    assert recs[k][0] == "DEN" and int(recs[k][1]) == b and len(recs[k]) == n + 2
                    den, k = list(map(int, recs[k][2:])), k + 1
                cols.append((num, den))
            for b, (num, den) in enumerate(cols):
                assert recs[k][0] == "OUT" and int(recs[k][1]) == b and len(recs[k]) == n + 2
                got = list(map(int, recs[k][2:]))
                assert recs[k + 1][0] == "TOT" and int(recs[k + 1][1]) == b
                got_total, got_zeros = int(recs[k + 1][2]), int(recs[k + 1][3])
                k += 2
                want, total, zeros = model(op, num, den, init[b])
                assert got == want, (op, n, batch, has_num, has_den, inplace, off, b, next(i for i in range(n) if got[i] != want[i]))
                assert (got_total, got_zeros) == (total, zeros), (op, n, batch, b)
                if n <= 3 * TILE:
                    values.update(num or []), values.update(den or [])
                if den is not None:
                    z = [i for i in range(n) if den[i] == 0]
                    zero_first += any(i % G == 0 for i in z)
                    zero_last += any(i % G == G - 1 for i in z)
                    tile_first += any(i % TILE == 0 for i in z)
                    tile_last += any(i % TILE == TILE - 1 for i in z)
                    whole_group += any(all(den[i] == 0 for i in range(g0, g0 + G)) for g0 in range(0, n - G + 1, G))
                    whole_column += len(z) == n and n > TILE
            many_tiles += n > TILE * TILE
            seen["n"].add(n), seen["op"].add(op), seen["form"].add((has_num, has_den)), seen["batch"].add(batch)
            seen["inplace"].add(inplace), seen["off"].add(off)
        else:
            assert r[0] == "BINV"
            count, off, inplace = map(int, r[1:])
            vin, vout = list(map(int, recs[k + 1][1:])), list(map(int, recs[k + 2][1:]))
            assert recs[k + 1][0] == "IN" and recs[k + 2][0] == "INV" and recs[k + 3][0] == "ZEROS" and len(vin) == len(vout) == count
            assert vout == [pow(v, -1, P) if v else 0 for v in vin], (count, off)
            assert int(recs[k + 3][1]) == vin.count(0)
            inverses += 1
            k += 4
    assert {1, 2, 3, G - 1, G, G + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 5} <= seen["n"] and many_tiles == 2
    assert seen["op"] == {0, 1} and seen["form"] == {(1, 1), (0, 1), (1, 0)} and seen["batch"] == {1, 3}
    assert seen["inplace"] == {0, 1, 2} and seen["off"] == {0, 1, 2, 3}
    assert {0, 1, P - 1} <= values and len(values) > 1000
    assert min(zero_first, zero_last, tile_first, tile_last, whole_group) > 10 and whole_column == 2
    assert inverses == 24
