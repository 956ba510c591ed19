"""The persistent tile loop of the two-step column passes with launch-invariant twiddle seeds, stepped on the CPU against the oracle
(tests/emu/emu_seed_hoist.cpp): grids of 2 and 32 workgroups (and a third where neither makes a workgroup walk several tiles on
one column tile) over 4 x 2^20 forward and inverse (the inverse carries n^-1 on the hoisted seed), 4 / 5 / 8 x 2^16 on 64-wide
256-point tiles, a forward coset transform at 2^16, Ext vectors at 2^16, and 16 x 2^20 on the benchmark's 32-wide 1024-point shape.
The launcher's predicate decides per launch, as on the device, whether a workgroup's first tile seeds all its tiles; every word is
compared with the oracle, and both forms of the loop must have run over several tiles per workgroup.  Once plain, once as a
stand-alone program under AddressSanitizer + UBSan (without the 16 x 2^20 case).  CPU only; the shipped library contains none of this."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "emu", "build")


def _build(sanitized: bool) -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_seed_hoist.cpp")
    orc = os.path.join(ROOT, "oracle", "toyni_oracle.c")
    out = os.path.join(BUILD, "emu_seed_hoist_asan" if sanitized else "emu_seed_hoist")
    obj = os.path.join(BUILD, "emu_seed_hoist_oracle.o")
    deps = [src, orc] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["gcc", "-O2", "-c", "-o", obj, orc])
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else ["-O2"]
        subprocess.check_call(["g++", *flags, "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-o", out, src, obj])
    return out


def _run(exe, *args):
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
    m = re.search(r"hoisted over several tiles (\d+), hoisted one tile per workgroup (\d+), per-tile seeds over several tiles (\d+)", res.stdout)
    assert m and int(m.group(1)) > 0 and int(m.group(3)) > 0, res.stdout[-500:]
    return res.stdout


def test_hoisted_seed_loop_matches_oracle_on_cpu():
    out = _run(_build(False))
    # the benchmark's shape: 32-wide 1024-point tiles, sixteen per workgroup on one column tile
    assert re.search(r"LAUNCH 16x2\^20 forward pass=0 lm=10 c=32 lq=0 grid=32 tiles=512 invariant=1 tiles_per_wg=16", out), out[-2000:]
    for case in ("4x2^20 forward", "4x2^20 inverse", "5x2^16 64-wide", "8x2^16 forward coset", "2x2^16 Ext"):
        assert re.search(r"LAUNCH " + re.escape(case) + r" pass=0 .* invariant=1 tiles_per_wg=([2-9]|\d\d)", out), case


def test_hoisted_seed_loop_is_memory_safe_under_asan_ubsan():
    _run(_build(True), "light")
