"""seeds_launch_invariant (toyni_amd/csrc/ntt_route.hpp) -- the launcher's rule for "every workgroup of this column pass stays on one
column tile, look the twiddle seeds up once per launch" -- against a brute-force walk of every workgroup's tile sequence through
the kernels' own Pass::tile_order and Pass::tile_of (tests/cpp/seed_hoist_predicate.cpp): 1 to 1024 tiles per prefix, tile counts
that are multiples of 16 (paired tile order) and not, tile widths 8 to 64.  For grids of 1, 32, 48, 256, 304 and 512 workgroups the
predicate must equal the walk; for ten more grids it may only err towards the per-tile lookups.  CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")


def build_predicate_check() -> str:
    src = os.path.join(ROOT, "tests", "cpp", "seed_hoist_predicate.cpp")
    out = os.path.join(ROOT, "build", "seed_hoist_predicate")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-o", out, src])
    return out


def test_predicate_equals_the_walk_over_every_workgroups_tiles():
    res = subprocess.run([build_predicate_check()], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout[-3000:] + res.stderr[-1000:]
    m = re.search(r"checked (\d+) launches: predicate true for (\d+), conservative for (\d+)", res.stdout)
    assert m and int(m.group(1)) >= 5000 and 0 < int(m.group(2)) < int(m.group(1)), res.stdout[-500:]
