"""The launch route of every transform call (toyni_amd/csrc/ntt_route.hpp: route_transform) and the pass shapes it dispatches to,
table-checked on the CPU: tests/cpp/route_table.cpp prints one line per knob profile and grid point, tests/golden/route_table.txt
holds the same lines as the commit BEFORE the route became one function computed them (see the fixture's header).  The grid holds
the points where a decision flips: every size at batch 1 and 3, the row sweeps' and the LDS sweep's thresholds, 2^21 / 2^22 either
side of the latency / streaming gates, Ext vectors, blow-ups up to and one beyond the first pass, chunked contexts, the
non-temporal boundary.  A new shape or threshold is one edit in the header and a visible diff in the fixture."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "route_table.txt")


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(ROOT, "build", "route_table")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "toyni_amd", "csrc"), "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "route_table.cpp")])
    return out


def _run(exe, knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith("TOYNI_")}
    env.update(knobs)
    return subprocess.run([exe], env=env, capture_output=True, text=True, check=True, timeout=300).stdout


def _blocks(text):
    blocks, name = {}, None
    for line in text.splitlines():
        if line.startswith("## "):
            name = line[3:]
            blocks[name] = []
        else:
            blocks[name].append(line)
    return blocks


def test_routes_and_pass_shapes_equal_the_parent_commits(exe):
    with open(FIXTURE) as f:
        want = "".join(line for line in f if not line.startswith("# "))
    got = _run(exe, {})
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        diff = [f"line {i + 1}:\n  got  {a}\n  want {b}" for i, (a, b) in enumerate(zip(g, w)) if a != b][:10]
        pytest.fail(f"{len(g)} lines against {len(w)} in the fixture; first differences:\n" + "\n".join(diff))


def test_the_environment_reaches_the_knobs(exe):
    """`default` is the only block whose knobs come from the environment (launch_knobs()): under TOYNI_P3_TILES=-1
    TOYNI_NT_MIN_BYTES=0 it must equal the two_step_nt block, which writes the same two fields of the struct."""
    blocks = _blocks(_run(exe, {"TOYNI_P3_TILES": "-1", "TOYNI_NT_MIN_BYTES": "0"}))
    assert blocks["default"] == blocks["two_step_nt"] and len(blocks["default"]) > 200
    plain = _blocks(_run(exe, {}))
    assert plain["default"] != plain["two_step_nt"] and plain["two_step_nt"] == blocks["two_step_nt"]
