"""The fused rounds of the transcript commit phase (include/toyni_hip.h 3l) -- the two instantiations of fri_tail_rounds_kernel
themselves, every GPU thread a fiber -- run on the CPU under the eight adversarial wave schedules of tests/sim/hip_sim.hpp by their own
driver, tests/sim/sim_fri_tail.cpp, as tests/test_sim_air_ext.py runs the AIR kernels.

The driver holds what a launch leaves -- every folded layer, every tree level, the betas, the transcript -- under each schedule to a
host model built from a fold on plain residues, a byte-oriented SHA-256 and the transcript as a byte vector.  Cases, base and Ext,
salted: m = 2^10 -> 1 (ten rounds, the widest level), m = 2^6 -> 4, and m = 2 -> 1, one round in which the leaf is the root.
Every synchronisation site reached is listed; each is switched off in turn, and some schedule must then fail.
CPU only, a stand-alone program, no sanitizer.  The test builds the driver."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
# the barrier behind the loads, the one behind beta, the one behind the leaves, the two of merkle_node_coop, the one that closes a
# level, and the one in front of the transcript's way back to global memory
SITES = {"fri_tail_rounds_kernel_base": 7, "fri_tail_rounds_kernel_ext": 7}
CASES = 3


def build_sim_fri_tail() -> str:
    sim = os.path.join(ROOT, "tests", "sim")
    src, out = os.path.join(sim, "sim_fri_tail.cpp"), os.path.join(sim, "build", "sim_fri_tail")
    deps = [src, os.path.join(sim, "hip_sim.hpp"), os.path.join(ROOT, "include", "toyni_hip.h")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", out, src])
    return out


def _sim(*args):
    res = subprocess.run([build_sim_fri_tail(), *args], capture_output=True, text=True, timeout=900)
    return res.returncode, res.stdout + res.stderr


@lru_cache(maxsize=None)
def _plain_runs():
    build_sim_fri_tail()
    with ThreadPoolExecutor(max_workers=2) as ex:
        return dict(zip(SITES, ex.map(lambda k: _sim("--only", k), SITES)))


def test_both_kernels_pass_under_all_eight_schedules():
    runs = _plain_runs()
    bad = [k + ":\n" + out[-3000:] for k, (rc, out) in runs.items() if rc != 0 or "ALL OK" not in out or "hard failures=0" not in out]
    assert not bad, "\n".join(bad)
    for k, (_, out) in runs.items():
        assert len(re.findall(r"^SCHEDULE \S+ failures=0$", out, re.M)) == 8, k + ": eight schedules\n" + out[-2000:]
        assert re.findall(r"^RAN (\S+)$", out, re.M) == [k]
        assert int(re.search(r"launches=(\d+)", out).group(1)) == 8 * CASES


def _sites_reached():
    sites = {}
    for k, (_, out) in _plain_runs().items():
        for m in re.finditer(r"^SITE (\w+):(\d+) (\S+) arrivals=(\d+)$", out, re.M):
            if m.group(1) == k:
                sites[(k, int(m.group(2)))] = (m.group(3), int(m.group(4)))
    return sites


def test_every_synchronisation_site_is_listed_and_needed():
    sites = _sites_reached()
    assert {k: sum(1 for s in sites if s[0] == k) for k in SITES} == SITES, sorted(sites.items())
    for key, (text, arrivals) in sites.items():
        assert "toyni_hip.hip" in text and arrivals > 0, (key, text)
    order = sorted(sites)
    with ThreadPoolExecutor(max_workers=4) as ex:
        outs = list(ex.map(lambda s: _sim("--drop", "%s:%d" % s), order))
    for key, (rc, out) in zip(order, outs):
        m = re.search(r"^DROP %s:%d \S+ (FAILS|SURVIVES)" % key, out, re.M)
        assert rc == 0 and m, "%s:%d: the mutation run broke\n%s" % (key + (out[-1500:],))
        assert m.group(1) == "FAILS", "%s:%d can be dropped and every schedule still matches the model" % key
