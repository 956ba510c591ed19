"""The AIR quotient kernels under Ext weights (include/toyni_hip.h 3k) -- the two `__global__` functions themselves, every GPU thread a
fiber -- run on the CPU under the eight adversarial wave schedules of tests/sim/hip_sim.hpp by their own small driver,
tests/sim/sim_air_ext.cpp, as tests/test_sim_scan_ext.py runs the Ext accumulator kernels.

The driver holds what the kernels write, under each schedule, to a host model that interprets the program point by point on plain
residues; cases log N = 10 / B = 2^3 (one workgroup) and log N = 12 / B = 2^8 (four), out_stride = N + 1, with a c output and with
accumulation.  Each kernel reaches one synchronisation site, the __syncthreads behind the table of 1 / Z_H per residue class; the
mutation pass switches it off and some schedule must fail.  CPU only, a stand-alone program, no sanitizer.  The test builds the driver."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
SITES = {"air_quotient_ext_kernel": 1, "air_quotient_ext_inline_kernel": 1}


def build_sim_air_ext() -> str:
    sim = os.path.join(ROOT, "tests", "sim")
    src, out = os.path.join(sim, "sim_air_ext.cpp"), os.path.join(sim, "build", "sim_air_ext")
    deps = [src, os.path.join(sim, "hip_sim.hpp"), os.path.join(ROOT, "include", "toyni_hip.h")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", out, src])
    return out


def _sim(*args):
    res = subprocess.run([build_sim_air_ext(), *args], capture_output=True, text=True, timeout=900)
    return res.returncode, res.stdout + res.stderr


@lru_cache(maxsize=None)
def _plain_runs():
    build_sim_air_ext()
    with ThreadPoolExecutor(max_workers=2) as ex:
        return dict(zip(SITES, ex.map(lambda k: _sim("--only", k), SITES)))


def test_both_kernels_pass_under_all_eight_schedules():
    runs = _plain_runs()
    bad = [k + ":\n" + out[-3000:] for k, (rc, out) in runs.items() if rc != 0 or "ALL OK" not in out or "hard failures=0" not in out]
    assert not bad, "\n".join(bad)
    for k, (_, out) in runs.items():
        assert len(re.findall(r"^SCHEDULE \S+ failures=0$", out, re.M)) == 8, k + ": eight schedules\n" + out[-2000:]
        assert re.findall(r"^RAN (\S+)$", out, re.M) == [k]
        assert int(re.search(r"launches=(\d+)", out).group(1)) == 16          # two cases x eight schedules


def _sites_reached():
    sites = {}
    for k, (_, out) in _plain_runs().items():
        for m in re.finditer(r"^SITE (\w+):(\d+) (\S+) arrivals=(\d+)$", out, re.M):
            if m.group(1) == k:
                sites[(k, int(m.group(2)))] = (m.group(3), int(m.group(4)))
    return sites


def test_the_barrier_behind_the_zh_table_is_the_only_site_and_is_needed():
    sites = _sites_reached()
    assert {k: sum(1 for s in sites if s[0] == k) for k in SITES} == SITES, sorted(sites.items())
    for key, (text, arrivals) in sites.items():
        assert "toyni_hip.hip" in text and arrivals > 0, (key, text)
    order = sorted(sites)
    with ThreadPoolExecutor(max_workers=2) as ex:
        outs = list(ex.map(lambda s: _sim("--drop", "%s:%d" % s), order))
    for key, (rc, out) in zip(order, outs):
        m = re.search(r"^DROP %s:%d \S+ (FAILS|SURVIVES)" % key, out, re.M)
        assert rc == 0 and m, "%s:%d: the mutation run broke\n%s" % (key + (out[-1500:],))
        assert m.group(1) == "FAILS", "%s:%d can be dropped and every schedule still matches the model" % key
