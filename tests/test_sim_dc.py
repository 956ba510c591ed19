"""The kernels of include/toyni_hip.h 3p themselves -- the two one-wave preparation kernels and the record-fed twins of the quotient
and of the two Ext accumulator kernels that read an operand, every GPU thread a fiber -- run on the CPU under the eight adversarial
wave schedules of tests/sim/hip_sim.hpp (unchanged) by their own driver, tests/sim/sim_dc.cpp, as tests/test_sim_air_ext.py and
tests/test_sim_scan_ext.py run the argument-fed kernels.

The preparation kernels share nothing between lanes (no LDS, no barrier: no site).  The twins inherit the synchronisation of their
originals: the quotient's barrier behind the table of 1 / Z_H per residue class, and for the scans the cross-lane rendezvous, the two
barriers of ext_accum_block_exclusive and the two of the zero counts.  The quotient twin is held to a host model on plain residues
(parameters and alphas with words >= p, the emit_ext weights); the scan twins to the argument-fed kernels on the same columns under
the reduced shifts, which tests/test_sim_scan_ext.py holds to tests/ext_model.py.

The mutation pass: every synchronisation site a twin reaches is switched off in turn and some schedule must fail; the sites that
tests/test_sim_scan_ext.py argues as invisible in the originals are invisible here for the same reason.  CPU only, a stand-alone
program, no sanitizer.  The test builds the driver itself."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import __graft_entry__ as entry
from test_sim_scan_ext import _ONCE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
SITES = {"air_quotient_ext_dc_kernel": 1, "extcol_aggregate_dc_kernel": 5, "extcol_apply_dc_kernel": 5}
ARGUED = {("extcol_aggregate_dc_kernel", 2): _ONCE, ("extcol_aggregate_dc_kernel", 4): _ONCE,
          ("extcol_apply_dc_kernel", 2): _ONCE, ("extcol_apply_dc_kernel", 4): _ONCE}
REQUIRED = ["air_dc_prepare_kernel", "air_quotient_ext_dc_kernel", "extcol_dc_prepare_kernel"] + \
           [k + inst for k in ("extcol_aggregate_dc_kernel", "extcol_apply_dc_kernel") for inst in ("<sum>", "<product>")]
WORKERS = 8


def build_sim_dc() -> str:
    sim = os.path.join(ROOT, "tests", "sim")
    src, out = os.path.join(sim, "sim_dc.cpp"), os.path.join(sim, "build", "sim_dc")
    deps = [src, os.path.join(sim, "hip_sim.hpp"), os.path.join(ROOT, "tests", "emu", "contract_case.hpp"), os.path.join(ROOT, "include", "toyni_hip.h")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", out, src])
    return out


def _sim(*args):
    res = subprocess.run([build_sim_dc(), *args], capture_output=True, text=True, timeout=900)
    return res.returncode, res.stdout + res.stderr


@lru_cache(maxsize=None)
def _plain_runs():
    build_sim_dc()
    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        return dict(zip(SITES, ex.map(lambda k: _sim("--only", k), SITES)))


def test_every_kernel_passes_under_all_eight_schedules():
    runs = _plain_runs()
    bad = [k + ":\n" + out[-3000:] for k, (rc, out) in runs.items() if rc != 0 or "ALL OK" not in out or "hard failures=0" not in out]
    assert not bad, "\n".join(bad)
    for k, (_, out) in runs.items():
        assert len(re.findall(r"^SCHEDULE \S+ failures=0$", out, re.M)) == 8, k + ": eight schedules\n" + out[-2000:]
    ran = {line[4:] for _, out in runs.values() for line in out.splitlines() if line.startswith("RAN ")}
    assert set(REQUIRED) <= ran, sorted(ran)


def _sites_reached():
    sites, silent = {}, set()
    for k, (_, out) in _plain_runs().items():
        for m in re.finditer(r"^SITE (\w+):(\d+) (\S+) arrivals=(\d+)$", out, re.M):
            if m.group(1) == k:
                sites[(k, int(m.group(2)))] = m.group(3)
            if "prepare" in m.group(1):
                silent.add(m.group(1))
    return sites, silent


def test_every_synchronisation_site_is_shown_needed_or_argued_and_the_preparation_kernels_have_none():
    sites, silent = _sites_reached()
    assert not silent, "a preparation kernel reached a synchronisation site: %s" % sorted(silent)
    assert {k: sum(1 for s in sites if s[0] == k) for k in SITES} == SITES, sorted(sites.items())
    assert all(key in sites for key in ARGUED), "ARGUED names a site that no kernel reaches"
    order = sorted(sites)
    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        outs = list(ex.map(lambda s: _sim("--drop", "%s:%d" % s), order))
    wrong = []
    for key, (rc, out) in zip(order, outs):
        m = re.search(r"^DROP %s:%d \S+ (FAILS|SURVIVES)" % key, out, re.M)
        if rc != 0 or not m:
            wrong.append("%s:%d %s: the mutation run broke\n%s" % (key + (sites[key], out[-1500:])))
        elif m.group(1) == "SURVIVES" and key not in ARGUED:
            wrong.append("%s:%d %s can be dropped and every schedule still matches: the cases cannot see what it protects" % (key + (sites[key],)))
        elif m.group(1) == "FAILS" and key in ARGUED:
            wrong.append("%s:%d %s is argued as invisible but a schedule does fail without it: move it to the needed sites" % (key + (sites[key],)))
    assert not wrong, "\n".join(wrong)
