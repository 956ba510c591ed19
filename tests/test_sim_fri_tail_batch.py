"""The one-workgroup batch twins of include/toyni_hip.h 3r -- both instantiations of fri_tail_rounds_batch_kernel and
merkle_tail_batch_kernel themselves, every GPU thread a fiber, three proofs (three workgroups) per launch -- run on the CPU under the
eight adversarial wave schedules of tests/sim/hip_sim.hpp by their own driver, tests/sim/sim_fri_tail_batch.cpp, as
tests/test_sim_fri_tail.py runs the single kernels.

The driver holds what a launch leaves for every proof -- every folded layer, every tree level, the betas, the transcript, and the
untouched gaps between the proofs -- under each schedule to the host model of sim_fri_tail.cpp, restated there.  The three transcripts
are 32, 55 and 1008 - 32 bytes long; one more launch per rounds kernel sets the status of the middle one.  Rounds: m = 2^10 -> 1,
2^6 -> 4 and 2 -> 1, salted; Merkle tail: m = 512, 3 and 1.  Every synchronisation site reached is listed; each is switched off in
turn, and some schedule must then fail.  CPU only, a stand-alone program, no sanitizer.  The test builds the driver."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
# rounds: the barrier behind the loads, the one behind beta, the one behind the leaves, the two of merkle_node_coop, the one that
# closes a level, and the one in front of the transcript's way back to global memory; Merkle tail: the one behind the level's load,
# the two of merkle_node_coop and the one that closes a level
SITES = {"fri_tail_rounds_batch_kernel_base": 7, "fri_tail_rounds_batch_kernel_ext": 7, "merkle_tail_batch_kernel": 4}
LAUNCHES = {"fri_tail_rounds_batch_kernel_base": 4, "fri_tail_rounds_batch_kernel_ext": 4, "merkle_tail_batch_kernel": 3}


def build_sim_fri_tail_batch() -> str:
    sim = os.path.join(ROOT, "tests", "sim")
    src, out = os.path.join(sim, "sim_fri_tail_batch.cpp"), os.path.join(sim, "build", "sim_fri_tail_batch")
    deps = [src, os.path.join(sim, "hip_sim.hpp"), os.path.join(ROOT, "include", "toyni_hip.h")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", out, src])
    return out


def _sim(*args):
    res = subprocess.run([build_sim_fri_tail_batch(), *args], capture_output=True, text=True, timeout=900)
    return res.returncode, res.stdout + res.stderr


@lru_cache(maxsize=None)
def _plain_runs():
    build_sim_fri_tail_batch()
    with ThreadPoolExecutor(max_workers=3) as ex:
        return dict(zip(SITES, ex.map(lambda k: _sim("--only", k), SITES)))


def test_the_three_kernels_pass_under_all_eight_schedules():
    runs = _plain_runs()
    bad = [k + ":\n" + out[-3000:] for k, (rc, out) in runs.items() if rc != 0 or "ALL OK" not in out or "hard failures=0" not in out]
    assert not bad, "\n".join(bad)
    for k, (_, out) in runs.items():
        assert len(re.findall(r"^SCHEDULE \S+ failures=0$", out, re.M)) == 8, k + ": eight schedules\n" + out[-2000:]
        assert re.findall(r"^RAN (\S+)$", out, re.M) == [k]
        assert int(re.search(r"launches=(\d+)", out).group(1)) == 8 * LAUNCHES[k]


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
