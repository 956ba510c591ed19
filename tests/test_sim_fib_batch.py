"""The thirteen kernels of include/toyni_hip.h 3s themselves -- the batch twins of the first half of a Fibonacci proof and the row
copy, every GPU thread a fiber -- run on the CPU through tests/sim/hip_sim.hpp (unchanged) by their own driver,
tests/sim/sim_fib_batch.cpp: three proofs per launch with guard bands between them, judged by the single kernels on each proof's
pointers and by plain host arithmetic, under each of the header's eight wave / lane schedules.  One transcript in the middle has its
status set; one is so long that absorbing four fields overflows it.

The quotient twin reaches the barrier behind its LDS fill, the two evaluation twins the three barriers of block_sum_mod; each is
switched off in turn.  Without the fill's barrier, the barrier behind block_sum_mod's store, or the one inside its tree (stage 2 on
300 partial sums per proof, so that two waves' values meet there), some schedule must fail.  The third site of block_sum_mod, behind
the read of red[0], is argued exactly as tests/test_sim_fib_dz.py argues it for the single forms: no output can show it, and a
schedule that does fail without it would be a finding.  The field absorb reaches the wave-order point of
transcript_absorb_fields_wave (every lane reads the length before lane 0 stores it): without it some lane schedule must fail too.
No other kernel of 3s reaches a synchronisation site.  CPU only, a stand-alone program, no sanitizer."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import __graft_entry__ as entry
from test_sim_schedules import _BLOCK_SUM_TAIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
SITES = {"fib_quotient_batch_kernel": 1, "poly_eval_partial_dz_batch_kernel": 3, "poly_eval_final_dz_batch_kernel": 3,
         "transcript_absorb_fields_batch_kernel": 1}
ARGUED = {("poly_eval_partial_dz_batch_kernel", 2): _BLOCK_SUM_TAIL, ("poly_eval_final_dz_batch_kernel", 2): _BLOCK_SUM_TAIL}
KERNELS = ["chacha20_fill_batch_kernel", "fib_mask_batch_kernel", "fib_quotient_batch_kernel", "transcript_squeeze_point_batch_kernel",
           "transcript_absorb_fields_batch_kernel", "poly_dz_prepare_batch_kernel", "poly_eval_partial_dz_batch_kernel",
           "poly_eval_final_dz_batch_kernel", "fib_deep_prepare_batch_kernel", "fib_deep_dz_batch_kernel", "query_rows_batch_kernel",
           "fri_phase_roots_batch_kernel", "copy_rows_kernel"]
WORKERS = 8


def build_sim_fib_batch(contracts_header=None) -> str:
    sim = os.path.join(ROOT, "tests", "sim")
    src, out = os.path.join(sim, "sim_fib_batch.cpp"), os.path.join(sim, "build", "sim_fib_batch" + ("_contracts" if contracts_header else ""))
    deps = [src, os.path.join(sim, "hip_sim.hpp"), os.path.join(ROOT, "tests", "emu", "contract_case.hpp"), os.path.join(ROOT, "include", "toyni_hip.h")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))] + [os.path.join(CSRC, "batch", "toyni_hip_fib_batch.hip")] + ([contracts_header] if contracts_header else [])
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        extra = ["-include", os.path.join(sim, "hip_sim.hpp"), "-include", contracts_header] if contracts_header else []
        subprocess.check_call([entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include")] + extra + ["-o", out, src])
    return out


def _sim(*args, contracts_header=None):
    res = subprocess.run([build_sim_fib_batch(contracts_header), *args], capture_output=True, text=True, timeout=900)
    return res.returncode, res.stdout, res.stderr


@lru_cache(maxsize=None)
def _plain_run():
    return _sim()


def test_every_kernel_passes_under_all_eight_schedules():
    rc, out, err = _plain_run()
    assert rc == 0 and "ALL OK" in out and "hard failures=0" in out, out[-3000:] + err[-2000:]
    assert len(re.findall(r"^SCHEDULE \S+ failures=0$", out, re.M)) == 8, out[-2000:]
    ran = {line[4:] for line in out.splitlines() if line.startswith("RAN ")}
    assert set(KERNELS) <= ran, sorted(ran)


def test_every_word_saturated():
    rc, out, err = _sim("--saturated")
    assert rc == 0 and "ALL OK" in out and "hard failures=0" in out, out[-3000:] + err[-2000:]


def test_the_barriers_of_the_quotient_and_evaluation_twins_are_needed_and_no_other_kernel_reaches_a_site():
    _, out, _ = _plain_run()
    sites = {(m.group(1), int(m.group(2))): m.group(3) for m in re.finditer(r"^SITE (\w+):(\d+) (\S+) arrivals=(\d+)$", out, re.M)}
    assert {k: sum(1 for s in sites if s[0] == k) for k in KERNELS} == {k: SITES.get(k, 0) for k in KERNELS}, sorted(sites.items())
    kinds = {k: {text.split("@")[0] for (name, _), text in sites.items() if name == k} for k in SITES}
    assert kinds == {k: {"wave_order" if k == "transcript_absorb_fields_batch_kernel" else "syncthreads"} for k in SITES}, sites
    assert all(key in sites for key in ARGUED), "ARGUED names a site that no kernel reaches"
    order = sorted(s for s in sites if s[0] in KERNELS)
    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        outs = list(ex.map(lambda s: _sim("--drop", "%s:%d" % s), order))
    wrong = []
    for key, (rc, o, e) in zip(order, outs):
        m = re.search(r"^DROP %s:%d \S+ (FAILS|SURVIVES)" % key, o, re.M)
        if rc != 0 or not m:
            wrong.append("%s:%d %s: the mutation run broke\n%s" % (key + (sites[key], (o + e)[-1500:])))
        elif m.group(1) == "FAILS" and key in ARGUED:
            wrong.append("%s:%d %s is argued as invisible but a schedule does fail without it" % (key + (sites[key],)))
        elif m.group(1) == "SURVIVES" and key not in ARGUED:
            wrong.append("%s:%d %s can be dropped and every schedule still matches: the cases cannot see what it protects" % (key + (sites[key],)))
    assert not wrong, "\n".join(wrong)
