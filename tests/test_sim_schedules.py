"""The kernels' own synchronisation, run on the CPU under adversarial wave schedules (tests/sim).

tests/emu steps the kernel BODIES and restates where the barriers stand; here the `__global__` functions of toyni_hip.hip
themselves run -- every GPU thread a fiber, the waves released at the kernels' own barriers in unfriendly orders (ascending,
descending, two seeded shuffles; lanes ascending and descending) -- and what they write is compared with the oracle.  A missing
or misplaced barrier, a false "this wave reads only what it wrote" claim, lanes that part ways at a barrier or a "uniform" value
that differs between lanes fails deterministically here; on the GPU it passes by timing.

The mutation pass gives the harness teeth: every synchronisation site a kernel reaches (barrier, __syncthreads, TOYNI_WAVE_ORDER,
__shfl_up rendezvous; numbered per kernel in order of first arrival) is switched off in the simulator's hook, one at a time, and
some schedule must then produce a mismatch or a hard failure.  A site no schedule can make fail is named in ARGUED below with
the reason.  CPU only, a stand-alone program, no sanitizer (the bounds of the same bodies are tests/emu's business)."""
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import __graft_entry__ as entry

# every kernel that must run, with the number of synchronisation sites it reaches (kernel, ordinal) -> shown needed unless ARGUED
SITES = {
    "ntt_pass_kernel": 3,                 # __syncthreads (stage twiddles), step-1/step-2 barrier, loop-end barrier
    "ntt_pass3_kernel": 4,                # stage table, step 1/2, step 2/3, loop end
    "ntt_pass3s_kernel": 5,               # __syncthreads, wave order (WAVE_LOCAL2) and its barrier twin, step 2/3, loop end
    "ntt_lds_kernel": 4,
    "ntt_row2048_kernel": 4,              # __syncthreads and the three wave orders
    "ntt_row4096_kernel": 4,
    "column_scan_aggregate_kernel": 3,    # the __shfl_up rendezvous and the two barriers of scan_block_exclusive
    "column_scan_prefix_kernel": 3,
    "column_scan_apply_kernel": 3,
    "batch_inverse_kernel": 1,
    "merkle_level_coop_kernel": 2,
    "merkle_tail_kernel": 4,              # level fill, the two hand-over barriers of merkle_node_coop, loop end
    "poly_eval_partial_kernel": 3,        # block_sum_mod: after the fill, inside the tree, after the read of red[0]
    "poly_eval_final_kernel": 3,
    "poly_eval_batch_partial_kernel": 3,
    "poly_eval_batch_final_kernel": 3,
    "fib_quotient_kernel": 1,
    "air_quotient_kernel": 1,
    "air_quotient_inline_kernel": 1,
}

_BLOCK_SUM_TAIL = ("block_sum_mod's last barrier keeps a wave from overwriting red[0] (the next call's fill) before every thread has read "
                   "the sum; but thread 0 is the only writer of red[0] and the only thread whose return value any caller stores "
                   "(`if (threadIdx.x == 0) ... = sum`), so with two and four points re-entering the function no output can change")
ARGUED = {
    ("poly_eval_partial_kernel", 2): _BLOCK_SUM_TAIL,
    ("poly_eval_final_kernel", 2): _BLOCK_SUM_TAIL,
    ("poly_eval_batch_partial_kernel", 2): _BLOCK_SUM_TAIL,
    ("poly_eval_batch_final_kernel", 2): _BLOCK_SUM_TAIL,
    ("ntt_lds_kernel", 0): ("the __syncthreads behind the copy of the phase-B twiddles into lds_tw1: phase B is the table's first reader and stands "
                            "behind the loop's first TOYNI_LDS_BARRIER, which every wave reaches after its own share of the copy -- at any tile "
                            "count; what the __syncthreads adds on the device is the drain of the first tile's loads (vmcnt), which has no CPU form"),
}

# what the printed list of instantiations must contain: all six transform templates, both WAVE_LOCAL2 values, the shapes of the issue
REQUIRED_INSTANTIATIONS = [
    r"ntt_pass_kernel<kind=0,.*lq=0,lz=0>", r"ntt_pass_kernel<kind=1,.*lq=0,lz=0>",      # two-step first and closing passes
    r"ntt_pass_kernel<kind=0,lm=7,", r"ntt_pass_kernel<kind=0,lm=8,", r"ntt_pass_kernel<kind=0,lm=9,",   # 2^14, 2^16, 2^18
    r"ntt_pass_kernel<.*lz=1>", r"ntt_pass_kernel<.*lz=4>",                                # LDE blow-up 2 and 16
    r"ntt_pass_kernel<.*lq=2,", r"ntt_pass_kernel<.*single-step>",
    r"ntt_pass3_kernel<kind=0,lm=8,", r"ntt_pass3_kernel<kind=1,lm=11,",                   # 2^16 latency shape, 2048 points of 2^21
    r"ntt_pass3s_kernel<.*WAVE_LOCAL2=true>", r"ntt_pass3s_kernel<kind=0,.*lz=5,WAVE_LOCAL2=false>",
    r"ntt_lds_kernel<", r"ntt_row2048_kernel<nt=0>", r"ntt_row2048_kernel<nt=1>", r"ntt_row4096_kernel<nt=0>", r"ntt_row4096_kernel<nt=1>",
    r"column_scan_aggregate_kernel<sum>", r"column_scan_aggregate_kernel<product>", r"column_scan_prefix_kernel<sum>",
    r"column_scan_prefix_kernel<product>", r"column_scan_apply_kernel<sum>", r"column_scan_apply_kernel<product>",
]

WORKERS = 8


def _sim(*args):
    res = subprocess.run([entry.build_sim(), *args], capture_output=True, text=True, timeout=900)
    return res.returncode, res.stdout + res.stderr


@lru_cache(maxsize=None)
def _plain_runs():
    """Every kernel's cases under all eight schedules, nothing dropped: one process per kernel, the slowest first."""
    entry.build_sim()
    order = sorted(SITES, key=lambda k: ("pass3" not in k, "ntt" not in k))
    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        return dict(zip(order, ex.map(lambda k: _sim("--only", k), order)))


def test_the_simulator_reports_its_hard_failures():
    """Toy kernels inside the driver: lanes of a wave of which some return ahead of a barrier, lanes that arrive from two source lines, a
    TOYNI_UNIFORM value that differs in one lane, a wave split between a wave rendezvous and a barrier -- each must end in exactly
    that hard failure under every schedule, and a well-formed toy (a whole wave returning early, lanes leaving ahead of a wave
    rendezvous) in none."""
    rc, out = _sim("--selftest")
    assert rc == 0 and "SELFTEST OK" in out, out[-3000:]


def test_every_kernel_passes_under_all_eight_schedules():
    runs = _plain_runs()
    bad = [k + ":\n" + out[-3000:] for k, (rc, out) in runs.items() if rc != 0 or "ALL OK" not in out or "hard failures=0" not in out]
    assert not bad, "\n".join(bad)
    for k, (_, out) in runs.items():
        assert len(re.findall(r"^SCHEDULE \S+ failures=0$", out, re.M)) == 8, k + ": eight schedules\n" + out[-2000:]
    ran = "\n".join(line for _, out in runs.values() for line in out.splitlines() if line.startswith("RAN "))
    for kernel in SITES:
        assert re.search(r"^RAN " + kernel + r"(<|$)", ran, re.M), kernel + " never ran"
    for pattern in REQUIRED_INSTANTIATIONS:
        assert re.search(r"^RAN " + pattern, ran, re.M), "no instantiation matching " + pattern + "\n" + ran


def _sites_reached():
    sites = {}
    for k, (_, out) in _plain_runs().items():
        for m in re.finditer(r"^SITE (\w+):(\d+) (\S+) arrivals=(\d+)$", out, re.M):
            if m.group(1) == k:
                sites[(k, int(m.group(2)))] = m.group(3)
    return sites


def test_every_synchronisation_site_is_shown_needed_or_argued():
    sites = _sites_reached()
    # no site may be left unclassified: the kernels reach exactly the sites of the table
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
            wrong.append("%s:%d %s can be dropped and every schedule still matches the oracle: the cases cannot see what it protects" % (key + (sites[key],)))
        elif m.group(1) == "FAILS" and key in ARGUED:
            wrong.append("%s:%d %s is argued as invisible but a schedule does fail without it: move it to the needed sites" % (key + (sites[key],)))
    assert not wrong, "\n".join(wrong)
    for kernel in SITES:   # a kernel with no site shown needed does not count as covered
        assert any(k == kernel and (k, i) not in ARGUED for k, i in sites), kernel
