"""The Ext accumulator-column kernels' own synchronisation (include/toyni_hip.h 3i), run on the CPU under the adversarial wave
schedules of tests/sim/hip_sim.hpp by a second small driver, tests/sim/sim_scan_ext.cpp -- the `__global__` functions themselves,
every GPU thread a fiber, as tests/test_sim_schedules.py runs the other kernels.

The driver compares, under each of the eight schedules, what the kernels write with a host model (Ext products, the inverse through
the Frobenius norm) and prints that model's inputs and outputs once; this file recomputes them with tests/ext_model.py in Python
integers, so the kernels are held to the same model as tests/test_emu_scan_ext.py.  Cases: single launches, two and three tiles, both
ops, width-1 and width-4 operands in six of the forms, in place on either operand, zero denominators (counted), step 2 alone on more
aggregates than one of its rounds takes, and the inversion kernel below and above a tile.

The mutation pass: every synchronisation site a kernel reaches is switched off in turn and some schedule must fail; a site no schedule
can make fail is named in ARGUED with the reason.  CPU only, a stand-alone program, no sanitizer.  The test builds the driver itself."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import __graft_entry__ as entry
import ext_model as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = E.P

# sites in order of first arrival: the __shfl_up rendezvous (one source line serves every cross-lane step), the two barriers of
# ext_accum_block_exclusive, the two barriers of scan_block_exclusive<SCAN_COUNT> (the zero counts)
SITES = {
    "ext_accum_aggregate_kernel": 5,
    "ext_accum_prefix_kernel": 5,
    "ext_accum_apply_kernel": 5,
    "ext_invert_columns_kernel": 1,
}
_ONCE = ("the second barrier of a block-wide scan keeps a wave from overwriting the waves' totals in LDS before every wave has read them; this "
         "kernel runs that scan once per workgroup on this array (the Ext values and the zero counts have an array each), so nothing is written "
         "after the read and no output can change.  The barrier stays: the function it ends is shared with callers that loop")
ARGUED = {
    ("ext_accum_aggregate_kernel", 2): _ONCE,
    ("ext_accum_aggregate_kernel", 4): _ONCE,
    ("ext_accum_prefix_kernel", 4): _ONCE,
    ("ext_accum_apply_kernel", 2): _ONCE,
    ("ext_accum_apply_kernel", 4): _ONCE,
}
REQUIRED = [k + inst for k in ("ext_accum_aggregate_kernel", "ext_accum_prefix_kernel", "ext_accum_apply_kernel") for inst in ("<sum>", "<product>")] + \
           ["ext_invert_columns_kernel"]
WORKERS = 8


def build_sim_scan_ext() -> str:
    sim = os.path.join(ROOT, "tests", "sim")
    src, out = os.path.join(sim, "sim_scan_ext.cpp"), os.path.join(sim, "build", "sim_scan_ext")
    deps = [src, os.path.join(sim, "hip_sim.hpp"), os.path.join(ROOT, "include", "toyni_hip.h")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", out, src])
    return out


def _sim(*args):
    res = subprocess.run([build_sim_scan_ext(), *args], capture_output=True, text=True, timeout=900)
    return res.returncode, res.stdout + res.stderr


@lru_cache(maxsize=None)
def _plain_runs():
    build_sim_scan_ext()
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


def _cols(recs, k, tag, b, count, n):
    out = []
    for c in range(count):
        assert recs[k + c][:3] == [tag, str(b), str(c)] and len(recs[k + c]) == n + 3, (tag, b, c)
        out.append(list(map(int, recs[k + c][3:])))
    return out, k + count


def _operand(cols, width, shift, i):
    if width == 0:
        return E.ONE
    v = E.embed(cols[0][i]) if width == 1 else tuple(c[i] for c in cols)
    return E.add(v, shift)


def test_the_drivers_model_is_ext_model():
    """What the driver holds the kernels to, recomputed in Python integers."""
    rc, out = _sim()
    assert rc == 0 and "ALL OK" in out, out[-3000:]
    recs = [l.split() for l in out.splitlines() if re.match(r"^(CASE|INIT|NSHIFT|DSHIFT|NUM|DEN|WANT|WTOT|AGG|IN|WZEROS) ", l)]
    k, kinds, zeros_seen, rounds = 0, set(), 0, 0
    tile = None
    while k < len(recs):
        assert recs[k][0] == "CASE"
        kind = recs[k][1]
        kinds.add(kind)
        if kind == "ACCUM":
            op, n, batch, nw, dw = map(int, recs[k][2:])
            init = list(map(int, recs[k + 1][1:]))
            nshift, dshift = tuple(map(int, recs[k + 2][1:])), tuple(map(int, recs[k + 3][1:]))
            k += 4
            for b in range(batch):
                num, k = _cols(recs, k, "NUM", b, nw, n)
                den, k = _cols(recs, k, "DEN", b, dw, n)
                want, k = _cols(recs, k, "WANT", b, 4, n)
                wtot = list(map(int, recs[k][3:]))
                k += 1
                dens = [_operand(den, dw, dshift, i) for i in range(n)]
                invs = E.batch_inverse(dens) if dw else [E.ONE] * n
                acc = tuple(init[4 * b:4 * b + 4])
                for i in range(n):
                    assert tuple(w[i] for w in want) == acc, (op, n, nw, dw, b, i)
                    term = E.mul(_operand(num, nw, nshift, i), invs[i])
                    acc = E.mul(acc, term) if op else E.add(acc, term)
                z = sum(1 for d in dens if not any(d))
                zeros_seen += z
                assert wtot == list(acc) + [z, 0, 0, 0]
        elif kind == "PREFIX":
            op, ntiles, batch = map(int, recs[k][2:])
            init = list(map(int, recs[k + 1][1:]))
            k += 2
            rounds = max(rounds, ntiles)
            for b in range(batch):
                agg, k = _cols(recs, k, "AGG", b, 5, ntiles)
                want, k = _cols(recs, k, "WANT", b, 4, ntiles)
                wtot = list(map(int, recs[k][3:]))
                k += 1
                acc = tuple(init[4 * b:4 * b + 4])
                for t in range(ntiles):
                    assert tuple(w[t] for w in want) == acc, (op, ntiles, b, t)
                    v = tuple(a[t] for a in agg[:4])
                    acc = E.mul(acc, v) if op else E.add(acc, v)
                assert wtot == list(acc) + [sum(agg[4]), 0, 0, 0]
        else:
            assert kind == "INVERT"
            count = int(recs[k][2])
            vin, k2 = _cols(recs, k + 1, "IN", 0, 4, count)
            want, k2 = _cols(recs, k2, "WANT", 0, 4, count)
            elems = [tuple(v[i] for v in vin) for i in range(count)]
            assert [tuple(w[i] for w in want) for i in range(count)] == [E.inverse(e) if any(e) else E.ZERO for e in elems]
            assert recs[k2][0] == "WZEROS" and int(recs[k2][1]) == sum(1 for e in elems if not any(e)) > 0
            k = k2 + 1
    assert kinds == {"ACCUM", "PREFIX", "INVERT"} and zeros_seen > 10
    import toyni_amd
    tile = toyni_amd.prover.column_scan_ext_tile()
    assert rounds > 2 * tile, "step 2 must be run on more aggregates than one of its rounds takes"


def _sites_reached():
    sites = {}
    for k, (_, out) in _plain_runs().items():
        for m in re.finditer(r"^SITE (\w+):(\d+) (\S+) arrivals=(\d+)$", out, re.M):
            if m.group(1) == k:
                sites[(k, int(m.group(2)))] = m.group(3)
    return sites


def test_every_synchronisation_site_is_shown_needed_or_argued():
    sites = _sites_reached()
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
            wrong.append("%s:%d %s can be dropped and every schedule still matches the model: the cases cannot see what it protects" % (key + (sites[key],)))
        elif m.group(1) == "FAILS" and key in ARGUED:
            wrong.append("%s:%d %s is argued as invisible but a schedule does fail without it: move it to the needed sites" % (key + (sites[key],)))
    assert not wrong, "\n".join(wrong)
    for kernel in SITES:
        assert any(k == kernel and (k, i) not in ARGUED for k, i in sites), kernel
