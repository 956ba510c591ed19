"""The kernels of include/toyni_hip.h 3o themselves -- the three preparation kernels, the three device-record twins of the hot kernels,
the two transcript helpers and query_rows_kernel, every GPU thread a fiber -- run on the CPU through tests/sim/hip_sim.hpp (unchanged)
by their own driver, tests/sim/sim_dz.cpp, which arranges the buffers as the entry points do and expects nothing itself.  Every
printed word is recomputed here from Python integers (tests/ext_model.py) and hashlib; under each of the header's eight wave / lane
schedules the outputs must be the first schedule's (the preparation kernels hand the shares of the claim from every lane to lane 0
through LDS behind a wave rendezvous: the one place where an order matters).

Evaluation: ncoeffs in {1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 5}, 1..4 points, batch 1 and 3.  DEEP: N in {2, 4, 1024}, 1, 64
and 65 slots (inline and staged), accumulate on and off, aligned and misaligned columns, z on the coset once.  CPU only, a stand-alone
program, no sanitizer."""
import os
import re
import subprocess
from functools import lru_cache

import numpy as np

import __graft_entry__ as entry
import ext_model as em
from test_emu_transcript import E_RANGE, Model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
P = em.P
KERNELS = ["poly_ext_prepare_kernel", "poly_eval_ext_batch_partial_dz_kernel", "poly_eval_ext_batch_final_dz_kernel", "deep_ext_prepare_inline_kernel",
           "deep_ext_prepare_kernel", "deep_combine_ext_dz_kernel", "transcript_squeeze_ext_point_kernel", "transcript_absorb_fields_kernel",
           "query_rows_kernel"]


def build_sim_dz(contracts_header=None) -> str:
    sim = os.path.join(ROOT, "tests", "sim")
    src, out = os.path.join(sim, "sim_dz.cpp"), os.path.join(sim, "build", "sim_dz" + ("_contracts" if contracts_header else ""))
    deps = [src, os.path.join(sim, "hip_sim.hpp"), os.path.join(ROOT, "tests", "emu", "contract_case.hpp"), os.path.join(ROOT, "include", "toyni_hip.h")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))] + ([contracts_header] if contracts_header else [])
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        extra = ["-include", os.path.join(sim, "hip_sim.hpp"), "-include", contracts_header] if contracts_header else []
        subprocess.check_call([entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include")] + extra + ["-o", out, src])
    return out


@lru_cache(maxsize=None)
def run(saturated=False, contracts_header=None):
    res = subprocess.run([build_sim_dz(contracts_header)] + (["saturated"] if saturated else []), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("DONE"), res.stdout[-2000:] + res.stderr[-3000:]
    return res.stdout, res.stderr


def ints(fields):
    return [int(v) for v in fields]


def judge(stdout, saturated):
    """every record against the integer model; -> (poly shapes, deep shapes, kinds of the transcript records)"""
    assert "DIFFER" not in stdout
    m = re.search(r"^SCHEDULES same=(\d+) differ=0\nlaunches=(\d+) launch failures=0 hard failures=0$", stdout, re.M)
    assert m and int(m.group(1)) > 0, stdout[-600:]
    recs = [l.split(" ") for l in stdout.split("\n")]
    k, polys, deeps, kinds = 0, set(), set(), []
    while recs[k][0] != "SCHEDULES":
        r = recs[k]
        if r[0] == "POLY":
            ncoeffs, npoints, batch = ints(r[1:])
            z, mults = ints(recs[k + 1][1:]), ints(recs[k + 2][1:])
            cols = [ints(recs[k + 3 + b][2:]) for b in range(batch)]
            assert all(len(c) == ncoeffs for c in cols) and recs[k + 3 + batch][0] == "POUT"
            got = np.array(ints(recs[k + 3 + batch][1:]), dtype=np.uint32).reshape(batch, npoints, 4)
            points = [tuple(c * mlt % P for c in z) for mlt in mults]
            want = np.array(em.poly_eval_ext_batch_model(cols, points), dtype=np.uint32).reshape(batch, npoints, 4)
            assert (got == want).all(), (ncoeffs, npoints, batch)
            polys.add((ncoeffs, npoints, batch))
            k += 4 + batch
        elif r[0] == "DEEP":
            log_n, log_b, width, stride, nslots, acc, off = ints(r[1:])
            N = 1 << log_n
            z = tuple(ints(recs[k + 1][1:]))
            slots = [ints(recs[k + 2 + t][1:]) for t in range(nslots)]
            base = k + 2 + nslots
            al, cl = (np.array(ints(recs[base + j][1:]), dtype=np.uint64).reshape(-1, 4) for j in (0, 1))
            cols = np.array([ints(recs[base + 2 + c][2:]) for c in range(width)], dtype=np.uint64)
            prev = np.array(ints(recs[base + 2 + width][1:]), dtype=np.uint64).reshape(-1, 4)
            assert recs[base + 3 + width][0] == "OUT"
            got = np.array(ints(recs[base + 3 + width][1:]), dtype=np.uint64).reshape(N, 4)
            terms = [(c, r_, tuple(int(v) for v in al[ai]), tuple(int(v) for v in cl[vi])) for c, r_, ai, vi in slots]
            want = em.deep_ext_model(cols, terms, 1 << log_b, 7, z).astype(np.uint64)
            if acc:
                want = (want + prev) % np.uint64(P)
            assert (got == want).all(), (log_n, nslots, acc, off)
            on_coset = not any(z[1:]) and not saturated
            if on_coset:
                assert not acc and not got[N - 1].any()
            deeps.add((N, nslots, acc, off, on_coset))
            k = base + 4 + width
        elif r[0] == "POINT":
            state = bytes.fromhex(r[1]) if r[1] != "-" else b""
            z, (length, status) = ints(r[2:6]), ints(r[6:8])
            mdl = Model(state)
            want = mdl.squeeze(4)
            assert any(want[1:]) and z == want and (length, status) == (32, 0) and bytes.fromhex(r[8]) == mdl.state
            kinds.append("POINT")
            k += 1
        elif r[0] == "FIELDS":
            state = bytes.fromhex(r[1]) if r[1] != "-" else b""
            words = ints(r[2:])
            t = recs[k + 1]
            mdl = Model(state)
            mdl.absorb(b"".join((w % P).to_bytes(8, "little") for w in words))
            assert t[0] == "T" and ints(t[1:3]) == [len(mdl.state), mdl.status] and (bytes.fromhex(t[3]) if t[3] != "-" else b"") == mdl.state
            kinds.append("FIELDS refused" if mdl.status == E_RANGE else "FIELDS")
            k += 2
        else:
            assert r[0] == "ROWS", r[:3]
            n, noffsets = ints(r[1:3])
            offsets, idx, got = ints(r[3:]), ints(recs[k + 1][1:]), ints(recs[k + 2][1:])
            assert len(offsets) == noffsets and got == [(i + o) % n for i in idx for o in offsets]
            kinds.append(("ROWS", n, noffsets))
            k += 3
    return polys, deeps, kinds


def test_every_new_kernel_matches_the_integer_model_under_every_schedule():
    stdout, _ = run()
    polys, deeps, kinds = judge(stdout, False)
    assert {p[0] for p in polys} == {1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 5} and {p[1] for p in polys} == {1, 2, 3, 4} and {p[2] for p in polys} == {1, 3}
    assert {(d[0], d[1]) for d in deeps} == {(N, s) for N in (2, 4, 1024) for s in (1, 64, 65)}
    assert {d[2] for d in deeps} == {0, 1} and {d[3] for d in deeps} == {0, 1} and sum(d[4] for d in deeps) >= 3
    assert kinds.count("POINT") == 4 and kinds.count("FIELDS") == 3 and kinds.count("FIELDS refused") == 1
    assert [kd[1:] for kd in kinds if kd[0] == "ROWS"] == [(1, 1), (1 << 32, 2), (1 << 14, 2), (96, 8)]


def test_every_new_kernel_with_every_word_saturated():
    stdout, _ = run(True)
    polys, deeps, kinds = judge(stdout, True)
    assert {p[0] for p in polys} == {17, 4097} and {(d[0], d[1]) for d in deeps} == {(1024, 64), (1024, 65)}
