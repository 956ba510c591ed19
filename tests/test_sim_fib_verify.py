"""The five kernels of include/toyni_hip.h 3t themselves -- toyni_amd/csrc/verify/toyni_hip_verify.hip, every GPU thread a fiber -- run on
the CPU through tests/sim/hip_sim.hpp (unchanged) by their own driver, tests/sim/sim_fib_verify.cpp, under each of the header's eight
wave / lane schedules, with guard bands between the images, between the proofs' parts of the work buffer and around the verdicts.

The images come from here: proofs of the oracle-only prover (tests/harness/ref_prover.py), packed by toyni_amd.verifier.pack_fib_proof.
One launch carries the three valid proofs and, behind them, one tampered copy of the middle proof per row of the tamper matrix
(tests/fib_verify_cases.py), a valid proof again after every eighth row: every valid proof must read 0 among its failing neighbours --
a proof that fails, fails alone.  The judge of every verdict is tests/harness/fib_verifier.py on the same proof; the word of every
record is held to verify_opening plus the position binding.  n = 8 and 16 are the smallest proofs there are (N = 256 / 512, 8 folds,
final layer of 1 / 2); n = 256 (9 folds, final layer of 16) runs the subset with one row per verdict code.

Synchronisation sites.  fib_verify_global_kernel reaches the three wave-order points of its any_lane (clear / set / read of one LDS
word) and three around its final-layer tree; each is switched off in turn at n = 256 and some schedule must then fail -- except the
point BEHIND the read of the flag word, which only keeps the next clear from overtaking the other lanes' reads: lane 0 alone uses what
it read, so no output can show that site (a schedule that does fail without it would be a finding).  fib_verify_replay_kernel runs on
ONE lane; the two wave-order points of transcript_squeeze_indices it passes have no second lane to order against, and dropping them
cannot change a word.  No other kernel of the unit reaches a site.  CPU only, a stand-alone program, no sanitizer."""
import os
import re
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import pytest

import __graft_entry__ as entry
import fib_verify_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
KERNELS = ["fib_verify_replay_kernel", "fib_verify_global_kernel", "merkle_verify_records_batch_kernel", "fib_verify_query_kernel",
           "fib_verify_verdict_kernel"]
SITES = {"fib_verify_global_kernel": 6, "fib_verify_replay_kernel": 2}
_ONE_LANE = "one lane runs the replay: a wave-order point has nothing to order"
_BEHIND_READ = "behind the read of the flag word: only lane 0 uses what it read"
ARGUED = {("fib_verify_replay_kernel", 0): _ONE_LANE, ("fib_verify_replay_kernel", 1): _ONE_LANE, ("fib_verify_global_kernel", 2): _BEHIND_READ}


def build_sim_fib_verify(contracts_header=None) -> str:
    sim = os.path.join(ROOT, "tests", "sim")
    src, out = os.path.join(sim, "sim_fib_verify.cpp"), os.path.join(sim, "build", "sim_fib_verify" + ("_contracts" if contracts_header else ""))
    deps = [src, os.path.join(sim, "hip_sim.hpp"), os.path.join(ROOT, "tests", "emu", "contract_case.hpp")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(CSRC, "verify", f) for f in ("toyni_hip_verify.hip", "verify_kernels.hpp")] + \
           ([contracts_header] if contracts_header else [])
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        extra = ["-include", os.path.join(sim, "hip_sim.hpp"), "-include", contracts_header] if contracts_header else []
        subprocess.check_call([entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable",
                               "-I", CSRC, "-I", os.path.join(ROOT, "include")] + extra + ["-o", out, src])
    return out


@lru_cache(maxsize=None)
def batch_of(n, full=True, saturated=False):
    """(the proofs of one launch in wire form, [(position, row)] of the tampered ones)"""
    entry.build_hip()
    valid = cases.proofs(n)
    for p in valid:
        assert cases.expected_of(p) == (True, "accept")
    rows = cases.matrix(valid[1], full=full) + [("op and op_pair swapped",) + (cases.swap_row(valid[1])[0],) + cases.swap_row(valid[1])[1:] + ("fri_merkle",)]
    raws, where = list(valid), []
    for k, row in enumerate(rows):
        if k % 8 == 7:
            raws.append(valid[(k // 8) % 3])
        where.append((len(raws), row))
        raws.append(cases.tampered(valid[1], row[1]))
    return raws, where


def write_images(raws, path):
    from toyni_amd import verifier
    n = int(raws[0]["trace_len"])
    with open(path, "wb") as f:
        f.write(struct.pack("<II", n, len(raws)))
        for r in raws:
            f.write(verifier.pack_fib_proof(r))
    return path


def run_driver(path, *args, contracts_header=None):
    res = subprocess.run([build_sim_fib_verify(contracts_header), path, *args], capture_output=True, text=True, timeout=600)
    return res.returncode, res.stdout, res.stderr


def judge(raws, where, out):
    from toyni_amd import verifier
    words = [int(w) for w in re.search(r"^VERDICTS (.*)$", out, re.M).group(1).split()]
    assert len(words) == len(raws)
    flags = dict((int(m.group(1)), m.group(2)) for m in re.finditer(r"^FLAGS (\d+) ([01?]+)$", out, re.M))
    tampered_at = {at for at, _ in where}
    for b, raw in enumerate(raws):
        if b not in tampered_at:
            assert words[b] == 0, f"valid proof at {b}: {verifier.decode_verdict(words[b])}"
        assert flags[b] == cases.expected_flags(raw), f"record words of proof {b}"
    for at, (label, _fn, query, layer, fixed) in where:
        got = verifier.decode_verdict(words[at])
        if label == "op and op_pair swapped":   # the one row where the position binding answers before the reference's check
            assert cases.expected_of(raws[at]) == (False, "fri_consistency") and got[1:] == ("fri_merkle", query, layer), got
            continue
        cases.check_verdict(label, got, raws[at], query, layer, fixed)


@pytest.mark.parametrize("n", [8, 16])
def test_the_tamper_matrix_under_all_eight_schedules(n, tmp_path):
    raws, where = batch_of(n)
    rc, out, err = run_driver(write_images(raws, str(tmp_path / "images.bin")))
    assert rc == 0 and "ALL OK" in out and "hard failures=0" in out, out[-3000:] + err[-2000:]
    assert len(re.findall(r"^SCHEDULE \S+ failures=0$", out, re.M)) == 8, out[-2000:]
    assert {line[4:] for line in out.splitlines() if line.startswith("RAN ")} == set(KERNELS)
    judge(raws, where, out)


@lru_cache(maxsize=None)
def _run_256(tmp):
    raws, where = batch_of(256, full=False)
    path = write_images(raws, os.path.join(tmp, "images256.bin"))
    return raws, where, path, run_driver(path)


def test_nine_folds_and_a_final_layer_of_sixteen(tmp_path_factory):
    raws, where, _, (rc, out, err) = _run_256(str(tmp_path_factory.getbasetemp()))
    assert rc == 0 and "ALL OK" in out and "hard failures=0" in out, out[-3000:] + err[-2000:]
    assert "folds=9 final_size=16" in out
    judge(raws, where, out)


def test_every_synchronisation_site_is_needed_or_argued(tmp_path_factory):
    _, _, path, (rc, out, _) = _run_256(str(tmp_path_factory.getbasetemp()))
    assert rc == 0
    sites = {(m.group(1), int(m.group(2))): m.group(3) for m in re.finditer(r"^SITE (\w+):(\d+) (\S+) arrivals=(\d+)$", out, re.M)}
    assert {k: sum(1 for s in sites if s[0] == k) for k in KERNELS} == {k: SITES.get(k, 0) for k in KERNELS}, sorted(sites.items())
    assert all(text.startswith("wave_order@") for text in sites.values()), sites
    assert all(key in sites for key in ARGUED)
    order = sorted(sites)
    with ThreadPoolExecutor(max_workers=8) as ex:
        outs = list(ex.map(lambda s: run_driver(path, "--drop", "%s:%d" % s), order))
    wrong = []
    for key, (rc, o, e) in zip(order, outs):
        m = re.search(r"^DROP %s:%d \S+ (FAILS|SURVIVES)" % key, o, re.M)
        if rc != 0 or not m:
            wrong.append("%s:%d %s: the mutation run broke\n%s" % (key + (sites[key], (o + e)[-1500:])))
        elif m.group(1) == "FAILS" and key in ARGUED:
            wrong.append("%s:%d %s is argued as invisible (%s) but a schedule does fail without it" % (key + (sites[key], ARGUED[key])))
        elif m.group(1) == "SURVIVES" and key not in ARGUED:
            wrong.append("%s:%d %s can be dropped and every schedule still matches: the cases cannot see what it protects" % (key + (sites[key],)))
    assert not wrong, "\n".join(wrong)
