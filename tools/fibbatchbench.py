#!/usr/bin/env python3
"""The three compiled Fibonacci provers in one process per configuration (include/toyni_hip.h 3s):

    (a) toyni::fib::Prover              host transcript, blocking
    (s) toyni::fib::StreamProver        device transcript, one synchronisation per proof
    (b) toyni::fib::BatchStreamProver   `batch` proofs in one chain of launches, one synchronisation per batch

tools/fibbatchbench.cpp holds all three; per (trace length, batch) one process first compares every proof of the batch with the
stream prover's proof of the same trace under the same key (and proof 0 with the blocking prover's), then alternates the three inside
every round: `reps` proofs of (a), `reps` of (s), `reps` batches of (b), wall time around calls that end in a synchronisation.
Reported per configuration: median, p10, p90 of all samples in ms PER PROOF (rounds x reps samples, at least 15), the prediction of
DESIGN.md 8r beside the batch's median with held / NOT HELD at +-25 %, and the two conditions of acceptance.

    python3 tools/fibbatchbench.py [--sizes 256,4096,65536] [--batches 1,4,16,64] [--rounds 6] [--reps 4] [--out profiles/fib_prove_batch.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# DESIGN.md 8r, written before the first timing run: the time of one batched call in microseconds, (b)(B) = (s)(1) + 30 + (B - 1) x work(n)
# + 6 x (launches of the openings - 1)
PREDICTED_US = {256: {1: 1073, 4: 1094, 16: 1178, 64: 1514}, 4096: {1: 1601, 4: 1817, 16: 2693, 64: 6185},
                65536: {1: 3276, 4: 6588, 16: 19830, 64: 72798}}


def build():
    import __graft_entry__ as entry
    entry.build_hip()
    out = os.path.join(ROOT, "build", "fibbatchbench")
    src = os.path.join(ROOT, "tools", "fibbatchbench.cpp")
    host = os.path.join(entry.CSRC, "host")
    deps = [src, entry.LIB] + [os.path.join(host, f) for f in os.listdir(host)]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-o", out, src, "-L", entry.LIB_DIR,
                               "-ltoyni_hip", f"-Wl,-rpath,{entry.LIB_DIR}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return out


def stats(v):
    q = statistics.quantiles(v, n=10)
    return statistics.median(v), q[0], q[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,4096,65536")
    ap.add_argument("--batches", default="1,4,16,64")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fib_prove_batch.txt"))
    a = ap.parse_args()
    exe = build()
    lines = [f"# tools/fibbatchbench.py --sizes {a.sizes} --batches {a.batches} --rounds {a.rounds} --reps {a.reps}: ms PER PROOF, median [p10 .. p90] of rounds x reps",
             "# samples; (a) blocking Prover, (s) StreamProver, (b) BatchStreamProver alternating inside every round of one process; the proofs of",
             "# the batch were compared with the stream prover's (and proof 0 with the blocking prover's) before the clock started"]
    verdicts = []
    for n in (int(s) for s in a.sizes.split(",")):
        for batch in (int(s) for s in a.batches.split(",")):
            res = subprocess.run([exe, str(n), str(batch), str(a.rounds), str(a.reps)], capture_output=True, text=True, timeout=900, cwd=ROOT)
            rows = [l for l in res.stdout.splitlines() if l.startswith("{")]
            out = json.loads(rows[-1]) if rows else {}
            if res.returncode != 0 or not out.get("equal"):
                lines.append(f"n=2^{n.bit_length() - 1} B={batch}: NOT MEASURED ({out.get('error', res.stderr[-300:].strip() or 'no output')})")
                print(lines[-1], flush=True)
                continue
            (am, a10, a90), (sm, s10, s90), (bm, b10, b90) = stats(out["a"]), stats(out["s"]), stats(out["b"])
            pred = PREDICTED_US.get(n, {}).get(batch)
            mark = ""
            if pred:
                off = (bm * batch * 1000 - pred) / pred
                mark = f"  batch {bm * batch * 1000:8.0f} us [{pred}] {'held' if abs(off) <= 0.25 else 'NOT HELD'} ({off:+.0%})"
            head = f"n=2^{n.bit_length() - 1:<2} B={batch:<3}"
            lines.append(f"{head} (a) {am:8.4f} [{a10:.4f} .. {a90:.4f}]  (s) {sm:8.4f} [{s10:.4f} .. {s90:.4f}]  (b) {bm:8.4f} [{b10:.4f} .. {b90:.4f}]  "
                         f"(a)/(b) {am / bm:6.2f}  (s)/(b) {sm / bm:6.2f}{mark}  ({len(out['b'])} samples; openings {out['open_launches']} launches; "
                         f"h2d {out['h2d_copies']}, d2h {out['d2h_copies']}, sync {out['synchronisations']})")
            print(lines[-1], flush=True)
            if batch == 1:
                ok = bm - sm <= s90 - s10
                verdicts.append(f"(i)  n=2^{n.bit_length() - 1}: (b)(1) - (s) = {1000 * (bm - sm):+.1f} us against the stream prover's own p10-p90 spread of "
                                f"{1000 * (s90 - s10):.1f} us: {'within it' if ok else 'MISSED'}")
            if n == 256 and batch == 16:
                ok = am - bm > a90 - a10
                verdicts.append(f"(ii) n=2^8, B=16: {1000 * bm:.1f} us per proof against the blocking prover's {1000 * am:.1f} (spread {1000 * (a90 - a10):.1f}): "
                                f"{am / bm:.1f} x: {'held' if ok else 'MISSED'}")
    lines += verdicts
    for v in verdicts:
        print(v, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
