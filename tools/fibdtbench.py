#!/usr/bin/env python3
"""The two compiled Fibonacci provers in ONE session (include/toyni_hip.h 3q):

    build/fib_prove                      toyni::fib::Prover: host transcript, six synchronisations per proof
    build/fib_prove_dt --in-flight 1     toyni::fib::StreamProver: device transcript, one synchronisation
    build/fib_prove_dt --in-flight 2, 4  several StreamProvers enqueued from one thread, then collected: ms per proof

Per trace length the four configurations alternate inside every round, so that clock drift hits all of them; a process proves once to
warm up (contexts, tables, buffers) and then --reps timed proofs, wall time around generate_proof / around enqueue-all + collect-all.
Reported: the median of all timed proofs of a configuration (rounds x reps, at least 15), min and max beside it, and for the stream
prover the median time per proof that the one thread spent inside enqueue().

    python3 tools/fibdtbench.py [--sizes 256,4096,65536] [--rounds 3] [--reps 6] [--out profiles/fib_prove_dt.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(exe, args):
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    if res.returncode != 0 or not lines:
        raise RuntimeError(f"{exe} {args}: exit {res.returncode}\n{res.stdout[-1000:]}{res.stderr[-1000:]}")
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,4096,65536")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fib_prove_dt.txt"))
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build_hip()
    host, dt = entry.build_fib_prove(), entry.build_fib_prove_dt()
    configs = [("fib_prove", host, []), ("fib_prove_dt in-flight 1", dt, ["--in-flight", 1]), ("fib_prove_dt in-flight 2", dt, ["--in-flight", 2]),
               ("fib_prove_dt in-flight 4", dt, ["--in-flight", 4])]
    lines = [f"# tools/fibdtbench.py --sizes {a.sizes} --rounds {a.rounds} --reps {a.reps}: ms per proof, median [min .. max] of rounds x reps warm proofs,",
             "# the configurations alternating inside every round"]
    for n in (int(s) for s in a.sizes.split(",")):
        ms = {name: [] for name, _, _ in configs}
        enq = {name: [] for name, _, _ in configs}
        counts = {}
        for rnd in range(a.rounds):
            for name, exe, extra in configs:
                out = run(exe, [n, 11 + rnd, a.reps] + extra)
                ms[name] += out["ms" if exe == host else "ms_per_proof"]
                enq[name] += out.get("enqueue_ms_per_proof", [])
                counts[name] = out["pcie"]
        base = statistics.median(ms["fib_prove"])
        for name, _, _ in configs:
            v = ms[name]
            med = statistics.median(v)
            c = counts[name]
            host_part = f"; of which inside enqueue() {statistics.median(enq[name]):.4f} ms" if enq[name] else ""
            lines.append(f"n=2^{n.bit_length() - 1:<2} {name:<26} {med:8.4f} ms  [{min(v):.4f} .. {max(v):.4f}]  x{base / med:5.2f} of fib_prove  "
                         f"({len(v)} proofs; d2h copies {c['d2h_copies']}, synchronisations {c.get('synchronisations', 'not counted: 6 in the source')}{host_part})")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
