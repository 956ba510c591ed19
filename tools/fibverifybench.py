#!/usr/bin/env python3
"""The device verifier of include/toyni_hip.h 3t under device events: the sibling of tools/fibbatchbench.py.

Per (trace length, batch): four proofs of the batched device prover (build/fib_verify_batch writes them) are packed into images and
repeated round-robin up to `batch` -- the work of a verification does not depend on which valid proof it is -- and uploaded ONCE, before
the clock.  Timed with device events on one stream, after `--warmup` runs, `--reps` times each:
    chain     everything toyni_fib_verify_batch_device enqueues (five launches)
    records   toyni_merkle_verify_records_batch_device alone over the same F + 2 groups (the positions the chain left in the work buffer)
Every verdict of every timed run must be 0.  Reported: median [p10 .. p90] in microseconds, the PREDICTION beside each, HELD / NOT HELD
at +-25 %.  The prediction is computed here, from the layout alone, by `predict` -- the figures it rests on were recorded before this
tool existed (profiles/pow_grind.txt: 20.9 G compressions/s on a full chip; profiles/fri_phase_batch.txt / DESIGN.md 9: 6.5 us per
two-block node hash on a lone wave, so 3.25 us per dependent compression).

    python3 tools/fibverifybench.py [--sizes 256,4096,65536] [--batches 1,16,64] [--reps 10] [--warmup 3] [--out profiles/fib_verify_batch.txt] [--append]
Run the same command twice (the second time with --append) for the run-to-run spread."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

US_PER_COMPRESSION = 3.25          # a dependent SHA-256 compression on a lone wave (half of the 6.5 us two-block node hash)
CHIP_COMPRESSIONS_PER_US = 20.9e3  # profiles/pow_grind.txt
RESIDENT_LANES = 256 * 4 * 4 * 64  # 256 CUs x 4 SIMDs x occupancy 4 (the record kernel's resource line) x 64 lanes
LAUNCH_US = 5.0                    # a dependent launch on a warm stream (profiles/r02_launchbench.txt)
QUERY_US = 20.0                    # 44 lanes: F + 1 inversions of 41 products and F fold steps each, no hashing


def counts(lay):
    """Hash work of ONE image, from the layout alone: (dependent compressions of the transcript replay, compressions of the final
    layer's tree along its critical path, compressions of all records, compressions of the deepest record)."""
    F = lay.folds
    blocks = lambda nbytes: (nbytes + 9 + 63) // 64
    replay = blocks(14 + 64)                      # derive_z: the tag and two roots (one try)
    replay += blocks(32 + 32 + 32)                # beta_0: digest, four values, fri_commitments[0]
    replay += (F - 1) * blocks(32 + 32)           # beta_k: digest and root k
    replay += blocks(32 + 32) + 43                # 44 indices: digest and the last root, then one block a step (no repeats assumed)
    levels = lay.final_size.bit_length() - 1
    tree = 1 + 2 * levels
    depth = [lay.group_leaves[g].bit_length() - 1 for g in range(lay.ngroups)]
    records = sum(lay.group_records[g] * (1 + 2 * depth[g]) for g in range(lay.ngroups))
    return replay, tree, records, 1 + 2 * max(depth)


def predict(lay, batch):
    """(chain us, records us): the serial parts in a row; the record walk is its deepest path, once per round of resident lanes, or the
    chip's hash rate, whichever is longer."""
    replay, tree, records, deepest = counts(lay)
    rounds = -(-batch * lay.nrecords // RESIDENT_LANES)
    rec = max(rounds * deepest * US_PER_COMPRESSION, batch * records / CHIP_COMPRESSIONS_PER_US) + LAUNCH_US
    chain = replay * US_PER_COMPRESSION + tree * US_PER_COMPRESSION + rec + QUERY_US + 4 * LAUNCH_US
    return chain, rec


def device_proofs(n, count=4):
    import __graft_entry__ as entry
    from test_fib_prover_cpp import _load_proof
    exe = entry.build_fib_verify_batch()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "proof.json")
        res = subprocess.run([exe, str(n), "3", "0", str(count), path], capture_output=True, text=True, timeout=600, cwd=ROOT)
        out = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
        assert out.get("verdicts") == [0] * count, out
        return [_load_proof(f"{path}.{b}") for b in range(count)]


def stats(v):
    q = statistics.quantiles(v, n=10)
    return statistics.median(v), q[0], q[-1]


def judged(got, want):
    dev = (got - want) / want
    return ("held" if abs(dev) <= 0.25 else "NOT HELD") + " (%+d%%)" % round(100 * dev)


def measure(ta, n, batch, reps, warmup):
    import numpy as np
    import torch
    lib, v = ta._lib.lib, ta.verifier
    dev = torch.device("cuda", 0)
    lay = v.fib_proof_layout(n)
    imgs = [np.frombuffer(v.pack_fib_proof(p), dtype=np.uint8) for p in device_proofs(n)]
    host = np.concatenate([imgs[b % len(imgs)] for b in range(batch)])
    stride = lay.image_bytes
    images = torch.from_numpy(host.copy()).to(dev)
    work_bytes = lib.toyni_fib_verify_work_bytes(n, batch)
    work = torch.zeros(work_bytes, dtype=torch.uint8, device=dev)
    out = torch.zeros(batch, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    ctx = ta.NttContext(lay.lde_size)
    wstride = work_bytes // batch // 4
    pos = work.data_ptr() + 4 * 380
    groups, first = [], 0
    for g in range(lay.ngroups):
        groups.append(v.MerkleVerifyGroup(images.data_ptr() + lay.group_offset[g], stride, lay.group_records[g], lay.group_leaves[g], 1, pos + 4 * first, wstride,
                                          images.data_ptr() + 32 * g, stride, pos + 4 * (lay.nrecords + first), wstride))
        first += lay.group_records[g]
    arr = (v.MerkleVerifyGroup * lay.ngroups)(*groups)

    def chain():
        ta._lib.check(lib.toyni_fib_verify_batch_device(ctx.handle, images.data_ptr(), stride, n, batch, work.data_ptr(), out.data_ptr(), s.cuda_stream), "verify")

    def records():
        ta._lib.check(lib.toyni_merkle_verify_records_batch_device(arr, lay.ngroups, batch, s.cuda_stream), "verify records")

    def timed(fn):
        us = []
        for r in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                a.record(s)
                fn()
                b.record(s)
            b.synchronize()
            if r >= warmup:
                us.append(1000.0 * a.elapsed_time(b))
            assert not out.cpu().numpy().any(), "a valid proof was refused"
        return us

    try:
        t_chain = timed(chain)
        t_rec = timed(records)       # the positions of the last chain are still in the work buffer
        flags = work.cpu().numpy().view(np.uint32).reshape(batch, wstride)[:, 380 + lay.nrecords:380 + 2 * lay.nrecords]
        assert (flags == 1).all(), "the record call alone refused a record"
    finally:
        ctx.destroy()
    return lay, t_chain, t_rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,4096,65536")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fib_verify_batch.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--predict-only", action="store_true", help="print the predictions (no GPU needed)")
    a = ap.parse_args()
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd as ta
    sizes, batches = [int(x) for x in a.sizes.split(",")], [int(x) for x in a.batches.split(",")]
    lines = []
    if not a.append:
        lines += [f"# tools/fibverifybench.py --sizes {a.sizes} --batches {a.batches} --reps {a.reps} --warmup {a.warmup}: device events around the enqueued chain of",
                  "# toyni_fib_verify_batch_device (images resident, uploaded before the clock) and around toyni_merkle_verify_records_batch_device alone;",
                  "# microseconds, median [p10 .. p90]; [prediction] held / NOT HELD at +-25 %.  PREDICTED from the layout by predict() of the tool, before the run:",
                  "#   chain = (replay + final tree) dependent compressions x 3.25 us + records + 20 us of queries + 4 x 5 us of launches",
                  "#   records = max(rounds of 262 144 resident lanes x (1 + 2 depth) x 3.25 us, compressions / 20.9 G/s) + 5 us"]
        for n in sizes:
            lay = ta.verifier.fib_proof_layout(n)
            replay, tree, records, deepest = counts(lay)
            lines.append(f"#   n=2^{n.bit_length() - 1}: replay {replay} dependent compressions, final tree {tree}, records {records} per image (deepest path {deepest}); "
                         + ", ".join("B=%d chain %.0f records %.0f" % ((b,) + predict(lay, b)) for b in batches))
    if a.predict_only:
        print("\n".join(lines))
        return
    assert ta.gpu_available(), "no GPU visible"
    lines.append("# run 2 (the same command again)" if a.append else "# run 1")
    for n in sizes:
        for batch in batches:
            lay, t_chain, t_rec = measure(ta, n, batch, a.reps, a.warmup)
            pc, pr = predict(lay, batch)
            (mc, lc, hc), (mr, lr, hr) = stats(t_chain), stats(t_rec)
            line = (f"n=2^{n.bit_length() - 1:<2} B={batch:<3} chain {mc:8.1f} us [{lc:.1f} .. {hc:.1f}] [{pc:.0f}] {judged(mc, pc)}   "
                    f"records {mr:8.1f} us [{lr:.1f} .. {hr:.1f}] [{pr:.0f}] {judged(mr, pr)}   "
                    f"({a.reps} samples; {batch * lay.nrecords} records; {mc / batch:.1f} us per proof)")
            print(line, flush=True)
            lines.append(line)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
