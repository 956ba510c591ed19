#!/usr/bin/env python3
"""The multi-column DEEP combination and the batched out-of-domain evaluation (include/toyni_hip.h 3e), device-resident, N = 2^21, B = 32.

Per repeat, in this order, so that clock drift hits every side:
    fib        toyni_fib_deep_device (trace and quotient = columns 0 and 1 of one allocation)    -- the baseline
    generic4   toyni_deep_combine_device with the four Fibonacci terms                          -- bound: 1.25 x fib
    copy(w)    toyni_memcpy_d2d_async of (w + 1) N words                                        -- the memory floor of width w
    deep(w)    toyni_deep_combine_device, w columns x rotations {0, 1, 2}, w in {8, 64}
    eval64x1   64 calls of toyni_poly_eval_device on 2^16 coefficients at 3 points
    evalbatch  one toyni_poly_eval_batch_device on the same 64 columns
Each figure is one event pair around BATCH back-to-back calls divided by BATCH.  The calls of a window are enqueued while the stream is
still busy with a few large copies placed ahead of the first event, so the window holds kernels running back to back and not the
host's launch pace (a 13 us kernel is shorter than one call takes to issue).  The table holds the median over the repeats and the
spread (min .. max).  The arithmetic floor of deep(w) is --lane-ops-per-term x 3 w N / 27e12 (the lane operations per term and point
of the shipped ISA, tools/isa_hist.py, over the 27 T lane-ops/s the pass kernels sustain).

    python3 tools/deepbench.py [--log-n 21] [--repeats 15] [--batch 50] > profiles/deep_columns.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 2013265921


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=21)
    ap.add_argument("--log-blowup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--head-copies", type=int, default=25, help="copies of 65 N words enqueued ahead of every timed window (about 0.2 ms each)")
    ap.add_argument("--lane-ops-per-term", type=float, default=152 / 32,
                    help="VALU instructions per term and point of the shipped term loop: tools/isa_hist.py <listing> deep_combine_kernel --loop "
                         "--without 'global_load_dword ' counts 152 per iteration of 4 terms x 8 points (40 of them v_mad_u64_u32)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import toyni_amd
    from csrc_hash import csrc_sha256
    lib = toyni_amd._lib.lib
    prover = toyni_amd.prover
    assert toyni_amd.gpu_available(), "deepbench needs the GPU: there is no fallback"
    dev = torch.device("cuda", 0)
    N, lb = 1 << args.log_n, args.log_blowup
    max_w = 64
    values = torch.randint(0, P, ((max_w + 1) * N,), dtype=torch.int32, device=dev)
    out = torch.empty((max_w + 1) * N, dtype=torch.int32, device=dev)
    ctx = toyni_amd.NttContext(N)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(1)
    shift, z = 7, 123456789
    ood = [int(v) for v in rng.integers(0, P, 4)]
    fib_terms = prover.deep_terms([0, 0, 0, 1], [0, 1, 2, 0], [1, 1, 1, 1], ood)

    def wide_terms(w):
        cols = [c for c in range(w) for _ in range(3)]
        rots = [r for _ in range(w) for r in range(3)]
        return prover.deep_terms(cols, rots, rng.integers(1, P, 3 * w), rng.integers(0, P, 3 * w))

    wide = {w: wide_terms(w) for w in (8, 64)}
    nco, ncols = 1 << 16, 64
    points = np.array([z, 5 * z % P, 25 * z % P], dtype=np.uint32)
    ev_out = torch.empty(3 * ncols, dtype=torch.int32, device=dev)

    def fib():
        prover.fib_deep_device(ctx, values.data_ptr(), values.data_ptr() + 4 * N, out.data_ptr(), lb, shift, z, ood, stream)

    def deep(terms, w):
        return lambda: prover.deep_combine_device(ctx, values.data_ptr(), w, N, lb, shift, z, terms, out.data_ptr(), stream=stream)

    def copy(w):
        return lambda: lib.toyni_memcpy_d2d_async(out.data_ptr(), values.data_ptr(), 4 * (w + 1) * N, stream)

    def eval_single():
        for b in range(ncols):
            prover.poly_eval_device(ctx, values.data_ptr() + 4 * b * nco, nco, points, ev_out.data_ptr() + 12 * b, stream)

    def eval_batch():
        prover.poly_eval_batch_device(ctx, values.data_ptr(), nco, nco, ncols, points, ev_out.data_ptr(), stream)

    cases = [("fib", fib), ("generic4", deep(fib_terms, 2))]
    for w in (8, 64):
        cases += [(f"copy({w})", copy(w)), (f"deep({w})", deep(wide[w], w))]
    cases += [("eval64x1", eval_single), ("evalbatch", eval_batch)]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.head_copies):            # keeps the stream busy while the window's calls are issued
            lib.toyni_memcpy_d2d_async(out.data_ptr(), values.data_ptr(), 4 * (max_w + 1) * N, stream)
        a.record()
        for _ in range(args.batch):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.batch

    for _, fn in cases:                              # warm-up: every shape, then one whole window each that is not kept
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _, fn in cases:
        timed(fn)
    samples = {name: [] for name, _ in cases}
    for _ in range(args.repeats):
        for name, fn in cases:
            samples[name].append(timed(fn))
    med = {k: statistics.median(v) for k, v in samples.items()}
    spread = (max(samples["fib"]) - min(samples["fib"])) / med["fib"]
    print(f"# tools/deepbench.py  N = 2^{args.log_n}, B = {1 << lb}, {args.repeats} repeats of {args.batch} calls enqueued behind {args.head_copies} copies, interleaved; times in ms")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    print(f"# csrc_sha256: {csrc_sha256()}")
    print(f"# fib spread (max - min) / median = {100 * spread:.1f} %" + ("  (> 5 %: repeat before judging)" if spread > 0.05 else ""))
    print(f"{'case':12s} {'median':>9s} {'min':>9s} {'max':>9s}  note")
    ok = True
    for name, _ in cases:
        s = samples[name]
        note = ""
        if name == "generic4":
            r = med[name] / med["fib"]
            ok = ok and r <= 1.25
            note = f"ratio to fib {r:.3f}, bound 1.250: {'ok' if r <= 1.25 else 'MISS'}"
        if name.startswith("deep("):
            w = int(name[5:-1])
            mem = med[f"copy({w})"]
            alu = args.lane_ops_per_term * 3 * w * N / 27e12 * 1e3
            note = f"memory floor {mem:.4f}, arithmetic floor {alu:.4f} ({args.lane_ops_per_term} lane-ops/term), ratio to the larger {med[name] / max(mem, alu):.2f}"
        if name == "evalbatch":
            faster = med[name] < med["eval64x1"]
            ok = ok and faster
            note = f"{med['eval64x1'] / med[name]:.1f}x the 64 single calls: {'ok' if faster else 'MISS'}"
        print(f"{name:12s} {statistics.median(s):9.4f} {min(s):9.4f} {max(s):9.4f}  {note}")
    ctx.destroy()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
