#!/usr/bin/env python3
"""The multi-column DEEP combination and the batched out-of-domain evaluation (include/toyni_hip.h 3e), device-resident, N = 2^21, B = 32.

Per repeat, in this order, so that clock drift hits every side:
    fib        toyni_fib_deep_device (trace and quotient = columns 0 and 1 of one allocation)    -- the baseline
    generic4   toyni_deep_combine_device with the four Fibonacci terms                          -- bound: 1.25 x fib
    copy(w)    toyni_memcpy_d2d_async of (w + 1) N words                                        -- the memory floor of width w
    deep(w)    toyni_deep_combine_device, w columns x rotations {0, 1, 2}, w in {8, 64}
    eval64x1   64 calls of toyni_poly_eval_device on 2^16 coefficients at 3 points
    evalbatch  one toyni_poly_eval_batch_device on the same 64 columns
and the same two steps under Ext challenges (include/toyni_hip.h 3h), each next to its base form of the same run:
    copyx(w)      toyni_memcpy_d2d_async of (w + 4) N / 2 words: the traffic of deep_ext(w) -- w N words read, 4 N written -- as a
                  copy, which reads and writes every word it moves
    deep_ext(w)   toyni_deep_combine_ext_device, the same 3 w (column, rotation) terms as deep(w), Ext z / weights / values
    evalext_batch one toyni_poly_eval_ext_batch_device on the 64 columns at 2 Ext points
Each figure is one event pair around BATCH back-to-back calls divided by BATCH.  The calls of a window are enqueued while the stream is
still busy with a few large copies placed ahead of the first event, so the window holds kernels running back to back and not the
host's launch pace (a 13 us kernel is shorter than one call takes to issue).  The table holds the median over the repeats and the
spread (min .. max).  The arithmetic floor of deep(w) is --lane-ops-per-term x 3 w N / 27e12 (the lane operations per term and point
of the shipped ISA, tools/isa_hist.py, over the 27 T lane-ops/s the pass kernels sustain).  The one of deep_ext(w) is
(--ext-lane-ops-per-term x 3 w + --ext-lane-ops-per-point) x N / 27e12: under Ext challenges the part of a point that does not grow
with the table (adj_z and m_z by Horner, the shared inversion, the closing Ext product) is as large as a dozen terms and is counted.

EXPECTED of deep_ext(w), written before the first run; "ok" or "not held" is printed beside each, and neither changes the exit status:
  (1) no slower than FOUR deep(w) calls of the same run -- what the four coordinates of its numerators alone would cost through the
      base entry point, reading the matrix four times;
  (2) its ratio to the larger of the copy floor copyx(w) and the arithmetic floor is reported as 3e reports its own; from the counts,
      w = 8 is expected to sit on the arithmetic floor (24 terms + the per-point part against 12 N words that stay in the Infinity
      Cache: at most 1.5 x the larger floor) and w = 64 between the two (at most 2 x the larger floor, where deep(64) takes 1.6 x
      its arithmetic floor).

    python3 tools/deepbench.py [--log-n 21] [--repeats 15] [--batch 50] > profiles/deep_ext.txt    (profiles/deep_columns.txt: the run before 3h)"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 2013265921
# deep_combine_ext_kernel.  Per term: tools/isa_hist.py <listing> deep_combine_ext_kernel --loop --without 'global_load_dword ' counts 256
# VALU instructions per iteration of 4 terms x 4 points (80 v_mad_u64_u32, 80 v_add_u32, 48 v_min_u32, 16 v_mul_lo_u32, 32 for addresses
# and moves).  Per point, outside the term loops, counted from the source at the listing's 5 instructions per Montgomery product and 6
# per two-term dot product: 130 products (adj_z and m_z by Horner 44, the domain points 5, Montgomery's trick 12, the Fermat chain 41,
# the scaling of adj_z 16, the multiples of 11 for the Ext product 12), 32 dot products and 84 additions per thread of 4 points =
# 1010.  (The static count of everything outside the loop, 1466, also holds the tail loop and the single-point path of N < 4.)
EXT_LANE_OPS_PER_TERM = 256 / 16
EXT_LANE_OPS_PER_POINT = 1010 / 4
EXT_EXPECT = {8: 1.5, 64: 2.0}      # expectation (2): deep_ext(w) / max(copy floor, arithmetic floor)


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
    ap.add_argument("--ext-lane-ops-per-term", type=float, default=EXT_LANE_OPS_PER_TERM,
                    help="the same count for deep_combine_ext_kernel's term loop: VALU instructions per iteration of 4 terms x 4 points, over 16")
    ap.add_argument("--ext-lane-ops-per-point", type=float, default=EXT_LANE_OPS_PER_POINT,
                    help="VALU instructions of deep_combine_ext_kernel outside its term loops (16-byte path), over the 4 points of a thread")
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

    def wide_ext_terms(w):
        cols = [c for c in range(w) for _ in range(3)]
        rots = [r for _ in range(w) for r in range(3)]
        return prover.deep_ext_terms(cols, rots, rng.integers(1, P, (3 * w, 4)), rng.integers(0, P, (3 * w, 4)))

    wide = {w: wide_terms(w) for w in (8, 64)}
    wide_ext = {w: wide_ext_terms(w) for w in (8, 64)}
    z_ext = [z, 2 * z % P, 3 * z % P, 5 * z % P]
    points_ext = np.array([z_ext, [5 * z % P, z, 7 * z % P, 1]], dtype=np.uint32)
    ev_out_ext = torch.empty(4 * 2 * 64, dtype=torch.int32, device=dev)
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

    def deep_ext(terms, w):
        return lambda: prover.deep_combine_ext_device(ctx, values.data_ptr(), w, N, lb, shift, z_ext, terms, out.data_ptr(), stream=stream)

    def copyx(w):
        return lambda: lib.toyni_memcpy_d2d_async(out.data_ptr(), values.data_ptr(), 4 * ((w + 4) * N // 2), stream)

    def eval_ext_batch():
        prover.poly_eval_ext_batch_device(ctx, values.data_ptr(), nco, nco, ncols, points_ext, ev_out_ext.data_ptr(), stream)

    cases = [("fib", fib), ("generic4", deep(fib_terms, 2))]
    for w in (8, 64):
        cases += [(f"copy({w})", copy(w)), (f"deep({w})", deep(wide[w], w)), (f"copyx({w})", copyx(w)), (f"deep_ext({w})", deep_ext(wide_ext[w], w))]
    cases += [("eval64x1", eval_single), ("evalbatch", eval_batch), ("evalext_batch", eval_ext_batch)]

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
    print(f"{'case':13s} {'median':>9s} {'min':>9s} {'max':>9s}  note")
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
        if name.startswith("deep_ext("):
            w = int(name[9:-1])
            four, mem = 4 * med[f"deep({w})"], med[f"copyx({w})"]
            alu = (args.ext_lane_ops_per_term * 3 * w + args.ext_lane_ops_per_point) * N / 27e12 * 1e3
            r = med[name] / max(mem, alu)
            note = (f"(1) four deep({w}) {four:.4f}: {'ok' if med[name] <= four else 'not held'}; (2) copy floor {mem:.4f}, arithmetic floor {alu:.4f} "
                    f"({args.ext_lane_ops_per_term} lane-ops/term + {args.ext_lane_ops_per_point}/point), ratio to the larger {r:.2f}, "
                    f"expected <= {EXT_EXPECT[w]}: {'ok' if r <= EXT_EXPECT[w] else 'not held'}")
        if name == "evalext_batch":
            note = f"{med[name] / med['evalbatch']:.1f}x evalbatch (2 Ext points against 3 base points)"
        if name == "evalbatch":
            faster = med[name] < med["eval64x1"]
            ok = ok and faster
            note = f"{med['eval64x1'] / med[name]:.1f}x the 64 single calls: {'ok' if faster else 'MISS'}"
        print(f"{name:13s} {statistics.median(s):9.4f} {min(s):9.4f} {max(s):9.4f}  {note}")
    ctx.destroy()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
