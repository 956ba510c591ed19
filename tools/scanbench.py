#!/usr/bin/env python3
"""Accumulator columns (include/toyni_hip.h 3g), device-resident: toyni_column_scan_device and toyni_batch_inverse_device.

Cases: a sum without denominators, a sum with denominators and a product with both operands, each on 1 x 2^20, 16 x 2^20 and 1 x 2^24
elements, and the inversion alone on 2^24.  Beside each:
    copy    toyni_memcpy_d2d_async of HALF the words the call reads and writes in all its launches (a copy reads and writes each word it
            moves): 3 n per column without denominators (read twice, written once), 5 n with both operands, 2 n for the inversion
    alu     the arithmetic floor: VALU instructions per element of the shipped kernels (steps 1 and 3 together; tools/isa_hist.py
            <listing> <kernel> --without 'global_(load|store)_dword ' counts the 16-byte path of each: sum 651 + 689, product
            722 + 804, inversion 454 per thread of 8 elements -- the blocks of all three operand forms included, so an upper bound)
            over the 27 T lane-ops/s the pass kernels sustain.  A sum without denominators forms no inverse:
            its floor is the copy.
and, for the condition that needs no number, 16 calls on one column of 2^20 beside the one call on 16 columns.

Per repeat every case runs once, in this order, so that clock drift hits every side.  Each figure is one event pair around BATCH
back-to-back calls divided by BATCH; the calls of a window are enqueued while the stream is still busy with a few large copies placed
ahead of the first event, so the window holds kernels running back to back and not the host's launch pace.  One window of every case
is run and dropped before the kept ones.  The table holds the median over the repeats and the spread (min .. max).

EXPECTED, written before the first run: steps 1 and 3 each read every operand, so the call is at best 1.0 x its copy.  Without
denominators nothing but the traffic counts: at most 1.3 x the copy.  With denominators the arithmetic floor (about 170 - 190
lane-ops per element) is 1.2 - 1.4 x the copy at 4 TB/s, and the three launches do not overlap: at most 2.5 x the copy, and at most
2 x for the inversion alone.  At 1 x 2^20 the call is three launches of 10 - 20 us: the ratio there is expected to be worse.

    python3 tools/scanbench.py [--repeats 15] [--batch 20] > profiles/column_scan.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 2013265921
LANE_OPS = {"sum": (651 + 689) / 8, "product": (722 + 804) / 8, "inverse": 454 / 8}
EXPECT = {"sum, no den": 1.3, "sum": 2.5, "product": 2.5, "inverse": 2.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--head-copies", type=int, default=12, help="copies of 2^26 words enqueued ahead of every timed window (about 0.15 ms each)")
    args = ap.parse_args()
    import torch
    import toyni_amd
    from csrc_hash import csrc_sha256
    lib = toyni_amd._lib.lib
    pv = toyni_amd.prover
    assert toyni_amd.gpu_available(), "scanbench needs the GPU: there is no fallback"
    dev = torch.device("cuda", 0)
    big = 1 << 24
    num = torch.randint(1, P, (big,), dtype=torch.int32, device=dev)
    den = torch.randint(1, P, (big,), dtype=torch.int32, device=dev)
    out = torch.empty(big, dtype=torch.int32, device=dev)
    src, dst = torch.empty(1 << 26, dtype=torch.int32, device=dev), torch.empty(1 << 26, dtype=torch.int32, device=dev)
    tot = torch.empty(32, dtype=torch.int32, device=dev)
    ctx = toyni_amd.NttContext(1 << 10)
    stream = torch.cuda.current_stream().cuda_stream

    def scan(op, with_num, with_den, n, batch):
        init = [1] * batch
        return lambda: pv.column_scan_device(ctx, num.data_ptr() if with_num else 0, den.data_ptr() if with_den else 0, out.data_ptr(), n, batch, op,
                                             init, tot.data_ptr(), stream=stream)

    def sixteen(op, with_den, n):
        one = [1]

        def run():
            for b in range(16):
                pv.column_scan_device(ctx, num.data_ptr() + 4 * b * n, den.data_ptr() + 4 * b * n if with_den else 0, out.data_ptr() + 4 * b * n, n, 1,
                                      op, one, tot.data_ptr() + 8 * b, stream=stream)
        return run

    def copy(words):
        return lambda: lib.toyni_memcpy_d2d_async(dst.data_ptr(), src.data_ptr(), 4 * words, stream)

    kinds = [("sum, no den", pv.SCAN_SUM, False, 3, None), ("sum", pv.SCAN_SUM, True, 5, "sum"), ("product", pv.SCAN_PRODUCT, True, 5, "product")]
    shapes = [(1, 1 << 20), (16, 1 << 20), (1, 1 << 24)]
    cases, rows = [], []          # rows: (label, call case, copy case, lane-ops per element or None, elements, expectation key, 16 x 1 case)
    for kind, op, with_den, traffic, alu in kinds:
        for batch, n in shapes:
            label = f"{kind} {batch}x2^{n.bit_length() - 1}"
            cases += [(label, scan(op, True, with_den, n, batch)), (label + " copy", copy(traffic * n * batch // 2))]
            single = None
            if batch == 16:
                single = label + " as 16 calls"
                cases.append((single, sixteen(op, with_den, n)))
            rows.append((label, label + " copy", LANE_OPS[alu] if alu else None, n * batch, kind, single))
    cases += [("inverse 2^24", lambda: pv.batch_inverse_device(den.data_ptr(), out.data_ptr(), big, tot.data_ptr(), stream=stream)),
              ("inverse 2^24 copy", copy(big))]
    rows.append(("inverse 2^24", "inverse 2^24 copy", LANE_OPS["inverse"], big, "inverse", None))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.head_copies):            # keeps the stream busy while the window's calls are issued
            lib.toyni_memcpy_d2d_async(dst.data_ptr(), src.data_ptr(), 4 << 26, stream)
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
    ref = "sum 1x2^24 copy"
    spread = (max(samples[ref]) - min(samples[ref])) / med[ref]
    print(f"# tools/scanbench.py  tile = {pv.column_scan_tile()}, {args.repeats} repeats of {args.batch} calls enqueued behind {args.head_copies} copies, interleaved; times in ms")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    print(f"# csrc_sha256: {csrc_sha256()}")
    print(f"# spread of '{ref}' (max - min) / median = {100 * spread:.1f} %" + ("  (> 5 %: repeat before judging)" if spread > 0.05 else ""))
    print("# expected before the first run (ratio to the copy): " + ", ".join(f"{k} <= {v}" for k, v in EXPECT.items()) + "; worse at 1x2^20 (launch-bound)")
    print(f"{'case':24s} {'median':>9s} {'min':>9s} {'max':>9s} {'copy':>9s} {'alu':>9s}  note")
    ok = True
    for label, cp, lane_ops, elements, kind, single in rows:
        s = samples[label]
        alu = lane_ops * elements / 27e12 * 1e3 if lane_ops else None
        ratio = med[label] / med[cp]
        note = f"{ratio:.2f} x copy, expected <= {EXPECT[kind]}: {'held' if ratio <= EXPECT[kind] else 'NOT held'}"
        if alu:
            note += f"; {med[label] / max(alu, med[cp]):.2f} x the larger floor"
        if single:
            faster = med[label] < med[single]
            ok = ok and faster
            note += f"; 16 calls on one column take {med[single]:.4f} ({med[single] / med[label]:.2f} x): {'ok' if faster else 'MISS'}"
        print(f"{label:24s} {statistics.median(s):9.4f} {min(s):9.4f} {max(s):9.4f} {med[cp]:9.4f} {alu if alu else float('nan'):9.4f}  {note}")
    ctx.destroy()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
