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

    python3 tools/scanbench.py [--repeats 15] [--batch 20] > profiles/column_scan.txt

--ext: the same method for the accumulator columns under an Ext challenge (include/toyni_hip.h 3i), toyni_column_scan_ext_device and
toyni_batch_inverse_ext_device, into profiles/column_scan_ext.txt.  Cases: the (1, 1) permutation form (two base columns, shift gamma,
product), the (1, 1) LogUp form (numerator shift 0, sum) and the (4, 4) form with each op, on 1 x 2^20, 4 x 2^20 and 1 x 2^24 Ext
elements, and the inversion on 2^24.  Beside each:
    copy    a copy of HALF the words the call moves: steps 1 and 3 each read every operand word and step 3 writes 4 words per element
            -- (1, 1): 8 words per element, (4, 4): 20, the inversion 8
    alu     VALU instructions of the shipped kernels per element, steps 1 + 3 (tools/isa_hist.py <listing> <kernel> --without
            'global_(load|store)_dword ' on the 16-byte path; a thread owns 4 elements): sum 2708 + 2872, product 3421 + 3939,
            inversion 811 per thread, over 27 T lane-ops/s.  The count holds the blocks of all eight operand forms, of which a call
            takes one, so it is an UPPER bound of what a call issues (a (1, 1) call forms no tower inverse, a (4, 4) call no norm form).
and the two conditions that need no floor:
    an Ext sum with a width-4 numerator and no denominator is coordinate-wise the base scan, so it runs beside toyni_column_scan_device
    on 4 x batch base columns in the same windows;
    one call on 4 Ext columns runs beside 4 calls on one.
EXPECTED FOR --ext, written before the first run: every form with a denominator is bound by arithmetic, not traffic (an Ext quotient
is 60 - 100 Montgomery products per element and step, several times the 8 - 20 words it moves), and the static count overstates the
path taken by about a third (§8f found a quarter with three forms; here there are eight): the call is expected at 0.5 - 1.0 x the
arithmetic floor as counted at 4 x 2^20 and 1 x 2^24, i.e. <= 1.0; the inversion <= 2.0 x the larger of its two floors, as in 3g.  At
1 x 2^20 the three dependent launches dominate: expected worse, <= 3 x.  The (4, 0) sum is expected within the min .. max spread of the
base scan on 4 x batch columns (same traffic, the same 12 words per element, but a group of 4 and four words per cross-lane step: if
anything this is where it shows).  One call on 4 Ext columns is expected faster than 4 calls on one.

    python3 tools/scanbench.py --ext [--repeats 15] [--batch 20] > profiles/column_scan_ext.txt"""
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
EXT_LANE_OPS = {"sum": (2708 + 2872) / 4, "product": (3421 + 3939) / 4, "inverse": 811 / 4}
EXT_EXPECT = {"large": 1.0, "one column of 2^20": 3.0, "inverse": 2.0}      # ratio to the larger floor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--head-copies", type=int, default=12, help="copies of 2^26 words enqueued ahead of every timed window (about 0.15 ms each)")
    ap.add_argument("--ext", action="store_true", help="the Ext calls of 3i instead of the base calls of 3g")
    args = ap.parse_args()
    if args.ext:
        return main_ext(args)
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


def main_ext(args):
    import torch
    import toyni_amd
    from csrc_hash import csrc_sha256
    lib = toyni_amd._lib.lib
    pv = toyni_amd.prover
    assert toyni_amd.gpu_available(), "scanbench needs the GPU: there is no fallback"
    dev = torch.device("cuda", 0)
    big = 1 << 24
    num = torch.randint(1, P, (4 * big,), dtype=torch.int32, device=dev)
    den = torch.randint(1, P, (4 * big,), dtype=torch.int32, device=dev)
    out = torch.empty(4 * big, dtype=torch.int32, device=dev)
    src, dst = torch.empty(1 << 28, dtype=torch.int32, device=dev), torch.empty(1 << 28, dtype=torch.int32, device=dev)
    tot = torch.empty(64, dtype=torch.int32, device=dev)
    ctx = toyni_amd.NttContext(1 << 10)
    stream = torch.cuda.current_stream().cuda_stream
    gamma = (1234567, 7654321, 99, 2013265920)

    def ext(op, nw, nshift, dw, n, batch, first=0):
        init = [(1, 0, 0, 0)] * batch
        a = pv.ExtOperand(num.data_ptr() + 4 * first * nw * n, n, nw, nshift) if nw else None
        b = pv.ExtOperand(den.data_ptr() + 4 * first * dw * n, n, dw, gamma) if dw else None
        return lambda: pv.column_scan_ext_device(ctx, a, b, out.data_ptr() + 16 * first * n, n, n, batch, op, init, tot.data_ptr() + 32 * first, stream=stream)

    def four(op, nw, nshift, dw, n):
        calls = [ext(op, nw, nshift, dw, n, 1, first=b) for b in range(4)]
        return lambda: [c() for c in calls]

    def base(n, columns):
        init = [0] * columns
        return lambda: pv.column_scan_device(ctx, num.data_ptr(), 0, out.data_ptr(), n, columns, pv.SCAN_SUM, init, tot.data_ptr(), stream=stream)

    def copy(words):
        return lambda: lib.toyni_memcpy_d2d_async(dst.data_ptr(), src.data_ptr(), 4 * words, stream)

    zero = (0, 0, 0, 0)
    forms = [("perm (1,1) product", pv.SCAN_PRODUCT, 1, gamma, 1, 8, "product"), ("logup (1,1) sum", pv.SCAN_SUM, 1, zero, 1, 8, "sum"),
             ("(4,4) sum", pv.SCAN_SUM, 4, gamma, 4, 20, "sum"), ("(4,4) product", pv.SCAN_PRODUCT, 4, gamma, 4, 20, "product")]
    shapes = [(1, 1 << 20), (4, 1 << 20), (1, 1 << 24)]
    cases, rows, pairs = [], [], []
    for kind, op, nw, nshift, dw, traffic, alu in forms:
        for batch, n in shapes:
            label = f"{kind} {batch}x2^{n.bit_length() - 1}"
            cases += [(label, ext(op, nw, nshift, dw, n, batch)), (label + " copy", copy(traffic * n * batch // 2))]
            single = None
            if batch == 4:
                single = label + " as 4 calls"
                cases.append((single, four(op, nw, nshift, dw, n)))
            rows.append((label, label + " copy", EXT_LANE_OPS[alu], n * batch, "one column of 2^20" if batch * n == 1 << 20 else "large", single))
    cases += [("inverse 2^24", lambda: pv.batch_inverse_ext_device(den.data_ptr(), big, out.data_ptr(), big, big, tot.data_ptr(), stream=stream)),
              ("inverse 2^24 copy", copy(4 * big))]
    rows.append(("inverse 2^24", "inverse 2^24 copy", EXT_LANE_OPS["inverse"], big, "inverse", None))
    for batch, n in shapes:                          # the condition that needs no floor: a (4, 0) sum beside the base scan on 4 x batch columns
        label = f"(4,0) sum {batch}x2^{n.bit_length() - 1}"
        cases += [(label, ext(pv.SCAN_SUM, 4, zero, 0, n, batch)), (label + " base", base(n, 4 * batch))]
        pairs.append((label, label + " base"))

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
    ref = "(4,4) sum 1x2^24 copy"
    spread = (max(samples[ref]) - min(samples[ref])) / med[ref]
    print(f"# tools/scanbench.py --ext  tile = {pv.column_scan_ext_tile()}, {args.repeats} repeats of {args.batch} calls enqueued behind {args.head_copies} copies, interleaved; times in ms")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    print(f"# csrc_sha256: {csrc_sha256()}")
    print(f"# spread of '{ref}' (max - min) / median = {100 * spread:.1f} %" + ("  (> 5 %: repeat before judging)" if spread > 0.05 else ""))
    print("# expected before the first run (ratio to the larger of the copy and the arithmetic floor): " + ", ".join(f"{k} <= {v}" for k, v in EXT_EXPECT.items()))
    print("# expected before the first run: (4,0) sum within the min .. max of the base scan on 4 x batch columns; one call on 4 Ext columns faster than 4 calls on one")
    print(f"{'case':30s} {'median':>9s} {'min':>9s} {'max':>9s} {'copy':>9s} {'alu':>9s}  note")
    ok = True
    for label, cp, lane_ops, elements, kind, single in rows:
        s = samples[label]
        alu = lane_ops * elements / 27e12 * 1e3
        ratio = med[label] / max(alu, med[cp])
        note = f"{med[label] / med[cp]:.2f} x copy; {ratio:.2f} x the larger floor, expected <= {EXT_EXPECT[kind]}: {'held' if ratio <= EXT_EXPECT[kind] else 'NOT held'}"
        if single:
            faster = med[label] < med[single]
            ok = ok and faster
            note += f"; 4 calls on one column take {med[single]:.4f} ({med[single] / med[label]:.2f} x): {'held' if faster else 'NOT held'}"
        print(f"{label:30s} {statistics.median(s):9.4f} {min(s):9.4f} {max(s):9.4f} {med[cp]:9.4f} {alu:9.4f}  {note}")
    for label, other in pairs:
        s, b = samples[label], samples[other]
        inside = min(b) <= med[label] <= max(b)
        print(f"{label:30s} {statistics.median(s):9.4f} {min(s):9.4f} {max(s):9.4f} {'':>9s} {'':>9s}  base scan on 4 x batch columns: {med[other]:.4f} "
              f"({min(b):.4f} .. {max(b):.4f}); {med[label] / med[other]:.2f} x; within its spread: {'held' if inside else 'NOT held'}")
    ctx.destroy()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
