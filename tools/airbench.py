#!/usr/bin/env python3
"""Constraint programs on the device (include/toyni_hip.h 3f), N = 2^21, B = 32.

Per repeat, in this order, so that clock drift hits every side:
    fib        toyni_fib_quotient_device (c and q written)                                      -- the yardstick, unchanged
    air-fib    toyni_air_quotient_device with the 13-instruction Fibonacci program, weights {1}  -- reported as a ratio to fib
    syn(L,m)   synthetic programs over a 64-column matrix: 64 CELLs, then MUL and ADD at 1:m up to L instructions, one EMIT
Each figure is one event pair around BATCH back-to-back calls divided by BATCH, enqueued behind a few large copies so that the window
holds kernels running back to back and not the host's launch pace (as tools/deepbench.py).  The table holds the median over the
repeats and the spread.  For the synthetic programs it adds ns per point-instruction next to two floors:
    VALU   lane operations per point of the interpreter's MUL and ADD blocks in the shipped ISA (tools/isa_hist.py on the listing:
           20 + 3 and 12 + 3 VALU instructions per group of 4 points: the products or sums and three LDS addresses) over the 27 T lane-ops/s the pass kernels sustain
    LDS    the layout's traffic per instruction and group of 4 points -- two ds_read_b128 (4 LDS cycles per wave each) and one
           ds_write_b128 (13) -- over 256 CUs at --clock-ghz

    python3 tools/airbench.py [--log-n 21] [--repeats 15] [--batch 20] > profiles/air_quotient.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 2013265921
GEN_2_27 = 440564289
CELL, CONST, X, XINV, ADD, SUB, MUL, EMIT = range(8)


def fib_program(n):
    g = pow(GEN_2_27, (1 << 27) // n, P)
    return [(CELL, 0, 0, 0, 0), (CELL, 1, 1, 0, 0), (CELL, 2, 2, 0, 0), (ADD, 0, 1, 0, 0), (SUB, 0, 2, 0, 0), (X, 1, 0, 0, 0),
            (CONST, 2, 0, 0, pow(g, n - 1, P)), (SUB, 2, 1, 2, 0), (MUL, 0, 0, 2, 0), (CONST, 2, 0, 0, pow(g, n - 2, P)), (SUB, 2, 1, 2, 0),
            (MUL, 0, 0, 2, 0), (EMIT, 0, 0, 0, 0)]


def synthetic(length, adds_per_mul, nregs=16):
    """CELL of column k into register k mod nregs for 64 columns, then MUL / ADD (1 : adds_per_mul) over the registers, one EMIT."""
    insns = [(CELL, k % nregs, 0, 0, k) for k in range(64)]
    k = 0
    while len(insns) < length - 1:
        op = MUL if k % (1 + adds_per_mul) == 0 else ADD
        insns.append((op, k % nregs, (k + 1) % nregs, (k + 5) % nregs, 0))
        k += 1
    return insns + [(EMIT, 0, 0, 0, 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=21)
    ap.add_argument("--log-blowup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--head-copies", type=int, default=10, help="copies of 65 N words enqueued ahead of every timed window")
    ap.add_argument("--valu-per-mul", type=float, default=23 / 4, help="VALU instructions per point of the MUL block (tools/isa_hist.py)")
    ap.add_argument("--valu-per-add", type=float, default=15 / 4, help="VALU instructions per point of the ADD block")
    ap.add_argument("--lds-cycles", type=float, default=4 + 4 + 13, help="LDS cycles per wave (256 points) and instruction: 2 x ds_read_b128 + ds_write_b128")
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    args = ap.parse_args()
    import torch
    import toyni_amd
    from csrc_hash import csrc_sha256
    lib = toyni_amd._lib.lib
    prover = toyni_amd.prover
    assert toyni_amd.gpu_available(), "airbench needs the GPU: there is no fallback"
    dev = torch.device("cuda", 0)
    N, lb = 1 << args.log_n, args.log_blowup
    width = 64
    values = torch.randint(0, P, ((width + 1) * N,), dtype=torch.int32, device=dev)
    out = torch.empty((width + 1) * N, dtype=torch.int32, device=dev)
    c_out, q_out = out.data_ptr(), out.data_ptr() + 4 * N
    ctx = toyni_amd.NttContext(N)
    stream = torch.cuda.current_stream().cuda_stream
    shift = 7
    progs = {"air-fib": prover.AirProgram(ctx, fib_program(N >> lb))}
    shapes = [(256, 1), (256, 3), (1024, 1), (1024, 3)]
    for length, m in shapes:
        progs[f"syn({length},1:{m})"] = prover.AirProgram(ctx, synthetic(length, m))

    def fib():
        prover.fib_quotient_device(ctx, values.data_ptr(), c_out, q_out, lb, shift, stream)

    def air(name, w):
        mats = [(values.data_ptr(), w, N)]
        return lambda: prover.air_quotient_device(ctx, progs[name], mats, lb, shift, [1], q_out, d_c_out=c_out, stream=stream)

    cases = [("fib", fib), ("air-fib", air("air-fib", 1))] + [(name, air(name, width)) for name in list(progs)[1:]]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.head_copies):            # keeps the stream busy while the window's calls are issued
            lib.toyni_memcpy_d2d_async(out.data_ptr() + 8 * N, values.data_ptr(), 4 * (width - 1) * N, stream)
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
    print(f"# tools/airbench.py  N = 2^{args.log_n}, B = {1 << lb}, {args.repeats} repeats of {args.batch} calls enqueued behind {args.head_copies} copies, interleaved; times in ms")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    print(f"# csrc_sha256: {csrc_sha256()}")
    print(f"# fib spread (max - min) / median = {100 * spread:.1f} %" + ("  (> 5 %: repeat before judging)" if spread > 0.05 else ""))
    print(f"{'case':16s} {'median':>9s} {'min':>9s} {'max':>9s}  note")
    lds_ns = args.lds_cycles / 256 / 256 / args.clock_ghz
    for name, _ in cases:
        s = samples[name]
        note = ""
        if name == "air-fib":
            note = f"ratio to fib {med[name] / med['fib']:.3f} (13 instructions, {progs[name].info.nregs} registers)"
        if name.startswith("syn("):
            info = progs[name].info
            m = int(name[:-1].split(":")[1])
            valu_ns = (args.valu_per_mul + m * args.valu_per_add) / (1 + m) / 27e12 * 1e9
            per = med[name] * 1e6 / N / info.ninsns
            note = (f"{per:.5f} ns per point-instruction; floors: VALU {valu_ns:.5f}, LDS {lds_ns:.5f}; ratio to the larger {per / max(valu_ns, lds_ns):.2f} "
                    f"({info.nregs} registers)")
        print(f"{name:16s} {statistics.median(s):9.4f} {min(s):9.4f} {max(s):9.4f}  {note}")
    for p in progs.values():
        p.destroy()
    ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
