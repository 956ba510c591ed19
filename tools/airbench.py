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

    python3 tools/airbench.py [--log-n 21] [--repeats 15] [--batch 20] > profiles/air_quotient.txt

--ext: the quotient under Ext weights (include/toyni_hip.h 3k).  ONE toyni_air_quotient_ext_device call against the FOUR
toyni_air_quotient_device calls it replaces (one per coordinate of the weights, each writing its own q column, no c), same program,
matrices and output buffer, both in every repeat, interleaved, each window timed as above.  Programs, all with 16 EMITs:
    staged     the sixteen base constraints of the staged AIR (four Ext constraints written with emit_ext) over its 4 + 8 columns
    syn16(L,m) the synthetic programs above with 16 EMITs of registers 0..15 in place of the one
The prediction, written before the first run, from the VALU instructions per group of 4 points of each interpreter block in the
shipped ISA (tools/isa_hist.py on the two kernels' listings; --valu-* below): the base kernel interprets the program four times,
the Ext kernel once with an EMIT block that holds three more products per point,
    predicted ratio = (sum over the program of the Ext kernel's blocks) / (4 x the same sum over the base kernel's blocks)
It counts issue slots alone: instruction decoding (scalar), LDS and cell traffic are paid once against four times as well, and the
Ext kernel's 76 VGPRs against 40 cost occupancy where the register file in LDS does not already bound it.

    python3 tools/airbench.py --ext > profiles/air_quotient_ext.txt"""
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
# --ext: VALU instructions per group of 4 points of the interpreter's other blocks, counted in the listing of the shipped kernels
# (hipcc -S, the blocks of the 4-point loop of air_quotient_kernel and air_quotient_ext_kernel; MUL 23 and ADD / SUB 15 as above).
# CELL: the 16-byte load path, 10 of address arithmetic + 4 conversions of 5.  XINV: one Fermat chain shared by the four points.
# EMIT: base 4 products + 4 sums with a select each (4 blocks of 11-13 + 2-3); Ext 16 products + 16 sums in one block of 129.
VALU_CELL, VALU_CONST, VALU_XINV, VALU_EMIT_BASE, VALU_EMIT_EXT = 30, 12, 290, 57, 129


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


def synthetic16(length, adds_per_mul, nregs=16):
    """synthetic() with 16 EMITs, constraint k = register k, all divided, in place of the one: `length` instructions in all."""
    return synthetic(length - 15, adds_per_mul, nregs)[:-1] + [(EMIT, 0, k, 0, k) for k in range(16)]


def staged_program(prover, gamma):
    """The staged AIR's four Ext constraints (a permutation product Z and a LogUp sum S under gamma, their boundary constraints divided
    through XINV): matrix 0 the four main columns, matrix 1 the accumulators Z (columns 0..3) and S (4..7).  Sixteen base constraints."""
    bld = prover.AirBuilder()
    g = bld.ext_const(gamma)
    a, b, u, w = (bld.cell(0, c) for c in range(4))
    zc, zn, sc, sn = bld.ext_cell(1, 0, 0), bld.ext_cell(1, 0, 1), bld.ext_cell(1, 4, 0), bld.ext_cell(1, 4, 1)
    bld.emit_ext(0, zn * (g + b) - zc * (g + a))
    bld.emit_ext(1, (sn - sc) * (g + w) - u)
    bld.emit_ext(2, (zc - 1) * bld.xinv(1), divide=False)
    bld.emit_ext(3, sc * bld.xinv(1), divide=False)
    return bld.compile()


def predicted_ratio(insns, args):
    """VALU instructions per group of 4 points: one Ext interpretation over four base interpretations."""
    block = {CELL: args.valu_cell, CONST: args.valu_const, X: args.valu_const, XINV: args.valu_xinv, ADD: args.valu_per_add * 4, SUB: args.valu_per_add * 4,
             MUL: args.valu_per_mul * 4}
    common = sum(block[i[0]] for i in insns if i[0] != EMIT)
    emits = sum(1 for i in insns if i[0] == EMIT)
    return (common + emits * args.valu_emit_ext) / (4 * (common + emits * args.valu_emit_base))


def main_ext(args):
    import numpy as np
    import torch
    import toyni_amd
    from csrc_hash import csrc_sha256
    lib = toyni_amd._lib.lib
    prover = toyni_amd.prover
    assert toyni_amd.gpu_available(), "airbench needs the GPU: there is no fallback"
    dev = torch.device("cuda", 0)
    N, lb = 1 << args.log_n, args.log_blowup
    width = 64
    values = torch.randint(0, P, (width * N,), dtype=torch.int32, device=dev)
    out = torch.empty(width * N, dtype=torch.int32, device=dev)
    q_out = out.data_ptr()
    ctx = toyni_amd.NttContext(N)
    stream = torch.cuda.current_stream().cuda_stream
    shift = 7
    rng = np.random.default_rng(0xE87)
    gamma = tuple(int(v) for v in rng.integers(0, P, 4))
    weights4 = rng.integers(0, P, (16, 4)).astype(np.uint32)
    columns = [np.ascontiguousarray(weights4[:, e]) for e in range(4)]
    programs = {"staged": (staged_program(prover, gamma), [(values.data_ptr(), 4, N), (values.data_ptr() + 4 * 4 * N, 8, N)])}
    for length, m in [(256, 1), (256, 3), (1024, 1), (1024, 3)]:
        programs[f"syn16({length},1:{m})"] = (synthetic16(length, m), [(values.data_ptr(), width, N)])
    progs = {name: prover.AirProgram(ctx, insns) for name, (insns, _) in programs.items()}
    predicted = {name: predicted_ratio(insns, args) for name, (insns, _) in programs.items()}      # before anything runs

    def one(name):
        mats = programs[name][1]
        return lambda: prover.air_quotient_ext_device(ctx, progs[name], mats, lb, shift, weights4, q_out, N, stream=stream)

    def four(name):
        mats = programs[name][1]

        def run():
            for e in range(4):
                prover.air_quotient_device(ctx, progs[name], mats, lb, shift, columns[e], q_out + 4 * e * N, stream=stream)
        return run

    cases = [(name, kind, fn(name)) for name in programs for kind, fn in (("one", one), ("four", four))]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.head_copies):            # keeps the stream busy while the window's calls are issued
            lib.toyni_memcpy_d2d_async(out.data_ptr() + 16 * N, values.data_ptr(), 4 * (width - 4) * N, stream)
        a.record()
        for _ in range(args.batch):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.batch

    for _, _, fn in cases:                           # warm-up: every shape, then one whole window each that is not kept
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _, _, fn in cases:
        timed(fn)
    samples = {(name, kind): [] for name, kind, _ in cases}
    for _ in range(args.repeats):
        for name, kind, fn in cases:
            samples[(name, kind)].append(timed(fn))
    print(f"# tools/airbench.py --ext  N = 2^{args.log_n}, B = {1 << lb}, {args.repeats} repeats of {args.batch} windows enqueued behind {args.head_copies} copies, "
          "interleaved; times in ms per window item (one call, or the four calls it replaces)")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    print(f"# csrc_sha256: {csrc_sha256()}")
    print(f"# predicted from VALU instructions per group of 4 points: CELL {args.valu_cell:g}, CONST / X {args.valu_const:g}, XINV {args.valu_xinv:g}, "
          f"ADD / SUB {args.valu_per_add * 4:g}, MUL {args.valu_per_mul * 4:g}, EMIT {args.valu_emit_base:g} (base) and {args.valu_emit_ext:g} (Ext)")
    print(f"{'program':18s} {'insns':>6s} {'regs':>5s} {'one':>9s} {'four':>9s} {'one/four':>9s} {'predicted':>10s} {'spread one':>11s} {'spread four':>12s}")
    worst = 0.0
    for name in programs:
        s1, s4 = samples[(name, "one")], samples[(name, "four")]
        m1, m4 = statistics.median(s1), statistics.median(s4)
        worst = max(worst, m1 / m4)
        info = progs[name].info
        print(f"{name:18s} {info.ninsns:6d} {info.nregs:5d} {m1:9.4f} {m4:9.4f} {m1 / m4:9.3f} {predicted[name]:10.3f} {100 * (max(s1) - min(s1)) / m1:10.1f}% "
              f"{100 * (max(s4) - min(s4)) / m4:11.1f}%")
    print(f"# largest one/four ratio: {worst:.3f}" + ("  -- the one call is NOT faster in every case" if worst >= 1.0 else ""))
    for p in progs.values():
        p.destroy()
    ctx.destroy()
    return 0


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
    ap.add_argument("--ext", action="store_true", help="the one call under Ext weights against the four base calls it replaces")
    ap.add_argument("--valu-cell", type=float, default=VALU_CELL, help="--ext: VALU instructions per group of 4 points of the CELL block")
    ap.add_argument("--valu-const", type=float, default=VALU_CONST, help="--ext: ... of the CONST / X block")
    ap.add_argument("--valu-xinv", type=float, default=VALU_XINV, help="--ext: ... of the XINV block")
    ap.add_argument("--valu-emit-base", type=float, default=VALU_EMIT_BASE, help="--ext: ... of the base kernel's EMIT block")
    ap.add_argument("--valu-emit-ext", type=float, default=VALU_EMIT_EXT, help="--ext: ... of the Ext kernel's EMIT block")
    args = ap.parse_args()
    if args.ext:
        return main_ext(args)
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
