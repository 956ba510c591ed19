#!/usr/bin/env python3
"""gamma and the constraint weights on the host and on the device (include/toyni_hip.h 3p).

Two measurements, both in ONE session, the sides of a comparison alternating inside every repeat so that clock drift hits both:

  A. per call, the _dc entry point against the host-argument entry point it is defined by:
       quotient  the staged AIR of tests/harness (16 base constraints, main 4 x N, accumulators 8 x N, B = 4) at N = 2^20:
                 toyni_air_quotient_ext_device under air_ext_weights(alphas) on the program with gamma as constants, against
                 toyni_air_quotient_ext_dc_device (TOYNI_AIR_WEIGHTS_EMIT_EXT) on the program with gamma as parameters 0..3
       scan      the permutation product (gamma + a) / (gamma + b) at n = 2^20: toyni_column_scan_ext_device against _dc_device
     A _dc call launches its one-wave preparation kernel ahead of the hot kernels, so each call is also timed at a shape where the
     hot kernels have nothing to do (N = 4; n = 4), both forms each:
       hot-kernel difference = (dc - host)[large] - (dc - host)[tiny],   preparation kernel + boundary = (dc - host)[tiny]
     Each figure is one event pair around --batch back-to-back calls behind a few large copies (tools/dzbench.py's window), divided
     by --batch.  VERDICT per call: the record-fed twins must not be slower than the argument-fed kernels by more than the run-to-run
     spread this tool measures on the argument-fed call, (max - min) / median over the repeats.  A miss is printed, not tuned away.
  B. the window "main columns committed -> quotient root absorbed" of a staged-AIR proof, B = 4, N = 2^12, 2^16, 2^20:
       host     steps 1-3 of tests/harness/air_ext_dz_prover.py as they stand: DOWNLOAD of the main root, gamma on the host
                transcript, two scans, the accumulators' commitment, DOWNLOAD of its root, the alphas, toyni_air_program_create
                (blocking), four toyni_air_quotient_device calls, the commitment, DOWNLOAD of its root -- three synchronisations
       device   absorb_device, squeeze, two _dc scans, the commitment, absorb_device, squeeze, ONE _dc quotient call on the program
                created once, the commitment, absorb_device -- none; one after the closing event
     one event pair around one window, started on an idle stream; and the WHOLE proof both ways (tests/harness/air_ext_dz_prover.py
     against air_ext_dc_prover.py, wall clock around prove(): trace upload, salts and the final downloads included in both).

The medians of --repeats (>= 20) runs after a warm-up of every shape; spreads are printed beside them.

    python3 tools/dcbench.py [--repeats 25] [--batch 40] [--out profiles/air_dc.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

P = 2013265921
MAIN_W, ACC_W, Q_W, NUM_WEIGHTS = 4, 8, 4, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--batch", type=int, default=40)
    ap.add_argument("--head-copies", type=int, default=12)
    ap.add_argument("--sizes", type=int, nargs="*", default=[12, 16, 20], help="log2 N of the window measurement")
    ap.add_argument("--proof-repeats", type=int, default=7, help="whole proofs per side and size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "air_dc.txt"))
    args = ap.parse_args()
    assert args.repeats >= 20, "the medians are of at least 20 runs"
    import numpy as np
    import torch
    import toyni_amd
    import ext_model as em
    from csrc_hash import csrc_sha256
    from harness import air_ext_dc_prover, air_ext_dz_prover
    from harness.air_ext_prover import constraint_program, coordinate_weights
    from harness.air_ext_verifier import squeeze_ext
    from harness.fib_verifier import COSET_SHIFT, Transcript
    pv, lib = toyni_amd.prover, toyni_amd._lib.lib
    assert toyni_amd.gpu_available(), "dcbench needs the GPU: there is no fallback"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    COL = toyni_amd.ROWS_COLUMN_MAJOR
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def rand(words):
        return torch.randint(0, P, (words,), dtype=torch.int32, device=dev)

    def empty(words):
        return torch.empty(words, dtype=torch.int32, device=dev)

    def pair(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3          # microseconds

    emit(f"# tools/dcbench.py  {args.repeats} repeats, interleaved; times in microseconds; median (min .. max)")
    emit(f"# device: {torch.cuda.get_device_name(0)}")
    emit(f"# csrc_sha256: {csrc_sha256()}")
    fmt = lambda s: f"{statistics.median(s):9.1f} ({min(s):8.1f} .. {max(s):8.1f})"
    spread = lambda s: (max(s) - min(s)) / statistics.median(s)
    rng = np.random.default_rng(5)
    gamma = tuple(int(v) for v in rng.integers(1, P, 4))
    alphas = [tuple(int(v) for v in rng.integers(0, P, 4)) for _ in range(NUM_WEIGHTS)]
    chal = torch.from_numpy(np.array([gamma] + alphas, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
    d_gamma, d_alphas = chal.data_ptr(), chal.data_ptr() + 16
    weights4 = toyni_amd.air_ext_weights(alphas)

    # ---- A. per call ----
    emit("")
    emit(f"A. per call, {args.batch} calls back to back behind {args.head_copies} copies; N = n = 2^20")
    N, log_b = 1 << 20, 2
    big, tiny = toyni_amd.NttContext(N), toyni_amd.NttContext(4)
    main_lde, acc_lde, q = rand(MAIN_W * N), rand(ACC_W * N), empty(Q_W * N)
    cols, acc = rand(2 * N), empty(4 * N)
    filler_src, filler_dst = rand(16 * N), empty(16 * N)
    progs = {"big c": pv.AirProgram(big, constraint_program(gamma)), "big p": pv.AirProgram(big, air_ext_dc_prover.constraint_program_params(), params=True),
             "tiny c": pv.AirProgram(tiny, constraint_program(gamma)), "tiny p": pv.AirProgram(tiny, air_ext_dc_prover.constraint_program_params(), params=True)}
    mats = lambda size: [(main_lde.data_ptr(), MAIN_W, size), (acc_lde.data_ptr(), ACC_W, size)]
    quo_host = lambda ctx, key, size, lb: pv.air_quotient_ext_device(ctx, progs[key], mats(size), lb, COSET_SHIFT, weights4, q.data_ptr(), size, stream=stream)
    quo_dc = lambda ctx, key, size, lb: pv.air_quotient_ext_dc_device(ctx, progs[key], mats(size), lb, COSET_SHIFT, d_gamma, 4, d_alphas, NUM_WEIGHTS,
                                                                      pv.AIR_WEIGHTS_EMIT_EXT, q.data_ptr(), size, stream=stream)
    scan_host = lambda size: pv.column_scan_ext_device(big, pv.ExtOperand(cols.data_ptr(), size, 1, gamma), pv.ExtOperand(cols.data_ptr() + 4 * N, size, 1, gamma),
                                                       acc.data_ptr(), size, size, 1, pv.SCAN_PRODUCT, [em.ONE], stream=stream)
    scan_dc = lambda size: pv.column_scan_ext_dc_device(big, pv.ExtOperandDc(cols.data_ptr(), size, 1, 0), pv.ExtOperandDc(cols.data_ptr() + 4 * N, size, 1, 0),
                                                        d_gamma, acc.data_ptr(), size, size, 1, pv.SCAN_PRODUCT, [em.ONE], stream=stream)
    cases = {
        "quot  host large": lambda: quo_host(big, "big c", N, log_b), "quot  dc   large": lambda: quo_dc(big, "big p", N, log_b),
        "quot  host tiny": lambda: quo_host(tiny, "tiny c", 4, 1), "quot  dc   tiny": lambda: quo_dc(tiny, "tiny p", 4, 1),
        "scan  host large": lambda: scan_host(N), "scan  dc   large": lambda: scan_dc(N),
        "scan  host tiny": lambda: scan_host(4), "scan  dc   tiny": lambda: scan_dc(4),
    }

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.head_copies):
            lib.toyni_memcpy_d2d_async(filler_dst.data_ptr(), filler_src.data_ptr(), 4 * 16 * N, stream)
        a.record()
        for _ in range(args.batch):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.batch

    for fn in cases.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for fn in cases.values():
        window(fn)
    samples = {k: [] for k in cases}
    for _ in range(args.repeats):
        for k, fn in cases.items():
            samples[k].append(window(fn))
    for k, s in samples.items():
        emit(f"{k:18s} {fmt(s)}   spread {100 * spread(s):.1f} %")
    med = {k: statistics.median(s) for k, s in samples.items()}
    for kind, what in (("quot ", "air_quotient_ext_dc_kernel"), ("scan ", "extcol_{aggregate,apply}_dc_kernel")):
        prep = med[f"{kind} dc   tiny"] - med[f"{kind} host tiny"]
        whole = med[f"{kind} dc   large"] - med[f"{kind} host large"]
        diff = whole - prep
        allowed = spread(samples[f"{kind} host large"]) * med[f"{kind} host large"]
        emit(f"{what}: the _dc call costs {whole:+.1f} us more than the host-argument call; preparation kernel + boundary {prep:.1f} us; hot-kernel "
             f"difference {diff:+.1f} us = {100 * diff / med[kind + ' host large']:+.2f} % of the argument-fed call; allowed (its own spread) {allowed:.1f} us: "
             f"{'ok' if diff <= allowed else 'NOT HELD'}")
    for p in progs.values():
        p.destroy()
    big.destroy(), tiny.destroy()
    del main_lde, acc_lde, q, cols, acc, filler_src, filler_dst

    # ---- B. the window, and the whole proof ----
    emit("")
    emit("B. main columns committed -> quotient root absorbed, B = 4: one event pair around one window")
    emit(f"{'N':>6s} {'host transcript':>34s} {'device transcript':>34s}  ratio  spread host / device")
    proofs = []
    for log_N in args.sizes:
        N, log_b = 1 << log_N, 2
        n = N >> log_b
        ctx_n, ctx_N = toyni_amd.ntt.get_or_create_ctx(n), toyni_amd.ntt.get_or_create_ctx(N)
        vals = rand(MAIN_W * n)
        salts = torch.randint(0, 256, (N, 16), dtype=torch.uint8, device=dev)
        levels = {k: torch.empty((lib.toyni_merkle_total_digests(N), 32), dtype=torch.uint8, device=dev) for k in ("main", "acc", "q")}
        coef, lde = {"main": empty(MAIN_W * n), "acc": empty(ACC_W * n)}, {"main": empty(MAIN_W * N), "acc": empty(ACC_W * N)}
        accs, qq, ch = empty(ACC_W * n), empty(Q_W * N), empty(4 + 4 * NUM_WEIGHTS)
        col = lambda c: vals.data_ptr() + 4 * c * n
        prog_p = air_ext_dc_prover.program_for(ctx_N)                            # once per AIR
        dtr = pv.DeviceTranscript()
        root = lambda k: bytes(levels[k][-1].cpu().numpy().tobytes())            # 32 bytes D2H: synchronises the stream
        two = lambda: [(lde["main"].data_ptr(), MAIN_W, N), (lde["acc"].data_ptr(), ACC_W, N)]

        def commit(name, d_columns, width):
            ctx_n.run_device(d_columns, coef[name].data_ptr(), width, True, stream=stream)
            ctx_N.lde_device(coef[name].data_ptr(), lde[name].data_ptr(), width, log_b, COSET_SHIFT, stream=stream)
            toyni_amd.merkle_commit_rows_device(lde[name].data_ptr(), N, width, COL, N, salts.data_ptr(), levels[name].data_ptr(), stream=stream)

        def host_window():
            tr = Transcript()
            tr.absorb(root("main"))
            g_ = squeeze_ext(tr)
            pv.column_scan_ext_device(ctx_n, pv.ExtOperand(col(0), n, 1, g_), pv.ExtOperand(col(1), n, 1, g_), accs.data_ptr(), n, n, 1, pv.SCAN_PRODUCT,
                                      [em.ONE], stream=stream)
            pv.column_scan_ext_device(ctx_n, pv.ExtOperand(col(2), n, 1, em.ZERO), pv.ExtOperand(col(3), n, 1, g_), accs.data_ptr() + 16 * n, n, n, 1,
                                      pv.SCAN_SUM, [em.ZERO], stream=stream)
            commit("acc", accs.data_ptr(), ACC_W)
            tr.absorb(root("acc"))
            al = [squeeze_ext(tr) for _ in range(NUM_WEIGHTS)]
            with pv.AirProgram(ctx_N, constraint_program(g_)) as prog:
                for c, wts in enumerate(coordinate_weights(al)):
                    pv.air_quotient_device(ctx_N, prog, two(), log_b, COSET_SHIFT, wts, qq.data_ptr() + 4 * c * N, stream=stream)
                toyni_amd.merkle_commit_rows_device(qq.data_ptr(), N, Q_W, COL, N, salts.data_ptr(), levels["q"].data_ptr(), stream=stream)
                tr.absorb(root("q"))
            return tr.state

        def device_window():
            dtr.absorb_device(levels["main"][-1].data_ptr(), 32, stream)
            dtr.squeeze(ch.data_ptr(), 4, stream)
            pv.column_scan_ext_dc_device(ctx_n, pv.ExtOperandDc(col(0), n, 1, 0), pv.ExtOperandDc(col(1), n, 1, 0), ch.data_ptr(), accs.data_ptr(), n, n, 1,
                                         pv.SCAN_PRODUCT, [em.ONE], stream=stream)
            pv.column_scan_ext_dc_device(ctx_n, pv.ExtOperandDc(col(2), n, 1), pv.ExtOperandDc(col(3), n, 1, 0), ch.data_ptr(), accs.data_ptr() + 16 * n, n, n, 1,
                                         pv.SCAN_SUM, [em.ZERO], stream=stream)
            commit("acc", accs.data_ptr(), ACC_W)
            dtr.absorb_device(levels["acc"][-1].data_ptr(), 32, stream)
            dtr.squeeze(ch.data_ptr() + 16, 4 * NUM_WEIGHTS, stream)
            pv.air_quotient_ext_dc_device(ctx_N, prog_p, two(), log_b, COSET_SHIFT, ch.data_ptr(), 4, ch.data_ptr() + 16, NUM_WEIGHTS, pv.AIR_WEIGHTS_EMIT_EXT,
                                          qq.data_ptr(), N, stream=stream)
            toyni_amd.merkle_commit_rows_device(qq.data_ptr(), N, Q_W, COL, N, salts.data_ptr(), levels["q"].data_ptr(), stream=stream)
            dtr.absorb_device(levels["q"][-1].data_ptr(), 32, stream)

        def device_run():
            dtr.load(b"toyni-stark-v1", stream)
            return pair(device_window)

        commit("main", vals.data_ptr(), MAIN_W)
        want = host_window()                             # warm-up, and the two sides agree on the transcript they leave
        for _ in range(3):
            host_window(), device_run()
        got, status = dtr.download()
        assert (got, status) == (want, 0), "the device window leaves another transcript than the host window"
        host, devc = [], []
        for _ in range(args.repeats):
            host.append(pair(host_window))
            devc.append(device_run())
        emit(f"2^{log_N:<4d} {fmt(host)} {fmt(devc)}  {statistics.median(host) / statistics.median(devc):5.2f}  {100 * spread(host):.0f} % / {100 * spread(devc):.0f} %")
        dtr.free()
        # the whole proof, both harnesses, wall clock around prove() (it ends with its own synchronisation and downloads)
        main = rng.integers(0, P, (MAIN_W, n), dtype=np.uint64)                  # the provers assert nothing about the trace
        wall = {"dz": [], "dc": []}
        for rep in range(args.proof_repeats + 1):
            for key, mod in (("dz", air_ext_dz_prover), ("dc", air_ext_dc_prover)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                proof = mod.prove(main, log_b, 1)
                dt = (time.perf_counter() - t0) * 1e6
                if rep:                                                          # the first of each is the warm-up
                    wall[key].append(dt)
                del proof
        proofs.append(f"2^{log_N:<4d} {fmt(wall['dz'])} {fmt(wall['dc'])}  {statistics.median(wall['dz']) / statistics.median(wall['dc']):5.2f}")
        del mod.EVENTS[:], air_ext_dz_prover.EVENTS[:]
    emit("")
    emit(f"   the whole proof, wall clock around prove(), {args.proof_repeats} runs each, interleaved")
    emit(f"{'N':>6s} {'quotient root onward (3o)':>34s} {'first root onward (3p)':>34s}  ratio")
    for line in proofs:
        emit(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0          # a verdict that is not held is a finding to record, not a failure of the tool


if __name__ == "__main__":
    sys.exit(main())
