#!/usr/bin/env python3
"""From "quotient root absorbed" to "DEEP root absorbed" with the transcript on the host and on the device (include/toyni_hip.h 3o).

Two measurements, both in ONE session, the sides of a comparison alternating inside every repeat so that clock drift hits both:

  A. the segment of tests/harness/air_ext_prover.py between the two roots, with that harness's 24 DEEP terms (4 main columns, 8
     accumulator columns at z and g z, 4 quotient columns), blow-up 4, N = 2^12, 2^16, 2^20:
       host     derive_z on a host transcript; toyni_poly_eval_ext_batch_device x 3 with host points; DOWNLOAD of the 24 values; host
                absorb and 96 host squeezes; toyni_deep_combine_ext_device x 3 with host terms; the row commitment; DOWNLOAD of its
                root; host absorb                                        -- two synchronisations in the window
       device   squeeze_ext_point; toyni_poly_eval_ext_batch_dz_device x 3; absorb_fields; one squeeze of 96 words;
                toyni_deep_combine_ext_dz_device x 3; the row commitment; absorb_device   -- none; one after the closing event
     One event pair around one segment; the window starts on an idle stream, as it does in a proof.
  B. the hot kernels at N = 2^20, device-record instantiation against the argument-fed one.  An entry point of 3o launches its
     one-wave preparation kernel ahead of the hot kernel, so a call is timed at the large shape and at a shape where the hot
     kernels have nothing to do (one coefficient; N = 4), both forms each:
       hot-kernel difference = (dz - host)[large] - (dz - host)[tiny],   preparation kernel = (dz - host)[tiny]
     Each figure is one event pair around --batch back-to-back calls behind a few large copies (tools/deepbench.py's window: the
     kernels run back to back, the host's launch pace is not in it), divided by --batch.
     VERDICT printed per kernel: the device form must not be slower than the argument-fed one by more than the run-to-run spread
     this tool measures on the argument-fed one, (max - min) / median over the repeats.  A miss is printed as such, not tuned away.

The medians of --repeats (>= 20) runs after a warm-up of every shape; spreads are printed beside them.

    python3 tools/dzbench.py [--repeats 25] [--batch 40] [--out profiles/deep_dz.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

P = 2013265921
MAIN_W, ACC_W, Q_W = 4, 8, 4
TERMS = [("main", c, 0) for c in range(MAIN_W)] + [("acc", c, r) for c in range(ACC_W) for r in (0, 1)] + [("quotient", c, 0) for c in range(Q_W)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--batch", type=int, default=40)
    ap.add_argument("--head-copies", type=int, default=12)
    ap.add_argument("--sizes", type=int, nargs="*", default=[12, 16, 20], help="log2 N of the segment measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_dz.txt"))
    args = ap.parse_args()
    assert args.repeats >= 20, "the medians are of at least 20 runs"
    import numpy as np
    import torch
    import toyni_amd
    from csrc_hash import csrc_sha256
    from harness.fib_verifier import Transcript, root_of_unity
    from harness.air_ext_verifier import absorb_ext, derive_z, squeeze_ext
    pv, lib = toyni_amd.prover, toyni_amd._lib.lib
    assert toyni_amd.gpu_available(), "dzbench needs the GPU: there is no fallback"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    COL, ROW = toyni_amd.ROWS_COLUMN_MAJOR, toyni_amd.ROWS_ROW_MAJOR
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def rand(words):
        return torch.randint(0, P, (words,), dtype=torch.int32, device=dev)

    def pair(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3          # microseconds

    emit(f"# tools/dzbench.py  {args.repeats} repeats, interleaved; times in microseconds; median (min .. max)")
    emit(f"# device: {torch.cuda.get_device_name(0)}")
    emit(f"# csrc_sha256: {csrc_sha256()}")
    fmt = lambda s: f"{statistics.median(s):9.1f} ({min(s):8.1f} .. {max(s):8.1f})"
    spread = lambda s: (max(s) - min(s)) / statistics.median(s)

    # ---- A. the segment ----
    emit("")
    emit("A. quotient root absorbed -> DEEP root absorbed, 24 terms, B = 4: one event pair around one segment")
    emit(f"{'N':>6s} {'host transcript':>34s} {'device transcript':>34s}  ratio  spread host / device")
    for log_N in args.sizes:
        N, log_b = 1 << log_N, 2
        n = N >> log_b
        g = root_of_unity(log_N - log_b)
        ctx_n, ctx_N = toyni_amd.NttContext(n), toyni_amd.NttContext(N)
        coef = {"main": rand(MAIN_W * n), "acc": rand(ACC_W * n), "quotient": rand(Q_W * N)}
        lde = {"main": (rand(MAIN_W * N), MAIN_W), "acc": (rand(ACC_W * N), ACC_W), "quotient": (rand(Q_W * N), Q_W)}
        ood, deep, z_dev, w_dev = (torch.empty(k, dtype=torch.int32, device=dev) for k in (4 * len(TERMS), 4 * N, 4, 4 * len(TERMS)))
        salts = torch.randint(0, 256, (N, 16), dtype=torch.uint8, device=dev)
        levels = torch.empty((lib.toyni_merkle_total_digests(N), 32), dtype=torch.uint8, device=dev)
        state0 = Transcript()
        state0.absorb(b"\x5a" * 96)                                           # three roots' worth of history
        slots = {name: pv.deep_ext_slots(*zip(*[(c, r, t, t) for t, (mat, c, r) in enumerate(TERMS) if mat == name])) for name in lde}
        dtr = pv.DeviceTranscript()

        def evals(point_args, fn):
            fn(ctx_n, coef["main"].data_ptr(), n, n, MAIN_W, *point_args([1]), ood.data_ptr(), stream=stream)
            fn(ctx_n, coef["acc"].data_ptr(), n, n, ACC_W, *point_args([1, g]), ood.data_ptr() + 16 * MAIN_W, stream=stream)
            fn(ctx_N, coef["quotient"].data_ptr(), N, N, Q_W, *point_args([1]), ood.data_ptr() + 16 * (MAIN_W + 2 * ACC_W), stream=stream)

        def host_segment():
            tr = Transcript()
            tr.state = state0.state
            z = derive_z(tr)
            evals(lambda mults: ([tuple(c * m % P for c in z) for m in mults],), pv.poly_eval_ext_batch_device)
            vals = [tuple(int(c) for c in v) for v in ood.cpu().numpy().view(np.uint32).reshape(-1, 4)]       # download 1
            for v in vals:
                absorb_ext(tr, v)
            ws = [squeeze_ext(tr) for _ in TERMS]
            for k, (name, (values, width)) in enumerate(lde.items()):
                mine = [(c, r, wt, val) for (mat, c, r), wt, val in zip(TERMS, ws, vals) if mat == name]
                pv.deep_combine_ext_device(ctx_N, values.data_ptr(), width, N, log_b, 7, z, pv.deep_ext_terms(*zip(*mine)), deep.data_ptr(), accumulate=k > 0,
                                           stream=stream)
            toyni_amd.merkle_commit_rows_device(deep.data_ptr(), N, 4, ROW, 0, salts.data_ptr(), levels.data_ptr(), stream=stream)
            tr.absorb(bytes(levels[-1].cpu().numpy().tobytes()))                                              # download 2
            return tr.state

        def device_segment():
            dtr.squeeze_ext_point(z_dev.data_ptr(), stream)
            evals(lambda mults: (z_dev.data_ptr(), mults), pv.poly_eval_ext_batch_dz_device)
            dtr.absorb_fields(ood.data_ptr(), 4 * len(TERMS), stream)
            dtr.squeeze(w_dev.data_ptr(), 4 * len(TERMS), stream)
            for k, (name, (values, width)) in enumerate(lde.items()):
                pv.deep_combine_ext_dz_device(ctx_N, values.data_ptr(), width, N, log_b, 7, z_dev.data_ptr(), w_dev.data_ptr(), ood.data_ptr(), slots[name],
                                              deep.data_ptr(), accumulate=k > 0, stream=stream)
            toyni_amd.merkle_commit_rows_device(deep.data_ptr(), N, 4, ROW, 0, salts.data_ptr(), levels.data_ptr(), stream=stream)
            dtr.absorb_device(levels[-1].data_ptr(), 32, stream)

        def device_run():
            dtr.load(state0.state, stream)
            return pair(device_segment)

        want = host_segment()                            # warm-up, and the two sides agree on the transcript they leave
        for _ in range(3):
            host_segment(), device_run()
        got, status = dtr.download()
        assert (got, status) == (want, 0), "the device segment leaves another transcript than the host segment"
        host, devc = [], []
        for _ in range(args.repeats):
            host.append(pair(host_segment))
            devc.append(device_run())
        emit(f"2^{log_N:<4d} {fmt(host)} {fmt(devc)}  {statistics.median(host) / statistics.median(devc):5.2f}  {100 * spread(host):.0f} % / {100 * spread(devc):.0f} %")
        dtr.free()
        ctx_n.destroy(), ctx_N.destroy()

    # ---- B. the hot kernels ----
    emit("")
    emit(f"B. per call, {args.batch} calls back to back behind {args.head_copies} copies; N = 2^20")
    N, log_b = 1 << 20, 2
    big, tiny = toyni_amd.NttContext(N), toyni_amd.NttContext(4)
    values, out = rand(ACC_W * N), torch.empty(4 * N, dtype=torch.int32, device=dev)
    filler_src, filler_dst = rand(16 * N), torch.empty(16 * N, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(3)
    z = [int(v) for v in rng.integers(1, P, 4)]
    z_dev = torch.tensor(z, dtype=torch.int32, device=dev)
    g = root_of_unity(18)
    nterms = 2 * ACC_W
    al, cl = rng.integers(0, P, (nterms, 4)), rng.integers(0, P, (nterms, 4))
    al_dev, cl_dev = (torch.from_numpy(a.astype(np.uint32).view(np.int32).reshape(-1)).to(dev) for a in (al, cl))
    cols, rots = [c for c in range(ACC_W) for _ in (0, 1)], [r for _ in range(ACC_W) for r in (0, 1)]
    terms, slots = pv.deep_ext_terms(cols, rots, al, cl), pv.deep_ext_slots(cols, rots, range(nterms), range(nterms))
    terms0, slots0 = pv.deep_ext_terms(cols, [0] * nterms, al, cl), pv.deep_ext_slots(cols, [0] * nterms, range(nterms), range(nterms))
    ev = torch.empty(4 * 2 * ACC_W, dtype=torch.int32, device=dev)
    pts = [z, [c * g % P for c in z]]
    cases = {
        "eval  host large": lambda: pv.poly_eval_ext_batch_device(big, values.data_ptr(), N, N, ACC_W, pts, ev.data_ptr(), stream=stream),
        "eval  dz   large": lambda: pv.poly_eval_ext_batch_dz_device(big, values.data_ptr(), N, N, ACC_W, z_dev.data_ptr(), [1, g], ev.data_ptr(), stream=stream),
        "eval  host tiny": lambda: pv.poly_eval_ext_batch_device(big, values.data_ptr(), 1, 1, 1, pts, ev.data_ptr(), stream=stream),
        "eval  dz   tiny": lambda: pv.poly_eval_ext_batch_dz_device(big, values.data_ptr(), 1, 1, 1, z_dev.data_ptr(), [1, g], ev.data_ptr(), stream=stream),
        "deep  host large": lambda: pv.deep_combine_ext_device(big, values.data_ptr(), ACC_W, N, log_b, 7, z, terms, out.data_ptr(), stream=stream),
        "deep  dz   large": lambda: pv.deep_combine_ext_dz_device(big, values.data_ptr(), ACC_W, N, log_b, 7, z_dev.data_ptr(), al_dev.data_ptr(), cl_dev.data_ptr(),
                                                                  slots, out.data_ptr(), stream=stream),
        "deep  host tiny": lambda: pv.deep_combine_ext_device(tiny, values.data_ptr(), ACC_W, 4, 0, 7, z, terms0, out.data_ptr(), stream=stream),
        "deep  dz   tiny": lambda: pv.deep_combine_ext_dz_device(tiny, values.data_ptr(), ACC_W, 4, 0, 7, z_dev.data_ptr(), al_dev.data_ptr(), cl_dev.data_ptr(),
                                                                 slots0, out.data_ptr(), stream=stream),
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
    for kind, what in (("eval ", "poly_eval_ext_batch_{partial,final}_dz_kernel"), ("deep ", "deep_combine_ext_dz_kernel")):
        prep = med[f"{kind} dz   tiny"] - med[f"{kind} host tiny"]
        diff = med[f"{kind} dz   large"] - med[f"{kind} host large"] - prep
        allowed = spread(samples[f"{kind} host large"]) * med[f"{kind} host large"]
        held = diff <= allowed
        emit(f"{what}: preparation kernel {prep:.1f} us; hot-kernel difference {diff:+.1f} us = {100 * diff / med[kind + ' host large']:+.2f} % of the "
             f"argument-fed call; allowed (its own spread) {allowed:.1f} us: {'ok' if held else 'NOT HELD'}")
    big.destroy(), tiny.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0          # a verdict that is not held is a finding to record, not a failure of the tool


if __name__ == "__main__":
    sys.exit(main())
