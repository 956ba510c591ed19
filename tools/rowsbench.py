#!/usr/bin/env python3
"""Row-leaf Merkle commitment against the single-column one (include/toyni_hip.h 3d against 3b), device-resident, n = 2^21 salted.

Per repeat, in this order, so that clock drift hits both sides:
    T1        toyni_merkle_commit_device on one column             -- the yardstick
    Trows(w)  toyni_merkle_commit_rows_device, column-major w in {1, 8, 64}, row-major w in {4, 8}
Each figure is one event pair around BATCH back-to-back launches, divided by BATCH; the table holds the median over the repeats and
the spread (min .. max).  Model: C(w) = ceil((8 w + 26) / 64) + 2 compressions per row (leaf blocks + two per node), so
Trows(w) ~ T1 C(w) / 3.  Accepted: Trows(1) <= 1.05 T1 (or T1's own spread if that is larger), Trows(w) <= 1.25 T1 C(w) / 3.
`w x T1` is what w separate trees would cost (orientation only).

    python3 tools/rowsbench.py [--log-n 21] [--repeats 15] [--batch 10] > profiles/rows_commit.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 2013265921
COL, ROW = 0, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--batch", type=int, default=10)
    args = ap.parse_args()
    import torch
    import toyni_amd
    from csrc_hash import csrc_sha256
    lib = toyni_amd._lib.lib
    assert toyni_amd.gpu_available(), "rowsbench needs the GPU: there is no fallback"
    dev = torch.device("cuda", 0)
    n = 1 << args.log_n
    max_w = 64
    values = torch.randint(0, P, (max_w * n,), dtype=torch.int32, device=dev)
    salts = torch.empty(16 * n, dtype=torch.uint8, device=dev)
    import numpy as np
    key = np.arange(32, dtype=np.uint8)
    assert lib.toyni_chacha20_fill_device(salts.data_ptr(), 16 * n, key.ctypes.data, 1, None) == 0
    levels = torch.empty(32 * lib.toyni_merkle_total_digests(n), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()

    def single():
        assert lib.toyni_merkle_commit_device(values.data_ptr(), salts.data_ptr(), n, levels.data_ptr(), stream) == 0

    def rows(layout, w):
        def run():
            assert lib.toyni_merkle_commit_rows_device(values.data_ptr(), n, w, layout, n, salts.data_ptr(), levels.data_ptr(), stream) == 0
        return run

    cases = [("T1 single column", None, 1, single)]
    cases += [(f"rows column-major w={w}", "col", w, rows(COL, w)) for w in (1, 8, 64)]
    cases += [(f"rows row-major    w={w}", "row", w, rows(ROW, w)) for w in (4, 8)]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.batch):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.batch

    for _, _, _, fn in cases:                        # warm-up: every shape the timed window uses
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name, _, _, _ in cases}
    for _ in range(args.repeats):
        for name, _, _, fn in cases:                 # interleaved
            samples[name].append(timed(fn))

    t1 = statistics.median(samples["T1 single column"])
    t1_lo, t1_hi = min(samples["T1 single column"]), max(samples["T1 single column"])
    spread = (t1_hi - t1_lo) / t1
    print(f"# tools/rowsbench.py  n = 2^{args.log_n} salted leaves, {args.repeats} repeats of {args.batch} launches, interleaved; times in ms")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    print(f"# csrc_sha256: {csrc_sha256()}")
    print(f"# T1 spread (max - min) / median = {100 * spread:.1f} %")
    print(f"{'case':28s} {'median':>8s} {'min':>8s} {'max':>8s} {'C(w)':>5s} {'model':>8s} {'ratio':>6s} {'bound':>6s} {'verdict':>8s} {'w x T1':>8s}")
    ok = True
    for name, layout, w, _ in cases:
        s = samples[name]
        med = statistics.median(s)
        if layout is None:
            print(f"{name:28s} {med:8.4f} {min(s):8.4f} {max(s):8.4f} {3:5d} {'':>8s} {'':>6s} {'':>6s} {'':>8s} {'':>8s}")
            continue
        c = (8 * w + 26 + 63) // 64 + 2
        model = t1 * c / 3
        bound = max(1.05, 1 + spread) if w == 1 else 1.25
        ratio = med / model
        verdict = "ok" if ratio <= bound else "MISS"
        ok = ok and verdict == "ok"
        print(f"{name:28s} {med:8.4f} {min(s):8.4f} {max(s):8.4f} {c:5d} {model:8.4f} {ratio:6.3f} {bound:6.3f} {verdict:>8s} {w * t1:8.4f}")
    print(f"# matrix read at w = 64: {4 * 64 * n / 2**20:.0f} MiB per commit")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
