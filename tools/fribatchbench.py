#!/usr/bin/env python3
"""The FRI commit phase of B proofs: B single calls in a row against one batched call (include/toyni_hip.h 3r).

Sizes m0 = 2^12, 2^16, 2^20 down to 16, salted, x0 7, base and Ext, B = 1, 4, 16, 64, TOYNI_FRI_TAIL_LOG as the environment has it.
  (a) B calls of toyni_fri_commit_phase_transcript[_ext]_device in a row on one stream, then one synchronisation: the only way to do
      this work before the batched calls existed;
  (b) toyni_fri_commit_phase_transcript[_ext]_batch_device, then one synchronisation.
Both read the same B layers, salts and transcripts (a stride apart in one allocation; (a) is handed proof b's pointers) and write
into arrays of their own, which are compared once, byte for byte with the final transcripts, before anything is timed.  The two
alternate within one process after a warm-up of both, the order flipped every round; a sample is a host clock around the call(s) and
the synchronisation that ends them.  The transcripts are not reloaded between samples: a squeeze leaves a 32-byte state, so they never
grow, and both sides pay the same.  Per line: median, p10, p90 and min of --reps samples; per B the two ratios DESIGN.md 8q asks for.
Needs a GPU; prints to stdout."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toyni_amd  # noqa: E402
from toyni_amd._lib import check, lib  # noqa: E402

P = 2013265921
SIZES, BATCHES, FINAL, X0 = (12, 16, 20), (1, 4, 16, 64), 16, 7


def spread(v):
    v = sorted(v)
    return (f"median {statistics.median(v):9.1f} us   p10 {v[len(v) // 10]:9.1f}   p90 {v[(9 * len(v)) // 10]:9.1f}   min {v[0]:9.1f}")


def case(ctx, ext, log_m0, B, reps, warmup):
    pv = toyni_amd.prover
    dev = torch.device("cuda", 0)
    W = 4 if ext else 1
    m0 = 1 << log_m0
    halves = [m0 >> (k + 1) for k in range(log_m0 - FINAL.bit_length() + 1)]
    assert halves[-1] == FINAL
    rounds, nsalt = len(halves), sum(halves[:-1])
    ndig = sum(lib.toyni_merkle_total_digests(h) for h in halves)
    # strides (words; bytes for salts and levels), each a little larger than the extent
    st_e, st_s, st_ly, st_lv, st_b = W * m0 + 4, 16 * nsalt + 16, W * sum(halves) + 4, 32 * ndig + 16, W * rounds + 4
    layer0 = torch.randint(0, P, (B * st_e,), dtype=torch.int32, device=dev)
    salts = torch.randint(0, 256, (B * st_s,), dtype=torch.uint8, device=dev)
    out = {k: (torch.empty(B * st_ly, dtype=torch.int32, device=dev), torch.empty(B * st_lv, dtype=torch.uint8, device=dev),
               torch.empty(B * st_b, dtype=torch.int32, device=dev)) for k in "ab"}
    states = [bytes((7 * b + i) & 0xFF for i in range(32 + (b % 3) * 23)) for b in range(B)]
    tr = {k: pv.DeviceTranscriptBatch(B) for k in "ab"}
    s = torch.cuda.Stream(device=dev)
    single = lib.toyni_fri_commit_phase_transcript_ext_device if ext else lib.toyni_fri_commit_phase_transcript_device
    batched = pv.fri_commit_phase_transcript_ext_batch_device if ext else pv.fri_commit_phase_transcript_batch_device
    ly, lv, bt = out["a"]
    # (a): the argument tuples are built once, so a sample pays the calls and not their preparation
    calls = [(ctx.handle, layer0.data_ptr() + 4 * b * st_e, m0, X0, FINAL, salts.data_ptr() + b * st_s, tr["a"].ptr + 1024 * b,
              ly.data_ptr() + 4 * b * st_ly, lv.data_ptr() + b * st_lv, bt.data_ptr() + 4 * b * st_b, s.cuda_stream) for b in range(B)]

    def a():
        for args in calls:
            check(single(*args), "single phase")
        ctx.synchronize(s.cuda_stream)

    def b():
        batched(ctx, layer0.data_ptr(), st_e, m0, X0, FINAL, salts.data_ptr(), st_s, tr["b"], out["b"][0].data_ptr(), st_ly, out["b"][1].data_ptr(),
                st_lv, out["b"][2].data_ptr(), st_b, s.cuda_stream)
        ctx.synchronize(s.cuda_stream)

    # once, before timing: the same bytes (the gaps between the proofs are compared too: both sides leave them as they were filled)
    for k in "ab":
        tr[k].load(states, s.cuda_stream)
        for t in out[k]:
            t.fill_(-1 if t.dtype == torch.int32 else 0xA5)
    torch.cuda.synchronize()
    a(), b()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(out["a"], out["b"])), "(a) and (b) disagree"
    assert tr["a"].download() == tr["b"].download() and not any(tr["b"].status()), "the transcripts disagree"
    samples = {"a": [], "b": []}
    for r in range(warmup + reps):
        for name, f in (("a", a), ("b", b)) if r % 2 == 0 else (("b", b), ("a", a)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if r >= warmup:
                samples[name].append((t1 - t0) * 1e6)
    for k in "ab":
        tr[k].free()
    return rounds, samples


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ext", action="store_true", help="Ext-valued layers")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES), help="log2 m0")
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from csrc_hash import csrc_sha256
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    ctx = toyni_amd.NttContext(1 << max(args.sizes))
    print(f"# tools/fribatchbench.py{' --ext' if args.ext else ''}  {'Ext' if args.ext else 'base'} FRI commit phase of B proofs on the device "
          f"transcript: (a) B single calls in a row + one synchronisation against (b) one batched call + one synchronisation; "
          f"TOYNI_FRI_TAIL_LOG={os.environ.get('TOYNI_FRI_TAIL_LOG', 'default')}, final_size {FINAL}, salted, x0 {X0}; {args.reps} alternating "
          f"samples after {args.warmup} warm-up rounds of both; host clock around calls that end in a synchronisation")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    print(f"# csrc_sha256: {csrc_sha256()}")
    for log_m0 in args.sizes:
        base_a = None
        for B in args.batches:
            rounds, s = case(ctx, args.ext, log_m0, B, args.reps, args.warmup)
            ma, mb = statistics.median(s["a"]), statistics.median(s["b"])
            print(f"m0 = 2^{log_m0} ({rounds} rounds), B = {B}")
            print(f"  (a) {B:2d} single calls + synchronise   {spread(s['a'])}")
            print(f"  (b) one batched call + synchronise  {spread(s['b'])}")
            print(f"  per proof: (a) {ma / B:9.1f} us   (b) {mb / B:9.1f} us   (a) / (b) = {ma / mb:.2f}")
            if B == 1:
                base_a = ma
                va = sorted(s["a"])
                width = va[(9 * len(va)) // 10] - va[len(va) // 10]
                print(f"  B = 1: (b) - (a) = {mb - ma:+.1f} us against the single call's own p10-p90 spread of {width:.1f} us: "
                      f"{'within it' if mb - ma <= width else 'A REGRESSION OF THE DESIGN'}")
            elif base_a is not None:
                print(f"  (b) at B = {B} / (a) at B = 1 = {mb / base_a:.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
