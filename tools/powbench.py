#!/usr/bin/env python3
"""Hash rate of toyni_transcript_grind_device (include/toyni_hip.h 3n), and what a proof pays for 16 and 20 bits.

Every figure is ONE device-event pair around ONE call (three launches: arm, search, finish).  The states have the shape a proof's
transcript has after its commit phase -- a 32-byte digest followed by a 32-byte root, 64 bytes: the midstate is one compression and a
candidate is one more.

    rate      bits = 28, log_tries = 32, start = 0, one call per state: (nonce - start + 1) / time.  The search tests at most one grid
              row (196 608 candidates) beyond the hit, which is negligible at 2^28.  Median and spread across the states.
    16 / 20   the same call at the bit counts a proof actually uses: launch-bound; median and spread across states and repeats.

Every nonce is checked with the library's host verifier (toyni_pow_check_host); minimality is the GPU tests' business.

    python3 tools/powbench.py [--states 10] [--repeats 5] [--out profiles/pow_grind.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bits", type=int, default=28)
    ap.add_argument("--log-tries", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pow_grind.txt"))
    args = ap.parse_args()
    assert args.states >= 8, "the rate is a median over at least eight states"
    import numpy as np
    import torch
    import toyni_amd
    from csrc_hash import csrc_sha256
    assert toyni_amd.gpu_available(), "powbench needs the GPU: there is no fallback"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0x3E)
    states = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(args.states)]
    tr = toyni_amd.prover.DeviceTranscript()
    nonce = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def one_call(state, bits, log_tries):
        """(milliseconds, nonce, status) of one grind on a freshly uploaded state"""
        tr.load(state, stream)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.grind(nonce.data_ptr(), bits, 0, log_tries, stream)
        b.record()
        torch.cuda.synchronize()
        got = int(nonce.cpu().numpy().view(np.uint64)[0])
        after, status = tr.download()
        if status == 0:
            assert toyni_amd.pow_check(state, got, bits) and after == state + got.to_bytes(8, "little"), "the device's nonce fails the host check"
        return a.elapsed_time(b), got, status

    for bits in (8, 16, 20):                           # warm-up: every launch site, every grid size class
        one_call(states[0], bits, 24)
    lines = [f"# tools/powbench.py  {args.states} states of 64 bytes (digest || root), one event pair around one call; times in ms",
             f"# device: {torch.cuda.get_device_name(0)}", f"# csrc_sha256: {csrc_sha256()}",
             f"# rate: bits = {args.bits}, log_tries = {args.log_tries}, start = 0; rate = (nonce + 1) / time",
             f"{'state':>5s} {'nonce':>12s} {'log2':>6s} {'ms':>9s} {'GH/s':>8s}"]
    rates = []
    for k, s in enumerate(states):
        ms, got, status = one_call(s, args.bits, args.log_tries)
        if status:
            lines.append(f"{k:5d} {'no hit':>12s} {'':>6s} {ms:9.3f} {(1 << args.log_tries) / ms / 1e6:8.2f}   (the whole window)")
            rates.append((1 << args.log_tries) / ms / 1e6)
            continue
        rates.append((got + 1) / ms / 1e6)
        lines.append(f"{k:5d} {got:12d} {np.log2(got + 1):6.2f} {ms:9.3f} {rates[-1]:8.2f}")
    lines.append(f"# rate: median {statistics.median(rates):.2f} GH/s, min {min(rates):.2f}, max {max(rates):.2f} "
                 f"(spread {100 * (max(rates) - min(rates)) / statistics.median(rates):.1f} % of the median)")
    for bits in (16, 20):
        ms_all, nonces = [], []
        for _ in range(args.repeats):
            for s in states:
                ms, got, status = one_call(s, bits, args.log_tries)
                assert status == 0
                ms_all.append(ms)
                nonces.append(got)
        lines.append(f"# bits = {bits}: one call {1e3 * statistics.median(ms_all):.1f} us median, {1e3 * min(ms_all):.1f} min, {1e3 * max(ms_all):.1f} max "
                     f"over {len(ms_all)} calls; nonces {min(nonces)} .. {max(nonces)}")
    tr.free()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
