#!/usr/bin/env python3
"""Per-round wall time of the FRI fold + commit rounds 2^21 -> 2^4 (diagnostic): where do the 2 ms of the phase go?
Prints, per round: leaves of the folded layer, us for fold+commit enqueue + stream drain, us for the 32-byte root read-back.

--ext: the commit phase over Ext-valued layers (include/toyni_hip.h 3j), m0 = 2^12, 2^16 and 2^20 Ext elements down to 16, salted:
toyni_fri_commit_phase_ext_device against the sequence a caller had to write before it existed -- per round toyni_fri_fold_ext_device,
toyni_merkle_commit_rows_device(width 4, row-major), toyni_stream_synchronize and a 32-byte toyni_memcpy_d2h of the root -- and one
round of each at m = 2^20.  Both sides run the same betas on the same layer and must produce the same roots; they alternate within
one process, after a warm-up of both, and each sample is a host clock around a call that ends blocked on the device.  The condition,
written down before the first run: the single call is not slower (median) than the composed sequence at any of the three sizes.
It is reported as measured; exit status 2 when it does not hold.

--transcript (with or without --ext): the commit phase on the device transcript (include/toyni_hip.h 3l) against the callback phase,
m0 = 2^12, 2^16 and 2^20 down to 16, salted.  (a) the callback phase, the yardstick: toyni_fri_commit_phase[_ext]_device with the
transcript of tests/harness (hashlib behind a ctypes callback -- what the Python provers pay per round; a compiled caller's callback is
cheaper by the interpreter's share); (new) toyni_fri_commit_phase_transcript[_ext]_device followed by one stream synchronisation, the
1 KiB upload of the initial transcript included.  --tail-log N sets TOYNI_FRI_TAIL_LOG for the process before the first call (the knob
is read once): -1 is variant (b), every round launched; the default is variant (c), the fused small rounds.  Both sides start from the
same transcript and must leave the same layers, trees and transcript; they alternate within one process after a warm-up of both.
With the fused tail a captured graph of the new phase at 2^16 is replayed as well (replay + synchronisation).

--ext --arity4: the four-to-one phase under coset leaves (include/toyni_hip.h 3m, toyni_fri4_commit_phase_transcript_ext_device)
against the two-to-one phase on the same device transcript (3l, toyni_fri_commit_phase_transcript_ext_device), m0 = 2^12, 2^16 and
2^20 down to 16, salted, the same layer 0 and x0.  The two are different protocols (other layers, other trees), so there is no output
to compare: each is held to its own judges by the tests.  Timing: device events around a WINDOW of back-to-back calls on one stream,
the window sized (from a calibration run) to --window seconds; the two phases alternate window by window within one process, --alternations
times, the order flipped every time, after a warm-up window of both.  The transcript is loaded once per window (a squeeze leaves a
32-byte state, so it never grows).  Per phase: the median time per call over the windows, the spread (max - min) / median over the
windows, and the host's enqueue time per call, which says whether a window was bound by the device or by the launches.  No threshold:
the expectation written down before the first run is the count of dependent tree levels; the ratio is reported as
measured, with whether it lies inside the spread."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toyni_amd  # noqa: E402
from toyni_amd._lib import lib  # noqa: E402

P = 2013265921


def main():
    dev = torch.device("cuda", 0)
    n = 1 << 21
    ctx = toyni_amd.NttContext(n)
    stream = torch.cuda.current_stream().cuda_stream
    lay = [torch.randint(0, P, (n >> k,), dtype=torch.int32, device=dev) for k in range(18)]
    lv = [torch.empty((lib.toyni_merkle_total_digests(n >> k), 32), dtype=torch.uint8, device=dev) for k in range(18)]
    salts = torch.randint(0, 255, (n, 16), dtype=torch.uint8, device=dev)
    reps = 20
    tot = 0.0
    for k in range(17):
        m = n >> k
        t_run = t_root = 0.0
        for r in range(reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toyni_amd.prover.fri_fold_commit_device(ctx, lay[k].data_ptr(), lay[k + 1].data_ptr(), m, 12345, 7, salts.data_ptr(), lv[k + 1].data_ptr(), stream=stream)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            root = lv[k + 1][-1].cpu()
            t2 = time.perf_counter()
            if r >= 2:
                t_run += t1 - t0
                t_root += t2 - t1
        print(f"round {k:2d}: {m // 2:8d} leaves  fold+commit {t_run / reps * 1e6:8.1f} us   root read-back {t_root / reps * 1e6:6.1f} us", flush=True)
        tot += (t_run + t_root) / reps
    print(f"sum {tot * 1e3:.3f} ms")


# ---- --ext ----
EXT_SIZES = (12, 16, 20)
EXT_FINAL = 16
EXT_X0 = 7


def ext_beta(rnd):
    return [(1234567 * (rnd + 1) + 89 * k) % P for k in range(4)]


def ext_phase_case(ctx, log_m0, reps, warmup, stream):
    from toyni_amd._lib import FRI_EXT_CHALLENGE_FN, check
    dev = torch.device("cuda", 0)
    m0 = 1 << log_m0
    halves = [m0 >> (k + 1) for k in range(log_m0 - EXT_FINAL.bit_length() + 1)]
    assert halves[-1] == EXT_FINAL
    layer0 = torch.randint(0, P, (4 * m0,), dtype=torch.int32, device=dev)
    salts = torch.randint(0, 256, (sum(halves[:-1]), 16), dtype=torch.uint8, device=dev)
    ndig = [lib.toyni_merkle_total_digests(h) for h in halves]
    out = {name: (torch.empty(4 * sum(halves), dtype=torch.int32, device=dev), torch.empty((sum(ndig), 32), dtype=torch.uint8, device=dev))
           for name in ("phase", "composed")}
    betas = [(ctypes.c_uint32 * 4)(*ext_beta(k)) for k in range(len(halves))]

    def _cb(_user, rnd, _root, beta_ptr):
        if beta_ptr:
            for k in range(4):
                beta_ptr[k] = betas[rnd][k]
        return 0

    cb = FRI_EXT_CHALLENGE_FN(_cb)
    roots = {name: (ctypes.c_uint8 * (32 * len(halves)))() for name in out}
    rounds = ctypes.c_uint(0)

    def phase():
        layers, levels = out["phase"]
        check(lib.toyni_fri_commit_phase_ext_device(ctx.handle, layer0.data_ptr(), m0, EXT_X0, EXT_FINAL, salts.data_ptr(), ctypes.cast(cb, ctypes.c_void_p),
                                                    None, layers.data_ptr(), levels.data_ptr(), roots["phase"], ctypes.byref(rounds), stream), "phase")

    def composed():
        layers, levels = out["composed"]
        cur, m, x, lo, dlo, slo = layer0.data_ptr(), m0, EXT_X0, layers.data_ptr(), levels.data_ptr(), salts.data_ptr()
        for k, h in enumerate(halves):
            last = k == len(halves) - 1
            check(lib.toyni_fri_fold_ext_device(ctx.handle, cur, lo, m, betas[k], x, stream), "fold")
            check(lib.toyni_merkle_commit_rows_device(lo, h, 4, toyni_amd.ROWS_ROW_MAJOR, 0, None if last else slo, dlo, stream), "commit")
            check(lib.toyni_stream_synchronize(ctx.handle, stream), "synchronize")
            check(lib.toyni_memcpy_d2h(ctypes.byref(roots["composed"], 32 * k), dlo + 32 * (ndig[k] - 1), 32), "root")
            cur, m, x, lo, dlo, slo = lo, h, x * x % P, lo + 16 * h, dlo + 32 * ndig[k], slo + (0 if last else 16 * h)

    samples = {"phase": [], "composed": []}
    for r in range(warmup + reps):
        for name, f in (("phase", phase), ("composed", composed)) if r % 2 == 0 else (("composed", composed), ("phase", phase)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if r >= warmup:
                samples[name].append((t1 - t0) * 1e6)
    torch.cuda.synchronize()
    assert rounds.value == len(halves) and bytes(roots["phase"]) == bytes(roots["composed"]), "the two sequences disagree on the roots"
    assert torch.equal(out["phase"][0], out["composed"][0]) and torch.equal(out["phase"][1], out["composed"][1]), "the two sequences disagree"
    return len(halves), samples


def ext_round_case(ctx, log_m, reps, warmup, stream):
    from toyni_amd._lib import check
    dev = torch.device("cuda", 0)
    m = 1 << log_m
    half = m // 2
    layer = torch.randint(0, P, (4 * m,), dtype=torch.int32, device=dev)
    salts = torch.randint(0, 256, (half, 16), dtype=torch.uint8, device=dev)
    ndig = lib.toyni_merkle_total_digests(half)
    out = {name: (torch.empty(4 * half, dtype=torch.int32, device=dev), torch.empty((ndig, 32), dtype=torch.uint8, device=dev)) for name in ("fused", "two calls")}
    beta = (ctypes.c_uint32 * 4)(*ext_beta(0))

    def fused():
        o, lv = out["fused"]
        check(lib.toyni_fri_fold_commit_ext_device(ctx.handle, layer.data_ptr(), o.data_ptr(), m, beta, EXT_X0, salts.data_ptr(), lv.data_ptr(), stream), "round")
        check(lib.toyni_stream_synchronize(ctx.handle, stream), "synchronize")

    def two_calls():
        o, lv = out["two calls"]
        check(lib.toyni_fri_fold_ext_device(ctx.handle, layer.data_ptr(), o.data_ptr(), m, beta, EXT_X0, stream), "fold")
        check(lib.toyni_merkle_commit_rows_device(o.data_ptr(), half, 4, toyni_amd.ROWS_ROW_MAJOR, 0, salts.data_ptr(), lv.data_ptr(), stream), "commit")
        check(lib.toyni_stream_synchronize(ctx.handle, stream), "synchronize")

    samples = {"fused": [], "two calls": []}
    for r in range(warmup + reps):
        for name, f in (("fused", fused), ("two calls", two_calls)) if r % 2 == 0 else (("two calls", two_calls), ("fused", fused)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if r >= warmup:
                samples[name].append((t1 - t0) * 1e6)
    assert torch.equal(out["fused"][0], out["two calls"][0]) and torch.equal(out["fused"][1], out["two calls"][1]), "the round and the two calls disagree"
    return samples


def spread(v):
    q = statistics.quantiles(v, n=10)
    return f"median {statistics.median(v):9.1f} us   p10 {q[0]:9.1f}   p90 {q[-1]:9.1f}   min {min(v):9.1f}"


def main_ext(reps, warmup):
    ctx = toyni_amd.NttContext(1 << max(EXT_SIZES))
    stream = torch.cuda.current_stream().cuda_stream or None
    print(f"Ext FRI commit phase, final_size {EXT_FINAL}, salted, x0 {EXT_X0}; {reps} alternating samples after {warmup} warm-up rounds of both; "
          f"host clock around blocking calls; device {torch.cuda.get_device_name(0)}")
    verdicts = []
    for log_m0 in EXT_SIZES:
        rounds, s = ext_phase_case(ctx, log_m0, reps, warmup, stream)
        a, b = statistics.median(s["phase"]), statistics.median(s["composed"])
        print(f"m0 = 2^{log_m0} ({rounds} rounds)")
        print(f"  toyni_fri_commit_phase_ext_device          {spread(s['phase'])}")
        print(f"  fold_ext + commit_rows + sync + d2h / round {spread(s['composed'])}")
        print(f"  composed / phase = {b / a:.3f}   ({(b - a) / rounds:+.1f} us per round)")
        verdicts.append((log_m0, a, b))
    s = ext_round_case(ctx, 20, reps, warmup, stream)
    a, b = statistics.median(s["fused"]), statistics.median(s["two calls"])
    print("one round at m = 2^20 (2^19 leaves), each followed by a stream synchronisation")
    print(f"  toyni_fri_fold_commit_ext_device           {spread(s['fused'])}")
    print(f"  fold_ext + commit_rows                     {spread(s['two calls'])}")
    print(f"  two calls / fused = {b / a:.3f}")
    failed = [(l, a, b) for l, a, b in verdicts if a > b]
    if failed:
        for l, a, b in failed:
            print(f"CONDITION NOT MET at m0 = 2^{l}: the single call took {a:.1f} us (median), the composed sequence {b:.1f} us")
        return 2
    print("CONDITION MET: the single call is not slower (median) than the composed sequence at 2^12, 2^16 and 2^20")
    return 0


# ---- --transcript ----
def transcript_case(ctx, ext, log_m0, reps, warmup, with_graph):
    import hashlib
    from toyni_amd import prover as pv
    dev = torch.device("cuda", 0)
    words = 4 if ext else 1
    m0 = 1 << log_m0
    halves = [m0 >> (k + 1) for k in range(log_m0 - EXT_FINAL.bit_length() + 1)]
    layer0 = torch.randint(0, P, (words * m0,), dtype=torch.int32, device=dev)
    salts = torch.randint(0, 256, (sum(halves[:-1]), 16), dtype=torch.uint8, device=dev)
    ndig = [lib.toyni_merkle_total_digests(h) for h in halves]
    out = {name: (torch.empty(words * sum(halves), dtype=torch.int32, device=dev), torch.empty((sum(ndig), 32), dtype=torch.uint8, device=dev))
           for name in ("callback", "device")}
    state0 = hashlib.sha256(b"toyni-stark-v1").digest() + bytes(range(32))      # a transcript that has squeezed and absorbed one root
    final = {}

    def callback():
        t = [state0]

        def squeeze():
            t[0] = hashlib.sha256(t[0]).digest()
            return int.from_bytes(t[0][:8], "little") % P

        def challenge(_rnd, root, want_beta):
            if root is not None:
                t[0] += root
            if not want_beta:
                return 0
            return [squeeze() for _ in range(4)] if ext else squeeze()

        layers, levels = out["callback"]
        entry = pv.fri_commit_phase_ext_device if ext else pv.fri_commit_phase_device
        entry(ctx, layer0.data_ptr(), m0, EXT_X0, EXT_FINAL, salts.data_ptr(), challenge, layers.data_ptr(), levels.data_ptr())
        final["callback"] = t[0]

    tr = pv.DeviceTranscript()
    entry_dev = pv.fri_commit_phase_transcript_ext_device if ext else pv.fri_commit_phase_transcript_device
    s = torch.cuda.Stream(device=dev)

    def enqueue(stream):
        layers, levels = out["device"]
        entry_dev(ctx, layer0.data_ptr(), m0, EXT_X0, EXT_FINAL, salts.data_ptr(), tr, layers.data_ptr(), levels.data_ptr(), 0, stream)

    def device():
        tr.load(state0, s.cuda_stream)
        enqueue(s.cuda_stream)
        ctx.synchronize(s.cuda_stream)

    samples = {"callback": [], "device": []}
    for r in range(warmup + reps):
        for name, f in (("callback", callback), ("device", device)) if r % 2 == 0 else (("device", device), ("callback", callback)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            t1 = time.perf_counter()
            if r >= warmup:
                samples[name].append((t1 - t0) * 1e6)
    torch.cuda.synchronize()
    assert torch.equal(out["callback"][0], out["device"][0]) and torch.equal(out["callback"][1], out["device"][1]), "the two phases disagree"
    assert tr.download() == (final["callback"], 0), "the two transcripts disagree"
    if with_graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            enqueue(s.cuda_stream)
        samples["graph"] = []
        for r in range(warmup + reps):
            tr.load(state0, s.cuda_stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.replay()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r >= warmup:
                samples["graph"].append((t1 - t0) * 1e6)
        assert torch.equal(out["callback"][0], out["device"][0]) and tr.download() == (final["callback"], 0), "the replay disagrees"
        del g
    tr.free()
    return len(halves), samples


def main_transcript(ext, reps, warmup, tail_log):
    if tail_log is not None:
        os.environ["TOYNI_FRI_TAIL_LOG"] = str(tail_log)
    knob = os.environ.get("TOYNI_FRI_TAIL_LOG", "default")
    fused = knob != "-1"
    ctx = toyni_amd.NttContext(1 << max(EXT_SIZES))
    print(f"{'Ext' if ext else 'base'} FRI commit phase on the device transcript, TOYNI_FRI_TAIL_LOG={knob} "
          f"({'variant (c): fused small rounds' if fused else 'variant (b): every round launched'}), final_size {EXT_FINAL}, salted, x0 {EXT_X0}; "
          f"{reps} alternating samples after {warmup} warm-up rounds of both; host clock around calls that end in a synchronisation; "
          f"device {torch.cuda.get_device_name(0)}")
    for log_m0 in EXT_SIZES:
        rounds, s = transcript_case(ctx, ext, log_m0, reps, warmup, with_graph=fused and log_m0 == 16)
        a, b = statistics.median(s["callback"]), statistics.median(s["device"])
        print(f"m0 = 2^{log_m0} ({rounds} rounds)")
        print(f"  (a) callback phase, hashlib transcript      {spread(s['callback'])}")
        print(f"  ({'c' if fused else 'b'}) device transcript + synchronise        {spread(s['device'])}")
        print(f"  (a) / new = {a / b:.3f}   ({(a - b) / rounds:+.1f} us per round; the new call {'beats' if b < a else 'DOES NOT beat'} (a))")
        if "graph" in s:
            print(f"  (c) captured graph, replay + synchronise    {spread(s['graph'])}")
    return 0


# ---- --ext --arity4 ----
def arity4_case(ctx, log_m0, window_s, alternations):
    from toyni_amd import prover as pv
    dev = torch.device("cuda", 0)
    m0 = 1 << log_m0
    halves = [m0 >> (k + 1) for k in range(log_m0 - EXT_FINAL.bit_length() + 1)]
    quarters = [m0 >> (2 * k + 2) for k in range((log_m0 - EXT_FINAL.bit_length() + 1) // 2)]
    assert halves[-1] == EXT_FINAL and quarters[-1] == EXT_FINAL
    layer0 = torch.randint(0, P, (4 * m0,), dtype=torch.int32, device=dev)
    salts = torch.randint(0, 256, (sum(halves[:-1]), 16), dtype=torch.uint8, device=dev)      # the four-to-one phase reads a prefix
    out2 = (torch.empty(4 * sum(halves), dtype=torch.int32, device=dev),
            torch.empty((sum(lib.toyni_merkle_total_digests(h) for h in halves), 32), dtype=torch.uint8, device=dev))
    out4 = (torch.empty(4 * sum(quarters), dtype=torch.int32, device=dev),
            torch.empty((sum(lib.toyni_merkle_total_digests(q // 4) for q in quarters), 32), dtype=torch.uint8, device=dev))
    import hashlib
    state0 = hashlib.sha256(b"toyni-stark-v1").digest() + bytes(range(32))
    tr = pv.DeviceTranscript()
    s = torch.cuda.Stream(device=dev)

    def two():
        pv.fri_commit_phase_transcript_ext_device(ctx, layer0.data_ptr(), m0, EXT_X0, EXT_FINAL, salts.data_ptr(), tr, out2[0].data_ptr(),
                                                  out2[1].data_ptr(), 0, s.cuda_stream)

    def four():
        pv.fri4_commit_phase_transcript_ext_device(ctx, layer0.data_ptr(), m0, EXT_X0, EXT_FINAL, salts.data_ptr(), tr, out4[0].data_ptr(),
                                                   out4[1].data_ptr(), 0, s.cuda_stream)

    def window(f, calls):
        """(device seconds per call, host enqueue seconds per call) of `calls` back-to-back calls"""
        tr.load(state0, s.cuda_stream)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(s)
        t0 = time.perf_counter()
        for _ in range(calls):
            f()
        t1 = time.perf_counter()
        b.record(s)
        torch.cuda.synchronize()
        assert tr.status() == 0
        return a.elapsed_time(b) * 1e-3 / calls, (t1 - t0) / calls

    phases = {"two-to-one": two, "four-to-one": four}
    calls = {}
    for name, f in phases.items():          # warm-up and calibration: a short window, then the count that fills window_s
        window(f, 5)
        calls[name] = max(5, int(window_s / window(f, 20)[0]) + 1)
        window(f, calls[name])
    dev_s, host_s = {n: [] for n in phases}, {n: [] for n in phases}
    for r in range(alternations):
        for name in (list(phases) if r % 2 == 0 else list(phases)[::-1]):
            d, h = window(phases[name], calls[name])
            dev_s[name].append(d)
            host_s[name].append(h)
    tr.free()
    return len(halves), len(quarters), calls, dev_s, host_s


def main_arity4(window_s, alternations):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from csrc_hash import csrc_sha256
    ctx = toyni_amd.NttContext(1 << max(EXT_SIZES))
    print(f"# tools/fri_rounds.py --ext --arity4  Ext FRI commit phase on the device transcript, four-to-one under coset leaves (3m) against "
          f"two-to-one (3l, TOYNI_FRI_TAIL_LOG={os.environ.get('TOYNI_FRI_TAIL_LOG', 'default')}); final_size {EXT_FINAL}, salted, x0 {EXT_X0}; "
          f"device events around windows of back-to-back calls sized to {window_s} s, {alternations} alternations, order flipped each time")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    print(f"# csrc_sha256: {csrc_sha256()}")
    print("# expectation written before the first run (a count, not a measurement): dependent tree levels two-to-one / four-to-one")
    for log_m0 in EXT_SIZES:
        r2, r4, calls, dev_s, host_s = arity4_case(ctx, log_m0, window_s, alternations)
        levels2 = sum(log_m0 - k - 1 for k in range(r2))                    # a tree of m / 2 leaves has log2(m) - 1 levels above its leaves
        levels4 = sum(log_m0 - 2 * k - 4 for k in range(r4))                # a tree of m / 16 leaves has log2(m) - 4
        print(f"m0 = 2^{log_m0}: {r2} rounds / {levels2} node levels two-to-one, {r4} rounds / {levels4} node levels four-to-one "
              f"(level ratio {levels2 / max(levels4, 1):.2f}, round ratio {r2 / r4:.2f})")
        med, spr = {}, {}
        for name in ("two-to-one", "four-to-one"):
            v = dev_s[name]
            med[name], spr[name] = statistics.median(v), (max(v) - min(v)) / statistics.median(v)
            print(f"  {name:11s}  {med[name] * 1e6:9.1f} us per call (median of {len(v)} windows of {calls[name]} calls, "
                  f"{med[name] * calls[name]:.2f} s each)   spread {spr[name] * 100:4.1f} %   min {min(v) * 1e6:9.1f}   max {max(v) * 1e6:9.1f}   "
                  f"host enqueue {statistics.median(host_s[name]) * 1e6:7.1f} us per call")
        ratio = med["two-to-one"] / med["four-to-one"]
        inside = abs(ratio - 1.0) <= spr["two-to-one"] + spr["four-to-one"]
        print(f"  two-to-one / four-to-one = {ratio:.3f}   ({'INSIDE' if inside else 'outside'} the run-to-run spread of the two)")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ext", action="store_true", help="the Ext commit phase against the composed sequence (see above)")
    ap.add_argument("--transcript", action="store_true", help="the commit phase on the device transcript against the callback phase (see above)")
    ap.add_argument("--tail-log", type=int, default=None, help="with --transcript: TOYNI_FRI_TAIL_LOG for this process (-1: every round launched)")
    ap.add_argument("--arity4", action="store_true", help="with --ext: the four-to-one phase under coset leaves against the two-to-one phase (see above)")
    ap.add_argument("--window", type=float, default=0.3, help="with --arity4: seconds of device time per timed window")
    ap.add_argument("--alternations", type=int, default=7, help="with --arity4: windows per phase (at least 5)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if args.arity4:
        if not args.ext or args.transcript or args.alternations < 5:
            ap.error("--arity4 goes with --ext alone, and with at least 5 alternations")
        sys.exit(main_arity4(args.window, args.alternations))
    if args.transcript:
        sys.exit(main_transcript(args.ext, args.reps, args.warmup, args.tail_log))
    sys.exit(main_ext(args.reps, args.warmup) if args.ext else main())
