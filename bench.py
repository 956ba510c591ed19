#!/usr/bin/env python3
"""bench.py -- BabyBear NTT throughput on MI355X (BASELINE.json metric).

A *step* is one pass of the hot path over one batch of synthetic input resident in HBM: every transform
of the per-GPU batch is taken forward and back (forward NTT + inverse NTT, BASELINE configs[1]) at
n = 2^20; the batch is the repeated-prover workload of configs[3] (1024 transforms per GPU, sharded over
ranks with no collective -- weak scaling).  value = transforms * n / seconds, whole job.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--log-n 20] [--batch 1024] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Rank 0 prints ONE JSON line.  torch is plumbing here (device memory, streams, torch.distributed); the
compute is libtoyni_hip.so through the C ABI.  The oracle is used only for the cpu_baseline leg and the checks.

A plain run does only what `value` needs: set-up, warm-up, the timed steps, --dump-outputs if given, the line.
--full adds everything else, after the timed steps: the round-trip and oracle checks, the roofline object (kernel
durations from a run of the measurement build), the side measurements of other sizes and entry points (extras),
the CPU baseline, and the multi-device workloads' exchange check and per-phase times.  --no-extras,
--no-cpu-baseline and --no-kernel-events leave parts of that out again.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

P = 2013265921
HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1024, help="transforms per GPU (weak scaling) / in the whole job (strong scaling)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak (DEFAULT; the driver's contract): --batch transforms on EVERY GPU.  strong: BASELINE configs[3] as written "
                         "(SURVEY 8(d) C4): --batch transforms in the whole job, batch/N per GPU (ranks < batch mod N take one more)")
    ap.add_argument("--chunk-elems", type=int, default=-1, help="override the context's batch chunking (-1: library default)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the checks, the roofline, the side measurements and the CPU baseline "
                         "(a plain run measures `value` only)")
    ap.add_argument("--no-extras", action="store_true", help="--full: skip single-transform / fold / host-path side measurements")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--chunks", type=int, default=1, help="slab workload: issue the exchange in this many asynchronous pieces")
    ap.add_argument("--no-kernel-events", action="store_true",
                    help="--full: do not bracket the pass launches of the timed region with HIP events (A/B check of their cost)")
    ap.add_argument("--probe-ranks", action="store_true",
                    help="launch check without a GPU: the ranks rendezvous over gloo, count themselves and exit (tests/test_bench_launch.py)")
    ap.add_argument("--exchange", choices=["peer", "rccl"], default="peer", help="slab-sp workload: how the one exchange moves its blocks")
    ap.add_argument("--slab-phases-child", action="store_true", help=argparse.SUPPRESS)   # internal: bench_slab_single_process's per-phase child
    ap.add_argument("--workload", choices=["batch", "fourstep", "slab", "slab-sp"], default="batch",
                    help="batch: the default sharded batch (weak scaling); fourstep: ONE transform of n = 2^log-n split over "
                         "the ranks with one all-to-all (BASELINE configs[4]; use --log-n 27, the field's limit); slab-sp: the same "
                         "transform driven from ONE process over --gpus devices through the C ABI (toyni_ntt_slab_multi_gpu_device)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="batch workload: after the timed steps write what the last step left in the batch (roundtrip.npy) and the forward "
                         "transform of a seeded choice of its transforms (forward.npy) as float64, 48 MB at most (rank 0's shard)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.workload != "batch":
        ap.error("--dump-outputs is implemented for the batch workload only")
    return args


DUMP_ELEMS = 1 << 22   # roundtrip.npy: the whole batch up to 2^22 elements, else a seeded sample of 2^22 (32 MB in float64)
DUMP_FORWARD_ELEMS = 1 << 21   # forward.npy: whole transforms up to 2^21 elements, else a seeded sample of one transform (16 MB)


def dump_outputs(dirname, ctx, data, batch, n, stream):
    """--dump-outputs: `data` as the last timed step left it, and the forward half of the step (the same context, outside the timed
    region) on whole transforms chosen with a fixed seed.  Element samples are fixed seeded index sets, so two runs with the same
    arguments write the same elements."""
    import numpy as np
    import torch
    os.makedirs(dirname, exist_ok=True)
    rng = np.random.default_rng(0xD0417)

    def sample(t, count):
        if t.numel() <= count:
            return t
        idx = np.sort(rng.choice(t.numel(), size=count, replace=False))
        return t.reshape(-1)[torch.from_numpy(idx).to(t.device)]

    def save(name, t):
        np.save(os.path.join(dirname, name + ".npy"), t.cpu().numpy().astype(np.float64))

    save("roundtrip", sample(data.view(batch, n), DUMP_ELEMS))
    k = min(batch, max(1, DUMP_FORWARD_ELEMS // n))
    rows = torch.from_numpy(np.sort(rng.choice(batch, size=k, replace=False))).to(data.device)
    fwd = data.view(batch, n)[rows].contiguous()
    ctx.run_device(fwd.data_ptr(), fwd.data_ptr(), k, False, stream=stream)
    save("forward", sample(fwd, DUMP_FORWARD_ELEMS))


def _oracle_bench_binary():
    """bench_oracle, rebuilt HERE with gcc -O3 -march=native: the binary is native to the host that times it.  It is
    built in a temporary directory removed at exit, never in the tree, which the user running the benchmark may not be able to write."""
    import atexit
    import shutil
    import subprocess
    import tempfile
    tmp = tempfile.mkdtemp(prefix="toyni_bench_oracle_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "bench_oracle")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "bench", f"BENCH={exe}"], stdout=subprocess.DEVNULL)
    return exe


def cpu_baseline(log_n, seconds):
    """The oracle (C restatement of src/ntt.rs:24-66 and src/math/fri.rs:27-48, u128 % multiply) timed in a C loop on this
    box's host cores: forward + inverse NTT at n on one thread (the reference is single-threaded), the same on all cores
    (one independent stream per process), and the FRI fold of a 2^20 layer on one thread."""
    import shutil
    import subprocess
    exe = _oracle_bench_binary()
    n = 1 << log_n

    def run(kind, lg, secs):
        o = subprocess.run([exe, kind, str(lg), str(secs)], capture_output=True, text=True, check=True).stdout.split()
        return int(o[2]), float(o[3])

    reps, el = run("ntt", log_n, seconds)
    workers = min(os.cpu_count() or 1, 64)
    procs = [subprocess.Popen([exe, "ntt", str(log_n), str(max(2.0, seconds / 3))], stdout=subprocess.PIPE, text=True) for _ in range(workers)]
    tot = 0.0
    for p in procs:
        o = p.communicate()[0].split()
        if len(o) >= 4:
            tot += 2 * int(o[2]) * n / float(o[3])
    # the metric's other size: two repetitions of forward + inverse n = 2^24 (a repetition takes ~4 s on one core)
    big = None
    if log_n != 24:
        breps, bel = run("ntt", 24, 4.5)
        big = {"value": 2 * breps * (1 << 24) / bel, "unit": "elements/s", "cores": 1, "kind": "port",
               "sample": f"{breps} x (forward + inverse) NTT n=2^24 on 1 thread, {bel:.1f} s"}
    fold_log = 20
    freps, fel = run("fold", fold_log, max(2.0, seconds / 3))
    fold_bytes = 6.0 * (1 << fold_log)          # algorithmic: 4 B read per input element + 2 B written
    return {
        "value": 2 * reps * n / el, "unit": "elements/s", "cores": 1, "kind": "port",
        "sample": f"{reps} x (forward + inverse) NTT n=2^{log_n} on 1 thread, {el:.1f} s; oracle/toyni_oracle.c timed by "
                  f"oracle/bench_oracle.c (gcc -O3 -march=native, C loop; reference algorithm src/ntt.rs:24-66; the Rust "
                  f"reference itself cannot be built here)",
        "host_cpus": os.cpu_count(),
        "all_cores": {"value": tot, "unit": "elements/s", "cores": workers, "note": "one independent transform stream per process"},
        "fold": {"value": freps * fold_bytes / fel / 1e9, "unit": "GB/s", "cores": 1, "kind": "port",
                 "elements_per_s": freps * (1 << fold_log) / fel,
                 "sample": f"{freps} x fri_fold of a 2^{fold_log} layer (xs = 7 w^i, one Fermat inversion per output as "
                           f"src/math/fri.rs:27-48), 1 thread, {fel:.1f} s; 6 B per input element"},
        "n2^24": big,
        "rust_toolchain_present": shutil.which("cargo") is not None,
    }


XGMI_LINK_GBPS, XGMI_LINKS = 153.0, 7   # per GPU: 7 point-to-point xGMI links of ~153 GB/s (task brief; MI355X_MICROARCH.md has no xGMI row)


def single_transform_cpu_baseline(log_n, seconds=6.0):
    """cpu_baseline object of the one-large-transform workloads: the oracle's forward + inverse at n on one thread -- measured at n
    itself up to 2^24 (a repetition takes ~4 s there), beyond that the 2^24 figure scaled by n log n and LABELLED as extrapolated
    (a 2^27 repetition would take ~40 s of a run that must finish in minutes)."""
    import subprocess
    exe = _oracle_bench_binary()
    lg = min(log_n, 24)
    o = subprocess.run([exe, "ntt", str(lg), str(seconds)], capture_output=True, text=True, check=True).stdout.split()
    reps, el = int(o[2]), float(o[3])
    rate = 2 * reps * (1 << lg) / el
    out = {"value": rate, "unit": "elements/s", "cores": 1, "kind": "port", "host_cpus": os.cpu_count(),
           "sample": f"{reps} x (forward + inverse) NTT n=2^{lg} on 1 thread, {el:.1f} s (oracle/bench_oracle.c, gcc -O3 -march=native)"}
    if lg != log_n:
        out["value"] = rate * lg / log_n
        out["extrapolated"] = True
        out["sample"] += f"; EXTRAPOLATED to n=2^{log_n} by n log n (x {lg}/{log_n} in elements/s): not measured at that size"
    return out


def multi_device_roofline(log_n, lanes, n_devices, step_s, phases_ms, exchange_kind):
    """roofline object of the one-transform-over-G-lanes workloads.  Algorithmic bytes: 8 B per element per transform
    (as everywhere), two transforms per step, against the HBM of the devices in use.  Exchange: what one rank sends (= receives) per
    transform -- its n / G words minus the block that stays -- against the xGMI links of one GPU."""
    n = 1 << log_n
    alg = 2 * 8.0 * n
    achieved = alg / step_s / 1e9
    ex_bytes = 4.0 * n / lanes * (lanes - 1) / lanes
    ex_ms = (phases_ms or {}).get("exchange")
    ex = {"bytes_sent_per_rank_per_transform": ex_bytes, "kind": exchange_kind,
          "peak_GBps_per_gpu": XGMI_LINK_GBPS * XGMI_LINKS, "peak_note": f"{XGMI_LINKS} xGMI links x ~{XGMI_LINK_GBPS:.0f} GB/s per GPU, point to point: one peer's block rides ONE link",
          "ms_per_step": ex_ms, "achieved_GBps_per_rank": (2 * ex_bytes / (ex_ms * 1e-3) / 1e9) if ex_ms else None,
          "frac": (2 * ex_bytes / (ex_ms * 1e-3) / 1e9 / (XGMI_LINK_GBPS * XGMI_LINKS)) if ex_ms else None}
    if n_devices == 1:
        ex["note"] = "all lanes on ONE device: the exchange is device-local copies (a rehearsal of the control flow, not a link measurement)"
    return {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS * n_devices, "unit": "GB/s", "frac": achieved / (HBM_PEAK_GBPS * n_devices),
            "algorithmic_bytes_per_step": alg, "traffic": None,
            "phases_ms_per_step": phases_ms, "phases_source": "HIP events on the launch stream between the stages of 3 extra steps after the timed region (rank 0 / lane 0)" if phases_ms else None,
            "exchange": ex}


def gather_rank_table(torch, dist, dev, coll_dev, rank, world, distributed, units, wall_s, steps, backend):
    """(rank, device ordinal, PCI id, uuid tag, work units per step, own ms/step) of every rank, gathered on all ranks; rank 0 prints it and
    asserts under RCCL that `world` ranks sit on `world` different GPUs."""
    import zlib
    prop = torch.cuda.get_device_properties(dev)
    uuid_tag = zlib.crc32(str(getattr(prop, "uuid", "")).encode())      # a second identity next to the PCI id (either one distinct = distinct GPUs)
    mine = torch.tensor([rank, dev.index, getattr(prop, "pci_domain_id", 0), getattr(prop, "pci_bus_id", -1), getattr(prop, "pci_device_id", -1),
                         units, int(wall_s * 1e9), uuid_tag], dtype=torch.int64, device=coll_dev)
    table = [torch.zeros_like(mine) for _ in range(world)]
    if distributed:
        dist.all_gather(table, mine)
    else:
        table = [mine]
    rows = [{"rank": int(t[0]), "device": int(t[1]), "pci": "%04x:%02x:%02x" % (int(t[2]), int(t[3]) & 0xFF, int(t[4]) & 0xFF),
             "uuid_crc32": "%08x" % int(t[7]), "units_per_step": int(t[5]), "ms_per_step": int(t[6]) / 1e6 / steps} for t in table]
    if rank == 0 and distributed:
        print("rank  device  pci           units/step  ms/step", file=sys.stderr)
        for r in rows:
            print("%4d  %6d  %-12s  %10d  %.3f" % (r["rank"], r["device"], r["pci"], r["units_per_step"], r["ms_per_step"]), file=sys.stderr)
        if backend == "nccl":
            assert len({(r["pci"], r["uuid_crc32"]) for r in rows}) == world, f"{world} ranks share GPUs: {rows}"
    return rows


def bench_fourstep(args, dev, rank, world, distributed):
    """One size-n transform over all ranks: local column transforms + twiddle, ONE all-to-all (RCCL), local row transforms."""
    import torch
    import torch.distributed as dist
    from toyni_amd import dist as tdist
    log_n = args.log_n
    slab = args.workload == "slab"   # transpose-free form (include/toyni_hip.h 2b); "fourstep" = the transpose-based one
    l1, l2 = tdist.slab_split(log_n, world) if slab else tdist.fourstep_split(log_n, world)
    ops = tdist.HipLocalOps(log_n, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x4057E9 + rank)
    cols = torch.randint(0, P, ((1 << l1), (1 << l2) // world), dtype=torch.int32, device=dev, generator=gen)

    keep = cols.clone() if args.full else None

    state = {"slab": cols}

    def step():
        if slab:                     # both directions overwrite their input; the inverse's result feeds the next step
            out = tdist.slab_forward(state["slab"], log_n, ops, rank, world, chunks=args.chunks)
            state["slab"] = tdist.slab_inverse(out, log_n, ops, rank, world, chunks=args.chunks)
            return state["slab"]
        out = tdist.fourstep_forward(cols, log_n, ops, rank, world)
        return tdist.fourstep_inverse(out, log_n, ops, rank, world)

    def fence():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        back = step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        back = step()
    fence()
    own_wall = time.perf_counter() - t0
    wall = tdist.max_over_ranks(own_wall, dev)
    backend = os.environ.get("TOYNI_BENCH_BACKEND", "nccl")
    ranks_table = gather_rank_table(torch, dist if distributed else None, dev, dev, rank, world, distributed, 2, own_wall, args.steps, backend)
    verified, phases, roof, base = None, None, None, None
    if args.full:
        assert torch.equal(back, keep), "round trip changed the data"
        # A round trip is the identity for many wrong exchanges too: the FORWARD half is gathered on rank 0 and compared with the
        # single-device transform of the gathered input (the first run on real links checks itself; outside the timed region).
        fwd = tdist.slab_forward(keep.clone(), log_n, ops, rank, world, chunks=args.chunks) if slab else tdist.fourstep_forward(keep, log_n, ops, rank, world)
        ins = [torch.empty_like(keep) for _ in range(world)]
        outs = [torch.empty_like(fwd) for _ in range(world)]
        if distributed:
            dist.all_gather(ins, keep.contiguous())
            dist.all_gather(outs, fwd.contiguous())
        else:
            ins, outs = [keep], [fwd]
        if rank == 0:
            in_index = tdist.slab_input_index if slab else tdist.fourstep_input_index
            out_index = tdist.slab_output_index if slab else tdist.fourstep_output_index
            x = torch.empty(1 << log_n, dtype=torch.int32, device=dev)
            for g in range(world):
                x[in_index(log_n, world, g).to(dev).reshape(-1)] = ins[g].reshape(-1)
            ops.big.run_device(x.data_ptr(), x.data_ptr(), 1, False, stream=torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize()
            verified = all(torch.equal(outs[h].reshape(-1), x[out_index(log_n, world, h).to(dev).reshape(-1)]) for h in range(world))
            assert verified, "the distributed forward transform differs from the single-device transform"
            del x
        del ins, outs, fwd
        # per-phase times (slab pass / exchange / relayout / rows ...): three more steps with a HIP event between the stages, every rank
        # runs them (the exchange is collective), rank 0 reports its own
        if args.chunks <= 1 or not slab:
            clock = tdist.PhaseClock(dev)
            psteps = 3
            cur = keep.clone()
            for _ in range(psteps):
                if slab:
                    out_p = tdist.slab_forward(cur, log_n, ops, rank, world, clock=clock)
                    cur = tdist.slab_inverse(out_p, log_n, ops, rank, world, clock=clock)
                else:
                    out_p = tdist.fourstep_forward(cur, log_n, ops, rank, world, clock=clock)
                    cur = tdist.fourstep_inverse(out_p, log_n, ops, rank, world, clock=clock)
            phases = {k: v / psteps for k, v in clock.ms().items()}
            del cur
        if rank == 0:
            roof = multi_device_roofline(log_n, world, len({r["pci"] for r in ranks_table}) if backend == "nccl" else 1, wall / args.steps, phases,
                                         "all_to_all_single over %s" % (dist.get_backend() if distributed else "one rank: identity"))
            if not args.no_cpu_baseline:
                base = single_transform_cpu_baseline(log_n)
    if rank == 0:
        print(json.dumps({
            "exchange_verified": verified, "ranks": ranks_table,
            "metric": "BabyBear NTT throughput, single transform split over GPUs (%s, one all-to-all)" % ("slab form" if slab else "4-step"), "value": 2 * args.steps * (1 << log_n) / wall,
            "unit": "elements/s", "n_gpus": world, "rccl_ranks": dist.get_world_size() if distributed else 1,
            "collective_backend": dist.get_backend() if distributed else None,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": wall / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u32", "data": "synthetic",
            "config": {"workload": f"forward+inverse {'slab-form' if slab else '4-step'} NTT n=2^{log_n} (n1=2^{l1} x n2=2^{l2}) over {world} GPU(s), one all_to_all_single per transform",
                       "log_n": log_n, "parallelism": f"column/row split x{world}, RCCL all-to-all"},
            "roofline": roof, "cpu_baseline": base,
        }))
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


def spawn_ranks(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it (the driver's SCALE runs): start the N ranks here.

    This process has not imported torch or touched HIP yet, and it never will: the ranks run in a child
    `python -m torch.distributed.run` (one process per GPU, RCCL), whose output and exit code are passed through.  A child
    process, not an exec: nothing GPU-related is ever replaced in place."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this pool (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=env)


def slab_phases_child(args):
    """Child of bench_slab_single_process: the same lanes through the MEASUREMENT build only (libtoyni_hip_tools.so), lane 0's stream
    carrying an event between the four stages of every transform; prints {"slab_phases": {...} | null} and nothing else on stdout."""
    import ctypes
    import torch
    import __graft_entry__ as entry
    from toyni_amd import dist as tdist   # (slab_split only; this process never calls the product library)
    lanes = args.gpus
    one_dev = os.environ.get("TOYNI_BENCH_LANES_ON_ONE_DEVICE") == "1" or torch.cuda.device_count() < lanes
    devices = [0] * lanes if one_dev else list(range(lanes))
    n = 1 << args.log_n
    exchange = 1 if args.exchange == "rccl" else 0   # TOYNI_EXCHANGE_RCCL / TOYNI_EXCHANGE_PEER_COPY (include/toyni_hip.h)
    tl = ctypes.CDLL(entry.build_tools())
    vp, ci = ctypes.c_void_p, ctypes.c_int
    tl.toyni_ntt_slab_multi_gpu_device.argtypes = [vp, ci, ctypes.c_uint32, vp, vp, ci, ci]
    tl.toyni_tools_slab_phases_read.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint)]
    slabs, rows = [], []
    for g, d in enumerate(devices):
        dev = torch.device("cuda", d)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x51AB + g)
        slabs.append(torch.randint(0, P, (n // lanes,), dtype=torch.int32, device=dev, generator=gen))
        rows.append(torch.empty(n // lanes, dtype=torch.int32, device=dev))
    before = [t.clone() for t in slabs]
    for d in set(devices):
        torch.cuda.synchronize(d)
    devs_c, slabs_c, rows_c = (ci * lanes)(*devices), (vp * lanes)(*[t.data_ptr() for t in slabs]), (vp * lanes)(*[t.data_ptr() for t in rows])
    run = lambda inv: tl.toyni_ntt_slab_multi_gpu_device(devs_c, lanes, n, slabs_c, rows_c, inv, exchange)
    phases, psteps = None, 3
    ok = run(0) == 0 and run(1) == 0 and tl.toyni_tools_slab_phases(1) == 0      # warm: contexts and buffers
    for _ in range(psteps):
        ok = ok and run(0) == 0 and run(1) == 0
    ms, cnt = (ctypes.c_float * 4)(), ctypes.c_uint(0)
    ok = ok and tl.toyni_tools_slab_phases_read(ms, ctypes.byref(cnt)) == 0 and tl.toyni_tools_slab_phases(0) == 0
    ok = ok and all(torch.equal(a, b) for a, b in zip(slabs, before))          # the round trips left the data as it was
    if ok and cnt.value == 2 * psteps:
        phases = {k: ms[i] / psteps for i, k in enumerate(("slab_pass", "exchange", "relayout", "row_transforms"))}
    print(json.dumps({"slab_phases": phases}), flush=True)
    return 0 if ok else 1


def bench_slab_single_process(args):
    """ONE process, --gpus devices: the slab transform behind the C ABI (include/toyni_hip.h 2c).  With fewer devices than lanes
    (TOYNI_BENCH_LANES_ON_ONE_DEVICE=1, e.g. the 1-GPU box) every lane sits on device 0 and the exchange is a local copy."""
    import torch
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    from toyni_amd import dist as tdist
    lanes = args.gpus
    one_dev = os.environ.get("TOYNI_BENCH_LANES_ON_ONE_DEVICE") == "1" or torch.cuda.device_count() < lanes
    devices = [0] * lanes if one_dev else list(range(lanes))
    log_n = args.log_n
    n = 1 << log_n
    l1, ls = tdist.slab_split(log_n, lanes)
    exchange = toyni_amd.ntt.EXCHANGE_RCCL if args.exchange == "rccl" else toyni_amd.ntt.EXCHANGE_PEER_COPY
    slabs, rows, keep = [], [], []
    for g, d in enumerate(devices):
        dev = torch.device("cuda", d)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x51AB + g)
        slabs.append(torch.randint(0, P, (n // lanes,), dtype=torch.int32, device=dev, generator=gen))
        rows.append(torch.empty(n // lanes, dtype=torch.int32, device=dev))
        if args.full:
            keep.append(slabs[-1].clone())
    sp, rp = [t.data_ptr() for t in slabs], [t.data_ptr() for t in rows]

    def step():
        toyni_amd.ntt_slab_multi_gpu_device(n, devices, sp, rp, False, exchange)
        toyni_amd.ntt_slab_multi_gpu_device(n, devices, sp, rp, True, exchange)

    for _ in range(args.warmup):
        step()
    for d in set(devices):
        torch.cuda.synchronize(d)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()                                   # the entry point blocks until every lane is done
    wall = time.perf_counter() - t0
    verified, phases = None, None
    if args.full:
        assert all(torch.equal(a, b) for a, b in zip(slabs, keep)), "round trip changed the data"
        # the forward half against the single-device transform (a round trip alone is the identity for many wrong exchanges): gather the
        # input in natural order, transform it on device 0 alone, compare every lane's row block
        if log_n <= 27:
            d0 = torch.device("cuda", devices[0])
            nat = torch.empty(n, dtype=torch.int32, device=d0)
            for g in range(lanes):
                nat[tdist.slab_input_index(log_n, lanes, g).to(d0).reshape(-1)] = keep[g].to(d0)
            one = toyni_amd.NttContext(n, device=devices[0])
            one.run_device(nat.data_ptr(), nat.data_ptr(), 1, False, stream=torch.cuda.current_stream(d0).cuda_stream)
            torch.cuda.synchronize(d0)
            toyni_amd.ntt_slab_multi_gpu_device(n, devices, sp, rp, False, exchange)
            verified = all(torch.equal(rows[h].to(d0), nat[tdist.slab_output_index(log_n, lanes, h).to(d0).reshape(-1)]) for h in range(lanes))
            assert verified, "multi-device forward transform differs from the single-device transform"
            del nat
        # where a step's time goes: three more steps through the measurement build of the same source, whose lane 0 carries an event
        # between the four stages (toyni_tools_slab_phases; one-piece exchanges only) -- in a CHILD process: the measured
        # process never holds a second copy of the library with its own contexts, exchange buffers and communicators, and nothing that
        # goes wrong there (build, out of memory, RCCL start-up) can take the already measured line down with it
        try:
            import subprocess
            slabs.clear(); rows.clear(); keep.clear()      # this process's buffers are no longer needed: the child allocates its own
            torch.cuda.empty_cache()
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", "slab-sp", "--slab-phases-child", "--log-n", str(log_n),
                                  "--gpus", str(lanes), "--exchange", args.exchange], capture_output=True, text=True, timeout=600)
            line = [l for l in res.stdout.splitlines() if l.startswith('{"slab_phases"')]
            if res.returncode == 0 and line:
                phases = json.loads(line[-1])["slab_phases"]
            else:
                print(f"bench.py: per-phase times unavailable (child status {res.returncode}): {res.stderr[-400:]}", file=sys.stderr)
        except Exception as exc:                        # the line goes out without the per-phase times
            print(f"bench.py: per-phase times unavailable ({type(exc).__name__}: {exc})", file=sys.stderr)
    pci = {}
    for d in sorted(set(devices)):
        pr = torch.cuda.get_device_properties(d)
        pci[d] = "%04x:%02x:%02x" % (getattr(pr, "pci_domain_id", 0), getattr(pr, "pci_bus_id", 0) & 0xFF, getattr(pr, "pci_device_id", 0) & 0xFF)
    print(json.dumps({
        "exchange_verified": verified, "devices": [{"lane": g, "device": d, "pci": pci[d]} for g, d in enumerate(devices)],
        "metric": "BabyBear NTT throughput, single transform split over GPUs from one process (slab form, one exchange)",
        "value": 2 * args.steps * n / wall, "unit": "elements/s", "n_gpus": len(set(devices)), "lanes": lanes, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": wall / args.steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "u32", "data": "synthetic",
        "config": {"workload": f"forward+inverse slab-form NTT n=2^{log_n} (M1=2^{l1} x S1=2^{ls}) over {lanes} lane(s) on device(s) {sorted(set(devices))}, "
                               f"single process, exchange by {'RCCL grouped send/recv' if args.exchange == 'rccl' else 'hipMemcpyPeerAsync'}",
                   "log_n": log_n, "parallelism": f"column/row split x{lanes}, one exchange"},
        "roofline": multi_device_roofline(log_n, lanes, len(set(devices)), wall / args.steps, phases,
                                          "RCCL grouped send/recv" if args.exchange == "rccl" else "hipMemcpyPeerAsync, one copy stream per source")
                    if args.full else None,
        "cpu_baseline": single_transform_cpu_baseline(log_n) if args.full and not args.no_cpu_baseline else None}))


def shard_batch(total, world, rank, scaling):
    """Transforms of the batch workload that `rank` runs per direction.  weak (the driver's contract, default): --batch on every GPU.
    strong (BASELINE configs[3] as written): --batch in the whole job, contiguous shards, no collective."""
    if scaling == "weak":
        return total
    return total // world + (1 if rank < total % world else 0)


def probe_ranks(args):
    """What `--gpus N` starts, checked without a GPU: every rank joins a gloo group, adds 1 and reports the shard of the batch
    it would run (the same shard_batch() call the real body makes); rank 0 prints the count and the per-rank table."""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        dist.init_process_group("gloo")
    t = torch.ones(1, dtype=torch.int64)
    mine = torch.tensor([rank, shard_batch(args.batch, world, rank, args.scaling)], dtype=torch.int64)
    table = [torch.zeros_like(mine) for _ in range(world)]
    if world > 1:
        dist.all_reduce(t)
        dist.all_gather(table, mine)
    else:
        table = [mine]
    if rank == 0:
        print(json.dumps({"probe": True, "n_gpus": world, "ranks_counted": int(t.item()), "requested_gpus": args.gpus, "scaling": args.scaling,
                          "ranks": [{"rank": int(r[0]), "transforms_per_step": 2 * int(r[1])} for r in table],
                          "batch_total": sum(int(r[1]) for r in table)}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


class ToolsLib:
    """libtoyni_hip_tools.so (the measurement build of the same source, include/toyni_hip_tools.h): launch-timing hooks.  The
    timed region that produces `value` runs on the shipped libtoyni_hip.so; the roofline object's kernel durations come from
    an identical region run through this build, with every pass launch bracketed by HIP events on the launch stream."""

    def __init__(self, path):
        import ctypes
        self.ct = ctypes
        self.lib = ctypes.CDLL(path)
        vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        sig = {"toyni_ntt_ctx_create": (ci, [ctypes.c_uint32, ci, ctypes.POINTER(vp)]), "toyni_ntt_ctx_destroy": (ci, [vp]),
               "toyni_ntt_ctx_passes": (ci, [vp]), "toyni_ntt_ctx_passes_for": (ci, [vp, sz]), "toyni_ntt_device": (ci, [vp, vp, vp, sz, ci, vp]),
               "toyni_ntt_ctx_timing": (ci, [vp, ci]), "toyni_ntt_ctx_timing_read": (ci, [vp, vp, vp])}
        for name, (res, args) in sig.items():
            f = getattr(self.lib, name)
            f.restype, f.argtypes = res, args

    def context(self, n, device):
        h = self.ct.c_void_p()
        rc = self.lib.toyni_ntt_ctx_create(n, device, self.ct.byref(h))
        assert rc == 0, f"tools context: status {rc}"
        return h

    def run(self, h, ptr, batch, inverse, stream):
        rc = self.lib.toyni_ntt_device(h, ptr, ptr, batch, int(inverse), stream or None)
        assert rc == 0, f"tools transform: status {rc}"

    def timed_region(self, h, fn, batch=None):
        """Runs fn() with launch timing on; returns {'forward': [ms per pass], 'inverse': [...], 'launches': {...}}."""
        assert self.lib.toyni_ntt_ctx_timing(h, 1) == 0
        fn()
        ms = (self.ct.c_float * 6)()
        cnt = (self.ct.c_uint32 * 6)()
        assert self.lib.toyni_ntt_ctx_timing_read(h, ms, cnt) == 0
        assert self.lib.toyni_ntt_ctx_timing(h, 0) == 0
        # launches per transform of THIS batch (n = 2^21 runs its two-pass plan whatever the batch)
        npass = self.lib.toyni_ntt_ctx_passes(h) if batch is None else self.lib.toyni_ntt_ctx_passes_for(h, batch)
        out = {"launches": {}}
        for d, name in enumerate(("forward", "inverse")):
            out[name] = [ms[3 * d + p] / cnt[3 * d + p] if cnt[3 * d + p] else None for p in range(npass)]
            out["launches"][name] = [int(cnt[3 * d + p]) for p in range(npass)]
        return out

    def destroy(self, h):
        self.lib.toyni_ntt_ctx_destroy(h)


def profile_provenance(path):
    """Which commit produced a committed profile, and whether the kernels have changed since: (short hash of the last commit that
    touched `path`, True if toyni_amd/csrc has commits after it).  Profiles collected since round 3 carry the sha256 of the sources they
    measured, which needs no git; for older ones the git history answers, and (None, None) comes back where there is no .git (the GPU box)."""
    import subprocess
    rel = os.path.relpath(path, ROOT)
    # 1. exact: the profile carries the sha256 of the sources it measured (tools/csrc_hash.py, recorded on the box at collection time)
    measured = None
    try:
        if path.endswith(".json"):
            measured = json.load(open(path)).get("csrc_sha256")
        elif os.path.exists(path.replace(".csv", ".meta.json")):
            measured = json.load(open(path.replace(".csv", ".meta.json"))).get("csrc_sha256")
    except (OSError, ValueError):
        measured = None
    if measured:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from csrc_hash import csrc_sha256
        return "sources sha256 " + measured[:12], measured != csrc_sha256()
    # 2. fallback for older profiles: git history
    try:
        h = subprocess.run(["git", "log", "-1", "--format=%h", "--", rel], cwd=ROOT, capture_output=True, text=True, timeout=20).stdout.strip()
        if h:
            newer = subprocess.run(["git", "log", "--format=%h", f"{h}..HEAD", "--", "toyni_amd/csrc"], cwd=ROOT, capture_output=True, text=True,
                                   timeout=20).stdout.split()
            return h, bool(newer)
    except (OSError, subprocess.SubprocessError):
        pass
    return None, None


def stamp(src, path):
    """`profiles/x.json (kernel)` -> the same string with the profile's commit; a warning on stderr when the kernels are newer."""
    h, stale = profile_provenance(path)
    if h is None:
        return src + " [commit unknown]"
    if stale:
        print(f"bench.py: WARNING: {os.path.relpath(path, ROOT)} was measured at commit {h}; toyni_amd/csrc has changed since -- "
              f"re-collect it (tools/collect_profiles.sh) before quoting roofline.traffic", file=sys.stderr)
    return f"{src} [measured at {h if h.startswith('sources') else 'commit ' + h}{'; kernels changed since: STALE' if stale else '; identical to the running sources'}]"


def committed_fold_profile():
    """rocprofv3 evidence of the fold kernel on a 2^27 layer (tools/collect_side_profiles.sh -> profiles/rNN_fold_stats.csv): average
    launch duration and HBM bytes per launch of fri_fold_kernel<true, false>, newest round first."""
    import csv
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_fold_stats.csv")), reverse=True):
        for r in csv.DictReader(open(f)):
            # round 3: large layers run fri_fold_stream_kernel<NT = true, 1024 threads, 2 in flight> (round 2: fri_fold_kernel<true, false>)
            if ("fri_fold_stream_kernel<true" in r["Name"] or "fri_fold_kernel<true, false>" in r["Name"]) and r.get("hbm_bytes_largest_launch=(2*FETCH+WRITE)*1024"):
                return {"rocprof_avg_ms": float(r["AverageNs"]) / 1e6, "rocprof_min_ms": float(r["MinNs"]) / 1e6, "launches": int(r["Calls"]),
                        "traffic": float(r["hbm_bytes_largest_launch=(2*FETCH+WRITE)*1024"]), "file": f}
    return None


def committed_counters(log_n, batch, dom_is_last_pass, n, t_fwd_s):
    """HBM traffic and VALU instruction counts cannot be collected inside this process (rocprofv3 --pmc runs the command from
    outside): they are the COMMITTED rocprofv3 measurements of the same command (tools/collect_profiles.sh -> profiles/
    rNN_traffic*.json, rNN_counters*.json), looked up by (log_n, batch); newest round first.  (None, None, None) if this
    workload has no committed measurement."""
    import glob
    traffic = traffic_src = valu = None
    want = "Pass<1" if dom_is_last_pass else "Pass<0"   # kernel symbols carry the pass KIND: 0 = strided column pass, 1 = closing row pass
    for tfile in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic*.json")), reverse=True):
        tj = json.load(open(tfile))
        if tj.get("log_n") != log_n or tj.get("batch_per_gpu") != batch:
            continue
        kernels = [(k, v) for k, v in tj["kernels"].items() if want in k or want.replace("Pass<", "Pass3<") in k]   # (Pass3: the streaming 2048-point shapes)
        if not kernels:
            continue
        k, v = max(kernels, key=lambda kv: kv[1].get("rocprof_avg_ns") or 0)
        traffic, traffic_src = v["hbm_bytes_per_launch"], stamp(f"profiles/{os.path.basename(tfile)} ({k.split('(')[0]})", tfile)
        cfile = tfile.replace("_traffic", "_counters")
        if os.path.exists(cfile):
            cj = json.load(open(cfile))
            ks = [c for kk, c in cj.items() if "ntt_pass" in kk and kk in tj["kernels"] and c.get("SQ_INSTS_VALU") and c.get("dispatches")]
            if ks:
                # a 3-pass plan launches its column-pass kernel twice per transform: weight every kernel by its launches per transform
                dmin = min(c["dispatches"] for c in ks)
                lane_ops = sum(c["SQ_INSTS_VALU"] * c["dispatches"] / dmin for c in ks) * 64.0 / (n * batch)
                ach = lane_ops * n * batch / t_fwd_s / 1e12
                valu = {"lane_ops_per_element_per_transform": lane_ops, "achieved_Tops": ach, "peak_Tops": 39.3, "frac": ach / 39.3,
                        "note": "forward transform; peak = the 4-cycle instruction class (mul/mad/min/add3) at 2.4 GHz; add/sub/xor issue "
                                "faster (~60 T lane-ops/s, profiles/r02_microbench.txt); sustained clock under this load is ~2.0-2.1 GHz"}
        break
    return traffic, traffic_src, valu


def main():
    args = parse()
    if args.workload == "slab-sp":
        if args.slab_phases_child:
            sys.exit(slab_phases_child(args))
        return bench_slab_single_process(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    if args.probe_ranks:
        return probe_ranks(args)
    import numpy as np
    import torch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    distributed = world > 1
    # TOYNI_BENCH_BACKEND=gloo is a REHEARSAL mode for boxes with fewer GPUs than ranks (ranks share devices round-robin,
    # collectives run on CPU tensors): it exercises this file's world > 1 control flow, not RCCL.  Default: nccl (= RCCL).
    backend = os.environ.get("TOYNI_BENCH_BACKEND", "nccl")
    dev_index = local_rank if backend == "nccl" else local_rank % max(torch.cuda.device_count(), 1)
    if distributed:
        import torch.distributed as dist
        torch.cuda.set_device(dev_index)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend)
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", dev_index if distributed else 0)
    coll_dev = dev if backend == "nccl" else torch.device("cpu")   # where collective payloads live

    import __graft_entry__ as entry
    if rank == 0:
        entry.build_hip()
        if args.full:
            entry.build_tools()
    if distributed:
        dist.barrier()
    import toyni_amd

    if args.workload in ("fourstep", "slab"):
        return bench_fourstep(args, dev, rank, world, distributed)

    n = 1 << args.log_n
    # weak: every rank runs --batch transforms.  strong: --batch is the job's total, sharded contiguously (no collective either way)
    batch = shard_batch(args.batch, world, rank, args.scaling)
    assert batch >= 1, f"--scaling strong: {args.batch} transforms cannot be sharded over {world} ranks"
    ctx = toyni_amd.NttContext(n, device=dev.index)
    if args.chunk_elems >= 0:
        ctx.set_chunk(args.chunk_elems)

    # synthetic batch: uniform residues, a different seed per rank (never zeros: clocks rise on trivial operands)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x70796E69 + rank)
    data = torch.empty(batch * n, dtype=torch.int32, device=dev)
    piece = 1 << 26
    for off in range(0, batch * n, piece):
        m = min(piece, batch * n - off)
        data[off:off + m] = torch.randint(0, P, (m,), dtype=torch.int32, device=dev, generator=gen)
    check_before = data.clone() if args.full else None   # the WHOLE batch: forward + inverse must leave every transform unchanged
    stream = torch.cuda.current_stream().cuda_stream
    ptr = data.data_ptr()

    def step():
        ctx.run_device(ptr, ptr, batch, False, stream=stream)
        ctx.run_device(ptr, ptr, batch, True, stream=stream)

    def fence():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(args.steps):
        step()
    ev1.record()
    fence()
    wall = time.perf_counter() - t0
    gpu_s = ev0.elapsed_time(ev1) / 1e3
    if rank == 0 and args.dump_outputs:     # before the measurement build runs the region again on the same data
        dump_outputs(args.dump_outputs, ctx, data, batch, n, stream)
    # Kernel durations for the roofline object: the SAME region (same data, same steps) once more through the measurement
    # build of the same source (libtoyni_hip_tools.so), where every pass launch is bracketed by HIP events on the launch stream.
    region, tools_ms_per_step = None, None
    if rank == 0 and args.full and not args.no_kernel_events:
        tl = ToolsLib(entry.build_tools())
        th = tl.context(n, dev.index)

        def tools_steps():
            for _ in range(args.steps):
                tl.run(th, ptr, batch, False, stream)
                tl.run(th, ptr, batch, True, stream)

        tl.run(th, ptr, batch, False, stream)     # warm: tables, intermediate buffer
        tl.run(th, ptr, batch, True, stream)
        torch.cuda.synchronize()
        t0t = time.perf_counter()
        region = tl.timed_region(th, tools_steps, batch)  # reading the events synchronises
        tools_ms_per_step = (time.perf_counter() - t0t) / args.steps * 1e3
        tl.destroy(th)
    # forward + inverse leaves the batch unchanged: an end-to-end check of the timed region over EVERY transform (a skipped
    # or duplicated tile anywhere shows up here), plus -- a round trip is the identity for many wrong transforms too -- one
    # forward transform (the last of the batch) against the oracle, outside the timed region
    if args.full:
        assert torch.equal(data, check_before), "round trip changed the data"
    del check_before
    if rank == 0 and args.full and args.log_n <= 22:
        import oracle
        last = data[(batch - 1) * n:].clone()
        ctx.run_device(last.data_ptr(), last.data_ptr(), 1, False, stream=stream)
        torch.cuda.synchronize()
        want = oracle.ntt(data[(batch - 1) * n:].cpu().numpy().view(np.uint32).astype(np.uint64))
        assert (last.cpu().numpy().view(np.uint32) == want).all(), "forward transform differs from the oracle"
        del last

    el = torch.tensor([wall], dtype=torch.float64, device=coll_dev)
    if distributed:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    wall_max = float(el.item())
    # Which device did every rank really run on?  (rank, device ordinal, PCI domain / bus / device, its transforms, its wall time):
    # rank 0 checks that N ranks sat on N different GPUs (under RCCL; the gloo rehearsal shares devices on purpose) and prints the
    # per-rank step times next to the maximum that `value` is computed from.
    rows = gather_rank_table(torch, dist if distributed else None, dev, coll_dev, rank, world, distributed, 2 * batch, wall, args.steps, backend)
    ranks_table = [dict(r, transforms_per_step=r["units_per_step"]) for r in rows]
    total_batch = sum(r["transforms_per_step"] for r in ranks_table) // 2
    transforms = 2 * total_batch * args.steps
    value = transforms * n / wall_max

    out = None
    if rank == 0:
        out = {
            "metric": "BabyBear NTT throughput (forward+inverse, device-resident)", "value": value, "unit": "elements/s",
            "n_gpus": world, "rccl_ranks": dist.get_world_size() if distributed else 1, "collective_backend": backend if distributed else None,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": wall_max / args.steps * 1e3,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "u32", "data": "synthetic",
            "config": {
                "workload": (f"forward+inverse NTT n=2^{args.log_n} (configs[1]) over a batch of {batch} transforms per GPU "
                             f"(configs[3] repeated-prover batch), in place, inputs resident in HBM") if args.scaling == "weak" else
                            (f"forward+inverse NTT n=2^{args.log_n} (configs[1]) over {total_batch} transforms in the whole job, "
                             f"{total_batch // world}{'+1' if total_batch % world else ''} per GPU (configs[3] as written: SURVEY 8(d) C4), in place, inputs resident in HBM"),
                "log_n": args.log_n, "batch_per_gpu": batch, "batch_total": total_batch, "passes_per_transform": ctx.passes_for(batch),
                "parallelism": f"batch-sharded x{world}, no collective",
            },
            "gpu_event_ms_per_step": gpu_s / args.steps * 1e3,
            "ranks": ranks_table,
            "roofline": None,
        }

    # ---- roofline of the dominant kernel: per-pass launch durations, HIP events on the launch stream ----
    if rank == 0 and args.full:
        npass = ctx.passes_for(batch)
        if region is not None:
            fwd_ms, inv_ms = region["forward"], region["inverse"]
            timing_src = (f"HIP events around each of the {sum(region['launches']['forward']) + sum(region['launches']['inverse'])} pass launches of "
                          f"{args.steps} steps of the same workload, run right after the timed region through the measurement build "
                          f"libtoyni_hip_tools.so (same source, -DTOYNI_TOOLS; {tools_ms_per_step:.3f} ms per step there)")
        else:   # --no-kernel-events: no per-kernel durations; the whole transform's share of the step instead
            fwd_ms = inv_ms = [wall_max / args.steps * 1e3 / (2 * npass)] * npass
            timing_src = "no kernel events requested: ms_per_step / launches per step"
        dom = max(range(npass), key=lambda p: fwd_ms[p] + inv_ms[p])
        # The forward and the inverse launch of pass `dom` are the SAME kernel symbol (rocprofv3 averages them together),
        # so the kernel's average launch duration is taken over both directions.
        dom_ms = 0.5 * (fwd_ms[dom] + inv_ms[dom])
        # algorithmic bytes: 8 B per element per transform; one launch is one of `npass` sweeps of the
        # batch, so its share is 8 * n * batch / npass.
        alg_bytes = 8.0 * n * batch / npass
        achieved = alg_bytes / (dom_ms * 1e-3) / 1e9
        traffic, traffic_src, valu = committed_counters(args.log_n, batch, npass > 1 and dom == npass - 1, n, sum(fwd_ms) * 1e-3)
        out["roofline"] = {
            "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
            "traffic": traffic, "traffic_source": traffic_src,
            "kernel": f"{'ntt_pass3s_kernel (streaming 2048-point closing pass)' if (args.log_n == 21 and dom == npass - 1) else 'ntt_pass_kernel'}, "
                      f"pass {dom} of {npass} (average over its forward and inverse launches)", "kernel_ms": dom_ms,
            "kernel_ms_source": timing_src,
            "algorithmic_bytes_per_launch": alg_bytes,
            "all_pass_ms": {"forward": fwd_ms, "inverse": inv_ms},
            "sum_of_pass_ms_per_step": sum(fwd_ms) + sum(inv_ms),
            "kernel_stream_GBps": 8.0 * n * batch / (dom_ms * 1e-3) / 1e9,
            "transform_algorithmic_GBps": 8.0 * n * batch / (sum(fwd_ms) * 1e-3) / 1e9,
            "valu": valu,
        }

    # ---- side measurements (not `value`) ----
    if rank == 0 and args.full and not args.no_extras and world == 1:  # side measurements only on the single-GPU run
        extras = {}

        def time_dev(fn, reps):
            fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / reps * 1e-3

        def verify_fold_samples(evals_t, out_t, m, beta, x0=None, xs_t=None, nsamp=1 << 17):
            """Outside every timed region: `nsamp` random outputs of a fold that was just timed (plus the first and last 64 and the
            neighbourhood of every 2^20-th quad) against the oracle's fri_fold (src/math/fri.rs:27-48) on the gathered pairs.  Points:
            x0 * w_m^i (structured) or xs_t[i] (explicit)."""
            import oracle
            half = m // 2
            rs = np.random.default_rng(0xF01D)
            seams = np.arange(0, half, 1 << 22)
            idx = np.unique(np.concatenate([rs.integers(0, half, nsamp), np.arange(64), half - 1 - np.arange(64),
                                            (seams[:, None] + np.arange(-4, 4)[None, :]).ravel() % half]))
            it = torch.from_numpy(idx).to(dev)
            u32 = lambda t: t.cpu().numpy().view(np.uint32).astype(np.uint64)
            a, b, got = u32(evals_t[it]), u32(evals_t[it + half]), u32(out_t[it])
            if xs_t is not None:
                xs = u32(xs_t[it])
            else:   # x0 * w_m^i by square-and-multiply over the index bits (vectorised; spot-checked against the oracle's pow below)
                w = oracle.root_of_unity(m.bit_length() - 1)
                xs = np.full(idx.size, x0, dtype=np.uint64)
                for bit in range(m.bit_length()):
                    sel = ((idx >> bit) & 1).astype(bool)
                    xs[sel] = (xs[sel] * np.uint64(w)) % np.uint64(P)
                    w = oracle.bb_mul(w, w)
                for j in (0, idx.size // 2, idx.size - 1):
                    assert int(xs[j]) == oracle.bb_mul(x0, oracle.bb_pow(oracle.root_of_unity(m.bit_length() - 1), int(idx[j])))
            want = oracle.fri_fold(np.concatenate([a, b]), xs, beta)
            assert (got == want).all(), f"fold of a 2^{m.bit_length() - 1} layer differs from the oracle at outputs {idx[got != want][:8]}"
            return int(idx.size)

        for ln in (20, 24):
            nn = 1 << ln
            time.sleep(1.0)   # a lone transform is timed on a chip that is not still shedding the heat of the batched run
            c1 = toyni_amd.NttContext(nn, device=dev.index)
            buf = torch.randint(0, P, (nn,), dtype=torch.int32, device=dev)
            p1 = buf.data_ptr()
            t_f = time_dev(lambda: c1.run_device(p1, p1, 1, False, stream=stream), 50)
            t_i = time_dev(lambda: c1.run_device(p1, p1, 1, True, stream=stream), 50)
            # the same launches replayed from a caller-side HIP graph (a warm context only enqueues kernels, so its calls capture)
            side = torch.cuda.Stream(device=dev)
            c1.run_device(p1, p1, 1, False, stream=side.cuda_stream)
            c1.synchronize(side.cuda_stream)
            graph, chain = torch.cuda.CUDAGraph(), 20
            with torch.cuda.graph(graph, stream=side):
                for _ in range(chain):
                    c1.run_device(p1, p1, 1, False, stream=side.cuda_stream)
            t_g = time_dev(graph.replay, 10) / chain
            del graph
            extras[f"single_n2^{ln}"] = {
                "forward_us": t_f * 1e6, "inverse_us": t_i * 1e6, "forward_us_graph_replay": t_g * 1e6, "forward_elements_per_s": nn / t_f,
                "frac_of_1e12_ceiling": nn / t_f / 1e12, "note": "one transform, kernel-only, working set cache-resident; graph_replay = "
                "20 dependent forward transforms captured by the caller into one HIP graph, per transform",
            }
            if ln == 24:
                # FRI fold GB/s on the 2^24 layer: algorithmic 6 B per input element
                o = torch.empty(nn // 2, dtype=torch.int32, device=dev)
                t_fold = time_dev(lambda: toyni_amd.fri_fold_device(c1, p1, o.data_ptr(), nn, 123456789, 7, stream=stream), 50)
                extras["fri_fold_m2^24"] = {"us": t_fold * 1e6, "GBps": 6.0 * nn / t_fold / 1e9, "frac_of_hbm_peak": 6.0 * nn / t_fold / 1e9 / HBM_PEAK_GBPS}
                big = torch.randint(0, P, (1 << 28,), dtype=torch.int32, device=dev)  # 1 GiB layer: beyond the Infinity Cache
                c27 = toyni_amd.NttContext(1 << 27, device=dev.index)
                o2 = torch.empty(1 << 26, dtype=torch.int32, device=dev)
                t_fold = time_dev(lambda: toyni_amd.fri_fold_device(c27, big.data_ptr(), o2.data_ptr(), 1 << 27, 123456789, 7, stream=stream), 20)
                extras["fri_fold_m2^27"] = {"us": t_fold * 1e6, "GBps": 6.0 * (1 << 27) / t_fold / 1e9, "frac_of_hbm_peak": 6.0 * (1 << 27) / t_fold / 1e9 / HBM_PEAK_GBPS}
                # what was timed is what is checked: the output of the last timed launch, sampled against the oracle
                fold_checked = verify_fold_samples(big, o2, 1 << 27, 123456789, x0=7)
                # the same object the NTT has: the fold kernel against the HBM roofline, kernel duration from HIP events here and from the
                # committed rocprofv3 run, HBM bytes from the committed FETCH_SIZE / WRITE_SIZE passes
                fp = committed_fold_profile()
                alg_fold = 6.0 * (1 << 27)
                out["roofline_fold"] = {
                    "bound": "hbm", "achieved": alg_fold / t_fold / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": alg_fold / t_fold / 1e9 / HBM_PEAK_GBPS,
                    "kernel": "fri_fold_stream_kernel<true, 1024, 2> (structured points, non-temporal, 1024-thread workgroups with two 16-byte load pairs in "
                              "flight per lane, one table lookup per four outputs), one 2^27 layer -> 2^26",
                    "kernel_ms": t_fold * 1e3, "kernel_ms_source": "HIP events on the launch stream around 20 back-to-back launches (after one warm launch)",
                    "algorithmic_bytes_per_launch": alg_fold,
                    "traffic": fp["traffic"] if fp else None,
                    "traffic_source": stamp(f"profiles/{os.path.basename(fp['file'])} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, gfx950 x2 fetch correction)", fp["file"]) if fp else None,
                    "rocprof_kernel_ms": fp["rocprof_avg_ms"] if fp else None, "rocprof_launches": fp["launches"] if fp else None,
                    "verified": True, "verified_outputs": fold_checked,
                    "verified_how": "outputs of the last timed launch, sampled (random + both ends + chunk seams), against the oracle's fri_fold on the gathered pairs; "
                                    "every output of the same kernel at 2^26 / 2^27: tests/test_gpu_fold_large.py",
                }
                # the same 2^27 layer through the reference's literal signature fri_fold(evals, xs, beta): explicit points resident in HBM
                # (8 B algorithmic per input element: 4 evals + 2 points read, 2 written), the non-temporal 16-per-inversion kernel
                xs27 = torch.randint(1, P, (1 << 26,), dtype=torch.int32, device=dev)
                t_xs27 = time_dev(lambda: toyni_amd.fri_fold_xs_device(big.data_ptr(), xs27.data_ptr(), o2.data_ptr(), 1 << 27, 123456789, stream=stream), 20)
                xs27_checked = verify_fold_samples(big, o2, 1 << 27, 123456789, xs_t=xs27)
                extras["fri_fold_xs_m2^27"] = {
                    "us": t_xs27 * 1e6, "GBps": 8.0 * (1 << 27) / t_xs27 / 1e9, "frac_of_hbm_peak": 8.0 * (1 << 27) / t_xs27 / 1e9 / HBM_PEAK_GBPS,
                    "verified": True, "verified_outputs": xs27_checked,
                    "note": "toyni_fri_fold_xs_device, 2^27 layer beyond the Infinity Cache: fri_fold_xs16_kernel<true, 256> (one 41-product Fermat chain per "
                            "16 outputs, coalesced quads, non-temporal); round 3's kernel: 238-243 us"}
                del big, o2, xs27
                c27.destroy()
                # the reference's OWN signature fri_fold(evals, xs, beta) device-resident (explicit points: VERDICT r2 bench gap): one Fermat
                # inversion chain per 4 outputs, so the bound is VALU, not HBM: 8 B per input element (4 evals + 2 xs read, 2 written)
                xs24 = torch.randint(1, P, (nn // 2,), dtype=torch.int32, device=dev)
                t_xs = time_dev(lambda: toyni_amd.fri_fold_xs_device(p1, xs24.data_ptr(), o.data_ptr(), nn, 123456789, stream=stream), 20)
                # round 4 (batch_inverse_scaled): 41 products of the shared inversion per SIXTEEN outputs plus 4 per output (prefix product,
                # back-substitution (3 instructions: lazy), the coefficient, the application): ~6.6 per output = 3.3 per input element,
                # 5 VALU instructions each, plus the adds, against the 39.3 T lane-ops/s of that instruction class
                xs_lane_ops, xs_ops_src = 3.3 * 5 + 8, "hand count (no committed counter profile found)"
                import glob as _glob
                for cf in sorted(_glob.glob(os.path.join(ROOT, "profiles", "r*_counters_fold_xs.json")), reverse=True):
                    cj = json.load(open(cf))
                    ks = [v for k, v in cj.get("kernels", {}).items() if "fri_fold_xs16_kernel" in k]
                    if ks and cj.get("layer_log") == 24:
                        xs_lane_ops = ks[0]["lane_ops_per_input_element"]
                        xs_ops_src = stamp(f"profiles/{os.path.basename(cf)} (rocprofv3 --pmc SQ_INSTS_VALU, {ks[0]['dispatches']} launches of fri_fold_xs16_kernel on a 2^24 layer)", cf)
                        break
                xs_checked = verify_fold_samples(buf, o, nn, 123456789, xs_t=xs24)
                extras["fri_fold_xs_m2^24"] = {
                    "us": t_xs * 1e6, "GBps": 8.0 * nn / t_xs / 1e9, "frac_of_hbm_peak": 8.0 * nn / t_xs / 1e9 / HBM_PEAK_GBPS,
                    "elements_per_s": nn / t_xs, "bound": "hbm (access pattern) from 2^24 up; valu below", "verified": True, "verified_outputs": xs_checked,
                    "valu": {"lane_ops_per_input_element": xs_lane_ops, "source": xs_ops_src, "achieved_Tops": xs_lane_ops * nn / t_xs / 1e12, "peak_Tops": 39.3,
                             "frac": xs_lane_ops * nn / t_xs / 1e12 / 39.3},
                    "note": "toyni_fri_fold_xs_device on a 2^24 layer, explicit points resident in HBM; 8 B algorithmic per input element (4 evals + 2 xs "
                            "read, 2 written); one Fermat inversion (41-product addition chain) per 16 outputs, points left in plain form, coalesced quads "
                            "(src/math/fri.rs:38-40 inverts per element); round 3's form of the same kernel: 26.1 us = 5.1 TB/s, round 2's 4-per-inversion kernel 3.0 TB/s"}
                del xs24
            # reference-shaped host-slice entry point (PCIe inclusive; never `value`)
            h = np.random.default_rng(1).integers(0, P, nn, dtype=np.uint64)
            c1.run_host(h, False)
            t0h = time.perf_counter()
            reps_h = 5
            for _ in range(reps_h):
                c1.run_host(h, False)
            th = (time.perf_counter() - t0h) / reps_h
            extras[f"host_slice_n2^{ln}"] = {"ms": th * 1e3, "elements_per_s": nn / th, "note": "ntt_cuda-shaped call: H2D u64 + kernels + D2H u64, pageable host memory"}
            c1.destroy()
        # ---- BabyBearDomain::fft(coeffs) through the host-slice entry points (PCIe inclusive): pad on the host + full upload
        #      (what the reference does, src/math/domain.rs:108-109) vs toyni_lde_host (coefficients only on the way in)
        c21 = toyni_amd.NttContext(1 << 21, device=dev.index)
        hc = np.random.default_rng(3).integers(0, P, 1 << 16, dtype=np.uint64)

        def host_pad():
            v = np.zeros(1 << 21, dtype=np.uint64)
            v[: hc.size] = hc
            c21.run_host(v, False, shift=7)
            return v

        ref_h = host_pad()
        assert (c21.lde_host(hc, shift=7) == ref_h).all()
        t0h = time.perf_counter()
        for _ in range(5):
            host_pad()
        t_pad_h = (time.perf_counter() - t0h) / 5
        t0h = time.perf_counter()
        for _ in range(5):
            c21.lde_host(hc, shift=7)
        t_lde_h = (time.perf_counter() - t0h) / 5
        extras["host_lde_2^16_to_2^21"] = {"ms_host_pad_then_ntt": t_pad_h * 1e3, "ms_lde_host": t_lde_h * 1e3,
                                            "note": "domain.fft(coeffs) on host slices, coset shift 7, pageable memory; PCIe inclusive"}
        c21.destroy()
        # ---- the other headline size, batched: 64 x n = 2^24 (4 GiB, three sweeps per transform)
        c24 = toyni_amd.NttContext(1 << 24, device=dev.index)
        n24, b24 = 1 << 24, 64
        buf24 = data[: n24 * b24] if data.numel() >= n24 * b24 else torch.randint(0, P, (n24 * b24,), dtype=torch.int32, device=dev)
        p24 = buf24.data_ptr()

        def fb24():
            c24.run_device(p24, p24, b24, False, stream=stream)
            c24.run_device(p24, p24, b24, True, stream=stream)

        t24 = time_dev(fb24, 5)
        extras["batched_n2^24"] = {"batch": b24, "ms_per_fwd_inv": t24 * 1e3, "elements_per_s": 2 * b24 * n24 / t24,
                                   "passes_per_transform": c24.passes, "note": "same step as `value` at n = 2^24"}
        # the same roofline object for this size: per-pass launch durations from HIP events around the launches of 5 more steps
        tl24 = ToolsLib(entry.build_tools())
        th24 = tl24.context(n24, dev.index)
        tl24.run(th24, p24, b24, False, stream)
        tl24.run(th24, p24, b24, True, stream)

        def steps24():
            for _ in range(5):
                tl24.run(th24, p24, b24, False, stream)
                tl24.run(th24, p24, b24, True, stream)

        r24 = tl24.timed_region(th24, steps24)
        tl24.destroy(th24)
        f24, i24 = r24["forward"], r24["inverse"]
        np24 = c24.passes
        d24 = max(range(np24), key=lambda p: f24[p] + i24[p])
        d24_ms = 0.5 * (f24[d24] + i24[d24])
        alg24 = 8.0 * n24 * b24 / np24
        tr24, tr24_src, _ = committed_counters(24, b24, np24 > 1 and d24 == np24 - 1, n24, sum(f24) * 1e-3)
        extras["batched_n2^24"]["roofline"] = {
            "bound": "hbm", "achieved": alg24 / (d24_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": alg24 / (d24_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": tr24, "traffic_source": tr24_src,
            "kernel": f"ntt_pass_kernel, pass {d24} of {np24}", "kernel_ms": d24_ms, "algorithmic_bytes_per_launch": alg24,
            "all_pass_ms": {"forward": f24, "inverse": i24},
            "kernel_stream_GBps": 8.0 * n24 * b24 / (d24_ms * 1e-3) / 1e9,
            "transform_algorithmic_GBps": 8.0 * n24 * b24 / (sum(f24) * 1e-3) / 1e9,
        }
        c24.destroy()

        # ---- n = 2^21, the prover's own LDE size (configs[2]), batched: 128 transforms (1 GiB).  Round 5: TWO sweeps (1024-point
        #      column pass + the streaming three-step 2048-point closing pass) where rounds 1-4 made three 128-point ones
        c21b = toyni_amd.NttContext(1 << 21, device=dev.index)
        n21, b21 = 1 << 21, 128
        buf21 = data[: n21 * b21] if data.numel() >= n21 * b21 else torch.randint(0, P, (n21 * b21,), dtype=torch.int32, device=dev)
        p21 = buf21.data_ptr()

        def fb21():
            c21b.run_device(p21, p21, b21, False, stream=stream)
            c21b.run_device(p21, p21, b21, True, stream=stream)

        t21 = time_dev(fb21, 5)
        extras["batched_n2^21"] = {"batch": b21, "ms_per_fwd_inv": t21 * 1e3, "elements_per_s": 2 * b21 * n21 / t21,
                                   "passes_per_transform": c21b.passes_for(b21),
                                   "note": "same step as `value` at n = 2^21; the three-pass plan of rounds 1-4: 2.70 ms (1.99e11 elements/s)"}
        tl21 = ToolsLib(entry.build_tools())
        th21 = tl21.context(n21, dev.index)
        tl21.run(th21, p21, b21, False, stream)
        tl21.run(th21, p21, b21, True, stream)

        def steps21():
            for _ in range(5):
                tl21.run(th21, p21, b21, False, stream)
                tl21.run(th21, p21, b21, True, stream)

        r21 = tl21.timed_region(th21, steps21, b21)
        tl21.destroy(th21)
        f21, i21 = r21["forward"], r21["inverse"]
        np21 = len(f21)
        d21 = max(range(np21), key=lambda p: f21[p] + i21[p])
        d21_ms = 0.5 * (f21[d21] + i21[d21])
        alg21 = 8.0 * n21 * b21 / np21
        tr21, tr21_src, _ = committed_counters(21, b21, np21 > 1 and d21 == np21 - 1, n21, sum(f21) * 1e-3)
        extras["batched_n2^21"]["roofline"] = {
            "bound": "hbm", "achieved": alg21 / (d21_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": alg21 / (d21_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": tr21, "traffic_source": tr21_src,
            "kernel": f"pass {d21} of {np21} ({'ntt_pass3s_kernel, the streaming 2048-point closing pass' if d21 == np21 - 1 else 'ntt_pass_kernel, the 1024-point column pass'})",
            "kernel_ms": d21_ms, "algorithmic_bytes_per_launch": alg21, "all_pass_ms": {"forward": f21, "inverse": i21},
            "kernel_stream_GBps": 8.0 * n21 * b21 / (d21_ms * 1e-3) / 1e9,
            "transform_algorithmic_GBps": 8.0 * n21 * b21 / (sum(f21) * 1e-3) / 1e9,
        }
        c21b.destroy()

        # ---- low-degree extension of a batch of columns (src/fibonacci.rs:101-103, blowup 32, coset shift 7): zero padding
        #      implied (toyni_lde_device) vs padded by hand + the ordinary coset transform
        l_out, l_blow, l_batch = 21, 5, 64
        c_lde = toyni_amd.NttContext(1 << l_out, device=dev.index)
        coeffs = torch.randint(0, P, (l_batch, (1 << l_out) >> l_blow), dtype=torch.int32, device=dev)
        ext = torch.empty((l_batch, 1 << l_out), dtype=torch.int32, device=dev)

        def lde_fused():
            c_lde.lde_device(coeffs.data_ptr(), ext.data_ptr(), l_batch, l_blow, 7, stream=stream)

        def lde_padded():
            ext.zero_()
            ext[:, : coeffs.shape[1]] = coeffs
            c_lde.run_device(ext.data_ptr(), ext.data_ptr(), l_batch, False, stream=stream, shift=7)

        lde_padded()
        ref = ext.clone()
        lde_fused()
        assert torch.equal(ext, ref), "lde_device differs from pad + coset transform"
        t_pad, t_lde = time_dev(lde_padded, 10), time_dev(lde_fused, 10)
        extras["lde_64x_2^16_to_2^21"] = {"ms_pad_then_transform": t_pad * 1e3, "ms_lde_device": t_lde * 1e3,
                                           "output_elements_per_s": l_batch * (1 << l_out) / t_lde,
                                           "note": "blowup 32, coset shift 7; first pass reads 1/32 of the rows and skips butterflies with a zero partner"}
        del coeffs, ext, ref
        c_lde.destroy()

        # ---- fft_ext / ifft_ext (src/math/domain.rs:129-151: what the downstream zkvm calls, src/ext.rs:1-8): 64 Ext vectors of 2^20
        #      elements, AoS ([n][4] words), device-resident, through the interleaved passes -- no de-interleave on either side
        e_log, e_vecs = 20, 64
        c_e = toyni_amd.NttContext(1 << e_log, device=dev.index)
        xe = torch.randint(0, P, (e_vecs * 4 << e_log,), dtype=torch.int32, device=dev)   # 1 GiB
        xe0 = xe.clone()
        pe = xe.data_ptr()
        t_ef = time_dev(lambda: c_e.run_device_ext_batch(pe, pe, e_vecs, False, shift=7, stream=stream), 10)
        xe.copy_(xe0)
        c_e.run_device_ext_batch(pe, pe, e_vecs, False, shift=7, stream=stream)
        c_e.run_device_ext_batch(pe, pe, e_vecs, True, shift=7, stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(xe, xe0), "Ext round trip changed the data"
        # one vector's coordinate 0 against the oracle (the last vector: a wrong tile order anywhere in the batch shows there or in the round trip)
        import oracle
        c_e.run_device_ext_batch(pe, pe, e_vecs, False, shift=7, stream=stream)
        torch.cuda.synchronize()
        last_in = xe0.view(e_vecs, 1 << e_log, 4)[e_vecs - 1, :, 0].cpu().numpy().view(np.uint32).astype(np.uint64)
        last_out = xe.view(e_vecs, 1 << e_log, 4)[e_vecs - 1, :, 0].cpu().numpy().view(np.uint32)
        assert (last_out == oracle.domain_fft(last_in, 1 << e_log, 7)).all(), "Ext transform differs from the oracle"
        t_ei = time_dev(lambda: c_e.run_device_ext_batch(pe, pe, e_vecs, True, shift=7, stream=stream), 10)
        t_eb = time_dev(lambda: c_e.run_device(pe, pe, 4 * e_vecs, False, shift=7, stream=stream), 10)   # the same bytes as base transforms
        ext_elems = e_vecs << e_log
        alg_ext = 32.0 * ext_elems        # 16 B read + 16 B written per Ext element per transform (the 8 B per base element of SURVEY 8(d), x 4)
        extras["ntt_ext_64x2^20"] = {
            "forward_ms": t_ef * 1e3, "inverse_ms": t_ei * 1e3, "ext_elements_per_s": ext_elems / t_ef,
            "base_transforms_same_bytes_ms": t_eb * 1e3, "overhead_vs_base": t_ef / t_eb - 1.0,
            "roofline": {"bound": "hbm", "achieved": alg_ext / t_ef / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": alg_ext / t_ef / 1e9 / HBM_PEAK_GBPS,
                         "algorithmic_bytes_per_call": alg_ext, "note": "whole transform (its two pass launches), 32 B per Ext element"},
            "verified": True,
            "note": "coset forward / inverse of 64 Ext vectors x 2^20 (AoS, 1 GiB) in ONE call; rounds 2-3 ran ext_split -> batch of 4 -> ext_join per vector "
                    "(two extra sweeps): A/B in profiles/r04_ab_ext.txt"}
        del xe, xe0
        c_e.destroy()

        # ---- the transforms of one proof (BASELINE configs[2]: trace_len 2^16, blowup 32 -> lde 2^21), device-resident, single
        #      transforms back to back: interpolate (INTT 2^16), coset LDE 2^16 -> 2^21, the two coset INTTs of src/fibonacci.rs:145,151
        lt, ll = 16, 21
        c_t, c_l = toyni_amd.NttContext(1 << lt, device=dev.index), toyni_amd.NttContext(1 << ll, device=dev.index)
        trace = torch.randint(0, P, (1 << lt,), dtype=torch.int32, device=dev)
        lde = torch.zeros(1 << ll, dtype=torch.int32, device=dev)
        q1 = torch.randint(0, P, (1 << ll,), dtype=torch.int32, device=dev)
        q2 = torch.randint(0, P, (1 << ll,), dtype=torch.int32, device=dev)
        t_intt16 = time_dev(lambda: c_t.run_device(trace.data_ptr(), trace.data_ptr(), 1, True, stream=stream), 50)
        t_lde21 = time_dev(lambda: c_l.lde_device(trace.data_ptr(), lde.data_ptr(), 1, 5, 7, stream=stream), 50)
        t_cntt21 = time_dev(lambda: c_l.run_device(q1.data_ptr(), q1.data_ptr(), 1, False, stream=stream, shift=7), 50)
        t_cintt21 = time_dev(lambda: c_l.run_device(q2.data_ptr(), q2.data_ptr(), 1, True, stream=stream, shift=7), 50)
        extras["prover_transforms_trace2^16_lde2^21"] = {
            "intt_2^16_us": t_intt16 * 1e6, "lde_2^16_to_2^21_us": t_lde21 * 1e6, "coset_ntt_2^21_us": t_cntt21 * 1e6,
            "coset_intt_2^21_us": t_cintt21 * 1e6, "note": "single transforms, kernel-only (latency configuration: three-step 4-wide tiles where the launch is small)"}

        # ---- the FRI phase as the PROTOCOL orders it (src/fibonacci.rs:222-245): beta_{k+1} is squeezed from a transcript that has
        #      absorbed round k's Merkle root, so every round is: fold + commit on the device -> 32-byte root to the host -> SHA-256
        #      transcript -> next beta.  17 rounds 2^21 -> 2^4.  `fused`: toyni_fri_fold_commit_device (leaf hashes inside the fold's
        #      sweep); `separate`: toyni_fri_fold_device + toyni_merkle_commit_device.
        import hashlib
        from toyni_amd._lib import lib as _tlib
        n_l = 1 << ll
        salts_all = torch.randint(0, 255, (n_l, 16), dtype=torch.uint8, device=dev)
        lay = [torch.empty(n_l >> k, dtype=torch.int32, device=dev) for k in range(18)]
        lay[0].copy_(q1)
        lvls = [torch.empty((_tlib.toyni_merkle_total_digests(n_l >> k), 32), dtype=torch.uint8, device=dev) for k in range(18)]

        def fri_phase(fused):
            state = b"toyni-stark-v1"
            x0 = 7
            soff = 0                                                         # salts of the salted layers back to back
            for k in range(17):
                state = hashlib.sha256(state).digest()                       # squeeze_challenge, src/transcript.rs
                beta = int.from_bytes(state[:8], "little") % P
                m = n_l >> k
                salted = (m // 2) != 16
                sp = salts_all.data_ptr() + 16 * soff if salted else 0
                soff += m // 2
                if fused:
                    toyni_amd.prover.fri_fold_commit_device(c_l, lay[k].data_ptr(), lay[k + 1].data_ptr(), m, beta, x0, sp, lvls[k + 1].data_ptr(), stream=stream)
                else:
                    toyni_amd.fri_fold_device(c_l, lay[k].data_ptr(), lay[k + 1].data_ptr(), m, beta, x0, stream=stream)
                    toyni_amd.merkle_commit_device(lay[k + 1].data_ptr(), sp, m // 2, lvls[k + 1].data_ptr(), stream=stream)
                x0 = x0 * x0 % P
                state += lvls[k + 1][-1].cpu().numpy().tobytes()             # absorb_commitment: the root crosses PCIe, the stream drains
            return state

        assert fri_phase(True) == fri_phase(False), "fused and separate FRI rounds disagree"

        # the same 17 rounds through toyni_fri_commit_phase_device: the loop runs inside the library, the transcript stays a callback
        lay_all = torch.empty(n_l - 16, dtype=torch.int32, device=dev)
        lvl_all = torch.empty((sum(_tlib.toyni_merkle_total_digests(n_l >> k) for k in range(1, 18)), 32), dtype=torch.uint8, device=dev)

        def fri_phase_one_call():
            st = {"t": b"toyni-stark-v1"}

            def challenge(_rnd, root, want_beta):
                if root is not None:
                    st["t"] += root
                if not want_beta:
                    return 0
                st["t"] = hashlib.sha256(st["t"]).digest()
                return int.from_bytes(st["t"][:8], "little") % P

            toyni_amd.prover.fri_commit_phase_device(c_l, lay[0].data_ptr(), n_l, 7, 16, salts_all.data_ptr(), challenge, lay_all.data_ptr(),
                                                     lvl_all.data_ptr(), stream=stream)
            return st["t"]

        assert fri_phase_one_call() == fri_phase(True), "one-call FRI phase and round-by-round calls disagree"

        def wall(fn, reps):
            fn()
            torch.cuda.synchronize()
            t0w = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0w) / reps

        extras["fri_phase_protocol_order_2^21"] = {
            "one_call_ms": wall(fri_phase_one_call, 5) * 1e3,
            "fused_fold_commit_ms": wall(lambda: fri_phase(True), 5) * 1e3, "separate_fold_then_commit_ms": wall(lambda: fri_phase(False), 5) * 1e3,
            "rounds": 17, "note": "wall time incl. the per-round root read-back and host transcript (beta_{k+1} depends on root_k); one_call = "
            "toyni_fri_commit_phase_device (the loop inside the library, the transcript a callback), the others one or two library calls per round"}
        del lay, lvls, salts_all, lay_all, lvl_all

        # ---- BASELINE configs[2]: the whole prover-shaped harness (tests/harness/fib_prover.py) at trace_len 2^16, blowup 32:
        #      every heavy step is a device call of this library (LDE, constraint/quotient, coset INTTs, OOD evaluations, DEEP, 17
        #      fold+commit rounds, 20 Merkle trees, ~1 700 openings); host work = transcript hashing.  The proof is checked by the
        #      verifier restatement in tests; timed here in its serialized form (openings as the records the device wrote).
        # Timed on the COMPILED prover (toyni_amd/csrc/host/fib_prover.hpp, run as build/fib_prove: C++ over the C ABI, its proofs
        # checked by the verifier restatement in tests/test_fib_prover_cpp.py); the Python harness' time is kept next to it.
        try:
            import subprocess
            exe = entry.build_fib_prove()
            res = subprocess.run([exe, str(1 << 16), "21", "9", "--phases"], capture_output=True, text=True, timeout=300, cwd=ROOT)
            line = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
            cj = json.loads(line)
            assert cj.get("gpu") and "error" not in cj, line[:300]
            ms_sorted = sorted(cj["ms"])
            fib = {"ms": ms_sorted[len(ms_sorted) // 2], "ms_all": cj["ms"], "phase_ms_with_syncs": cj["phases"], "pcie_per_proof": cj["pcie"],
                   "proof_bytes": cj["proof_bytes"], "caller": "C++ (toyni_amd/csrc/host/fib_prover.hpp via build/fib_prove), one process, two streams (the trace tree is built beside the quotient kernels)",
                   "note": "wall time per proof, warm, median of 9, salts and mask from a ChaCha20 keystream on the device; the reference prover is "
                           "infeasible at this size (O(n^3) interpolation, SURVEY F5)"}
        except Exception as exc:
            fib = {"ms": None, "error": str(exc)[:300]}
        try:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from harness import fib_prover
            col = fib_prover.fibonacci_trace(1 << 16)
            fib_prover.generate_proof(col, seed=11, raw=True)            # warm (contexts, tables)
            times = []
            for sd in (12, 13, 14):
                torch.cuda.synchronize()
                t0p = time.perf_counter()
                fib_prover.generate_proof(col, seed=sd, raw=True)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0p) * 1e3)
            fib["python_harness_ms"] = sorted(times)[1]
        except Exception as exc:
            fib["python_harness_error"] = str(exc)[:300]
        extras["fib_prove_trace2^16_blowup32"] = fib

        # one 2^27 transform through the single-process multi-GPU entry point (include/toyni_hip.h 2c), 8 lanes on this one device
        try:
            ln27, lanes27 = 27, 8
            sl = [torch.randint(0, P, ((1 << ln27) // lanes27,), dtype=torch.int32, device=dev) for _ in range(lanes27)]
            rw = [torch.empty_like(t) for t in sl]
            spp, rpp = [t.data_ptr() for t in sl], [t.data_ptr() for t in rw]

            def slab_sp():
                toyni_amd.ntt_slab_multi_gpu_device(1 << ln27, [dev.index] * lanes27, spp, rpp, False)
                toyni_amd.ntt_slab_multi_gpu_device(1 << ln27, [dev.index] * lanes27, spp, rpp, True)

            slab_sp()
            torch.cuda.synchronize()
            t0s = time.perf_counter()
            for _ in range(5):
                slab_sp()
            extras["slab_2^27_single_process_8_lanes_on_one_gpu"] = {
                "ms_per_fwd_inv": (time.perf_counter() - t0s) / 5 * 1e3,
                "note": "toyni_ntt_slab_multi_gpu_device: slab pass, 64 local block copies standing in for the xGMI exchange, relayout, row transforms; blocking calls"}
            del sl, rw
        except Exception as exc:
            extras["slab_2^27_single_process_8_lanes_on_one_gpu"] = {"error": str(exc)[:300]}

        # batched host-slice transform (ntt_cuda-shaped, PCIe inclusive): pageable memory (what a Rust Vec is) against pinned
        # memory from toyni_host_alloc, which takes the pipelined path (upload / kernels / download overlapped)
        try:
            hb_n, hb_batch = 1 << 20, 256                                    # 2 GiB of u64
            hctx = toyni_amd.NttContext(hb_n, device=dev.index)
            pageable = np.random.default_rng(21).integers(0, P, hb_n * hb_batch, dtype=np.uint64)
            pinned = toyni_amd.PinnedArray(hb_n * hb_batch)
            pinned.array[:] = pageable
            res = {}
            for name, arr in (("pageable", pageable), ("pinned", pinned.array)):
                hctx.run_host(arr, False, batch=hb_batch)
                t0h = time.perf_counter()
                hctx.run_host(arr, True, batch=hb_batch)
                hctx.run_host(arr, False, batch=hb_batch)
                res[name] = (time.perf_counter() - t0h) / 2
            assert (pinned.array == pageable).all()
            extras["host_batch_256x2^20"] = {"pageable_ms": res["pageable"] * 1e3, "pinned_pipelined_ms": res["pinned"] * 1e3,
                                             "pinned_elements_per_s": hb_n * hb_batch / res["pinned"],
                                             "pinned_GBps_each_way": 8.0 * hb_n * hb_batch / res["pinned"] / 1e9,
                                             "note": "toyni_ntt_host on 2 GiB of u64 in place; PCIe-bound, never `value`"}
            pinned.free()
            del pageable
            hctx.destroy()
        except Exception as exc:
            extras["host_batch_256x2^20"] = {"error": str(exc)[:300]}

        # the reference-shaped fold call fri_fold(evals, xs, beta) on host slices (src/math/fri.rs:27-48), PCIe inclusive
        hm = 1 << 20
        he = np.random.default_rng(7).integers(0, P, hm, dtype=np.uint64)
        hx = np.random.default_rng(8).integers(1, P, hm, dtype=np.uint64)
        toyni_amd.fri_fold(he, hx, 12345)
        t0h = time.perf_counter()
        for _ in range(5):
            toyni_amd.fri_fold(he, hx, 12345)
        th = (time.perf_counter() - t0h) / 5
        extras["fri_fold_host_m2^20"] = {"ms": th * 1e3, "GBps_algorithmic": 6.0 * hm / th / 1e9,
                                         "note": "toyni_fri_fold_host: u64 evals + xs up, u64 layer down, explicit points (one Fermat chain per 4), pageable memory"}

        # Merkle commitment of one lde-size layer (the prover builds 3 of these plus 17 shrinking FRI layers): SURVEY 8(f) rank 2
        from toyni_amd._lib import lib as _tlib
        nl = 1 << ll
        salts = torch.randint(0, 2**31 - 1, (nl * 4,), dtype=torch.int32, device=dev)
        lv = torch.empty(_tlib.toyni_merkle_total_digests(nl) * 8, dtype=torch.int32, device=dev)
        t_m = time_dev(lambda: toyni_amd.merkle_commit_device(q1.data_ptr(), salts.data_ptr(), nl, lv.data_ptr(), stream=stream), 20)
        extras["merkle_commit_2^21_salted"] = {"us": t_m * 1e6, "note": "SHA-256 leaves + 21 node levels, device-resident, 22 launches"}
        out["extras"] = extras
        # BASELINE.json's metric has three single-GPU parts; `value` is the first, the other two are lifted out of the extras
        out["metric_parts"] = {
            "ntt_n2^20_elements_per_s": out["value"],
            "ntt_n2^24_elements_per_s": extras.get("batched_n2^24", {}).get("elements_per_s"),
            "fri_fold_GBps": extras.get("fri_fold_m2^27", {}).get("GBps"),
            "fri_fold_frac_of_hbm_peak": extras.get("fri_fold_m2^27", {}).get("frac_of_hbm_peak"),
        }

    if rank == 0 and args.full and not args.no_cpu_baseline and world == 1:
        out["cpu_baseline"] = cpu_baseline(args.log_n, args.cpu_seconds)
    elif rank == 0:
        out["cpu_baseline"] = None

    if rank == 0:
        print(json.dumps(out))
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
