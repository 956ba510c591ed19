"""bench.py's launch contract: `python bench.py --gpus N` (no launcher around it, exactly how the driver's SCALE runs start it)
must itself bring up N ranks -- before anything touches the GPU -- and report n_gpus = N."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last_json(text):
    lines = [l for l in text.splitlines() if l.startswith("{")]
    assert lines, text[-3000:]
    return json.loads(lines[-1])


@pytest.mark.parametrize("gpus", [1, 2, 4])
def test_bare_invocation_spawns_ranks(gpus):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--probe-ranks"],
                         capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = _last_json(res.stdout)
    assert out["n_gpus"] == gpus and out["ranks_counted"] == gpus


@pytest.mark.parametrize("gpus,batch", [(2, 1024), (4, 1024), (4, 10), (8, 1024)])
def test_strong_scaling_shards_the_job_total(gpus, batch):
    """`--scaling strong` = BASELINE configs[3] as written (1024 transforms in the whole job, 1024/G per GPU); the
    default stays weak (--batch on every GPU), which is what the driver's contract asks for."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    for scaling in ("strong", "weak"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--probe-ranks", "--batch", str(batch)] +
                             (["--scaling", "strong"] if scaling == "strong" else []),
                             capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        out = _last_json(res.stdout)
        per = [r["transforms_per_step"] // 2 for r in sorted(out["ranks"], key=lambda r: r["rank"])]
        assert out["scaling"] == scaling and len(per) == gpus
        if scaling == "strong":
            assert sum(per) == batch == out["batch_total"] and max(per) - min(per) <= 1 and per == sorted(per, reverse=True)
        else:
            assert per == [batch] * gpus and out["batch_total"] == batch * gpus


def test_under_a_launcher_no_second_spawn():
    # the contract's other form: the driver starts torch.distributed.run itself; bench.py must then NOT spawn again
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--probe-ranks"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"), cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    outs = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(outs) == 1 and json.loads(outs[0])["ranks_counted"] == 2


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_rehearsal():
    """world = 2 through the real bench body on the one GPU of the box (gloo carries the collectives, both ranks share cuda:0):
    the batch workload and the slab workload (one all-to-all per transform)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["TOYNI_BENCH_BACKEND"] = "gloo"
    for extra in (["--batch", "8"], ["--workload", "slab", "--log-n", "22"], ["--workload", "fourstep", "--log-n", "20"]):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                              "--full", "--no-extras", "--no-cpu-baseline"] + extra, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        out = _last_json(res.stdout)
        assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and out["value"] > 0
        if "--workload" in extra:    # the forward half was gathered and compared with the single-device transform
            assert out["exchange_verified"] is True
            # the one-transform lines carry a roofline object (HBM + exchange, per-phase times from events)
            roof = out["roofline"]
            assert roof["bound"] == "hbm" and 0 < roof["frac"] < 1 and roof["algorithmic_bytes_per_step"] == 16 * (1 << int(extra[-1]))
            assert roof["phases_ms_per_step"]["exchange"] > 0 and roof["exchange"]["bytes_sent_per_rank_per_transform"] > 0
            assert ("slab_pass" in roof["phases_ms_per_step"]) == (extra[1] == "slab")
        if "--batch" in extra:       # the per-rank table: which device every rank used and its own step time
            assert [r["rank"] for r in out["ranks"]] == [0, 1] and all(r["ms_per_step"] > 0 and r["transforms_per_step"] == 16 for r in out["ranks"])
            assert "rank  device  pci" in res.stderr
    # strong scaling through the real body: 9 transforms over 2 ranks = 5 + 4
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-extras",
                          "--no-cpu-baseline", "--batch", "9", "--scaling", "strong"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = _last_json(res.stdout)
    assert out["scaling"] == "strong" and [r["transforms_per_step"] for r in out["ranks"]] == [10, 8] and out["config"]["batch_total"] == 9


@pytest.mark.gpu
def test_single_process_slab_line_carries_roofline_and_baseline():
    """The configs[4] line as an 8-GPU node would print it, rehearsed with 8 lanes on the one device: `roofline` (algorithmic bytes vs
    the HBM of the devices in use, exchange bytes vs the xGMI links) and `cpu_baseline` (the oracle at n, or extrapolated and labelled)."""
    env = dict(os.environ, TOYNI_BENCH_LANES_ON_ONE_DEVICE="1")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "slab-sp", "--gpus", "8", "--log-n", "25", "--steps", "2", "--warmup", "1",
                          "--full"],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = _last_json(res.stdout)
    assert out["exchange_verified"] is True and out["lanes"] == 8
    roof, base = out["roofline"], out["cpu_baseline"]
    assert roof["bound"] == "hbm" and roof["peak"] == 8000.0 and 0 < roof["frac"] < 1
    ph = roof["phases_ms_per_step"]                      # lane 0's stages from the measurement build's events
    assert set(ph) == {"slab_pass", "exchange", "relayout", "row_transforms"} and all(v > 0 for v in ph.values())
    assert sum(ph.values()) < 3 * out["ms_per_step"]     # one lane's stages: the same order of magnitude as a step (eight lanes share the device)
    assert roof["exchange"]["bytes_sent_per_rank_per_transform"] == 4 * (1 << 25) / 8 * 7 / 8 and "ONE device" in roof["exchange"]["note"]
    assert base["kind"] == "port" and base["cores"] == 1 and base["value"] > 0 and base["extrapolated"] is True and "EXTRAPOLATED" in base["sample"]


def test_dump_outputs_and_steps_are_checked_before_any_work():
    for extra in (["--steps", "0"], ["--dump-outputs", "d", "--workload", "slab"]):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert res.returncode == 2 and "error:" in res.stderr, res.stderr[-2000:]


@pytest.mark.gpu
def test_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    """--dump-outputs: float64 arrays of what the timed path computed, identical from two runs with the same arguments; the forward
    half of the step agrees with the oracle on the transforms the batch held after the last step."""
    import numpy as np
    import oracle
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--log-n", "12", "--batch", "8", "--steps", "3", "--warmup", "1",
                              "--no-extras", "--no-cpu-baseline", "--no-kernel-events", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        out = _last_json(res.stdout)
        assert out["steps"] == 3 and out["ms_per_step"] > 0
        assert sorted(os.listdir(d)) == ["forward.npy", "roundtrip.npy"]
        dumps.append({f: np.load(d / f) for f in ("forward.npy", "roundtrip.npy")})
    for f, a in dumps[0].items():
        assert a.dtype == np.float64 and a.shape == (8, 1 << 12) and (a == dumps[1][f]).all(), f
    rt, fwd = dumps[0]["roundtrip.npy"], dumps[0]["forward.npy"]   # 8 transforms of 2^12: every one is dumped whole
    for i in range(8):
        assert (fwd[i].astype(np.uint64) == oracle.ntt(rt[i].astype(np.uint64))).all(), i


@pytest.mark.gpu
def test_plain_run_measures_value_only_and_full_adds_the_rest():
    """A plain run prints the headline figure and nothing that takes work of its own; --full adds the checks and the roofline
    object (kernel durations from the measurement build) to the same line."""
    small = ["--log-n", "12", "--batch", "8", "--steps", "3", "--warmup", "1"]
    lines = {}
    for mode in ("plain", "full"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + small + (["--full", "--no-extras", "--no-cpu-baseline"] if mode == "full" else []),
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        lines[mode] = _last_json(res.stdout)
    for out in lines.values():
        assert out["metric"] == "BabyBear NTT throughput (forward+inverse, device-resident)" and out["unit"] == "elements/s"
        assert out["higher_is_better"] is True and out["dtype"] == "u32" and out["steps"] == 3 and out["warmup"] == 1
        assert out["value"] > 0 and out["ms_per_step"] > 0 and out["value"] == pytest.approx(2 * 8 * 3 * (1 << 12) / (out["ms_per_step"] * 3e-3))
    plain, full = lines["plain"], lines["full"]
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and "extras" not in plain
    roof = full["roofline"]
    assert roof["kernel_ms"] > 0 and "HIP events" in roof["kernel_ms_source"] and len(roof["all_pass_ms"]["forward"]) == full["config"]["passes_per_transform"]
    # the one-transform workloads: the exchange check and the per-phase times are --full's as well
    env = dict(os.environ, TOYNI_BENCH_LANES_ON_ONE_DEVICE="1")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "slab-sp", "--gpus", "8", "--log-n", "25", "--steps", "2", "--warmup", "1"],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = _last_json(res.stdout)
    assert out["value"] > 0 and out["exchange_verified"] is None and out["roofline"] is None and out["cpu_baseline"] is None


def test_cpu_baseline_binary_is_built_outside_the_tree():
    """The benchmark may run as a user who cannot write the tree that build() filled: the host-native timing binary of the
    cpu_baseline leg goes to a temporary directory."""
    import bench
    exe = bench._oracle_bench_binary()
    assert os.access(exe, os.X_OK) and not os.path.abspath(exe).startswith(ROOT + os.sep), exe
