"""bench.py prints ONE JSON line with the driver's contract fields plus `roofline`; a plain run measures nothing else, `--full` adds
`sustained` and the other secondary objects (with the CPU legs switched off here for speed: no `cpu_baseline`); `--workloads-only` prints
the other SURVEY 8(d) workloads."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _last_json(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


def test_bench_line_contract():
    env = dict(os.environ, MIOPEN_LOG_LEVEL="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "2", "--full", "--sustained", "2",
                        "--alt-steps", "2", "--no-cpu-baseline", "--no-workloads"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "sustained", "hip_ms_per_step", "host_enqueue_ms_per_step"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "images/s"
    # VERDICT r02 ruling (a), (b): the default arithmetic names the split, and the pure fp32-MFMA step stays in the line beside it
    assert d["dtype"] == "f32 (bf16x3-split MFMA, fp32 accumulate)" and "3-piece" in d["config"]["workload"]
    assert d["fp32_mfma_convolutions"]["ms_per_step"] > 0 and d["fp32_mfma_convolutions"]["dtype"].startswith("f32")
    assert d["vs_baseline"] is None and d["scaling"] == "weak" and d["higher_is_better"] is True and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 2 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    rf = d["roofline"]
    assert rf["kernel"] == "sc_sdf_backward_fused" and rf["bound"] in ("mfma", "hbm") and rf["unit"] == "TFLOP/s"
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and rf["peak"] == 157.3
    assert d["sustained"]["steps"] == 2 and d["sustained"]["ms_per_step"] > 0
    assert "sc_sdf_forward" in d["hip_ms_per_step"] and "sc_rgb_composite_backward" in d["hip_ms_per_step"]


def test_bench_plain_run_measures_only_the_headline():
    """`bench.py --steps K --warmup W` without --full, at the headline batch: the contract fields and what the timed region recorded,
    none of the secondary measurements that take runs of their own."""
    env = dict(os.environ, MIOPEN_LOG_LEVEL="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len([l for l in r.stdout.splitlines() if l.startswith("{")]) == 1
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["config"]["global_batch"] == 32
    assert d["metric"] == "train-step images/sec (Pix3D cfg, bs32/GPU)" and d["unit"] == "images/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32 (bf16x3-split MFMA, fp32 accumulate)" and abs(d["value"] - 32 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    assert d["roofline"]["kernel"] == "sc_sdf_backward_fused" and "sc_sdf_forward" in d["hip_ms_per_step"]
    assert d["sustained"] is None
    for k in ("fp32_mfma_convolutions", "config1_bs16", "allreduce", "cpu_baseline", "workloads"):
        assert k not in d, k


def test_bench_dump_outputs_are_reproducible(tmp_path):
    """`--dump-outputs DIR` writes what the last timed step computed; the inputs are seeded and the step is deterministic, so two runs with
    the same arguments write the same arrays, bit for bit, and the line still times exactly `--steps` steps."""
    import numpy as np
    env = dict(os.environ, MIOPEN_LOG_LEVEL="1")
    runs = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "2", "--sustained", "0",
                            "--no-alt", "--no-cpu-baseline", "--no-workloads", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        line = _last_json(r.stdout)
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dump_outputs"]["files"] == len(list(d.iterdir()))
        runs.append({f.name: np.load(f) for f in d.iterdir()})
    a, b = runs
    assert set(a) == set(b) and sum(x.nbytes for x in a.values()) <= 64 << 20
    assert {"loss.all.npy", "var.rgb_recon.npy", "var.mask_recon.npy", "var.grad_eikonal.npy"} <= set(a)
    assert any(n.startswith("param.") for n in a) and any(n.startswith("grad.") for n in a)
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert np.isfinite(a["loss.all.npy"]).all()
    differ = [n for n in a if not np.array_equal(a[n], b[n], equal_nan=True)]
    assert not differ, differ[:10]


def test_bench_default_batch_reports_config1_beside_the_headline():
    """At the headline batch (bs32) the line also carries BASELINE config[1] (bs16 on one GPU) as a secondary object; contract keys unchanged."""
    env = dict(os.environ, MIOPEN_LOG_LEVEL="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--full", "--sustained", "0", "--alt-steps", "3",
                        "--no-cpu-baseline", "--no-workloads"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    assert d["config"]["global_batch"] == 32 and d["metric"].endswith("bs32/GPU)") and abs(d["value"] - 32 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    c1 = d["config1_bs16"]
    assert c1["steps"] == 3 and c1["ms_per_step"] > 0 and abs(c1["value"] - 16 / (c1["ms_per_step"] * 1e-3)) < 0.01 * c1["value"]
    assert len([l for l in r.stdout.splitlines() if l.startswith("{")]) == 1


def test_bench_two_ranks_through_the_launcher():
    """The driver's N > 1 invocation (`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`) on the one GPU of this
    box: two ranks share cuda:0 and exchange over gloo (SC_BENCH_BACKEND), everything else is the code the scaling run executes --
    barrier-bracketed timing, MAX over ranks, whole-job value, the overlapped flat all-reduce, ONE JSON line from rank 0."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MIOPEN_LOG_LEVEL="1", SC_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "2",
                        "--full", "--sustained", "2"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len([l for l in r.stdout.splitlines() if l.startswith("{")]) == 1
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 4 and abs(d["value"] - 4 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]       # whole-job images / s
    assert d["allreduce"]["payload_bytes"] > 140e6 and d["allreduce"]["ms"] > 0
    assert "cpu_baseline" not in d and "workloads" not in d                    # rank 0 does no extra work the other ranks would wait for
    assert d["sustained"]["steps"] == 2


def test_bench_self_launches_its_ranks():
    """VERDICT r04 next #1a/b: plain `python bench.py --gpus 2` -- no torch.distributed.run in front, no RANK / WORLD_SIZE in the environment
    -- starts its own two ranks (gloo on the one GPU of this box) and prints ONE line with n_gpus == 2 and the multi-rank extras."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MIOPEN_LOG_LEVEL="1", SC_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "2",
                        "--full", "--sustained", "0", "--opt=--hip.reserve_cus=16"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len([l for l in r.stdout.splitlines() if l.startswith("{")]) == 1
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 4
    rk, ar = d["ranks"], d["allreduce"]
    assert rk["backend"] == "gloo" and rk["backend_world_size"] == 2 and 0 < rk["ms_per_step_min"] <= rk["ms_per_step_max"]
    assert abs(rk["ms_per_step_max"] - d["ms_per_step"]) < 0.02 * d["ms_per_step"]          # the line's time is the slowest rank's
    assert ar["bus_GBps"] > 0 and ar["reserved_cus"] == 16 and ar["persistent_grid_cus"] == torch_cus() - 16
    assert ar["schedule"].startswith("single flat")


def torch_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_reserved_cus_same_results():
    """`--hip.reserve_cus`: the stream-K 3x3 convolution (split arithmetic) and its weight gradient on a (CUs - 32) grid give the values of
    the full grid up to the summation order of the shared tiles (fp32 rounding), and the setting is undone by 0.  The 3x3 kernels only:
    the stem and the 1x1 / stride 2 shortcut run on reduced grids in tests/test_gpu_gemm_partition_exact.py, the stride-2 3x3 kernels in
    tests/test_gpu_conv_plan.py."""
    import torch
    from shapeclipper_amd import ops
    torch.manual_seed(0)
    x = torch.randn(8, 128, 28, 28, device="cuda")
    w = torch.randn(128, 128, 3, 3, device="cuda") * 0.05
    gy = torch.randn(8, 128, 28, 28, device="cuda")
    try:
        full = ops.set_reserved_cus(0)
        y0, dw0 = ops.conv3x3_forward(x, w, split=True), ops.conv3x3_backward_weight(gy, x, split=True)
        assert ops.set_reserved_cus(32) == full - 32
        y1, dw1 = ops.conv3x3_forward(x, w, split=True), ops.conv3x3_backward_weight(gy, x, split=True)
        y2 = ops.conv3x3_forward(x, w, split=True)
    finally:
        assert ops.set_reserved_cus(0) == full
    ref = torch.nn.functional.conv2d(x.double(), w.double(), None, 1, 1)
    assert torch.equal(y1, y2)                                             # deterministic on the reduced grid
    assert (y1.double() - ref).abs().max() < 2e-5 * ref.abs().max() and (y0 - y1).abs().max() < 2e-5 * ref.abs().max()
    assert (dw0 - dw1).abs().max() < 2e-5 * dw0.abs().max()
    y3 = ops.conv3x3_forward(x, w, split=True)
    assert torch.equal(y0, y3)


def test_bench_eight_ranks_config3_code_path():
    """BASELINE config[3]'s rank count (8 processes, `--gpus 8`), one rank per GPU, exchanging over gloo, one image per rank -- the
    launcher / rank / barrier / MAX-over-ranks / flat all-reduce code the 8-GPU scaling run executes, inside GPUTEST (VERDICT r03 next #4c;
    profiles/r03_config3_8ranks_one_gpu.json is the same run at bs32 per rank).  Eight ranks plus this process on a single device are more
    processes than one GPU may be shared among, so the test needs eight GPUs; the two-rank tests above cover the N > 1 path on one."""
    import torch
    n = torch.cuda.device_count()
    if n < 8:
        pytest.skip("needs 8 GPUs, found %d" % n)
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MIOPEN_LOG_LEVEL="1", SC_BENCH_BACKEND="gloo", OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1", "--batch", "1",
                        "--full", "--sustained", "0"], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len([l for l in r.stdout.splitlines() if l.startswith("{")]) == 1
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 8 and d["config"]["parallelism"] == "dp8" and d["config"]["global_batch"] == 8 and d["scaling"] == "weak"
    assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    assert d["allreduce"]["payload_bytes"] > 140e6 and "cpu_baseline" not in d and "workloads" not in d


def test_workloads_line():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sc_workloads_test", os.path.join(ROOT, "tools", "workloads.py"))
    w = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(w)
    out = w.level_grid_100(with_cpu=False)
    for k in ("workload", "ms", "algorithmic_flop", "algorithmic_bytes", "achieved", "peak", "unit", "bound", "frac"):
        assert k in out, k
    assert out["algorithmic_flop"] == 80640 * 101 ** 3 and 0 < out["frac"] < 1.0
    from oracle import build_chamfer_ref
    assert build_chamfer_ref.load_or_build() is not None, "oracle/_ref/chamfer_3D_ref.so missing and /root/reference absent: reference leg cannot run"
    c = w.chamfer(1, N=20000, with_cpu=False, with_reference_gpu=True)
    assert c["all_pairs"]["algorithmic_flop"] == 16.0 * 20000 * 20000 and 0 < c["all_pairs"]["frac"] < 1.0
    assert c["same_results_as_all_pairs"] is True and c["speedup_vs_all_pairs"] > 0 and c["ms"] > 0
    sc = c["surface_clouds"]                       # the evaluation's kind of cloud: surfaces a few cells apart
    assert sc["same_results_as_all_pairs"] is True and sc["ms"] > 0 and sc["all_pairs_ms"] > 0
    # the opt-in leg runs the reference's own kernels (oracle/_ref, prebuilt) on the SAME uniform clouds: bit-identical results.
    # this flag read `false` in the driver's record because the product buffers had been reused for other clouds.
    assert "reference_gpu" in c, "oracle/_ref/chamfer_3D_ref.so did not load"
    assert c["reference_gpu"]["same_results"] is True and c["reference_gpu"]["ms"] > 0
    assert "reference_gpu" not in w.chamfer(1, N=4096, with_cpu=False)          # never by default
