"""xGMI peer all-reduce (IPC + one fused kernel) with 2 and 4 processes sharing the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", [2, 4])
def test_xgmi_allreduce_multiprocess(tmp_path, world):
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.dist_workers import xgmi_spawn_main; " \
           f"xgmi_spawn_main({str(tmp_path)!r}, {world})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rank in range(world):
        z = dict(np.load(tmp_path / f"xgmi{rank}.npz"))
        for k, v in z.items():
            if k.startswith("ok_") or k in ("sgd_ok", "planes_exact"):
                assert float(v) == 1.0, (rank, k)
            elif k.startswith("ar_"):
                assert float(v) < (1e-6 if "float32" in k else 1e-14), (rank, k, float(v))
        assert float(z["sgd_err"]) < 1e-4
        assert float(z["trainer_w1_diff"]) < 1e-5 and float(z["trainer_w2_diff"]) < 1e-5
        for H in (300, 1024):  # 2 ranks: a+b is exact in any order -> bitwise; 4 ranks: rounding only
            assert float(z[f"bucketed_diff_{H}"]) <= (0.0 if world == 2 else 1e-6), (H, float(z[f"bucketed_diff_{H}"]))


def test_xgmi_stress_four_ranks():
    """Many back-to-back all-reduces (both buffer halves, all epochs) with 4 ranks on one GPU: no stale reads."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "stress_xgmi.py"), "4", "10"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "bad_elements=0" in r.stdout, r.stdout[-2000:]


def test_xgmi_fused_wgrad_stress_two_ranks():
    """200 data-parallel steps with the all-reduce fused into the wgrad launch == the same steps through
    the separate all-reduce kernel, bitwise, on both ranks."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "stress_fused.py"), "2", "200"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fused_ranks=2 bad_elements=0" in r.stdout, r.stdout[-2000:]


def test_allreduce_bench_two_ranks_shared_gpu(tmp_path):
    """bench/allreduce_bench.py end to end (xGMI kernel path, 2 ranks sharing the GPU): every size correct."""
    import json

    out = tmp_path / "ar.json"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29661",
                        os.path.join(ROOT, "bench", "allreduce_bench.py"), "--paths", "xgmi", "xgmi-bf16", "--max-bytes",
                        str(1 << 20), "--iters", "5", "--json", str(out)],
                       capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, CME_SHARED_GPU="1", OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    recs = json.loads(out.read_text())
    assert len(recs) >= 5 and all(x["correct"] and x["peer_wait_timeouts"] == 0 for x in recs), recs


def test_xgmi_stalled_peer_applies_nothing_and_fails_everywhere(tmp_path):
    """Fault hook for the peer-to-peer all-reduce: rank 1 skips a step.  Rank 0's bounded waits time out,
    and neither the separate kernel nor the all-reduce fused into the wgrad launch changes a parameter or
    a bf16 plane; a rank in error is a no-op afterwards (no second wait, nothing published), and the
    collective check raises CommFailure on BOTH ranks at the end of the next epoch."""
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.dist_workers import xgmi_stall_main; " \
           f"xgmi_stall_main({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z0 = dict(np.load(tmp_path / "stall0.npz"))
    z1 = dict(np.load(tmp_path / "stall1.npz"))
    assert float(z0["A_first_ok"]) == 1.0 and float(z1["A_first_ok"]) == 1.0
    assert float(z0["A_err"]) == 1.0 and float(z0["A_untouched"]) == 1.0, z0
    # the peer wait is bounded by WALL time (s_memrealtime, 2 s: csrc/common/hip_common.h kPeerWaitUs), not by a
    # poll count: the stalled peer is detected within 3 s
    assert 1.5 <= float(z0["A_timeout_s"]) <= 3.0, z0
    assert float(z0["A_after_untouched"]) == 1.0 and float(z0["A_after_s"]) < 0.5 * float(z0["A_timeout_s"]), z0
    for z in (z0, z1):
        assert float(z["A_collective_err"]) == 1.0
        assert float(z["B_fused"]) == 1.0
        assert float(z["B_comm_failed"]) == 1.0
        assert float(z["B_raised"]) == 1.0, z
    # rank 0 (in error) applies nothing in the whole epoch; rank 1 may complete ONE more step on the
    # complete tile rank 0 published before its wait timed out, then times out itself
    assert float(z0["B_untouched"]) == 1.0 and float(z0["B_epoch_untouched"]) == 1.0, z0


def test_dp_paths_shared_gpu_rehearsal(tmp_path):
    """The one-rank-per-GPU DP test's worker, rehearsed with 2 ranks sharing GPU 0 over gloo (every path
    except RCCL itself): replicas bitwise equal, result == the single-process run of the same global batch."""
    res = _run_multigpu(tmp_path, 2, "gloo", ("xgmi-fused", "xgmi-push", "xgmi", "xgmi-bf16wire", "xgmi-2shot",
                                              "xgmi-2shot-f32", "rccl", "host"), ("weak", "strong"),
                        dict(os.environ, CME_SHARED_GPU="1", OMP_NUM_THREADS="2"))
    for s in ("weak", "strong"):  # the owner-tile push form leaves the one-shot's bits
        assert res[f"xgmi-push/{s}"]["digest"] == res[f"xgmi-fused/{s}"]["digest"], s


def test_dp_owner_tile_push_four_ranks_shared_gpu(tmp_path):
    """The owner-tile push form of the fused all-reduce (tile t reduced and applied by rank t % 4, pushed both ways
    as tagged granules) with 4 ranks sharing GPU 0 at H = 32 (every rank's fused launch co-resident): replicas
    bitwise equal, bitwise the one-shot (pull) form's result, and == the single-process run of the global batch."""
    res = _run_multigpu(tmp_path, 4, "gloo", ("xgmi-fused-h32", "xgmi-push-h32"), ("weak", "strong"),
                        dict(os.environ, CME_SHARED_GPU="1", OMP_NUM_THREADS="2"))
    for s in ("weak", "strong"):
        assert res[f"xgmi-push-h32/{s}"]["digest"] == res[f"xgmi-fused-h32/{s}"]["digest"], s


def test_dp_two_shot_four_ranks_shared_gpu(tmp_path):
    """The two-shot xGMI all-reduce (chunk owner = chunk % world) with 4 ranks sharing GPU 0: replicas bitwise
    equal and the data-parallel result == the single-process run of the same global batch."""
    _run_multigpu(tmp_path, 4, "gloo", ("xgmi-2shot", "xgmi-2shot-f32"), ("weak",),
                  dict(os.environ, CME_SHARED_GPU="1", OMP_NUM_THREADS="2"))


def _run_multigpu(tmp_path, world, backend, modes, scalings, env):
    import json

    code = (f"import sys; sys.path.insert(0, {ROOT!r}); from tests.dist_workers import multigpu_dp_main; "
            f"multigpu_dp_main({str(tmp_path)!r}, {world}, {modes!r}, {scalings!r}, 3, {backend!r})")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads((tmp_path / "multigpu.json").read_text())
    assert set(res) == {f"{m}/{s}" for m in modes for s in scalings}, res
    for key, v in res.items():
        assert v["replicas_equal"], (key, v)
        assert v["moved"] > 0, (key, v)
        # fp32 paths: reassociation only; the bf16 wire rounds each rank's gradient to bf16 (2^-9), and the
        # bf16 compute path (xgmi-2shot at H = 1024) re-rounds its bf16 weight shadow after reassociated sums
        bf16ish = "bf16wire" in key or key.startswith("xgmi-2shot/")
        assert v["rel_vs_single"] <= (2e-3 if bf16ish else 2e-6), (key, v)
        if key.startswith("xgmi"):
            assert v["impl"] == key.split("/")[0].replace("-2shot-f32", "-2shot").replace("-h32", ""), (key, v)
    return res


def _gpus() -> int:
    try:
        import torch

        return torch.cuda.device_count()
    except Exception:  # pragma: no cover
        return 0


@pytest.mark.parametrize("world", [2, 4, 8])
def test_dp_one_rank_per_gpu(tmp_path, world):
    """One process per GPU over RCCL (skipped unless >= world GPUs are visible): every all-reduce path
    (xGMI fused / separate kernel, RCCL incl. the bucketed side-stream backward at H=4096 captured in a HIP
    graph, host-staged) at weak and strong scaling against the single-process run of the same global batch."""
    if _gpus() < world:
        pytest.skip(f"needs {world} GPUs, {_gpus()} visible")
    modes = ("xgmi-fused", "xgmi-push", "xgmi", "xgmi-bf16wire", "xgmi-2shot", "xgmi-2shot-f32", "rccl",
             "rccl-bucketed", "host")
    _run_multigpu(tmp_path, world, "nccl", modes, ("weak", "strong"), dict(os.environ, OMP_NUM_THREADS="2"))


@pytest.mark.parametrize("world,H", [(2, 1024), (4, 4096)])
def test_tensor_parallel_xgmi_z2_allreduce(tmp_path, world, H):
    """BASELINE config 4's chosen plan: hidden-sharded training whose only collective, the 16 x B z2 SUM, runs
    on the xGMI one-shot kernel (ranks sharing the GPU here) == single-process training of the full model."""
    import json

    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.dist_workers import tp_xgmi_main; " \
           f"tp_xgmi_main({str(tmp_path)!r}, {world}, {H})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads((tmp_path / "tp_xgmi.json").read_text())
    assert res["impl"] == "xgmi-z2" and not res["failed"], res
    assert res["rel"] < 1e-5 and res["b_err"] < 1e-6, res


@pytest.mark.parametrize("gpus", [2, 4])
def test_bench_tunes_allreduce_shared_gpu(gpus):
    """bench.py --gpus N (self-launched, N ranks on GPU 0): the gradient sync is chosen by measurement -- the
    policy's xGMI pick (the fused pull), the fused owner-tile push, the xGMI two-shot (N >= 3) and the communicator's
    all-reduce each run the probe, every
    timing is in the record, the fastest ran the timed region, and the record is valid (replicas bitwise equal)."""
    import json

    env = dict(os.environ, CME_SHARED_GPU="1", OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "20",
                        "--warmup", "5", "--tune-steps", "20"], capture_output=True, text=True, timeout=600, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    cfg = rec["config"]
    tune = cfg["allreduce_tuning_us_per_step"]
    assert rec["n_gpus"] == gpus and cfg["ranks_seen"] == gpus and cfg["replicas_bitwise_equal"], rec
    # (the policy's pick, the two-shot at N >= 3, RCCL; and where the pick is the fused one-shot pull, the fused
    # owner-tile push too -- four ranks on one GPU do not get the fused form: its launch needs the whole GPU)
    fused = "xgmi-fused" in tune
    assert len(tune) == (2 if gpus == 2 else 3) + fused and any(k.startswith("xgmi") for k in tune), tune
    assert fused == ("xgmi-push" in tune), tune
    nums = {k: v for k, v in tune.items() if isinstance(v, (int, float))}
    assert nums and cfg["allreduce"] == min(nums, key=nums.get), (cfg["allreduce"], tune)


def test_bench_probes_dp_vs_tp_and_records_prediction():
    """bench.py --gpus 2 on a wide layer (784-1024-10, global batch 1600; 2 ranks sharing GPU 0): with
    --parallel auto the data- and tensor-parallel steps are both probed, the faster one is timed, and the record
    carries the probes, the chosen parallelism, the measured all-reduce and the cost model's prediction
    (allreduce_pred_us); the weak-scaling run rides along as the secondary sub-record."""
    import json

    env = dict(os.environ, CME_SHARED_GPU="1", OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--hidden", "1024",
                        "--batch", "1600", "--steps", "10", "--warmup", "2", "--tune-steps", "10", "--full"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    cfg = rec["config"]
    probes = cfg["parallel_tuning_us_per_step"]
    assert set(probes) == {"dp2", "tp2"}, probes
    nums = {k: v for k, v in probes.items() if isinstance(v, (int, float))}
    assert nums and cfg["parallelism"] == min(nums, key=nums.get), (cfg["parallelism"], probes)
    assert cfg["allreduce_pred_us"] > 0 and cfg["allreduce_us"] > 0, cfg
    assert rec["scaling"] == "strong" and cfg["global_batch"] == 1600
    assert rec["weak"]["global_batch"] == 3200 and rec["weak"]["parallelism"] == cfg["parallelism"]


def test_bench_probe_budget_skips_candidates():
    """A zero probe budget: the all-reduce policy's own pick still runs, every other candidate is recorded as
    'skipped: budget' and the timed region runs the pick."""
    import json

    env = dict(os.environ, CME_SHARED_GPU="1", OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "10",
                        "--warmup", "2", "--tune-steps", "10", "--tune-budget-s", "0", "--secondary", "off"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    tune = rec["config"]["allreduce_tuning_us_per_step"]
    assert "skipped: budget" in tune.values(), tune
    assert "weak" not in rec
