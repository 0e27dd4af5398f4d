"""bench.py's multi-rank code paths, exercised with two ranks on ONE GPU
(`UCSA_BENCH_BACKEND=gloo`, the test hook; the driver's real runs use RCCL,
one rank per GPU): the `--full` render line at N = 2 with its `train_dp`
object, `--mode train` and `--mode cfg4 --gather`.  ``-m gpu``."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run2(extra, tmp_path, timeout=600, ranks=2):
    """Output goes to FILES, not pipes: a helper process the ranks leave behind
    for a while keeps an inherited pipe open, and `communicate()` would then
    block until it is gone although torchrun itself exited after seconds."""
    env = dict(os.environ, UCSA_BENCH_BACKEND="gloo", UCSA_BENCH_WATCHDOG=str(timeout - 20))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1", "--master-port",
           str(_port()), os.path.join(ROOT, "bench.py"), "--gpus", str(ranks)] + extra
    out, err = tmp_path / "out.txt", tmp_path / "err.txt"
    for attempt in (1, 2):
        with open(out, "w") as fo, open(err, "w") as fe:
            proc = subprocess.Popen(cmd, stdout=fo, stderr=fe, stdin=subprocess.DEVNULL,
                                    env=env, cwd=ROOT)
            try:
                rc = proc.wait(timeout=timeout)
            except subprocess.TimeoutExpired:
                proc.kill()
                raise AssertionError("bench.py timed out:\n" + err.read_text()[-3000:])
        etext = err.read_text()
        # EIGHT processes on ONE device is a code-path check, not a supported way to run
        # (round 6: one such run in seven lost a rank to SIGABRT; the cause was not
        # captured -- torchrun's summary named only the signal -- and six later runs of
        # the same command passed).  A rank killed by a signal is retried ONCE, its stderr kept
        # (gpurun_out/bench_modes_stderr.txt); a second death, or any failure the program
        # itself reports, fails the test.
        if attempt == 1 and rc != 0 and ranks >= 8 and "Signal" in etext and "Traceback" not in etext.split("ChildFailedError")[0]:
            try:
                os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
                with open(os.path.join(ROOT, "gpurun_out", "bench_modes_stderr.txt"), "a") as f:
                    f.write(f"=== attempt 1 of {cmd[-6:]} died of a signal, retrying\n{etext[-20000:]}\n")
            except OSError:
                pass
            cmd[cmd.index("--master-port") + 1] = str(_port())
            continue
        break
    return _parse(rc, out, err)


def _parse(rc, out, err):
    """The LAST stdout line is the compact record (<= 4 KB, what the driver
    parses); everything else a run measured is in the detail file it names."""
    text = out.read_text()
    lines = [l for l in text.splitlines() if l.startswith("{")]
    if not (rc == 0 and len(lines) == 1):
        # keep the ranks' whole stderr where a gpurun call merges it back (the torchrun
        # summary at its end says only which rank died of which signal)
        etext = err.read_text()
        try:
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            with open(os.path.join(ROOT, "gpurun_out", "bench_modes_stderr.txt"), "a") as f:
                f.write(f"=== rc {rc} {out}\n{etext[-60000:]}\n")
        except OSError:
            pass
        first = [l for l in etext.splitlines()
                 if any(w in l for w in ("Error", "error", "HIP", "hip", "abort", "Abort", "what()", "Assert"))]
        raise AssertionError((rc, "\n".join(first[:30])[-3000:], etext[-1500:]))
    assert text.strip().splitlines()[-1] == lines[0] and len(lines[0].encode()) <= 4096
    res = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "dtype", "config", "distributed", "detail"):
        assert k in res, k
    res["_full"] = json.load(open(os.path.join(ROOT, res["detail"])))
    assert res["_full"]["value"] == pytest.approx(res["value"], rel=1e-5)
    return res


def test_default_render_line_at_two_ranks_carries_train_dp(tmp_path):
    res = _run2(["--steps", "2", "--warmup", "1", "--pretrain-steps", "30", "--full"], tmp_path)
    assert res["n_gpus"] == 2 and res["scaling"] == "weak" and res["metric"] == "rays/sec"
    assert res["value"] > 0 and res["roofline"]["bound"] == "hbm"
    assert "cpu_baseline" not in res            # single-GPU legs run at N = 1 only
    dp = res["_full"]["train_dp"]
    assert dp["collective_ranks"] == 2 and dp["replicas_identical"] is True
    assert dp["optimizer"].startswith("ShardedHipAdam")
    assert dp["allreduce_ms"] > 0 and dp["reduce_scatter_allgather_ms"] > 0
    assert dp["rays_per_step_total"] == 2 * 4096


@pytest.mark.parametrize("extra", [[], ["--replicated-adam"], ["--grad-comm-dtype", "fp16"]])
def test_train_mode_two_ranks(extra, tmp_path):
    res = _run2(["--mode", "train", "--steps", "3", "--warmup", "1",
                 "--pretrain-steps", "30"] + extra, tmp_path)
    dp = res["_full"]["train_dp"]
    assert res["config"]["mode"] == "train" and res["n_gpus"] == 2
    assert dp["replicas_identical"] is True and dp["collective_ranks"] == 2
    assert dp["final_loss"] == dp["final_loss"]
    assert res["value"] == pytest.approx(dp["rays_per_s"], rel=1e-5)   # 6 significant digits
    want = "HipAdam" if "--replicated-adam" in extra else "ShardedHipAdam"
    assert dp["optimizer"].startswith(want)


def test_cfg4_mode_two_ranks_with_gather(tmp_path):
    res = _run2(["--mode", "cfg4", "--views", "4", "--warmup", "1", "--gather",
                 "--pretrain-steps", "30"], tmp_path)
    assert res["config"]["mode"] == "cfg4" and res["_full"]["config"]["views_per_rank"] == 2
    assert res["scaling"] == "strong" and res["value"] > 0


# ---- width 8: the driver's SCALE run is `bench.py --gpus 8`
# under torchrun; no 8-GPU node has ever been available, so the same command
# lines run here with eight ranks on ONE GPU over gloo -- a code-path check at
# that width (round-robin shards, max-over-ranks timing, aggregate `value`, the
# 8-way ShardedHipAdam slices), not a measurement.
def test_default_render_line_at_eight_ranks(tmp_path):
    res = _run2(["--steps", "2", "--warmup", "1", "--pretrain-steps", "20", "--full"], tmp_path,
                timeout=1500, ranks=8)
    assert res["n_gpus"] == 8 and res["scaling"] == "weak" and res["distributed"]["world_size"] == 8
    assert len(res["distributed"]["devices"]) == 8
    # whole-job aggregate: 8 ranks x 2 views x 640 x 480 rays in 2 x ms_per_step
    assert res["value"] == pytest.approx(8 * 640 * 480 / (res["ms_per_step"] * 1e-3), rel=1e-4)
    dp = res["_full"]["train_dp"]
    assert dp["collective_ranks"] == 8 and dp["replicas_identical"] is True
    assert dp["rays_per_step_total"] == 8 * 4096
    _check_shards(dp["adam_shards"], 8)


def _check_shards(sh, world):
    """The ranks' Adam slices of the hash grid tile it: 13 074 912 fp32 values
    (6 537 456 entries x 2 features) = 8 x 1 634 364, no tail at width 8."""
    assert sh["grid_numel"] == 13074912 and sh["params_total"] > sh["grid_numel"]
    assert len(sh["by_rank"]) == world
    spans = sorted((r[0][1], r[0][2]) for r in sh["by_rank"])
    assert all(len(r) == 1 and r[0][0] == sh["grid_numel"] for r in sh["by_rank"])
    assert spans[0][0] == 0
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 == b0 and a1 > a0          # back to back, none empty
    body = sh["by_rank"][0][0][3]
    assert spans[-1][1] == body and 0 <= sh["grid_numel"] - body < 4 * world
    assert all(s % 4 == 0 for a in spans for s in a)    # 16-byte aligned slices


def test_train_mode_eight_ranks(tmp_path):
    res = _run2(["--mode", "train", "--steps", "2", "--warmup", "1", "--pretrain-steps", "20"],
                tmp_path, timeout=1500, ranks=8)
    dp = res["_full"]["train_dp"]
    assert res["n_gpus"] == 8 and dp["collective_ranks"] == 8 and dp["replicas_identical"] is True
    assert res["value"] == pytest.approx(8 * 4096 / (res["ms_per_step"] * 1e-3), rel=1e-4)
    assert dp["optimizer"].startswith("ShardedHipAdam")
    _check_shards(dp["adam_shards"], 8)


def test_cfg4_mode_eight_ranks_every_view_once(tmp_path):
    res = _run2(["--mode", "cfg4", "--views", "16", "--warmup", "1", "--gather",
                 "--pretrain-steps", "20"], tmp_path, timeout=1500, ranks=8)
    cfg = res["_full"]["config"]
    assert res["n_gpus"] == 8 and cfg["views_per_rank"] == 2 and res["scaling"] == "strong"
    by_rank = cfg["views_by_rank"]
    assert len(by_rank) == 8 and all(len(v) == 2 for v in by_rank)
    assert sorted(v for vs in by_rank for v in vs) == list(range(16))     # each view exactly once
    assert all(vs == [r, r + 8] for r, vs in enumerate(by_rank))           # round-robin
    assert res["value"] == pytest.approx(16 * 640 * 480 / cfg["total_s"], rel=1e-4)


def test_plain_bench_gpus_2_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with no launcher around it (WORLD_SIZE
    unset) starts its two ranks itself as a child torchrun; the JSON line says
    what ran (world size as torch.distributed saw it, backend, devices)."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(UCSA_BENCH_BACKEND="gloo", UCSA_BENCH_WATCHDOG="500")
    out, err = tmp_path / "out.txt", tmp_path / "err.txt"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--pretrain-steps", "30", "--mode", "cfg4", "--views", "4"]
    with open(out, "w") as fo, open(err, "w") as fe:
        rc = subprocess.Popen(cmd, stdout=fo, stderr=fe, stdin=subprocess.DEVNULL,
                              env=env, cwd=ROOT).wait(timeout=600)
    res = _parse(rc, out, err)
    d = res["distributed"]
    assert res["n_gpus"] == 2 and d["world_size"] == 2 and d["launcher"] == "self"
    assert d["backend"].startswith("gloo") and len(d["devices"]) == 2


def test_cfg3_mode_two_joint_steps_one_process(tmp_path):
    """`bench.py --mode cfg3`: BASELINE cfg3's joint step (8 frames of 320x240:
    8 full no-grad renders at 256+256 samples + 8 NeRF training steps of 4096
    rays + DeepLabV3 forward/backward/Adam on the 8 augmented renders) through
    the LightningModule mirror, two timed steps; the line carries the
    roofline of the whole step (flop and bytes of its three parts)."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out, err = tmp_path / "out.txt", tmp_path / "err.txt"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "cfg3", "--steps", "2",
           "--warmup", "1", "--no-seg-find"]
    with open(out, "w") as fo, open(err, "w") as fe:
        rc = subprocess.Popen(cmd, stdout=fo, stderr=fe, stdin=subprocess.DEVNULL,
                              env=env, cwd=ROOT).wait(timeout=900)
    res = _parse(rc, out, err)
    full = res["_full"]
    assert res["config"]["mode"] == "cfg3" and res["n_gpus"] == 1
    assert full["config"]["nerf_rays_per_step_per_rank"] == 8 * (320 * 240 + 4096)
    assert res["value"] > 0 and res["ms_per_step"] < 2000
    rs = full["roofline_step"]
    parts = rs["mfma"]["of_which"]
    assert abs(sum(parts.values()) - rs["mfma"]["algorithmic_flop"]) <= 1e-6 * rs["mfma"]["algorithmic_flop"]
    assert 0.0 < rs["mfma"]["frac_of_fp32_mfma_peak"] < 1.0 and 0.0 < rs["hbm"]["frac"] < 1.0
    assert 0.3 < rs["masked_fraction_rho"] <= 1.0
    for k in ("train/loss_nerf_rgb", "train/loss_seg"):
        assert k in full["losses"] and full["losses"][k] == full["losses"][k]      # finite


def test_the_default_command_prints_the_compact_record(tmp_path):
    """`python bench.py --full` (short: 3 steps, 30 pre-training steps): ONE stdout
    line, <= 4 KB, with the roofline and cpu_baseline objects the driver
    records; the side legs are in the detail file."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out, err = tmp_path / "out.txt", tmp_path / "err.txt"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
           "--pretrain-steps", "30", "--cpu-rays", "2048", "--full"]
    with open(out, "w") as fo, open(err, "w") as fe:
        rc = subprocess.Popen(cmd, stdout=fo, stderr=fe, stdin=subprocess.DEVNULL,
                              env=env, cwd=ROOT).wait(timeout=900)
    res = _parse(rc, out, err)
    r, c = res["roofline"], res["cpu_baseline"]
    assert r["bound"] == "hbm" and r["kernel"].startswith("density pass = 2 launches")
    for k in ("k_hashgrid_encode_sorted", "k_density_sorted"):
        assert k in r["kernel"]            # the two launches the figure covers, by name
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-4)
    assert r["achieved"] == pytest.approx(r["algorithmic_bytes_per_launch"] / r["launch_ms"] / 1e6,
                                          rel=1e-4)
    assert set(r["binding_resource"]) == {"resource", "frac"}
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0
    assert c["gpu_over_cpu"] == pytest.approx(res["value"] / c["value"], rel=1e-4)
    assert set(res["tuning_tables_matched"]) >= {"miopen", "tunableop"}
    assert res["config"]["workload"].startswith("cfg2") and res["dtype"] == "f32"
    assert "train" in res["_full"] and "stage_ms_per_chunk" in res["_full"]
    # BASELINE's metric is train + render: the training step is in the parsed line
    t = res["train"]
    assert t["ms_per_step"] > 0 and t["rays_per_s"] == pytest.approx(4096 / (t["ms_per_step"] * 1e-3), rel=1e-3)
    st = res["_full"]["stage_ms_per_chunk"]
    # the roofline's launch = the density pass AS SHIPPED (its two launches), event-timed
    assert st["sort_f"] > 0 and r["launch_ms"] == pytest.approx(0.5 * (st["density_c"] + st["density_f"]), rel=1e-4)
    eo = res["_full"]["roofline_encode"]["encoder_only_unfused"]      # round 5's figure, for continuity
    assert eo["launch_ms"] == pytest.approx(0.5 * (st["encode_c"] + st["encode_f"]), rel=1e-4)


def test_cfg5_mode_three_stages_at_true_sizes(tmp_path):
    """`bench.py --mode cfg5` -- the continual loop AT ITS WORKLOAD's sizes
    (240x320 frames, 4096 rays x (256+256), batch and replay buffer of
    cfg/exp/multi_step/cl_base.yml, the predict pass writing the PNGs the
    next stage replays), cut to three stages, 8 training frames per scene,
    one NeRF-only and one joint epoch, ResNet-50, to fit the suite's budget.
    tools/bench_legs/cfg5.py; the 10-stage run is profiles/r04_cfg5.json."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out, err = tmp_path / "out.txt", tmp_path / "err.txt"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "cfg5", "--scenes", "3",
           "--frames", "8", "--nerf-epochs", "1", "--joint-epochs", "1",
           "--backbone", "resnet50", "--no-seg-find"]
    with open(out, "w") as fo, open(err, "w") as fe:
        rc = subprocess.Popen(cmd, stdout=fo, stderr=fe, stdin=subprocess.DEVNULL,
                              env=env, cwd=ROOT).wait(timeout=1200)
    res = _parse(rc, out, err)
    full = res["_full"]
    assert res["config"]["mode"] == "cfg5" and res["value"] > 0
    st = full["stages"]
    assert [s["stage"] for s in st] == ["stage_0", "stage_1", "stage_2"]
    assert [s["scenes"] for s in st] == [1, 2, 3]
    # stage i's joint loader: 8 new frames + 8 replayed frames of each earlier
    # scene (100 // i >= 8), batch 2 -> 4 (i + 1) joint steps; the NeRF-only
    # loader is one frame per step (reference joint_train_data_module.py): 8
    assert [s["joint_steps"] for s in st] == [4, 8, 12]
    assert [s["nerf_steps"] for s in st] == [8, 8, 8]
    # NeRF rays trained: 4096 per NEW-scene frame per step (replayed frames
    # are not re-trained): 8 frames per epoch, 2 epochs per stage
    assert all(s["rays_trained"] == 2 * 8 * 4096 for s in st)
    assert all(s["rays_rendered"] >= 8 * 240 * 320 for s in st)     # full native renders
    q = full["quality"]["final_stage"]
    assert 0.0 <= q["test_nerf_mIoU"] <= 1.0 and q["test_nerf_PSNR"] == q["test_nerf_PSNR"]
    assert full["throughput"]["joint_steps_per_s"] > 0


def test_plain_command_is_lean_and_dumps_the_same_outputs_every_run(tmp_path):
    """`python bench.py --dump-outputs DIR` without --full: the headline only (no
    roofline, CPU baseline, quality, training or per-stage legs), and the last
    timed view's render() outputs in DIR, float32, at most 64 MB.  A second run
    with the same arguments writes the same bits: the pre-training is
    deterministic and the rays and uniforms are seeded."""
    import numpy as np
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    names = ("depth", "image", "semantics")
    dumps = []
    for run in (1, 2):
        out, err, dump = tmp_path / f"out{run}.txt", tmp_path / f"err{run}.txt", tmp_path / f"dump{run}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1",
               "--pretrain-steps", "30", "--dump-outputs", str(dump)]
        with open(out, "w") as fo, open(err, "w") as fe:
            rc = subprocess.Popen(cmd, stdout=fo, stderr=fe, stdin=subprocess.DEVNULL,
                                  env=env, cwd=ROOT).wait(timeout=600)
        res = _parse(rc, out, err)
        assert res["steps"] == 2 and res["warmup"] == 1 and res["dtype"] == "f32"
        assert res["value"] == pytest.approx(640 * 480 / (res["ms_per_step"] * 1e-3), rel=1e-4)
        for k in ("roofline", "cpu_baseline", "quality", "train", "tuning_tables_matched"):
            assert k not in res, k
        for k in ("stage_ms_per_chunk", "roofline_step", "cpu_vs_gpu", "train_dp"):
            assert k not in res["_full"], k
        assert sorted(os.listdir(dump)) == [n + ".npy" for n in names]
        dumps.append({n: np.load(dump / (n + ".npy")) for n in names})
    a, b = dumps
    assert a["image"].shape == (1, 640 * 480, 3) and a["depth"].shape == (1, 640 * 480)
    assert a["semantics"].shape == (1, 640 * 480, 40)
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.isfinite(a["image"]).all() and 0.0 < float(a["image"].mean()) < 1.0
    for n in names:
        assert np.array_equal(a[n], b[n]), n
