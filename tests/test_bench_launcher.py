"""`python bench.py --gpus N` must start N ranks itself and never measure fewer.

The driver's SCALE step calls `bench.py --gpus N` (and, for N > 1, the same under torch.distributed.run).  Both forms are covered
here without a GPU: the launcher's refusals on the real script, and the whole entry — launcher, two gloo ranks, timed region, JSON
line — through tests/bench_cpu_entry.py on the CPU port with a scene cut down for host cores.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
SMALL = ["--steps", "2", "--warmup", "1", "--settle-iters", "0", "--scene", "none", "--no-mc", "--no-hbm-kernels", "--no-cpu-baseline", "--no-config2",
         "--no-alt-mode", "--no-kernel-events", "--no-curves"]


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(OMP_NUM_THREADS="2", **kw)
    return env


def test_gpus_n_without_n_devices_exits_non_zero():
    """No GPU in this container: `--gpus 2` must refuse (exit 2) instead of running one rank and printing n_gpus 1."""
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2"] + SMALL, env=_env(HIP_VISIBLE_DEVICES="",
                       CUDA_VISIBLE_DEVICES=""), capture_output=True, text=True, timeout=600)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert "refusing to measure fewer ranks" in r.stderr and not r.stdout.strip()


def test_world_size_that_contradicts_gpus_is_refused():
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "4"] + SMALL,
                       env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--gpus 4 but WORLD_SIZE=2" in r.stderr and not r.stdout.strip()


def _line(args, **env):
    r = subprocess.run([sys.executable, str(REPO / "tests" / "bench_cpu_entry.py")] + args + SMALL, env=_env(**env),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "rank 0 prints ONE JSON line: %r" % r.stdout[-500:]
    return json.loads(lines[0])


def test_gpus_2_launches_two_ranks_with_identical_replicas():
    """The entry with `--gpus 2` and no torchrun environment: two ranks over gloo, one line with n_gpus 2, a step time per rank,
    the shared-gradient exchange timed and replicas bit-identical after the run (both with --full); twice the frames of the
    one-rank job per step."""
    two = _line(["--gpus", "2", "--full"])
    assert two["n_gpus"] == 2 and two["scaling"] == "weak" and two["steps"] == 2
    cfg = two["config"]
    assert len(cfg["per_rank_ms_per_step"]) == 2 and all(v > 0 for v in cfg["per_rank_ms_per_step"])
    assert cfg["shared_grad_allreduce_us"] > 0 and cfg["shared_grad_bytes"] > 1e6
    assert cfg["replicas_bit_identical"] is True
    assert "dp2" in cfg["parallelism"]
    assert abs(two["value"] - 2 * 1e3 / two["ms_per_step"]) < 1e-2 * two["value"]       # whole-job rate: N iterations per step time
    one = _line(["--gpus", "1"])
    assert one["n_gpus"] == 1 and one["config"]["per_rank_ms_per_step"] is None and one["config"]["replicas_bit_identical"] is None


def test_plain_run_times_the_steps_only_and_dumps_its_last_step(tmp_path):
    """A plain run (no --full, none of the --no-* options) leaves out everything beyond the headline, and --dump-outputs writes what
    its last timed step computed: float32 / float64 arrays under 64 MB, the ray count of the LAST step (the line's average differs),
    and the same arrays bit for bit when the same command runs again."""
    plain = ["--steps", "3", "--warmup", "1", "--settle-iters", "0", "--scene", "none", "--no-curves"]
    runs = []
    for k in range(2):
        r = subprocess.run([sys.executable, str(REPO / "tests" / "bench_cpu_entry.py"), "--gpus", "1",
                            "--dump-outputs", str(tmp_path / str(k))] + plain, env=_env(), capture_output=True, text=True,
                           timeout=1500)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-500:]
        runs.append(json.loads(lines[0]))
    line = runs[0]
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["config"]["replicas_bit_identical"] is None
    for key in ("roofline", "cpu_baseline", "hbm_kernels", "config2", "high_convergence", "full_load", "mc_extract_ms_257",
                "busy_fraction_timed_region"):
        assert key not in line, key
    assert line["matrix_tflop_per_step"] is None
    out = [{p.stem: np.load(p) for p in (tmp_path / str(k)).glob("*.npy")} for k in range(2)]
    assert {"loss", "rays", "mesh.garment_vs.0", "model.sdf.lin0.weight_v", "dataset.poses"} <= set(out[0]), sorted(out[0])
    assert all(a.dtype in (np.float32, np.float64) for a in out[0].values())
    assert sum(a.nbytes for a in out[0].values()) <= 64 * 10 ** 6
    assert np.isfinite(out[0]["loss"]).all() and out[0]["loss"].shape == ()
    assert out[0]["rays"] == line["config"]["rays_per_iter"]              # the last step's count, not the line's average
    assert out[0]["mesh.garment_vs.0"].ndim == 2 and out[0]["mesh.garment_vs.0"].shape[1] == 3
    assert set(out[0]) == set(out[1]) and all(np.array_equal(out[0][k], out[1][k]) for k in out[0])


def test_dump_outputs_samples_large_arrays_and_keeps_small_ones(tmp_path, monkeypatch):
    """bench.dump_outputs over its size limit: arrays above DUMP_KEEP_WHOLE elements are cut to one seeded sample (the same
    on every call), the returned scalars and small tensors are written whole."""
    import types
    import torch
    sys.path.insert(0, str(REPO))
    import bench
    gen = torch.Generator().manual_seed(3)
    ds = types.SimpleNamespace(**{k: torch.randn(4, 3, generator=gen) for k in bench._SCENE_DATASET})
    loop = types.SimpleNamespace(_BUFFERS=(), dataset=ds, garment_vs=[torch.randn(50000, 3, generator=gen)])
    state = {"sdf.lin0.weight_v": torch.randn(512, 512, generator=gen), "sdf.lin0.bias": torch.randn(512, generator=gen)}
    loop.state_dict = lambda: state
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 400_000)
    for k in range(2):
        bench.dump_outputs(loop, torch.tensor(1.5), 84, tmp_path / str(k))
    out = [{p.stem: np.load(p) for p in (tmp_path / str(k)).glob("*.npy")} for k in range(2)]
    assert out[0]["loss"] == np.float32(1.5) and out[0]["rays"] == 84.0 and out[0]["rays"].dtype == np.float64
    np.testing.assert_array_equal(out[0]["model.sdf.lin0.bias"], state["sdf.lin0.bias"].numpy())
    np.testing.assert_array_equal(out[0]["dataset.poses"], ds.poses.numpy())
    w = out[0]["model.sdf.lin0.weight_v"]
    assert w.ndim == 1 and 0 < w.size < 512 * 512 and np.isin(w, state["sdf.lin0.weight_v"].numpy()).all()
    assert sum(a.nbytes for a in out[0].values()) <= 400_000
    assert all(np.array_equal(out[0][k], out[1][k]) for k in out[0])


def test_frames_at_counts_the_short_last_batch_of_an_epoch():
    """bench.frames_at: frames a rank takes in iteration `it` — batch_size except at an epoch's last position (64 frames, 3 per step:
    every 22nd iteration has one frame), the same deal HotLoop.frame_batch_at makes, also when frames are sharded over ranks."""
    import types
    sys.path.insert(0, str(REPO))
    import bench
    from recmv.loop import iters_per_epoch

    def fake(F, bs, world, rank):
        loop = types.SimpleNamespace(batch_size=bs, world_size=world, rank=rank, dataset=types.SimpleNamespace(F=F))
        loop.iters_per_epoch = lambda: iters_per_epoch(F, bs, world)
        return loop
    one = fake(64, 3, 1, 0)
    assert one.iters_per_epoch() == 22
    assert [bench.frames_at(one, it) for it in range(22)] == [3] * 21 + [1]
    assert bench.frames_at(one, 22 + 5) == 3 and bench.frames_at(one, 43) == 1
    two = [fake(64, 3, 2, r) for r in range(2)]
    assert two[0].iters_per_epoch() == 11
    assert [bench.frames_at(two[0], it) for it in range(11)] == [3] * 10 + [2]
    assert [bench.frames_at(two[1], it) for it in range(11)] == [3] * 10 + [2]
    # fewer remaining frames than ranks: the permutation wraps so that every rank still has one
    three = [fake(10, 3, 3, r) for r in range(3)]            # 9 per step, 2 positions, the second holds 1 frame for 3 ranks
    assert three[0].iters_per_epoch() == 2
    assert [bench.frames_at(three[r], 1) for r in range(3)] == [1, 1, 1]


def test_frozen_scene_round_trip_on_the_cpu_port(tmp_path):
    """bench.save_scene / load_scene: the tensors the optimisation moves and Adam's two moments go through the file (matrices of
    >= 2^14 elements as f16, moments as bf16), the loaded loop re-meshes from the file's SDF nets and continues right after that
    re-mesh; a file that does not describe the loop is refused."""
    import pytest
    import torch
    for p in (REPO / "rec-mv_amd", REPO):
        if str(p) not in sys.path:
            sys.path.insert(0, str(p))
    import bench
    from oracle import cpu_port
    sys.path.insert(0, str(REPO / "tests"))
    from test_loop_cpu import _tiny_loop
    cpu_port.install()
    try:
        a = _tiny_loop(curves=True)
        for it in range(3):
            a.step(it)
        path = str(tmp_path / "scene.pt")
        bench.save_scene(a, path, 2, note="test")
        b = _tiny_loop(curves=True, seed=5)                       # another seed: everything the file holds must be overwritten
        it0 = bench.load_scene(b, path)
        assert it0 == 3 and b.forward_time == 1 and b.opt_times == a.opt_times
        ta, tb = bench._scene_tensors(a), bench._scene_tensors(b)
        assert set(ta) == set(tb) and any(k.startswith("model.inter_free_curve.") for k in ta) and "dataset.poses" in ta
        for k in ta:
            x, y = ta[k].detach(), tb[k].detach()
            if x.is_floating_point() and x.numel() >= (1 << 14):
                assert torch.equal(y, x.half().float()), k        # the file's rounding, nothing else
            else:
                assert torch.equal(y, x), k
        pa = [q for g in a.optimizer.param_groups for q in g['params']]
        pb = [q for g in b.optimizer.param_groups for q in g['params']]
        seen = 0
        for qa, qb in zip(pa, pb):
            if qa in a.optimizer.state:
                sa, sb = a.optimizer.state[qa], b.optimizer.state[qb]
                assert float(sb['step']) == float(sa['step']) == 3.0
                assert torch.equal(sb['exp_avg'], sa['exp_avg'].bfloat16().float())
                assert torch.equal(sb['exp_avg_sq'], sa['exp_avg_sq'].bfloat16().float())
                seen += 1
        assert seen > 20
        assert [tuple(v.shape) for v in b.garment_vs] and all(v.requires_grad for v in b.garment_vs)
        loss, rays = b.step(it0)                                  # and the loop runs on from there
        assert torch.isfinite(loss) and rays > 0 and b.forward_time == 2
        c = _tiny_loop(curves=False)                              # no curve branch: the file has tensors this loop lacks
        with pytest.raises(SystemExit):
            bench.load_scene(c, path)
    finally:
        cpu_port.uninstall()
