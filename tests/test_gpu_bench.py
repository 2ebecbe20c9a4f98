"""bench.py as it is started for every change: the plain run (`--gpus 1 --steps N --warmup W`) measures its headline and nothing
else, `--full` adds every other figure after the timed frames."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
# what a run measures besides its headline, by the key of the result line
FULL_ONLY = ("one_frame_in_flight", "procedural_track", "ms_per_step_instrumented", "roofline", "hashgrid_lookup", "mfma", "train",
             "cpu_baseline")


def _bench(args, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), wall


def test_plain_run_measures_the_headline_only_and_spends_at_most_30_s_outside_its_steps(tmp_path):
    """The whole run, from the start of a new process to its exit, less (steps + warmup) x ms_per_step, is what the run spends
    outside its steps: at most 30 s (set-up, graph capture and spin-up included; measured 3.2 - 4.0 s on MI355X, against
    27 - 30 s while a default run still carried the training legs, the CPU baseline and the instrumented pass)."""
    n, w = 20, 5
    r, wall = _bench(["--gpus", "1", "--steps", str(n), "--warmup", str(w), "--dump-outputs", str(tmp_path / "dump")], timeout=600)
    outside = wall - (n + w) * r["ms_per_step"] * 1e-3
    print("plain run: %.1f s in all, %.3f ms per step, %.1f s outside the steps" % (wall, r["ms_per_step"], outside))
    assert outside <= 30.0
    assert all(k in r for k in HEADLINE) and r["full"] is False
    assert r["metric"] == "novel_pose_render_frames_per_sec_512x512" and r["unit"] == "frames/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f32" and r["steps"] == n and r["warmup"] == w and r["frames_per_rank"] == [n]
    assert abs(r["value"] * r["ms_per_step"] * 1e-3 - 1.0) < 1e-9          # one GPU: value = 1 / time per step
    assert r["samples_per_ray"] > 0 and 0.02 < r["alpha_coverage"] < 1
    assert not [k for k in FULL_ONLY if k in r]
    assert sorted(os.listdir(tmp_path / "dump")) == ["alpha.npy", "counter.npy", "depth.npy", "rgb.npy"]
    assert sorted(r["dump_outputs"]["arrays"]) == ["alpha", "counter", "depth", "rgb"]


def test_full_run_adds_every_other_figure_to_the_same_headline():
    r, wall = _bench(["--gpus", "1", "--steps", "20", "--warmup", "5", "--train-steps", "20", "--full"], timeout=600)   # exit 0 within 10 minutes
    print("--full run: %.1f s in all" % wall)
    assert all(k in r for k in HEADLINE) and r["full"] is True
    assert r["metric"] == "novel_pose_render_frames_per_sec_512x512" and r["steps"] == 20 and r["frames_per_rank"] == [20]
    assert not [k for k in FULL_ONLY if k not in r]
    assert r["one_frame_in_flight"]["frame_latency_ms"] > 0 and r["procedural_track"]["frames_per_s"] > 0
    assert r["ms_per_step_instrumented"] > 0 and r["roofline"]["kernel"] in ("k_search", "k_field") and r["roofline"]["achieved"] > 0
    assert r["hashgrid_lookup"]["Gsamples_per_s"] > 0 and "error" not in r["hashgrid_lookup"]["frame_coherent"]
    t = r["train"]
    assert "error" not in t and t["it_per_sec"] > 0 and t["uniform_rays"]["it_per_sec"] > 0
    assert "error" not in t["refine"] and t["refine"]["it_per_sec"] > 0 and "error" not in t["fit_stage"] and t["fit_stage"]["it_per_sec"] > 0
    assert r["cpu_baseline"]["value"] > 0 and len(r["cpu_baseline"]["frame_seconds"]) == 3
