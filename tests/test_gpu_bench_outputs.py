"""bench.py's plain and --full runs and --dump-outputs: the
plain line holds the headline's keys only, --steps sets the timed steps, and
the dumped images are the last timed step's frame, bit for bit, the same from
a plain and a --full run.  Two short bench runs (2 spp)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu

BENCH = os.path.join(ROOT, "bench.py")
STEPS, SPP, SEED = 3, 2, 7
HEAD = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("one_frame_in_flight", "roofline", "first_frame_ms", "check_equals_oracle", "counts_rank0")


def bench(out_dir, *extra):
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--spp", str(SPP),
           "--seed", str(SEED), "--dump-outputs", str(out_dir)] + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), np.load(out_dir / "linear.npy"), np.load(out_dir / "rgba.npy")


@pytest.fixture(scope="module")
def last_step_frame():
    """The last timed step's frame (seed SEED + STEPS - 1), rendered on its own."""
    import rtgo
    from gpu_util import render_dev

    scene = rtgo.Scene.load_from_file(os.path.join(SCENES, "sphere_reflections_light_facing.json"))
    st = rtgo.default_settings()
    st.samples, st.max_depth, st.seed, st.num_workers = SPP, 50, SEED + STEPS - 1, 1
    lin, rgba, _, _ = render_dev(scene, 800, 600, st)
    return lin.reshape(600, 800, 3), rgba.reshape(600, 800, 4)


def check_dump(lin, rgba, frame):
    assert lin.dtype == np.float32 and lin.shape == (600, 800, 3)
    assert rgba.dtype == np.float32 and rgba.shape == (600, 800, 4)
    assert lin.nbytes + rgba.nbytes <= 64 * 1000 * 1000
    assert np.array_equal(lin.view(np.uint32), frame[0].view(np.uint32))
    assert np.array_equal(rgba, frame[1].astype(np.float32))
    assert (rgba[..., :3] > 0).any()


def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path, last_step_frame):
    line, lin, rgba = bench(tmp_path)
    for k in HEAD:
        assert k in line, k
    assert line["steps"] == STEPS and sum(line["launch_frames"]) == STEPS and line["full"] is False
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    # value is the frame's samples over ms_per_step (printed to 1e-4 ms: under 1 % of a step of >= 0.01 ms)
    assert line["ms_per_step"] >= 0.01
    assert abs(line["value"] - 800 * 600 * SPP / (line["ms_per_step"] * 1e-3) / 1e6) <= 1e-2 * line["value"]
    for k in FULL_ONLY + ("cpu_baseline", "render_e2e"):
        assert k not in line, k
    check_dump(lin, rgba, last_step_frame)


def test_full_run_adds_its_legs_and_dumps_the_same_frame(tmp_path, last_step_frame):
    line, lin, rgba = bench(tmp_path, "--full", "--no-cpu-baseline", "--no-e2e")
    for k in HEAD + FULL_ONLY:
        assert k in line, k
    assert line["steps"] == STEPS and line["full"] is True
    assert line["check_equals_oracle"] is True
    check_dump(lin, rgba, last_step_frame)
