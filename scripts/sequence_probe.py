#!/usr/bin/env python3
"""What a camera sequence buys: the facing headline scene at
800x600x100, depth 50, seen from a 20-camera look-at orbit of 360 degrees.

  a_new    one rt_context_render_cameras_async launch of the 20 cameras, its
           schedule (the union live list) built inside the timing: a sequence
           rendered once
  a_again  the same launch with the schedule already there (other seeds)
  b        what a user does without the entry point: per frame,
           rt_context_set_scene with that camera, then rt_context_render_async
  c        rt_context_render_frames_async, 20 seeds of the first camera: the
           ceiling (one camera, its schedule already there)

The variants alternate in one process, `--rounds` runs each (wall clock around
the calls and the synchronize that follows; each variant has a context of its
own).  Printed: one JSON line per variant with the median, min and max of the
launch's milliseconds, ms per frame and Mrays/s, then the union's live pixels
(rt_context_stats.stream_live_pixels) next to every frame's own live count.

    python scripts/sequence_probe.py [--rounds 7] [--frames 20] [--out FILE]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "concurrent-raytracer-go_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rtgo  # noqa: E402

SCENE = os.path.join(ROOT, "scenes", "sphere_reflections_light_facing.json")
W, H, SPP, DEPTH = 800, 600, 100, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    n = args.frames
    base = json.load(open(SCENE))
    cams = rtgo.camera_orbit(base["camera"], n, 360.0)
    scenes = []
    for cam in cams:  # (b)'s scenes, made ahead: a user has them, or edits one
        d = copy.deepcopy(base)
        d["camera"] = cam
        scenes.append(rtgo.Scene.from_json_text(json.dumps(d)))
    st = rtgo.default_settings()
    st.samples, st.max_depth, st.camera = SPP, DEPTH, rtgo.RT_CAMERA_LOOKAT
    lin = torch.zeros((n, W * H * 3), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((n, W * H * 4), dtype=torch.uint8, device="cuda")
    lp, rp = [lin[f].data_ptr() for f in range(n)], [rgba[f].data_ptr() for f in range(n)]
    ctx = {k: rtgo.Context(0) for k in ("a", "b", "c")}
    for c in ctx.values():
        c.set_scene(scenes[0])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def run_a(seed0):
        ctx["a"].render_cameras_async(W, H, st, cams, lp, rp, seeds=[seed0 + f for f in range(n)])

    def run_b(seed0):
        for f in range(n):
            st.seed = seed0 + f
            ctx["b"].set_scene(scenes[f])
            ctx["b"].render_async(W, H, st, lp[f], rp[f], 0)
        st.seed = 1

    def run_c(seed0):
        ctx["c"].render_frames_async(W, H, st, [seed0 + f for f in range(n)], lp, rp, 0)

    ms = {"a_new": [], "a_again": [], "b": [], "c": []}
    built = {}
    for r in range(args.rounds + 1):  # (round 0 warms every variant up and is dropped)
        seed0 = 1000 * r + 1
        ctx["a"].set_scene(scenes[0])  # a new scene generation: a_new builds its schedule
        b0 = ctx["a"].stats()["schedules_built"]
        row = {"a_new": timed(lambda: run_a(seed0))}
        built["a_new"] = ctx["a"].stats()["schedules_built"] - b0
        b0 = ctx["a"].stats()["schedules_built"]
        row["a_again"] = timed(lambda: run_a(seed0 + 100))
        built["a_again"] = ctx["a"].stats()["schedules_built"] - b0
        b0 = ctx["b"].stats()["schedules_built"]
        row["b"] = timed(lambda: run_b(seed0))
        built["b"] = ctx["b"].stats()["schedules_built"] - b0
        run_c(seed0)  # (its schedule, outside the timing)
        b0 = ctx["c"].stats()["schedules_built"]
        row["c"] = timed(lambda: run_c(seed0 + 100))
        built["c"] = ctx["c"].stats()["schedules_built"] - b0
        if r > 0:
            for k, v in row.items():
                ms[k].append(v)
    union = ctx["a"].stats()["stream_live_pixels"]
    a_stats = ctx["a"].stats()
    rays = n * W * H * SPP / 1e6
    lines = []
    for k in ("a_new", "a_again", "b", "c"):
        v = ms[k]
        med = statistics.median(v)
        lines.append({"variant": k, "frames": n, "runs": len(v), "ms_median": round(med, 3), "ms_min": round(min(v), 3),
                      "ms_max": round(max(v), 3), "ms_per_frame": round(med / n, 4),
                      "mrays_per_s_median": round(rays / (med * 1e-3), 1),
                      "mrays_per_s_min": round(rays / (max(v) * 1e-3), 1),
                      "mrays_per_s_max": round(rays / (min(v) * 1e-3), 1), "schedules_built_per_run": built[k]})
    # every frame's own live pixels: a streamed one-sample render of the scene with that camera
    own = rtgo.Context(0)
    own.set_tuning(rtgo.default_tuning(stream=1))
    st1 = rtgo.default_settings()
    st1.samples, st1.max_depth, st1.camera = 1, DEPTH, rtgo.RT_CAMERA_LOOKAT
    per_frame = []
    for f in range(n):
        own.set_scene(scenes[f])
        own.render_async(W, H, st1, lp[0], rp[0], 0)
        torch.cuda.synchronize()
        per_frame.append(int(own.stats()["stream_live_pixels"]))
    lines.append({"pixels": W * H, "union_live_pixels": int(union), "frame_live_pixels": per_frame,
                  "frame_live_mean": round(statistics.mean(per_frame), 1),
                  "stream_launches_of_a": int(a_stats["stream_launches"]), "batched_launches_of_a": int(a_stats["batched_launches"])})
    a, b = statistics.median(ms["a_new"]), statistics.median(ms["b"])
    lines.append({"b_over_a_new": round(b / a, 3), "b_over_a_again": round(b / statistics.median(ms["a_again"]), 3),
                  "a_again_over_c": round(statistics.median(ms["a_again"]) / statistics.median(ms["c"]), 3)})
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for c in list(ctx.values()) + [own]:
        c.close()


if __name__ == "__main__":
    main()
