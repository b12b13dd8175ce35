#!/usr/bin/env python3
"""What the opt-in look-at camera costs: information, no threshold.

Three views of the headline workload (bench.py's c2: 800x600, 100 samples,
depth 50, soft shadows and recursion on), each timed the same way -- launches
of B frames that differ in their seed (rt_context_render_frames_async) on one
context, one launch in flight, a host clock around work that ends in a device
synchronise, W launches of warm-up (the first builds the schedule):

  reference   sphere_reflections_light_facing.json, RT_CAMERA_REFERENCE
  identity    the same scene with lookAt = position + (0, 0, -1), up +Y, fov 90
              in RT_CAMERA_LOOKAT: the same rays bit for bit, so the difference
              is the look-at branch of the camera-ray code and of the culling
  committed   sphere_reflections_light.json through its OWN camera (z = -8,
              looking at the origin, fov 60): another image, another amount of
              work -- the scene as its author framed it

usage: camera_cost.py [--steps K] [--warmup W] [--frames-per-launch B] [--repeats R]
Prints one JSON line per view and repeat (views alternate within a repeat).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "concurrent-raytracer-go_amd"))
sys.path.insert(0, ROOT)

W, H, SPP = 800, 600, 100


def views(rtgo):
    sc = os.path.join(ROOT, "scenes")
    facing = json.load(open(os.path.join(sc, "sphere_reflections_light_facing.json")))
    ident = json.loads(json.dumps(facing))
    p = ident["camera"]["position"]
    ident["camera"].update(lookAt=[p[0], p[1], p[2] - 1], up=[0, 1, 0], fov=90)
    committed = json.load(open(os.path.join(sc, "sphere_reflections_light.json")))
    return [("reference", facing, rtgo.RT_CAMERA_REFERENCE), ("identity", ident, rtgo.RT_CAMERA_LOOKAT),
            ("committed", committed, rtgo.RT_CAMERA_LOOKAT)]


class View:
    def __init__(self, rtgo, torch, name, scene, camera, B):
        self.name, self.B = name, B
        self.ctx = rtgo.Context(0)
        self.ctx.set_scene(rtgo.Scene.from_json_text(json.dumps(scene)))
        self.st = rtgo.default_settings()
        self.st.samples, self.st.max_depth, self.st.camera = SPP, 50, camera
        self.lin = [torch.zeros(W * H * 3, dtype=torch.float32, device="cuda") for _ in range(B)]
        self.stream = torch.cuda.Stream()
        self.seed = 1

    def launch(self):
        seeds = list(range(self.seed, self.seed + self.B))
        self.seed += self.B
        self.ctx.render_frames_async(W, H, self.st, seeds, [t.data_ptr() for t in self.lin], None,
                                     self.stream.cuda_stream)

    def timed(self, torch, launches, warmup):
        for _ in range(warmup):
            self.launch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            self.launch()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        frames = launches * self.B
        lit = float((self.lin[0] > 0).float().mean())
        return {"view": self.name, "frames": frames, "ms_per_frame": dt / frames * 1e3,
                "mrays_per_s": W * H * SPP * frames / dt / 1e6, "lit_fraction": round(lit, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=96, help="frames timed per view and repeat")
    ap.add_argument("--warmup", type=int, default=2, help="launches before the timed ones")
    ap.add_argument("--frames-per-launch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch

    import rtgo

    if not torch.cuda.is_available():
        sys.exit("camera_cost.py needs a GPU")
    B = max(1, min(a.frames_per_launch, rtgo.RT_MAX_FRAMES))
    vs = [View(rtgo, torch, n, s, c, B) for n, s, c in views(rtgo)]
    launches = max(1, a.steps // B)
    for rep in range(a.repeats):
        for v in vs:
            r = v.timed(torch, launches, a.warmup if rep == 0 else 1)
            r["repeat"] = rep
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
