#!/usr/bin/env python3
"""What the specular-through guide buys and costs, on one device.

Quality (--quality): S_CUBE of tests/sequence_cases.py at 144x96, depth 50, the
set-up of §4.13 to §4.15 rendered on the GPU.  Truth is the 512-spp render with
seed 77.  Per seed (--seeds, default 3 4 5), RMSE of the linear image over the
whole image and over the pixels whose first hit (the 1-spp first-hit pass of the
same seed) is object 3 (the roughness-0 metal cube), 0 (the roughness-0.2 metal
sphere) and 1 (the Lambertian sphere):
  noisy      the 1-spp render
  denoise    rt_denoise_async at its defaults, guide "first" and "specular"
  variance   the single frame through rt_variance_async (spatial estimate) and
             rt_denoise_var_async, both guides
  temporal   six 1-spp frames, the camera moving 0.05 in x per frame, seeds
             seed .. seed + 5, accumulated (rt_temporal_async); the last frame
             accumulated, then through rt_denoise_async and through the variance
             chain (moments), both guides; truth is the 512-spp render from the
             last camera
The specular pass runs at rt_aov_spec_default (4 bounces, max_roughness 0.1).

Cost (--cost): the specular-through pass next to the first-hit pass, device time
from rt_context_last_kernel_seconds, at 800x600x4 and 1920x1080x1 on the facing
headline scene and on S_MIRROR of tests/spec_cases.py (mirrors that show
mirrors): two warm-up rounds, then ten rounds in which the two alternate;
median, min and max milliseconds, and the mean reflections followed per pixel.

One JSON line per figure.

    python scripts/specular_guide_probe.py [--quality] [--cost] [--seeds 3 4 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "concurrent-raytracer-go_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import rtgo  # noqa: E402
from sequence_cases import S_CUBE  # noqa: E402
from spec_cases import S_MIRROR  # noqa: E402

W, H, DEPTH, TRUTH_SPP, TRUTH_SEED, FRAMES, STEP = 144, 96, 50, 512, 77, 6, 0.05
REGIONS = {"whole": None, "metal_cube": 3, "metal_sphere": 0, "lambertian_sphere": 1}
HEADLINE = os.path.join(ROOT, "scenes", "sphere_reflections_light_facing.json")
COST_SIZES = [(800, 600, 4), (1920, 1080, 1)]
WARMUP, ROUNDS = 2, 10


def rmse(img, truth, mask):
    d = (img.astype(np.float64) - truth.astype(np.float64)) ** 2
    d = d if mask is None else d[mask]
    return float(np.sqrt(d.mean()))


def renderer(samples, seed):
    r = rtgo.ParallelRenderer(1)
    r.set_samples(samples)
    r.set_seed(seed)
    r.settings.max_depth = DEPTH
    return r


def quality(seeds):
    scene = rtgo.Scene.from_json_text(json.dumps(S_CUBE))
    cam0 = dict(S_CUBE["camera"])
    cams = [dict(cam0, position=[cam0["position"][0] + STEP * f] + list(cam0["position"][1:])) for f in range(FRAMES)]
    t = renderer(TRUTH_SPP, TRUTH_SEED)
    t.render(scene, W, H)
    truth = t.last_linear.copy()
    t.render_sequence(scene, W, H, [cams[-1]])
    truth_last = t.last_linear[0].copy()
    t.close()
    lines = []

    def add(seed, stage, guide, img, tr, obj):
        for name, idx in REGIONS.items():
            mask = None if idx is None else obj == idx
            lines.append({"probe": "quality", "seed": seed, "stage": stage, "guide": guide, "region": name,
                          "pixels": int(W * H if mask is None else mask.sum()), "rmse": rmse(img, tr, mask)})

    for seed in seeds:
        r = renderer(1, seed)
        obj = r.render_aov(scene, W, H)["object"]
        r.render(scene, W, H)
        add(seed, "noisy", "-", r.last_linear, truth, obj)
        for guide in ("first", "specular"):
            r.render_denoised(scene, W, H, guide=guide)
            add(seed, "denoise", guide, r.last_denoised_linear, truth, obj)
            r.render_denoised(scene, W, H, variance=True, guide=guide)
            add(seed, "variance", guide, r.last_denoised_linear, truth, obj)
        # the six-frame chain; regions by the last frame's own first hits (its seed and camera)
        r.set_seed(seed + FRAMES - 1)
        obj_last = r.render_aov(scene, W, H, camera=cams[-1])["object"]
        r.set_seed(seed)
        r.render_sequence(scene, W, H, cams, temporal=True)
        add(seed, "temporal noisy", "-", r.last_linear[-1], truth_last, obj_last)
        add(seed, "temporal accumulated", "-", r.last_temporal_linear[-1], truth_last, obj_last)
        for guide in ("first", "specular"):
            r.render_sequence(scene, W, H, cams, temporal=True, denoise=True, guide=guide)
            add(seed, "temporal denoise", guide, r.last_denoised_linear[-1], truth_last, obj_last)
            r.render_sequence(scene, W, H, cams, temporal=True, variance=True, guide=guide)
            add(seed, "temporal variance", guide, r.last_denoised_linear[-1], truth_last, obj_last)
        r.close()
    return lines


def cost():
    import torch

    lines = []
    st = rtgo.default_settings()
    st.max_depth = DEPTH
    spec = rtgo.default_aov_spec()
    stream = torch.cuda.current_stream().cuda_stream
    scenes = {"headline": rtgo.Scene.load_from_file(HEADLINE), "S_MIRROR": rtgo.Scene.from_json_text(json.dumps(S_MIRROR))}
    for sname, scene in scenes.items():
        ctx = rtgo.Context(0)
        ctx.set_scene(scene)
        for w, h, spp in COST_SIZES:
            st.samples = spp
            n = w * h
            f = {k: torch.zeros(n * (3 if k in ("albedo", "normal") else 1),
                                dtype=torch.int32 if k == "object" else torch.float32, device="cuda")
                 for k in rtgo.AOV_SPEC_NAMES}
            first = rtgo.AovBuffers(*[f[k].data_ptr() for k in rtgo.AOV_NAMES])
            both = rtgo.AovSpecBuffers(*[f[k].data_ptr() for k in rtgo.AOV_SPEC_NAMES])

            def run_first():
                ctx.render_aov_async(w, h, st, first, stream=stream)
                return 1e3 * ctx.last_kernel_seconds()

            def run_spec():
                ctx.render_aov_spec_async(w, h, st, both, spec=spec, stream=stream)
                return 1e3 * ctx.last_kernel_seconds()

            ms = {"first_hit": [], "specular_through": []}
            for rnd in range(WARMUP + ROUNDS):
                row = {"first_hit": run_first(), "specular_through": run_spec()}
                if rnd >= WARMUP:
                    for k, v in row.items():
                        ms[k].append(v)
            torch.cuda.synchronize()
            extra = {"mean_bounces": float(f["bounces"].mean().item()),
                     "specular_pixels": int((f["specular"] > 0).sum().item()),
                     "hit_pixels": int((f["coverage"] > 0).sum().item())}
            for k, v in ms.items():
                lines.append(dict({"probe": "cost", "scene": sname, "size": f"{w}x{h}x{spp}", "variant": k, "runs": len(v),
                                   "ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                                   "ms_max": round(max(v), 4)}, **extra))
        ctx.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--seeds", type=int, nargs="+", default=[3, 4, 5])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    both = not args.quality and not args.cost
    lines = []
    if args.cost or both:
        lines += cost()
    if args.quality or both:
        lines += quality(args.seeds)
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
