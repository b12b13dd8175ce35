#!/usr/bin/env python3
"""What adaptive sampling buys: an adaptive progression
against the plain progression of the same passes, on the headline scene
(800x600, cap 100, passes of 10, tolerance 1, patience 2, min_samples 20) and
on one BVH config (C4's 10k-sphere scene at 960x540, cap 64, passes of 8).

Per case and mode it prints one JSON line: the sum of the per-pixel sample
counts, the mean samples per pixel, the summed rt_context_last_kernel_seconds
of the adds (for an adaptive add that is its render launches and the update
kernel), the host seconds around the adds, the schedules built, and the
share of the host time spent in the adds that built one.  A last line per
case gives the cost of an adaptive add in which every pixel is still active
against a plain add of the same size (the first add of each progression,
median over the repetitions).

    python scripts/adaptive_probe.py [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "concurrent-raytracer-go_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rtgo  # noqa: E402

CASES = [
    # name, scene, W, H, cap, pass, (tolerance, patience, min_samples), tuning
    ("headline_block", "sphere_reflections_light_facing.json", 800, 600, 100, 10, (1, 2, 20), {"stream": 0}),
    ("headline_stream", "sphere_reflections_light_facing.json", 800, 600, 100, 10, (1, 2, 20), {"stream": 1}),
    ("c4_960x540", "gen:10000", 960, 540, 64, 8, (1, 2, 16), {}),
]


def load_scene(spec):
    if spec.startswith("gen:"):
        from scene_cases import spheres10k_scene

        return spheres10k_scene(rtgo, int(spec[4:]))
    return rtgo.Scene.load_from_file(os.path.join(ROOT, "scenes", spec))


def progression(ctx, w, h, cap, pas, adaptive):
    import torch

    st = rtgo.default_settings()
    st.samples = cap
    rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    ctx.progressive_begin(w, h, st)
    if adaptive is not None:
        ctx.progressive_set_adaptive(*adaptive)
    built0 = ctx.stats()["schedules_built"]
    adds, done = [], 0
    while done < cap:
        n = min(pas, cap - done)
        b0 = ctx.stats()["schedules_built"]
        t0 = time.perf_counter()
        ctx.progressive_add(n, 0, rgba.data_ptr(), 0)
        torch.cuda.synchronize()
        host = time.perf_counter() - t0
        done += n
        state = ctx.progressive_state()
        adds.append({"kernel_s": ctx.last_kernel_seconds(), "host_s": host, "active": state["active"],
                     "built": ctx.stats()["schedules_built"] - b0})
        if adaptive is not None and state["active"] == 0:
            break
    state = ctx.progressive_state()
    ctx.progressive_end()
    host = sum(a["host_s"] for a in adds)
    return {
        "adds": len(adds),
        "sum_count": state["samples"],
        "mean_spp": state["samples"] / max(1, state["pixels"]),
        "kernel_ms": 1e3 * sum(a["kernel_s"] for a in adds),
        "host_ms": 1e3 * host,
        "schedules_built": ctx.stats()["schedules_built"] - built0,
        "rebuild_share_of_host": sum(a["host_s"] for a in adds if a["built"]) / host if host > 0 else 0.0,
        "first_add_kernel_ms": 1e3 * adds[0]["kernel_s"],
        "active_after_each_add": [a["active"] for a in adds],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    for name, spec, w, h, cap, pas, rule, tun in CASES:
        ctx = rtgo.Context(0)
        ctx.set_tuning(rtgo.default_tuning(**tun))
        ctx.set_scene(load_scene(spec))
        progression(ctx, w, h, cap, pas, None)  # warm: code objects, buffers
        runs = {"plain": [], "adaptive": []}
        for _ in range(args.reps):
            for mode, ad in (("plain", None), ("adaptive", rule)):
                runs[mode].append(progression(ctx, w, h, cap, pas, ad))
        for mode in ("plain", "adaptive"):
            r = sorted(runs[mode], key=lambda x: x["kernel_ms"])[len(runs[mode]) // 2]  # the median run
            lines.append({"case": name, "mode": mode, "size": f"{w}x{h}", "cap": cap, "pass": pas,
                          "rule": list(rule) if mode == "adaptive" else None, **r})
        lines.append({"case": name, "first_add_kernel_ms": {
            m: statistics.median(x["first_add_kernel_ms"] for x in runs[m]) for m in runs}})
        ctx.close()
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
