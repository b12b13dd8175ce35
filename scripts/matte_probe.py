#!/usr/bin/env python3
"""What the matte pass and the edge resolve cost, on the
facing headline scene, depth 50, one device, the look-at camera model.

At 800x600, beside each other:
  render_1spp     rt_context_render_async, 1 sample per pixel
  aov_1 / aov_16  rt_context_render_aov_async, 1 and 16 samples (the first-hit
                  pass: the same rays and hits as the matte pass, sums instead
                  of slots)
  matte_4 / _8 / _16   rt_context_render_matte_async, object level, 4 ranks
  matte_16_face   the same at the face level
At 1920x1080, on a 1-spp render with its first-hit features and a 16-sample
matte:
  denoise         rt_denoise_async with the defaults
  resolve_r1..r4  rt_matte_resolve_async at radius 1..4 (both outputs)

Each variant is timed by HIP events recorded on the stream around `--reps`
calls in a row (the image passes are far below a millisecond: one call would
measure the clock); the figure is the window over reps.  Two warm-up rounds,
then `--rounds` rounds in which ALL variants alternate, so that a drift of the
clocks falls on all of them alike.  Printed: one JSON line per variant with the
median, min and max milliseconds per call, and the mixed pixels of the frame.

    python scripts/matte_probe.py [--rounds 9] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "concurrent-raytracer-go_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import rtgo  # noqa: E402

SCENE = os.path.join(ROOT, "scenes", "sphere_reflections_light_facing.json")
DEPTH, WARMUP, RANKS = 50, 2, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    scene = rtgo.Scene.load_from_file(SCENE)
    ctx = rtgo.Context(0)
    ctx.set_scene(scene)
    stream = torch.cuda.current_stream().cuda_stream

    def settings(samples):
        st = rtgo.default_settings()
        st.samples, st.max_depth, st.camera, st.seed = samples, DEPTH, rtgo.RT_CAMERA_LOOKAT, 1
        return st

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def measure(runs):
        ms = {k: [] for k in runs}
        for rnd in range(WARMUP + args.rounds):
            for k, fn in runs.items():
                v = timed(fn)
                if rnd >= WARMUP:
                    ms[k].append(v)
        return ms

    def buffers(w, h):
        n = w * h
        b = {"lin": torch.zeros(n * 3, dtype=torch.float32, device="cuda"),
             "rgba": torch.zeros(n * 4, dtype=torch.uint8, device="cuda"),
             "out": torch.zeros(n * 3, dtype=torch.float32, device="cuda"),
             "id": torch.zeros(RANKS * n, dtype=torch.int32, device="cuda"),
             "count": torch.zeros(RANKS * n, dtype=torch.int32, device="cuda"),
             "rest": torch.zeros(n, dtype=torch.int32, device="cuda")}
        for k in ("albedo", "normal", "depth", "object"):
            b[k] = torch.zeros(n * (3 if k in ("albedo", "normal") else 1),
                               dtype=torch.int32 if k == "object" else torch.float32, device="cuda")
        return b

    def aov(w, h, b, samples):
        ctx.render_aov_async(w, h, settings(samples), rtgo.AovBuffers(b["albedo"].data_ptr(), b["normal"].data_ptr(),
                                                                      b["depth"].data_ptr(), None, b["object"].data_ptr()),
                             stream=stream)

    def matte(w, h, b, samples, level="object"):
        ctx.render_matte_async(w, h, settings(samples),
                               rtgo.MatteBuffers(b["id"].data_ptr(), b["count"].data_ptr(), b["rest"].data_ptr()),
                               params=rtgo.default_matte(ranks=RANKS, level=level), stream=stream)

    def mixed_pixels(b, samples):
        cnt = b["count"].view(RANKS, -1)
        parts = (cnt > 0).sum(dim=0) + ((samples - cnt.sum(dim=0) - b["rest"]) > 0) + (b["rest"] > 0)
        return int((parts >= 2).sum().item())

    lines = []

    def report(size, ms, extra):
        for k, v in ms.items():
            lines.append(dict({"size": size, "variant": k, "runs": len(v), "reps": args.reps,
                               "ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                               "ms_max": round(max(v), 4)}, **extra.get(k, {})))

    # ---- 800x600: the matte pass beside the first-hit pass and a 1-spp render
    w, h = 800, 600
    b = buffers(w, h)
    runs = {"render_1spp": lambda: ctx.render_async(w, h, settings(1), b["lin"].data_ptr(), b["rgba"].data_ptr(), stream),
            "aov_1": lambda: aov(w, h, b, 1), "aov_16": lambda: aov(w, h, b, 16),
            "matte_4": lambda: matte(w, h, b, 4), "matte_8": lambda: matte(w, h, b, 8),
            "matte_16": lambda: matte(w, h, b, 16), "matte_16_face": lambda: matte(w, h, b, 16, "face")}
    extra = {}
    for s in (4, 8, 16):
        matte(w, h, b, s)
        torch.cuda.synchronize()
        extra[f"matte_{s}"] = {"mixed_pixels": mixed_pixels(b, s), "pixels": w * h}
    report(f"{w}x{h}", measure(runs), extra)

    # ---- 1920x1080: the resolve beside the denoiser
    w, h = 1920, 1080
    b = buffers(w, h)
    nbytes = rtgo.denoise_workspace_bytes(w, h)
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ctx.render_async(w, h, settings(1), b["lin"].data_ptr(), b["rgba"].data_ptr(), stream)
    aov(w, h, b, 1)
    matte(w, h, b, 16)
    torch.cuda.synchronize()
    mixed = mixed_pixels(b, 16)

    def resolve(radius):
        rtgo.matte_resolve_async(w, h, b["lin"].data_ptr(), b["object"].data_ptr(), b["id"].data_ptr(),
                                 b["count"].data_ptr(), b["rest"].data_ptr(), RANKS, 16, b["out"].data_ptr(),
                                 b["rgba"].data_ptr(), rtgo.default_matte_resolve(radius=radius), stream)

    runs = {"denoise": lambda: rtgo.denoise_async(w, h, b["lin"].data_ptr(), b["normal"].data_ptr(), b["depth"].data_ptr(),
                                                  b["albedo"].data_ptr(), b["object"].data_ptr(), b["out"].data_ptr(),
                                                  b["rgba"].data_ptr(), work.data_ptr(), nbytes, None, stream)}
    for r in (1, 2, 3, 4):
        runs[f"resolve_r{r}"] = lambda r=r: resolve(r)
    report(f"{w}x{h}", measure(runs), {f"resolve_r{r}": {"mixed_pixels": mixed, "pixels": w * h} for r in (1, 2, 3, 4)})

    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
