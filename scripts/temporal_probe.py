#!/usr/bin/env python3
"""What temporal accumulation costs next to the frame it accumulates (DESIGN.md
§4.14): the facing headline scene at 800x600 and 1920x1080, depth 50, on one
device, the look-at camera model, the previous camera one step of a 120-view
orbit (3 degrees) before the current one.

  a  a one-frame 4-spp render (rt_context_render_async), its device time from
     rt_context_last_kernel_seconds: the HIP events the library itself records
     on the stream around the render's launch (as scripts/denoise_probe.py
     times it), so the row holds the render and not the call's host work
  c  rt_denoise_async with the defaults and all five inputs: HIP events
     recorded on the stream around the call
  t  rt_temporal_async with all inputs (ids, normals, out_rgba), the previous
     frame's colour and count being a first call's outputs: HIP events around
     the call (one launch)
  t_all_valid, c_all_valid  the same two calls with every pixel of both frames
     made valid (depth 3, one object, the normal towards the camera): the scene
     covers a small part of the frame, and a pixel that is not valid costs
     neither a tap nor a reprojection

Per size: two warm-up rounds, then `--rounds` rounds in which the variants
alternate.  Printed: one JSON line per size and variant with the median, min
and max milliseconds; for t also the unique bytes the call must move -- per
pixel 32 read of the current frame (colour 12, depth 4, object 4, normal 12),
36 of the previous one (the same and count 4) and 20 written (colour 12, count
4, RGBA 4): 88 -- the four taps' re-reads being cache traffic, the bytes per
second that implies, and the share of pixels that kept a history.

    python scripts/temporal_probe.py [--rounds 5] [--out FILE]
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
SIZES = [(800, 600), (1920, 1080)]
SPP, DEPTH, WARMUP = 4, 50, 2
TEMPORAL_BYTES_PER_PIXEL = 32 + 36 + 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    scene = rtgo.Scene.load_from_file(SCENE)
    st = rtgo.default_settings()
    st.samples, st.max_depth, st.camera = SPP, DEPTH, rtgo.RT_CAMERA_LOOKAT
    cams = rtgo.camera_orbit(scene, 120)[:2]  # (prev, cur): one step of 3 degrees
    ctx = rtgo.Context(0)
    ctx.set_scene(scene)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []
    for w, h in SIZES:
        n = w * h
        lin = [torch.zeros(n * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
        rgba = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
        feat = [{k: torch.zeros(n * (3 if k in ("albedo", "normal") else 1),
                                dtype=torch.int32 if k == "object" else torch.float32, device="cuda")
                 for k in ("albedo", "normal", "depth", "object")} for _ in range(2)]
        acc = [torch.zeros(n * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
        cnt = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(2)]
        nbytes = rtgo.denoise_workspace_bytes(w, h)
        work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        out_lin = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        out_rgba = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
        frames = [rtgo.camera_frame(c, "lookat", w, h) for c in cams]
        # both frames' renders and features; frame 0 starts the history that frame 1's timed call reprojects
        ctx.render_cameras_async(w, h, st, cams, [t.data_ptr() for t in lin], None, seeds=[1, 2], stream=stream)
        for f in range(2):
            st_f = rtgo.Settings.from_buffer_copy(st)
            st_f.seed = 1 + f
            ctx.render_aov_async(w, h, st_f, rtgo.AovBuffers(feat[f]["albedo"].data_ptr(), feat[f]["normal"].data_ptr(),
                                                            feat[f]["depth"].data_ptr(), None,
                                                            feat[f]["object"].data_ptr()), camera=cams[f], stream=stream)

        def tframe(f, color, count=None):
            return rtgo.temporal_frame(frames[f], color.data_ptr(), feat[f]["depth"].data_ptr(),
                                       feat[f]["object"].data_ptr(), feat[f]["normal"].data_ptr(),
                                       count.data_ptr() if count is not None else None)

        def start_history():
            rtgo.temporal_async(w, h, tframe(0, lin[0]), None, acc[0].data_ptr(), cnt[0].data_ptr(), None, None, stream)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def run_a():
            ctx.render_async(w, h, st, out_lin.data_ptr(), rgba.data_ptr(), stream)
            return 1e3 * ctx.last_kernel_seconds()

        def run_c():
            return timed(lambda: rtgo.denoise_async(
                w, h, lin[1].data_ptr(), feat[1]["normal"].data_ptr(), feat[1]["depth"].data_ptr(),
                feat[1]["albedo"].data_ptr(), feat[1]["object"].data_ptr(), out_lin.data_ptr(), out_rgba.data_ptr(),
                work.data_ptr(), nbytes, None, stream))

        def run_t():
            return timed(lambda: rtgo.temporal_async(w, h, tframe(1, lin[1]), tframe(0, acc[0], cnt[0]),
                                                     acc[1].data_ptr(), cnt[1].data_ptr(), rgba.data_ptr(), None, stream))

        start_history()
        ms = {"a": [], "c": [], "t": []}
        for r in range(WARMUP + args.rounds):
            row = {"a": run_a(), "c": run_c(), "t": run_t()}
            if r >= WARMUP:
                for k, v in row.items():
                    ms[k].append(v)
        valid = int(torch.isfinite(feat[1]["depth"]).sum().item())
        kept = {"t": int((cnt[1] > 1).sum().item())}
        # every pixel valid in both frames: a plane 3 units along the view axis, one object, one normal
        for f in range(2):
            feat[f]["depth"].fill_(3.0)
            feat[f]["object"].fill_(0)
            feat[f]["normal"].view(-1, 3)[:] = torch.tensor([0.0, 0.0, 1.0], device="cuda")
        start_history()
        ms["c_all_valid"], ms["t_all_valid"] = [], []
        for r in range(WARMUP + args.rounds):
            row = {"c_all_valid": run_c(), "t_all_valid": run_t()}
            if r >= WARMUP:
                for k, v in row.items():
                    ms[k].append(v)
        kept["t_all_valid"] = int((cnt[1] > 1).sum().item())
        for k, v in ms.items():
            med = statistics.median(v)
            line = {"size": f"{w}x{h}", "variant": k, "runs": len(v), "ms_median": round(med, 4),
                    "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
            if k != "a":
                line["valid_pixels"] = n if k.endswith("all_valid") else valid
            if k.startswith("t"):
                moved = TEMPORAL_BYTES_PER_PIXEL * n
                line.update({"pixels_with_history": kept[k], "bytes_moved": moved,
                             "gb_per_s_median": round(moved / (med * 1e-3) / 1e9, 1)})
            lines.append(line)
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
