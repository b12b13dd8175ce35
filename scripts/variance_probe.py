#!/usr/bin/env python3
"""What variance-guided denoising costs next to the calls it stands beside
(DESIGN.md §4.15): the facing headline scene at one size, 4 spp, depth 50, on
one device, two views one degree apart (rt_camera_orbit).

  t   rt_temporal_async of view 1 over view 0's accumulation
  tm  rt_temporal_moments_async of the same frames (albedo and moments given)
  v   rt_variance_async of tm's result (moments and count given, min_history 1:
      every pixel with a history takes the temporal branch), and vs with
      min_history 1e9 (every valid pixel runs the 7 x 7 window)
  d   rt_denoise_async at its defaults over the accumulation
  dv  rt_denoise_var_async at its defaults over the same, with v's variance,
      and dv_np with prefilter 0

Every variant is timed between HIP events recorded on the stream around the
call.  Two warm-up rounds, then `--rounds` rounds in which the variants
alternate.  With --all-valid every pixel of both views is made valid (depth 1,
normal +Z, one object, the same camera for both views, so that every pixel
finds its history): the scene covers a small part of the frame, and a pixel
that is not valid costs no tap.  One size per process, so that each step of a
job can run under a time limit of its own.

Printed: one JSON line per variant with the median, min and max milliseconds and
the unique bytes per pixel the call must move, counted as §4.13 counts them (the
taps' re-reads are cache traffic):
  t    32 (cur) + 36 (prev) in, 20 out                      = 88
  tm   t + 12 (albedo) + 8 (prev moments) in, + 8 out       = 116
  v    32 in (normal, depth, object, moments, count), 4 out = 36
  d    (44 + 32) + 3 * (32 + 16) + (32 + 24 + 16)           = 292
  dv   (48 + 36) + 3 * (36 + 16) + (36 + 24 + 16)           = 316

    python scripts/variance_probe.py --size 800x600 [--all-valid] [--rounds 5] [--out FILE]
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
SPP, DEPTH, WARMUP = 4, 50, 2
BYTES = {"t": 88, "tm": 116, "v": 36, "vs": 36, "d": 292, "dv": 316, "dv_np": 316}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="800x600")
    ap.add_argument("--all-valid", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    import torch

    scene = rtgo.Scene.load_from_file(SCENE)
    st = rtgo.default_settings()
    st.samples, st.max_depth = SPP, DEPTH
    ctx = rtgo.Context(0)
    ctx.set_scene(scene)
    stream = torch.cuda.current_stream().cuda_stream
    n = w * h
    f32 = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda")
    cams = rtgo.camera_orbit(scene, 2, 1.0)
    lin = [f32(n * 3) for _ in range(2)]
    ctx.render_cameras_async(w, h, st, cams, [t.data_ptr() for t in lin], None, seeds=[st.seed, st.seed + 1],
                             stream=stream)
    feat = [{k: torch.zeros(n * (3 if k in ("albedo", "normal") else 1),
                            dtype=torch.int32 if k == "object" else torch.float32, device="cuda")
             for k in ("albedo", "normal", "depth", "object")} for _ in range(2)]
    for i in range(2):
        ft = feat[i]
        ctx.render_aov_async(w, h, st, rtgo.AovBuffers(ft["albedo"].data_ptr(), ft["normal"].data_ptr(),
                                                       ft["depth"].data_ptr(), None, ft["object"].data_ptr()),
                             camera=cams[i], stream=stream)
    torch.cuda.synchronize()
    frames = [rtgo.camera_frame(cams[i], int(st.camera), w, h) for i in range(2)]
    if args.all_valid:
        for ft in feat:
            ft["depth"].fill_(1.0)
            ft["normal"].view(-1, 3)[:, 2] = 1.0
            ft["object"].fill_(0)
        frames[0] = frames[1]
    acc, cnt, mom = [f32(n * 3) for _ in range(2)], [f32(n) for _ in range(2)], [f32(n * 2) for _ in range(2)]
    var, out_lin = f32(n), f32(n * 3)
    rgba = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    nb_d, nb_dv = rtgo.denoise_workspace_bytes(w, h), rtgo.denoise_var_workspace_bytes(w, h)
    work = torch.zeros(max(nb_d, nb_dv), dtype=torch.uint8, device="cuda")

    def frame(i, color, count=None):
        ft = feat[i]
        return rtgo.temporal_frame(frames[i], color.data_ptr(), ft["depth"].data_ptr(), ft["object"].data_ptr(),
                                   ft["normal"].data_ptr(), count.data_ptr() if count is not None else None)

    # view 0 starts the history (not timed); view 1 over it is what is timed
    rtgo.temporal_moments_async(w, h, frame(0, lin[0]), None, feat[0]["albedo"].data_ptr(), None, acc[0].data_ptr(),
                                cnt[0].data_ptr(), mom[0].data_ptr(), None, None, stream)
    cur, prev = frame(1, lin[1]), frame(0, acc[0], cnt[0])
    ft = feat[1]
    guides = (ft["normal"].data_ptr(), ft["depth"].data_ptr())

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    vp = {"v": rtgo.default_variance(min_history=1), "vs": rtgo.default_variance(min_history=1e9)}
    dvp = {"dv": rtgo.default_denoise_var(), "dv_np": rtgo.default_denoise_var(prefilter=0)}
    variants = {
        "t": lambda: rtgo.temporal_async(w, h, cur, prev, acc[1].data_ptr(), cnt[1].data_ptr(), rgba.data_ptr(), None,
                                         stream),
        "tm": lambda: rtgo.temporal_moments_async(w, h, cur, prev, ft["albedo"].data_ptr(), mom[0].data_ptr(),
                                                  acc[1].data_ptr(), cnt[1].data_ptr(), mom[1].data_ptr(),
                                                  rgba.data_ptr(), None, stream),
        **{k: (lambda k=k: rtgo.variance_async(w, h, acc[1].data_ptr(), *guides, ft["albedo"].data_ptr(),
                                               ft["object"].data_ptr(), mom[1].data_ptr(), cnt[1].data_ptr(),
                                               var.data_ptr(), vp[k], stream)) for k in vp},
        "d": lambda: rtgo.denoise_async(w, h, acc[1].data_ptr(), *guides, ft["albedo"].data_ptr(),
                                        ft["object"].data_ptr(), out_lin.data_ptr(), rgba.data_ptr(), work.data_ptr(),
                                        nb_d, None, stream),
        **{k: (lambda k=k: rtgo.denoise_var_async(w, h, acc[1].data_ptr(), *guides, var.data_ptr(),
                                                  ft["albedo"].data_ptr(), ft["object"].data_ptr(), out_lin.data_ptr(),
                                                  rgba.data_ptr(), None, work.data_ptr(), nb_dv, dvp[k], stream))
           for k in dvp},
    }
    order = ["t", "tm", "vs", "v", "d", "dv", "dv_np"]  # (v last of its pair: dv reads the temporal variance)
    ms = {k: [] for k in order}
    for r in range(WARMUP + args.rounds):
        for k in order:
            t = timed(variants[k])
            if r >= WARMUP:
                ms[k].append(t)
    valid = int(torch.isfinite(ft["depth"]).sum().item())
    history = int((cnt[1] > 1).sum().item())
    lines = []
    for k in order:
        med = statistics.median(ms[k])
        lines.append({"size": f"{w}x{h}", "all_valid": bool(args.all_valid), "variant": k, "runs": len(ms[k]),
                      "ms_median": round(med, 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4),
                      "valid_pixels": valid, "pixels_with_history": history, "bytes_per_pixel": BYTES[k],
                      "gb_per_s_median": round(BYTES[k] * n / (med * 1e-3) / 1e9, 1)})
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
