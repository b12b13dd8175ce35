#!/usr/bin/env python3
"""What the motion table costs temporal accumulation: the
kernels of rt_temporal_motion_async against rt_temporal_async and
rt_temporal_moments_async of the same build, on the facing headline scene at
800x600 and 1920x1080, 4 spp, depth 50, one device, the look-at camera model,
the previous camera one step of a 120-view orbit (3 degrees) before the current
one (the set-up of scripts/temporal_probe.py).

  t    rt_temporal_async with all inputs (ids, normals, out_rgba)
  mt   rt_temporal_motion_async, the colour-only form, the same inputs and a
       table with one row per object (every object moved by a pixel or so)
  tm   rt_temporal_moments_async (albedo, moments; no out_rgba)
  mtm  rt_temporal_motion_async with moments, the same inputs and table
  *_one_id  the same four with every pixel of both frames made valid (depth 3,
       the normal towards the camera) and one object id everywhere, the set-up
       of scripts/temporal_probe.py's t_all_valid: every lane gathers the same
       table row
  *_bands   the same with the ids in bands of 16 rows over the objects (the
       orbit shifts the image sideways, so the histories survive): every lane
       gathers a row, the rows differ from band to band

Each call is one launch, timed by HIP events recorded on the stream around it.
Per size: two warm-up rounds, then `--rounds` rounds in which the variants
alternate, so that a drift of the clocks falls on all of them alike.  Printed:
one JSON line per size and variant with the median, min and max milliseconds
(the spread of a variant is max - min), and per pair the difference of the
medians.  Both passes move about 90 bytes per pixel; the table adds one cached
24-byte read per valid pixel.

    python scripts/motion_probe.py [--rounds 9] [--out FILE]
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

import numpy as np  # noqa: E402

import rtgo  # noqa: E402

SCENE = os.path.join(ROOT, "scenes", "sphere_reflections_light_facing.json")
SIZES = [(800, 600), (1920, 1080)]
SPP, DEPTH, WARMUP = 4, 50, 2
PAIRS = [("t", "mt"), ("tm", "mtm")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    scene = rtgo.Scene.load_from_file(SCENE)
    nobj = scene.num_objects
    st = rtgo.default_settings()
    st.samples, st.max_depth, st.camera = SPP, DEPTH, rtgo.RT_CAMERA_LOOKAT
    cams = rtgo.camera_orbit(scene, 120)[:2]  # (prev, cur): one step of 3 degrees
    ctx = rtgo.Context(0)
    ctx.set_scene(scene)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(4)
    table = torch.from_numpy((rng.random((nobj, 3)) - 0.5) * 0.02).to("cuda")
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
        mom = [torch.zeros(n * 2, dtype=torch.float32, device="cuda") for _ in range(2)]
        frames = [rtgo.camera_frame(c, "lookat", w, h) for c in cams]
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

        def start_history():  # frame 0's colour, count and moments: what the timed calls reproject
            rtgo.temporal_moments_async(w, h, tframe(0, lin[0]), None, feat[0]["albedo"].data_ptr(), None,
                                        acc[0].data_ptr(), cnt[0].data_ptr(), mom[0].data_ptr(), None, None, stream)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        cur, prev = lambda: tframe(1, lin[1]), lambda: tframe(0, acc[0], cnt[0])
        runs = {
            "t": lambda: rtgo.temporal_async(w, h, cur(), prev(), acc[1].data_ptr(), cnt[1].data_ptr(), rgba.data_ptr(),
                                             None, stream),
            "mt": lambda: rtgo.temporal_motion_async(w, h, cur(), prev(), table.data_ptr(), nobj, acc[1].data_ptr(),
                                                     cnt[1].data_ptr(), rgba.data_ptr(), None, stream),
            "tm": lambda: rtgo.temporal_moments_async(w, h, cur(), prev(), feat[1]["albedo"].data_ptr(),
                                                      mom[0].data_ptr(), acc[1].data_ptr(), cnt[1].data_ptr(),
                                                      mom[1].data_ptr(), None, None, stream),
            "mtm": lambda: rtgo.temporal_motion_async(w, h, cur(), prev(), table.data_ptr(), nobj, acc[1].data_ptr(),
                                                      cnt[1].data_ptr(), None, None, stream,
                                                      d_cur_albedo=feat[1]["albedo"].data_ptr(),
                                                      d_prev_moments=mom[0].data_ptr(), d_out_moments=mom[1].data_ptr()),
        }

        def measure(suffix):
            start_history()
            ms = {k + suffix: [] for k in runs}
            kept = {}
            for r in range(WARMUP + args.rounds):
                for k, fn in runs.items():
                    v = timed(fn)
                    if r >= WARMUP:
                        ms[k + suffix].append(v)
            for k, fn in runs.items():  # (the share that kept a history, from one more call each)
                fn()
                kept[k + suffix] = int((cnt[1] > 1).sum().item())
            return ms, kept

        valid = int(torch.isfinite(feat[1]["depth"]).sum().item())
        ms, kept = measure("")
        # every pixel valid in both frames: a plane 3 units along the view axis; one id, then bands of 16 rows
        bands = ((torch.arange(n, device="cuda") // w) // 16 % nobj).to(torch.int32)
        for suffix, ids in (("_one_id", torch.zeros_like(bands)), ("_bands", bands)):
            for f in range(2):
                feat[f]["depth"].fill_(3.0)
                feat[f]["object"].copy_(ids)
                feat[f]["normal"].view(-1, 3)[:] = torch.tensor([0.0, 0.0, 1.0], device="cuda")
            ms2, kept2 = measure(suffix)
            ms.update(ms2)
            kept.update(kept2)
        med = {}
        for k, v in ms.items():
            med[k] = statistics.median(v)
            lines.append({"size": f"{w}x{h}", "variant": k, "runs": len(v), "ms_median": round(med[k], 4),
                          "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                          "valid_pixels": n if k.endswith(("_one_id", "_bands")) else valid, "pixels_with_history": kept[k]})
        for suffix in ("", "_one_id", "_bands"):
            for a, b in PAIRS:
                lines.append({"size": f"{w}x{h}", "pair": f"{b}{suffix} - {a}{suffix}",
                              "ms_difference_of_medians": round(med[b + suffix] - med[a + suffix], 4)})
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
