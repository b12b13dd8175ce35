#!/usr/bin/env python3
"""What history rectification costs temporal accumulation, and which of its two
kernel forms is faster: rt_temporal_clip_async against
rt_temporal_motion_async of the same build on the same buffers, on the facing
headline scene at 800x600 and 1920x1080, 4 spp, depth 50, one device, the
look-at camera model, the previous camera one step of a 120-view orbit before
the current one (the set-up of scripts/motion_probe.py).

  mt / mtm          rt_temporal_motion_async, colour-only / with moments: the
                    parent's pass, the yardstick
  plain_rR[_m]      rt_temporal_clip_async, the plain form (RTGO_CLIP_FORM),
                    radius R in 1..4, the default gamma and min_taps, the
                    frame's albedo; _m: with moments
  staged_rR[_m]     the same call, the staged form
  *_cover           the same with every pixel of both frames made valid (depth
                    3, the normal towards the camera) and the ids in bands of
                    16 rows: every pixel has a history and a full window.  This
                    is the A/B that decides the form.

Each call is one launch, timed by HIP events recorded on the stream around it.
Per size: two warm-up rounds, then `--rounds` rounds in which ALL variants
alternate, so that a drift of the clocks falls on all of them alike.  Printed:
one JSON line per size and variant with the median, min and max milliseconds
(the spread of a variant is max - min), and per radius the A/B staged - plain
with twice the larger spread of the two beside it.  Before timing, the two
forms' outputs are compared bit for bit.

    python scripts/clip_probe.py [--rounds 9] [--out FILE]
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
RADII = (1, 2, 3, 4)


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
        clp = torch.zeros(n, dtype=torch.float32, device="cuda")
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

        def motion(moments):
            if moments:
                rtgo.temporal_motion_async(w, h, cur(), prev(), table.data_ptr(), nobj, acc[1].data_ptr(),
                                           cnt[1].data_ptr(), None, None, stream,
                                           d_cur_albedo=feat[1]["albedo"].data_ptr(), d_prev_moments=mom[0].data_ptr(),
                                           d_out_moments=mom[1].data_ptr())
            else:
                rtgo.temporal_motion_async(w, h, cur(), prev(), table.data_ptr(), nobj, acc[1].data_ptr(),
                                           cnt[1].data_ptr(), rgba.data_ptr(), None, stream)

        def clip(form, radius, moments):
            os.environ["RTGO_CLIP_FORM"] = form  # (read by the library at every launch)
            rtgo.temporal_clip_async(w, h, cur(), prev(), acc[1].data_ptr(), cnt[1].data_ptr(),
                                     None if moments else rgba.data_ptr(), None, stream,
                                     clip=rtgo.default_history_clip(radius=radius), d_motion=table.data_ptr(),
                                     num_objects=nobj, d_cur_albedo=feat[1]["albedo"].data_ptr(),
                                     d_prev_moments=mom[0].data_ptr() if moments else None,
                                     d_out_moments=mom[1].data_ptr() if moments else None,
                                     d_out_clipped=clp.data_ptr())

        runs = {"mt": lambda: motion(False), "mtm": lambda: motion(True)}
        for r in RADII:
            for form in ("plain", "staged"):
                runs[f"{form}_r{r}"] = lambda form=form, r=r: clip(form, r, False)
                runs[f"{form}_r{r}_m"] = lambda form=form, r=r: clip(form, r, True)

        def measure(suffix):
            start_history()
            for r in RADII:  # the two forms give the same bits
                for m in ("", "_m"):
                    outs = []
                    for form in ("plain", "staged"):
                        runs[f"{form}_r{r}{m}"]()
                        outs.append([t.clone() for t in (acc[1], cnt[1], mom[1], clp)])
                    for a, b in zip(*outs):
                        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (w, h, r, m, suffix)
            ms = {k + suffix: [] for k in runs}
            extra = {}
            for rnd in range(WARMUP + args.rounds):
                for k, fn in runs.items():
                    v = timed(fn)
                    if rnd >= WARMUP:
                        ms[k + suffix].append(v)
            for k, fn in runs.items():  # (what one more call each kept and clipped)
                clp.zero_()
                fn()
                extra[k + suffix] = (int((cnt[1] > 1).sum().item()), int(clp.sum().item()))
            return ms, extra

        valid = int(torch.isfinite(feat[1]["depth"]).sum().item())
        ms, extra = measure("")
        # every pixel valid in both frames: a plane 3 units along the view axis, ids in bands of 16 rows
        bands = ((torch.arange(n, device="cuda") // w) // 16 % nobj).to(torch.int32)
        for f in range(2):
            feat[f]["depth"].fill_(3.0)
            feat[f]["object"].copy_(bands)
            feat[f]["normal"].view(-1, 3)[:] = torch.tensor([0.0, 0.0, 1.0], device="cuda")
        ms2, extra2 = measure("_cover")
        ms.update(ms2)
        extra.update(extra2)
        med, spread = {}, {}
        for k, v in ms.items():
            med[k], spread[k] = statistics.median(v), max(v) - min(v)
            lines.append({"size": f"{w}x{h}", "variant": k, "runs": len(v), "ms_median": round(med[k], 4),
                          "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                          "valid_pixels": n if k.endswith("_cover") else valid, "pixels_with_history": extra[k][0],
                          "pixels_clipped": extra[k][1]})
        for suffix in ("", "_cover"):
            for r in RADII:
                for m in ("", "_m"):
                    a, b = f"plain_r{r}{m}{suffix}", f"staged_r{r}{m}{suffix}"
                    lines.append({"size": f"{w}x{h}", "ab": f"{b} - {a}", "ms_difference_of_medians": round(med[b] - med[a], 4),
                                  "twice_the_larger_spread": round(2 * max(spread[a], spread[b]), 4),
                                  "parent_pass_ms": round(med[("mtm" if m else "mt") + suffix], 4)})
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
