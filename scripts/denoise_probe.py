#!/usr/bin/env python3
"""What the denoiser costs next to the frame it cleans: the
facing headline scene at 800x600 and 1920x1080, depth 50, on one device.

  a  a one-frame 4-spp render (rt_context_render_async), its device time from
     rt_context_last_kernel_seconds
  b  the first-hit feature pass at 4 spp (rt_context_render_aov_async), the same
  c  rt_denoise_async with the defaults and all five inputs (levels 4), and
     again with levels 2 and 6: HIP events recorded on the stream around the
     call (its prepare kernel and its level kernels); c4_all_valid is the
     default call once more with every pixel made valid (the scene covers a
     small part of the frame, and a pixel that is not valid costs no tap)

Per size: two warm-up rounds, then `--rounds` rounds in which the variants
alternate.  Printed: one JSON line per size and variant with the median, min
and max milliseconds; for c also the bytes the call must move -- per pixel the
unique reads and writes of its records and buffers (prepare: 44 in, 32 out; a
level: 32 in, 16 out; the last level: 32 + 24 in, 16 out), the taps' re-reads
being cache traffic -- and the bytes per second that implies.  The records of a
frame (48 B per pixel) stay in the L2 and the Infinity Cache at these sizes, so
the figure is no share of the HBM peak.

    python scripts/denoise_probe.py [--rounds 5] [--out FILE]
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
LEVELS = [4, 2, 6]


def denoise_bytes_per_pixel(levels):
    return (44 + 32) + (levels - 1) * (32 + 16) + (32 + 24 + 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    scene = rtgo.Scene.load_from_file(SCENE)
    st = rtgo.default_settings()
    st.samples, st.max_depth = SPP, DEPTH
    ctx = rtgo.Context(0)
    ctx.set_scene(scene)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []
    for w, h in SIZES:
        n = w * h
        lin = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        rgba = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
        f = {k: torch.zeros(n * (3 if k in ("albedo", "normal") else 1),
                            dtype=torch.int32 if k == "object" else torch.float32, device="cuda")
             for k in ("albedo", "normal", "depth", "object")}
        aov = rtgo.AovBuffers(f["albedo"].data_ptr(), f["normal"].data_ptr(), f["depth"].data_ptr(), None,
                              f["object"].data_ptr())
        nbytes = rtgo.denoise_workspace_bytes(w, h)
        work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        out_lin = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        out_rgba = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
        params = {lv: rtgo.default_denoise(levels=lv) for lv in LEVELS}

        def run_a():
            ctx.render_async(w, h, st, lin.data_ptr(), rgba.data_ptr(), stream)
            return 1e3 * ctx.last_kernel_seconds()

        def run_b():
            ctx.render_aov_async(w, h, st, aov, stream=stream)
            return 1e3 * ctx.last_kernel_seconds()

        def run_c(lv):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rtgo.denoise_async(w, h, lin.data_ptr(), f["normal"].data_ptr(), f["depth"].data_ptr(),
                               f["albedo"].data_ptr(), f["object"].data_ptr(), out_lin.data_ptr(), out_rgba.data_ptr(),
                               work.data_ptr(), nbytes, params[lv], stream)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        ms = {"a": [], "b": [], **{f"c{lv}": [] for lv in LEVELS}}
        for r in range(WARMUP + args.rounds):
            row = {"a": run_a(), "b": run_b()}
            for lv in LEVELS:
                row[f"c{lv}"] = run_c(lv)
            if r >= WARMUP:
                for k, v in row.items():
                    ms[k].append(v)
        valid = int(torch.isfinite(f["depth"]).sum().item())
        # the scene covers a small part of the frame, and a pixel that is not valid costs no tap: the same
        # call with every pixel made valid (depth 1, normal +Z, one object) is the filter's full cost
        f["depth"].fill_(1.0)
        f["normal"].view(-1, 3)[:, 2] = 1.0
        f["object"].fill_(0)
        ms["c4_all_valid"] = [run_c(4) for _ in range(WARMUP + args.rounds)][WARMUP:]
        for k, v in ms.items():
            med = statistics.median(v)
            line = {"size": f"{w}x{h}", "variant": k, "runs": len(v), "ms_median": round(med, 4),
                    "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
            if k.startswith("c"):
                lv = int(k[1:].split("_")[0])
                moved = denoise_bytes_per_pixel(lv) * n
                line.update({"levels": lv, "valid_pixels": n if k.endswith("all_valid") else valid, "bytes_moved": moved,
                             "gb_per_s_median": round(moved / (med * 1e-3) / 1e9, 1),
                             "workspace_bytes": nbytes})
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
