#!/usr/bin/env python3
"""What the BVH over spheres and cubes buys, and from how many cubes on
(a dev tool, not the bench contract).

usage: mixed_bvh_ab.py gain  [PARENT_LIB]
         10k spheres (scenes/gen_spheres.py generate(10000), the scene of
         tests/scene_cases.py spheres10k_scene and of bench.py's C4) with one
         floor cube of 80 x 1 x 90 under them, 320x180x4: this build's tree on
         the wavefront path and on the megakernel against the linear scan
         (force_bvh = -1, and, when PARENT_LIB names a librtgo.so of the parent
         commit, that build at force_bvh = 0), alternating; the same scene
         without the cube; and the share of soft shadow rays the wavefront
         path traced (rt_counts.soft_occlusion) rather than settled by lists.
       mixed_bvh_ab.py sweep
         cubes-only grids of 8, 16, 32, 64 and 128 cubes at 640x480x16, and 70
         spheres with three cubes (tests/mixed_cases.py field70), force_bvh =
         -1 against the tree on this build, alternating.
       mixed_bvh_ab.py c4 PARENT_LIB
         a C4 frame (10k spheres, 1920x1080x64, no cube) on this build and on
         the parent's, alternating: the sphere-only wavefront kernels.

Every measurement runs in a process of its own (RTGO_LIB picks the library)
and prints kernel ms per frame (HIP events) and the image checksum.
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIS = os.path.join(ROOT, "concurrent-raytracer-go_amd", "build", "librtgo.so")

CHILD = r'''
import json, os, sys
sys.path.insert(0, os.path.join(ROOT, "concurrent-raytracer-go_amd")); sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, rtgo
spec = json.loads(sys.argv[1])
if spec["scene"] == "grid":
    import mixed_cases as mc
    text = json.dumps(mc.cube_grid(spec["n"]))
elif spec["scene"] == "field70":
    import mixed_cases as mc
    text = json.dumps(mc.field70())
else:
    import importlib.util
    sp = importlib.util.spec_from_file_location("gen_spheres", os.path.join(ROOT, "scenes", "gen_spheres.py"))
    g = importlib.util.module_from_spec(sp); sp.loader.exec_module(g)
    sc = g.generate(10000)
    if spec["scene"] == "10k_floor":  # a floor cube under the field (the spheres' y is in [-20, 20])
        sc["objects"].append({"type": "cube", "position": [0, -22, -45], "size": [80, 1, 90],
                              "material": {"type": "lambertian", "color": [0.5, 0.5, 0.5]}})
    text = g.dumps(sc)
scene = rtgo.Scene.from_json_text(text)
w, h, spp, reps = spec["w"], spec["h"], spec["spp"], spec["reps"]
s = torch.cuda.Stream(); torch.cuda.set_stream(s)
ctx = rtgo.Context(0)
if spec.get("mega"):
    ctx.set_tuning(rtgo.default_tuning(path=rtgo.RT_PATH_MEGAKERNEL))
ctx.set_scene(scene, force_bvh=spec["force"])
st = rtgo.default_settings(); st.samples = spp
lin = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
ms = []
for i in range(reps + spec["warm"]):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(s); ctx.render_async(w, h, st, lin.data_ptr(), rgba.data_ptr(), s.cuda_stream); e1.record(s)
    torch.cuda.synchronize()
    if i >= spec["warm"]: ms.append(e0.elapsed_time(e1))
extra = {}
if spec.get("cones"):  # one counting render: the soft rays traced by wf_occlude<soft> against all soft rays
    c = ctx.count(w, h, st, lin.data_ptr(), rgba.data_ptr(), s.cuda_stream, full=True)
    torch.cuda.synchronize()
    d = c.as_dict()
    extra = {"soft": d["shadow_rays"] - d["light_evals"], "traced": c.soft_occlusion_dict()["shadow_rays"]}
ctx.close()
print("RESULT", json.dumps(dict({"ms": ms, "sum": float(torch.nan_to_num(lin.double()).sum())}, **extra)))
'''.replace("ROOT", repr(ROOT))


def measure(lib, **spec):
    env = dict(os.environ, RTGO_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps(spec)], env=env, capture_output=True, text=True,
                       timeout=spec.get("limit", 300))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")]
    if r.returncode != 0 or not line:
        print("FAILED rc=%d" % r.returncode, spec, r.stderr[-2000:], flush=True)
        sys.exit(r.returncode or 1)  # (nothing more is started on the GPU)
    return json.loads(line[0][7:])


def show(label, res):
    ms = res["ms"]
    print("%-44s median %10.3f ms  min %10.3f  max %10.3f  (n=%d)  sum %.9g" %
          (label, statistics.median(ms), min(ms), max(ms), len(ms), res["sum"]), flush=True)
    if "soft" in res:
        print("%-44s soft shadow rays %d, traced %d: %.1f %% of the clear cones" %
              (label, res["soft"], res["traced"], 100.0 * res["traced"] / max(1, res["soft"])), flush=True)


def gain(parent):
    frame = dict(w=320, h=180, spp=4)
    for rnd in range(2):
        show("round %d: 10k + floor cube, tree, wavefront" % rnd,
             measure(THIS, scene="10k_floor", force=0, reps=3, warm=1, cones=rnd == 0, **frame))
        show("round %d: 10k + floor cube, tree, megakernel" % rnd,
             measure(THIS, scene="10k_floor", force=0, mega=1, reps=3, warm=1, **frame))
        show("round %d: 10k, no cube (wavefront)" % rnd,
             measure(THIS, scene="10k", force=0, reps=3, warm=1, **frame))
        show("round %d: 10k + floor cube, linear scan" % rnd,
             measure(THIS, scene="10k_floor", force=-1, reps=2, warm=1, limit=420, **frame))
        if parent:
            show("round %d: 10k + floor cube, parent build" % rnd,
                 measure(parent, scene="10k_floor", force=0, reps=2, warm=1, limit=420, **frame))


def sweep():
    frame = dict(w=640, h=480, spp=16)
    for n in (8, 16, 32, 64, 128):
        for rnd in range(2):
            for force, mega, name in ((-1, 0, "linear"), (1, 0, "tree, wavefront"), (1, 1, "tree, megakernel")):
                show("%3d cubes, %s, round %d" % (n, name, rnd),
                     measure(THIS, scene="grid", n=n, force=force, mega=mega, reps=4, warm=1, **frame))
    for rnd in range(2):
        for force, mega, name in ((-1, 0, "linear"), (0, 0, "tree, wavefront"), (0, 1, "tree, megakernel")):
            show("70 spheres + 3 cubes, %s, round %d" % (name, rnd),
                 measure(THIS, scene="field70", force=force, mega=mega, reps=4, warm=1, **frame))


def c4(parent):
    frame = dict(w=1920, h=1080, spp=64)
    for rnd in range(3):
        show("C4 frame, this build, round %d" % rnd, measure(THIS, scene="10k", force=0, reps=2, warm=1, **frame))
        show("C4 frame, parent build, round %d" % rnd, measure(parent, scene="10k", force=0, reps=2, warm=1, **frame))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "gain":
        gain(sys.argv[2] if len(sys.argv) > 2 else None)
    elif len(sys.argv) > 1 and sys.argv[1] == "sweep":
        sweep()
    elif len(sys.argv) > 2 and sys.argv[1] == "c4":
        c4(sys.argv[2])
    else:
        sys.exit(__doc__)
