"""The specular-through feature buffers (rt_context_render_aov_spec_async,
include/rt_api.h) restated in Python from the oracle's own
parts, for the tests that demand equal bits of the kernel.

Ray 0 is aov_reference.camera_ray; hit j is hitWorld as aov_reference.first_hit
scans it (hittable order, tmax = the closest so far, a tie to the later one),
kept here with the whole HitRecord because the chain needs its Point
(rec[1:4]); ray j + 1 leaves that Point in the direction
oracle.vec_op("reflect", d_j, Normal_j), not normalised.  A material is
followed iff its kind is metal, shiny or perfectmirror and
oracle_go_min(roughness, 1.0) <= max_roughness.  The per-pixel sums are Python
floats (binary64), added in ascending s; per sample the albedo product and the
sum of T are formed in chain order.

aov_reference.py is used as it is: its _hittables gives geometry and albedo per
hittable, the material is read beside it from the same scene view.
reference() is cached like aov_reference.reference and returns read-only
arrays, with `stats`, counts over the samples that the tests' conditions read."""
import ctypes
import functools
import json

import numpy as np

import oracle
import rtgo
from aov_reference import INF, _hittables, bits, camera_ray, first_hit  # noqa: F401 (bits: for the tests)

NAMES = ["albedo", "normal", "depth", "coverage", "object", "specular", "bounces"]
FOLLOWED_KINDS = tuple(rtgo.MATERIAL_KINDS[k] for k in ("metal", "shiny", "perfectmirror"))


def follows(kind, roughness, max_roughness):
    """The followed-material predicate: Go's math.Min clamp, a NaN comparing false."""
    return kind in FOLLOWED_KINDS and oracle.lib().oracle_go_min(float(roughness), 1.0) <= max_roughness


def hittables_with_materials(scene):
    """aov_reference._hittables(scene) and, beside it, [(kind, roughness)] per hittable."""
    v = scene.view
    mats = [(int(v.objects[i].material.kind), float(v.objects[i].material.roughness)) for i in range(v.num_objects)]
    return _hittables(scene), mats


def hit_record(hittables, o, d):
    """hitWorld(ray, 0.001, +Inf) as aov_reference.first_hit scans it, returning (hittable index, rec):
    the whole 8-double HitRecord (T, Point, Normal, front)."""
    lib = oracle.lib()
    co, cd, rec = oracle.d3(o), oracle.d3(d), (ctypes.c_double * 8)()
    closest, best = INF, None
    for i, (kind, geo, _) in enumerate(hittables):
        hit = None
        if kind == "sphere":
            if lib.oracle_sphere_hit(geo[0], geo[1], co, cd, 0.001, closest, rec):
                hit = tuple(rec)
        else:  # Mesh.Hit: the closest of its triangles within [tmin, closest]
            mclosest = closest
            for v0, v1, v2 in geo:
                if lib.oracle_triangle_hit(v0, v1, v2, co, cd, 0.001, mclosest, rec):
                    hit = tuple(rec)
                    mclosest = hit[0]
        if hit is not None:
            closest = hit[0]
            best = (i, hit)
    return best


def chain(hittables, mats, o, d, max_bounces, max_roughness):
    """The chain of one sample: [(hittable index, rec, ray origin, ray direction)] of the existing hits
    0 .. terminal, and how it ended: "miss0", "not followed", "cap" or "mirror miss"."""
    out = []
    j = 0
    while True:
        hit = hit_record(hittables, o, d)
        if hit is None:
            return out, ("mirror miss" if out else "miss0")
        idx, rec = hit
        out.append((idx, rec, o, d))
        if not follows(mats[idx][0], mats[idx][1], max_roughness):
            return out, "not followed"
        if j >= max_bounces:
            return out, "cap"
        o, d = tuple(rec[1:4]), oracle.vec_op("reflect", d, rec[4:7])
        j += 1


@functools.lru_cache(maxsize=None)
def reference(scene_text, w, h, samples, seed, camera_text=None, model=rtgo.RT_CAMERA_REFERENCE, max_bounces=4,
              max_roughness=0.1):
    """The seven buffers as read-only numpy arrays (NAMES; specular and bounces (H, W) float32), and under
    "stats" a dict of counts: first_k2 (pixels whose lowest hitting sample has k >= 2), mirror_miss and cap
    (samples whose chain ended that way)."""
    scene = rtgo.Scene.from_json_text(scene_text)
    cam = json.loads(camera_text) if camera_text is not None else scene
    frame = [float(c) for c in rtgo.camera_frame(cam, model, w, h)]
    hittables, mats = hittables_with_materials(scene)
    out = {"albedo": np.zeros((h, w, 3), np.float32), "normal": np.zeros((h, w, 3), np.float32),
           "depth": np.zeros((h, w), np.float32), "coverage": np.zeros((h, w), np.float32),
           "object": np.zeros((h, w), np.int32), "specular": np.zeros((h, w), np.float32),
           "bounces": np.zeros((h, w), np.float32)}
    stats = {"first_k2": 0, "mirror_miss": 0, "cap": 0}
    n = float(samples)
    for y in range(h):
        for x in range(w):
            sum_a, sum_n, sum_t, sum_k, hits, m, first = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0.0, 0.0, 0, 0, -1
            for s in range(samples):
                o, d = camera_ray(frame, w, h, seed, x, y, s)
                links, end = chain(hittables, mats, o, d, max_bounces, max_roughness)
                if not links:
                    continue
                a = list(hittables[links[0][0]][2])
                t = links[0][1][0]
                for idx, rec, _, _ in links[1:]:
                    for c in range(3):
                        a[c] = a[c] * hittables[idx][2][c]
                    t = t + rec[0]
                k = len(links) - 1
                idx, rec = links[-1][0], links[-1][1]
                for c in range(3):
                    sum_a[c] += a[c]
                    sum_n[c] += rec[4 + c]
                sum_t += t
                sum_k += float(k)
                if follows(mats[links[0][0]][0], mats[links[0][0]][1], max_roughness):
                    m += 1
                if hits == 0:
                    first = idx
                    stats["first_k2"] += k >= 2
                hits += 1
                stats["mirror_miss"] += end == "mirror miss"
                stats["cap"] += end == "cap" and max_bounces > 0
            out["albedo"][y, x] = [sum_a[c] / n for c in range(3)]
            out["normal"][y, x] = [sum_n[c] / n for c in range(3)]
            out["depth"][y, x] = sum_t / hits if hits else INF
            out["coverage"][y, x] = hits / n
            out["object"][y, x] = first
            out["specular"][y, x] = m / n
            out["bounces"][y, x] = sum_k / n
    for a in out.values():
        a.flags.writeable = False
    out["stats"] = stats
    return out
