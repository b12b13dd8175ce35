"""The first-hit feature buffers (rt_context_render_aov_async, include/rt_api.h;
DESIGN.md §4.12) restated in Python from the oracle's own parts, for the tests
that demand equal bits of the kernel.

Sample s of pixel (x, y): the frame of rtgo.camera_frame, the draws of
oracle.rng_draws(seed, y * W + x, s, 2), the ray ((ll + h u) + v v) - o per
component; hitWorld (renderer.go:333-346) as a scan over the hittables in scene
order with tmax = the closest so far (an exact tie goes to the later one), a
sphere through oracle.sphere_hit, a cube as Mesh.Hit over its twelve
oracle.cube_triangles through oracle.triangle_hit.  The per-pixel sums are
Python floats (binary64), added in ascending s.

reference() takes the scene as JSON text (and the camera as JSON text or None)
so that its results can be cached: one computation per case, shared by every
test that needs it, returned read-only."""
import ctypes
import functools
import json

import numpy as np

import oracle
import rtgo

INF = float("inf")
KIND_DIELECTRIC, KIND_DIFFUSELIGHT = rtgo.MATERIAL_KINDS["dielectric"], rtgo.MATERIAL_KINDS["diffuselight"]


def _hittables(scene):
    """[(kind, geometry, albedo)] in hittable order (GetHittables, scene.go:59-90)."""
    out = []
    v = scene.view
    for i in range(v.num_objects):
        o = v.objects[i]
        m = o.material
        if m.kind == KIND_DIELECTRIC:
            albedo = (1.0, 1.0, 1.0)
        elif m.kind == KIND_DIFFUSELIGHT:
            albedo = (0.0, 0.0, 0.0)
        else:
            albedo = tuple(m.color)
        # (the geometry as the C arrays oracle.sphere_hit / oracle.triangle_hit would make per call)
        if o.type == rtgo.RT_OBJ_SPHERE:
            out.append(("sphere", (oracle.d3(o.position), float(o.radius)), albedo))
        else:
            tris = oracle.cube_triangles(tuple(o.position), tuple(o.size))
            out.append(("cube", [tuple(oracle.d3(p) for p in t) for t in tris], albedo))
    return out


def first_hit(hittables, o, d):
    """hitWorld(ray, 0.001, +Inf): (hittable index, T, Normal, albedo) or None.
    oracle.sphere_hit and oracle.triangle_hit, called on arrays made once per ray and per scene."""
    lib = oracle.lib()
    co, cd, rec = oracle.d3(o), oracle.d3(d), (ctypes.c_double * 8)()
    closest, best = INF, None
    for i, (kind, geo, albedo) in enumerate(hittables):
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
            best = (i, hit[0], (hit[4], hit[5], hit[6]), albedo)
    return best


def camera_ray(frame, w, h, seed, x, y, s):
    """(origin, direction) of sample s of pixel (x, y): the render's own camera ray."""
    o, ll, hz, vt = frame[0:3], frame[3:6], frame[6:9], frame[9:12]
    draws, _ = oracle.rng_draws(seed, y * w + x, s, 2)
    u = (x + float(draws[0])) / float(w)
    v = (y + float(draws[1])) / float(h)
    d = tuple(((float(ll[k]) + float(hz[k]) * u) + float(vt[k]) * v) - float(o[k]) for k in range(3))
    return tuple(float(c) for c in o), d


@functools.lru_cache(maxsize=None)
def reference(scene_text, w, h, samples, seed, camera_text=None, model=rtgo.RT_CAMERA_REFERENCE):
    """The five buffers as read-only numpy arrays: albedo, normal (H, W, 3) float32, depth, coverage
    (H, W) float32, object (H, W) int32.  camera_text: a scene-file camera as JSON, None: the scene's."""
    scene = rtgo.Scene.from_json_text(scene_text)
    cam = json.loads(camera_text) if camera_text is not None else scene
    frame = [float(c) for c in rtgo.camera_frame(cam, model, w, h)]
    hittables = _hittables(scene)
    out = {"albedo": np.zeros((h, w, 3), np.float32), "normal": np.zeros((h, w, 3), np.float32),
           "depth": np.zeros((h, w), np.float32), "coverage": np.zeros((h, w), np.float32),
           "object": np.zeros((h, w), np.int32)}
    n = float(samples)
    for y in range(h):
        for x in range(w):
            sum_a, sum_n, sum_t, hits, first = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0.0, 0, -1
            for s in range(samples):
                o, d = camera_ray(frame, w, h, seed, x, y, s)
                hit = first_hit(hittables, o, d)
                if hit is None:
                    continue
                idx, t, normal, albedo = hit
                for k in range(3):
                    sum_a[k] += albedo[k]
                    sum_n[k] += normal[k]
                sum_t += t
                if hits == 0:
                    first = idx
                hits += 1
            out["albedo"][y, x] = [sum_a[k] / n for k in range(3)]
            out["normal"][y, x] = [sum_n[k] / n for k in range(3)]
            out["depth"][y, x] = sum_t / hits if hits else INF
            out["coverage"][y, x] = hits / n
            out["object"][y, x] = first
    for a in out.values():
        a.flags.writeable = False
    return out


def bits(a):
    """The bit patterns of a float32 (or int32) array, for exact comparison (NaN-safe)."""
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)
