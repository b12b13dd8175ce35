"""Matte layers and the edge resolve (rt_context_render_matte_async,
rt_matte_resolve_async, include/rt_api.h) restated in Python,
for the tests that demand equal bits of the kernels and the host twin.

The matte.  Sample s of pixel (x, y) is aov_reference.camera_ray's; its hit is
hitWorld(ray, 0.001, +Inf) as aov_reference.first_hit scans it -- the hittables
in scene order with tmax = the closest so far, a sphere through
oracle.sphere_hit, a cube as Mesh.Hit over its twelve oracle.cube_triangles
through oracle.triangle_hit -- in a loop of its own that also keeps WHICH of
the twelve triangles was hit last, the ordinal the face level needs.  keys()
holds the (object, triangle) of every sample of a frame and is cached, so that
every level, rank count and SMALLER sample count of the same frame (a ray
depends on seed, pixel and s only) comes from one walk.

The resolve.  resolve() is the definition of rt_api.h in Python floats
(binary64), in its written order, rounded once through np.float32."""
import functools
import json

import numpy as np

import oracle
import rtgo
from aov_reference import INF, _hittables, bits, camera_ray  # noqa: F401  (bits: re-exported)

SLOTS = 16


def first_hit_face(hittables, o, d):
    """hitWorld(ray, 0.001, +Inf): (hittable index, triangle ordinal 0..11 in its cube, 0 for a sphere) or None."""
    import ctypes

    lib = oracle.lib()
    co, cd, rec = oracle.d3(o), oracle.d3(d), (ctypes.c_double * 8)()
    closest, best = INF, None
    for i, (kind, geo, _) in enumerate(hittables):
        if kind == "sphere":
            if lib.oracle_sphere_hit(geo[0], geo[1], co, cd, 0.001, closest, rec):
                closest, best = rec[0], (i, 0)
        else:  # Mesh.Hit: the closest of its triangles within [tmin, closest]; a later one replaces on acceptance
            mclosest, tri = closest, None
            for f, (v0, v1, v2) in enumerate(geo):
                if lib.oracle_triangle_hit(v0, v1, v2, co, cd, 0.001, mclosest, rec):
                    mclosest, tri = rec[0], f
            if tri is not None:
                closest, best = mclosest, (i, tri)
    return best


@functools.lru_cache(maxsize=None)
def keys(scene_text, w, h, samples, seed, camera_text=None, model=rtgo.RT_CAMERA_REFERENCE):
    """(H, W, samples, 2) int32, read-only: the (object, triangle) of each sample's hit, (-1, -1) for a miss."""
    scene = rtgo.Scene.from_json_text(scene_text)
    cam = json.loads(camera_text) if camera_text is not None else scene
    frame = [float(c) for c in rtgo.camera_frame(cam, model, w, h)]
    hittables = _hittables(scene)
    out = np.full((h, w, samples, 2), -1, np.int32)
    for y in range(h):
        for x in range(w):
            for s in range(samples):
                o, d = camera_ray(frame, w, h, seed, x, y, s)
                hit = first_hit_face(hittables, o, d)
                if hit is not None:
                    out[y, x, s] = hit
    out.flags.writeable = False
    return out


def walk(sample_keys):
    """One pixel's slots after its samples in ascending s: ([(key, count)] in slot order, hits, overflow).
    sample_keys: the key of each sample, None for a miss."""
    slots, hits, overflow = [], 0, 0
    for k in sample_keys:
        if k is None:
            continue
        hits += 1
        for i, (sk, sc) in enumerate(slots):
            if sk == k:
                slots[i] = (sk, sc + 1)
                break
        else:
            if len(slots) < SLOTS:
                slots.append((k, 1))
            else:
                overflow += 1
    return slots, hits, overflow


def matte_of(kk, samples, ranks=4, level="object"):
    """The matte of the first `samples` samples of keys() array kk: id, count (K, H, W) int32, rest (H, W) int32,
    and for the conditions hits, overflow, used (slots taken) and tie (two ranks within K + 1 of equal count)."""
    h, w = kk.shape[:2]
    assert samples <= kk.shape[2]
    out = {"id": np.full((ranks, h, w), -1, np.int32), "count": np.zeros((ranks, h, w), np.int32),
           "rest": np.zeros((h, w), np.int32), "hits": np.zeros((h, w), np.int32),
           "overflow": np.zeros((h, w), np.int32), "used": np.zeros((h, w), np.int32), "tie": np.zeros((h, w), bool)}
    for y in range(h):
        for x in range(w):
            ks = []
            for s in range(samples):
                obj, tri = int(kk[y, x, s, 0]), int(kk[y, x, s, 1])
                ks.append(None if obj < 0 else (obj * 16 + tri if level == "face" else obj))
            slots, hits, overflow = walk(ks)
            order = sorted(slots, key=lambda kc: (-kc[1], kc[0]))  # count descending, key ascending among equals
            rest = hits
            for r, (k, c) in enumerate(order[:ranks]):
                out["id"][r, y, x], out["count"][r, y, x] = k, c
                rest -= c
            out["rest"][y, x], out["hits"][y, x], out["overflow"][y, x], out["used"][y, x] = rest, hits, overflow, len(slots)
            out["tie"][y, x] = any(order[i][1] == order[i + 1][1] for i in range(min(ranks, len(order) - 1)))
    for a in out.values():
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def reference(scene_text, w, h, samples, seed, ranks=4, level="object", camera_text=None,
              model=rtgo.RT_CAMERA_REFERENCE, walk_samples=None):
    """matte_of over keys() of the frame; walk_samples: the (larger) sample count of the cached walk to share."""
    return matte_of(keys(scene_text, w, h, walk_samples or samples, seed, camera_text, model), samples, ranks, level)


def parts_of(count, rest, n):
    """(H, W) int: the number of parts of each pixel in the resolve's step 1."""
    count = np.asarray(count, np.int64)
    rs = np.zeros(count.shape[1:], np.int64) if rest is None else np.asarray(rest, np.int64)
    pos = np.where(count > 0, count, 0)
    miss = n - pos.sum(axis=0) - rs
    return (count > 0).sum(axis=0) + (miss > 0) + (rs > 0)


def resolve(color, obj, ids, count, rest, n, radius=2, background=(0.0, 0.0, 0.0)):
    """rt_matte_resolve_host's out_linear, (H, W, 3) float32, by the definition."""
    color = np.asarray(color, np.float32)
    h, w = color.shape[:2]
    K = count.shape[0]
    out = color.copy()
    parts = parts_of(count, rest, n)
    col = color.astype(np.float64)
    R = radius

    def gather(x, y, key):
        sw, sc = 0.0, [0.0, 0.0, 0.0]
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                qx, qy = x + dx, y + dy
                if qx < 0 or qx >= w or qy < 0 or qy >= h or int(obj[qy, qx]) != key:
                    continue
                wt = 1.0 / (1.0 + float(dx * dx + dy * dy))
                sw += wt
                for k in range(3):
                    sc[k] += wt * float(col[qy, qx, k])
        if not sw > 0:
            return None
        return [sc[k] / sw for k in range(3)]

    for y, x in np.argwhere(parts >= 2):
        y, x = int(y), int(x)
        own = [float(col[y, x, k]) for k in range(3)]
        rs = 0 if rest is None else int(rest[y, x])
        acc, total = [0.0, 0.0, 0.0], 0
        for r in range(K):
            c = int(count[r, y, x])
            if c <= 0:
                continue
            total += c
            part = gather(x, y, int(ids[r, y, x])) or own
            share = float(c) / float(n)
            for k in range(3):
                acc[k] += share * part[k]
        miss = n - total - rs
        if miss > 0:
            part = gather(x, y, -1) or [float(b) for b in background]
            share = float(miss) / float(n)
            for k in range(3):
                acc[k] += share * part[k]
        if rs > 0:
            share = float(rs) / float(n)
            for k in range(3):
                acc[k] += share * own[k]
        with np.errstate(over="ignore", invalid="ignore"):
            out[y, x] = [np.float32(a) for a in acc]
    return out


# ---- scenes and synthetic inputs shared by the CPU and the GPU tests

def overflow_scene():
    """A 5x5 grid of small spheres that all lie inside ONE pixel of a 2x2 image (reference camera at z = 3, aspect
    1: the viewport is 2 high at focal length 1, so a pixel is 3 world units wide at z = 0): at 64 samples that
    pixel meets more than 16 objects, so samples overflow its slots."""
    objs = [{"type": "sphere", "position": [0.3 + 0.58 * i, 0.3 + 0.58 * j, 0.0], "radius": 0.28,
             "material": {"type": "lambertian", "color": [0.2 + 0.03 * i, 0.5, 0.2 + 0.03 * j]}}
            for j in range(5) for i in range(5)]
    return json.dumps({"camera": {"position": [0, 0, 3], "lookAt": [0, 0, 0], "up": [0, 1, 0], "fov": 60,
                                  "aspectRatio": 1.0},
                       "objects": objs,
                       "lights": [{"type": "point", "position": [0, 4, 4], "color": [1, 1, 1], "intensity": 30.0}]})


SYN_SIZES = [(1, 1), (5, 3), (72, 48)]
NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]  # the NaN an invalid operation makes on x86


def syn_inputs(w, h, special=True, K=3, n=8, seed=11):
    """Synthetic resolve inputs, deterministic: patches of object ids -1..4, counts that make about a third of
    the pixels mixed (with ranks whose object has no tap in any window, a rest, and sums past n), and with
    `special` NaN and +-Inf colours.  The NaN is the one bit pattern an invalid operation itself produces, so
    that which operand a NaN is taken from decides nothing.  Returns (color, object, id, count, rest)."""
    rng = np.random.RandomState(seed + 131 * w + h)
    color = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    obj = ((np.arange(w)[None, :] // 3 + np.arange(h)[:, None] // 2) % 6 - 1).astype(np.int32)
    ids = rng.randint(-1, 6, (K, h, w)).astype(np.int32)
    ids[0] = obj
    count = np.zeros((K, h, w), np.int32)
    count[0] = n
    mixed = rng.uniform(size=(h, w)) < 0.35
    c1 = rng.randint(1, n, (h, w))
    count[0][mixed] = (n - c1)[mixed]
    count[1][mixed] = np.minimum(c1, rng.randint(0, n, (h, w)))[mixed]
    if K > 2:
        count[2][mixed & (rng.uniform(size=(h, w)) < 0.2)] = 1
    rest = np.where(mixed & (rng.uniform(size=(h, w)) < 0.25), 1, 0).astype(np.int32)
    count[0][rng.uniform(size=(h, w)) < 0.03] = n + 3   # sums past n: no contract on values, none on addresses
    count[1][rng.uniform(size=(h, w)) < 0.03] = -2      # not a part
    if special and w * h > 1:
        m = rng.uniform(size=(h, w, 3))
        color[m < 0.02] = NEG_NAN
        color[(m > 0.02) & (m < 0.04)] = np.inf
        color[(m > 0.04) & (m < 0.05)] = -np.inf
        color[0, 0, 0], color[-1, -1, 1], color[h // 2, w // 2, 2] = NEG_NAN, np.inf, -np.inf  # (at least one each)
    return color, obj, ids, count, rest
