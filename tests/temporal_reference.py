"""Temporal accumulation (rt_temporal_async / rt_temporal_host, include/rt_api.h;
DESIGN.md §4.14) restated in numpy, for the tests that demand equal bits of the
host function and of the kernel.

Float64 arithmetic on values widened from float32, float32 stores, and the
definition's own order: the per-call constants g, a, aa, hh, vv; per pixel the
world point, its place (fx, fy) in the previous image, the four taps with j in
the outer and i in the inner loop, and the blend.  A step is one whole-image
operation here, which changes nothing per pixel: every pixel sees its taps in
the same order, and a skipped tap leaves its sums as they are (np.where, not an
added zero).  reference() also returns each pixel's class, so that the tests
can show that every branch is taken.

synthetic() makes the seeded inputs every bit-equality test shares."""
import functools

import numpy as np

import rtgo

DEFAULTS = dict(max_history=32.0, depth_tol=0.05, normal_min=0.9, min_weight=0.25)
# a pixel's class: not valid; history from all four taps; from some of them; none because the point is
# behind or outside the previous image; none because the taps were rejected (sumw < min_weight)
INVALID, ALL_FOUR, PARTIAL, LEFT, REJECTED, STARTED = 0, 1, 2, 3, 4, 5


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def reference(cur, prev=None, **params):
    """(color (H, W, 3) float32, count (H, W) float32, class (H, W) int).  cur / prev: dicts of color, depth,
    frame and optionally object, normal (and count in prev); params: fields of rt_temporal over DEFAULTS."""
    p = dict(DEFAULTS, **params)
    max_history, depth_tol = float(p["max_history"]), float(p["depth_tol"])
    normal_min, min_weight = float(p["normal_min"]), float(p["min_weight"])
    color = np.ascontiguousarray(cur["color"], np.float32)
    h, w = cur["depth"].shape
    valid = np.isfinite(cur["depth"])
    out = color.copy()
    count = np.where(valid, np.float32(1), np.float32(0)).astype(np.float32)
    if prev is None:
        return out, count, np.where(valid, STARTED, INVALID)
    fc, fp = [float(v) for v in cur["frame"]], [float(v) for v in prev["frame"]]
    o, l, hz, vt = fc[0:3], fc[3:6], fc[6:9], fc[9:12]
    po, pl, ph, pv = fp[0:3], fp[3:6], fp[6:9], fp[9:12]
    g = [pl[k] - po[k] for k in range(3)]
    a = [(g[k] + ph[k] * 0.5) + pv[k] * 0.5 for k in range(3)]
    aa, hh, vv = dot(a, a), dot(ph, ph), dot(pv, pv)
    assert aa > 0 and hh > 0 and vv > 0
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        z = cur["depth"].astype(np.float64)
        u = (xx.astype(np.float64) + 0.5) / float(w)
        v = (yy.astype(np.float64) + 0.5) / float(h)
        d = []
        for k in range(3):
            direction = ((l[k] + hz[k] * u) + vt[k] * v) - o[k]
            P = o[k] + direction * z
            d.append(P - po[k])
        t = dot(d, a) / aa
        e = [d[k] / t - g[k] for k in range(3)]
        fx = (dot(e, ph) / hh) * float(w) - 0.5
        fy = (dot(e, pv) / vv) * float(h) - 0.5
        inside = valid & (t > 0) & (fx > -1) & (fx < w) & (fy > -1) & (fy < h)
        flx, fly = np.floor(np.where(inside, fx, 0.0)), np.floor(np.where(inside, fy, 0.0))
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        wx, wy = fx - flx, fy - fly
        c64 = color.astype(np.float64)
        pc, pz, pn = prev["color"].astype(np.float64), prev["depth"], prev["count"].astype(np.float64)
        ids = cur.get("object") is not None
        nrm = cur.get("normal") is not None
        assert ids == (prev.get("object") is not None) and nrm == (prev.get("normal") is not None)
        if nrm:
            n_p, n_q = cur["normal"].astype(np.float64), prev["normal"].astype(np.float64)
        sumw, sums, sumn = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w))
        taken = np.zeros((h, w), np.int64)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = ix + i, iy + j
                ok = inside & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)  # (read somewhere; masked by ok)
                zq = pz[cy, cx]
                ok &= np.isfinite(zq)
                if ids:
                    ok &= prev["object"][cy, cx] == cur["object"]
                if nrm:
                    q = n_q[cy, cx]
                    nd = (n_p[..., 0] * q[..., 0] + n_p[..., 1] * q[..., 1]) + n_p[..., 2] * q[..., 2]
                    ok &= ~(nd < normal_min)
                if depth_tol > 0:
                    dz = zq.astype(np.float64) - t
                    ok &= ~(np.where(dz < 0, -dz, dz) > depth_tol * t)
                wgt = (wx if i else 1.0 - wx) * (wy if j else 1.0 - wy)
                sumw = np.where(ok, sumw + wgt, sumw)
                sums = np.where(ok[..., None], sums + wgt[..., None] * pc[cy, cx], sums)
                sumn = np.where(ok, sumn + wgt * pn[cy, cx], sumn)
                taken += ok
        has = inside & (sumw >= min_weight)
        hist = sums / sumw[..., None]
        n1 = sumn / sumw + 1.0
        n1 = np.where(n1 > max_history, max_history, n1)
        blend = (hist + (c64 - hist) / n1[..., None]).astype(np.float32)
        out = np.where(has[..., None], blend, color)
        count = np.where(has, n1.astype(np.float32), count).astype(np.float32)
    cls = np.where(~valid, INVALID, np.where(~inside, LEFT, np.where(~has, REJECTED,
                                                                      np.where(taken == 4, ALL_FOUR, PARTIAL))))
    return out, count, cls


# The two cameras of the synthetic cases (the look-at model: nothing is axis-aligned): the previous one is the
# current one trucked by about five pixels' worth at depth 2 and turned a little about its position.
CAM_CUR = {"position": [3, 2, -5], "lookAt": [0.5, 0, 0.25], "up": [0.1, 1, 0.2], "fov": 50, "aspectRatio": 33 / 17}
CAM_PREV = {"position": [3.42, 2.05, -4.8], "lookAt": [0.62, 0.07, 0.3], "up": [0.1, 1, 0.2], "fov": 50,
            "aspectRatio": 33 / 17}


@functools.lru_cache(maxsize=None)
def synthetic(w, h, seed=5, swap=False):
    """(cur, prev), read-only dicts.  Per frame: colour in [0, 2); depth 2 +- 4 % with about 15 % +Inf (none
    at 1 x 1); object ids 0, 1, 2 in blocks of 11 x 6 pixels (-1 where the pixel is not valid); normals near
    the view axis with jitter; in prev, counts in [1, 40].  The frames are rtgo.camera_frame of CAM_CUR /
    CAM_PREV (look-at), the other way round with swap."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    axis = np.array(CAM_CUR["lookAt"], np.float64) - np.array(CAM_CUR["position"], np.float64)
    axis /= np.linalg.norm(axis)
    frames = []
    for cam in ((CAM_PREV, CAM_CUR) if swap else (CAM_CUR, CAM_PREV)):
        color = (rng.random((h, w, 3)) * 2).astype(np.float32)
        depth = (2 * (1 + 0.08 * (rng.random((h, w)) - 0.5))).astype(np.float32)
        invalid = (rng.random((h, w)) < 0.15) & (w * h > 1)
        depth[invalid] = np.inf
        obj = ((xx // 11 + yy // 6) % 3).astype(np.int32)
        obj[invalid] = -1
        nrm = -axis + 0.5 * (rng.random((h, w, 3)) - 0.5)
        normal = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
        count = rng.integers(1, 41, (h, w)).astype(np.float32)
        f = dict(color=color, depth=depth, object=obj, normal=normal, count=count,
                 frame=rtgo.camera_frame(cam, "lookat", w, h))
        for arr in f.values():
            arr.flags.writeable = False
        frames.append(f)
    return frames[0], frames[1]


# The cases the host function and the kernel are both held to.  33 x 17 leaves a partial wave in every row
# and a partial block of rows; 70 x 5 spans two waves per row, the second cut at the image edge; 1 x 1 has
# at most one tap inside the image.
BASE = dict(w=33, h=17, params={})
CASES = {
    "33x17": BASE,
    "1x1": dict(w=1, h=1, params={}),
    "70x5": dict(w=70, h=5, swap=True, params={}),  # (swapped: the columns that leave are on the left)
    "object NULL": dict(BASE, drop=("object",)),
    "normal NULL": dict(BASE, drop=("normal",)),
    "depth_tol 0": dict(BASE, params=dict(depth_tol=0.0)),
    "max_history 8, min_weight 0.6": dict(BASE, params=dict(max_history=8.0, min_weight=0.6)),
    "prev NULL": dict(BASE, no_prev=True),
}
MECHANISMS = ["object NULL", "normal NULL", "depth_tol 0", "max_history 8, min_weight 0.6"]


def case_inputs(name):
    """(cur, prev or None, the rt_temporal fields the case sets); a dropped buffer is absent from both frames."""
    c = CASES[name]
    cur, prev = (dict(f) for f in synthetic(c["w"], c["h"], swap=c.get("swap", False)))
    for k in c.get("drop", ()):
        del cur[k], prev[k]
    del cur["count"]
    return cur, (None if c.get("no_prev") else prev), dict(c["params"])


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """The case's reference (color, count, class), computed once, read-only, and checked to be finite."""
    cur, prev, params = case_inputs(name)
    out = reference(cur, prev, **params)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all(), name
    for arr in out:
        arr.flags.writeable = False
    return out


def bits(a):
    """The bit patterns of a float32 (or integer) array, for exact comparison (NaN-safe)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
