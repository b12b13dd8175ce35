"""Variance-guided denoising (rt_temporal_moments_async, rt_variance_async,
rt_denoise_var_async and their _host twins, include/rt_api.h)
restated in numpy from the header's text, for the tests that demand equal bits
of the host functions and of the kernels.

Float64 arithmetic on values widened from float32, float32 stores, and the
definitions' own order.  As in temporal_reference.py and denoise_reference.py a
tap is one whole-image operation, which changes nothing per pixel: every pixel
sees its taps in the same order and a skipped tap leaves its sums as they are
(np.where, not an added zero).

synthetic() makes the seeded inputs every bit-equality test shares."""
import functools

import numpy as np

import denoise_reference as dref
import temporal_reference as tref

AMIN = 2.0 ** -6
EPS = 2.0 ** -40
H3 = (0.375, 0.25, 0.0625)
K3 = (0.25, 0.125, 0.0625)
VARIANCE_DEFAULTS = dict(min_history=4.0, normal_power=32, sigma_depth=0.05)
FILTER_DEFAULTS = dict(levels=4, normal_power=32, sigma_lum=2.0, sigma_depth=0.05, demodulate=1, prefilter=1)
TEMPORAL, SPATIAL, INVALID = 1, 2, 0  # a pixel's branch in the variance pass


def lum(e):
    return (0.2126 * e[..., 0] + 0.7152 * e[..., 1]) + 0.0722 * e[..., 2]


def demod(color, albedo):
    """e(c, a) in float64, not rounded in between."""
    c = color.astype(np.float64)
    if albedo is None:
        return c
    a = albedo.astype(np.float64)
    return c / np.where(a > AMIN, a, AMIN)


# ---- 1. the moments pass
def moments_reference(cur, prev=None, **params):
    """(color, count, moments (H, W, 2) float32, had a history (H, W) bool).  cur / prev as in
    temporal_reference.reference, cur optionally with albedo, prev with moments."""
    p = dict(tref.DEFAULTS, **params)
    max_history, depth_tol = float(p["max_history"]), float(p["depth_tol"])
    normal_min, min_weight = float(p["normal_min"]), float(p["min_weight"])
    color = np.ascontiguousarray(cur["color"], np.float32)
    h, w = cur["depth"].shape
    valid = np.isfinite(cur["depth"])
    with np.errstate(all="ignore"):
        l = lum(demod(color, cur.get("albedo")))
        mcur = np.stack([l, l * l], axis=-1)
    moments = mcur.astype(np.float32)
    count = np.where(valid, np.float32(1), np.float32(0)).astype(np.float32)
    if prev is None:
        return color.copy(), count, moments, np.zeros((h, w), bool)
    dot = tref.dot
    fc, fp = [float(v) for v in cur["frame"]], [float(v) for v in prev["frame"]]
    o, lo, hz, vt = fc[0:3], fc[3:6], fc[6:9], fc[9:12]
    po, pl, ph, pv = fp[0:3], fp[3:6], fp[6:9], fp[9:12]
    g = [pl[k] - po[k] for k in range(3)]
    a = [(g[k] + ph[k] * 0.5) + pv[k] * 0.5 for k in range(3)]
    aa, hh, vv = dot(a, a), dot(ph, ph), dot(pv, pv)
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        z = cur["depth"].astype(np.float64)
        u = (xx.astype(np.float64) + 0.5) / float(w)
        v = (yy.astype(np.float64) + 0.5) / float(h)
        d = []
        for k in range(3):
            direction = ((lo[k] + hz[k] * u) + vt[k] * v) - o[k]
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
        pm = prev["moments"].astype(np.float64)
        ids, nrm = cur.get("object") is not None, cur.get("normal") is not None
        if nrm:
            n_p, n_q = cur["normal"].astype(np.float64), prev["normal"].astype(np.float64)
        sumw, sums, sumn, summ = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w, 2))
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
                summ = np.where(ok[..., None], summ + wgt[..., None] * pm[cy, cx], summ)
        has = inside & (sumw >= min_weight)
        hist = sums / sumw[..., None]
        n1 = sumn / sumw + 1.0
        n1 = np.where(n1 > max_history, max_history, n1)
        blend = (hist + (c64 - hist) / n1[..., None]).astype(np.float32)
        hm = summ / sumw[..., None]
        mblend = (hm + (mcur - hm) / n1[..., None]).astype(np.float32)
        out = np.where(has[..., None], blend, color)
        count = np.where(has, n1.astype(np.float32), count).astype(np.float32)
        moments = np.where(has[..., None], mblend, moments)
    return out, count, moments, has


# ---- the guide weight of both spatial passes: steps 2 and 3 of the denoiser's tap weight, continued from wgt
def guide_weight(wgt, n, z, P, Q, power, sigma_depth):
    if power > 0:
        t = (n[P][..., 0] * n[Q][..., 0] + n[P][..., 1] * n[Q][..., 1]) + n[P][..., 2] * n[Q][..., 2]
        t = np.where(t > 0, t, 0.0)
        for _ in range(power.bit_length() - 1):
            t = t * t
        wgt = wgt * t
    if sigma_depth > 0:
        r = (z[Q] - z[P]) / (sigma_depth * z[P])
        wgt = wgt / (1.0 + r * r)
    return wgt


def windows(h, w, oy, ox):
    """(P, Q): the pixels p whose neighbour q = p + (ox, oy) is inside the image, and those q; None if none."""
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


# ---- 2. the variance pass
def variance_reference(color, normal, depth, albedo=None, object=None, moments=None, count=None, **params):
    """(variance (H, W) float32, branch (H, W) int: TEMPORAL, SPATIAL or INVALID)."""
    p = dict(VARIANCE_DEFAULTS, **params)
    min_history, power, sigma_depth = float(p["min_history"]), int(p["normal_power"]), float(p["sigma_depth"])
    assert (moments is None) == (count is None)
    h, w = depth.shape
    valid = np.isfinite(depth)
    z, n = depth.astype(np.float64), normal.astype(np.float64)
    ids = np.zeros((h, w), np.int32) if object is None else np.asarray(object, np.int32)
    with np.errstate(all="ignore"):
        if moments is not None:
            m = moments.astype(np.float64)
            c = count.astype(np.float64)
            nn = np.where(c > 1, c, 1.0)
            temporal = valid & (c >= min_history)
        else:
            l = lum(demod(np.ascontiguousarray(color, np.float32), albedo))
            m = np.stack([l, l * l], axis=-1)
            nn = np.ones((h, w))
            temporal = np.zeros((h, w), bool)
        vt = m[..., 1] - m[..., 0] * m[..., 0]
        vt = np.where(vt > 0, vt, 0.0)
        out_t = (vt / nn).astype(np.float32)
        sumw, s1, s2 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                pq = windows(h, w, dy, dx)
                if pq is None:
                    continue
                P, Q = pq
                ok = valid[P] & valid[Q] & (ids[P] == ids[Q])
                wgt = guide_weight(np.ones(ok.shape), n, z, P, Q, power, sigma_depth)
                s1[P] = np.where(ok, s1[P] + wgt * m[Q][..., 0], s1[P])
                s2[P] = np.where(ok, s2[P] + wgt * m[Q][..., 1], s2[P])
                sumw[P] = np.where(ok, sumw[P] + wgt, sumw[P])
        a = s1 / sumw
        vs = s2 / sumw - a * a
        vs = np.where(vs > 0, vs, 0.0)
        out_s = np.where(sumw > 0, (vs / nn).astype(np.float32), np.float32(0)).astype(np.float32)
    out = np.where(valid, np.where(temporal, out_t, out_s), np.float32(0)).astype(np.float32)
    return out, np.where(~valid, INVALID, np.where(temporal, TEMPORAL, SPATIAL))


# ---- 3. the variance-guided filter
def filter_reference(color, normal, depth, variance, albedo=None, object=None, **params):
    """(linear (H, W, 3) float32, variance after the last level (H, W) float32)."""
    p = dict(FILTER_DEFAULTS, **params)
    levels, power = int(p["levels"]), int(p["normal_power"])
    sigma_lum, sigma_depth, prefilter = float(p["sigma_lum"]), float(p["sigma_depth"]), int(p["prefilter"])
    color = np.ascontiguousarray(color, np.float32)
    h, w = depth.shape
    valid = np.isfinite(depth)
    z, n = depth.astype(np.float64), normal.astype(np.float64)
    ids = np.zeros((h, w), np.int32) if object is None else np.asarray(object, np.int32)
    dm = bool(p["demodulate"]) and albedo is not None
    var = np.ascontiguousarray(variance, np.float32).copy()
    with np.errstate(all="ignore"):
        if dm:
            a = albedo.astype(np.float64)
            floor = np.where(a > AMIN, a, AMIN)
            e = (color.astype(np.float64) / floor).astype(np.float32)
        else:
            e = color.copy()
        for i in range(levels):
            s = 1 << i
            e64, v64 = e.astype(np.float64), var.astype(np.float64)
            if sigma_lum > 0:
                g = v64
                if prefilter:
                    sumg, sumk = np.zeros((h, w)), np.zeros((h, w))
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            pq = windows(h, w, dy, dx)
                            if pq is None:
                                continue
                            P, Q = pq
                            ok = valid[P] & valid[Q] & (ids[P] == ids[Q])
                            k = K3[abs(dx) + abs(dy)]
                            sumg[P] = np.where(ok, sumg[P] + k * v64[Q], sumg[P])
                            sumk[P] = np.where(ok, sumk[P] + k, sumk[P])
                    g = sumg / sumk
                inv = 1.0 / ((sigma_lum * sigma_lum) * g + EPS)
                le = lum(e64)
            sumw, sums, sumv = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    pq = windows(h, w, s * dy, s * dx)
                    if pq is None:
                        continue
                    P, Q = pq
                    ok = valid[P] & valid[Q] & (ids[P] == ids[Q])
                    wgt = guide_weight(np.full(ok.shape, H3[abs(dx)] * H3[abs(dy)]), n, z, P, Q, power, sigma_depth)
                    if sigma_lum > 0:
                        d = le[Q] - le[P]
                        wgt = wgt / (1.0 + (d * d) * inv[P])
                    sumw[P] = np.where(ok, sumw[P] + wgt, sumw[P])
                    sums[P] = np.where(ok[..., None], sums[P] + wgt[..., None] * e64[Q], sums[P])
                    sumv[P] = np.where(ok, sumv[P] + (wgt * wgt) * v64[Q], sumv[P])
            upd = valid & (sumw > 0)
            e = np.where(upd[..., None], (sums / sumw[..., None]).astype(np.float32), e)
            var = np.where(upd, (sumv / (sumw * sumw)).astype(np.float32), var)
        out = (e.astype(np.float64) * floor).astype(np.float32) if dm else e
    return np.where(valid[..., None], out, color), var


# ---- the seeded inputs
@functools.lru_cache(maxsize=None)
def synthetic(w, h, seed=17):
    """Read-only: (cur, prev) frames of temporal_reference.synthetic (colour, depth with about 15 % +Inf,
    ids 0..2, normals, look-at cameras), cur with an albedo in [0, 1) that has about 10 % exact zeros and
    prev with moments: m1 in [0, 2), m2 = m1^2 + a variance in [0, 0.5).  And the spatial passes' inputs
    over the CURRENT frame: counts in [1, 40] (so that min_history 4 splits the pixels), moments likewise."""
    rng = np.random.default_rng(seed)
    cur, prev = (dict(f) for f in tref.synthetic(w, h))
    albedo = rng.random((h, w, 3)).astype(np.float32)
    albedo[rng.random((h, w, 3)) < 0.1] = 0

    def moments():
        m1 = rng.random((h, w)) * 2
        return np.stack([m1, m1 * m1 + rng.random((h, w)) * 0.5], axis=-1).astype(np.float32)

    cur["albedo"] = albedo
    prev["moments"] = moments()
    cur_moments = moments()
    cur_count = rng.integers(1, 41, (h, w)).astype(np.float32)
    cur_count[rng.random((h, w)) < 0.25] = np.float32(2)  # (a quarter of the histories is shorter than 4)
    variance = (rng.random((h, w)) * 0.2).astype(np.float32)
    variance[rng.random((h, w)) < 0.1] = 0
    for a in (albedo, prev["moments"], cur_moments, cur_count, variance):
        a.flags.writeable = False
    return cur, prev, dict(moments=cur_moments, count=cur_count, variance=variance)


# The cases all three calls are held to (each call reads the fields that are its own).  33 x 17: a partial
# wave and a partial block of rows; 70 x 5: two waves per row; 3 x 2: the 7 x 7 window, the 3 x 3
# prefilter and every à-trous step exceed the image; levels 5: step 16 against 33 x 17.
BASE = dict(w=33, h=17)
CASES = {
    "33x17": BASE,
    "1x1": dict(w=1, h=1),
    "70x5": dict(w=70, h=5),
    "3x2": dict(w=3, h=2),
    "levels 1": dict(BASE, filter=dict(levels=1)),
    "levels 5": dict(BASE, filter=dict(levels=5)),
    "sigma_lum 0": dict(BASE, filter=dict(sigma_lum=0.0)),
    "prefilter 0": dict(BASE, filter=dict(prefilter=0)),
    "normal_power 0": dict(BASE, filter=dict(normal_power=0), variance=dict(normal_power=0)),
    "sigma_depth 0": dict(BASE, filter=dict(sigma_depth=0.0), variance=dict(sigma_depth=0.0)),
    "albedo NULL": dict(BASE, drop=("albedo",)),
    "object NULL": dict(BASE, drop=("object",)),
    "moments NULL": dict(BASE, drop=("moments",)),
    "moments and albedo NULL": dict(BASE, drop=("moments", "albedo")),
    "prev NULL": dict(BASE, no_prev=True),
    "min_history 1": dict(BASE, variance=dict(min_history=1.0)),
    "min_history 1e9": dict(BASE, variance=dict(min_history=1e9)),
}
MOMENTS_CASES = ["33x17", "1x1", "70x5", "3x2", "albedo NULL", "object NULL", "prev NULL"]
VARIANCE_CASES = ["33x17", "1x1", "70x5", "3x2", "normal_power 0", "sigma_depth 0", "albedo NULL", "object NULL",
                  "moments NULL", "moments and albedo NULL", "min_history 1", "min_history 1e9"]
FILTER_CASES = ["33x17", "1x1", "70x5", "3x2", "levels 1", "levels 5", "sigma_lum 0", "prefilter 0", "normal_power 0",
                "sigma_depth 0", "albedo NULL", "object NULL"]
FILTER_BASE = dict(levels=3)  # (the cases' levels unless they set it: steps 1, 2, 4)


def moments_inputs(name):
    """(cur, prev or None, rt_temporal fields): the frames of the moments pass."""
    c = CASES[name]
    cur, prev, _ = synthetic(c["w"], c["h"])
    cur, prev = dict(cur), dict(prev)
    for k in c.get("drop", ()):
        if k == "albedo":
            del cur[k]
        elif k == "object":
            del cur[k], prev[k]
    del cur["count"]
    return cur, (None if c.get("no_prev") else prev), {}


def spatial_inputs(name):
    """(dict of color, normal, depth, albedo, object, moments, count, variance -- None where the case drops
    it --, rt_variance fields, rt_denoise_var fields): the inputs of the variance pass and of the filter."""
    c = CASES[name]
    cur, _, extra = synthetic(c["w"], c["h"])
    inp = dict(color=cur["color"], normal=cur["normal"], depth=cur["depth"], albedo=cur["albedo"],
               object=cur["object"], **extra)
    for k in c.get("drop", ()):
        inp[k] = None
        if k == "moments":
            inp["count"] = None
    return inp, dict(c.get("variance", {})), dict(FILTER_BASE, **c.get("filter", {}))


def _frozen(arrs):
    for a in arrs:
        a.flags.writeable = False
    return arrs


@functools.lru_cache(maxsize=None)
def moments_case_reference(name):
    cur, prev, params = moments_inputs(name)
    out = moments_reference(cur, prev, **params)
    assert all(np.isfinite(a).all() for a in out[:3]), name
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def variance_case_reference(name):
    inp, vp, _ = spatial_inputs(name)
    out = variance_reference(inp["color"], inp["normal"], inp["depth"], inp["albedo"], inp["object"], inp["moments"],
                             inp["count"], **vp)
    assert np.isfinite(out[0]).all(), name
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def filter_case_reference(name):
    inp, _, fp = spatial_inputs(name)
    out = filter_reference(inp["color"], inp["normal"], inp["depth"], inp["variance"], inp["albedo"], inp["object"], **fp)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all(), name
    return _frozen(out)


bits = dref.bits
