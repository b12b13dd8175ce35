"""History rectification (rt_temporal_clip_async / rt_temporal_clip_host,
include/rt_api.h) restated in numpy from the header's
definition: motion_reference.reference's steps (the table optional, and then
the ids too), and between step 5 and step 6 the window of 5a and the clip of 5b.

Float64 arithmetic on values widened from float32, float32 stores, the
definition's own order; a step is one whole-image operation, a skipped tap
leaves its sums as they are (np.where, not an added zero).  reference() also
returns what the tests need to show that every branch is taken: each pixel's
class (temporal_reference's), the number of channels clipped, nw, and whether
the window was cut by the image edge or by an id change.

The synthetic cases are temporal_reference.synthetic at the sizes at which a
tile or a window can go wrong, with motion_reference's table and extras."""
import functools

import numpy as np

import temporal_reference as tref
from motion_reference import TABLE, _extras
from temporal_reference import ALL_FOUR, INVALID, LEFT, PARTIAL, REJECTED, STARTED  # noqa: F401
from variance_reference import AMIN, demod, lum

DEFAULT_CLIP = dict(radius=1, min_taps=5, gamma=1.0, min_half=0.0)  # rt_history_clip_default


def floor_albedo(albedo):
    """floor(a) of rt_variance's e: the albedo in float64, AMIN where it is not above AMIN."""
    a = albedo.astype(np.float64)
    return np.where(a > AMIN, a, AMIN)


def reference(cur, prev=None, motion=None, moments=False, clip=None, **params):
    """A dict: color (H, W, 3) float32, count (H, W) float32, moments (H, W, 2) float32 or None, clipped (H, W)
    float32, and the diagnostics cls, channels (clipped channels per pixel), nw, has, cut_edge, cut_id.
    cur / prev: dicts of color, depth, frame and optionally object, normal (count in prev; albedo optionally in
    cur; with moments, moments in prev); motion: (num_objects, 3) float64 or None; clip: rt_history_clip's
    fields; params: fields of rt_temporal."""
    p = dict(tref.DEFAULTS, **params)
    k = dict(DEFAULT_CLIP, **(clip or {}))
    radius, min_taps, gamma, min_half = int(k["radius"]), int(k["min_taps"]), float(k["gamma"]), float(k["min_half"])
    max_history, depth_tol = float(p["max_history"]), float(p["depth_tol"])
    normal_min, min_weight = float(p["normal_min"]), float(p["min_weight"])
    color = np.ascontiguousarray(cur["color"], np.float32)
    h, w = cur["depth"].shape
    valid = np.isfinite(cur["depth"])
    ids = cur.get("object")
    albedo = cur.get("albedo")
    out = color.copy()
    count = np.where(valid, np.float32(1), np.float32(0)).astype(np.float32)
    zero = np.zeros((h, w))
    res = dict(moments=None, clipped=zero.astype(np.float32), channels=zero.astype(np.int64),
               nw=zero.astype(np.int64), has=zero.astype(bool), cut_edge=zero.astype(bool), cut_id=zero.astype(bool))
    if moments:
        with np.errstate(all="ignore"):
            l = lum(demod(color, albedo))
            mcur = np.stack([l, l * l], axis=-1)
        res["moments"] = mcur.astype(np.float32)
    if prev is None:
        return dict(res, color=out, count=count, cls=np.where(valid, STARTED, INVALID))
    dot = tref.dot
    fc, fp = [float(v) for v in cur["frame"]], [float(v) for v in prev["frame"]]
    o, lo_, hz, vt = fc[0:3], fc[3:6], fc[6:9], fc[9:12]
    po, pl, ph, pv = fp[0:3], fp[3:6], fp[6:9], fp[9:12]
    g = [pl[j] - po[j] for j in range(3)]
    a = [(g[j] + ph[j] * 0.5) + pv[j] * 0.5 for j in range(3)]
    aa, hh, vv = dot(a, a), dot(ph, ph), dot(pv, pv)
    assert aa > 0 and hh > 0 and vv > 0
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w, 3))
    if motion is not None:
        motion = np.asarray(motion, np.float64)
        assert ids is not None and motion.ndim == 2 and motion.shape[1] == 3 and motion.shape[0] >= 1
        in_table = (ids >= 0) & (ids < motion.shape[0])  # (compared before it indexes)
        m = np.where(in_table[..., None], motion[np.where(in_table, ids, 0)], 0.0)
    with np.errstate(all="ignore"):
        z = cur["depth"].astype(np.float64)
        u = (xx.astype(np.float64) + 0.5) / float(w)
        v = (yy.astype(np.float64) + 0.5) / float(h)
        d = []
        for j in range(3):
            direction = ((lo_[j] + hz[j] * u) + vt[j] * v) - o[j]
            P = o[j] + direction * z
            d.append((P - m[..., j]) - po[j])
        t = dot(d, a) / aa
        e = [d[j] / t - g[j] for j in range(3)]
        fx = (dot(e, ph) / hh) * float(w) - 0.5
        fy = (dot(e, pv) / vv) * float(h) - 0.5
        inside = valid & (t > 0) & (fx > -1) & (fx < w) & (fy > -1) & (fy < h)
        flx, fly = np.floor(np.where(inside, fx, 0.0)), np.floor(np.where(inside, fy, 0.0))
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        wx, wy = fx - flx, fy - fly
        c64 = color.astype(np.float64)
        pc, pz, pn = prev["color"].astype(np.float64), prev["depth"], prev["count"].astype(np.float64)
        nrm = cur.get("normal") is not None
        assert nrm == (prev.get("normal") is not None) and (ids is not None) == (prev.get("object") is not None)
        if nrm:
            n_p, n_q = cur["normal"].astype(np.float64), prev["normal"].astype(np.float64)
        if moments:
            pm = prev["moments"].astype(np.float64)
        sumw, sums, sumn, summ = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w, 2))
        taken = np.zeros((h, w), np.int64)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = ix + i, iy + j
                ok = inside & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)  # (read somewhere; masked by ok)
                zq = pz[cy, cx]
                ok &= np.isfinite(zq)
                if ids is not None:
                    ok &= prev["object"][cy, cx] == ids
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
                if moments:
                    summ = np.where(ok[..., None], summ + wgt[..., None] * pm[cy, cx], summ)
                taken += ok
        has = inside & (sumw >= min_weight)
        hist = sums / sumw[..., None]
        # 5a. the window over the current frame, dy outer and dx inner
        channels = np.zeros((h, w), np.int64)
        nw = np.zeros((h, w), np.int64)
        cut_edge, cut_id = np.zeros((h, w), bool), np.zeros((h, w), bool)
        if radius > 0:
            ev = demod(color, albedo)  # e(q), float64
            s1, s2 = np.zeros((h, w, 3)), np.zeros((h, w, 3))
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    qx, qy = xx + dx, yy + dy
                    inimg = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    cut_edge |= ~inimg
                    cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    ok = inimg & np.isfinite(cur["depth"][cy, cx])
                    if ids is not None:
                        same = ids[cy, cx] == ids
                        cut_id |= ok & ~same
                        ok &= same
                    eq = ev[cy, cx]
                    nw = np.where(ok, nw + 1, nw)
                    s1 = np.where(ok[..., None], s1 + eq, s1)
                    s2 = np.where(ok[..., None], s2 + eq * eq, s2)
            n = nw.astype(np.float64)[..., None]
            mu = s1 / n
            var = s2 / n - mu * mu
            var = np.where(var > 0, var, 0.0)
            half = gamma * np.sqrt(var) + min_half
            fa = floor_albedo(albedo) if albedo is not None else np.ones((h, w, 3))
            he = hist / fa
            lo, hi = mu - half, mu + half
            hc = np.where(he < lo, lo, np.where(he > hi, hi, he))
            replace = (has & (nw >= min_taps))[..., None] & (hc != he)
            hist = np.where(replace, hc * fa, hist)
            channels = replace.sum(axis=-1)
        n1 = sumn / sumw + 1.0
        n1 = np.where(n1 > max_history, max_history, n1)
        blend = (hist + (c64 - hist) / n1[..., None]).astype(np.float32)
        out = np.where(has[..., None], blend, color)
        count = np.where(has, n1.astype(np.float32), count).astype(np.float32)
        if moments:
            hm = summ / sumw[..., None]
            mblend = (hm + (mcur - hm) / n1[..., None]).astype(np.float32)
            res["moments"] = np.where(has[..., None], mblend, res["moments"])
    cls = np.where(~valid, INVALID, np.where(~inside, LEFT, np.where(~has, REJECTED,
                                                                      np.where(taken == 4, ALL_FOUR, PARTIAL))))
    return dict(res, color=out, count=count, cls=cls, clipped=(channels > 0).astype(np.float32), channels=channels,
                nw=np.where(has, nw, 0), has=has, cut_edge=cut_edge & has, cut_id=cut_id & has)


# ---- the synthetic cases: sizes at which a tile (64 x 4) or a window can go wrong
SIZES = [(1, 1), (5, 3), (64, 4), (65, 5), (130, 9), (72, 48)]
# a narrow range so that the random frames clip in one, two and three channels and also pass; min_taps 7 so that
# windows cut by ids, invalid depths and the image edge fall below it
SYN_CLIP = dict(radius=2, min_taps=7, gamma=0.5, min_half=0.01)
# which of (moments, albedo, ids, table, out_clipped, prev) each variant carries: every switch on and off at
# every size (a table needs ids)
VARIANTS = {
    "all": dict(moments=True, albedo=True, ids=True, table=True, clipped=True, prev=True),
    "colour": dict(moments=False, albedo=False, ids=True, table=True, clipped=True, prev=True),
    "albedo, no moments": dict(moments=False, albedo=True, ids=True, table=False, clipped=False, prev=True),
    "no ids": dict(moments=True, albedo=False, ids=False, table=False, clipped=True, prev=True),
    "moments, no table": dict(moments=True, albedo=True, ids=True, table=False, clipped=False, prev=True),
    "prev NULL": dict(moments=True, albedo=True, ids=True, table=True, clipped=True, prev=False),
}


def clip_of(w, h):
    return dict(SYN_CLIP, radius=3) if (w, h) == (5, 3) else dict(SYN_CLIP)  # (image smaller than the window)


def syn_inputs(w, h, variant):
    """(cur, prev or None, table or None) of a synthetic case; the arrays are read-only."""
    v = VARIANTS[variant]
    cur, prev = (dict(f) for f in tref.synthetic(w, h))
    del cur["count"]
    albedo, mom = _extras(w, h)
    if v["albedo"]:
        cur["albedo"] = albedo
    if v["moments"]:
        prev["moments"] = mom
    if not v["ids"]:
        del cur["object"], prev["object"]
    return cur, (prev if v["prev"] else None), (TABLE if v["table"] else None)


@functools.lru_cache(maxsize=None)
def syn_reference(w, h, variant):
    """The case's reference, computed once and read-only."""
    cur, prev, table = syn_inputs(w, h, variant)
    out = reference(cur, prev, table, VARIANTS[variant]["moments"], clip_of(w, h))
    for arr in out.values():
        if arr is not None:
            arr.flags.writeable = False
    return out


bits = tref.bits
