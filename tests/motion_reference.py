"""Temporal accumulation with per-object motion (rt_temporal_motion_async /
rt_temporal_motion_host, include/rt_api.h) restated in numpy:
temporal_reference.reference, and variance_reference.moments_reference's moment
sums beside it, plus the one subtraction of step 3 -- the world point is moved
back by its object's translation before it is taken into the previous camera.

Float64 arithmetic on values widened from float32, float32 stores, the
definition's own order; a step is one whole-image operation, a skipped tap
leaves its sums as they are (np.where, not an added zero).  reference() also
returns each pixel's class (temporal_reference's), so that the tests can show
that every branch is taken.

The cases are temporal_reference.CASES with the table TABLE for the synthetic
ids 0, 1, 2; case_inputs() adds the albedo and the previous moments that the
form with moments reads."""
import functools

import numpy as np

import temporal_reference as tref
from temporal_reference import ALL_FOUR, INVALID, LEFT, PARTIAL, REJECTED, STARTED  # noqa: F401
from variance_reference import demod, lum

# ids 0 and 1 move by about a pixel or two at depth 2 (a pixel is about 0.03 wide there), id 2 stands still
TABLE = np.array([[0.12, 0.05, -0.04], [-0.10, 0.08, 0.06], [0, 0, 0]], np.float64)
TABLE.flags.writeable = False


def reference(cur, prev=None, motion=None, moments=False, **params):
    """(color (H, W, 3) float32, count (H, W) float32, class (H, W) int, moments (H, W, 2) float32 or None).
    cur / prev: dicts of color, depth, object, frame and optionally normal (count in prev; with moments, albedo
    optionally in cur and moments in prev); motion: (num_objects, 3) float64; params: fields of rt_temporal."""
    p = dict(tref.DEFAULTS, **params)
    max_history, depth_tol = float(p["max_history"]), float(p["depth_tol"])
    normal_min, min_weight = float(p["normal_min"]), float(p["min_weight"])
    motion = np.asarray(motion, np.float64)
    assert motion.ndim == 2 and motion.shape[1] == 3 and motion.shape[0] >= 1
    color = np.ascontiguousarray(cur["color"], np.float32)
    h, w = cur["depth"].shape
    valid = np.isfinite(cur["depth"])
    out = color.copy()
    count = np.where(valid, np.float32(1), np.float32(0)).astype(np.float32)
    mom = None
    if moments:
        with np.errstate(all="ignore"):
            l = lum(demod(color, cur.get("albedo")))
            mcur = np.stack([l, l * l], axis=-1)
        mom = mcur.astype(np.float32)
    if prev is None:
        return out, count, np.where(valid, STARTED, INVALID), mom
    dot = tref.dot
    fc, fp = [float(v) for v in cur["frame"]], [float(v) for v in prev["frame"]]
    o, lo, hz, vt = fc[0:3], fc[3:6], fc[6:9], fc[9:12]
    po, pl, ph, pv = fp[0:3], fp[3:6], fp[6:9], fp[9:12]
    g = [pl[k] - po[k] for k in range(3)]
    a = [(g[k] + ph[k] * 0.5) + pv[k] * 0.5 for k in range(3)]
    aa, hh, vv = dot(a, a), dot(ph, ph), dot(pv, pv)
    assert aa > 0 and hh > 0 and vv > 0
    yy, xx = np.mgrid[0:h, 0:w]
    ids = np.asarray(cur["object"])
    in_table = (ids >= 0) & (ids < motion.shape[0])  # (compared before it indexes)
    m = np.where(in_table[..., None], motion[np.where(in_table, ids, 0)], 0.0)
    with np.errstate(all="ignore"):
        z = cur["depth"].astype(np.float64)
        u = (xx.astype(np.float64) + 0.5) / float(w)
        v = (yy.astype(np.float64) + 0.5) / float(h)
        d = []
        for k in range(3):
            direction = ((lo[k] + hz[k] * u) + vt[k] * v) - o[k]
            P = o[k] + direction * z
            Pm = P - m[..., k]  # the one addition: where that surface point was
            d.append(Pm - po[k])
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
        nrm = cur.get("normal") is not None
        assert nrm == (prev.get("normal") is not None)
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
        n1 = sumn / sumw + 1.0
        n1 = np.where(n1 > max_history, max_history, n1)
        blend = (hist + (c64 - hist) / n1[..., None]).astype(np.float32)
        out = np.where(has[..., None], blend, color)
        count = np.where(has, n1.astype(np.float32), count).astype(np.float32)
        if moments:
            hm = summ / sumw[..., None]
            mblend = (hm + (mcur - hm) / n1[..., None]).astype(np.float32)
            mom = np.where(has[..., None], mblend, mom)
    cls = np.where(~valid, INVALID, np.where(~inside, LEFT, np.where(~has, REJECTED,
                                                                      np.where(taken == 4, ALL_FOUR, PARTIAL))))
    return out, count, cls, mom


@functools.lru_cache(maxsize=None)
def _extras(w, h):
    """Read-only (albedo, previous moments) for a w x h case: an albedo in [0, 1) with about 10 % exact zeros;
    m1 in [0, 2), m2 = m1^2 + a variance in [0, 0.5)."""
    rng = np.random.default_rng(1000 * w + h)
    albedo = rng.random((h, w, 3)).astype(np.float32)
    albedo[rng.random((h, w, 3)) < 0.1] = 0
    m1 = rng.random((h, w)) * 2
    mom = np.stack([m1, m1 * m1 + rng.random((h, w)) * 0.5], axis=-1).astype(np.float32)
    albedo.flags.writeable = False
    mom.flags.writeable = False
    return albedo, mom


def case_inputs(name, moments=False):
    """temporal_reference.case_inputs(name), and with moments cur's albedo and prev's moments."""
    cur, prev, params = tref.case_inputs(name)
    if moments:
        h, w = cur["depth"].shape
        albedo, mom = _extras(w, h)
        cur["albedo"] = albedo
        if prev is not None:
            prev["moments"] = mom
    return cur, prev, params


@functools.lru_cache(maxsize=None)
def case_reference(name, moments=False, zero=False, rows=3):
    """The case's reference (color, count, class, moments) with TABLE (zero: a table of zeros; rows: only the
    table's first rows), computed once, read-only, and checked to be finite.  Not for "object NULL": the call
    refuses it."""
    cur, prev, params = case_inputs(name, moments)
    table = (np.zeros_like(TABLE) if zero else TABLE)[:rows]
    out = reference(cur, prev, table, moments, **params)
    assert all(np.isfinite(a).all() for a in out if a is not None), name
    for arr in out:
        if arr is not None:
            arr.flags.writeable = False
    return out


bits = tref.bits
