"""The à-trous denoiser (rt_denoise_async / rt_denoise_host, include/rt_api.h;
DESIGN.md §4.13) restated in numpy, for the tests that demand equal bits of the
host function and of the kernels.

Float64 arithmetic on values widened from float32, float32 stores, and the
definition's own order: per level the 25 taps with dy in the outer and dx in
the inner loop, each tap's weight built by steps 1 to 4 in that order, the
sums continued tap by tap.  A tap is one whole-image operation here (the pixels
p whose neighbour q = p + s * (dx, dy) is inside the image), which changes
nothing per pixel: every pixel still sees its taps in the same order, and a
skipped tap leaves its sums as they are (np.where, not an added zero).

synthetic() makes the seeded inputs every bit-equality test shares."""
import functools

import numpy as np

AMIN = 2.0 ** -6
H3 = (0.375, 0.25, 0.0625)
DEFAULTS = dict(levels=4, normal_power=32, sigma_color=0.5, sigma_depth=0.05, demodulate=1)


def reference(color, normal, depth, albedo=None, object=None, **params):
    """The filter's linear output, (H, W, 3) float32.  params: fields of rt_denoise over DEFAULTS."""
    p = dict(DEFAULTS, **params)
    levels, power = int(p["levels"]), int(p["normal_power"])
    sigma_color, sigma_depth = float(p["sigma_color"]), float(p["sigma_depth"])
    assert 1 <= levels <= 8 and (power == 0 or (power & (power - 1) == 0 and power <= 128))
    nsq = power.bit_length() - 1  # log2(power); unused when power == 0
    color = np.ascontiguousarray(color, np.float32)
    h, w = depth.shape
    valid = np.isfinite(depth)
    z, n = depth.astype(np.float64), normal.astype(np.float64)
    ids = np.zeros((h, w), np.int32) if object is None else np.asarray(object, np.int32)
    demod = bool(p["demodulate"]) and albedo is not None
    with np.errstate(all="ignore"):
        if demod:
            a = albedo.astype(np.float64)
            floor = np.where(a > AMIN, a, AMIN)
            e = (color.astype(np.float64) / floor).astype(np.float32)
        else:
            e = color.copy()
        for i in range(levels):
            s = 1 << i
            sc = sigma_color * 2.0 ** -i
            sc2 = sc * sc
            e64 = e.astype(np.float64)
            sumw, sums = np.zeros((h, w)), np.zeros((h, w, 3))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = s * dy, s * dx
                    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue  # q is outside the image for every p
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    ok = valid[P] & valid[Q] & (ids[P] == ids[Q])
                    wgt = np.full(ok.shape, H3[abs(dx)] * H3[abs(dy)])
                    if power > 0:
                        t = (n[P][..., 0] * n[Q][..., 0] + n[P][..., 1] * n[Q][..., 1]) + n[P][..., 2] * n[Q][..., 2]
                        t = np.where(t > 0, t, 0.0)
                        for _ in range(nsq):
                            t = t * t
                        wgt = wgt * t
                    if sigma_depth > 0:
                        r = (z[Q] - z[P]) / (sigma_depth * z[P])
                        wgt = wgt / (1.0 + r * r)
                    if sigma_color > 0:
                        d = e64[Q] - e64[P]
                        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                        wgt = wgt / (1.0 + d2 / sc2)
                    sumw[P] = np.where(ok, sumw[P] + wgt, sumw[P])
                    sums[P] = np.where(ok[..., None], sums[P] + wgt[..., None] * e64[Q], sums[P])
            new = (sums / sumw[..., None]).astype(np.float32)
            e = np.where((valid & (sumw > 0))[..., None], new, e)
        out = (e.astype(np.float64) * floor).astype(np.float32) if demod else e
    return np.where(valid[..., None], out, color)


@functools.lru_cache(maxsize=None)
def synthetic(w, h, seed=11, all_valid=False):
    """Seeded inputs, read-only: colour in [0, 2); albedo in [0, 1) with about 10 % exact zeros (they
    exercise amin); normals near +Z with jitter; depth in [1, 1.2] with about 15 % +Inf (none with
    all_valid); object ids 0, 1, 2 in blocks of 5 x 4 pixels, -1 where the pixel is not valid."""
    rng = np.random.default_rng(seed)
    color = (rng.random((h, w, 3)) * 2).astype(np.float32)
    albedo = rng.random((h, w, 3)).astype(np.float32)
    albedo[rng.random((h, w, 3)) < 0.1] = 0
    nrm = np.array([0.0, 0.0, 1.0]) + 0.6 * (rng.random((h, w, 3)) - 0.5)
    normal = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    depth = (1 + 0.2 * rng.random((h, w))).astype(np.float32)
    invalid = (rng.random((h, w)) < 0.15) & (not all_valid)
    depth[invalid] = np.inf
    yy, xx = np.mgrid[0:h, 0:w]
    obj = ((xx // 5 + yy // 4) % 3).astype(np.int32)
    obj[invalid] = -1
    out = dict(color=color, albedo=albedo, normal=normal, depth=depth, object=obj)
    for a in out.values():
        a.flags.writeable = False
    return out


# The cases the host function and the kernels are both held to.  33 x 17 leaves a partial wave in
# every row and a partial block of rows; 70 x 5 spans two waves per row, the second cut at the image
# edge, and its steps (up to 128) reach past the image in both directions; 1 x 1 has only its centre tap.
BASE = dict(w=33, h=17, params=dict(levels=3))
CASES = {
    "33x17 levels 3": BASE,
    "1x1": dict(w=1, h=1, all_valid=True, params={}),
    "70x5 levels 8": dict(w=70, h=5, params=dict(levels=8)),
    "normal_power 0": dict(BASE, params=dict(levels=3, normal_power=0)),
    "sigma_depth 0": dict(BASE, params=dict(levels=3, sigma_depth=0.0)),
    "sigma_color 0": dict(BASE, params=dict(levels=3, sigma_color=0.0)),
    "demodulate 0": dict(BASE, params=dict(levels=3, demodulate=0)),
    "albedo NULL": dict(BASE, drop=("albedo",)),
    "object NULL": dict(BASE, drop=("object",)),
}
MECHANISMS = ["normal_power 0", "sigma_depth 0", "sigma_color 0", "demodulate 0", "albedo NULL", "object NULL"]


def case_inputs(name):
    """(inputs with None for the buffers the case does not give, the rt_denoise fields it sets)."""
    c = CASES[name]
    inp = dict(synthetic(c["w"], c["h"], all_valid=c.get("all_valid", False)))
    for k in c.get("drop", ()):
        inp[k] = None
    return inp, dict(c["params"])


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """The case's reference output, computed once, read-only, and checked to be finite."""
    inp, params = case_inputs(name)
    out = reference(inp["color"], inp["normal"], inp["depth"], inp["albedo"], inp["object"], **params)
    assert np.isfinite(out).all(), name
    out.flags.writeable = False
    return out


def bits(a):
    """The bit patterns of a float32 (or integer) array, for exact comparison (NaN-safe)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
