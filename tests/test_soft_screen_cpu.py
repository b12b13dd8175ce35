"""CPU: the screen in front of a soft shadow ray's exact test (rt_soft_screen).

The spheres-only stream kernels decide most soft shadow rays from the
unnormalised direction and a binary32 reciprocal length (rt_internal.h
soft_screen); rt_soft_screen runs that same function with a caller-given
reciprocal.  Whenever it is sure, its answer must be the boolean Sphere.Hit
(sphere.go:22-40) returns on the ray normalised as vector.go does -- restated
here in plain binary64 numpy, no fused operation -- with the reciprocal exact
and off by its documented bound (2e-7) in either direction.  It may leave at
most 1e-3 of the headline's cone rays undecided, so it cannot pass by deciding
nothing; NaN and infinities in any input are always undecided.
"""
import json
import os

import numpy as np
import pytest

import rtgo
from scene_cases import SCENES

IL_BOUND = 2e-7  # |il |u| - 1| the kernels' reciprocal stays within (rt_internal.h kSoftScreenIl)
TMIN = 0.001


def exact_hit(c, r, P, u, tmin, tmax):
    """Sphere.Hit's boolean on Ray{P, u.Normalize()} (vector.go: Length, then three divisions)."""
    c, P, u = (np.asarray(a, np.float64).reshape(-1, 3) for a in (c, P, u))
    r, tmin, tmax = (np.broadcast_to(np.asarray(a, np.float64), (c.shape[0],)) for a in (r, tmin, tmax))
    with np.errstate(all="ignore"):
        ln = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])
        safe = np.where(ln == 0, 1.0, ln)
        d = np.where((ln == 0)[:, None], 0.0, u / safe[:, None])
        oc = P - c
        a = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        hb = oc[:, 0] * d[:, 0] + oc[:, 1] * d[:, 1] + oc[:, 2] * d[:, 2]
        cc = (oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1] + oc[:, 2] * oc[:, 2]) - r * r
        disc = hb * hb - a * cc
        sq = np.sqrt(disc)
        r1 = (-hb - sq) / a
        r2 = (-hb + sq) / a
        out1 = (r1 < tmin) | (tmax < r1)
        out2 = (r2 < tmin) | (tmax < r2)
        return ~(disc < 0) & (~out1 | ~out2)


def inv_len(u):
    u = np.asarray(u, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return 1.0 / np.sqrt((u * u).sum(axis=1))


def check(c, r, P, u, tmax, tmin=TMIN):
    """Every sure answer equals the exact one, for the three reciprocals; returns the undecided share (exact il)."""
    c, P, u = (np.asarray(a, np.float64).reshape(-1, 3) for a in (c, P, u))
    n = c.shape[0]
    r = np.broadcast_to(np.asarray(r, np.float64), (n,))
    want = exact_hit(c, r, P, u, tmin, tmax)
    il = inv_len(u)
    shares = []
    for f in (1.0, 1.0 + IL_BOUND, 1.0 - IL_BOUND):
        got = rtgo.soft_screen(c, r * r, P, u, il * f, tmin, tmax)
        sure = got != rtgo.SOFT_UNDECIDED
        bad = sure & ((got == rtgo.SOFT_HIT) != want)
        assert not bad.any(), (f, int(bad.sum()), c[bad][:3], r[bad][:3], P[bad][:3], u[bad][:3], got[bad][:3])
        shares.append(1.0 - sure.mean())
    return shares


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def ball_points(rng, n):
    """n points of RandomVec3InUnitSphere's distribution (uniform in the unit ball)."""
    p = rng.uniform(-1, 1, (3 * n, 3))
    p = p[(p * p).sum(axis=1) < 1][:n]
    assert p.shape[0] == n
    return p


def nudge(x, k):
    """x moved by k ulps."""
    return (np.asarray(x, np.float64).view(np.int64) + np.int64(k)).view(np.float64)


def headline():
    sc = json.load(open(os.path.join(SCENES, "sphere_reflections_light_facing.json")))
    sph = [(np.array(o["position"], np.float64), float(o["radius"])) for o in sc["objects"]]
    lights = [np.array(lt["position"], np.float64) for lt in sc["lights"]]
    return sph, lights


def test_headline_cone_rays():
    """2.1 M cone rays: hit points on each headline sphere, towards each light, against each sphere."""
    sph, lights = headline()
    rng = np.random.default_rng(7)
    per = 42_000
    C, R, Ps, U, T = [], [], [], [], []
    for ca, ra in sph:
        for L in lights:
            P = ca + ra * unit(rng.normal(size=(per, 3)))
            lv = L - P
            ldist = np.sqrt((lv * lv).sum(axis=1))
            u = lv / ldist[:, None] + ball_points(rng, per) * 0.1
            for cb, rb in sph:
                C.append(np.broadcast_to(cb, (per, 3)))
                R.append(np.full(per, rb))
                Ps.append(P)
                U.append(u)
                T.append(ldist)
    C, R, Ps, U, T = np.concatenate(C), np.concatenate(R), np.concatenate(Ps), np.concatenate(U), np.concatenate(T)
    assert C.shape[0] >= 2_000_000
    shares = check(C, R, Ps, U, T)
    print("undecided share (il exact, +bound, -bound):", shares)
    assert max(shares) <= 1e-3, shares


def tangent_cases():
    """Rays tangent to a sphere, the direction nudged by ulps in one component."""
    rng = np.random.default_rng(11)
    C, R, Ps, U, T = [], [], [], [], []
    for _ in range(400):
        c = rng.uniform(-3, 3, 3)
        r = float(10 ** rng.uniform(-3, 1))
        dd = r * float(rng.uniform(1.05, 8))
        w = unit(rng.normal(size=3))           # P -> c
        P = c - dd * w
        e = unit(np.cross(w, rng.normal(size=3)))
        s = r / dd                              # sin of the tangent's angle with w
        t = (np.sqrt(1 - s * s) * w + s * e) * float(rng.uniform(0.9, 1.1))
        for k in (0, 1, -1, 2, -2, 16, -16, 2 ** 10, -2 ** 10, 2 ** 20, -2 ** 20, 2 ** 24, -2 ** 24, 2 ** 28, -2 ** 28,
                  2 ** 32, -2 ** 32):
            for ax in range(3):
                u = t.copy()
                u[ax] = nudge(u[ax], k)
                for tmax in (dd * 0.5, dd, dd * 3):
                    C.append(c), R.append(r), Ps.append(P), U.append(u), T.append(tmax)
    return C, R, Ps, U, T


def root_cases():
    """Roots at tmin and at tmax, a few ulps to either side; a sphere centred on the light."""
    rng = np.random.default_rng(13)
    C, R, Ps, U, T = [], [], [], [], []
    ks = (0, 1, -1, 2, -2, 3, -3, 8, -8, 64, -64, 2 ** 12, -2 ** 12, 2 ** 30, -2 ** 30)
    for _ in range(300):
        P = rng.uniform(-3, 3, 3)
        w = unit(rng.normal(size=3))
        u = w * float(rng.uniform(0.9, 1.1))
        tmax = float(rng.uniform(0.5, 9))
        r = float(10 ** rng.uniform(-3, 0))
        # first root at tmin; second root at tmin; first root at tmax; second root at tmax; centred on the light
        for dist in (TMIN + r, TMIN - r, tmax + r, tmax - r, tmax):
            for k in ks:
                c = P + nudge(dist, k) * w
                C.append(c), R.append(r), Ps.append(P), U.append(u), T.append(tmax)
    return C, R, Ps, U, T


def surface_cases():
    """P on the candidate's surface on both sides of the terminator, inside it, at its centre; radii 0 .. 1000."""
    rng = np.random.default_rng(17)
    C, R, Ps, U, T = [], [], [], [], []
    for r in (1.0, 0.3, 1e-3, 1000.0, 0.0, -0.5):
        for _ in range(60):
            c = rng.uniform(-2, 2, 3)
            n = unit(rng.normal(size=3))
            e = unit(np.cross(n, rng.normal(size=3)))
            for cs in (0.0, 1e-12, 1e-9, 1e-6, 1e-4, 1e-3, 4e-3, 1e-2, 0.1015, 0.5, 1.0):
                for sg in (1, -1):
                    u = (sg * cs * n + np.sqrt(1 - cs * cs) * e) * float(rng.uniform(0.9, 1.1))
                    for P in (c + r * n, c + abs(r) * n * float(rng.uniform(0, 1)), c.copy(),
                              c + r * n * (1 + 2e-3), c + r * n * (1 - 2e-3)):
                        for tmax in (0.05, 3.0, 2500.0):
                            C.append(c), R.append(r), Ps.append(P), U.append(u), T.append(tmax)
    return C, R, Ps, U, T


@pytest.mark.parametrize("cases", [tangent_cases, root_cases, surface_cases], ids=["tangent", "roots", "surface"])
def test_constructed_rays(cases):
    C, R, Ps, U, T = cases()
    shares = check(np.array(C), np.array(R), np.array(Ps), np.array(U), np.array(T))
    print(cases.__name__, len(R), "cases, undecided share", shares)


def test_random_scales():
    """Spheres, origins and intervals over many orders of magnitude, directions of length 0.9 .. 1.1."""
    rng = np.random.default_rng(19)
    n = 300_000
    c = rng.normal(size=(n, 3)) * 10 ** rng.uniform(-3, 3, (n, 1))
    r = 10 ** rng.uniform(-4, 3, n)
    P = c + rng.normal(size=(n, 3)) * (r * 10 ** rng.uniform(-1, 1, n))[:, None]
    u = unit(rng.normal(size=(n, 3))) * rng.uniform(0.9, 1.1, (n, 1))
    tmax = 10 ** rng.uniform(-3, 4, n)
    shares = check(c, r, P, u, tmax)
    print("undecided share", shares)
    assert min(shares) < 0.5  # (it decides most of these too)


def test_nan_and_infinity_are_undecided():
    base = dict(c=[0.3, 0.2, -4.0], r2=[0.49], P=[0.1, -0.2, 1.0], u=[0.02, 0.05, -0.99], il=[1.0], tmin=[TMIN], tmax=[9.0])
    base["il"] = [float(inv_len(base["u"])[0])]
    ok = rtgo.soft_screen(base["c"], base["r2"], base["P"], base["u"], base["il"], base["tmin"], base["tmax"])
    assert ok[0] == rtgo.SOFT_HIT  # the base case itself is decided
    for key, vals in base.items():
        for i in range(len(vals)):
            for bad in (np.nan, np.inf, -np.inf):
                a = {k: list(v) for k, v in base.items()}
                a[key][i] = bad
                got = rtgo.soft_screen(a["c"], a["r2"], a["P"], a["u"], a["il"], a["tmin"], a["tmax"])
                assert got[0] == rtgo.SOFT_UNDECIDED, (key, i, bad, got)
    # an empty interval (tmax < tmin), and a tmin in the underflow range, decide nothing
    assert rtgo.soft_screen(base["c"], base["r2"], base["P"], base["u"], base["il"], [2.0], [1.0])[0] == rtgo.SOFT_UNDECIDED
    assert rtgo.soft_screen(base["c"], base["r2"], base["P"], base["u"], base["il"], [1e-300], [9.0])[0] == rtgo.SOFT_UNDECIDED


def test_arguments():
    out = np.zeros(1, np.int32)
    assert rtgo.lib().rt_soft_screen(None, None, None, None, None, None, None, 1,
                                     out.ctypes.data_as(rtgo.ctypes.POINTER(rtgo.ctypes.c_int32))) != rtgo.RT_OK
    assert rtgo.soft_screen(np.zeros((0, 3)), [], np.zeros((0, 3)), np.zeros((0, 3)), [], [], []).shape == (0,)
