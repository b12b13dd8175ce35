"""CPU: the shadow-cone rows (rt_scene_cone_rows, scene_flat.cpp cone_rows).

A row of (light, hit sphere) has to be a SUPERSET of what the kernels' cone
test (rt_shadow.h in_cone) can admit for any hit point on that sphere under
that light: the spheres-only stream kernels test only the spheres of the row,
and their candidate mask stays what it was only while that holds.  Here
in_cone is restated in binary64 with its two binary32 roots taken 2e-7 wide
both ways, and run over random hit points P within 1e-9 (relative) of the
surface, on both faces; every sphere it admits must have its bit set.  The
headline scene's rows are pinned exactly, so margins cannot grow until every
row is full and the test passes for nothing.
"""
import copy
import json
import os

import numpy as np
import pytest

import rtgo
from degenerate_cases import INF, NAN
from scene_cases import EDGE_SCENES, SCENES

LAMB = {"type": "lambertian", "color": [0.6, 0.5, 0.4]}
CAM = {"position": [0, 0.5, 6], "aspectRatio": 1.5}
POINTS_PER_FAMILY = 100_000
FULL = np.uint64(0xFFFFFFFFFFFFFFFF)


def _sph(p, r):
    return {"type": "sphere", "position": [float(x) for x in p], "radius": float(r), "material": LAMB}


def _light(p):
    return {"position": [float(x) for x in p], "color": [1, 1, 1], "intensity": 10.0}


def _scene(objects, lights, camera=None):
    return {"camera": copy.deepcopy(camera or CAM), "objects": objects, "lights": lights}


def _rows(sc, force_bvh=0):
    return rtgo.cone_rows(rtgo.Scene.from_python(sc["camera"], sc["objects"], sc["lights"]), force_bvh)


def _headline():
    return json.load(open(os.path.join(SCENES, "sphere_reflections_light_facing.json")))


def _spheres_only(sc):
    sc = copy.deepcopy(sc)
    sc["objects"] = [o for o in sc["objects"] if o["type"] == "sphere"]
    return sc


# ------------------------------------------------------------ in_cone, restated
def _admitted(C, R, P, L):
    """in_cone for hit points P (K, 3) under light L against spheres (C, R):
    (K, n) bool, true where ANY choice of the two roots within 2e-7 admits."""
    lv = L[None, :] - P
    ldist = np.sqrt((lv * lv).sum(1))
    lit = ~(ldist < 0.001)
    with np.errstate(divide="ignore", invalid="ignore"):
        ldir = np.where(ldist[:, None] == 0, 0.0, lv / ldist[:, None])
    v = C[None, :, :] - P[:, None, :]
    dc2 = (v * v).sum(2)
    vl = (v * ldir[:, None, :]).sum(2)
    out = np.zeros(dc2.shape, bool)
    for e1 in (1 - 2e-7, 1 + 2e-7):
        dc = np.sqrt(dc2) * e1
        ra = np.abs(R)[None, :] * (1.0 + 1e-5) + 1e-5 * dc + 1e-12
        inside = ~(dc > ra)
        beyond = dc - ra > (ldist * (1.0 + 1e-5) + 1e-9)[:, None]
        for e2 in (1 - 2e-7, 1 + 2e-7):
            tl = np.sqrt(np.maximum(dc2 - ra * ra, 0.0)) * e2
            meets = ~(vl < 0.99498 * tl - 0.1 * ra - 1e-5 * dc)
            out |= inside | (~beyond & meets)
    return out & lit[:, None]


def _hit_points(rng, c, r, toward, k):
    """k points within 1e-9 relative of the sphere (c, |r|), both faces: half
    uniform, half around the directions `toward` (the light, the other spheres:
    where a row's boundary is decided)."""
    u = rng.normal(size=(k, 3))
    if len(toward):
        t = toward[rng.integers(len(toward), size=k // 2)] - c[None, :]
        n = np.linalg.norm(t, axis=1, keepdims=True)
        t = np.where(n > 0, t / np.where(n > 0, n, 1.0), 0.0)
        spread = 10.0 ** rng.uniform(-3, 0.3, size=(k // 2, 1))
        sign = np.where(rng.random((k // 2, 1)) < 0.25, -1.0, 1.0)
        u[: k // 2] = sign * t + spread * u[: k // 2]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    face = 1.0 + rng.uniform(-1e-9, 1e-9, size=(k, 1))
    return c[None, :] + abs(r) * face * u


def _check_superset(sc, rng, k):
    """Every (light, sphere) of a sphere-only scene with k hit points each;
    returns the points tested."""
    rows = _rows(sc)
    C = np.array([o["position"] for o in sc["objects"]], np.float64)
    R = np.array([o["radius"] for o in sc["objects"]], np.float64)
    Ls = np.array([l["position"] for l in sc["lights"]], np.float64).reshape(-1, 3)
    n = len(R)
    assert rows.shape == (len(Ls), n)
    done = 0
    for li, L in enumerate(Ls):
        for a in range(n):
            assert (int(rows[li, a]) >> a) & 1, ("own bit", li, a)
            P = _hit_points(rng, C[a], R[a], np.vstack([L[None, :], np.delete(C, a, 0)]), k)
            adm = _admitted(C, R, P, L).any(0)
            have = np.array([(int(rows[li, a]) >> b) & 1 for b in range(n)], bool)
            missing = np.nonzero(adm & ~have)[0]
            assert missing.size == 0, ("light %d, hit sphere %d: in_cone admits %s, row %#x"
                                       % (li, a, missing.tolist(), int(rows[li, a])))
            done += k
    return done


def _family(scenes, seed):
    rng = np.random.default_rng(seed)
    pairs = sum(len(s["objects"]) * len(s["lights"]) for s in scenes)
    k = max(64, -(-POINTS_PER_FAMILY // pairs))
    done = sum(_check_superset(s, rng, k) for s in scenes)
    assert done >= POINTS_PER_FAMILY


# ------------------------------------------------------------------ families
def _random_scenes(seed, count):
    """Sizes, radii and light positions over several orders of magnitude."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        scale = 10.0 ** rng.uniform(-3, 4)
        centre = rng.normal(size=3) * scale * 10.0 ** rng.uniform(-1, 2)
        n = int(rng.integers(2, 9))
        objs = [_sph(centre + rng.normal(size=3) * scale * 3, scale * 10.0 ** rng.uniform(-2.5, 0.5) * (-1 if j == 1 and i % 7 == 0 else 1))
                for j in range(n)]
        if i % 3 == 0:  # a ground sphere a thousand times the others
            objs.append(_sph(centre + np.array([0, -1000 * scale - scale, 0]), 1000 * scale))
        lights = [_light(centre + rng.normal(size=3) * scale * 10.0 ** rng.uniform(-0.5, 2)) for _ in range(int(rng.integers(1, 4)))]
        out.append(_scene(objs, lights, {"position": list(centre + np.array([0, 0, 6 * scale])), "aspectRatio": 1.5}))
    return out


def test_random_scenes():
    _family(_random_scenes(11, 60), 1)


def test_headline_superset():
    _family([_headline()], 2)


def test_headline_rows_are_exactly_the_derived_table():
    """The other spheres that can enter a cone, per (hit sphere, light), as
    derived for the headline scene, plus each sphere's own bit."""
    others = {0: ((), ()), 1: ((), (0,)), 2: ((0,), ()), 3: ((), ()), 4: ((0,), (0,))}
    rows = _rows(_headline())
    assert rows.shape == (2, 5)
    for a, per_light in others.items():
        for li, bs in enumerate(per_light):
            want = (1 << a) | sum(1 << b for b in bs)
            assert int(rows[li, a]) == want, (a, li, hex(int(rows[li, a])), hex(want))


def test_edge_scenes_without_their_cube():
    _family([_spheres_only(s) for s in EDGE_SCENES.values()], 3)


def test_lights_inside_spheres():
    rng = np.random.default_rng(5)
    scenes = []
    for i in range(12):
        objs = [_sph((0, -1001, 0), 1000), _sph((-1.5, 0, 0), 1.0), _sph((1.2, -0.2, 0.5), 0.8), _sph((0, 0.4, -2), 1.4)]
        inside = objs[1 + i % 3]
        c, r = np.array(inside["position"]), inside["radius"]
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        lights = [_light(c + d * r * f) for f in (0.0, 0.5, 0.998, 0.9999)][i % 4:][:2] + [_light((5, 8, 6))]
        scenes.append(_scene(objs, lights))
    _family(scenes, 6)


def test_intersecting_spheres():
    rng = np.random.default_rng(7)
    scenes = []
    for i in range(12):
        sep = [0.1, 0.5, 1.0, 1.5, 1.9, 1.999][i % 6]
        objs = [_sph((0, -1001, 0), 1000), _sph((-sep / 2, 0, 0), 1.0), _sph((sep / 2, 0.1 * (i % 2), 0), 1.0 - 0.3 * (i % 3)),
                _sph((0, 0.3, -3), 0.7)]
        lights = [_light(rng.normal(size=3) * 4 + np.array([0, 5, 2])), _light((0.0, 0.2, 0.0)), _light((-4, 2, 3))]
        scenes.append(_scene(objs, lights))
    _family(scenes, 8)


def test_a_sphere_nested_inside_another():
    rng = np.random.default_rng(9)
    scenes = []
    for i in range(12):
        off = rng.normal(size=3) * 0.2
        inner_r = [0.05, 0.3, 0.7, 0.95][i % 4] * (1.0 - np.linalg.norm(off))
        objs = [_sph((0, -1001, 0), 1000), _sph((0, 0, 0), 1.0), _sph(off, inner_r), _sph((2.5, 0, 0), 0.8),
                _sph((0, 0, 0), 1.0)]  # and a concentric twin of the outer one
        lights = [_light((4, 6, 6)), _light(off * 0.5), _light((0.0, 1.002, 0.0))]
        scenes.append(_scene(objs[: 5 if i % 2 else 4], lights))
    _family(scenes, 10)


# -------------------------------------------------------------- full rows
@pytest.mark.parametrize("what", ["centre_nan", "centre_inf", "radius_nan", "radius_inf", "light_nan", "light_inf"])
def test_non_finite_scenes_get_full_rows(what):
    sc = _headline()
    bad = NAN if what.endswith("nan") else INF
    if what.startswith("centre"):
        sc["objects"][2]["position"][1] = bad
    elif what.startswith("radius"):
        sc["objects"][3]["radius"] = bad
    else:
        sc["lights"][1]["position"][0] = bad
    rows = _rows(sc)
    assert rows.shape == (2, 5) and (rows == FULL).all(), rows


def test_cube_hittables_get_full_rows_and_bits_count_spheres():
    """Rows are indexed by hittable, bits by sphere: with a cube in front, the
    headline's spheres are hittables 1..5 and spheres 0..4."""
    sc = _headline()
    sc["objects"] = [{"type": "cube", "position": [8, 8, -20], "size": [0.5, 0.5, 0.5], "material": LAMB}] + sc["objects"]
    rows = _rows(sc)
    assert rows.shape == (2, 6)
    assert (rows[:, 0] == FULL).all()
    plain = _rows(_headline())
    assert (rows[:, 1:] == plain).all(), (rows, plain)


def test_scenes_without_masks_get_full_rows():
    sc = _headline()
    assert (_rows(sc, force_bvh=1) == FULL).all()      # a tree
    many = _scene([_sph((i % 10 - 4.5, i // 10 - 3, -3), 0.3) for i in range(65)], [_light((4, 6, 6))])
    assert (_rows(many) == FULL).all()                 # more than 64 spheres (a tree by default)
    assert (_rows(many, force_bvh=-1) == FULL).all()   # ... and scanned linearly


def test_capacity_is_checked():
    import ctypes

    s = rtgo.Scene.from_python(CAM, _headline()["objects"], _headline()["lights"])
    out = (ctypes.c_uint64 * 9)()
    assert rtgo.lib().rt_scene_cone_rows(ctypes.byref(s.view), 0, out, 9) != rtgo.RT_OK
    assert b"cone rows" in rtgo.lib().rt_last_error()
    assert rtgo.lib().rt_scene_cone_rows(ctypes.byref(s.view), 0, out, 10) == rtgo.RT_OK
