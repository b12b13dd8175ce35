"""GPU: the opt-in look-at camera (rt_settings.camera = RT_CAMERA_LOOKAT,
DESIGN.md §4.9) in every device path that generates or culls camera rays.

The oracle knows only the reference camera (getRay, renderer.go:377-390) and
is always called with camera = 0.  The checks are built around that:

1. an IDENTITY look-at camera (looking down -Z, up +Y, fov 90) shoots the
   reference's rays bit for bit, so its render equals the oracle's, byte for
   byte, on the block kernel, the stream kernel, the wavefront path, with
   triangles, packed shares, batched frames and a progression;
2. a HALF-TURNED look-at camera on scene S equals the oracle's reference
   render of S turned the same way (sign flips are exact in binary64 and a
   dot product keeps its term order), pixel for pixel;
3. an ARBITRARY orientation against an independent numpy model of primary
   visibility (which sphere each jittered camera ray sees);
4. with full shading in that orientation, every path, partition and way of
   launching equals the plain block kernel byte for byte, and the oriented
   primary-ray culling culls only samples that miss;
5. one context switches between the models and builds a new schedule.

A BVH takes sphere-only scenes (rt_context_set_scene refuses force_bvh = 1
with cubes), so the force_bvh cases use the all-materials scene without its
two cubes, as tests/test_gpu_wavefront.py does, against that scene's own
oracle image / block-kernel baseline.  Every case is at most 75x50 pixels and
8 samples; oracle images and baselines are computed once and shared.
"""
import copy
import functools
import json
import os

import numpy as np
import pytest

import oracle
import rng_spec
import rtgo
from conftest import SCENES
from gpu_util import render_dev, unpack_dev
from scene_cases import ALL_MATERIALS, make_settings

pytestmark = pytest.mark.gpu

REF, LOOKAT = rtgo.RT_CAMERA_REFERENCE, rtgo.RT_CAMERA_LOOKAT
GENERAL = {"position": [3, 2, -5], "lookAt": [0.5, 0, 0.25], "up": [0.1, 1, 0.2], "fov": 50, "aspectRatio": 4 / 3}
BLOCK = {"stream": 0}  # the block kernel (one-frame launches take it by default; said explicitly)


def _spheres_only(d):
    d = copy.deepcopy(d)
    d["objects"] = [o for o in d["objects"] if o["type"] == "sphere"]
    return d


def _identity(d):
    """d seen through a look-at camera that is the reference camera."""
    d = copy.deepcopy(d)
    p = np.array(d["camera"]["position"], np.float64)
    la = p + np.array([0, 0, -1.0])
    assert np.array_equal(p - la, np.array([0, 0, 1.0]))
    d["camera"].update(lookAt=la.tolist(), up=[0, 1, 0], fov=90)
    return d


def _with_camera(d, cam):
    d = copy.deepcopy(d)
    d["camera"] = dict(cam)
    return d


@functools.lru_cache(maxsize=None)
def _scene(name):
    silver = json.load(open(os.path.join(SCENES, "final_silver_prism_purple_cube_facing.json")))
    d = {
        "allm_identity": lambda: _identity(ALL_MATERIALS),
        "allm_spheres_identity": lambda: _identity(_spheres_only(ALL_MATERIALS)),
        "silver_identity": lambda: _identity(silver),
        "allm_general": lambda: _with_camera(ALL_MATERIALS, GENERAL),
        "allm_spheres_general": lambda: _with_camera(_spheres_only(ALL_MATERIALS), GENERAL),
        "rgb_general": lambda: RGB_SCENE,
    }[name]()
    return rtgo.Scene.from_json_text(json.dumps(d))


def _settings(over, seed, camera):
    st = make_settings(rtgo, dict(over), seed)
    st.camera = camera
    return st


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, over, seed):
    """The oracle's (float32 linear, RGBA8) of the scene under the REFERENCE camera."""
    lin, rgba, _ = oracle.render(_scene(name), w, h, _settings(over, seed, REF))
    return lin.astype(np.float32), rgba


def _render(scene, w, h, st, tun=None, force_bvh=0):
    lin, rgba, _, _ = render_dev(scene, w, h, st, tuning=rtgo.default_tuning(**(tun or {})), force_bvh=force_bvh)
    return lin.reshape(h, w, 3), rgba.reshape(h, w, 4)


def _same(got, want, what=""):
    assert got[0].tobytes() == want[0].tobytes(), what
    assert got[1].tobytes() == want[1].tobytes(), what


class _Ctx:
    """One rt_context with image buffers of its own."""

    def __init__(self, scene, w, h, tun=None, force_bvh=0, frames=1):
        import torch

        self.w, self.h = w, h
        self.ctx = rtgo.Context(0)
        if tun is not None:
            self.ctx.set_tuning(rtgo.default_tuning(**tun))
        self.ctx.set_scene(scene, force_bvh=force_bvh)
        self.lin = [torch.full((w * h * 3,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(frames)]
        self.rgba = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(frames)]

    def image(self, f=0):
        import torch

        torch.cuda.synchronize()
        return (self.lin[f].cpu().numpy().reshape(self.h, self.w, 3),
                self.rgba[f].cpu().numpy().reshape(self.h, self.w, 4))

    def render(self, st):
        self.ctx.render_async(self.w, self.h, st, self.lin[0].data_ptr(), self.rgba[0].data_ptr(), 0)
        return self.image()

    def frames(self, st, seeds):
        self.ctx.render_frames_async(self.w, self.h, st, seeds, [t.data_ptr() for t in self.lin],
                                     [t.data_ptr() for t in self.rgba], 0)
        return [self.image(f) for f in range(len(seeds))]

    def progression(self, st, adds):
        self.ctx.progressive_begin(self.w, self.h, st)
        out = []
        for n in adds:
            self.ctx.progressive_add(n, self.lin[0].data_ptr(), self.rgba[0].data_ptr(), 0)
            out.append(self.image())
        self.ctx.progressive_end()
        return out

    def close(self):
        self.ctx.close()


def _shares(scene, w, h, st, world, tun=None, balanced=False):
    """The frame rendered rank by rank as packed shares on device 0 and reassembled."""
    part = None
    if balanced:
        ctx = rtgo.Context(0)
        ctx.set_scene(scene)
        part = ctx.balanced_partition(w, h, st, world)
        ctx.close()
    t = rtgo.default_tuning(**(tun or {}))
    shares = [render_dev(scene, w, h, st, rank=r, world=world, tuning=t, partition=part)[2] for r in range(world)]
    return unpack_dev(w, h, world, shares, partition=part)


# ------------------------------------------------- 1. identity == the oracle
IDENTITY = [
    ("block", "allm_identity", 64, 48, 4, BLOCK, 0),
    ("stream", "allm_identity", 64, 48, 4, {"stream": 1}, 0),
    ("wavefront", "allm_spheres_identity", 64, 48, 4, None, 1),
    ("triangles", "silver_identity", 64, 48, 3, BLOCK, 0),
]


@pytest.mark.parametrize("name,scene,w,h,spp,tun,bvh", IDENTITY, ids=[c[0] for c in IDENTITY])
def test_identity_lookat_equals_the_oracle(name, scene, w, h, spp, tun, bvh):
    over = (("samples", spp),)
    got = _render(_scene(scene), w, h, _settings(over, 3, LOOKAT), tun, force_bvh=bvh)
    _same(got, _oracle(scene, w, h, over, 3), name)
    assert got[1][..., :3].any()
    if name == "stream":  # (the stream kernel did render it)
        c = _Ctx(_scene(scene), w, h, tun)
        _same(c.render(_settings(over, 3, LOOKAT)), got)
        assert c.ctx.stats()["stream_launches"] == 1
        c.close()


def test_identity_lookat_packed_shares_of_3_ranks():
    w, h, over = 75, 50, (("samples", 3),)
    got = _shares(_scene("allm_identity"), w, h, _settings(over, 5, LOOKAT), 3)
    _same(got, _oracle("allm_identity", w, h, over, 5))


def test_identity_lookat_batched_frames_and_a_progression():
    w, h = 64, 48
    c = _Ctx(_scene("allm_identity"), w, h, frames=2)
    two = c.frames(_settings((("samples", 4),), 3, LOOKAT), [3, 11])
    assert c.ctx.stats()["batched_launches"] == 1
    for img, seed in zip(two, (3, 11)):
        _same(img, _oracle("allm_identity", w, h, (("samples", 4),), seed), seed)
    after2, after4 = c.progression(_settings((("samples", 4),), 3, LOOKAT), [2, 2])
    c.close()
    _same(after2, _oracle("allm_identity", w, h, (("samples", 2),), 3))
    _same(after4, _oracle("allm_identity", w, h, (("samples", 4),), 3))


# ------------------------------------- 2. half-turns == the oracle of the turned scene
def _half_turn_scene(pos):
    """The committed sphere_reflections_light geometry with lambertian and
    diffuselight materials and two point lights (no random direction enters
    the radiance with soft shadows and recursion off)."""
    def sph(p, r, kind, col):
        return {"type": "sphere", "position": list(p), "radius": r, "material": {"type": kind, "color": col}}

    return {
        "camera": {"position": list(pos), "aspectRatio": 1.33},
        "objects": [sph((0, 0, 0), 1.0, "lambertian", [0.8, 0.8, 0.9]), sph((2, 0, 0), 0.5, "lambertian", [0.7, 0.3, 0.2]),
                    sph((-2, 0, 0), 0.7, "diffuselight", [0.8, 0.2, 0.2]), sph((0, 2, 0), 0.3, "lambertian", [0.9, 0.9, 0.1]),
                    sph((0, -2, 0), 0.4, "diffuselight", [0.2, 0.8, 0.2])],
        "lights": [{"type": "point", "position": [5, 5, 5], "color": [1, 1, 1], "intensity": 30.0},
                   {"type": "point", "position": [-3, 3, -6], "color": [0.8, 0.8, 1], "intensity": 15.0}],
    }


def _turned(d, flip):
    d = copy.deepcopy(d)
    f = np.array(flip, np.float64)
    for o in d["objects"] + d["lights"] + [d["camera"]]:
        o["position"] = (np.array(o["position"], np.float64) * f).tolist()
    return d


# (id, camera position, looking down dz, up dy, the coordinates the turn negates)
HALF_TURNS = [("plusZ_upY", (0, 0, -8), +1, +1, (-1, 1, -1)), ("minusZ_downY", (0, 0, 8), -1, -1, (-1, -1, 1)),
              ("plusZ_downY", (0, 0, -8), +1, -1, (1, -1, -1))]
HT_OVER = (("samples", 4), ("soft_shadows", 0), ("recursive_reflections", 0))


@pytest.mark.parametrize("bvh", [0, 1], ids=["block", "wavefront"])
@pytest.mark.parametrize("name,pos,dz,uy,flip", HALF_TURNS, ids=[t[0] for t in HALF_TURNS])
def test_half_turn_equals_the_oracle_of_the_turned_scene(name, pos, dz, uy, flip, bvh):
    w, h = 64, 48
    S = _half_turn_scene(pos)
    S["camera"].update(lookAt=[pos[0], pos[1], pos[2] + dz], up=[0, uy, 0], fov=90)
    scene = rtgo.Scene.from_json_text(json.dumps(S))
    turned = rtgo.Scene.from_json_text(json.dumps(_turned(_half_turn_scene(pos), flip)))
    ref, ref_rgba, _ = oracle.render(turned, w, h, _settings(HT_OVER, 6, REF))
    assert ref_rgba[..., :3].any()
    got = _render(scene, w, h, _settings(HT_OVER, 6, LOOKAT), BLOCK if not bvh else None, force_bvh=bvh)
    assert np.array_equal(got[0], ref.astype(np.float32))
    assert got[1].tobytes() == ref_rgba.tobytes()
    if dz > 0:  # the committed camera: behind the scene for getRay's fixed -Z view
        black = _render(scene, w, h, _settings(HT_OVER, 6, REF), BLOCK if not bvh else None, force_bvh=bvh)
        assert not black[0].any() and not black[1][..., :3].any()
        assert got[0].any()


# -------------------- 3. arbitrary orientation == a numpy model of primary visibility
def _np_frame(cam, w, h):
    pos, la, up = (np.array(cam[k], np.float64) for k in ("position", "lookAt", "up"))
    wv = pos - la
    wv = wv / np.sqrt(wv @ wv)
    U = np.cross(up, wv)
    U = U / np.sqrt(U @ U)
    V = np.cross(wv, U)
    hh = np.tan(np.float64(cam["fov"]) * (np.pi / 360))
    hor, ver = U * (2.0 * hh * cam["aspectRatio"]), V * (2.0 * hh)
    return pos, pos - hor / 2 - ver / 2 - wv, hor, ver, (U, V, wv)


def _rgb_scene():
    """Three diffuselight spheres (pure red, green, blue; no lights) placed in
    the general camera's own axes so that all are in view and none overlap."""
    _, _, _, _, (U, V, wv) = _np_frame(GENERAL, 48, 36)
    c0 = np.array(GENERAL["lookAt"], np.float64)
    spheres = [(c0, 1.2, [1.5, 0, 0]), (c0 + 2.6 * U + 0.4 * V, 0.9, [0, 0.75, 0]),
               (c0 - 2.3 * U - 1.5 * V + 1.0 * wv, 0.6, [0, 0, 3.0])]
    return {"camera": dict(GENERAL), "lights": [],
            "objects": [{"type": "sphere", "position": [round(float(x), 3) for x in c], "radius": r,
                         "material": {"type": "diffuselight", "color": col}} for c, r, col in spheres]}


RGB_SCENE = _rgb_scene()
RGB_W, RGB_H, RGB_SPP, RGB_SEED = 48, 36, 4, 9


@functools.lru_cache(maxsize=None)
def _predicted_hits():
    """Per pixel and channel, the samples whose camera ray sees that sphere
    first: jitter from tests/rng_spec.py, the ray from the numpy frame, the
    spheres intersected analytically (Sphere.Hit's roots, t > 0.001)."""
    w, h, spp = RGB_W, RGB_H, RGB_SPP
    o, ll, hor, ver, _ = _np_frame(GENERAL, w, h)
    u = np.empty((h, w, spp))
    v = np.empty((h, w, spp))
    for y in range(h):
        for x in range(w):
            for s in range(spp):
                _, (a, b) = rng_spec.draws(RGB_SEED, y * w + x, s, 2)
                u[y, x, s] = (x + a) / w
                v[y, x, s] = (y + b) / h
    d = ((ll + hor * u[..., None]) + ver * v[..., None]) - o
    best = np.full((h, w, spp), np.inf)
    who = np.full((h, w, spp), -1)
    for i, ob in enumerate(RGB_SCENE["objects"]):
        oc = o - np.array(ob["position"], np.float64)
        a = (d * d).sum(-1)
        hb = (d * oc).sum(-1)
        cc = oc @ oc - ob["radius"] ** 2
        disc = hb * hb - a * cc
        # the guard: no sample close enough to a silhouette for rounding to decide it
        assert (np.abs(disc) > 1e-9 * (hb * hb + np.abs(a * cc))).all(), "a sample grazes a sphere: pick another seed"
        sq = np.sqrt(np.maximum(disc, 0))
        for root in ((-hb - sq) / a, (-hb + sq) / a):  # nearest acceptable root (the camera is outside every sphere)
            assert (np.abs(root[disc > 0] - 0.001) > 1e-9).all(), "a hit at the near bound: pick another seed"
            ok = (disc > 0) & (root > 0.001) & (root < best)
            best = np.where(ok, root, best)
            who = np.where(ok, i, who)
    return np.stack([(who == i).sum(-1) for i in range(3)], -1)


RGB_VARIANTS = [("frustum", {"frustum": 1}, 0), ("no_frustum", {"frustum": 0}, 0), ("unstaged", {"stage": 0}, 0),
                ("stream", {"stream": 1}, 0), ("wavefront", None, 1)]


@pytest.mark.parametrize("name,tun,bvh", RGB_VARIANTS, ids=[v[0] for v in RGB_VARIANTS])
def test_general_orientation_sees_what_the_numpy_model_sees(name, tun, bvh):
    """A hit on sphere c returns its emission in channel c and, in every
    channel, the renderer's constant ambient term (calculateDirectLighting adds
    it whatever the albedo), so channel c of a pixel is (n_c E_c + n_other A_c)
    / samples: E_c and A_c are read off pixels the model says lie wholly inside
    sphere c / another sphere, and the sample count the image implies for
    sphere c must be the predicted one within 1e-5."""
    want = _predicted_hits()
    lin, rgba = _render(_scene("rgb_general"), RGB_W, RGB_H, _settings((("samples", RGB_SPP),), RGB_SEED, LOOKAT), tun,
                        force_bvh=bvh)
    full = [np.argwhere(want[..., c] == RGB_SPP) for c in range(3)]
    for c in range(3):
        assert len(full[c]) > 0, f"no pixel lies wholly inside sphere {c}"
    assert not lin[want.sum(-1) == 0].any()  # no sample sees anything there: black
    for c in range(3):
        e_c = float(lin[full[c][0][0], full[c][0][1], c])
        a_c = [float(lin[full[k][0][0], full[k][0][1], c]) for k in range(3) if k != c]
        assert e_c > a_c[0] == a_c[1] >= 0
        n_other = want.sum(-1) - want[..., c]
        counts = (lin[..., c].astype(np.float64) * RGB_SPP - n_other * a_c[0]) / e_c
        print(name, "channel", c, "emission + ambient", e_c, "ambient", a_c[0], "samples seen", int(want[..., c].sum()),
              "largest deviation", float(np.abs(counts - want[..., c]).max()))
        assert np.abs(counts - want[..., c]).max() < 1e-5
    assert 0 < (want.sum(-1) > 0).sum() < RGB_W * RGB_H  # some pixels see nothing at all: culling has work


# ------------------------------- 4. every path agrees in a general orientation
SIZES = [(37, 29, 3), (64, 48, 4)]


@functools.lru_cache(maxsize=None)
def _baseline(name, w, h, spp, bvh=0):
    """The block kernel with no culling, staging or streaming."""
    return _render(_scene(name), w, h, _settings((("samples", spp),), 4, LOOKAT),
                   {"frustum": 0, "stage": 0, "stream": 0}, force_bvh=-1 if bvh else 0)


TUNINGS = [("defaults", None), ("stream", {"stream": 1}), ("tail_helpers", {"tail_helpers": 64})]


@pytest.mark.parametrize("w,h,spp", SIZES, ids=["37x29x3", "64x48x4"])
@pytest.mark.parametrize("name,tun", TUNINGS, ids=[t[0] for t in TUNINGS])
def test_general_orientation_tunings_equal_the_block_kernel(name, tun, w, h, spp):
    base = _baseline("allm_general", w, h, spp)
    assert base[1][..., :3].any()
    _same(_render(_scene("allm_general"), w, h, _settings((("samples", spp),), 4, LOOKAT), tun), base, name)


@pytest.mark.parametrize("w,h,spp", SIZES, ids=["37x29x3", "64x48x4"])
@pytest.mark.parametrize("name,tun", [("megakernel_bvh", {"path": rtgo.RT_PATH_MEGAKERNEL}), ("wavefront", None)])
def test_general_orientation_bvh_paths_equal_the_block_kernel(name, tun, w, h, spp):
    base = _baseline("allm_spheres_general", w, h, spp, bvh=1)
    assert base[1][..., :3].any()
    got = _render(_scene("allm_spheres_general"), w, h, _settings((("samples", spp),), 4, LOOKAT), tun, force_bvh=1)
    _same(got, base, name)


@pytest.mark.parametrize("w,h,spp", SIZES, ids=["37x29x3", "64x48x4"])
def test_general_orientation_partitions_and_the_renderer(w, h, spp):
    base = _baseline("allm_general", w, h, spp)
    scene, st = _scene("allm_general"), _settings((("samples", spp),), 4, LOOKAT)
    _same(_shares(scene, w, h, st, 3), base, "strided")
    _same(_shares(scene, w, h, st, 3, balanced=True), base, "balanced")
    r = rtgo.ParallelRenderer(devices=[0, 0, 0])
    st3 = _settings((("samples", spp),), 4, LOOKAT)
    st3.num_devices = 3
    r.settings = st3
    rgba = r.render(scene, w, h)
    lin = r.last_linear.copy()
    r.close()
    _same((lin, rgba), base, "rt_renderer, 3 ranks on device 0")


def test_general_orientation_progression_and_batched_frames():
    w, h, spp = 37, 29, 3
    base = _baseline("allm_general", w, h, spp)
    c = _Ctx(_scene("allm_general"), w, h, frames=2)
    st = _settings((("samples", spp),), 4, LOOKAT)
    _, after3 = c.progression(st, [1, 2])
    _same(after3, base, "1 + 2 samples")
    two = c.frames(st, [4, 17])
    assert c.ctx.stats()["batched_launches"] == 1
    _same(two[0], base, "frame 0 of the batch")
    own = c.render(_settings((("samples", spp),), 17, LOOKAT))
    c.close()
    _same(two[1], own, "frame 1 of the batch against its own render")


def test_general_orientation_culling_culls_only_misses():
    """The counting variant walks every camera sample and reports the culled
    ones apart: they must all be misses (no culled sample is shaded), there
    must be some in this view (the sky above the horizon), they cannot
    outnumber the samples that hit nothing, and the image with culling is the
    image without."""
    w, h, spp = 64, 48, 4
    scene, st = _scene("allm_general"), _settings((("samples", spp),), 4, LOOKAT)

    def counted(tun, over=()):
        s = _settings((("samples", spp),) + over, 4, LOOKAT)
        lin, rgba, _, c = render_dev(scene, w, h, s, tuning=rtgo.default_tuning(**tun), count="full")
        return (lin.reshape(h, w, 3), rgba.reshape(h, w, 4)), c

    img1, c1 = counted({"frustum": 1})
    img0, c0 = counted({"frustum": 0})
    _same(img1, img0)
    _same(img1, _baseline("allm_general", w, h, spp))
    # the reference's path counts do not depend on the culling
    for k in ("camera_rays", "bounce_rays", "shade_events", "light_evals"):
        assert getattr(c1, k) == getattr(c0, k), k
    cull = c1.culled_dict()
    assert c0.culled_dict()["camera_rays"] == 0
    assert 0 < cull["camera_rays"] < c1.camera_rays == w * h * spp
    assert cull["shade_events"] == cull["light_evals"] == 0
    assert c1.executed_dict()["shade_events"] == c0.shade_events
    # one bounce at most: every closest-hit query is a camera ray, so the misses are countable
    _, d0 = counted({"frustum": 0}, (("max_depth", 1),))
    _, d1 = counted({"frustum": 1}, (("max_depth", 1),))
    misses = d0.camera_rays - d0.shade_events
    assert d0.bounce_rays == d0.camera_rays and 0 < misses < d0.camera_rays
    assert d1.culled_dict()["camera_rays"] == cull["camera_rays"] <= misses
    print("camera samples", c1.camera_rays, "misses", misses, "culled", cull["camera_rays"])


# ------------------------------------------------ 5. switching on one context
def test_switching_the_model_on_one_context_builds_a_new_schedule():
    w, h = 64, 48
    c = _Ctx(_scene("allm_general"), w, h)
    ref_st, la_st = _settings((("samples", 3),), 2, REF), _settings((("samples", 3),), 2, LOOKAT)
    first = c.render(ref_st)
    n1 = c.ctx.stats()["schedules_built"]
    second = c.render(la_st)
    n2 = c.ctx.stats()["schedules_built"]
    third = c.render(ref_st)
    n3 = c.ctx.stats()["schedules_built"]
    again = c.render(ref_st)
    assert c.ctx.stats()["schedules_built"] == n3  # (the same model again: the schedule is reused)
    c.close()
    _same(first, third)
    _same(third, again)
    assert n1 < n2 < n3
    assert first[0].tobytes() != second[0].tobytes()
    _same(first, _oracle("allm_general", w, h, (("samples", 3),), 2))  # reference mode ignores lookAt / up / fov


def test_a_degenerate_camera_is_refused_by_the_render_entry_points():
    bad = _with_camera(ALL_MATERIALS, dict(GENERAL, up=[0, 0, 0]))
    c = _Ctx(rtgo.Scene.from_json_text(json.dumps(bad)), 32, 24)
    with pytest.raises(rtgo.RenderError, match="camera"):
        c.render(_settings((("samples", 1),), 1, LOOKAT))
    with pytest.raises(rtgo.RenderError, match="camera"):
        c.ctx.progressive_begin(32, 24, _settings((("samples", 2),), 1, LOOKAT))
    with pytest.raises(rtgo.RenderError, match="camera"):
        c.frames(_settings((("samples", 1),), 1, LOOKAT), [1])
    assert c.render(_settings((("samples", 1),), 1, REF))[1][..., 3].all()  # the reference model reads none of it
    c.close()
