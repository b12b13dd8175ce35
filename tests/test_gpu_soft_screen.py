"""GPU: the soft-ray screen does not change a bit.

The spheres-only stream kernels decide a soft shadow ray from its unnormalised
direction wherever soft_screen (rt_internal.h) is sure, and run the exact test
only for the rays it leaves undecided.  Every image must stay what it was:
each case is one batched launch of 2-3 seeds at 96x64, depth 8, under the auto
rule and with rt_tuning.stream = 1, must have streamed (stream_launches == 1),
and every frame must equal the oracle's byte for byte, float3 and RGBA8.  The
scenes sit where the screen decides differently or not at all: two occluders
in one cone over a ground sphere (which mostly falls back: its radius is
1000), a light that grazes the sphere that fills the frame (the hit sphere is
its own candidate, and nearly every lane owns soft rays: the queue form), one
small far occluder over such a sphere (a few owners per wave: the cooperative
form), intersecting spheres, a light inside a glass sphere and one 2e-3 above
a surface, small spheres beside and around a light (roots at tmax), 1e-3
spheres 2e-3 above a surface (roots at tmin), and the sphere-only edge scenes;
a camera sequence and a progression's second add run the other two kernels.
"""
import copy
import functools
import json

import numpy as np
import pytest

import oracle
import rtgo
from scene_cases import EDGE_SCENES, make_settings, scene_path
from sequence_cases import POSITIONS, at, scene_json

pytestmark = pytest.mark.gpu

W, H = 96, 64
TUNINGS = [("auto", {}), ("forced", {"stream": 1})]
LAMB = {"type": "lambertian", "color": [0.6, 0.5, 0.4]}
RED = {"type": "lambertian", "color": [0.8, 0.2, 0.2]}
METAL = {"type": "metal", "color": [0.9, 0.8, 0.7], "roughness": 0.1}
GLASS = {"type": "glass", "color": [0.95, 0.95, 1.0], "refractionIndex": 1.5}
CAM = {"position": [0, 0.5, 6], "aspectRatio": 1.5}
NEAR = {"position": [0, 0, 3.2], "aspectRatio": 1.5}  # a radius-2.5 sphere at the origin fills its frame


def _sph(p, r, m):
    return {"type": "sphere", "position": [float(v) for v in p], "radius": r, "material": m}


def _light(p, i):
    return {"position": [float(v) for v in p], "color": [1, 1, 1], "intensity": i}


def _headline():
    return json.load(open(scene_path("sphere_reflections_light_facing.json")))


def _penumbra():
    """Two occluders whose penumbrae overlap on the ground sphere and cross the frame."""
    return {"camera": copy.deepcopy(CAM),
            "objects": [_sph((0, -1001, 0), 1000, LAMB), _sph((0, 0, 0), 1.0, METAL), _sph((0.9, 1.7, 0.4), 0.45, RED)],
            "lights": [_light((3, 6, 2), 60), _light((-4, 3, 4), 20)]}


def _grazing():
    """The sphere fills the frame and the first light lies close to the tangent plane of the cap the camera
    sees: N.L stays below 0.1015 over much of it, so the sphere is a candidate of its own soft rays."""
    return {"camera": copy.deepcopy(NEAR),
            "objects": [_sph((0, 0, 0), 2.5, LAMB), _sph((1.9, 0.3, 2.4), 0.25, RED)],
            "lights": [_light((9, 0.5, 2.7), 60), _light((-6, 2, 3.1), 30)]}


def _sparse():
    """The sphere fills the frame, lit from behind the camera; one small occluder behind the camera too: its
    penumbra covers a few pixels, so a wave has a few soft-ray owners at most."""
    return {"camera": copy.deepcopy(NEAR),
            "objects": [_sph((0, 0, 0), 2.5, LAMB), _sph((0.25, 0.15, 5.0), 0.06, RED)],
            "lights": [_light((0.5, 0.4, 9), 60)]}


def _intersecting():
    return {"camera": copy.deepcopy(CAM),
            "objects": [_sph((0, -1001, 0), 1000, LAMB), _sph((-0.5, 0, 0), 1.0, METAL), _sph((0.6, 0.2, 0.3), 0.9, GLASS),
                        _sph((0.1, 0.9, 0.6), 0.5, RED), _sph((2.4, -0.3, 0.5), 0.7, LAMB)],
            "lights": [_light((4, 6, 6), 40), _light((-5, 3, 4), 20)]}


def _lights_on_and_in():
    """A light 2e-3 above the metal sphere, one inside the glass sphere."""
    return {"camera": copy.deepcopy(CAM),
            "objects": [_sph((0, -1001, 0), 1000, LAMB), _sph((0, 0, 0), 1, METAL), _sph((2.2, 0, 0), 0.9, GLASS),
                        _sph((-2.2, 0, 0), 0.9, LAMB)],
            "lights": [_light((0, 1.002, 0), 2), _light((2.3, 0.2, 0.1), 3), _light((4, 6, 6), 40)]}


def _roots_at_tmax():
    """A 0.05 sphere 0.07 beside the first light (the hard ray mostly passes, soft rays end in it or just
    short of it) and one centred on the second light."""
    l0, l1 = (2.0, 4.0, 3.0), (-3.0, 3.0, 2.0)
    return {"camera": copy.deepcopy(CAM),
            "objects": [_sph((0, -1.0, 0), 1.0, LAMB), _sph((1.6, -0.5, 0.8), 0.5, METAL), _sph((-1.7, -0.4, 0.6), 0.6, LAMB),
                        _sph((l0[0] + 0.07, l0[1], l0[2]), 0.05, RED), _sph(l1, 0.05, RED)],
            "lights": [_light(l0, 40), _light(l1, 30)]}


def _roots_at_tmin():
    """Twenty 1e-3 spheres whose centres are 2e-3 above the unit sphere, over the cap that faces camera and light."""
    objs = [_sph((0, 0, 0), 1.0, LAMB)]
    for i in range(20):
        a, b = 0.25 * (i % 5) - 0.5, 0.25 * (i // 5) - 0.25
        n = np.array([a, b + 0.3, 1.0])
        n /= np.sqrt((n * n).sum())
        objs.append(_sph(n * 1.002, 1e-3, RED))
    return {"camera": {"position": [0, 0.3, 2.4], "aspectRatio": 1.5}, "objects": objs,
            "lights": [_light((1, 2, 6), 40), _light((-2, 1, 5), 20)]}


def _edge(name):
    sc = copy.deepcopy(EDGE_SCENES[name])
    sc["objects"] = [o for o in sc["objects"] if o["type"] == "sphere"]
    return sc


BUILDERS = {
    "headline": _headline,
    "penumbra_two_candidates": _penumbra,
    "grazing_light_queue_form": _grazing,
    "sparse_coop_form": _sparse,
    "intersecting": _intersecting,
    "lights_on_and_in": _lights_on_and_in,
    "roots_at_tmax": _roots_at_tmax,
    "roots_at_tmin": _roots_at_tmin,
    "edge_huge_ground": lambda: _edge("huge_ground"),
    "edge_far_coordinates": lambda: _edge("far_coordinates"),
    "edge_tiny_spheres": lambda: _edge("tiny_spheres"),
    "edge_light_on_surface": lambda: _edge("light_on_surface"),
}


@functools.lru_cache(maxsize=None)
def _scene(name, cam_key=None):
    if name == "S":
        return rtgo.Scene.from_json_text(scene_json("S", json.loads(cam_key) if cam_key else None))
    return rtgo.Scene.from_json_text(json.dumps(BUILDERS[name]()))


@functools.lru_cache(maxsize=None)
def _oracle(name, over, seed, cam_key=None):
    """The oracle's (float32 linear bytes, RGBA8 bytes), computed once."""
    ref, ref_rgba, _ = oracle.render(_scene(name, cam_key), W, H, make_settings(rtgo, dict(over), seed))
    return ref.astype(np.float32).tobytes(), ref_rgba.tobytes()


def _buffers(n):
    import torch

    lin = torch.full((n, W * H * 3), float("nan"), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((n, W * H * 4), dtype=torch.uint8, device="cuda")
    return lin, rgba


def _same(lin, rgba, f, want, what):
    assert lin[f].tobytes() == want[0], what
    assert rgba[f].tobytes() == want[1], what


def _context(name, tun):
    c = rtgo.Context(0)
    c.set_tuning(rtgo.default_tuning(**tun))
    c.set_scene(_scene(name))
    return c


# (scene, samples, seeds)
CASES = [
    ("headline", 8, (1, 2, 3)),
    ("penumbra_two_candidates", 6, (1, 2)),
    ("grazing_light_queue_form", 4, (1, 2)),
    ("sparse_coop_form", 4, (1, 2)),
    ("intersecting", 6, (3, 4)),
    ("lights_on_and_in", 6, (2, 3)),
    ("roots_at_tmax", 6, (1, 2)),
    ("roots_at_tmin", 8, (1, 2)),
    ("edge_huge_ground", 4, (1, 2)),
    ("edge_far_coordinates", 4, (1, 2)),
    ("edge_tiny_spheres", 4, (1, 2)),
    ("edge_light_on_surface", 4, (1, 2)),
]


@pytest.mark.parametrize("tname,tun", TUNINGS, ids=[t[0] for t in TUNINGS])
@pytest.mark.parametrize("name,spp,seeds", CASES, ids=[c[0] for c in CASES])
def test_screen_keeps_every_image(name, spp, seeds, tname, tun):
    import torch

    over = (("max_depth", 8), ("samples", spp))
    n = len(seeds)
    lin, rgba = _buffers(n)
    c = _context(name, tun)
    c.render_frames_async(W, H, make_settings(rtgo, dict(over), 1), list(seeds), [lin[f].data_ptr() for f in range(n)],
                          [rgba[f].data_ptr() for f in range(n)], 0, 0, 1, rtgo.RT_LAYOUT_IMAGE)
    torch.cuda.synchronize()
    stats = c.stats()
    c.close()
    assert stats["stream_launches"] == 1, stats
    lin, rgba = lin.cpu().numpy(), rgba.cpu().numpy()
    for f, seed in enumerate(seeds):
        _same(lin, rgba, f, _oracle(name, over, seed), (name, seed))


@pytest.mark.parametrize("tname,tun", TUNINGS, ids=[t[0] for t in TUNINGS])
def test_camera_sequence_kernel(tname, tun):
    """Three frames, each from a camera of its own: the `cams` kernel."""
    import torch

    over, seed = (("max_depth", 8), ("samples", 4)), 3
    cams = [at(p) for p in POSITIONS[:3]]
    lin, rgba = _buffers(3)
    c = _context("S", tun)
    c.render_cameras_async(W, H, make_settings(rtgo, dict(over), seed), cams, [lin[f].data_ptr() for f in range(3)],
                           [rgba[f].data_ptr() for f in range(3)])
    torch.cuda.synchronize()
    stats = c.stats()
    c.close()
    assert stats["stream_launches"] == 1, stats
    lin, rgba = lin.cpu().numpy(), rgba.cpu().numpy()
    for f, cam in enumerate(cams):
        _same(lin, rgba, f, _oracle("S", over, seed, json.dumps(cam, sort_keys=True)), (tname, f))


def test_sample_base_kernel():
    """Adds of 3 and 5 samples: the second add's entries carry sample_base = 3 (the `base` kernel); the
    image after it is the 8-sample one."""
    import torch

    over = (("max_depth", 8), ("samples", 8))
    c = _context("headline", {"stream": 1})
    lin, rgba = _buffers(1)
    c.progressive_begin(W, H, make_settings(rtgo, dict(over), 2))
    for n in (3, 5):
        c.progressive_add(n, lin[0].data_ptr(), rgba[0].data_ptr(), 0)
    torch.cuda.synchronize()
    assert c.progressive_samples() == 8
    c.progressive_end()
    stats = c.stats()
    c.close()
    assert stats["stream_launches"] == 2, stats
    _same(lin.cpu().numpy(), rgba.cpu().numpy(), 0, _oracle("headline", over, 2), "progression")
