"""GPU: the shadow-cone rows do not change a bit.

The spheres-only stream kernels test, per (light, hit sphere), only the
spheres of that pair's row (rt_scene_cone_rows), which the host derives from
the scene alone.  While every row is a superset of what the cone test admits,
the candidate mask -- and with it every image -- is what it was.  Each case is
one batched launch of 2-3 seeds under the auto rule and with rt_tuning.stream
= 1, must have streamed (stream_launches == 1), and every image must equal the
oracle's byte for byte, float3 and RGBA8.  The scenes sit where a row could be
wrong: an occluder on either side of a row's boundary (its bit set / clear is
asserted, so the case means what it says), a light almost on a surface and one
inside a glass sphere, intersecting spheres, bit 63 and wide mode with four
lights, and the sphere-only edge scenes.
"""
import copy
import functools
import json
import os

import numpy as np
import pytest

import oracle
import rtgo
from scene_cases import EDGE_SCENES, SCENES, make_settings

pytestmark = pytest.mark.gpu

TUNINGS = [("auto", {}), ("forced", {"stream": 1})]
LAMB = {"type": "lambertian", "color": [0.6, 0.5, 0.4]}
RED = {"type": "lambertian", "color": [0.8, 0.2, 0.2]}
METAL = {"type": "metal", "color": [0.9, 0.8, 0.7], "roughness": 0.1}
GLASS = {"type": "glass", "color": [0.95, 0.95, 1.0], "refractionIndex": 1.5}
CAM = {"position": [0, 0.5, 6], "aspectRatio": 1.5}


def _sph(p, r, m):
    return {"type": "sphere", "position": list(p), "radius": r, "material": m}


def _headline():
    return json.load(open(os.path.join(SCENES, "sphere_reflections_light_facing.json")))


# ---- an occluder at the boundary of the row of (sphere 1, light 0)
# Sphere 1 (radius 1 at the origin) under a light 5 above it: its shadow rays
# fill a solid around the y axis.  The occluder (sphere 2, radius 0.3) sits at
# height 2.2 beside it, at distance x from the axis; its shadow on the ground
# (sphere 0) is in the frame whatever x is.
def _boundary_scene(x):
    return {"camera": copy.deepcopy(CAM),
            "objects": [_sph((0, -1001, 0), 1000, LAMB), _sph((0, 0, 0), 1.0, METAL), _sph((x, 2.2, 0.4), 0.3, RED)],
            "lights": [{"position": [0, 5, 0], "color": [1, 1, 1], "intensity": 40},
                       {"position": [-4, 3, 4], "color": [1, 0.9, 0.8], "intensity": 20}]}


def _bit(x):
    sc = _boundary_scene(x)
    rows = rtgo.cone_rows(rtgo.Scene.from_python(sc["camera"], sc["objects"], sc["lights"]))
    return (int(rows[0, 1]) >> 2) & 1


@functools.lru_cache(maxsize=None)
def _boundary():
    """(lo, hi): neighbouring x with the occluder's bit set at lo, clear at hi."""
    lo, hi = 0.3, 4.0
    assert _bit(lo) == 1 and _bit(hi) == 0
    while hi - lo > 1e-12:
        mid = 0.5 * (lo + hi)
        if _bit(mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


def _light_cases():
    """A light 2e-3 above the metal sphere, one inside the glass sphere."""
    return {"camera": copy.deepcopy(CAM),
            "objects": [_sph((0, -1001, 0), 1000, LAMB), _sph((0, 0, 0), 1, METAL), _sph((2.2, 0, 0), 0.9, GLASS),
                        _sph((-2.2, 0, 0), 0.9, LAMB)],
            "lights": [{"position": [0, 1.002, 0], "color": [1, 1, 1], "intensity": 2},
                       {"position": [2.3, 0.2, 0.1], "color": [1, 1, 1], "intensity": 3},
                       {"position": [4, 6, 6], "color": [1, 1, 1], "intensity": 40}]}


def _intersecting():
    return {"camera": copy.deepcopy(CAM),
            "objects": [_sph((0, -1001, 0), 1000, LAMB), _sph((-0.5, 0, 0), 1.0, METAL), _sph((0.6, 0.2, 0.3), 0.9, GLASS),
                        _sph((0.1, 0.9, 0.6), 0.5, RED), _sph((2.4, -0.3, 0.5), 0.7, LAMB)],
            "lights": [{"position": [4, 6, 6], "color": [1, 1, 1], "intensity": 40},
                       {"position": [-5, 3, 4], "color": [0.8, 0.8, 1], "intensity": 20}]}


def _sixty_four_four_lights():
    """64 spheres (bit 63; 16 or more reach wide mode) under four lights: an
    8 x 8 grid in two z layers in front of a large sphere 63."""
    mats = [METAL, {"type": "glass", "color": [0.8, 0.2, 0.2]}, LAMB,
            {"type": "metal", "color": [0.9, 0.9, 0.1], "roughness": 0.3}]
    objs = []
    for i in range(63):
        gx, gy = i % 8, i // 8
        objs.append(_sph((gx * 0.9 - 3.15, gy * 0.7 - 2.45, -0.8 * ((gx + gy) % 2)), 0.3 + 0.02 * (i % 5), mats[i % 4]))
    objs.append(_sph((0, 0, -9), 6.0, mats[0]))
    return {"camera": copy.deepcopy(CAM), "objects": objs,
            "lights": [{"position": [4, 6, 6], "color": [1, 1, 1], "intensity": 40},
                       {"position": [-5, 3, 4], "color": [0.8, 0.8, 1], "intensity": 20},
                       {"position": [0, 0.1, 1.5], "color": [1, 0.6, 0.6], "intensity": 3},
                       {"position": [0.45, -0.35, -0.4], "color": [0.6, 1, 0.6], "intensity": 2}]}


def _edge(name):
    sc = copy.deepcopy(EDGE_SCENES[name])
    sc["objects"] = [o for o in sc["objects"] if o["type"] == "sphere"]
    return sc


BUILDERS = {
    "headline": _headline,
    "occluder_well_inside": lambda: _boundary_scene(_boundary()[0] * 0.9),
    "occluder_inside_margin": lambda: _boundary_scene(_boundary()[0]),
    "occluder_outside_margin": lambda: _boundary_scene(_boundary()[1]),
    "occluder_well_outside": lambda: _boundary_scene(_boundary()[1] * 1.1),
    "lights_on_and_in": _light_cases,
    "intersecting": _intersecting,
    "sixty_four_four_lights": _sixty_four_four_lights,
    "edge_huge_ground": lambda: _edge("huge_ground"),
    "edge_far_coordinates": lambda: _edge("far_coordinates"),
    "edge_tiny_spheres": lambda: _edge("tiny_spheres"),
    "edge_light_on_surface": lambda: _edge("light_on_surface"),
}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return rtgo.Scene.from_json_text(json.dumps(BUILDERS[name]()))


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, over, seed):
    ref, ref_rgba, _ = oracle.render(_scene(name), w, h, make_settings(rtgo, dict(over), seed))
    return ref.astype(np.float32), ref_rgba


def _batched(name, w, h, over, seeds, tun):
    import torch

    n = len(seeds)
    lin = torch.full((n, w * h * 3), float("nan"), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((n, w * h * 4), dtype=torch.uint8, device="cuda")
    c = rtgo.Context(0)
    c.set_tuning(rtgo.default_tuning(**tun))
    c.set_scene(_scene(name))
    c.render_frames_async(w, h, make_settings(rtgo, over, 1), list(seeds), [lin[f].data_ptr() for f in range(n)],
                          [rgba[f].data_ptr() for f in range(n)], 0, 0, 1, rtgo.RT_LAYOUT_IMAGE)
    torch.cuda.synchronize()
    stats = c.stats()
    c.close()
    assert stats["stream_launches"] == 1, stats
    lin, rgba = lin.cpu().numpy().reshape(n, h, w, 3), rgba.cpu().numpy().reshape(n, h, w, 4)
    for f, seed in enumerate(seeds):
        ref, ref_rgba = _oracle(name, w, h, tuple(sorted(over.items())), seed)
        assert lin[f].tobytes() == ref.tobytes(), (name, seed)
        assert rgba[f].tobytes() == ref_rgba.tobytes(), (name, seed)


# (scene, width, height, settings, seeds)
CASES = [
    ("headline", 64, 48, {"samples": 8, "max_depth": 50}, (1, 2, 3)),
    ("occluder_well_inside", 56, 40, {"samples": 6, "max_depth": 50}, (1, 2)),
    ("occluder_inside_margin", 56, 40, {"samples": 6, "max_depth": 50}, (1, 2)),
    ("occluder_outside_margin", 56, 40, {"samples": 6, "max_depth": 50}, (1, 2)),
    ("occluder_well_outside", 56, 40, {"samples": 6, "max_depth": 50}, (1, 2)),
    ("lights_on_and_in", 64, 48, {"samples": 6, "max_depth": 50}, (2, 3)),
    ("intersecting", 64, 48, {"samples": 6, "max_depth": 50}, (3, 4)),
    ("sixty_four_four_lights", 64, 48, {"samples": 4, "max_depth": 50}, (1, 2)),
    ("edge_huge_ground", 56, 40, {"samples": 4, "max_depth": 50}, (1, 2)),
    ("edge_far_coordinates", 56, 40, {"samples": 4, "max_depth": 50}, (1, 2)),
    ("edge_tiny_spheres", 56, 40, {"samples": 4, "max_depth": 50}, (1, 2)),
    ("edge_light_on_surface", 56, 40, {"samples": 4, "max_depth": 50}, (1, 2)),
]


@pytest.mark.parametrize("tname,tun", TUNINGS, ids=[t[0] for t in TUNINGS])
@pytest.mark.parametrize("name,w,h,over,seeds", CASES, ids=[c[0] for c in CASES])
def test_rows_keep_every_image(name, w, h, over, seeds, tname, tun):
    _batched(name, w, h, over, seeds, tun)


def test_the_occluder_cases_sit_on_both_sides_of_the_row():
    """The four occluder scenes mean what their names say: the occluder's bit
    in the row of (sphere 1, light 0) is set up to the margin and clear beyond
    it, and the two margin scenes are neighbours (1e-12 apart)."""
    lo, hi = _boundary()
    assert hi - lo <= 1e-12
    assert [_bit(x) for x in (lo * 0.9, lo, hi, hi * 1.1)] == [1, 1, 0, 0]
    sc = _boundary_scene(hi)
    rows = rtgo.cone_rows(rtgo.Scene.from_python(sc["camera"], sc["objects"], sc["lights"]))
    # sphere 1 under light 0: itself and the ground it stands on, not the occluder
    assert int(rows[0, 1]) == 0b011, hex(int(rows[0, 1]))
    assert (int(rows[0, 0]) >> 2) & 1, "the ground must keep the occluder: its shadow is in the frame"
