"""Scenes of the specular-through feature-buffer tests.

S_MIRROR is S_CUBE (tests/sequence_cases.py: a roughness-0.2 metal sphere, a
Lambertian and a glass sphere, a roughness-0 metal cube) plus
  - a second roughness-0 metal cube, a wide slab lying under the scene: its
    top face (y = -0.85) faces the first cube's bottom face (y = -0.8) and
    shows every object from below, the first cube's mirror faces among them,
    so that chains of two and more reflections exist (slab -> cube ->
    ..., cube -> slab -> ...) and most of its own reflections leave the scene;
  - a perfectmirror sphere behind the first cube, standing over the slab
    (chains of three mirrors: the cap at max_bounces = 2);
  - a shiny sphere with roughness exactly 0.1, the default max_roughness.
The positions were fixed on the reference (tests/aov_spec_reference.py) alone:
at 72x48x4, seed 3, it has the pixels and samples that
test_gpu_aov_spec.py's conditions ask for.

FACING_CUBES / FACING_SPHERES: two mirrors facing each other along z with the
camera between them, far wider than any chain of 16 reflections drifts, so
every chain runs to the cap.  field70_mirrors: the 70-sphere field of
tests/mixed_cases.py with every third sphere a perfectmirror."""
import copy
import json

from mixed_cases import field70
from sequence_cases import S_CUBE

MIRROR0 = {"type": "metal", "color": [0.8, 0.9, 0.7], "roughness": 0.0, "metallic": 1.0}
PERFECT = {"type": "perfectmirror", "color": [0.9, 0.9, 0.95], "roughness": 0.0}
SHINY01 = {"type": "shiny", "color": [0.8, 0.3, 0.5], "roughness": 0.1, "metallic": 0.3, "specular": 0.8}

S_MIRROR = copy.deepcopy(S_CUBE)
S_MIRROR["objects"] += [
    {"type": "sphere", "position": [2.0, -0.4, -0.9], "radius": 0.6, "material": PERFECT},
    {"type": "cube", "position": [0, -1.0, 0], "size": [8, 0.3, 8], "material": MIRROR0},
    {"type": "sphere", "position": [-0.3, 1.1, 0.3], "radius": 0.35, "material": SHINY01},
]
# hittable indices in S_MIRROR
ROUGH_METAL_SPHERE, LAMBERTIAN_SPHERE, GLASS_SPHERE, CUBE_1, MIRROR_SPHERE, CUBE_2, SHINY_SPHERE = range(7)

_LIGHTS = copy.deepcopy(S_CUBE["lights"])
FACING_CUBES = {
    "camera": {"position": [0.3, 0.2, 0], "lookAt": [0, 0, -1], "up": [0, 1, 0], "fov": 60, "aspectRatio": 1.5},
    "objects": [
        {"type": "cube", "position": [0, 0, -3], "size": [400, 400, 1], "material": MIRROR0},
        {"type": "cube", "position": [0, 0, 3], "size": [400, 400, 1], "material": dict(MIRROR0, color=[0.9, 0.7, 0.8])},
    ],
    "lights": _LIGHTS,
}
FACING_SPHERES = {
    "camera": copy.deepcopy(FACING_CUBES["camera"]),
    "objects": [
        {"type": "sphere", "position": [0, 0, -1003], "radius": 1000, "material": PERFECT},
        {"type": "sphere", "position": [0, 0, 1003], "radius": 1000, "material": MIRROR0},
    ],
    "lights": _LIGHTS,
}


def field70_mirrors():
    sc = field70()
    spheres = [o for o in sc["objects"] if o["type"] == "sphere"]
    for o in spheres[::3]:
        o["material"] = copy.deepcopy(PERFECT)
    return sc


def text(scene, cam=None):
    d = copy.deepcopy(scene)
    if cam is not None:
        d["camera"] = dict(cam)
    return json.dumps(d)
