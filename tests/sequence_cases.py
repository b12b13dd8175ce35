"""Scenes and cameras of the camera-sequence tests.

Scene S: three spheres, no ground, the two strong lights of ALL_MATERIALS;
S_CUBE adds a metal cube.  POSITIONS are five camera positions for the
reference camera (which looks down -Z whatever lookAt says): the fourth,
(0, 0, -10), looks away from everything, so its frame is all black, and the
others see different parts of the scene -- a sequence over them holds pixels
that are live for one frame only, and a frame in which every pixel of the
union misses.  At 72x48x4, seed 3, the oracle's nonzero pixels per frame are
ORACLE_NONZERO (the union: ORACLE_UNION of 3456)."""
import copy
import json

from scene_cases import ALL_MATERIALS

S = {
    "camera": {"position": [0, 0, 3], "lookAt": [0, 0, 0], "up": [0, 1, 0], "fov": 60, "aspectRatio": 1.5},
    "objects": [
        {"type": "sphere", "position": [-1.2, 0, 0], "radius": 0.8,
         "material": {"type": "metal", "color": [0.9, 0.6, 0.3], "roughness": 0.2, "metallic": 0.85, "specular": 0.7}},
        {"type": "sphere", "position": [0.9, 0.2, -0.5], "radius": 0.7,
         "material": {"type": "lambertian", "color": [0.3, 0.3, 0.9]}},
        {"type": "sphere", "position": [0.1, -0.6, 1.0], "radius": 0.4,
         "material": {"type": "glass", "color": [0.9, 0.95, 1.0], "refractionIndex": 1.5}},
    ],
    "lights": copy.deepcopy(ALL_MATERIALS["lights"][:2]),
}
S_CUBE = copy.deepcopy(S)
S_CUBE["objects"].append({"type": "cube", "position": [2.2, -0.4, 0.6], "size": [0.8, 0.8, 0.8],
                          "material": {"type": "metal", "color": [0.7, 0.7, 0.9], "roughness": 0.0, "metallic": 1.0}})
SCENES = {"S": S, "S_CUBE": S_CUBE}

POSITIONS = [(0, 0, 3), (2.5, 0, 3), (-2.5, 0.5, 2.5), (0, 0, -10), (0, 1.8, 3.5)]
ORACLE_NONZERO = {"S": [335, 348, 445, 0, 248], "S_CUBE": [490, 449, 445, 0, 359]}
ORACLE_UNION = {"S": 1188, "S_CUBE": 1330}
# (the GENERAL camera of tests/test_gpu_camera.py: nothing about it is axis-aligned)
GENERAL = {"position": [3, 2, -5], "lookAt": [0.5, 0, 0.25], "up": [0.1, 1, 0.2], "fov": 50, "aspectRatio": 4 / 3}


def at(position, base=None):
    """The scene's camera (or `base`) moved to `position`."""
    cam = dict(base or S["camera"])
    cam["position"] = [float(v) for v in position]
    return cam


def with_camera(name, cam):
    d = copy.deepcopy(SCENES[name])
    d["camera"] = dict(cam)
    return d


def scene_json(name, cam=None):
    return json.dumps(with_camera(name, cam) if cam is not None else SCENES[name])
