"""Scenes of the history-rectification tests, fixed on the
reference (the oracle's renders) alone.

C_FLOOR: a Lambertian floor slab (object 0), a Lambertian sphere above it
(object 1) that moves by FLOOR_MOVE per frame -- about 5 pixels at 144x96 --
one point light above and to the side, the reference camera at (0, 0.6, 3)
standing still.  The sphere's shadow sweeps over floor pixels that do not move:
their reprojected history is exact geometry and stale light.

C_LIGHT: the same geometry standing still and the light moving by LIGHT_MOVE
per frame: the whole floor's lighting changes and no pixel moves.

S_CUBE is sequence_cases' (a metal sphere, a Lambertian one, glass, a mirror
cube): the static scene the clip must not hurt."""
import copy
import json

from sequence_cases import SCENES as _SEQ

C_FLOOR = {
    "camera": {"position": [0, 0.6, 3], "lookAt": [0, 0, 0], "up": [0, 1, 0], "fov": 60, "aspectRatio": 1.5},
    "objects": [
        {"type": "cube", "position": [0, -1.0, -1.0], "size": [9.0, 0.4, 7.0],
         "material": {"type": "lambertian", "color": [0.8, 0.75, 0.7]}},
        {"type": "sphere", "position": [-0.9, -0.2, -0.4], "radius": 0.45,
         "material": {"type": "lambertian", "color": [0.3, 0.4, 0.9]}},
    ],
    "lights": [{"type": "point", "position": [-1.0, 5.0, 2.0], "color": [1, 1, 1], "intensity": 40.0}],
}
C_LIGHT = copy.deepcopy(C_FLOOR)
SCENES = {"C_FLOOR": C_FLOOR, "C_LIGHT": C_LIGHT, "S_CUBE": _SEQ["S_CUBE"]}
CAMERA = dict(C_FLOOR["camera"])
FLOOR_MOVE = (0.25, 0.0, 0.0)  # object 1 per frame
LIGHT_MOVE = (0.9, 0.0, 0.0)   # light 0 per frame
FLOOR_ID, SPHERE_ID = 0, 1


def frame_scene(name, f):
    """Frame f of the case as a scene dict: C_FLOOR with the sphere moved, C_LIGHT with the light moved, any
    other scene as it is."""
    d = copy.deepcopy(SCENES[name])
    if name == "C_FLOOR":
        d["objects"][SPHERE_ID]["position"] = [float(d["objects"][SPHERE_ID]["position"][k]) + f * FLOOR_MOVE[k]
                                               for k in range(3)]
    if name == "C_LIGHT":
        d["lights"][0]["position"] = [float(d["lights"][0]["position"][k]) + f * LIGHT_MOVE[k] for k in range(3)]
    return d


def frame_json(name, f, cam=None):
    d = frame_scene(name, f)
    if cam is not None:
        d["camera"] = dict(cam)
    return json.dumps(d)
