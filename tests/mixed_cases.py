"""Scenes with spheres and cubes for the mixed BVH (bvh.cpp: one tree over
spheres and cube boxes), shared by test_bvh_mixed_cpu.py and
test_gpu_bvh_cubes.py.  Plain dicts for rtgo.Scene.from_json_text / from_python.
"""
import copy

CAM = {"position": [0, 0.5, 6], "aspectRatio": 1.5}
LIGHTS = [{"position": [0, 6, 3], "color": [1, 1, 1], "intensity": 60},
          {"position": [-4, 2, -2], "color": [1, 0.9, 0.8], "intensity": 30}]

LAMB = {"type": "lambertian", "color": [0.7, 0.6, 0.5]}
GREY = {"type": "lambertian", "color": [0.5, 0.5, 0.5]}
RED = {"type": "lambertian", "color": [0.8, 0.2, 0.2]}
BLUE = {"type": "lambertian", "color": [0.2, 0.3, 0.8]}
GREEN = {"type": "lambertian", "color": [0.2, 0.7, 0.3]}
METAL = {"type": "metal", "color": [0.9, 0.8, 0.7], "roughness": 0.1, "metallic": 0.9}
MIRROR = {"type": "metal", "color": [0.95, 0.95, 0.95], "roughness": 0.0, "metallic": 1.0}
GLASS = {"type": "glass", "color": [0.9, 0.95, 1.0], "refractionIndex": 1.5}
DIEL = {"type": "dielectric", "refractionIndex": 1.33}


def sph(p, r, m):
    return {"type": "sphere", "position": list(p), "radius": r, "material": m}


def cube(p, s, m):
    return {"type": "cube", "position": list(p), "size": list(s), "material": m}


def scene(objects, lights=None, camera=None):
    return {"camera": copy.deepcopy(camera or CAM), "objects": copy.deepcopy(objects),
            "lights": copy.deepcopy(lights or LIGHTS)}


def field70(extra=(), floor_cube=True):
    """70 small spheres (more than 64: a tree by the automatic rule) standing on
    a floor cube whose top is y = -1, a glass cube and a mirrored cube (one
    negative size component: its normals point out) among them."""
    objs = [cube((0, -1.5, 0), (40, 1, 40), GREY)] if floor_cube else [sph((0, -1001, 0), 1000, GREY)]
    for i in range(70):
        x = (i % 10) * 0.7 - 3.15
        z = -(i // 10) * 0.7 + 1.0
        objs.append(sph((x, -0.8 + 0.1 * (i % 3), z), 0.22, [METAL, GLASS, RED, DIEL][i % 4]))
    objs += [cube((-0.6, 0.2, 1.4), (1.0, 1.0, 1.0), GLASS), cube((1.3, 0.0, 0.8), (-0.8, 0.8, 0.8), RED)]
    return scene(objs + list(extra))


def spheres70():
    """The same field on a ground sphere, without any cube (the sphere-only tree)."""
    sc = field70(floor_cube=False)
    sc["objects"] = [o for o in sc["objects"] if o["type"] == "sphere"]
    return sc


def cube_grid(n=100):
    """n cubes and no sphere: a 10-wide grid of small cubes over a floor cube
    (the first of the n), materials in turn."""
    objs = [cube((0, -1.5, 0), (40, 1, 40), GREY)]
    mats = [RED, METAL, GLASS, BLUE, MIRROR, GREEN, DIEL]
    for i in range(n - 1):
        x = (i % 10) * 0.75 - 3.4
        z = -(i // 10) * 0.75 + 2.0
        h = 0.3 + 0.1 * (i % 4)
        objs.append(cube((x, -1.0 + h / 2 + 0.05 * (i % 2), z), (0.5, h, 0.5), mats[i % 7]))
    return scene(objs)


def one_cube():
    return scene([cube((0.3, 0, 0), (1.6, 1.2, 1.4), RED)])


def coplanar_neighbours():
    """Cubes that share faces exactly (a ray along the shared plane meets two
    coplanar faces at the same t), two coincident cubes of different materials
    and a sphere tangent to a cube face, on a floor cube."""
    objs = [cube((0, -1.5, 0), (40, 1, 40), GREY)]
    for i, m in enumerate([RED, GREEN, BLUE, METAL]):
        objs.append(cube((-1.5 + i, -0.5, 0), (1, 1, 1), m))       # faces shared at x = -1, 0, 1
    objs.append(cube((0, 0.5, 0), (1, 1, 1), GLASS))                # stands on two of them
    objs += [cube((2.5, -0.5, 1), (1, 1, 1), METAL), cube((2.5, -0.5, 1), (1, 1, 1), BLUE)]
    objs.append(sph((-2.5, -0.5, 0), 0.5, MIRROR))                  # touches the face x = -2
    return scene(objs)


def shadows_across_kinds():
    """A sphere shadowing a floor cube, a cube shadowing a sphere and the floor,
    and a light inside a glass cube."""
    objs = [cube((0, -1.5, 0), (40, 1, 40), GREY), sph((-1.8, 0.2, 0), 0.7, RED),
            cube((1.2, 0.9, 0.2), (1.0, 0.4, 1.0), METAL), sph((1.2, -0.5, 0.2), 0.5, GREEN),
            cube((-0.2, -0.4, 1.8), (1.0, 1.0, 1.0), GLASS)]
    lights = [{"position": [0.5, 6, 2], "color": [1, 1, 1], "intensity": 60},
              {"position": [-0.2, -0.3, 1.8], "color": [1, 0.8, 0.6], "intensity": 4},
              {"position": [-5, 3, 4], "color": [0.8, 0.8, 1], "intensity": 30}]
    return scene(objs, lights)
