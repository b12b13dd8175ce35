"""The BVH builder on scenes with cubes (bvh.cpp: one tree over spheres and
cube boxes), on the CPU alone.

tests/c/bvh_mixed_check.cpp is compiled here, stand-alone, from the host
sources scene_json.cpp, scene_flat.cpp, bvh.cpp and oracle/oracle.c under
AddressSanitizer + UndefinedBehaviorSanitizer, and run on each scene.  It
checks that every sphere and cube sits in exactly one leaf and leaves hold one
kind; leaf counts and depth within their caps; each primitive inside its
leaf's float box, that box inside its quantized box; and, for seeded random
rays, that every sphere and triangle the oracle's exact Sphere.Hit /
Triangle.Hit accepts is reached by a conservative walk of the float boxes and
of the quantized boxes.  A sphere-only scene must yield the tree it always
did: tests/golden/bvh_sphere_trees.json holds the hashes of the trees the
sphere-only builder made before cubes were added (bvh_mixed_check hash).
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import degenerate_cases as dc
import mixed_cases as mc
from conftest import GOLDEN, ROOT
from scene_cases import ALL_MATERIALS, CUBE_SCENES

CDIR = os.path.join(ROOT, "tests", "c")
SRC = os.path.join(ROOT, "concurrent-raytracer-go_amd", "csrc")
SAN = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
       "-g", "-O1", "-ffp-contract=off"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
RAYS = 3000

SCENES = {
    "all_materials": ALL_MATERIALS,
    "field70_three_cubes": mc.field70(),
    "cube_grid_100": mc.cube_grid(100),
    "one_cube": mc.one_cube(),
    "coplanar_neighbours": mc.coplanar_neighbours(),
    "flat_cubes": dc.clean(dc.SCENES["flat_cubes"]),
    "mirrored_cubes": CUBE_SCENES["mirrored_cubes"],
    "coincident": dc.clean(dc.SCENES["coincident"]),
    "cubes_among_70_spheres": CUBE_SCENES["cubes_among_70_spheres"],
}
# (bins, leaf) of rt_tuning: the defaults, the smallest and the largest
SHAPES = [(0, 0), (2, 1), (64, 7)]
SPHERE_ONLY = {"spheres70": mc.spheres70(), "field70_coincident": dc.clean(dc.SCENES["field70_coincident"])}


@functools.lru_cache(maxsize=None)
def checker():
    out = os.path.join(CDIR, "build")
    os.makedirs(out, exist_ok=True)
    obj = os.path.join(out, "bvh_mixed_oracle.o")
    exe = os.path.join(out, "bvh_mixed_check")
    subprocess.run(["gcc", "-std=c11", "-D_GNU_SOURCE", *SAN, "-c", os.path.join(ROOT, "oracle", "oracle.c"), "-o", obj],
                   check=True, capture_output=True, timeout=600)
    subprocess.run(["g++", "-std=c++17", *SAN, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(CDIR, "bvh_mixed_check.cpp"), os.path.join(SRC, "scene_json.cpp"),
                    os.path.join(SRC, "scene_flat.cpp"), os.path.join(SRC, "bvh.cpp"), obj, "-o", exe,
                    "-lz", "-lm", "-pthread"], check=True, capture_output=True, timeout=900)
    return exe


def run(mode, scene, tmp_path, *args):
    path = os.path.join(str(tmp_path), "scene.json")
    with open(path, "w") as f:
        json.dump(scene, f, allow_nan=False)
    p = subprocess.run([checker(), mode, path, *[str(a) for a in args]], capture_output=True, text=True, timeout=600,
                       env=ENV)
    print(p.stdout)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    return p


@pytest.mark.parametrize("name", list(SCENES))
def test_mixed_tree_holds_every_primitive_and_loses_no_hit(name, tmp_path):
    for bins, leaf in SHAPES:
        p = run("check", SCENES[name], tmp_path, bins, leaf, RAYS if (bins, leaf) == (0, 0) else RAYS // 6)
        assert p.returncode == 0, (bins, leaf, p.stdout[-2000:], p.stderr[-3000:])
        assert "bvh_mixed_check: 0 failures" in p.stdout


def test_the_scenes_are_what_they_are_meant_to_be():
    def kinds(sc):
        return (sum(o["type"] == "sphere" for o in sc["objects"]), sum(o["type"] == "cube" for o in sc["objects"]))

    assert kinds(SCENES["field70_three_cubes"]) == (70, 3)
    assert kinds(SCENES["cube_grid_100"]) == (0, 100)
    assert kinds(SCENES["one_cube"]) == (0, 1)
    assert kinds(SCENES["all_materials"])[1] == 2
    assert any(0 in o["size"] for o in SCENES["flat_cubes"]["objects"] if o["type"] == "cube")
    assert any(min(o["size"]) < 0 for o in SCENES["mirrored_cubes"]["objects"] if o["type"] == "cube")
    cubes = [(tuple(o["position"]), tuple(o["size"])) for o in SCENES["coincident"]["objects"] if o["type"] == "cube"]
    assert len(cubes) != len(set(cubes))
    for sc in SPHERE_ONLY.values():
        assert kinds(sc)[0] > 64 and kinds(sc)[1] == 0


@pytest.mark.parametrize("name", list(SPHERE_ONLY))
def test_sphere_only_scenes_get_the_tree_they_always_did(name, tmp_path):
    golden = json.load(open(os.path.join(GOLDEN, "bvh_sphere_trees.json")))
    for bins, leaf in SHAPES:
        p = run("hash", SPHERE_ONLY[name], tmp_path, bins, leaf)
        assert p.returncode == 0, p.stderr[-3000:]
        line = next(ln for ln in p.stdout.splitlines() if ln.startswith("tree "))
        assert line == golden[f"{name}/{bins}/{leaf}"], (name, bins, leaf)
        # ... and passes the same checks as a mixed one
        p = run("check", SPHERE_ONLY[name], tmp_path, bins, leaf, RAYS // 6)
        assert p.returncode == 0 and "bvh_mixed_check: 0 failures" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_the_tie_scene_has_ties_to_resolve():
    """A guard on the fixture of the GPU tie tests (coplanar_neighbours): the
    later of its two coincident cubes shows (the oracle's last hittable wins), so
    dropping it changes the image and a traversal that kept the first would fail."""
    import copy

    import oracle
    import rtgo
    from scene_cases import make_settings

    sc = copy.deepcopy(mc.coplanar_neighbours())
    assert sc["objects"][-2]["position"] == sc["objects"][-3]["position"]
    st = make_settings(rtgo, {"samples": 3})
    full = oracle.render(rtgo.Scene.from_json_text(json.dumps(sc)), 72, 48, st)[1]
    del sc["objects"][-2]
    less = oracle.render(rtgo.Scene.from_json_text(json.dumps(sc)), 72, 48, st)[1]
    assert (np.asarray(full) != np.asarray(less)).any()
