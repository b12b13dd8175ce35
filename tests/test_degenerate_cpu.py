"""The degenerate scenes (tests/degenerate_cases.py) on the CPU alone.

The GPU tests (test_gpu_degenerate.py) hold the kernels to the oracle on these
scenes; this module holds the scenes to their purpose, with the oracle alone:
  - the oracle renders each the same with 1 and with 7 threads, byte for byte;
  - sensitivity: with the degenerate objects and lights dropped or repaired the
    oracle's image changes (else a kernel that ignored them would pass);
  - the finite families are not trivial (>= 30 % of the pixels lit, >= 100
    distinct RGBA values), and the families meant to produce special values
    (NaN, Inf or negative radiance) produce them in fewer than half the pixels;
  - the finite scenes render the same when loaded from JSON text;
and the host code (flattening, the schedule's tile inputs, the BVH builder)
and the oracle run them under AddressSanitizer and UndefinedBehaviorSanitizer
(with float-cast-overflow) in the stand-alone tests/c/sanitize_driver, which
reads them from tests/golden/degenerate_scenes.txt.

All at 72 x 48 with 4 samples, seeds 1 and 2, as the GPU tests render them.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import degenerate_cases as dc
import oracle
import rtgo
from conftest import GOLDEN, ROOT
from scene_cases import make_settings

W, H, SPP = 72, 48, 4
SEEDS = (1, 2)
NAMES = list(dc.SCENES)


@functools.lru_cache(maxsize=None)
def _render(name, seed, variant="scene", nthreads=7):
    """(float32 linear (H*W, 3), RGBA8 (H*W, 4)) of the oracle."""
    sc = dc.SCENES[name]
    if variant == "repaired":
        sc = dc.repaired(sc)
    scene = rtgo.Scene.from_json_text(dc.to_json(sc)) if variant == "json" else dc.load(rtgo, sc)
    lin, rgba, _ = oracle.render(scene, W, H, make_settings(rtgo, {"samples": SPP}, seed), nthreads=nthreads)
    return lin.astype(np.float32).reshape(-1, 3), rgba.reshape(-1, 4)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_is_the_same_with_one_and_seven_threads(name, seed):
    lin7, rgba7 = _render(name, seed)
    lin1, rgba1 = _render(name, seed, nthreads=1)
    assert lin1.tobytes() == lin7.tobytes()
    assert rgba1.tobytes() == rgba7.tobytes()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", NAMES)
def test_the_degenerate_objects_change_the_image(name, seed):
    lin, rgba = _render(name, seed)
    lin_r, rgba_r = _render(name, seed, "repaired")
    changed = (rgba != rgba_r).any(axis=1).sum()
    print(name, seed, "pixels changed by the repair:", changed)
    assert changed > 0
    assert lin.tobytes() != lin_r.tobytes()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", dc.FINITE)
def test_finite_scenes_are_not_trivial(name, seed):
    _, rgba = _render(name, seed)
    lit = (rgba[:, :3] > 0).any(axis=1).mean()
    distinct = len(np.unique(rgba, axis=0))
    print(name, seed, "lit", lit, "distinct", distinct)
    assert lit >= 0.30
    assert distinct >= 100


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", dc.SPECIAL)
def test_special_values_are_present_in_less_than_half_the_frame(name, seed):
    """NaN, Inf or negative radiance (negative tone-maps to NaN: byte 0)."""
    lin, rgba = _render(name, seed)
    special = (~np.isfinite(lin) | (lin < 0)).any(axis=1)
    print(name, seed, "special pixels", special.mean(), "distinct", len(np.unique(rgba, axis=0)))
    assert 0 < special.mean() < 0.5
    assert len(np.unique(rgba, axis=0)) >= 100


@pytest.mark.parametrize("seed", SEEDS)
def test_later_hittables_replace_the_nan_objects(seed):
    """nan_first: NaN objects first in hittable order; after such a hit the
    closest-so-far is NaN and every later hittable the ray meets is accepted,
    so the scene behind still shows."""
    _, rgba = _render("nonfinite_geometry_nan_first", seed)
    assert len(np.unique(rgba, axis=0)) >= 100


@pytest.mark.parametrize("name", dc.FINITE)
def test_finite_scenes_are_the_same_from_json_text(name):
    lin, rgba = _render(name, 1)
    lin_j, rgba_j = _render(name, 1, "json")
    assert lin.tobytes() == lin_j.tobytes() and rgba.tobytes() == rgba_j.tobytes()


def test_every_family_is_there():
    for fam in ("neg_zero_radius", "coincident", "coincident_wide", "zero_neg_colour", "odd_materials", "flat_cubes",
                "on_surfaces", "nonfinite_lights", "nonfinite_materials", "nonfinite_materials_inf_colour"):
        assert fam in dc.LINEAR
    assert len(dc.GEOMETRY) == 7 and len(dc.FIELD) == 6
    assert not any(n in dc.FINITE for n in dc.GEOMETRY + ["nonfinite_lights", "nonfinite_materials", "nonfinite_materials_inf_colour"])
    # coincident_wide: the partners sit on different helpers for S = 16, 8 and 4
    objs = dc.SCENES["coincident_wide"]["objects"]
    assert all(o["type"] == "sphere" for o in objs) and len(objs) >= 20
    by_pos = {}
    for i, o in enumerate(objs):
        by_pos.setdefault((tuple(o["position"]), o["radius"]), []).append(i)
    groups = [g for g in by_pos.values() if len(g) > 1]
    assert len(groups) >= 4
    for g in groups:
        for s in (16, 8, 4):
            assert g[-1] % s != g[-2] % s, (g, s)


def test_nonfinite_geometry_with_cubes_is_refused_by_rt_validate():
    """Non-finite geometry is rendered for spheres alone (rt_api.h): with a cube
    in the scene, or in a cube, RT_E_INVALID names the object and the field."""
    import ctypes

    st = make_settings(rtgo, {"samples": 1})
    want = {"nonfinite_geometry_nan_radius": "object 6: sphere radius is not finite in a scene with cubes",
            "nonfinite_geometry_nan_centre": "object 6: sphere position is not finite in a scene with cubes",
            "nonfinite_geometry_inf_radius": "object 6: sphere radius is not finite in a scene with cubes",
            "nonfinite_geometry_inf_centre": "object 6: sphere position is not finite in a scene with cubes",
            "nonfinite_geometry_nan_cube": "object 6: cube size is not finite",
            "nonfinite_geometry_inf_cube": "object 6: cube size is not finite",
            "nonfinite_geometry_nan_first": "object 0: sphere radius is not finite in a scene with cubes"}
    assert sorted(want) == sorted(dc.GEOMETRY)
    for name, message in want.items():
        scene = dc.load(rtgo, dc.SCENES[name])
        assert rtgo.lib().rt_validate(ctypes.byref(scene.view), W, H, ctypes.byref(st)) != rtgo.RT_OK, name
        assert rtgo.lib().rt_last_error().decode().startswith(message), name
        alone = dc.load(rtgo, dc.spheres_only(dc.SCENES[name]))  # the same spheres without the cubes: accepted
        assert rtgo.lib().rt_validate(ctypes.byref(alone.view), W, H, ctypes.byref(st)) == rtgo.RT_OK, name
    for name in dc.SCENES:  # lights and materials stay accepted
        if name not in dc.GEOMETRY:
            scene = dc.load(rtgo, dc.SCENES[name])
            assert rtgo.lib().rt_validate(ctypes.byref(scene.view), W, H, ctypes.byref(st)) == rtgo.RT_OK, name


# ------------------------------------------------------------ host code
FIXTURE = os.path.join(GOLDEN, "degenerate_scenes.txt")


def test_the_committed_fixture_is_the_scenes():
    """tests/golden/degenerate_scenes.txt (make_degenerate.py) is what the driver reads."""
    assert open(FIXTURE).read() == dc.fixture_text(rtgo)


def test_host_code_and_oracle_are_clean_under_asan_and_ubsan():
    """flatten_scene, tile_primary_masks and tile_cost at 72x48 and 800x600,
    lpt_partition, build_sphere_bvh (default, leaf 1, leaf 7 / 4 bins, ...) and
    a small oracle render of every degenerate scene in the sanitizer build."""
    cdir = os.path.join(ROOT, "tests", "c")
    subprocess.run(["make", "-C", cdir, "-j4", "build/sanitize_driver"], check=True, capture_output=True, timeout=900)
    # (the options of test_sanitizers.py)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([os.path.join(cdir, "build", "sanitize_driver"), "--degenerate", FIXTURE],
                       capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-5000:]
    assert "sanitize_driver: 0 failures" in p.stdout
    for name in dc.SCENES:
        assert f"\n{name}: " in "\n" + p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
