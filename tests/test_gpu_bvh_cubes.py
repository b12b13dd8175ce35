"""GPU: a BVH over spheres and cubes (bvh.cpp, rt_device.h closest_hit /
any_hit with leaves of cubes) against the oracle's linear scan.

A scene with cubes gets a tree with force_bvh > 0, or by the automatic rule
(more than 64 spheres, or more than 64 cubes).  Every image here is compared
byte for byte, float32 radiance and RGBA8, with the oracle, which scans every
hittable linearly whatever the GPU does.  Both BVH paths are rendered: the
wavefront kernels' mixed instantiations (RT_PATH_AUTO; wf_extend_mix and its
siblings) and the megakernel (RT_PATH_MEGAKERNEL;
render_kernel_mix).  Every render says which path it expects, and _render
checks that the wavefront kernels ran exactly then: a plain render through
the context's per-kernel profile (launches of the closest-hit kernel), a
counting render through the closest-hit kernel's own share of the counts.

Images are at most 72x48 with 3 to 7 samples.
"""
import copy
import ctypes
import functools
import json

import numpy as np
import pytest

import degenerate_cases as dc
import mixed_cases as mc
import oracle
import rtgo
from gpu_util import render_dev
from scene_cases import ALL_MATERIALS, CUBE_SCENES, make_settings
from test_gpu_wavefront import PATH_KEYS

pytestmark = pytest.mark.gpu

W, H = 72, 48
NAN, INF = float("nan"), float("inf")
RT_E_INVALID = -1
PATHS = [("auto", rtgo.RT_PATH_AUTO), ("megakernel", rtgo.RT_PATH_MEGAKERNEL)]


def _nonfinite_light():
    sc = mc.field70()
    sc["lights"] = sc["lights"] + [{"position": [INF, 4, 2], "color": [1, 1, 1], "intensity": 30.0},
                                   {"position": [1, NAN, 3], "color": [1, 1, 1], "intensity": 30.0}]
    return sc


def _nonfinite_material():
    sc = mc.field70()
    sc["objects"][5]["material"] = {"type": "metal", "color": [0.9, NAN, 0.7], "roughness": 0.1, "metallic": 0.9}
    sc["objects"][12]["material"] = {"type": "metal", "color": [0.9, 0.8, 0.7], "roughness": NAN, "metallic": 0.9}
    sc["objects"][72]["material"] = {"type": "glass", "color": [0.9, 0.95, 1.0], "refractionIndex": NAN}  # the mirrored cube
    return sc


SCENES = {
    "all_materials": ALL_MATERIALS,
    "field70": mc.field70(),
    "cube_grid_100": mc.cube_grid(100),
    "one_cube": mc.one_cube(),
    "coplanar_neighbours": mc.coplanar_neighbours(),
    "shadows_across_kinds": mc.shadows_across_kinds(),
    "coincident": dc.clean(dc.SCENES["coincident"]),
    "flat_cubes": dc.clean(dc.SCENES["flat_cubes"]),
    "nonfinite_light": _nonfinite_light(),
    "nonfinite_material": _nonfinite_material(),
}
SCENES.update({"cube_" + k: v for k, v in CUBE_SCENES.items()})


@functools.lru_cache(maxsize=None)
def _scene(name):
    sc = SCENES[name]
    return rtgo.Scene.from_python(sc["camera"], sc["objects"], sc["lights"])


def _settings(over):
    return make_settings(rtgo, dict(over), over.get("seed", 1))


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, over):
    """(float32 linear (w*h, 3), RGBA8 (w*h, 4)) of the oracle, computed once."""
    lin, rgba, _ = oracle.render(_scene(name), w, h, _settings(dict(over)))
    return lin.astype(np.float32).reshape(-1, 3), rgba.reshape(-1, 4)


def _key(over):
    return tuple(sorted(over.items()))


def _render(name, over, path, force_bvh=1, w=W, h=H, count=False, tun=None, rank=0, world=1, wf=None):
    """wf: the wavefront kernels must have run (default: RT_PATH_AUTO and a tree
    not forbidden; a caller whose scene gets no tree says wf=False)."""
    import torch

    if wf is None:
        wf = path == rtgo.RT_PATH_AUTO and force_bvh >= 0
    t = rtgo.default_tuning(**(tun or {}))
    t.path = path
    if count:
        lin, rgba, _, full = render_dev(_scene(name), w, h, _settings(over), rank=rank, world=world, tuning=t,
                                        force_bvh=force_bvh, count="full")
        ext = full.extend_dict()
        assert (ext["box_tests"] > 0) == wf, (name, path, ext)
        counts = full.as_dict()
        counts["wf_triangle_tests"] = ext["triangle_tests"]
        counts["wf_soft_rays_traced"] = full.soft_occlusion_dict()["shadow_rays"]
        return lin, rgba, counts
    if world > 1:
        lin, rgba, _, _ = render_dev(_scene(name), w, h, _settings(over), rank=rank, world=world, tuning=t,
                                     force_bvh=force_bvh)
        return lin, rgba, None
    ctx = rtgo.Context(0)
    try:
        ctx.set_tuning(t)
        ctx.set_scene(_scene(name), force_bvh=force_bvh)
        ctx.profile(True)
        d_lin = torch.full((w * h * 3,), float("nan"), dtype=torch.float32, device="cuda")
        d_rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
        ctx.render_async(w, h, _settings(over), d_lin.data_ptr(), d_rgba.data_ptr(), 0)
        torch.cuda.synchronize()
        launches = ctx.kernel_seconds()["extend"][1]
    finally:
        ctx.close()
    assert (launches > 0) == (wf and over.get("max_depth", 50) >= 0), (name, path, launches)
    return d_lin.cpu().numpy().reshape(-1, 3), d_rgba.cpu().numpy().reshape(-1, 4), None


def _same(got, want, what):
    """Byte for byte; NaN pixels included (the same bits)."""
    bad = (got[0].view(np.uint32) != want[0].view(np.uint32)).any(axis=1)
    print(what, "pixels that differ:", int(bad.sum()), "of", len(bad))
    assert got[0].tobytes() == want[0].tobytes(), what
    assert got[1].tobytes() == want[1].tobytes(), what


# ---------------------------------------------------------------- 1. forced trees against the oracle
FORCED = ["all_materials"] + ["cube_" + k for k in CUBE_SCENES] + ["cube_grid_100", "one_cube"]


@pytest.mark.parametrize("pname,path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("name", FORCED)
def test_forced_tree_equals_the_oracle(name, pname, path):
    over = {"samples": 4}
    lin, rgba, counts = _render(name, over, path, count=True)
    _same((lin, rgba), _oracle(name, W, H, _key(over)), (name, pname))
    assert counts["box_tests"] > 0 and counts["triangle_tests"] > 0, counts
    # (the wavefront's closest-hit kernel told triangles from spheres: it tested triangles itself)
    assert (counts["wf_triangle_tests"] > 0) == (pname == "auto"), counts


# ---------------------------------------------------------------- 2. the automatic rule
def test_auto_rule_builds_a_tree_for_70_spheres_and_three_cubes():
    over = {"samples": 5}
    ref = _oracle("field70", W, H, _key(over))
    auto = _render("field70", over, rtgo.RT_PATH_AUTO, force_bvh=0, count=True)
    mega = _render("field70", over, rtgo.RT_PATH_MEGAKERNEL, force_bvh=0, count=True)
    assert auto[2]["box_tests"] > 0 and mega[2]["box_tests"] > 0
    _same(auto, ref, "auto")
    _same(mega, ref, "megakernel")
    assert {k: auto[2][k] for k in PATH_KEYS} == {k: mega[2][k] for k in PATH_KEYS}
    lin = _render("field70", over, rtgo.RT_PATH_AUTO, force_bvh=-1, count=True)
    assert lin[2]["box_tests"] == 0
    _same(lin, auto, "linear scan")
    assert {k: lin[2][k] for k in PATH_KEYS} == {k: auto[2][k] for k in PATH_KEYS}


def test_auto_rule_counts_cubes_and_leaves_small_scenes_alone():
    over = {"samples": 3}
    grid = _render("cube_grid_100", over, rtgo.RT_PATH_AUTO, force_bvh=0, count=True)   # 100 cubes > 64
    assert grid[2]["box_tests"] > 0
    _same(grid, _oracle("cube_grid_100", W, H, _key(over)), "100 cubes")
    small = _render("all_materials", over, rtgo.RT_PATH_AUTO, force_bvh=0, count=True, wf=False)  # 9 spheres, 2 cubes
    assert small[2]["box_tests"] == 0
    forbidden = _render("cube_grid_100", over, rtgo.RT_PATH_AUTO, force_bvh=-1, count=True)
    assert forbidden[2]["box_tests"] == 0
    _same(forbidden, grid, "forbidden")


# ---------------------------------------------------------------- 3. ties and degenerate cubes
@pytest.mark.parametrize("pname,path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("name", ["coincident", "coplanar_neighbours", "flat_cubes", "cube_mirrored_cubes"])
@pytest.mark.parametrize("seed", [1, 2])
def test_ties_and_degenerate_cubes(name, seed, pname, path):
    over = {"samples": 4, "seed": seed}
    _same(_render(name, over, path)[:2], _oracle(name, W, H, _key(over)), (name, seed, pname))


# ---------------------------------------------------------------- 4. shadows across kinds
@pytest.mark.parametrize("pname,path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("over", [{"samples": 5}, {"samples": 4, "soft_shadows": 0}], ids=["soft", "hard"])
def test_shadows_across_kinds(over, pname, path):
    _same(_render("shadows_across_kinds", over, path)[:2], _oracle("shadows_across_kinds", W, H, _key(over)),
          (over, pname))


def test_cones_that_start_on_a_floor_cube_are_traced_and_exact():
    """The wavefront cone walk keeps lists of spheres only: a cone that reaches a
    cube's bounding sphere ends as "too many candidates" and its 16 rays are
    traced.  On the floor cube every cone does (the floor's sphere holds the hit
    point); on the spheres some cones are listed.  The image is the oracle's
    either way, and the soft kernel's own count says how many rays were traced."""
    over = {"samples": 5}
    lin, rgba, c = _render("field70", over, rtgo.RT_PATH_AUTO, force_bvh=0, count=True)
    _same((lin, rgba), _oracle("field70", W, H, _key(over)), "field70 soft shadows")
    soft = c["shadow_rays"] - c["light_evals"]  # (one hard ray per evaluated light, 16 soft rays per clear one)
    assert soft > 0 and soft % 16 == 0
    print("soft rays", soft, "traced", c["wf_soft_rays_traced"], "share", c["wf_soft_rays_traced"] / soft)
    assert 0 < c["wf_soft_rays_traced"] <= soft


# ---------------------------------------------------------------- 5. tree and capacity shapes
SHAPES = [({"bvh_leaf": 1}, {}), ({"bvh_leaf": 7, "bvh_bins": 4}, {}), ({"wf_lds_nodes": 0}, {}),
          ({"wf_lds_nodes": 31}, {}), ({"wf_paths": 64}, {}), ({}, {"max_depth": 0}), ({}, {"max_depth": 1})]


@pytest.mark.parametrize("pname,path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("tun,extra", SHAPES, ids=["leaf1", "leaf7_bins4", "lds0", "lds31", "paths64", "depth0", "depth1"])
def test_tree_and_capacity_shapes(tun, extra, pname, path):
    over = dict({"samples": 3}, **extra)
    _same(_render("field70", over, path, force_bvh=0, tun=tun)[:2], _oracle("field70", W, H, _key(over)),
          (tun, extra, pname))


# ---------------------------------------------------------------- 6. non-finite rays
@pytest.mark.parametrize("pname,path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("name", ["nonfinite_light", "nonfinite_material"])
def test_nonfinite_rays_take_the_mixed_scan(name, pname, path):
    """A light at x = +Inf or y = NaN gives shadow rays, a NaN roughness or
    index bounce rays, that no box serves: the fallback scans spheres and cubes."""
    over = {"samples": 4}
    ref = _oracle(name, W, H, _key(over))
    print(name, "pixels with a NaN or Inf:", int((~np.isfinite(ref[0])).any(axis=1).sum()))
    _same(_render(name, over, path, force_bvh=0)[:2], ref, (name, pname))


# ---------------------------------------------------------------- 7. the entry points around it
def test_progression_of_3_plus_4_equals_7_samples():
    from test_gpu_progressive import _Prog

    p = _Prog(_scene("field70"))
    try:
        p.begin(W, H, _settings({"samples": 7}))
        for n, done in ((3, 3), (4, 7)):
            lin, rgba = p.add(n)
            ref = _oracle("field70", W, H, _key({"samples": done}))
            _same((lin.reshape(-1, 3), rgba.reshape(-1, 4)), ref, done)
    finally:
        p.close()


def test_adaptive_progression_stops_pixels_at_the_oracles_samples():
    """test_gpu_adaptive's 37x29 row on all materials, now with a forced tree
    over its nine spheres and two cubes."""
    import test_gpu_adaptive as ta

    for tun in (None, {"path": rtgo.RT_PATH_MEGAKERNEL}):
        ta._run(ta.ROW_B, tun, force_bvh=1).close()


def test_rank_1_of_3_packed_tiles():
    over = {"samples": 3}
    a = _render("field70", over, rtgo.RT_PATH_AUTO, force_bvh=0, rank=1, world=3)
    b = _render("field70", over, rtgo.RT_PATH_MEGAKERNEL, force_bvh=0, rank=1, world=3)
    c = _render("field70", over, rtgo.RT_PATH_MEGAKERNEL, force_bvh=-1, rank=1, world=3)
    _same(a[:2], b[:2], "auto against megakernel")
    _same(a[:2], c[:2], "tree against linear scan")
    assert np.isfinite(a[0]).any()


def test_renderer_reports_the_build_time_of_a_mixed_tree():
    r = rtgo.ParallelRenderer()
    r.set_samples(3)
    rgba = r.render(_scene("field70"), W, H)
    assert r.last_stats.bvh_build_seconds > 0
    ref_rgba = oracle.render(_scene("field70"), W, H, r.settings)[1]
    assert np.asarray(rgba).reshape(-1, 4).tobytes() == ref_rgba.reshape(-1, 4).tobytes()


def test_sky_kernel_of_a_mixed_tree_equals_the_linear_scan():
    """An opted-in sky has kernels of its own (and its exp / pow are the
    GPU's, so the oracle is compared at a tolerance elsewhere): here the tree
    against the linear scan of the same build, byte for byte."""
    over = {"samples": 4, "sky": rtgo.SKIES["white"]}
    tree = _render("field70", over, rtgo.RT_PATH_AUTO, force_bvh=0, count=True)
    scan = _render("field70", over, rtgo.RT_PATH_AUTO, force_bvh=-1, count=True)
    assert tree[2]["box_tests"] > 0 and scan[2]["box_tests"] == 0
    _same(tree, scan, "sky")
    plain = _render("field70", {"samples": 4}, rtgo.RT_PATH_AUTO, force_bvh=0)
    assert plain[0].tobytes() != tree[0].tobytes()  # the sky shows


# ---------------------------------------------------------------- 8. refusals that stay
@pytest.mark.parametrize("name", ["nonfinite_geometry_nan_cube", "nonfinite_geometry_inf_cube",
                                  "nonfinite_geometry_nan_radius", "nonfinite_geometry_inf_centre"])
def test_nonfinite_geometry_beside_a_cube_is_still_refused(name):
    scene = dc.load(rtgo, dc.SCENES[name])
    ctx = rtgo.Context(0)
    try:
        rc = rtgo.lib().rt_context_set_scene(ctx._h, ctypes.byref(scene.view), 1)
        assert rc == RT_E_INVALID
        assert b"not finite" in rtgo.lib().rt_last_error()
    finally:
        ctx.close()


# ---------------------------------------------------------------- 9. cross-lane reads
XLANE_CHILD = r"""
import ctypes, hashlib, json, sys
sys.path[:0] = [%(tests)r, %(pkg)r]
import mixed_cases as mc
import rtgo
from scene_cases import make_settings


def renders():
    out = []
    # (both get a tree by the automatic rule: 70 spheres; 100 cubes)
    for sc, over in ((mc.field70(), {"samples": 6}), (mc.cube_grid(100), {"samples": 4}),
                     (mc.field70(), {"samples": 5, "soft_shadows": 0, "max_depth": 12})):
        r = rtgo.ParallelRenderer()
        r.settings = make_settings(rtgo, over, 3)
        r.render(rtgo.Scene.from_json_text(json.dumps(sc)), 48, 32)
        out.append(hashlib.sha1(r.last_linear.tobytes()).hexdigest())
        r.close()
    return out


lib = rtgo.lib()
n = ctypes.c_uint64(0)
check = %(check)r
if check:
    assert lib.rt_debug_xlane_faults(0, 1, ctypes.byref(n)) == 0, lib.rt_last_error()
h = renders()
if check:
    assert lib.rt_debug_xlane_faults(0, 0, ctypes.byref(n)) == 0, lib.rt_last_error()
print("XLANE_FAULTS", n.value)
print("HASHES", json.dumps(h))
"""


def test_mixed_kernels_read_no_inactive_lane():
    """The kernels that walk cube leaves (the wavefront's mixed kernels, which
    the renderer takes for these scenes) in the cross-lane
    checking build (test_gpu_xlane.py) on the 70-sphere field and the 100-cube
    grid, soft and hard shadows: zero reads from inactive lanes, and the
    product's bits."""
    import os
    import subprocess
    import sys

    from conftest import PKG, ROOT
    from test_gpu_xlane import XLIB

    assert os.path.exists(XLIB), "build() makes build/xlane/librtgo.so"

    def child(lib, check):
        code = XLANE_CHILD % {"tests": os.path.join(ROOT, "tests"), "pkg": PKG, "check": check}
        env = dict(os.environ)
        if lib:
            env["RTGO_LIB"] = lib
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        return (int(p.stdout.split("XLANE_FAULTS")[1].split()[0]),
                json.loads(p.stdout.split("HASHES")[1].strip().splitlines()[0]))

    faults, hashes = child(XLIB, True)
    assert faults == 0
    assert child(None, False)[1] == hashes
