"""Specular-through feature buffers (rt_context_render_aov_spec_async, DESIGN.md
§4.16), CPU: the declarations and their ctypes mirrors, the defaults, the
followed-material predicate (rt_aov_spec_follows) over every kind and around
the threshold, the Python layer's argument checks, and the reference helper of
the GPU tests (tests/aov_spec_reference.py) held to what it restates: with no
bounce it is aov_reference.reference bit for bit, and its reflected ray is the
ray oracle.scatter makes for a roughness-0 metal."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import rtgo
from aov_reference import bits, camera_ray, reference as first_hit_reference
from aov_spec_reference import chain, hittables_with_materials, reference
from conftest import ROOT
from sequence_cases import scene_json
from spec_cases import CUBE_1, CUBE_2, S_MIRROR, text

HEADER = os.path.join(ROOT, "include", "rt_api.h")
W, H, SPP, SEED = 72, 48, 4, 3
RT_E_INVALID = -1
FUNCS = ["rt_aov_spec_default", "rt_aov_spec_follows", "rt_context_render_aov_spec_async"]


def test_declared_exported_and_mirrored(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\}\s*rt_aov_spec\s*;", src) and re.search(r"\}\s*rt_aov_spec_buffers\s*;", src)
    lib = ctypes.CDLL(rtgo.LIB_PATH)
    for f in FUNCS:
        assert hasattr(lib, f) and f in rtgo.EXPORTED_SYMBOLS, f
    assert rtgo.lib().rt_abi_version() == 8  # (additive: the version stays)
    assert rtgo.AOV_SPEC_NAMES == rtgo.AOV_NAMES + ["specular", "bounces"]
    assert rtgo.AOV_NAMES == ["albedo", "normal", "depth", "coverage", "object"]
    inc = os.path.join(ROOT, "include")
    typ = tmp_path / "spec_type.c"  # the declarations have exactly these types (compiled only)
    typ.write_text('#include "rt_api.h"\n'
                   "void (*const f0)(rt_aov_spec*) = rt_aov_spec_default;\n"
                   "int (*const f1)(const rt_material*, const rt_aov_spec*) = rt_aov_spec_follows;\n"
                   "int (*const f2)(rt_context*, int32_t, int32_t, const rt_settings*, const rt_camera*,\n"
                   "                const rt_aov_spec*, const rt_aov_spec_buffers*, void*) =\n"
                   "    rt_context_render_aov_spec_async;\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", inc, "-c", str(typ), "-o", str(tmp_path / "t.o")],
                   check=True)
    structs = {"rt_aov_spec": (rtgo.AovSpec, ["max_bounces", "max_roughness"]),
               "rt_aov_spec_buffers": (rtgo.AovSpecBuffers, ["d_" + n for n in rtgo.AOV_SPEC_NAMES])}
    assert [n for n, _ in rtgo.AovSpecBuffers._fields_] == structs["rt_aov_spec_buffers"][1]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_api.h"', "int main(void) {"]
    for c, (_, fields) in structs.items():
        lines.append(f'printf("{c} sizeof %zu\\n", sizeof({c}));')
        lines += [f'printf("{c} {n} %zu\\n", offsetof({c}, {n}));' for n in fields]
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = {tuple(ln.split()[:2]): int(ln.split()[2])
           for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    for c, (cls, fields) in structs.items():
        assert got[(c, "sizeof")] == ctypes.sizeof(cls), c
        for n in fields:
            assert got[(c, n)] == getattr(cls, n).offset, (c, n)


def test_defaults():
    sp = rtgo.AovSpec(99, 99, 99.0)
    rtgo.lib().rt_aov_spec_default(ctypes.byref(sp))
    assert (sp.max_bounces, sp._pad, sp.max_roughness) == (4, 0, 0.1)
    d = rtgo.default_aov_spec(max_bounces=2)
    assert (d.max_bounces, d.max_roughness) == (2, 0.1)
    with pytest.raises(rtgo.RenderError):
        rtgo.default_aov_spec(bounces=2)


def _follows(kind, roughness, max_roughness, max_bounces=4):
    m = rtgo.Material()
    m.kind = rtgo.MATERIAL_KINDS[kind]
    m.color[:] = (0.5, 0.5, 0.5)
    m.roughness = roughness
    m.refraction_index = 1.5
    sp = rtgo.AovSpec(max_bounces, 0, max_roughness)
    return rtgo.lib().rt_aov_spec_follows(ctypes.byref(m), ctypes.byref(sp))


def test_follows_over_kinds_and_around_the_threshold():
    assert len(rtgo.MATERIAL_KINDS) == 7
    below, above = float(np.nextafter(0.1, 0)), float(np.nextafter(0.1, 1))
    for kind in rtgo.MATERIAL_KINDS:
        mirror = kind in ("metal", "shiny", "perfectmirror")
        assert _follows(kind, below, 0.1) == int(mirror), kind
        assert _follows(kind, 0.1, 0.1) == int(mirror), kind  # at the threshold: followed
        assert _follows(kind, above, 0.1) == 0, kind
        assert _follows(kind, 0.0, 0.0) == int(mirror), kind
        assert _follows(kind, 5.0, 1.0) == int(mirror), kind  # the constructors' clamp: Min(5, 1) <= 1
        assert _follows(kind, 5.0, 0.999) == 0, kind
        assert _follows(kind, float("nan"), 1.0) == 0, kind  # a NaN compares false
        assert _follows(kind, float("nan"), 1e300) == 0, kind
        assert _follows(kind, -1.0, 0.0) == int(mirror), kind
    # the Python wrapper, on scene-file materials
    assert rtgo.aov_spec_follows({"type": "metal", "color": [1, 1, 1], "roughness": 0.1}) is True
    assert rtgo.aov_spec_follows({"type": "metal", "color": [1, 1, 1], "roughness": 0.2}) is False
    assert rtgo.aov_spec_follows({"type": "metal", "color": [1, 1, 1], "roughness": 0.2}, {"max_roughness": 0.2}) is True
    assert rtgo.aov_spec_follows({"type": "glass", "color": [1, 1, 1], "refractionIndex": 1.5}, "default") is False


def test_bad_parameters_are_refused():
    lib = rtgo.lib()
    m = rtgo.Material()
    m.kind = rtgo.MATERIAL_KINDS["metal"]
    ok = rtgo.default_aov_spec()
    assert lib.rt_aov_spec_follows(None, ctypes.byref(ok)) == RT_E_INVALID
    assert lib.rt_aov_spec_follows(ctypes.byref(m), None) == RT_E_INVALID
    for mb, mr in ((-1, 0.1), (17, 0.1), (4, -0.001), (4, float("nan")), (4, float("inf")), (4, float("-inf"))):
        assert _follows("metal", 0.0, mr, mb) == RT_E_INVALID, (mb, mr)
        assert lib.rt_last_error()
    for mb, mr in ((0, 0.0), (16, 1e300)):
        assert _follows("metal", 0.0, mr, mb) == 1, (mb, mr)
    # the call refuses NULLs before it looks at a device
    st, out = rtgo.default_settings(), rtgo.AovSpecBuffers()
    assert lib.rt_context_render_aov_spec_async(None, 8, 8, ctypes.byref(st), None, ctypes.byref(ok),
                                                ctypes.byref(out), None) == RT_E_INVALID
    with pytest.raises(rtgo.RenderError):
        rtgo.aov_spec_follows({"type": "metal", "color": [1, 1, 1]}, {"max_bounces": 17})


def test_python_layer_rejects_bad_arguments_before_a_context_is_made():
    r = rtgo.ParallelRenderer(1)
    r.set_samples(2)
    scene = rtgo.Scene.from_json_text(text(S_MIRROR))
    with pytest.raises(rtgo.RenderError, match="image size"):
        r.render_aov(scene, 0, 8, specular="default")
    with pytest.raises(rtgo.RenderError, match="specular"):
        r.render_aov(scene, 8, 8, specular=3)
    with pytest.raises(rtgo.RenderError, match="guide"):
        r.render_denoised(scene, 8, 8, guide="second")
    with pytest.raises(rtgo.RenderError, match="guide"):
        r.render_denoised(scene, 8, 8, specular="default")  # (parameters without the guide they belong to)
    with pytest.raises(rtgo.RenderError, match="denoise"):
        r.render_progressive(scene, 8, 8, 1, guide="specular")
    with pytest.raises(rtgo.RenderError, match="denoise or variance"):
        r.render_sequence(scene, 8, 8, [{"position": [0, 0, 3]}], temporal=True, guide="specular")
    assert r._prog_ctx is None and r._r is None  # nothing touched a device


def test_reference_without_bounces_is_the_first_hit_reference():
    s_cube = scene_json("S_CUBE")
    want = first_hit_reference(s_cube, W, H, SPP, SEED)
    got = reference(s_cube, W, H, SPP, SEED, max_bounces=0)
    for k in rtgo.AOV_NAMES:
        assert got[k].dtype == want[k].dtype and np.array_equal(bits(got[k]), bits(want[k])), k
    assert not got["bounces"].any()
    assert (got["specular"] > 0).sum() >= 50  # (the cube is followed, and flagged, with no bounce taken)
    assert np.array_equal(got["specular"] > 0, reference(s_cube, W, H, SPP, SEED)["specular"] > 0)


def test_reflected_ray_is_the_scattered_ray_of_a_roughness_0_metal():
    scene = rtgo.Scene.from_json_text(text(S_MIRROR))
    hittables, mats = hittables_with_materials(scene)
    frame = [float(c) for c in rtgo.camera_frame(scene, rtgo.RT_CAMERA_REFERENCE, W, H)]
    seen = {CUBE_1: 0, CUBE_2: 0}
    for y in range(0, H, 2):
        for x in range(0, W, 3):
            o, d = camera_ray(frame, W, H, SEED, x, y, 0)
            links, _ = chain(hittables, mats, o, d, 4, 0.1)
            for (idx, rec, ro, rd), nxt in zip(links, links[1:]):
                if idx not in seen:
                    continue
                mat = scene.view.objects[idx].material
                assert mat.kind == rtgo.MATERIAL_KINDS["metal"] and mat.roughness == 0.0
                ok, sd, _, draws = oracle.scatter(mat, ro, rd, rec, seed=SEED, pixel=y * W + x, sample=0)
                assert ok and draws == 0, (x, y)
                assert np.array_equal(np.array(nxt[3]).view(np.uint64), np.array(sd).view(np.uint64)), (x, y, idx)
                assert np.array_equal(np.array(nxt[2]).view(np.uint64), np.array(rec[1:4]).view(np.uint64))
                seen[idx] += 1
    assert seen[CUBE_1] >= 20 and seen[CUBE_2] >= 20, seen
