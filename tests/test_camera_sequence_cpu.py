"""Camera sequences, the parts that need no device:
rt_camera_orbit / rtgo.camera_orbit, the two new declarations of
include/rt_api.h against their ctypes signatures, and the argument errors of
ParallelRenderer.render_sequence that are found before a context is made."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import rtgo
from conftest import ROOT
from sequence_cases import GENERAL

HEADER = os.path.join(ROOT, "include", "rt_api.h")
RT_E_INVALID = -1
SIMPLE = {"position": [0, 0, 5], "lookAt": [0, 0, 0], "up": [0, 1, 0], "fov": 60, "aspectRatio": 1.5}


def _cam(d):
    c = rtgo.Camera()
    c.position[:] = d["position"]
    c.look_at[:] = d["lookAt"]
    c.up[:] = d["up"]
    c.fov, c.aspect_ratio = d["fov"], d["aspectRatio"]
    return c


def _orbit_rc(d, n, degrees, out_n=None):
    out = (rtgo.Camera * max(1, out_n if out_n is not None else n))()
    return rtgo.lib().rt_camera_orbit(ctypes.byref(_cam(d)), n, degrees, out), out


def test_view_zero_is_the_camera_bit_for_bit():
    for d in (SIMPLE, GENERAL):
        for n, deg in ((1, 360.0), (4, 360.0), (7, 33.5), (3, -90.0)):
            rc, out = _orbit_rc(d, n, deg)
            assert rc == 0
            assert bytes(out[0]) == bytes(_cam(d))
            assert rtgo.camera_orbit(d, n, deg)[0] == {k: (list(map(float, v)) if isinstance(v, list) else float(v))
                                                       for k, v in d.items()}
            # every other field of every view is copied
            for k in range(n):
                for f in ("look_at", "up"):
                    assert list(getattr(out[k], f)) == list(getattr(out[0], f))
                assert (out[k].fov, out[k].aspect_ratio) == (out[0].fov, out[0].aspect_ratio)


def test_a_quarter_turn_about_y():
    views = rtgo.camera_orbit(SIMPLE, 4, 360.0)
    assert len(views) == 4
    assert np.abs(np.array(views[1]["position"]) - np.array([5.0, 0.0, 0.0])).max() <= 1e-14
    assert np.abs(np.array(views[2]["position"]) - np.array([0.0, 0.0, -5.0])).max() <= 1e-14
    # the default is a full turn
    assert rtgo.camera_orbit(SIMPLE, 4) == views


def test_the_formula_in_its_stated_order():
    """position = look_at + v cos + (a x v) sin + a (a . v) (1 - cos), plain binary64, term by term."""
    n, deg = 6, 300.0
    p, la, up = (np.array(GENERAL[k], np.float64) for k in ("position", "lookAt", "up"))
    ul = math.sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2])
    a = up / ul
    v = p - la
    axv = [a[1] * v[2] - a[2] * v[1], a[2] * v[0] - a[0] * v[2], a[0] * v[1] - a[1] * v[0]]
    adv = a[0] * v[0] + a[1] * v[1] + a[2] * v[2]
    views = rtgo.camera_orbit(GENERAL, n, deg)
    for k in range(1, n):
        th = (deg * k / n) * (math.pi / 180)
        ct, st = math.cos(th), math.sin(th)
        want = [((la[i] + v[i] * ct) + axv[i] * st) + (a[i] * adv) * (1 - ct) for i in range(3)]
        assert views[k]["position"] == want, k


def test_radius_and_height_are_kept():
    p, la, up = (np.array(GENERAL[k], np.float64) for k in ("position", "lookAt", "up"))
    a = up / np.linalg.norm(up)
    r0, h0 = np.linalg.norm(p - la), float(np.dot(p - la, a))
    for k, view in enumerate(rtgo.camera_orbit(GENERAL, 12, 360.0)):
        v = np.array(view["position"]) - la
        assert abs(np.linalg.norm(v) - r0) <= 1e-12 * r0, k
        assert abs(float(np.dot(v, a)) - h0) <= 1e-12 * abs(h0), k
    # and the views are distinct
    ps = {tuple(v["position"]) for v in rtgo.camera_orbit(GENERAL, 12, 360.0)}
    assert len(ps) == 12


def test_invalid_inputs():
    assert _orbit_rc(SIMPLE, 0, 360.0, out_n=1)[0] == RT_E_INVALID
    assert _orbit_rc(SIMPLE, -3, 360.0, out_n=1)[0] == RT_E_INVALID
    assert rtgo.lib().rt_last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert _orbit_rc(SIMPLE, 4, bad)[0] == RT_E_INVALID
        for field, idx in (("position", 0), ("lookAt", 1), ("up", 2)):
            d = {k: (list(v) if isinstance(v, list) else v) for k, v in SIMPLE.items()}
            d[field][idx] = bad
            assert _orbit_rc(d, 4, 360.0)[0] == RT_E_INVALID, (field, bad)
        for field in ("fov", "aspectRatio"):
            assert _orbit_rc(dict(SIMPLE, **{field: bad}), 4, 360.0)[0] == RT_E_INVALID, (field, bad)
    assert _orbit_rc(dict(SIMPLE, up=[0, 0, 0]), 4, 360.0)[0] == RT_E_INVALID
    out = (rtgo.Camera * 2)()
    assert rtgo.lib().rt_camera_orbit(None, 2, 360.0, out) == RT_E_INVALID
    assert rtgo.lib().rt_camera_orbit(ctypes.byref(_cam(SIMPLE)), 2, 360.0, None) == RT_E_INVALID
    with pytest.raises(rtgo.RenderError):
        rtgo.camera_orbit(SIMPLE, 0)
    with pytest.raises(rtgo.RenderError):
        rtgo.camera_orbit(dict(SIMPLE, up=[0, 0, 0]), 3)


# C parameter type -> the ctypes type the binding must declare
VP = ctypes.c_void_p
CTYPES = {
    "rt_context*": VP, "int32_t": ctypes.c_int32, "const rt_settings*": ctypes.POINTER(rtgo.Settings),
    "const rt_camera*": ctypes.POINTER(rtgo.Camera), "rt_camera*": ctypes.POINTER(rtgo.Camera),
    "const uint64_t*": ctypes.POINTER(ctypes.c_uint64), "float* const*": ctypes.POINTER(VP),
    "uint8_t* const*": ctypes.POINTER(VP), "void*": VP, "double": ctypes.c_double, "int": ctypes.c_int,
}


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^([A-Za-z_][\w \*]*?)\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.M | re.S)
    assert m, name
    params = []
    for p in m.group(2).split(","):
        t = re.sub(r"\s+", " ", p.strip())
        t = re.sub(r"\s*\b\w+$", "", t)  # drop the parameter's name
        params.append(re.sub(r"\s*\*", "*", t))
    return m.group(1).strip(), params


@pytest.mark.parametrize("name", ["rt_context_render_cameras_async", "rt_camera_orbit"])
def test_ctypes_signature_matches_the_header(name):
    res, params = _declaration(name)
    f = getattr(rtgo.lib(), name)
    assert name in rtgo.EXPORTED_SYMBOLS
    assert f.restype is CTYPES[res]
    assert [CTYPES[p] for p in params] == list(f.argtypes), params
    if name == "rt_context_render_cameras_async":
        assert len(params) == 13
        # rt_context_render_frames_async with the cameras before the seeds
        _, fp = _declaration("rt_context_render_frames_async")
        assert params[:5] + params[6:] == fp


def test_abi_version_stays_8_and_max_frames():
    assert rtgo.lib().rt_abi_version() == 8
    text = open(HEADER).read()
    assert re.search(r"#define RT_MAX_FRAMES (\d+)", text).group(1) == str(rtgo.RT_MAX_FRAMES)


def test_render_sequence_argument_errors_need_no_device():
    scene = rtgo.Scene.load_from_file(os.path.join(ROOT, "scenes", "sphere_reflections_light_facing.json"))
    r = rtgo.ParallelRenderer(1, num_devices=2)
    with pytest.raises(rtgo.RenderError, match="one device"):
        r.render_sequence(scene, 8, 8, [SIMPLE])
    r = rtgo.ParallelRenderer(1, devices=[0, 0])
    with pytest.raises(rtgo.RenderError, match="one device"):
        r.render_sequence(scene, 8, 8, [SIMPLE])
    r = rtgo.ParallelRenderer(1)
    with pytest.raises(rtgo.RenderError, match="at least one camera"):
        r.render_sequence(scene, 8, 8, [])
    with pytest.raises(rtgo.RenderError, match="seeds"):
        r.render_sequence(scene, 8, 8, [SIMPLE, SIMPLE], seeds=[1])
    with pytest.raises(rtgo.RenderError, match="image size"):
        r.render_sequence(scene, 0, 8, [SIMPLE])
