"""The opt-in look-at camera on the host (no GPU): rt_camera_frame's two
models, rt_validate's look-at checks, the default and the CLI flag.

The frame is origin, lower_left, horizontal, vertical (include/rt_api.h
rt_camera_frame).  The reference model is getRay's (renderer.go:377-390);
the look-at model with the camera looking down -Z, up +Y and fov 90 must
give the very same numbers, because the GPU checks compare such a render
with the oracle byte for byte."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rtgo
from conftest import ROOT, SCENES

REF, LOOKAT = rtgo.RT_CAMERA_REFERENCE, rtgo.RT_CAMERA_LOOKAT
GENERAL = {"position": [3, 2, -5], "lookAt": [0.5, 0, 0.25], "up": [0.1, 1, 0.2], "fov": 50, "aspectRatio": 4 / 3}
POSITIONS = [(0.0, 0.5, 6.0), (-3.25, 7.0, 0.1), (0.0, 0.0, 0.0), (1e5, -2.5e3, 17.0)]
ASPECTS = [1.5, 1.78, 4 / 3, 1.0]


def reference_frame(pos, aspect):
    """getRay's numbers as make_cam has always computed them."""
    cx, cy, cz = (np.float64(v) for v in pos)
    vw = np.float64(2.0) * np.float64(aspect)
    return np.array([cx, cy, cz, cx - vw / 2, cy - 1, cz - 1, vw, 0, 0, 0, 2, 0], np.float64)


def numpy_lookat_frame(cam, w, h):
    """The look-at formulas of include/rt_api.h in numpy float64, same order."""
    pos, la, up = (np.array(cam[k], np.float64) for k in ("position", "lookAt", "up"))

    def norm(v):
        return v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])

    wv = norm(pos - la)
    U = norm(cross(up, wv))
    V = cross(wv, U)
    fov = np.float64(cam["fov"])
    hh = np.float64(1.0) if fov == 90 else np.tan(fov * (np.pi / 360))
    a = np.float64(cam.get("aspectRatio", 0.0))
    if a == 0:
        a = np.float64(w) / np.float64(h)
    vh = 2.0 * hh
    vw = vh * a
    hor, ver = U * vw, V * vh
    ll = pos - hor / 2 - ver / 2 - wv
    return np.concatenate([pos, ll, hor, ver]), (U, V, wv)


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("aspect", ASPECTS)
def test_reference_model_is_get_ray_bit_for_bit(pos, aspect):
    cam = {"position": list(pos), "lookAt": [9, 9, 9], "up": [0, 0, 0], "fov": 60, "aspectRatio": aspect}
    got = rtgo.camera_frame(cam, REF, 64, 48)
    assert got.tobytes() == reference_frame(pos, aspect).tobytes()
    assert rtgo.camera_frame(cam, "reference", 7, 5).tobytes() == got.tobytes()


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("aspect", ASPECTS)
def test_identity_lookat_equals_the_reference_frame(pos, aspect):
    p = np.array(pos, np.float64)
    la = p + np.array([0, 0, -1.0])
    assert np.array_equal(p - la, np.array([0, 0, 1.0]))  # exactly: the premise of the GPU byte comparisons
    cam = {"position": list(pos), "lookAt": la.tolist(), "up": [0, 1, 0], "fov": 90, "aspectRatio": aspect}
    got = rtgo.camera_frame(cam, LOOKAT, 64, 48)
    assert np.all(got == reference_frame(pos, aspect))  # (==: -0 and +0 are equal)


# looking down dz with up dy: the frame is the reference frame of the camera
# at position * flip, with the same components negated
HALF_TURNS = [("plusZ_upY", +1, +1, (-1, 1, -1)), ("minusZ_downY", -1, -1, (-1, -1, 1)),
              ("plusZ_downY", +1, -1, (1, -1, -1))]


@pytest.mark.parametrize("name,dz,uy,flip", HALF_TURNS, ids=[t[0] for t in HALF_TURNS])
@pytest.mark.parametrize("pos", POSITIONS)
def test_half_turns_are_the_reference_frame_of_the_turned_position(name, dz, uy, flip, pos):
    aspect = 1.5
    p = np.array(pos, np.float64)
    la = p + np.array([0, 0, float(dz)])
    assert np.array_equal(p - la, np.array([0, 0, -float(dz)]))
    cam = {"position": list(pos), "lookAt": la.tolist(), "up": [0, float(uy), 0], "fov": 90, "aspectRatio": aspect}
    got = rtgo.camera_frame(cam, LOOKAT, 64, 48).reshape(4, 3)
    f = np.array(flip, np.float64)
    want = reference_frame(tuple(p * f), aspect).reshape(4, 3) * f
    assert np.all(got == want)


def test_general_camera_matches_numpy_and_is_orthonormal():
    w, h = 48, 36
    got = rtgo.camera_frame(GENERAL, LOOKAT, w, h)
    want, (U, V, wv) = numpy_lookat_frame(GENERAL, w, h)
    # a dozen correctly rounded operations of at most 2^-53 each on a well-conditioned camera
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    o, ll, hor, ver = got.reshape(4, 3)
    hh = np.tan(50 * (np.pi / 360))
    gU, gV = hor / (2 * hh * (4 / 3)), ver / (2 * hh)
    gW = o - hor / 2 - ver / 2 - ll
    for a in (gU, gV, gW):
        assert abs(np.dot(a, a) - 1) < 1e-14
    for a, b in ((gU, gV), (gU, gW), (gV, gW)):
        assert abs(np.dot(a, b)) < 1e-14
    # looking from position towards lookAt: -w points at the target
    to = np.array(GENERAL["lookAt"]) - np.array(GENERAL["position"])
    assert np.dot(-gW, to / np.linalg.norm(to)) > 1 - 1e-14
    assert np.array_equal(o, np.array(GENERAL["position"], np.float64))


def test_aspect_ratio_zero_uses_width_over_height():
    cam = dict(GENERAL, aspectRatio=0.0)
    a = rtgo.camera_frame(cam, LOOKAT, 48, 36)
    b = rtgo.camera_frame(dict(GENERAL, aspectRatio=48 / 36), LOOKAT, 48, 36)
    assert a.tobytes() == b.tobytes()
    c = rtgo.camera_frame(cam, LOOKAT, 64, 48)  # the same ratio from another size
    assert c.tobytes() == a.tobytes()
    d = rtgo.camera_frame(cam, LOOKAT, 50, 20)
    assert np.linalg.norm(d[6:9]) / np.linalg.norm(d[9:12]) == pytest.approx(2.5, rel=1e-15)


def _scene(cam):
    objs = [{"type": "sphere", "position": [0, 0, 0], "radius": 1, "material": {"type": "lambertian",
                                                                                   "color": [0.5, 0.5, 0.5]}}]
    return rtgo.Scene.from_python(cam, objs, [])


def _validate(cam, model, w=64, h=48):
    st = rtgo.default_settings()
    st.camera = model
    s = _scene(cam)
    rc = rtgo.lib().rt_validate(ctypes.byref(s.view), w, h, ctypes.byref(st))
    return rc, (rtgo.lib().rt_last_error() or b"").decode()


nan, inf = float("nan"), float("inf")
DEGENERATE = {
    "nan_position": dict(GENERAL, position=[nan, 2, -5]),
    "inf_look_at": dict(GENERAL, lookAt=[0.5, inf, 0.25]),
    "nan_up": dict(GENERAL, up=[0.1, nan, 0.2]),
    "nan_fov": dict(GENERAL, fov=nan),
    "inf_aspect": dict(GENERAL, aspectRatio=inf),
    "position_is_look_at": dict(GENERAL, lookAt=GENERAL["position"]),
    # (an axis-aligned view: w = (0, 0, -1) exactly, so the cross product is exactly zero)
    "up_parallel_to_view": dict(GENERAL, lookAt=[3, 2, 0], up=[0, 0, 2.0]),
    "up_antiparallel": dict(GENERAL, lookAt=[3, 2, 0], up=[0, 0, -0.5]),
    "zero_up": dict(GENERAL, up=[0, 0, 0]),
    "fov_zero": dict(GENERAL, fov=0.0),
    "fov_negative": dict(GENERAL, fov=-30.0),
    "fov_180": dict(GENERAL, fov=180.0),
    "fov_270": dict(GENERAL, fov=270.0),
    "negative_aspect": dict(GENERAL, aspectRatio=-1.5),
}


@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_cameras_are_invalid_in_lookat_mode_only(name):
    cam = DEGENERATE[name]
    rc, msg = _validate(cam, LOOKAT)
    assert rc == -1 and "camera" in msg, (rc, msg)  # RT_E_INVALID with a message
    rc, _ = _validate(cam, REF)
    assert rc == 0  # the reference model reads none of these (a non-finite position or aspect renders as ever)
    with pytest.raises(rtgo.RenderError):
        rtgo.camera_frame(cam, LOOKAT, 64, 48)


def test_valid_cameras_and_unknown_models():
    assert _validate(GENERAL, LOOKAT)[0] == 0
    assert _validate(GENERAL, REF)[0] == 0
    for bad in (2, -1, 7):
        rc, msg = _validate(GENERAL, bad)
        assert rc == -1 and "camera" in msg
        with pytest.raises(rtgo.RenderError):
            rtgo.camera_frame(GENERAL, bad, 64, 48)
    assert rtgo.lib().rt_camera_frame(None, REF, 8, 8, None) == -1


def test_default_is_the_reference_camera_and_the_struct_keeps_its_size():
    st = rtgo.default_settings()
    assert st.camera == rtgo.RT_CAMERA_REFERENCE == 0 and rtgo.RT_CAMERA_LOOKAT == 1
    assert ctypes.sizeof(rtgo.Settings) == 48  # as before: camera took the place of the padding word
    assert rtgo.Settings.camera.offset == 44 and rtgo.Settings.sky.offset == 40
    assert rtgo.lib().rt_abi_version() == 8
    r = rtgo.ParallelRenderer()
    assert r.settings.camera == 0
    r.set_camera("lookat")
    assert r.settings.camera == rtgo.RT_CAMERA_LOOKAT
    r.set_camera("reference")
    assert r.settings.camera == rtgo.RT_CAMERA_REFERENCE
    with pytest.raises(KeyError):
        r.set_camera("fisheye")


def test_settings_layout_matches_the_header(tmp_path):
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_api.h"\nint main(void){printf("%zu %zu %d %d %d\\n",'
                   "sizeof(rt_settings), offsetof(rt_settings, camera), RT_CAMERA_REFERENCE, RT_CAMERA_LOOKAT,"
                   "RT_ABI_VERSION);return 0;}\n")
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["48", "44", "0", "1", "8"]


EXE = os.path.join(ROOT, "concurrent-raytracer-go_amd", "build", "raytracer")
SCENE = os.path.join(SCENES, "sphere_reflections_light.json")


def test_cli_rejects_an_unknown_camera(tmp_path):
    out = tmp_path / "o.png"
    p = subprocess.run([EXE, SCENE, str(out), "8", "-3", "--camera", "foo"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1, p.stdout + p.stderr
    assert "--camera foo" in p.stderr
    assert not out.exists() and "Loading scene" not in p.stdout


@pytest.mark.parametrize("name", ["reference", "lookat"])
def test_cli_accepts_both_camera_names(tmp_path, name):
    """A size with no tile needs no device (tests/test_abi.py, the negative-size
    case): the flag is parsed, the run goes on as without it and exits 0."""
    out = tmp_path / "o.png"
    p = subprocess.run([EXE, SCENE, str(out), "8", "-3", "--camera", name], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Rendering complete!" in p.stdout and out.exists()
    q = subprocess.run([EXE, SCENE, str(tmp_path / "p.png"), "8", "-3"], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0
    assert out.read_bytes() == (tmp_path / "p.png").read_bytes()
