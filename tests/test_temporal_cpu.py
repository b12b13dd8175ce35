"""Temporal accumulation (rt_temporal_host), CPU: the declarations
and their ctypes mirrors, the host function held bit for bit to the numpy
restatement of the definition (tests/temporal_reference.py), conditions on that
restatement alone so that no comparison passes vacuously, geometry that is exact
in binary64 (it pins sign, orientation and the blend without the restatement),
a static camera (the running mean), disocclusion, the refused calls, a
stand-alone sanitizer run of the per-pixel function, and what the feature is
for: over six one-sample frames of S_CUBE from a moving camera the last frame
must come closer to a 512-sample render (figures in DESIGN.md §4.14)."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import rtgo
from aov_reference import reference as aov_reference
from conftest import ROOT
from scene_cases import make_settings
from sequence_cases import at, scene_json
from temporal_reference import (ALL_FOUR, CASES, INVALID, LEFT, MECHANISMS, PARTIAL, REJECTED, bits, case_inputs,
                                case_reference, reference, synthetic)

HEADER = os.path.join(ROOT, "include", "rt_api.h")
RT_E_INVALID = -1
FUNCS = ["rt_temporal_default", "rt_temporal_async", "rt_temporal_host"]


def test_declared_exported_and_version_stays_8():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(rtgo.LIB_PATH)
    for f in FUNCS:
        assert re.search(r"^[\w \*]+\b%s\s*\(" % f, text, flags=re.M), f
        assert hasattr(lib, f) and f in rtgo.EXPORTED_SYMBOLS, f
    assert re.search(r"\}\s*rt_temporal\s*;", text) and re.search(r"\}\s*rt_temporal_frame\s*;", text)
    assert re.search(r"#define\s+RT_ABI_VERSION\s+8\b", text)
    assert rtgo.lib().rt_abi_version() == 8


def test_ctypes_signatures_and_struct_layouts_match_c(tmp_path):
    L = rtgo.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    T, F = ctypes.POINTER(rtgo.Temporal), ctypes.POINTER(rtgo.TemporalFrame)
    assert (L.rt_temporal_default.restype, list(L.rt_temporal_default.argtypes)) == (None, [T])
    assert (L.rt_temporal_async.restype, list(L.rt_temporal_async.argtypes)) == (ctypes.c_int,
                                                                                [T, i32, i32, F, F, vp, vp, vp, vp])
    assert (L.rt_temporal_host.restype, list(L.rt_temporal_host.argtypes)) == (ctypes.c_int,
                                                                              [T, i32, i32, F, F, vp, vp, vp])
    inc = os.path.join(ROOT, "include")
    # the declarations have exactly these types (a mismatch does not compile; compiled only, not linked)
    typ = tmp_path / "tp_type.c"
    typ.write_text('#include "rt_api.h"\n'
                   "void (*const f0)(rt_temporal*) = rt_temporal_default;\n"
                   "int (*const f1)(const rt_temporal*, int32_t, int32_t, const rt_temporal_frame*,\n"
                   "                const rt_temporal_frame*, float*, float*, uint8_t*, void*) = rt_temporal_async;\n"
                   "int (*const f2)(const rt_temporal*, int32_t, int32_t, const rt_temporal_frame*,\n"
                   "                const rt_temporal_frame*, float*, float*, uint8_t*) = rt_temporal_host;\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", inc, "-c", str(typ), "-o", str(tmp_path / "tp_type.o")],
                   check=True)
    structs = {"rt_temporal": (rtgo.Temporal, ["max_history", "depth_tol", "normal_min", "min_weight"]),
               "rt_temporal_frame": (rtgo.TemporalFrame, ["color", "depth", "object", "normal", "count", "frame"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_api.h"', "int main(void) {"]
    for c, (_, fields) in structs.items():
        lines.append(f'printf("{c} sizeof %zu\\n", sizeof({c}));')
        lines += [f'printf("{c} {n} %zu\\n", offsetof({c}, {n}));' for n in fields]
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "tp_layout.c", tmp_path / "tp_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = {tuple(ln.split()[:2]): int(ln.split()[2])
           for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    for c, (cls, fields) in structs.items():
        assert got[(c, "sizeof")] == ctypes.sizeof(cls), c
        assert [n for n, _ in cls._fields_] == fields, c
        for n in fields:
            assert got[(c, n)] == getattr(cls, n).offset, (c, n)


def test_defaults():
    t = rtgo.default_temporal()
    assert (t.max_history, t.depth_tol, t.normal_min, t.min_weight) == (32.0, 0.05, 0.9, 0.25)
    assert rtgo.default_temporal(max_history=4, depth_tol=0.0).max_history == 4.0
    with pytest.raises(rtgo.RenderError):
        rtgo.default_temporal(history=1)


def test_render_sequence_refuses_denoise_without_temporal_before_any_device():
    r = rtgo.ParallelRenderer(1)
    r.set_samples(1)
    with pytest.raises(rtgo.RenderError, match="needs temporal"):
        r.render_sequence(rtgo.Scene.from_json_text(scene_json("S_CUBE")), 8, 8, [at((0, 0, 3))], denoise=True)


def _tonemapped(lin):
    want = np.zeros(lin.shape[:2] + (4,), np.uint8)
    rtgo.lib().rt_tonemap_rgba(lin.ctypes.data, lin.shape[0] * lin.shape[1], want.ctypes.data)
    return want


def _same(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert got.shape == want.shape and got.dtype == want.dtype and bad.size == 0, (what, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_host_equals_the_numpy_reference_bit_for_bit(name):
    ref_color, ref_count, _ = case_reference(name)
    cur, prev, params = case_inputs(name)
    color, count, rgba = rtgo.temporal_host(cur, prev, params)
    _same(color, ref_color, (name, "color"))
    _same(count, ref_count, (name, "count"))
    # out_rgba is rt_tonemap_rgba of out_color
    assert rgba.tobytes() == _tonemapped(color).tobytes() and (rgba[..., 3] == 255).all()


def _frames(cur, prev, keep):
    """TemporalFrames over numpy arrays (kept alive in `keep`)."""
    def one(d):
        if d is None:
            return None
        a = {k: np.ascontiguousarray(d[k]) for k in ("color", "depth", "object", "normal", "count") if d.get(k) is not None}
        keep.append(a)
        return rtgo.temporal_frame(d["frame"], *[a[k].ctypes.data if k in a else None
                                                 for k in ("color", "depth", "object", "normal", "count")])
    return one(cur), one(prev)


def test_host_without_out_rgba():
    cur, prev, params = case_inputs("33x17")
    ref_color, ref_count, _ = case_reference("33x17")
    keep = []
    fc, fp = _frames(cur, prev, keep)
    h, w = cur["depth"].shape
    color, count = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    p = rtgo.default_temporal(**params)
    assert rtgo.lib().rt_temporal_host(ctypes.byref(p), w, h, ctypes.byref(fc), ctypes.byref(fp), color.ctypes.data,
                                       count.ctypes.data, None) == 0
    _same(color, ref_color, "color")
    _same(count, ref_count, "count")


def test_reference_conditions_nothing_passes_vacuously():
    cur, prev = synthetic(33, 17)
    for f in (cur, prev):
        valid = np.isfinite(f["depth"])
        assert 0.10 <= 1 - valid.mean() <= 0.30, valid.mean()
        assert set(np.unique(f["object"][valid]).tolist()) == {0, 1, 2} and (f["object"][~valid] == -1).all()
    assert prev["count"].min() >= 1 and prev["count"].max() <= 40 and len(np.unique(prev["count"])) > 20
    assert not np.array_equal(cur["frame"], prev["frame"])
    color, count, cls = case_reference("33x17")
    valid = np.isfinite(cur["depth"])
    assert ((cls == INVALID) == ~valid).all()
    # every branch holds at least 5 % of the valid pixels
    for k, what in ((ALL_FOUR, "all four taps"), (PARTIAL, "some taps"), (LEFT, "left the previous image"),
                    (REJECTED, "taps rejected")):
        share = (cls[valid] == k).mean()
        assert share >= 0.05, (what, share)
    has = (cls == ALL_FOUR) | (cls == PARTIAL)
    assert (count[has] > 1).all() and (count[has] <= 32).all() and (count[has] == 32).any() and (count[has] < 32).any()
    assert (bits(color)[has] != bits(cur["color"])[has]).any(axis=-1).all()
    for name in CASES:
        c2, _, _ = case_inputs(name)
        r2, n2, k2 = case_reference(name)
        none = (k2 == INVALID) | (k2 == LEFT) | (k2 == REJECTED)
        assert np.array_equal(bits(r2)[none], bits(c2["color"])[none]), name  # cur.color bit for bit
        assert (n2[k2 == INVALID] == 0).all() and (n2[(k2 == LEFT) | (k2 == REJECTED)] == 1).all(), name
    for name in MECHANISMS:  # switching each test off (or other parameters) changes the output
        assert (bits(case_reference(name)[0]) != bits(color)).any(), name
    assert (case_reference("prev NULL")[1] == valid).all()
    k1 = case_reference("1x1")[2]
    assert k1[0, 0] in (ALL_FOUR, PARTIAL)  # (one pixel, and it has a history)
    k70 = case_reference("70x5")[2]
    assert ((k70 == ALL_FOUR) | (k70 == PARTIAL))[:, 64:].any()  # (in the second wave of a row too)


# ---- geometry that is exact in binary64: the reference camera model, aspect ratio 2, 32 x 16, every depth 2
GW, GH = 32, 16


def _exact(move):
    rng = np.random.default_rng(8)
    q = lambda shape: (rng.integers(0, 512, shape) / 256.0).astype(np.float32)  # multiples of 2^-8 in [0, 2)
    cam_prev = {"position": [0.25, -0.5, 3], "lookAt": [0, 0, 0], "up": [0, 1, 0], "fov": 60, "aspectRatio": 2.0}
    cam_cur = dict(cam_prev, position=[cam_prev["position"][k] + move[k] for k in range(3)])
    depth = np.full((GH, GW), 2.0, np.float32)
    obj = np.zeros((GH, GW), np.int32)
    cur = dict(color=q((GH, GW, 3)), depth=depth, object=obj, frame=rtgo.camera_frame(cam_cur, "reference", GW, GH))
    prev = dict(color=q((GH, GW, 3)), depth=depth, object=obj, count=np.full((GH, GW), 3, np.float32),
                frame=rtgo.camera_frame(cam_prev, "reference", GW, GH))
    return cur, prev


def _blend4(prev, cur):
    p = prev.astype(np.float64)
    return (p + (cur.astype(np.float64) - p) / 4.0).astype(np.float32)


def test_exact_geometry_a_move_along_x():
    cur, prev = _exact((0.75, 0, 0))  # three pixels at depth 2: fx = x + 3
    color, count, _ = rtgo.temporal_host(cur, prev, {"max_history": 32})
    _same(color[:, :29], _blend4(prev["color"][:, 3:], cur["color"][:, :29]), "x <= 28")
    assert (count[:, :29] == 4).all()
    _same(color[:, 29:], cur["color"][:, 29:], "columns 29 to 31")
    assert (count[:, 29:] == 1).all()
    ref = reference(cur, prev)
    _same(color, ref[0], "reference")


def test_exact_geometry_a_move_along_y():
    cur, prev = _exact((0, 0.5, 0))  # two pixels: fy = y + 2, row 0 is the bottom
    color, count, _ = rtgo.temporal_host(cur, prev, {"max_history": 32})
    _same(color[:14], _blend4(prev["color"][2:], cur["color"][:14]), "y <= 13")
    assert (count[:14] == 4).all()
    _same(color[14:], cur["color"][14:], "the top two rows")
    assert (count[14:] == 1).all()


def _static(n, max_history, seed=21):
    rng = np.random.default_rng(seed)
    w, h = 33, 17
    cam = {"position": [3, 2, -5], "lookAt": [0.5, 0, 0.25], "up": [0.1, 1, 0.2], "fov": 50, "aspectRatio": 33 / 17}
    frame = rtgo.camera_frame(cam, "lookat", w, h)
    depth = np.full((h, w), 2.5, np.float32)
    inputs = [(rng.random((h, w, 3)) * 2).astype(np.float32) for _ in range(n)]
    state, counts, results = None, [], []
    for c in inputs:
        cur = dict(color=c, depth=depth, frame=frame)
        color, count, _ = rtgo.temporal_host(cur, state, {"max_history": max_history})
        state = dict(cur, color=color, count=count)
        counts.append(count)
        results.append(color)
    return inputs, results, counts


def test_static_camera_is_the_running_mean():
    inputs, results, counts = _static(8, 32)
    for k, c in enumerate(counts):
        assert (c == k + 1).all(), (k, np.unique(c))
    mean = np.mean(np.stack([a.astype(np.float64) for a in inputs]), axis=0)
    # each call rounds one value below 2 to float32 on store, and the neighbour taps' weights are about 1e-13
    # at most (fx is x to within rounding): 2^-22 per call bounds both with room, 8 * 2^-22 absolute in all
    err = np.abs(results[-1].astype(np.float64) - mean).max()
    print(f"static camera, 8 frames: largest |accumulated - mean| {err:.3e} (bound {8 * 2.0 ** -22:.3e})")
    assert err <= 8 * 2.0 ** -22, err
    _, _, counts4 = _static(8, 4)
    assert [float(np.unique(c)[0]) for c in counts4] == [1, 2, 3, 4, 4, 4, 4, 4]
    assert all(len(np.unique(c)) == 1 for c in counts4)


def test_disocclusion_restarts_every_pixel():
    cur, prev, _ = case_inputs("33x17")
    # (every pixel valid in both frames; the previous surface is 20 % farther than the reprojected point)
    z = np.where(np.isfinite(cur["depth"]), cur["depth"], np.float32(2.0)).astype(np.float32)
    cur = dict(cur, depth=z, frame=cur["frame"])
    prev = dict(prev, depth=(z * np.float32(1.2)).astype(np.float32), frame=cur["frame"])
    for f in (cur, prev):
        del f["object"], f["normal"]
    color, count, _ = rtgo.temporal_host(cur, prev, {"depth_tol": 0.05})
    _same(color, cur["color"], "cur.color")
    assert (count == 1).all()
    # (the same call without the depth test keeps a history: the test above is what rejected it)
    assert (rtgo.temporal_host(cur, prev, {"depth_tol": 0.0})[1] > 1).mean() > 0.9


def test_every_refused_call_leaves_the_outputs_untouched():
    lib = rtgo.lib()
    cur, prev, _ = case_inputs("33x17")
    h, w = cur["depth"].shape
    color = np.full((h, w, 3), -1234.5, np.float32)
    count = np.full((h, w), -1234.5, np.float32)
    rgba = np.full((h, w, 4), 0xA5, np.uint8)
    keep = []
    T = rtgo.default_temporal
    nan, inf = float("nan"), float("inf")

    def call(params=T(), w=w, h=h, cur_on=True, prev_on=True, color_out=color, count_out=count, cur_drop=(),
             prev_drop=(), cur_frame=None, prev_frame=None, alias=None, entry=lib.rt_temporal_host):
        c = {k: v for k, v in cur.items() if k not in cur_drop}
        p = {k: v for k, v in prev.items() if k not in prev_drop}
        if cur_frame is not None:
            c["frame"] = cur_frame
        if prev_frame is not None:
            p["frame"] = prev_frame
        fc, fp = _frames(c, p, keep)
        if alias == "color":
            fp.color = color_out.ctypes.data
        if alias == "count":
            fp.count = count_out.ctypes.data
        args = [ctypes.byref(params) if params is not None else None, w, h, ctypes.byref(fc) if cur_on else None,
                ctypes.byref(fp) if prev_on else None, color_out.ctypes.data if color_out is not None else None,
                count_out.ctypes.data if count_out is not None else None, rgba.ctypes.data]
        return entry(*args) if entry is lib.rt_temporal_host else entry(*args, None)

    def frame_with(f, i, v):
        g = np.array(f, np.float64)
        g[i] = v
        return g

    zero_h = frame_with(frame_with(frame_with(prev["frame"], 6, 0.0), 7, 0.0), 8, 0.0)
    zero_v = frame_with(frame_with(frame_with(prev["frame"], 9, 0.0), 10, 0.0), 11, 0.0)
    # lower_left = origin - horizontal / 2 - vertical / 2 (exact here) puts the centre ray at zero: aa == 0
    zero_a = np.array([0, 0, 0, -1, -0.5, 0, 2, 0, 0, 0, 1, 0], np.float64)
    cases = {
        "NULL params": dict(params=None), "NULL cur": dict(cur_on=False),
        "NULL cur.color": dict(cur_drop=("color",)), "NULL cur.depth": dict(cur_drop=("depth",)),
        "NULL prev.color": dict(prev_drop=("color",)), "NULL prev.depth": dict(prev_drop=("depth",)),
        "NULL prev.count": dict(prev_drop=("count",)),
        "object in cur only": dict(prev_drop=("object",)), "object in prev only": dict(cur_drop=("object",)),
        "normal in cur only": dict(prev_drop=("normal",)), "normal in prev only": dict(cur_drop=("normal",)),
        "NULL out_color": dict(color_out=None), "NULL out_count": dict(count_out=None),
        "out_color == prev.color": dict(alias="color"), "out_count == prev.count": dict(alias="count"),
        "w = 0": dict(w=0), "h = 0": dict(h=0), "w = -1": dict(w=-1), "h = 65537": dict(h=65537),
        "too many pixels": dict(w=65536, h=65536),
        "max_history 0.5": dict(params=T(max_history=0.5)), "max_history NaN": dict(params=T(max_history=nan)),
        "max_history inf": dict(params=T(max_history=inf)),
        "depth_tol < 0": dict(params=T(depth_tol=-0.01)), "depth_tol NaN": dict(params=T(depth_tol=nan)),
        "depth_tol inf": dict(params=T(depth_tol=inf)),
        "normal_min 1.5": dict(params=T(normal_min=1.5)), "normal_min -1.5": dict(params=T(normal_min=-1.5)),
        "normal_min NaN": dict(params=T(normal_min=nan)),
        "min_weight 0": dict(params=T(min_weight=0.0)), "min_weight 1.5": dict(params=T(min_weight=1.5)),
        "min_weight NaN": dict(params=T(min_weight=nan)),
        "NaN in cur.frame": dict(cur_frame=frame_with(cur["frame"], 4, nan)),
        "inf in cur.frame": dict(cur_frame=frame_with(cur["frame"], 0, inf)),
        "NaN in prev.frame": dict(prev_frame=frame_with(prev["frame"], 11, nan)),
        "hh == 0": dict(prev_frame=zero_h), "vv == 0": dict(prev_frame=zero_v), "aa == 0": dict(prev_frame=zero_a),
    }
    for entry in (lib.rt_temporal_host, lib.rt_temporal_async):  # (async: refused before it touches a device)
        for what, kw in cases.items():
            assert call(entry=entry, **kw) == RT_E_INVALID, (what, entry.__name__)
            msg = lib.rt_last_error()
            assert msg and (b"rt_temporal_host" if entry is lib.rt_temporal_host else b"rt_temporal_async") in msg, what
            assert (color == -1234.5).all() and (count == -1234.5).all() and (rgba == 0xA5).all(), what
    assert call() == 0  # (the same call with nothing wrong)
    _same(color, case_reference("33x17")[0], "after the refused calls")
    _same(count, case_reference("33x17")[1], "after the refused calls")
    assert (rgba[..., 3] == 255).all()
    # normal_min -1 and depth_tol 0 are in range (the tests' off values); prev NULL needs no prev rules
    assert call(params=T(normal_min=-1.0, depth_tol=0.0, min_weight=1.0, max_history=1.0)) == 0
    assert call(prev_on=False) == 0
    with pytest.raises(rtgo.RenderError):
        rtgo.temporal_host(dict(cur, depth=cur["depth"][:5]), prev)


# ---- the per-pixel function under the host sanitizers: a stand-alone program, nothing is loaded into Python
def test_per_pixel_function_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no g++ (the compiler of the suite's other sanitizer programs)"
    src = os.path.join(ROOT, "tests", "c", "temporal_sanitize.cpp")
    exe = str(tmp_path / "temporal_sanitize")
    # (float-cast-overflow is not part of "undefined": it reports the (int)floor(fx) of an fx out of range.
    # The runtimes are linked INTO the program, so it runs in whatever environment the machine sets.)
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
             "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
             "-I", os.path.join(ROOT, "include")]
    # a trivial program decides whether the sanitizer runtimes link and start here; the real source must then build
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("no sanitizer runtime links on this machine: " + (p.stderr.strip().splitlines() or ["?"])[-1])
    p = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, timeout=60)
    if p.returncode != 0:
        pytest.skip("a sanitized program does not start on this machine: " + (p.stderr.strip().splitlines() or ["?"])[-1])
    p = subprocess.run([cxx] + flags + [src, "-o", exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "temporal_sanitize ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


# ---- quality: the definition over six one-sample frames from a moving camera (the numpy reference alone)
QW, QH, QFRAMES, QSTEP = 144, 96, 6, 0.05  # (0.05 in x per frame: 0.8 pixels at the spheres' depth, 4 in all)


@functools.lru_cache(maxsize=None)
def _quality():
    state = None
    for f in range(QFRAMES):
        cam = at((QSTEP * f, 0, 3))
        text = scene_json("S_CUBE", cam)
        scene = rtgo.Scene.from_json_text(text)
        noisy, _, _ = oracle.render(scene, QW, QH, make_settings(rtgo, {"samples": 1, "max_depth": 50}, 3 + f))
        feat = aov_reference(text, QW, QH, 1, 3 + f)
        cur = dict(color=noisy.astype(np.float32), depth=feat["depth"], object=feat["object"], normal=feat["normal"],
                   frame=rtgo.camera_frame(cam, "reference", QW, QH))
        host = rtgo.temporal_host(cur, state)
        color, count, _ = reference(cur, state)
        assert np.array_equal(bits(host[0]), bits(color)) and np.array_equal(bits(host[1]), bits(count)), f
        state = dict(cur, color=color, count=count)
    truth, _, _ = oracle.render(scene, QW, QH, make_settings(rtgo, {"samples": 512, "max_depth": 50}, 77))
    return cur["color"], color, count, feat["object"], truth.astype(np.float64)


def test_quality_over_six_one_sample_frames_of_s_cube():
    """Measured: whole image 0.01073 -> 0.00857 (ratio 0.799); object 0 (metal sphere) 0.857,
    object 1 (the Lambertian sphere, 305 pixels) 0.03606 -> 0.02283 (ratio 0.633), object 2 0.707, object 3
    (the metal cube) 0.921.  The bound on object 1 is the midpoint between 0.633 and 1: half the gain, kept
    as margin against a different seed."""
    noisy, out, count, obj, truth = _quality()
    assert np.isfinite(out).all()

    def rmse(img, mask=None):
        d = (img.astype(np.float64) - truth) ** 2
        return float(np.sqrt((d if mask is None else d[mask]).mean()))

    whole = rmse(out) / rmse(noisy)
    sphere = obj == 1  # the Lambertian sphere
    assert int(sphere.sum()) >= 300, int(sphere.sum())
    part = rmse(out, sphere) / rmse(noisy, sphere)
    print(f"whole image {rmse(noisy):.5f} -> {rmse(out):.5f} ratio {whole:.3f}; "
          f"object 1 ({int(sphere.sum())} pixels) {rmse(noisy, sphere):.5f} -> {rmse(out, sphere):.5f} ratio {part:.3f}")
    for k in range(4):
        m = obj == k
        if m.any():
            print(f"object {k}: {int(m.sum())} pixels, {rmse(noisy, m):.5f} -> {rmse(out, m):.5f} "
                  f"ratio {rmse(out, m) / rmse(noisy, m):.3f}, mean history {float(count[m].mean()):.2f}")
    assert whole < 1.0, whole
    assert part < 0.817, part
    assert float(count[sphere].mean()) > 4  # (most of the sphere kept its history over the six frames)
