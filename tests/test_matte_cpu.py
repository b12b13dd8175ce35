"""Matte layers and the edge resolve (rt_context_render_matte_async,
rt_matte_resolve_host), CPU: the declarations and their ctypes
mirrors, the Python restatement of the matte (tests/matte_reference.py) held to
aov_reference on its own, conditions on that restatement alone so that no
comparison passes vacuously, the host resolve held bit for bit to the numpy
restatement, the refused calls, the Python layer's refusals before any device
call, a stand-alone sanitizer run of include/rt_matte.h, and what the feature is
for: a denoised one-sample frame comes closer to a 512-sample render once its
silhouettes are resolved (figures in DESIGN.md §4.19)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import matte_quality as mq
import rtgo
from aov_reference import reference as aov_reference
from conftest import ROOT
from matte_reference import (NEG_NAN, SYN_SIZES, bits, keys, matte_of, overflow_scene, parts_of, reference, resolve,
                             syn_inputs)
from sequence_cases import scene_json

HEADER = os.path.join(ROOT, "include", "rt_api.h")
RT_E_INVALID = -1
FUNCS = ["rt_matte_default", "rt_context_render_matte_async", "rt_matte_resolve_default", "rt_matte_resolve_async",
         "rt_matte_resolve_host"]
S_CUBE = scene_json("S_CUBE")


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


def _tonemapped(lin):
    out = np.zeros(lin.shape[:2] + (4,), np.uint8)
    lin = np.ascontiguousarray(lin)
    rtgo.lib().rt_tonemap_rgba(lin.ctypes.data, lin.shape[0] * lin.shape[1], out.ctypes.data)
    return out


def test_declared_exported_and_version_stays_8():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(rtgo.LIB_PATH)
    for f in FUNCS:
        assert re.search(r"^[\w \*]+\b%s\s*\(" % f, text, flags=re.M), f
        assert hasattr(lib, f) and f in rtgo.EXPORTED_SYMBOLS, f
    for t in ("rt_matte", "rt_matte_buffers", "rt_matte_resolve", "rt_matte_resolve_inputs"):
        assert re.search(r"\}\s*%s\s*;" % t, text), t
    for name, value in (("RT_MATTE_SLOTS", 16), ("RT_MATTE_MAX_RANKS", 8), ("RT_MATTE_OBJECT", 0), ("RT_MATTE_FACE", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
        assert getattr(rtgo, name) == value
    assert re.search(r"#define\s+RT_ABI_VERSION\s+8\b", text)
    assert rtgo.lib().rt_abi_version() == 8
    for name in ("Matte", "MatteBuffers", "MatteResolve", "MatteResolveInputs", "default_matte", "default_matte_resolve",
                 "matte_resolve_async", "matte_resolve_host", "matte_mask"):
        assert callable(getattr(rtgo, name)), name
    assert callable(rtgo.Context.render_matte_async) and callable(rtgo.ParallelRenderer.render_matte)
    m = rtgo.default_matte()
    assert (m.ranks, m.level) == (4, rtgo.RT_MATTE_OBJECT)
    assert rtgo.default_matte(ranks=8, level="face").level == rtgo.RT_MATTE_FACE
    r = rtgo.default_matte_resolve()
    assert r.radius == 2 and list(r.background) == [0.0, 0.0, 0.0]
    assert list(rtgo.default_matte_resolve(radius=4, background=(0.5, 0.25, 1)).background) == [0.5, 0.25, 1.0]
    for bad in (dict(slots=3), dict(level="triangle")):
        with pytest.raises(rtgo.RenderError):
            rtgo.default_matte(**bad)
    with pytest.raises(rtgo.RenderError):
        rtgo.default_matte_resolve(sigma=1)


def test_ctypes_signatures_and_struct_layouts_match_c(tmp_path):
    L = rtgo.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    P = ctypes.POINTER
    assert (L.rt_context_render_matte_async.restype, list(L.rt_context_render_matte_async.argtypes)) == (
        ctypes.c_int, [vp, i32, i32, P(rtgo.Settings), P(rtgo.Camera), P(rtgo.Matte), P(rtgo.MatteBuffers), vp])
    assert (L.rt_matte_resolve_async.restype, list(L.rt_matte_resolve_async.argtypes)) == (
        ctypes.c_int, [P(rtgo.MatteResolve), i32, i32, P(rtgo.MatteResolveInputs), vp, vp, vp])
    assert (L.rt_matte_resolve_host.restype, list(L.rt_matte_resolve_host.argtypes)) == (
        ctypes.c_int, [P(rtgo.MatteResolve), i32, i32, P(rtgo.MatteResolveInputs), vp, vp])
    assert (L.rt_matte_default.restype, list(L.rt_matte_default.argtypes)) == (None, [P(rtgo.Matte)])
    assert (L.rt_matte_resolve_default.restype, list(L.rt_matte_resolve_default.argtypes)) == (None, [P(rtgo.MatteResolve)])
    inc = os.path.join(ROOT, "include")
    # the declarations have exactly these types (a mismatch does not compile; compiled only, not linked)
    typ = tmp_path / "mt_type.c"
    typ.write_text('#include "rt_api.h"\n'
                   "int (*const f1)(rt_context*, int32_t, int32_t, const rt_settings*, const rt_camera*, const rt_matte*,\n"
                   "                const rt_matte_buffers*, void*) = rt_context_render_matte_async;\n"
                   "int (*const f2)(const rt_matte_resolve*, int32_t, int32_t, const rt_matte_resolve_inputs*, float*,\n"
                   "                uint8_t*, void*) = rt_matte_resolve_async;\n"
                   "int (*const f3)(const rt_matte_resolve*, int32_t, int32_t, const rt_matte_resolve_inputs*, float*,\n"
                   "                uint8_t*) = rt_matte_resolve_host;\n"
                   "void (*const f4)(rt_matte*) = rt_matte_default;\n"
                   "void (*const f5)(rt_matte_resolve*) = rt_matte_resolve_default;\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", inc, "-c", str(typ), "-o", str(tmp_path / "mt_type.o")],
                   check=True)
    structs = {"rt_matte": (rtgo.Matte, 8), "rt_matte_buffers": (rtgo.MatteBuffers, 24),
               "rt_matte_resolve": (rtgo.MatteResolve, 32), "rt_matte_resolve_inputs": (rtgo.MatteResolveInputs, 48)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_api.h"', "int main(void) {"]
    for c, (py, _) in structs.items():
        lines.append(f'printf("{c} sizeof %zu\\n", sizeof({c}));')
        lines += [f'printf("{c} {n} %zu\\n", offsetof({c}, {n}));' for n, _ in py._fields_]
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "mt_layout.c", tmp_path / "mt_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = {tuple(ln.split()[:2]): int(ln.split()[2])
           for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    for c, (py, size) in structs.items():
        assert got[(c, "sizeof")] == ctypes.sizeof(py) == size, c
        for n, _ in py._fields_:
            assert got[(c, n)] == getattr(py, n).offset, (c, n)


# ---- the restatement of the matte, on its own
def test_the_restatement_agrees_with_the_first_hit_reference():
    w, h, n, seed = 72, 48, 4, 3
    aov = aov_reference(S_CUBE, w, h, n, seed)
    for level in ("object", "face"):
        for ranks in (1, 4):
            m = reference(S_CUBE, w, h, n, seed, ranks, level)
            total = m["count"].sum(axis=0) + m["rest"]
            assert np.array_equal(total, m["hits"])
            assert np.array_equal(total, np.rint(aov["coverage"].astype(np.float64) * n).astype(np.int32)), (level, ranks)
            assert (m["count"][:-1] >= m["count"][1:]).all() and ((m["id"] < 0) == (m["count"] == 0)).all()
    m = reference(S_CUBE, w, h, n, seed, 4, "object")
    one = m["used"] == 1  # a pixel that sees one object: rank 0 is the first-hit pass's d_object
    assert one.sum() > 400 and np.array_equal(m["id"][0][one], aov["object"][one])
    assert np.array_equal(m["hits"] == 0, aov["object"] < 0)
    f = reference(S_CUBE, w, h, n, seed, 4, "face")
    cube = (f["id"] >= 3 * 16) & (f["count"] > 0)  # object 3 is the cube: keys 48..59
    assert cube.any() and (f["id"][cube] < 3 * 16 + 12).all() and len(np.unique(f["id"][cube])) >= 4
    assert (f["id"][(f["count"] > 0) & ~cube] % 16 == 0).all()  # (a sphere's f is 0)
    assert np.array_equal(f["id"][0][one] // 16, m["id"][0][one])
    # a smaller sample count is a prefix of the same walk
    assert all(np.array_equal(matte_of(keys(S_CUBE, w, h, n, seed), 2)[k], reference(S_CUBE, w, h, 2, seed)[k])
               for k in ("id", "count", "rest"))


def test_conditions_on_the_restatement_alone():
    """Nothing below passes vacuously: an overflowing pixel, a tie that the key order decides, more slots than
    ranks, and enough mixed pixels for the quality figures."""
    o = reference(overflow_scene(), 2, 2, 64, 3)
    print("overflow scene: used", o["used"].tolist(), "overflow", o["overflow"].tolist(), "rest", o["rest"].tolist())
    assert (o["overflow"] > 0).any() and (o["used"] == 16).any()
    assert (o["hits"] == 0).any()  # (and a pixel that sees nothing at all)
    assert np.array_equal(o["count"].sum(axis=0) + o["rest"], o["hits"])
    m = reference(S_CUBE, 72, 48, 17, 3, 2, "face")
    assert (m["used"] > 2).any() and (m["rest"] > 0).any()  # (three faces in a pixel, two ranks: one is dropped)
    m = reference(S_CUBE, 72, 48, 2, 3, 2, "face", walk_samples=17)
    assert m["tie"].any() and (m["id"][0][m["tie"]] < m["id"][1][m["tie"]]).all()  # (1 : 1, the smaller key first)
    assert o["tie"].any() and (o["used"] > 4).any()
    m16 = matte_of(keys(mq.scene_text("S_CUBE"), mq.QW, mq.QH, mq.MATTE_SPP, 3), mq.MATTE_SPP)
    mixed = int((parts_of(m16["count"], m16["rest"], mq.MATTE_SPP) >= 2).sum())
    assert mixed >= 250, mixed


# ---- the host resolve against the numpy restatement
@pytest.mark.parametrize("with_rest", [True, False], ids=["rest", "no rest"])
@pytest.mark.parametrize("size", SYN_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_resolve_equals_the_numpy_restatement_bit_for_bit(size, with_rest):
    w, h = size
    radius = 4 if (w, h) == (5, 3) else 2  # (5x3 at radius 4: the window is larger than the image)
    n, bg = 8, (0.25, 0.0, 1.5)
    color, obj, ids, count, rest = syn_inputs(w, h)
    rest = rest if with_rest else None
    want = resolve(color, obj, ids, count, rest, n, radius, bg)
    parts = parts_of(count, rest, n)
    if w * h > 1:
        assert (parts >= 2).any() and (parts < 2).any()
        assert not np.isfinite(color).all() and (bits(color) == bits(np.array(NEG_NAN))).any()
        assert (bits(want) != bits(color)).any()
    got, rgba = rtgo.matte_resolve_host(color, obj, ids, count, rest, n, dict(radius=radius, background=bg))
    _same(got, want, (size, with_rest))
    _same(got[parts < 2], color[parts < 2], "unmixed pixels keep their bits")
    assert rgba.tobytes() == _tonemapped(got).tobytes() and (rgba[..., 3] == 255).all()


def test_host_resolve_every_radius_and_single_outputs():
    w, h, n = 5, 3, 8
    color, obj, ids, count, rest = syn_inputs(w, h)
    lib, keep = rtgo.lib(), []
    for radius in (1, 2, 3, 4):
        want = resolve(color, obj, ids, count, rest, n, radius)
        got, _ = rtgo.matte_resolve_host(color, obj, ids, count, rest, n, dict(radius=radius))
        _same(got, want, radius)
    # one output at a time: the other is not needed
    p = rtgo.default_matte_resolve()
    inp = rtgo.MatteResolveInputs(color.ctypes.data, obj.ctypes.data, ids.ctypes.data, count.ctypes.data,
                                  rest.ctypes.data, 3, n)
    lin, rgba = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 4), np.uint8)
    assert lib.rt_matte_resolve_host(ctypes.byref(p), w, h, ctypes.byref(inp), lin.ctypes.data, None) == 0
    assert lib.rt_matte_resolve_host(ctypes.byref(p), w, h, ctypes.byref(inp), None, rgba.ctypes.data) == 0
    _same(lin, resolve(color, obj, ids, count, rest, n, 2), "out_linear alone")
    assert rgba.tobytes() == _tonemapped(lin).tobytes()
    keep.append(inp)


def test_a_single_pixel_with_a_nan_colour_and_a_miss_part():
    color = np.full((1, 1, 3), NEG_NAN, np.float32)
    obj = np.array([[2]], np.int32)
    ids, count = np.array([[[2]], [[5]]], np.int32), np.array([[[3]], [[1]]], np.int32)
    for bg in ((0.0, 0.0, 0.0), (4.0, 2.0, 1.0)):
        got, _ = rtgo.matte_resolve_host(color, obj, ids, count, None, 8, dict(background=bg))
        _same(got, resolve(color, obj, ids, count, None, 8, 2, bg), bg)
    color = np.array([[[1.0, 2.0, 4.0]]], np.float32)
    got, _ = rtgo.matte_resolve_host(color, obj, ids, count, None, 8, dict(background=(4.0, 2.0, 1.0)))
    # 3/8 own (gathered from itself), 1/8 own (object 5 has no tap), 4/8 background
    assert got[0, 0].tolist() == [0.5 * 1.0 + 0.5 * 4.0, 2.0, 0.5 * 4.0 + 0.5 * 1.0]


def test_invalid_arguments_are_refused_and_touch_nothing():
    lib = rtgo.lib()
    w, h, n = 5, 3, 8
    color, obj, ids, count, rest = syn_inputs(w, h)
    lin = np.full((h, w, 3), -1234.5, np.float32)
    rgba = np.full((h, w, 4), 0xA5, np.uint8)
    R = rtgo.default_matte_resolve
    nan, inf = float("nan"), float("inf")
    A = lambda a: a.ctypes.data if a is not None else None

    def call(params=R(), w=w, h=h, inputs=True, color_in=color, obj_in=obj, ids_in=ids, count_in=count, rest_in=rest,
             ranks=3, samples=n, lin_out=lin, rgba_out=rgba, entry=lib.rt_matte_resolve_host):
        inp = rtgo.MatteResolveInputs(A(color_in), A(obj_in), A(ids_in), A(count_in), A(rest_in), ranks, samples)
        args = [ctypes.byref(params) if params is not None else None, w, h, ctypes.byref(inp) if inputs else None,
                A(lin_out), A(rgba_out)]
        return entry(*args) if entry is lib.rt_matte_resolve_host else entry(*args, None)

    cases = {
        "NULL params": dict(params=None), "NULL inputs": dict(inputs=False), "NULL color": dict(color_in=None),
        "NULL object": dict(obj_in=None), "NULL id": dict(ids_in=None), "NULL count": dict(count_in=None),
        "both outputs NULL": dict(lin_out=None, rgba_out=None), "out == color": dict(lin_out=color),
        "w = 0": dict(w=0), "h = -1": dict(h=-1), "h = 65537": dict(h=65537), "too many pixels": dict(w=65536, h=65536),
        "ranks 0": dict(ranks=0), "ranks 9": dict(ranks=9), "samples 0": dict(samples=0), "samples -4": dict(samples=-4),
        "radius 0": dict(params=R(radius=0)), "radius 5": dict(params=R(radius=5)), "radius -1": dict(params=R(radius=-1)),
        "background NaN": dict(params=R(background=(0, nan, 0))), "background inf": dict(params=R(background=(inf, 0, 0))),
        "background -inf": dict(params=R(background=(0, 0, -inf))),
    }
    before = color.copy()
    for entry in (lib.rt_matte_resolve_host, lib.rt_matte_resolve_async):  # (async: refused before any device)
        tag = b"rt_matte_resolve_host" if entry is lib.rt_matte_resolve_host else b"rt_matte_resolve_async"
        for what, kw in cases.items():
            assert call(entry=entry, **kw) == RT_E_INVALID, (what, entry.__name__)
            msg = lib.rt_last_error()
            assert msg and tag in msg, what
            assert (lin == -1234.5).all() and (rgba == 0xA5).all() and bits(color).tobytes() == bits(before).tobytes(), what
    assert call() == 0  # (the same call with nothing wrong)
    _same(lin, resolve(color, obj, ids, count, rest, n, 2), "after the refused calls")
    assert call(rest_in=None) == 0 and call(lin_out=None) == 0 and call(rgba_out=None) == 0
    assert call(ranks=1) == 0 and call(params=R(radius=4, background=(1e300, -1e300, 0))) == 0
    for bad in (dict(radius=9), dict(sigma=1.0)):
        with pytest.raises(rtgo.RenderError):
            rtgo.matte_resolve_host(color, obj, ids, count, rest, n, bad)
    with pytest.raises(rtgo.RenderError):
        rtgo.matte_resolve_host(color, obj[:, :2], ids, count, rest, n)


def test_matte_mask_and_the_python_layers_refusals_before_any_device():
    matte = {"id": np.array([[[1, 2]], [[2, -1]]], np.int32),
             "coverage": np.array([[[0.75, 1.0]], [[0.25, 0.0]]], np.float32)}
    assert rtgo.matte_mask(matte, 2).tolist() == [[0.25, 1.0]] and rtgo.matte_mask(matte, 1).tolist() == [[0.75, 0.0]]
    assert rtgo.matte_mask(matte, 7).tolist() == [[0.0, 0.0]] and rtgo.matte_mask(matte, 2).dtype == np.float32
    r = rtgo.ParallelRenderer(1)
    r.set_samples(1)
    scene = rtgo.Scene.from_json_text(S_CUBE)
    cams = [dict(mq.CAMERA), dict(mq.CAMERA)]
    for bad in (dict(sigma=1), "default", 0, dict(samples=0), dict(ranks=9), 2.5):
        with pytest.raises(rtgo.RenderError, match="matte"):
            r.render_denoised(scene, 8, 8, matte=bad)
        with pytest.raises(rtgo.RenderError, match="matte"):
            r.render_sequence(scene, 8, 8, cams, temporal=True, matte=bad)
    with pytest.raises(rtgo.RenderError, match="matte"):
        r.render_sequence(scene, 8, 8, cams, matte=True)  # (needs temporal)
    with pytest.raises(rtgo.RenderError, match="matte"):
        r.render_progressive(scene, 8, 8, 1, matte=True)  # (needs denoise)
    for bad in (dict(samples=0), dict(ranks=0), dict(ranks=9), dict(level="edge"), dict(width=0)):
        kw = dict(dict(width=8, height=8), **bad)
        with pytest.raises(rtgo.RenderError):
            r.render_matte(scene, kw.pop("width"), kw.pop("height"), **kw)


# ---- include/rt_matte.h under the host sanitizers: a stand-alone program, nothing is loaded into Python
def test_slots_ranking_and_resolve_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no g++ (the compiler of the suite's other sanitizer programs)"
    src = os.path.join(ROOT, "tests", "c", "matte_sanitize.cpp")
    exe = str(tmp_path / "matte_sanitize")
    # (the runtimes are linked INTO the program, so it runs in whatever environment the machine sets)
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
    assert "matte_sanitize ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


# ---- quality: 1 spp -> rt_denoise_host -> rt_matte_resolve_host at 144x96 against 512 samples (tests/matte_quality.py)
BOUND = {"S_CUBE": 0.492, "C_FLOOR": 0.754}


@pytest.mark.parametrize("name", ["S_CUBE", "C_FLOOR"])
def test_quality_resolved_silhouettes_come_closer_to_the_converged_frame(name):
    """Measured on the host twin, whole-image RMSE against 512 samples, denoised -> resolved with a
    16-sample matte, and the ratio:
      S_CUBE   seed 3: 0.00834 -> 0.00373 (0.447)   seed 4: 0.00836 -> 0.00347 (0.415)   seed 5: 0.00869 -> 0.00341 (0.392)
      C_FLOOR  seed 3: 0.00887 -> 0.00608 (0.685)   seed 4: 0.00944 -> 0.00567 (0.600)   seed 5: 0.00885 -> 0.00590 (0.667)
    The bound is the worst of the three seeds times 1.1 (0.447 * 1.1 = 0.492, 0.685 * 1.1 = 0.754): the inputs are
    deterministic, the margin covers another seed.  Edge pixels (a 4-neighbour of another object), seed 3: S_CUBE 593
    pixels 0.0389 -> 0.0146, C_FLOOR 336 pixels 0.0464 -> 0.0209.  With fewer matte samples, seed 3 / 4 / 5:
      S_CUBE   8 samples 0.526 / 0.495 / 0.466    4 samples 0.593 / 0.635 / 0.562
      C_FLOOR  8 samples 0.705 / 0.645 / 0.702    4 samples 0.783 / 0.694 / 0.765"""
    for seed in mq.SEEDS:
        fig = mq.figures(name, seed)
        den, out = fig["image"]
        print(f"{name} seed {seed}: image {den:.5f} -> {out:.5f} ratio {out / den:.3f}; edge pixels ({fig['edge'][2]}) "
              f"{fig['edge'][0]:.4f} -> {fig['edge'][1]:.4f}; {fig['mixed']} mixed pixels")
        assert fig["unmixed_same"], (name, seed)  # (a pixel with fewer than two parts is not changed at all)
        assert fig["mixed"] >= 100, (name, seed, fig["mixed"])
        assert out / den < BOUND[name], (name, seed, out / den)
    for samples in (8, 4):  # (recorded, not bounded)
        fig = mq.figures(name, 3, samples)
        print(f"{name} seed 3, {samples} matte samples: ratio {fig['image'][1] / fig['image'][0]:.3f}")


def test_quality_after_six_accumulated_frames_is_recorded():
    """Recorded, S_CUBE from a camera that moves 0.05 per frame, six one-sample frames through
    rt_temporal_host, the last one through rt_denoise_host, then resolved with that frame's 16-sample matte:
    0.01021 -> 0.00313 (ratio 0.306; 8 samples 0.403, 4 samples 0.480).  The history smears the silhouettes the
    camera moved across, so there is MORE for the resolve to repair here, not less.  No bound is set on a figure
    that was measured once; the resolve must only not hurt."""
    den, out, mixed = mq.sequence()
    print(f"six accumulated frames: image {den:.5f} -> {out:.5f} ratio {out / den:.3f}; {mixed} mixed pixels")
    assert mixed >= 100 and out < den


def test_quality_a_resolve_that_does_nothing_gains_nothing():
    """The quality test above fails for a no-op: with a one-sample matte of the frame's own seed every pixel has
    one part (its own first hit or a miss), and the output is the input to the bit."""
    fig = mq.figures("S_CUBE", 3, 1)
    assert fig["mixed"] == 0 and fig["image"][0] == fig["image"][1]
