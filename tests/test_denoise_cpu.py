"""À-trous denoiser (rt_denoise_host), CPU: the declarations and
their ctypes mirrors, the host function held bit for bit to the numpy
restatement of the definition (tests/denoise_reference.py), conditions on that
restatement alone so that no comparison passes vacuously, the refused calls,
and what the filter is for: on a one-sample render of S_CUBE it must bring the
image closer to a 512-sample render (figures in DESIGN.md §4.13)."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import rtgo
from aov_reference import reference as aov_reference
from conftest import ROOT
from denoise_reference import CASES, MECHANISMS, bits, case_inputs, case_reference, reference, synthetic
from scene_cases import make_settings
from sequence_cases import scene_json

HEADER = os.path.join(ROOT, "include", "rt_api.h")
RT_E_INVALID = -1
FUNCS = ["rt_denoise_default", "rt_denoise_workspace_bytes", "rt_denoise_async", "rt_denoise_host"]


def test_declared_exported_and_version_stays_8():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(rtgo.LIB_PATH)
    for f in FUNCS:
        assert re.search(r"^[\w \*]+\b%s\s*\(" % f, text, flags=re.M), f
        assert hasattr(lib, f) and f in rtgo.EXPORTED_SYMBOLS, f
    assert re.search(r"\}\s*rt_denoise\s*;", text) and re.search(r"\}\s*rt_denoise_inputs\s*;", text)
    assert re.search(r"#define\s+RT_ABI_VERSION\s+8\b", text)
    assert rtgo.lib().rt_abi_version() == 8


def test_ctypes_signatures_and_struct_layouts_match_c(tmp_path):
    L = rtgo.lib()
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_size_t
    D, I = ctypes.POINTER(rtgo.Denoise), ctypes.POINTER(rtgo.DenoiseInputs)
    assert (L.rt_denoise_default.restype, list(L.rt_denoise_default.argtypes)) == (None, [D])
    assert (L.rt_denoise_workspace_bytes.restype, list(L.rt_denoise_workspace_bytes.argtypes)) == (sz, [i32, i32])
    assert (L.rt_denoise_async.restype, list(L.rt_denoise_async.argtypes)) == (ctypes.c_int,
                                                                              [D, i32, i32, I, vp, vp, vp, sz, vp])
    assert (L.rt_denoise_host.restype, list(L.rt_denoise_host.argtypes)) == (ctypes.c_int, [D, i32, i32, I, vp, vp])
    inc = os.path.join(ROOT, "include")
    # the declarations have exactly these types (a mismatch does not compile; compiled only, not linked)
    typ = tmp_path / "dn_type.c"
    typ.write_text('#include "rt_api.h"\n'
                   "void (*const f0)(rt_denoise*) = rt_denoise_default;\n"
                   "size_t (*const f1)(int32_t, int32_t) = rt_denoise_workspace_bytes;\n"
                   "int (*const f2)(const rt_denoise*, int32_t, int32_t, const rt_denoise_inputs*, float*, uint8_t*,\n"
                   "                void*, size_t, void*) = rt_denoise_async;\n"
                   "int (*const f3)(const rt_denoise*, int32_t, int32_t, const rt_denoise_inputs*, float*,\n"
                   "                uint8_t*) = rt_denoise_host;\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", inc, "-c", str(typ), "-o", str(tmp_path / "dn_type.o")],
                   check=True)
    structs = {"rt_denoise": (rtgo.Denoise, ["levels", "normal_power", "sigma_color", "sigma_depth", "demodulate"]),
               "rt_denoise_inputs": (rtgo.DenoiseInputs, ["color", "normal", "depth", "albedo", "object"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_api.h"', "int main(void) {"]
    for c, (_, fields) in structs.items():
        lines.append(f'printf("{c} sizeof %zu\\n", sizeof({c}));')
        lines += [f'printf("{c} {n} %zu\\n", offsetof({c}, {n}));' for n in fields]
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "dn_layout.c", tmp_path / "dn_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = {tuple(ln.split()[:2]): int(ln.split()[2])
           for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    for c, (cls, fields) in structs.items():
        assert got[(c, "sizeof")] == ctypes.sizeof(cls), c
        assert [n for n, _ in cls._fields_][:len(fields)] == fields, c
        for n in fields:
            assert got[(c, n)] == getattr(cls, n).offset, (c, n)


def test_defaults_and_workspace_bytes():
    d = rtgo.default_denoise()
    assert (d.levels, d.normal_power, d.sigma_color, d.sigma_depth, d.demodulate) == (4, 32, 0.5, 0.05, 1)
    assert rtgo.default_denoise(levels=2, sigma_color=0.25).levels == 2
    with pytest.raises(rtgo.RenderError):
        rtgo.default_denoise(sigma=1)
    for w, h in ((1, 1), (33, 17), (800, 600), (1920, 1080), (65536, 8192)):
        n = rtgo.denoise_workspace_bytes(w, h)
        assert 0 < n <= 64 * w * h + 256, (w, h, n)
    for w, h in ((0, 4), (4, 0), (-1, 4), (65537, 1), (65536, 8193)):
        assert rtgo.denoise_workspace_bytes(w, h) == 0, (w, h)


def _host(name):
    inp, params = case_inputs(name)
    return rtgo.denoise_host(inp["color"], inp["normal"], inp["depth"], inp["albedo"], inp["object"], params)


@pytest.mark.parametrize("name", list(CASES))
def test_host_equals_the_numpy_reference_bit_for_bit(name):
    ref = case_reference(name)
    lin, rgba = _host(name)
    assert lin.dtype == np.float32 and lin.shape == ref.shape
    bad = np.argwhere(bits(lin) != bits(ref))
    assert bad.size == 0, (name, len(bad), bad[:4].tolist())
    # out_rgba is rt_tonemap_rgba of out_linear
    want = np.zeros(rgba.shape, np.uint8)
    rtgo.lib().rt_tonemap_rgba(lin.ctypes.data, lin.shape[0] * lin.shape[1], want.ctypes.data)
    assert rgba.tobytes() == want.tobytes() and (rgba[..., 3] == 255).all()


def test_host_in_place_and_single_outputs():
    inp, params = case_inputs("33x17 levels 3")
    ref = case_reference("33x17 levels 3")
    h, w = inp["depth"].shape
    p = rtgo.default_denoise(**params)
    color = inp["color"].copy()  # (overwritten: out_linear == color)
    di = rtgo.DenoiseInputs(color.ctypes.data, inp["normal"].ctypes.data, inp["depth"].ctypes.data,
                            inp["albedo"].ctypes.data, inp["object"].ctypes.data)
    rgba = np.zeros((h, w, 4), np.uint8)
    assert rtgo.lib().rt_denoise_host(ctypes.byref(p), w, h, ctypes.byref(di), color.ctypes.data, rgba.ctypes.data) == 0
    assert np.array_equal(bits(color), bits(ref))
    want_rgba = _host("33x17 levels 3")[1]
    assert rgba.tobytes() == want_rgba.tobytes()
    # only one output each
    di = rtgo.DenoiseInputs(*[inp[k].ctypes.data for k in ("color", "normal", "depth", "albedo", "object")])
    lin = np.zeros((h, w, 3), np.float32)
    assert rtgo.lib().rt_denoise_host(ctypes.byref(p), w, h, ctypes.byref(di), lin.ctypes.data, None) == 0
    assert np.array_equal(bits(lin), bits(ref))
    rgba2 = np.zeros((h, w, 4), np.uint8)
    assert rtgo.lib().rt_denoise_host(ctypes.byref(p), w, h, ctypes.byref(di), None, rgba2.ctypes.data) == 0
    assert rgba2.tobytes() == want_rgba.tobytes()


def test_reference_conditions_nothing_passes_vacuously():
    inp = synthetic(33, 17)
    valid = np.isfinite(inp["depth"])
    frac = 1 - valid.mean()
    assert 0.10 <= frac <= 0.30, frac
    assert set(np.unique(inp["object"][valid]).tolist()) == {0, 1, 2} and (inp["object"][~valid] == -1).all()
    assert (inp["albedo"][valid] == 0).mean() > 0.05  # (amin is exercised)
    ref = case_reference("33x17 levels 3")
    changed = (bits(ref) != bits(inp["color"])).any(axis=-1)
    assert changed[valid].mean() >= 0.90, changed[valid].mean()
    assert not changed[~valid].any()  # a pixel that is not valid is the input bit for bit
    for name in CASES:
        i2 = case_inputs(name)[0]
        r2, v2 = case_reference(name), np.isfinite(i2["depth"])
        assert np.array_equal(bits(r2)[~v2], bits(i2["color"])[~v2]), name
    for name in MECHANISMS:  # switching each mechanism off changes the output
        assert (bits(case_reference(name)) != bits(ref)).any(), name
    one = synthetic(1, 1, all_valid=True)
    assert np.isfinite(one["depth"]).all()
    # 70 x 5 at levels 8: the steps 8 .. 128 put most taps outside the image, and levels matter
    i70, p70 = case_inputs("70x5 levels 8")
    r4 = reference(i70["color"], i70["normal"], i70["depth"], i70["albedo"], i70["object"], **dict(p70, levels=4))
    assert (bits(r4) != bits(case_reference("70x5 levels 8"))).any()


def test_every_refused_call_leaves_the_outputs_untouched():
    lib = rtgo.lib()
    inp = synthetic(33, 17)
    h, w = inp["depth"].shape
    lin = np.full((h, w, 3), -1234.5, np.float32)
    rgba = np.full((h, w, 4), 0xA5, np.uint8)
    ptr = {k: inp[k].ctypes.data for k in inp}

    def call(params=rtgo.default_denoise(), w=w, h=h, inputs=True, lin=lin, rgba=rgba, **drop):
        di = rtgo.DenoiseInputs(*[None if drop.get(k) else ptr[k] for k in ("color", "normal", "depth", "albedo",
                                                                              "object")])
        return lib.rt_denoise_host(ctypes.byref(params) if params is not None else None, w, h,
                                   ctypes.byref(di) if inputs else None,
                                   lin.ctypes.data if lin is not None else None,
                                   rgba.ctypes.data if rgba is not None else None)

    D = rtgo.default_denoise
    cases = {
        "NULL params": dict(params=None), "NULL inputs": dict(inputs=False),
        "NULL color": dict(color=True), "NULL normal": dict(normal=True), "NULL depth": dict(depth=True),
        "both outputs NULL": dict(lin=None, rgba=None),
        "width 0": dict(w=0), "height 0": dict(h=0), "width -1": dict(w=-1), "height 65537": dict(h=65537),
        "too many pixels": dict(w=65536, h=65536),
        "levels 0": dict(params=D(levels=0)), "levels 9": dict(params=D(levels=9)),
        "normal_power 3": dict(params=D(normal_power=3)), "normal_power 256": dict(params=D(normal_power=256)),
        "normal_power -2": dict(params=D(normal_power=-2)),
        "sigma_color NaN": dict(params=D(sigma_color=float("nan"))),
        "sigma_color inf": dict(params=D(sigma_color=float("inf"))),
        "sigma_color < 0": dict(params=D(sigma_color=-0.5)),
        "sigma_depth NaN": dict(params=D(sigma_depth=float("nan"))),
        "sigma_depth inf": dict(params=D(sigma_depth=float("inf"))),
        "sigma_depth < 0": dict(params=D(sigma_depth=-1.0)),
        "demodulate 2": dict(params=D(demodulate=2)),
    }
    for what, kw in cases.items():
        assert call(**kw) == RT_E_INVALID, what
        assert lib.rt_last_error(), what
        assert (lin == -1234.5).all() and (rgba == 0xA5).all(), what
    assert call() == 0  # (the same call with nothing wrong)
    assert (lin != -1234.5).any() and (rgba[..., 3] == 255).all()
    # the device entry point refuses the same before it touches a device (none is needed here)
    p = rtgo.default_denoise(levels=0)
    di = rtgo.DenoiseInputs(*[ptr[k] for k in ("color", "normal", "depth", "albedo", "object")])
    assert lib.rt_denoise_async(ctypes.byref(p), w, h, ctypes.byref(di), lin.ctypes.data, None, lin.ctypes.data,
                                1 << 30, None) == RT_E_INVALID
    p = rtgo.default_denoise()
    assert lib.rt_denoise_async(ctypes.byref(p), w, h, ctypes.byref(di), lin.ctypes.data, None, None, 1 << 30,
                                None) == RT_E_INVALID


# ---- quality: the definition on a real one-sample render (the numpy reference alone)
QW, QH = 144, 96


@functools.lru_cache(maxsize=None)
def _quality_inputs():
    text = scene_json("S_CUBE")
    scene = rtgo.Scene.from_json_text(text)
    noisy, _, _ = oracle.render(scene, QW, QH, make_settings(rtgo, {"samples": 1, "max_depth": 50}, 3))
    truth, _, _ = oracle.render(scene, QW, QH, make_settings(rtgo, {"samples": 512, "max_depth": 50}, 77))
    return noisy.astype(np.float32), truth.astype(np.float64), aov_reference(text, QW, QH, 1, 3)


def test_quality_on_a_one_sample_render_of_s_cube():
    noisy, truth, f = _quality_inputs()
    out = reference(noisy, f["normal"], f["depth"], f["albedo"], f["object"])
    assert np.isfinite(out).all()
    # (the host function agrees on real inputs too)
    assert np.array_equal(bits(rtgo.denoise_host(noisy, f["normal"], f["depth"], f["albedo"], f["object"])[0]), bits(out))

    def rmse(img, mask=None):
        d = (img.astype(np.float64) - truth) ** 2
        return float(np.sqrt((d if mask is None else d[mask]).mean()))

    whole = rmse(out) / rmse(noisy)
    sphere = f["object"] == 1  # the Lambertian sphere
    assert int(sphere.sum()) >= 300, int(sphere.sum())
    part = rmse(out, sphere) / rmse(noisy, sphere)
    print(f"whole image {rmse(noisy):.5f} -> {rmse(out):.5f} ratio {whole:.3f}; "
          f"object 1 ({int(sphere.sum())} pixels) {rmse(noisy, sphere):.5f} -> {rmse(out, sphere):.5f} ratio {part:.3f}")
    for k in range(4):
        m = f["object"] == k
        if m.any():
            print(f"object {k}: {int(m.sum())} pixels, {rmse(noisy, m):.5f} -> {rmse(out, m):.5f}")
    assert whole < 1.0, whole
    assert part < 0.8, part
