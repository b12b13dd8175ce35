"""Variance-guided denoising (rt_temporal_moments_host, rt_variance_host,
rt_denoise_var_host), CPU: the declarations and their ctypes
mirrors, the three host functions held bit for bit to the numpy restatement of
the definitions (tests/variance_reference.py), conditions on that restatement
alone so that no comparison passes vacuously, cross-checks against
rt_temporal_host and rt_denoise_host as they stand, cases that are exact in
binary64, the refused calls, a stand-alone sanitizer run of the per-pixel
functions, and what the feature is for: over six one-sample frames of S_CUBE
the chain must beat the accumulated colour, and the existing filter on the
metal cube (figures in DESIGN.md §4.15)."""
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
import temporal_reference as tref
from aov_reference import reference as aov_reference
from conftest import ROOT
from denoise_reference import reference as denoise_reference
from scene_cases import make_settings
from sequence_cases import at, scene_json
from variance_reference import (CASES, FILTER_CASES, INVALID, MOMENTS_CASES, SPATIAL, TEMPORAL, VARIANCE_CASES, bits,
                                filter_case_reference, filter_reference, moments_case_reference, moments_inputs,
                                moments_reference, spatial_inputs, synthetic, variance_case_reference,
                                variance_reference)

HEADER = os.path.join(ROOT, "include", "rt_api.h")
RT_E_INVALID = -1
FUNCS = ["rt_temporal_moments_async", "rt_temporal_moments_host", "rt_variance_default", "rt_variance_async",
         "rt_variance_host", "rt_denoise_var_default", "rt_denoise_var_workspace_bytes", "rt_denoise_var_async",
         "rt_denoise_var_host"]
SENT = -1234.5


def test_declared_exported_and_version_stays_8():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(rtgo.LIB_PATH)
    for f in FUNCS:
        assert re.search(r"^[\w \*]+\b%s\s*\(" % f, text, flags=re.M), f
        assert hasattr(lib, f) and f in rtgo.EXPORTED_SYMBOLS, f
    for s in ("rt_variance", "rt_variance_inputs", "rt_denoise_var"):
        assert re.search(r"\}\s*%s\s*;" % s, text), s
    assert re.search(r"#define\s+RT_ABI_VERSION\s+8\b", text)
    assert rtgo.lib().rt_abi_version() == 8


def test_ctypes_signatures_and_struct_layouts_match_c(tmp_path):
    L = rtgo.lib()
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_size_t
    T, F = ctypes.POINTER(rtgo.Temporal), ctypes.POINTER(rtgo.TemporalFrame)
    V, VI = ctypes.POINTER(rtgo.Variance), ctypes.POINTER(rtgo.VarianceInputs)
    D, DI = ctypes.POINTER(rtgo.DenoiseVar), ctypes.POINTER(rtgo.DenoiseInputs)
    want = {
        "rt_temporal_moments_async": (ctypes.c_int, [T, i32, i32, F, F, vp, vp, vp, vp, vp, vp, vp]),
        "rt_temporal_moments_host": (ctypes.c_int, [T, i32, i32, F, F, vp, vp, vp, vp, vp, vp]),
        "rt_variance_default": (None, [V]),
        "rt_variance_async": (ctypes.c_int, [V, i32, i32, VI, vp, vp]),
        "rt_variance_host": (ctypes.c_int, [V, i32, i32, VI, vp]),
        "rt_denoise_var_default": (None, [D]),
        "rt_denoise_var_workspace_bytes": (sz, [i32, i32]),
        "rt_denoise_var_async": (ctypes.c_int, [D, i32, i32, DI, vp, vp, vp, vp, vp, sz, vp]),
        "rt_denoise_var_host": (ctypes.c_int, [D, i32, i32, DI, vp, vp, vp, vp]),
    }
    for name, (res, args) in want.items():
        f = getattr(L, name)
        assert (f.restype, list(f.argtypes)) == (res, args), name
    inc = os.path.join(ROOT, "include")
    # the declarations have exactly these types (a mismatch does not compile; compiled only, not linked)
    typ = tmp_path / "vr_type.c"
    typ.write_text(
        '#include "rt_api.h"\n'
        "int (*const f0)(const rt_temporal*, int32_t, int32_t, const rt_temporal_frame*, const rt_temporal_frame*,\n"
        "                const float*, const float*, float*, float*, float*, uint8_t*, void*) = rt_temporal_moments_async;\n"
        "int (*const f1)(const rt_temporal*, int32_t, int32_t, const rt_temporal_frame*, const rt_temporal_frame*,\n"
        "                const float*, const float*, float*, float*, float*, uint8_t*) = rt_temporal_moments_host;\n"
        "void (*const f2)(rt_variance*) = rt_variance_default;\n"
        "int (*const f3)(const rt_variance*, int32_t, int32_t, const rt_variance_inputs*, float*, void*) = rt_variance_async;\n"
        "int (*const f4)(const rt_variance*, int32_t, int32_t, const rt_variance_inputs*, float*) = rt_variance_host;\n"
        "void (*const f5)(rt_denoise_var*) = rt_denoise_var_default;\n"
        "size_t (*const f6)(int32_t, int32_t) = rt_denoise_var_workspace_bytes;\n"
        "int (*const f7)(const rt_denoise_var*, int32_t, int32_t, const rt_denoise_inputs*, const float*, float*,\n"
        "                uint8_t*, float*, void*, size_t, void*) = rt_denoise_var_async;\n"
        "int (*const f8)(const rt_denoise_var*, int32_t, int32_t, const rt_denoise_inputs*, const float*, float*,\n"
        "                uint8_t*, float*) = rt_denoise_var_host;\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", inc, "-c", str(typ), "-o", str(tmp_path / "vr_type.o")],
                   check=True)
    structs = {"rt_variance": (rtgo.Variance, ["min_history", "sigma_depth", "normal_power", "_pad"]),
               "rt_variance_inputs": (rtgo.VarianceInputs,
                                      ["color", "normal", "depth", "albedo", "object", "moments", "count"]),
               "rt_denoise_var": (rtgo.DenoiseVar,
                                  ["levels", "normal_power", "sigma_lum", "sigma_depth", "demodulate", "prefilter"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_api.h"', "int main(void) {"]
    for c, (_, fields) in structs.items():
        lines.append(f'printf("{c} sizeof %zu\\n", sizeof({c}));')
        lines += [f'printf("{c} {n} %zu\\n", offsetof({c}, {n}));' for n in fields]
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "vr_layout.c", tmp_path / "vr_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = {tuple(ln.split()[:2]): int(ln.split()[2])
           for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    for c, (cls, fields) in structs.items():
        assert got[(c, "sizeof")] == ctypes.sizeof(cls), c
        assert [n for n, _ in cls._fields_] == fields, c
        for n in fields:
            assert got[(c, n)] == getattr(cls, n).offset, (c, n)


def test_defaults_and_the_python_arguments():
    v = rtgo.default_variance()
    assert (v.min_history, v.normal_power, v.sigma_depth) == (4.0, 32, 0.05)
    d = rtgo.default_denoise_var()
    assert (d.levels, d.normal_power, d.sigma_lum, d.sigma_depth, d.demodulate, d.prefilter) == (4, 32, 2.0, 0.05, 1, 1)
    assert rtgo.default_denoise_var(sigma_lum=8, prefilter=0).sigma_lum == 8.0
    with pytest.raises(rtgo.RenderError):
        rtgo.default_variance(history=1)
    with pytest.raises(rtgo.RenderError):
        rtgo.default_denoise_var(sigma_color=1)
    # a dict's fields go to the struct that has them, the shared ones to both
    vv, dd = rtgo._as_variance({"min_history": 2, "sigma_depth": 0.1, "levels": 2})
    assert (vv.min_history, vv.sigma_depth, dd.sigma_depth, dd.levels) == (2.0, 0.1, 0.1, 2)
    with pytest.raises(rtgo.RenderError):
        rtgo._as_variance({"sigma_color": 1})
    n = 33 * 17
    assert rtgo.denoise_var_workspace_bytes(33, 17) >= 52 * n and rtgo.denoise_var_workspace_bytes(33, 17) <= 64 * n + 256
    assert rtgo.denoise_var_workspace_bytes(0, 17) == 0 and rtgo.denoise_var_workspace_bytes(65536, 65536) == 0


def test_python_layer_refuses_bad_combinations_before_any_device():
    r = rtgo.ParallelRenderer(1)
    r.set_samples(1)
    scene = rtgo.Scene.from_json_text(scene_json("S_CUBE"))
    with pytest.raises(rtgo.RenderError, match="needs temporal"):
        r.render_sequence(scene, 8, 8, [at((0, 0, 3))], variance=True)
    with pytest.raises(rtgo.RenderError, match="variance and denoise"):
        r.render_sequence(scene, 8, 8, [at((0, 0, 3))], temporal=True, denoise=True, variance=True)
    with pytest.raises(rtgo.RenderError, match="variance and params"):
        r.render_denoised(scene, 8, 8, params={"levels": 2}, variance=True)
    with pytest.raises(rtgo.RenderError, match="no such field"):
        r.render_sequence(scene, 8, 8, [at((0, 0, 3))], temporal=True, variance={"sigma_color": 1})


def _tonemapped(lin):
    want = np.zeros(lin.shape[:2] + (4,), np.uint8)
    rtgo.lib().rt_tonemap_rgba(lin.ctypes.data, lin.shape[0] * lin.shape[1], want.ctypes.data)
    return want


def _same(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert got.shape == want.shape and got.dtype == want.dtype and bad.size == 0, (what, len(bad), bad[:4].tolist())


def _variance_host(inp, params):
    return rtgo.variance_host(inp["color"], inp["normal"], inp["depth"], inp["albedo"], inp["object"], inp["moments"],
                              inp["count"], params)


def _filter_host(inp, params):
    return rtgo.denoise_var_host(inp["color"], inp["normal"], inp["depth"], inp["variance"], inp["albedo"],
                                 inp["object"], params)


@pytest.mark.parametrize("name", MOMENTS_CASES)
def test_moments_host_equals_the_numpy_reference_bit_for_bit(name):
    ref_color, ref_count, ref_moments, _ = moments_case_reference(name)
    cur, prev, params = moments_inputs(name)
    color, count, moments, rgba = rtgo.temporal_moments_host(cur, prev, params)
    _same(color, ref_color, (name, "color"))
    _same(count, ref_count, (name, "count"))
    _same(moments, ref_moments, (name, "moments"))
    assert rgba.tobytes() == _tonemapped(color).tobytes()
    # colour and count are rt_temporal_host's as it stands, and the numpy restatement of §4.14's
    plain_cur = {k: v for k, v in cur.items() if k != "albedo"}
    plain_prev = None if prev is None else {k: v for k, v in prev.items() if k != "moments"}
    host = rtgo.temporal_host(plain_cur, plain_prev, params)
    _same(color, host[0], (name, "color, rt_temporal_host"))
    _same(count, host[1], (name, "count, rt_temporal_host"))
    assert rgba.tobytes() == host[2].tobytes()
    ref = tref.reference(plain_cur, plain_prev, **params)
    _same(color, ref[0], (name, "color, temporal_reference"))
    _same(count, ref[1], (name, "count, temporal_reference"))


@pytest.mark.parametrize("name", VARIANCE_CASES)
def test_variance_host_equals_the_numpy_reference_bit_for_bit(name):
    inp, vp, _ = spatial_inputs(name)
    _same(_variance_host(inp, vp), variance_case_reference(name)[0], name)


@pytest.mark.parametrize("name", FILTER_CASES)
def test_filter_host_equals_the_numpy_reference_bit_for_bit(name):
    inp, _, fp = spatial_inputs(name)
    ref_lin, ref_var = filter_case_reference(name)
    lin, rgba, var = _filter_host(inp, fp)
    _same(lin, ref_lin, (name, "linear"))
    _same(var, ref_var, (name, "variance"))
    assert rgba.tobytes() == _tonemapped(lin).tobytes() and (rgba[..., 3] == 255).all()


def test_filter_host_outputs_are_optional_and_in_place_is_allowed():
    inp, _, fp = spatial_inputs("33x17")
    ref_lin, ref_var = filter_case_reference("33x17")
    h, w = inp["depth"].shape
    keep = {k: np.ascontiguousarray(v) for k, v in inp.items() if v is not None}
    color, variance = keep["color"].copy(), keep["variance"].copy()
    di = rtgo.DenoiseInputs(color.ctypes.data, keep["normal"].ctypes.data, keep["depth"].ctypes.data,
                            keep["albedo"].ctypes.data, keep["object"].ctypes.data)
    p = rtgo.default_denoise_var(**fp)
    rgba = np.zeros((h, w, 4), np.uint8)
    L = rtgo.lib()
    # out_rgba alone, out_variance NULL
    assert L.rt_denoise_var_host(ctypes.byref(p), w, h, ctypes.byref(di), variance.ctypes.data, None, rgba.ctypes.data,
                                 None) == 0
    assert rgba.tobytes() == _tonemapped(ref_lin).tobytes()
    # out_linear == color and out_variance == variance, out_rgba NULL
    assert L.rt_denoise_var_host(ctypes.byref(p), w, h, ctypes.byref(di), variance.ctypes.data, color.ctypes.data, None,
                                 variance.ctypes.data) == 0
    _same(color, ref_lin, "in place")
    _same(variance, ref_var, "variance in place")


def test_reference_conditions_nothing_passes_vacuously():
    cur, prev, extra = synthetic(33, 17)
    valid = np.isfinite(cur["depth"])
    assert 0.10 <= 1 - valid.mean() <= 0.30
    assert set(np.unique(cur["object"][valid]).tolist()) == {0, 1, 2}
    assert (cur["albedo"] == 0).mean() > 0.05 and (extra["variance"] == 0).mean() > 0.05
    # the moments pass: at least 25 % of the valid pixels blend a history, at least 25 % restart, and a blend
    # is neither the current nor the previous moments
    color, count, moments, has = moments_case_reference("33x17")
    assert has[valid].mean() >= 0.25 and (~has)[valid].mean() >= 0.25, has[valid].mean()
    started = moments_case_reference("prev NULL")[2]
    assert (bits(moments)[has] != bits(started)[has]).all(axis=-1).mean() > 0.95
    _same(moments[~has], started[~has], "no history: ((float)l, (float)(l * l))")
    assert (bits(moments_case_reference("albedo NULL")[2]) != bits(moments)).any(axis=-1)[valid].mean() > 0.8
    # the variance pass on the main case: each branch takes at least 15 % of the pixels
    var, branch = variance_case_reference("33x17")
    for k, what in ((TEMPORAL, "temporal"), (SPATIAL, "spatial"), (INVALID, "invalid")):
        assert (branch == k).mean() >= 0.15, (what, (branch == k).mean())
    assert ((branch == INVALID) == ~valid).all() and (var[~valid] == 0).all()
    assert (var[branch == TEMPORAL] > 0).mean() > 0.9 and (var[branch == SPATIAL] > 0).mean() > 0.9
    assert (variance_case_reference("min_history 1")[1] != SPATIAL).all()
    assert (variance_case_reference("min_history 1e9")[1] != TEMPORAL).all()
    for name in ("normal_power 0", "sigma_depth 0", "object NULL", "moments NULL", "min_history 1", "min_history 1e9"):
        assert (bits(variance_case_reference(name)[0]) != bits(var)).any(), name
    assert (bits(variance_case_reference("moments and albedo NULL")[0])
            != bits(variance_case_reference("moments NULL")[0])).any()
    # the filter changes most valid pixels and their variance, and each mechanism changes the output
    inp, _, _ = spatial_inputs("33x17")
    lin, fvar = filter_case_reference("33x17")
    assert (bits(lin) != bits(inp["color"])).any(axis=-1)[valid].mean() > 0.9
    assert (bits(fvar) != bits(inp["variance"]))[valid].mean() > 0.9
    _same(lin[~valid], inp["color"][~valid], "not valid: the input colour")
    _same(fvar[~valid], inp["variance"][~valid], "not valid: the input variance")
    for name in FILTER_CASES[4:]:
        assert (bits(filter_case_reference(name)[0]) != bits(lin)).any(), name
    assert (bits(filter_case_reference("70x5")[0]) != bits(spatial_inputs("70x5")[0]["color"])).any(axis=-1)[:, 64:].any()
    for name in CASES:
        assert name in MOMENTS_CASES or name in VARIANCE_CASES or name in FILTER_CASES, name


def test_filter_without_the_luminance_stop_is_rt_denoise_without_the_colour_stop():
    for name in ("33x17", "70x5", "3x2", "albedo NULL", "object NULL"):
        inp, _, fp = spatial_inputs(name)
        lin, rgba, _ = _filter_host(inp, dict(fp, sigma_lum=0.0))
        want_lin, want_rgba = rtgo.denoise_host(inp["color"], inp["normal"], inp["depth"], inp["albedo"], inp["object"],
                                                dict(levels=fp["levels"], sigma_color=0.0))
        _same(lin, want_lin, name)
        assert rgba.tobytes() == want_rgba.tobytes(), name
        _same(lin, denoise_reference(inp["color"], inp["normal"], inp["depth"], inp["albedo"], inp["object"],
                                     levels=fp["levels"], sigma_color=0.0), (name, "denoise_reference"))


# ---- cases that are exact in binary64
def test_exact_uniform_image_one_level_scales_the_variance_by_4900_over_65536():
    h, w = 9, 11
    color = np.full((h, w, 3), 0.75, np.float32)
    normal = np.zeros((h, w, 3), np.float32)
    normal[..., 2] = 1
    depth = np.full((h, w), 2.0, np.float32)
    for v in (0.5, 2.0 ** -7):
        variance = np.full((h, w), v, np.float32)
        lin, _, var = rtgo.denoise_var_host(color, normal, depth, variance, params=dict(levels=1, sigma_lum=0.0))
        # every weight is h[|dx|] * h[|dy|]: sumw = 1 and sum w^2 = (70 / 256)^2 in the interior (two pixels from the edge)
        assert (var[2:-2, 2:-2] == np.float32(v * 4900 / 65536)).all() and v * 4900 / 65536 == float(np.float32(v * 4900 / 65536))
        assert (var[0] != np.float32(v * 4900 / 65536)).all()  # (an edge row has fewer taps)
        _same(lin, color, "a uniform colour stays")
        _same(var, filter_reference(color, normal, depth, variance, levels=1, sigma_lum=0.0)[1], "reference")


def _static(n, seed=23):
    rng = np.random.default_rng(seed)
    w, h = 33, 17
    frame = rtgo.camera_frame(tref.CAM_CUR, "lookat", w, h)
    depth = np.full((h, w), 2.5, np.float32)
    inputs = [(rng.random((h, w, 3)) * 2).astype(np.float32) for _ in range(n)]
    state, out = None, []
    for c in inputs:
        cur = dict(color=c, depth=depth, frame=frame)
        color, count, moments, _ = rtgo.temporal_moments_host(cur, state)
        ref = moments_reference(cur, state)
        _same(moments, ref[2], "reference")
        state = dict(cur, color=color, count=count, moments=moments)
        out.append((count, moments))
    return inputs, out


def test_static_camera_moments_are_the_running_means():
    inputs, out = _static(8)
    lums = [(0.2126 * c[..., 0].astype(np.float64) + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2] for c in inputs]
    for k, (count, moments) in enumerate(out):
        assert (count == k + 1).all()
        m1 = np.mean(np.stack(lums[:k + 1]), axis=0)
        m2 = np.mean(np.stack([l * l for l in lums[:k + 1]]), axis=0)
        # each call rounds one value to float32 on store (below 2: half an ulp is 2^-24; below 4: 2^-23) and the
        # neighbour taps' weights are about 1e-13 (fx is x to within rounding): 2^-22 and 2^-21 per call bound
        # both with room
        e1, e2 = np.abs(moments[..., 0] - m1).max(), np.abs(moments[..., 1] - m2).max()
        assert e1 <= (k + 1) * 2.0 ** -22 and e2 <= (k + 1) * 2.0 ** -21, (k, e1, e2)
    # ... so the temporal variance of the last frame is the frames' sample variance over n
    count, moments = out[-1]
    color = np.zeros((17, 33, 3), np.float32)
    normal = np.zeros((17, 33, 3), np.float32)
    depth = np.full((17, 33), 2.5, np.float32)
    var = rtgo.variance_host(color, normal, depth, moments=moments, count=count)
    want = np.var(np.stack(lums), axis=0) / 8
    assert np.abs(var - want).max() <= 2.0 ** -18, np.abs(var - want).max()  # (m2 - m1^2 of values within 8 * 2^-21)


def test_disocclusion_restarts_the_moments():
    cur, prev, _ = moments_inputs("33x17")
    z = np.where(np.isfinite(cur["depth"]), cur["depth"], np.float32(2.0)).astype(np.float32)
    cur = dict(cur, depth=z)
    prev = dict(prev, depth=(z * np.float32(1.2)).astype(np.float32), frame=cur["frame"])
    for f in (cur, prev):
        del f["object"], f["normal"]
    color, count, moments, _ = rtgo.temporal_moments_host(cur, prev, {"depth_tol": 0.05})
    assert (count == 1).all()
    _same(moments, moments_reference(cur, None)[2], "((float)l, (float)(l * l))")
    _same(color, cur["color"], "cur.color")
    assert (rtgo.temporal_moments_host(cur, prev, {"depth_tol": 0.0})[1] > 1).mean() > 0.9


# ---- refused calls
def _refused(cases, call, outputs, names):
    """Every case returns RT_E_INVALID from the _host and the _async entry (async: refused before it touches
    a device), names the entry and leaves the sentinel-filled outputs as they are; then call() succeeds."""
    lib = rtgo.lib()
    for entry in ("host", "async"):
        for what, kw in cases.items():
            assert call(entry=entry, **kw) == RT_E_INVALID, (what, entry)
            msg = lib.rt_last_error()
            assert msg and names[entry] in msg, (what, msg)
            for a in outputs:
                assert (a == (SENT if a.dtype == np.float32 else 0xA5)).all(), (what, entry)
    assert call(entry="host") == 0


def test_moments_refused_calls_leave_the_outputs_untouched():
    lib = rtgo.lib()
    cur, prev, _ = moments_inputs("33x17")
    h, w = cur["depth"].shape
    color, count = np.full((h, w, 3), SENT, np.float32), np.full((h, w), SENT, np.float32)
    moments, rgba = np.full((h, w, 2), SENT, np.float32), np.full((h, w, 4), 0xA5, np.uint8)
    keep = []
    T = rtgo.default_temporal

    def call(entry, params=T(), w=w, h=h, cur_drop=(), prev_on=True, prev_drop=(), out_drop=(), alias=None,
             moments_on=True, prev_frame=None):
        def frame(d, drop):
            a = {k: np.ascontiguousarray(d[k]) for k in ("color", "depth", "object", "normal", "count", "albedo", "moments")
                 if d.get(k) is not None and k not in drop}
            keep.append(a)
            fr = d["frame"] if prev_frame is None or d is cur else prev_frame
            return rtgo.temporal_frame(fr, *[a[k].ctypes.data if k in a else None
                                             for k in ("color", "depth", "object", "normal", "count")]), a
        fc, ac = frame(cur, cur_drop)
        fp, ap = frame(prev, prev_drop)
        outs = {"color": color, "count": count, "moments": moments}
        ptr = {k: (None if k in out_drop else a.ctypes.data) for k, a in outs.items()}
        pm = ap["moments"].ctypes.data if moments_on else None
        if alias == "color":
            fp.color = ptr["color"]
        if alias == "count":
            fp.count = ptr["count"]
        if alias == "moments":
            pm = ptr["moments"]
        args = [ctypes.byref(params) if params is not None else None, w, h, ctypes.byref(fc),
                ctypes.byref(fp) if prev_on else None, ac["albedo"].ctypes.data, pm, ptr["color"], ptr["count"],
                ptr["moments"], rgba.ctypes.data]
        return lib.rt_temporal_moments_host(*args) if entry == "host" else lib.rt_temporal_moments_async(*args, None)

    nan = float("nan")
    bad_frame = np.array(prev["frame"], np.float64)
    bad_frame[6:9] = 0
    cases = {
        "NULL params": dict(params=None), "NULL cur.color": dict(cur_drop=("color",)),
        "NULL prev.count": dict(prev_drop=("count",)), "object in cur only": dict(prev_drop=("object",)),
        "prev without prev_moments": dict(moments_on=False), "prev_moments without prev": dict(prev_on=False),
        "NULL out_color": dict(out_drop=("color",)), "NULL out_count": dict(out_drop=("count",)),
        "NULL out_moments": dict(out_drop=("moments",)),
        "out_color == prev.color": dict(alias="color"), "out_count == prev.count": dict(alias="count"),
        "out_moments == prev_moments": dict(alias="moments"),
        "w = 0": dict(w=0), "h = 65537": dict(h=65537), "too many pixels": dict(w=65536, h=65536),
        "max_history 0.5": dict(params=T(max_history=0.5)), "max_history NaN": dict(params=T(max_history=nan)),
        "depth_tol < 0": dict(params=T(depth_tol=-0.01)), "normal_min NaN": dict(params=T(normal_min=nan)),
        "min_weight 0": dict(params=T(min_weight=0.0)), "hh == 0": dict(prev_frame=bad_frame),
    }
    _refused(cases, call, (color, count, moments, rgba),
             {"host": b"rt_temporal_moments_host", "async": b"rt_temporal_moments_async"})
    ref = moments_case_reference("33x17")
    _same(color, ref[0], "after the refused calls")
    _same(moments, ref[2], "after the refused calls")
    assert call("host", prev_on=False, moments_on=False) == 0  # (no prev needs no prev_moments)


def test_variance_refused_calls_leave_the_output_untouched():
    lib = rtgo.lib()
    inp, _, _ = spatial_inputs("33x17")
    h, w = inp["depth"].shape
    out = np.full((h, w), SENT, np.float32)
    keep = {k: np.ascontiguousarray(v) for k, v in inp.items()}
    V = rtgo.default_variance

    def call(entry, params=V(), w=w, h=h, drop=(), inputs_on=True, out_on=True):
        vi = rtgo.VarianceInputs(*[None if k in drop else keep[k].ctypes.data
                                   for k in ("color", "normal", "depth", "albedo", "object", "moments", "count")])
        args = [ctypes.byref(params) if params is not None else None, w, h, ctypes.byref(vi) if inputs_on else None,
                out.ctypes.data if out_on else None]
        return lib.rt_variance_host(*args) if entry == "host" else lib.rt_variance_async(*args, None)

    nan, inf = float("nan"), float("inf")
    cases = {
        "NULL params": dict(params=None), "NULL inputs": dict(inputs_on=False), "NULL color": dict(drop=("color",)),
        "NULL normal": dict(drop=("normal",)), "NULL depth": dict(drop=("depth",)), "NULL out_var": dict(out_on=False),
        "moments without count": dict(drop=("count",)), "count without moments": dict(drop=("moments",)),
        "w = 0": dict(w=0), "h = -1": dict(h=-1), "w = 65537": dict(w=65537), "too many pixels": dict(w=65536, h=65536),
        "min_history 0.5": dict(params=V(min_history=0.5)), "min_history NaN": dict(params=V(min_history=nan)),
        "min_history inf": dict(params=V(min_history=inf)), "normal_power 3": dict(params=V(normal_power=3)),
        "normal_power 256": dict(params=V(normal_power=256)), "normal_power -1": dict(params=V(normal_power=-1)),
        "sigma_depth < 0": dict(params=V(sigma_depth=-1.0)), "sigma_depth NaN": dict(params=V(sigma_depth=nan)),
    }
    _refused(cases, call, (out,), {"host": b"rt_variance_host", "async": b"rt_variance_async"})
    _same(out, variance_case_reference("33x17")[0], "after the refused calls")
    assert call("host", drop=("albedo", "object", "moments", "count")) == 0


def test_filter_refused_calls_leave_the_outputs_and_the_workspace_untouched():
    lib = rtgo.lib()
    inp, _, fp = spatial_inputs("33x17")
    h, w = inp["depth"].shape
    lin, var = np.full((h, w, 3), SENT, np.float32), np.full((h, w), SENT, np.float32)
    rgba = np.full((h, w, 4), 0xA5, np.uint8)
    nbytes = rtgo.denoise_var_workspace_bytes(w, h)
    work = np.full(nbytes, 0xA5, np.uint8)  # (host memory: a refused async call never reads the pointer)
    keep = {k: np.ascontiguousarray(v) for k, v in inp.items()}
    D = lambda **kw: rtgo.default_denoise_var(**dict(fp, **kw))

    def call(entry, params=None, w=w, h=h, drop=(), inputs_on=True, outs=("lin", "rgba", "var"), work_on=True,
             work_bytes=nbytes, null_params=False):
        params = D() if params is None else params
        di = rtgo.DenoiseInputs(*[None if k in drop else keep[k].ctypes.data
                                  for k in ("color", "normal", "depth", "albedo", "object")])
        args = [None if null_params else ctypes.byref(params), w, h, ctypes.byref(di) if inputs_on else None,
                None if "variance" in drop else keep["variance"].ctypes.data,
                lin.ctypes.data if "lin" in outs else None, rgba.ctypes.data if "rgba" in outs else None,
                var.ctypes.data if "var" in outs else None]
        if entry == "host":
            return lib.rt_denoise_var_host(*args)
        return lib.rt_denoise_var_async(*args, work.ctypes.data if work_on else None, work_bytes, None)

    nan, inf = float("nan"), float("inf")
    cases = {
        "NULL params": dict(null_params=True), "NULL inputs": dict(inputs_on=False), "NULL color": dict(drop=("color",)),
        "NULL normal": dict(drop=("normal",)), "NULL depth": dict(drop=("depth",)),
        "NULL variance": dict(drop=("variance",)), "out_linear and out_rgba NULL": dict(outs=("var",)),
        "w = 0": dict(w=0), "h = 65537": dict(h=65537), "too many pixels": dict(w=65536, h=65536),
        "levels 0": dict(params=D(levels=0)), "levels 9": dict(params=D(levels=9)),
        "normal_power 3": dict(params=D(normal_power=3)), "sigma_lum < 0": dict(params=D(sigma_lum=-1.0)),
        "sigma_lum NaN": dict(params=D(sigma_lum=nan)), "sigma_lum inf": dict(params=D(sigma_lum=inf)),
        "sigma_depth NaN": dict(params=D(sigma_depth=nan)), "demodulate 2": dict(params=D(demodulate=2)),
        "prefilter 2": dict(params=D(prefilter=2)), "prefilter -1": dict(params=D(prefilter=-1)),
    }
    _refused(cases, call, (lin, rgba, var, work), {"host": b"rt_denoise_var_host", "async": b"rt_denoise_var_async"})
    _same(lin, filter_case_reference("33x17")[0], "after the refused calls")
    _same(var, filter_case_reference("33x17")[1], "after the refused calls")
    lin[:], var[:], rgba[:] = SENT, SENT, 0xA5
    for what, kw in {"NULL workspace": dict(work_on=False), "a workspace one byte short": dict(work_bytes=nbytes - 1)}.items():
        assert call("async", **kw) == RT_E_INVALID, what
        assert b"rt_denoise_var_workspace_bytes" in lib.rt_last_error(), what
        assert (lin == SENT).all() and (var == SENT).all() and (rgba == 0xA5).all() and (work == 0xA5).all(), what


# ---- the per-pixel functions under the host sanitizers: a stand-alone program, nothing is loaded into Python
def test_per_pixel_functions_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no g++ (the compiler of the suite's other sanitizer programs)"
    src = os.path.join(ROOT, "tests", "c", "variance_sanitize.cpp")
    exe = str(tmp_path / "variance_sanitize")
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
    assert "variance_sanitize ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


# ---- quality: the chain over six one-sample frames from a moving camera (the numpy reference and the oracle alone)
QW, QH, QFRAMES, QSTEP = 144, 96, 6, 0.05  # (the set-up of test_temporal_cpu's quality test)


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
                   albedo=feat["albedo"], frame=rtgo.camera_frame(cam, "reference", QW, QH))
        color, count, moments, _ = moments_reference(cur, state)
        state = dict(cur, color=color, count=count, moments=moments)
    truth, _, _ = oracle.render(scene, QW, QH, make_settings(rtgo, {"samples": 512, "max_depth": 50}, 77))
    g = (feat["normal"], feat["depth"])
    plain = denoise_reference(color, *g, feat["albedo"], feat["object"])  # (b): the existing filter at its defaults
    var, branch = variance_reference(color, *g, feat["albedo"], feat["object"], moments, count)
    chain, _ = filter_reference(color, *g, var, feat["albedo"], feat["object"])  # (c): the new chain at its defaults
    # the single-frame case: the last one-sample render alone, spatial variance only
    var1, _ = variance_reference(cur["color"], *g, feat["albedo"], feat["object"])
    single, _ = filter_reference(cur["color"], *g, var1, feat["albedo"], feat["object"])
    plain1 = denoise_reference(cur["color"], *g, feat["albedo"], feat["object"])
    return dict(noisy=cur["color"], acc=color, plain=plain, chain=chain, single=single, plain1=plain1, branch=branch,
                obj=feat["object"], truth=truth.astype(np.float64))


def test_quality_over_six_one_sample_frames_of_s_cube():
    """Measured, RMSE against the 512-sample render on the last of six frames: (a) the
    accumulated colour, (b) (a) through rt_denoise at its defaults, (c) the chain at its defaults (sigma_lum 2).
    Whole image (a) 0.00857, (b) 0.00869, (c) 0.00853: (c) / (a) 0.9955.  Object 1 (the Lambertian sphere, 305
    pixels) (a) 0.02283, (b) 0.02192, (c) 0.02177: (c) / (a) 0.9535.  Object 3 (the metal cube) (a) 0.00129, (b)
    0.00362, (c) 0.00129: (c) / (b) 0.3571.  Each bound is the midpoint between the measured ratio and 1: half
    the gain, kept as margin against a different seed.  The single-frame case (one 1-spp render, spatial
    variance only) is printed, not asserted: whole image 0.01073 -> 0.00879 (rt_denoise: 0.00865), metal cube
    0.00140 -> 0.00144 (rt_denoise: 0.00360)."""
    q = _quality()
    truth, obj = q["truth"], q["obj"]
    assert np.isfinite(q["chain"]).all()

    def rmse(img, mask=None):
        d = (img.astype(np.float64) - truth) ** 2
        return float(np.sqrt((d if mask is None else d[mask]).mean()))

    for name in ("noisy", "acc", "plain", "chain", "plain1", "single"):
        print(f"{name:7s} whole {rmse(q[name]):.5f} " +
              " ".join(f"object {k} {rmse(q[name], obj == k):.5f}" for k in range(4)))
    valid = obj >= 0
    print(f"temporal branch: {(q['branch'][valid] == TEMPORAL).mean():.3f} of the valid pixels")
    sphere, cube = obj == 1, obj == 3
    assert int(sphere.sum()) >= 300, int(sphere.sum())
    whole = rmse(q["chain"]) / rmse(q["acc"])
    part = rmse(q["chain"], sphere) / rmse(q["acc"], sphere)
    metal = rmse(q["chain"], cube) / rmse(q["plain"], cube)
    print(f"(c) / (a) whole {whole:.4f}, object 1 {part:.4f}; (c) / (b) object 3 {metal:.4f}")
    assert whole < 0.9978, whole
    assert part < 0.9768, part
    assert metal < 0.6786, metal
    assert (q["branch"][valid] == TEMPORAL).mean() > 0.8  # (the variance the chain used is mostly the temporal one)
