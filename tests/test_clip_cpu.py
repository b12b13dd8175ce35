"""History rectification (rt_temporal_clip_host), CPU: the
declarations and their ctypes mirrors, the host function held bit for bit to the
numpy restatement (tests/clip_reference.py) with and without moments, albedo,
ids, the table, out_clipped and a previous frame, conditions on that restatement
alone so that no comparison passes vacuously, radius 0 held to the existing
calls, the refused calls, render_sequence's refusals before any device call, a
stand-alone sanitizer run of the per-pixel functions, and what the feature is
for: over six one-sample frames, the trail behind a moving shadow (C_FLOOR) and
the floor under a moving light (C_LIGHT) come closer to a 512-sample render than
under the pass without the clip, and static content is not hurt (figures in
DESIGN.md §4.18)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import clip_quality as cq
import rtgo
import temporal_reference as tref
from clip_reference import (DEFAULT_CLIP, SIZES, SYN_CLIP, TABLE, VARIANTS, bits, clip_of, reference, syn_inputs,
                            syn_reference)
from conftest import ROOT
from motion_reference import case_inputs as motion_inputs
from test_temporal_cpu import _frames, _same, _tonemapped

HEADER = os.path.join(ROOT, "include", "rt_api.h")
RT_E_INVALID = -1
FUNCS = ["rt_history_clip_default", "rt_temporal_clip_async", "rt_temporal_clip_host"]


def test_declared_exported_and_version_stays_8():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(rtgo.LIB_PATH)
    for f in FUNCS:
        assert re.search(r"^[\w \*]+\b%s\s*\(" % f, text, flags=re.M), f
        assert hasattr(lib, f) and f in rtgo.EXPORTED_SYMBOLS, f
    assert re.search(r"\}\s*rt_history_clip\s*;", text)
    assert re.search(r"#define\s+RT_ABI_VERSION\s+8\b", text)
    assert rtgo.lib().rt_abi_version() == 8
    for name in ("HistoryClip", "default_history_clip", "temporal_clip_async", "temporal_clip_host"):
        assert callable(getattr(rtgo, name)), name
    c = rtgo.default_history_clip()
    assert {k: getattr(c, k) for k in DEFAULT_CLIP} == DEFAULT_CLIP  # (the restatement's defaults are the library's)
    assert rtgo.default_history_clip(radius=3, gamma=2.5).gamma == 2.5
    with pytest.raises(rtgo.RenderError):
        rtgo.default_history_clip(sigma=1)


def test_ctypes_signatures_and_struct_layouts_match_c(tmp_path):
    L = rtgo.lib()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    T, F, M = ctypes.POINTER(rtgo.Temporal), ctypes.POINTER(rtgo.TemporalFrame), ctypes.POINTER(rtgo.Motion)
    K = ctypes.POINTER(rtgo.HistoryClip)
    assert (L.rt_temporal_clip_async.restype, list(L.rt_temporal_clip_async.argtypes)) == (
        ctypes.c_int, [T, i32, i32, F, F, M, K, vp, vp, vp, vp, vp, vp, vp, vp])
    assert (L.rt_temporal_clip_host.restype, list(L.rt_temporal_clip_host.argtypes)) == (
        ctypes.c_int, [T, i32, i32, F, F, M, K, vp, vp, vp, vp, vp, vp, vp])
    assert (L.rt_history_clip_default.restype, list(L.rt_history_clip_default.argtypes)) == (None, [K])
    inc = os.path.join(ROOT, "include")
    # the declarations have exactly these types (a mismatch does not compile; compiled only, not linked)
    typ = tmp_path / "cl_type.c"
    typ.write_text('#include "rt_api.h"\n'
                   "int (*const f1)(const rt_temporal*, int32_t, int32_t, const rt_temporal_frame*,\n"
                   "                const rt_temporal_frame*, const rt_motion*, const rt_history_clip*, const float*,\n"
                   "                const float*, float*, float*, float*, float*, uint8_t*, void*) = rt_temporal_clip_async;\n"
                   "int (*const f2)(const rt_temporal*, int32_t, int32_t, const rt_temporal_frame*,\n"
                   "                const rt_temporal_frame*, const rt_motion*, const rt_history_clip*, const float*,\n"
                   "                const float*, float*, float*, float*, float*, uint8_t*) = rt_temporal_clip_host;\n"
                   "void (*const f3)(rt_history_clip*) = rt_history_clip_default;\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", inc, "-c", str(typ), "-o", str(tmp_path / "cl_type.o")],
                   check=True)
    fields = ["radius", "min_taps", "gamma", "min_half"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_api.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(rt_history_clip));']
    lines += [f'printf("{n} %zu\\n", offsetof(rt_history_clip, {n}));' for n in fields]
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "cl_layout.c", tmp_path / "cl_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = {ln.split()[0]: int(ln.split()[1])
           for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert got["sizeof"] == ctypes.sizeof(rtgo.HistoryClip) == 24
    assert [n for n, _ in rtgo.HistoryClip._fields_] == fields
    for n in fields:
        assert got[n] == getattr(rtgo.HistoryClip, n).offset, n


# ---- the host function against the numpy restatement
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_equals_the_numpy_reference_bit_for_bit(size, variant):
    w, h = size
    v = VARIANTS[variant]
    cur, prev, table = syn_inputs(w, h, variant)
    ref = syn_reference(w, h, variant)
    got = rtgo.temporal_clip_host(cur, prev, table, moments=v["moments"], clip=clip_of(w, h))
    _same(got[0], ref["color"], (size, variant, "color"))
    _same(got[1], ref["count"], (size, variant, "count"))
    _same(got[-2], ref["clipped"], (size, variant, "clipped"))
    if v["moments"]:
        _same(got[2], ref["moments"], (size, variant, "moments"))
    # out_rgba is rt_tonemap_rgba of out_color
    assert got[-1].tobytes() == _tonemapped(got[0]).tobytes() and (got[-1][..., 3] == 255).all()


def test_host_without_out_clipped_and_out_rgba():
    w, h = 65, 5
    cur, prev, table = syn_inputs(w, h, "all")
    ref = syn_reference(w, h, "all")
    keep = []
    fc, fp = _frames(cur, prev, keep)
    color, count = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    mom = np.zeros((h, w, 2), np.float32)
    albedo, pmom = np.ascontiguousarray(cur["albedo"]), np.ascontiguousarray(prev["moments"])
    p, k = rtgo.default_temporal(), rtgo.default_history_clip(**clip_of(w, h))
    m = rtgo.Motion(TABLE.ctypes.data, 3, 0)
    assert rtgo.lib().rt_temporal_clip_host(ctypes.byref(p), w, h, ctypes.byref(fc), ctypes.byref(fp), ctypes.byref(m),
                                            ctypes.byref(k), albedo.ctypes.data, pmom.ctypes.data, color.ctypes.data,
                                            count.ctypes.data, mom.ctypes.data, None, None) == 0
    _same(color, ref["color"], "color")
    _same(count, ref["count"], "count")
    _same(mom, ref["moments"], "moments")


def test_reference_conditions_nothing_passes_vacuously():
    """On the restatement alone: in the cases used, pixels are clipped in one, two and three channels, some keep
    their history unclipped, nw < min_taps occurs, windows are cut by the image edge and by an id change, the
    clip changes the output where it says so and nowhere else, and n, the count and the moments are untouched."""
    seen = {k: 0 for k in ("one", "two", "three", "unclipped", "few taps", "edge", "id")}
    for w, h in SIZES:
        for variant, v in VARIANTS.items():
            if not v["prev"]:
                ref = syn_reference(w, h, variant)
                assert not ref["has"].any() and not ref["clipped"].any()
                continue
            ref = syn_reference(w, h, variant)
            ch, has = ref["channels"], ref["has"]
            assert not ch[~has].any() and ((ch > 0) == (ref["clipped"] == 1)).all()
            few = has & (ref["nw"] < clip_of(w, h)["min_taps"])
            assert not ch[few].any()
            for name, n in (("one", ((ch == 1) & has).sum()), ("two", ((ch == 2) & has).sum()),
                            ("three", ((ch == 3) & has).sum()), ("unclipped", ((ch == 0) & has & ~few).sum()),
                            ("few taps", few.sum()), ("edge", ref["cut_edge"].sum()), ("id", ref["cut_id"].sum())):
                seen[name] += int(n)
            # against the same call without the clip: only clipped pixels differ, and only in colour
            cur, prev, table = syn_inputs(w, h, variant)
            off = reference(cur, prev, table, v["moments"], dict(radius=0))
            assert not off["clipped"].any()
            differs = (bits(ref["color"]) != bits(off["color"])).any(axis=-1)
            assert not differs[ch == 0].any()
            assert np.array_equal(bits(ref["count"]), bits(off["count"]))
            if v["moments"]:
                assert np.array_equal(bits(ref["moments"]), bits(off["moments"]))
            if (w, h) == (72, 48):
                assert differs[ch > 0].mean() > 0.9, variant
    print(seen)
    assert min(seen.values()) >= 10, seen
    # the image smaller than its window: every window of 5x3 at radius 3 is cut by the edge
    ref = syn_reference(5, 3, "no ids")
    assert ref["has"].any() and (ref["cut_edge"] == ref["has"]).all() and ref["nw"].max() <= 15
    # a NaN history fails both comparisons and stays a NaN: it is pulled to neither edge (hc != he holds for a
    # NaN, so the pixel counts as clipped where its window had min_taps taps, and nowhere else)
    cur, prev, _ = syn_inputs(65, 5, "no ids")
    prev = dict(prev, color=np.full_like(prev["color"], np.nan))
    out = reference(cur, prev, None, True, SYN_CLIP)
    assert out["has"].any() and np.isnan(out["color"][out["has"]]).all()
    assert ((out["clipped"] == 1) == (out["has"] & (out["nw"] >= SYN_CLIP["min_taps"]))).all()
    got = rtgo.temporal_clip_host(cur, prev, None, moments=True, clip=SYN_CLIP)
    assert np.isnan(got[0][out["has"]]).all() and np.array_equal(got[0][~out["has"]], out["color"][~out["has"]])
    _same(got[-2], out["clipped"], "NaN history")


@pytest.mark.parametrize("name", [n for n in tref.CASES])
def test_radius_0_is_the_existing_calls_bit_for_bit(name):
    off = dict(radius=0)
    # without a table: rt_temporal_host and rt_temporal_moments_host (ids optional)
    cur, prev, params = tref.case_inputs(name)
    want = rtgo.temporal_host(cur, prev, params)
    got = rtgo.temporal_clip_host(cur, prev, None, params, clip=off)
    for a, b, what in zip((got[0], got[1], got[-1]), want, ("color", "count", "rgba")):
        _same(a, b, (name, what))
    assert not got[-2].any()
    mcur, mprev, _ = motion_inputs(name, True)
    want = rtgo.temporal_moments_host(mcur, mprev, params)
    got = rtgo.temporal_clip_host(mcur, mprev, None, params, moments=True, clip=off)
    for a, b, what in zip((got[0], got[1], got[2], got[-1]), want, ("color", "count", "moments", "rgba")):
        _same(a, b, (name, what))
    # with a table: rt_temporal_motion_host
    if name == "object NULL":
        with pytest.raises(rtgo.RenderError, match="object is required"):
            rtgo.temporal_clip_host(cur, prev, TABLE, params, clip=off)
        return
    for moments in (False, True):
        c, p, _ = motion_inputs(name, moments)
        want = rtgo.temporal_motion_host(c, p, TABLE, params, moments=moments)
        got = rtgo.temporal_clip_host(c, p, TABLE, params, moments=moments, clip=off)
        _same(got[0], want[0], (name, moments, "color"))
        _same(got[1], want[1], (name, moments, "count"))
        assert got[-1].tobytes() == want[-1].tobytes()
        if moments:
            _same(got[2], want[2], (name, "moments"))


# ---- the refused calls
def test_every_refused_call_leaves_the_outputs_untouched():
    lib = rtgo.lib()
    w, h = 65, 5
    cur, prev, _ = syn_inputs(w, h, "all")
    color = np.full((h, w, 3), -1234.5, np.float32)
    count = np.full((h, w), -1234.5, np.float32)
    mom = np.full((h, w, 2), -1234.5, np.float32)
    clp = np.full((h, w), -1234.5, np.float32)
    rgba = np.full((h, w, 4), 0xA5, np.uint8)
    albedo, pmom = np.ascontiguousarray(cur["albedo"]), np.ascontiguousarray(prev["moments"])
    table = np.array(TABLE)
    keep = []
    T, K = rtgo.default_temporal, rtgo.default_history_clip
    nan, inf = float("nan"), float("inf")
    A = lambda a: a.ctypes.data if a is not None else None

    def call(params=T(), clip=K(**clip_of(w, h)), w=w, h=h, cur_on=True, prev_on=True, color_out=color, count_out=count,
             mom_out=mom, clp_out=clp, cur_albedo=albedo, prev_mom=pmom, cur_drop=(), prev_drop=(), prev_frame=None,
             alias=None, motion_on=True, table_ptr=table.ctypes.data, rows=3, entry=lib.rt_temporal_clip_host):
        c = {k: v for k, v in cur.items() if k not in cur_drop}
        p = {k: v for k, v in prev.items() if k not in prev_drop}
        if prev_frame is not None:
            p["frame"] = prev_frame
        fc, fp = _frames(c, p, keep)
        if alias == "color":
            fp.color = color_out.ctypes.data
        if alias == "count":
            fp.count = count_out.ctypes.data
        m = rtgo.Motion(table_ptr, rows, 0)
        args = [ctypes.byref(params) if params is not None else None, w, h, ctypes.byref(fc) if cur_on else None,
                ctypes.byref(fp) if prev_on else None, ctypes.byref(m) if motion_on else None,
                ctypes.byref(clip) if clip is not None else None, A(cur_albedo),
                A(mom_out) if alias == "moments" else A(prev_mom), A(color_out), A(count_out), A(mom_out), A(clp_out),
                rgba.ctypes.data]
        return entry(*args) if entry is lib.rt_temporal_clip_host else entry(*args, None)

    zero_h = np.array(prev["frame"], np.float64)
    zero_h[6:9] = 0
    nan_frame = np.array(prev["frame"], np.float64)
    nan_frame[11] = nan
    colour_only = dict(mom_out=None, prev_mom=None)
    cases = {
        # the clip's own rules
        "NULL clip": dict(clip=None), "radius -1": dict(clip=K(radius=-1)), "radius 5": dict(clip=K(radius=5)),
        "min_taps 0": dict(clip=K(min_taps=0)), "min_taps -3": dict(clip=K(min_taps=-3)),
        "gamma < 0": dict(clip=K(gamma=-0.25)), "gamma NaN": dict(clip=K(gamma=nan)), "gamma inf": dict(clip=K(gamma=inf)),
        "min_half < 0": dict(clip=K(min_half=-1e-9)), "min_half NaN": dict(clip=K(min_half=nan)),
        "min_half -inf": dict(clip=K(min_half=-inf)),
        "out_clipped == out_color": dict(clp_out=color), "out_clipped == out_count": dict(clp_out=count),
        "out_clipped == out_moments": dict(clp_out=mom),
        # the table's
        "NULL table": dict(table_ptr=None), "num_objects 0": dict(rows=0), "num_objects -1": dict(rows=-1),
        "a table, NULL cur.object": dict(cur_drop=("object",)), "a table, NULL prev.object": dict(prev_drop=("object",)),
        "a table, NULL object in both frames": dict(cur_drop=("object",), prev_drop=("object",)),
        # without a table: ids in both frames or in neither
        "no table, object in cur only": dict(motion_on=False, prev_drop=("object",)),
        "no table, object in prev only": dict(motion_on=False, cur_drop=("object",)),
        # the moments'
        "prev_moments without out_moments": dict(colour_only, prev_mom=pmom),
        "prev without prev_moments": dict(prev_mom=None), "prev_moments without prev": dict(prev_on=False),
        "out_moments == prev_moments": dict(alias="moments"),
        # rt_temporal_async's
        "NULL params": dict(params=None), "NULL cur": dict(cur_on=False),
        "NULL cur.color": dict(cur_drop=("color",)), "NULL cur.depth": dict(cur_drop=("depth",)),
        "NULL prev.color": dict(prev_drop=("color",)), "NULL prev.depth": dict(prev_drop=("depth",)),
        "NULL prev.count": dict(prev_drop=("count",)),
        "normal in cur only": dict(prev_drop=("normal",)), "normal in prev only": dict(cur_drop=("normal",)),
        "NULL out_color": dict(color_out=None), "NULL out_count": dict(count_out=None),
        "out_color == prev.color": dict(alias="color"), "out_count == prev.count": dict(alias="count"),
        "w = 0": dict(w=0), "h = -1": dict(h=-1), "h = 65537": dict(h=65537), "too many pixels": dict(w=65536, h=65536),
        "max_history 0.5": dict(params=T(max_history=0.5)), "max_history NaN": dict(params=T(max_history=nan)),
        "depth_tol < 0": dict(params=T(depth_tol=-0.01)), "normal_min 1.5": dict(params=T(normal_min=1.5)),
        "min_weight 0": dict(params=T(min_weight=0.0)),
        "NaN in prev.frame": dict(prev_frame=nan_frame), "hh == 0": dict(prev_frame=zero_h),
    }
    for entry in (lib.rt_temporal_clip_host, lib.rt_temporal_clip_async):  # (async: refused before any device)
        tag = b"rt_temporal_clip_host" if entry is lib.rt_temporal_clip_host else b"rt_temporal_clip_async"
        for what, kw in cases.items():
            assert call(entry=entry, **kw) == RT_E_INVALID, (what, entry.__name__)
            msg = lib.rt_last_error()
            assert msg and tag in msg, what
            assert (color == -1234.5).all() and (count == -1234.5).all() and (mom == -1234.5).all() \
                and (clp == -1234.5).all() and (rgba == 0xA5).all(), what
    assert call() == 0  # (the same call with nothing wrong)
    ref = syn_reference(w, h, "all")
    _same(color, ref["color"], "after the refused calls")
    _same(count, ref["count"], "after the refused calls")
    _same(mom, ref["moments"], "after the refused calls")
    _same(clp, ref["clipped"], "after the refused calls")
    assert (rgba[..., 3] == 255).all()
    # allowed: the colour-only form WITH albedo (it feeds the window), no table, no ids, no previous frame,
    # no out_clipped, the extremes of the ranges
    assert call(**colour_only) == 0 and call(cur_albedo=None, **colour_only) == 0
    assert call(motion_on=False) == 0 and call(motion_on=False, cur_drop=("object",), prev_drop=("object",)) == 0
    assert call(prev_on=False, prev_mom=None) == 0 and call(clp_out=None) == 0
    assert call(clip=K(radius=0, min_taps=1, gamma=0.0, min_half=0.0)) == 0
    assert call(clip=K(radius=4, min_taps=2 ** 31 - 1, gamma=1e300, min_half=1e300)) == 0
    with pytest.raises(rtgo.RenderError):
        rtgo.temporal_clip_host(cur, prev, np.zeros((3, 2)))
    with pytest.raises(rtgo.RenderError):
        rtgo.temporal_clip_host(cur, prev, TABLE, clip=dict(radius=9))
    with pytest.raises(rtgo.RenderError):
        rtgo.temporal_clip_host(cur, prev, TABLE, clip=dict(sigma=1.0))


def test_render_sequence_refuses_clip_without_temporal_and_bad_light_offsets_before_any_device():
    r = rtgo.ParallelRenderer(1)
    r.set_samples(1)
    from clip_cases import frame_json

    scene = rtgo.Scene.from_json_text(frame_json("C_FLOOR", 0))
    cams = [cq.CAMERA, cq.CAMERA]
    for clip in (True, "default", dict(radius=2), rtgo.default_history_clip()):
        with pytest.raises(rtgo.RenderError, match="clip"):
            r.render_sequence(scene, 8, 8, cams, clip=clip)
    with pytest.raises(rtgo.RenderError, match="clip"):
        r.render_sequence(scene, 8, 8, cams, temporal=True, clip=dict(sigma=2.0))
    with pytest.raises(rtgo.RenderError, match="clip"):
        r.render_sequence(scene, 8, 8, cams, temporal=True, clip=7)
    for bad in (np.zeros((2, 2, 3)), np.zeros((3, 1, 3)), np.zeros((2, 1, 2)), np.zeros((2, 1))):
        with pytest.raises(rtgo.RenderError, match="light_offsets"):
            r.render_sequence(scene, 8, 8, cams, light_offsets=bad)
    with pytest.raises(rtgo.RenderError, match="light_offsets"):
        r.render_sequence(scene, 8, 8, cams, temporal=True, clip=True, light_offsets=np.full((2, 1, 3), np.inf))
    # Scene.relit moves the lights and nothing else
    lit = scene.relit([[0.5, -1.0, 2.0]])
    assert list(lit.view.lights[0].position) == [-0.5, 4.0, 4.0]
    assert rtgo.scene_motion(scene, lit).tolist() == [[0, 0, 0], [0, 0, 0]]
    with pytest.raises(rtgo.RenderError):
        scene.relit(np.zeros((2, 3)))


# ---- the per-pixel functions under the host sanitizers: a stand-alone program, nothing is loaded into Python
def test_per_pixel_functions_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no g++ (the compiler of the suite's other sanitizer programs)"
    src = os.path.join(ROOT, "tests", "c", "clip_sanitize.cpp")
    exe = str(tmp_path / "clip_sanitize")
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
    assert "clip_sanitize ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


# ---- quality: six one-sample frames at 144x96 against 512 samples of the last one (tests/clip_quality.py)
def _ratios(name):
    fig = cq.figures(name, DEFAULT_CLIP)
    for region, (a, b, n) in fig.items():
        print(f"{name} {region}: {n} pixels, with the clip {a:.5f}, without {b:.5f}, ratio {a / b:.3f}")
    return {region: a / b for region, (a, b, n) in fig.items()}, fig


def test_quality_the_trail_behind_a_moving_shadow():
    """Measured, C_FLOOR with the defaults (radius 1, gamma 1, min_taps 5), RMSE against 512
    samples.  The trail (floor pixels whose 512-sample luminance differs by more than 0.02 between the last frame
    and the frame two before it, 178 pixels): 0.05557 without the clip, 0.04169 with it, ratio 0.750; the bound
    0.875 is the midpoint between 0.750 and 1.  The floor outside the trail (4759 static pixels): 0.00988 ->
    0.00829, ratio 0.839, bound 0.920.  Whole image 0.01086 -> 0.00938: no worse than without the clip."""
    ratio, fig = _ratios("C_FLOOR")
    assert fig["trail"][2] >= 150, fig["trail"][2]
    clipped = cq.accumulate("C_FLOOR", DEFAULT_CLIP)[2]
    assert clipped[cq.masks("C_FLOOR")[1]].mean() > 0.1  # (the clip is at work on the trail)
    assert ratio["trail"] < 0.875, ratio
    assert ratio["static"] < 0.920, ratio
    assert ratio["image"] <= 1.0, ratio


def test_quality_the_floor_under_a_moving_light():
    """Measured, C_LIGHT with the defaults: the floor as a whole (4936 pixels), RMSE against 512
    samples 0.04397 without the clip, 0.01175 with it, ratio 0.267; the bound 0.634 is the midpoint between 0.267
    and 1.  Whole image 0.02724 -> 0.00933."""
    ratio, _ = _ratios("C_LIGHT")
    assert ratio["floor"] < 0.634, ratio
    assert ratio["image"] <= 1.0, ratio


def test_quality_static_content_is_not_hurt():
    """Measured, S_CUBE standing still under a fixed camera, the defaults: whole image RMSE
    against 512 samples 0.00881 without the clip, 0.00869 with it, ratio 0.985; the bound 0.993 is the midpoint
    between 0.985 and 1 (rounded up to three places).  Over 20 frames the clip costs 1.2 %."""
    ratio, _ = _ratios("S_CUBE")
    assert ratio["image"] < 0.993, ratio


def test_quality_a_clip_that_does_nothing_gains_nothing():
    """The quality tests above fail for a no-op clip: with radius 0 the ratios are exactly 1."""
    fig = cq.figures("C_FLOOR", dict(radius=0))
    assert all(a == b for a, b, _ in fig.values())
