"""GPU: variance-guided denoising (rt_temporal_moments_async, rt_variance_async,
rt_denoise_var_async).

Each kernel is held, bit for bit, to its _host twin and to the numpy
restatement of the definitions (tests/variance_reference.py) on the cases of
the CPU tests: a partial wave and a partial block of rows (33x17), one pixel,
two waves per row (70x5), an image smaller than every window (3x2), levels 1
and 5, every mechanism off in turn, every optional buffer and output NULL.  One
real chain renders the three-camera look-at orbit of S_CUBE of
test_gpu_temporal.py and runs the moments pass with ping-pong buffers, the
variance pass and the filter by hand; the Python layer and the CLI must hand
out the same bytes.  The rest pins what the calls promise around the image: a
refused call touches nothing and nothing is written behind an output or the
workspace.  Every case is at most 72x48 pixels; the references are computed
once (variance_reference's caches) and shared."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import rtgo
from conftest import ROOT
from scene_cases import make_settings
from sequence_cases import scene_json
from variance_reference import (FILTER_CASES, MOMENTS_CASES, VARIANCE_CASES, bits, filter_case_reference,
                                moments_case_reference, moments_inputs, spatial_inputs, variance_case_reference)

pytestmark = pytest.mark.gpu

RT_E_INVALID = -1
W, H, SPP, SEED, ORBIT_N, ORBIT_DEG = 72, 48, 2, 3, 3, 6.0
S_CUBE = scene_json("S_CUBE")
SENT_F, SENT_B, GUARD = -1234.5, 0xA5, 64
EXE = os.path.join(ROOT, "concurrent-raytracer-go_amd", "build", "raytracer")
FRAME_NAMES = ("color", "depth", "object", "normal", "count")


def _same(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert got.shape == want.shape and got.dtype == want.dtype and bad.size == 0, (what, len(bad), bad[:4].tolist())


def _up(d, names):
    import torch

    return {k: torch.from_numpy(np.array(d[k])).cuda() for k in names if d.get(k) is not None}


def _ptr(t, k):
    return t[k].data_ptr() if k in t else None


class _Out:
    """Sentinel-filled device outputs, each with GUARD elements behind it that no call may touch."""

    def __init__(self, **sizes):
        import torch

        self.torch, self.sizes = torch, sizes
        self.t = {k: torch.full((n + GUARD,), SENT_B if k in ("rgba", "work") else SENT_F,
                                dtype=torch.uint8 if k in ("rgba", "work") else torch.float32, device="cuda")
                  for k, n in sizes.items()}

    def ptr(self, k):
        return self.t[k].data_ptr()

    def get(self, k, shape):
        n = self.sizes[k]
        return self.t[k][:n].cpu().numpy().reshape(shape)

    def guards_intact(self):
        self.torch.cuda.synchronize()
        return all(bool((t[self.sizes[k]:] == (SENT_B if k in ("rgba", "work") else SENT_F)).all())
                   for k, t in self.t.items())

    def untouched(self, *names):
        self.torch.cuda.synchronize()
        return all(bool((self.t[k] == (SENT_B if k in ("rgba", "work") else SENT_F)).all())
                   for k in (names or self.t))


# ---- the moments pass
def _moments_device(cur, prev, params, rgba=True):
    h, w = cur["depth"].shape
    n = w * h
    dc, dp = _up(cur, FRAME_NAMES + ("albedo",)), (_up(prev, FRAME_NAMES + ("moments",)) if prev is not None else None)
    fc = rtgo.temporal_frame(cur["frame"], *[_ptr(dc, k) for k in FRAME_NAMES])
    fp = rtgo.temporal_frame(prev["frame"], *[_ptr(dp, k) for k in FRAME_NAMES]) if prev is not None else None
    out = _Out(color=n * 3, count=n, moments=n * 2, rgba=n * 4)
    rtgo.temporal_moments_async(w, h, fc, fp, _ptr(dc, "albedo"), _ptr(dp, "moments") if dp else None, out.ptr("color"),
                                out.ptr("count"), out.ptr("moments"), out.ptr("rgba") if rgba else None, params, 0)
    assert out.guards_intact()
    return out.get("color", (h, w, 3)), out.get("count", (h, w)), out.get("moments", (h, w, 2)), out.get("rgba", (h, w, 4))


@pytest.mark.parametrize("name", MOMENTS_CASES)
def test_moments_device_equals_host_and_reference_bit_for_bit(name):
    cur, prev, params = moments_inputs(name)
    ref = moments_case_reference(name)
    host = rtgo.temporal_moments_host(cur, prev, params)
    dev = _moments_device(cur, prev, params)
    for i, what in enumerate(("color", "count", "moments")):
        _same(dev[i], ref[i], (name, what, "reference"))
        _same(dev[i], host[i], (name, what, "host"))
    assert dev[3].tobytes() == host[3].tobytes(), name
    if name == "33x17":  # (the comparison is of an accumulation that did something)
        assert (dev[1] > 1).mean() > 0.3 and (dev[1] == 1).mean() > 0.3 and (dev[1] == 0).mean() > 0.1


def test_moments_without_out_rgba():
    cur, prev, params = moments_inputs("33x17")
    dev = _moments_device(cur, prev, params, rgba=False)
    _same(dev[2], moments_case_reference("33x17")[2], "moments")
    assert (dev[3] == SENT_B).all()


# ---- the variance pass
VNAMES = ("color", "normal", "depth", "albedo", "object", "moments", "count")


def _variance_device(inp, params):
    h, w = inp["depth"].shape
    d = _up(inp, VNAMES)
    out = _Out(var=w * h)
    rtgo.variance_async(w, h, *[_ptr(d, k) for k in VNAMES], out.ptr("var"), params, 0)
    assert out.guards_intact()
    return out.get("var", (h, w))


@pytest.mark.parametrize("name", VARIANCE_CASES)
def test_variance_device_equals_host_and_reference_bit_for_bit(name):
    inp, vp, _ = spatial_inputs(name)
    dev = _variance_device(inp, vp)
    _same(dev, variance_case_reference(name)[0], (name, "reference"))
    _same(dev, rtgo.variance_host(*[inp[k] for k in VNAMES], vp), (name, "host"))


# ---- the filter
FNAMES = ("color", "normal", "depth", "variance", "albedo", "object")


def _filter_device(inp, params, outs=("lin", "rgba", "var"), in_place=False):
    h, w = inp["depth"].shape
    n = w * h
    d = _up(inp, FNAMES)
    nbytes = rtgo.denoise_var_workspace_bytes(w, h)
    out = _Out(lin=n * 3, rgba=n * 4, var=n, work=nbytes)
    lin_ptr = d["color"].data_ptr() if in_place else out.ptr("lin")
    rtgo.denoise_var_async(w, h, *[_ptr(d, k) for k in FNAMES], lin_ptr if "lin" in outs else None,
                           out.ptr("rgba") if "rgba" in outs else None, out.ptr("var") if "var" in outs else None,
                           out.ptr("work"), nbytes, params, 0)
    assert out.guards_intact()
    lin = d["color"].cpu().numpy().reshape(h, w, 3) if in_place else out.get("lin", (h, w, 3))
    return lin, out.get("rgba", (h, w, 4)), out.get("var", (h, w))


@pytest.mark.parametrize("name", FILTER_CASES)
def test_filter_device_equals_host_and_reference_bit_for_bit(name):
    inp, _, fp = spatial_inputs(name)
    ref_lin, ref_var = filter_case_reference(name)
    host = rtgo.denoise_var_host(*[inp[k] for k in FNAMES], fp)
    lin, rgba, var = _filter_device(inp, fp)
    _same(lin, ref_lin, (name, "linear, reference"))
    _same(var, ref_var, (name, "variance, reference"))
    _same(lin, host[0], (name, "linear, host"))
    _same(var, host[2], (name, "variance, host"))
    assert rgba.tobytes() == host[1].tobytes(), name


def test_filter_optional_outputs_and_in_place():
    inp, _, fp = spatial_inputs("33x17")
    ref_lin, ref_var = filter_case_reference("33x17")
    host_rgba = rtgo.denoise_var_host(*[inp[k] for k in FNAMES], fp)[1]
    lin, rgba, var = _filter_device(inp, fp, outs=("lin",))  # out_rgba NULL, out_variance NULL
    _same(lin, ref_lin, "linear alone")
    assert (rgba == SENT_B).all() and (var == SENT_F).all()
    lin, rgba, var = _filter_device(inp, fp, outs=("rgba", "var"))  # out_linear NULL
    assert rgba.tobytes() == host_rgba.tobytes() and (lin == SENT_F).all()
    _same(var, ref_var, "variance")
    lin, rgba, _ = _filter_device(inp, fp, in_place=True)  # out_linear == color
    _same(lin, ref_lin, "in place")
    assert rgba.tobytes() == host_rgba.tobytes()


def test_refused_calls_touch_nothing_and_the_same_calls_then_succeed():
    lib = rtgo.lib()
    cur, prev, _ = moments_inputs("33x17")
    inp, _, fp = spatial_inputs("33x17")
    h, w = cur["depth"].shape
    n = w * h
    dc, dp = _up(cur, FRAME_NAMES + ("albedo",)), _up(prev, FRAME_NAMES + ("moments",))
    di = _up(inp, VNAMES + ("variance",))
    nbytes = rtgo.denoise_var_workspace_bytes(w, h)
    out = _Out(color=n * 3, count=n, moments=n * 2, rgba=n * 4, var=n, lin=n * 3, work=nbytes)
    T, V = rtgo.default_temporal, rtgo.default_variance
    D = lambda **kw: rtgo.default_denoise_var(**dict(fp, **kw))
    nan = float("nan")

    def moments(params=T(), w=w, h=h, prev_on=True, moments_on=True, out_moments=True, alias=False):
        fc = rtgo.temporal_frame(cur["frame"], *[_ptr(dc, k) for k in FRAME_NAMES])
        fpv = rtgo.temporal_frame(prev["frame"], *[_ptr(dp, k) for k in FRAME_NAMES])
        pm = out.ptr("moments") if alias else (dp["moments"].data_ptr() if moments_on else None)
        return lib.rt_temporal_moments_async(ctypes.byref(params), w, h, ctypes.byref(fc),
                                             ctypes.byref(fpv) if prev_on else None, dc["albedo"].data_ptr(), pm,
                                             out.ptr("color"), out.ptr("count"), out.ptr("moments") if out_moments else None,
                                             out.ptr("rgba"), None)

    def variance(params=V(), w=w, drop=(), out_on=True):
        vi = rtgo.VarianceInputs(*[None if k in drop else _ptr(di, k) for k in VNAMES])
        return lib.rt_variance_async(ctypes.byref(params), w, h, ctypes.byref(vi), out.ptr("var") if out_on else None, None)

    def filt(params=None, w=w, drop=(), outs=True, work_bytes=nbytes, work_on=True):
        params = D() if params is None else params
        fi = rtgo.DenoiseInputs(*[None if k in drop else _ptr(di, k) for k in ("color", "normal", "depth", "albedo", "object")])
        return lib.rt_denoise_var_async(ctypes.byref(params), w, h, ctypes.byref(fi),
                                        None if "variance" in drop else di["variance"].data_ptr(),
                                        out.ptr("lin") if outs else None, out.ptr("rgba") if outs else None, out.ptr("var"),
                                        out.ptr("work") if work_on else None, work_bytes, None)

    cases = {
        "moments: prev without prev_moments": lambda: moments(moments_on=False),
        "moments: prev_moments without prev": lambda: moments(prev_on=False),
        "moments: NULL out_moments": lambda: moments(out_moments=False),
        "moments: out_moments == prev_moments": lambda: moments(alias=True),
        "moments: w = 0": lambda: moments(w=0), "moments: max_history NaN": lambda: moments(params=T(max_history=nan)),
        "variance: NULL depth": lambda: variance(drop=("depth",)), "variance: NULL out_var": lambda: variance(out_on=False),
        "variance: moments without count": lambda: variance(drop=("count",)),
        "variance: too wide": lambda: variance(w=65537), "variance: min_history 0": lambda: variance(params=V(min_history=0.0)),
        "variance: sigma_depth NaN": lambda: variance(params=V(sigma_depth=nan)),
        "filter: NULL variance": lambda: filt(drop=("variance",)), "filter: NULL color": lambda: filt(drop=("color",)),
        "filter: both images NULL": lambda: filt(outs=False), "filter: w = 0": lambda: filt(w=0),
        "filter: levels 9": lambda: filt(params=D(levels=9)), "filter: sigma_lum NaN": lambda: filt(params=D(sigma_lum=nan)),
        "filter: prefilter 2": lambda: filt(params=D(prefilter=2)), "filter: NULL workspace": lambda: filt(work_on=False),
        "filter: a workspace one byte short": lambda: filt(work_bytes=nbytes - 1),
    }
    for what, call in cases.items():
        assert call() == RT_E_INVALID, what
        assert lib.rt_last_error(), what
        assert out.untouched(), what
    assert moments() == 0 and variance() == 0 and filt() == 0  # (the same calls with nothing wrong)
    assert out.guards_intact()
    _same(out.get("moments", (h, w, 2)), moments_case_reference("33x17")[2], "moments after the refused calls")
    _same(out.get("var", (h, w)), filter_case_reference("33x17")[1], "variance after the refused calls")
    _same(out.get("lin", (h, w, 3)), filter_case_reference("33x17")[0], "linear after the refused calls")


# ---- the real chain
def _settings(seed=SEED):
    return make_settings(rtgo, {"samples": SPP, "max_depth": 50, "camera": rtgo.RT_CAMERA_LOOKAT}, seed)


def _cameras():
    return rtgo.camera_orbit(rtgo.Scene.from_json_text(S_CUBE), ORBIT_N, ORBIT_DEG)


@functools.lru_cache(maxsize=None)
def _chain():
    """The real chain at 72x48x2 on S_CUBE, by hand: one render_cameras_async of the three views (seed
    SEED + f), then per frame render_aov_async, the moments pass with ping-pong buffers, the variance pass
    and the filter.  Returns, per frame, the downloaded inputs and outputs."""
    import torch

    cams = _cameras()
    ctx = rtgo.Context(0)
    ctx.set_scene(rtgo.Scene.from_json_text(S_CUBE))
    n = W * H
    f32 = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda")
    lin = torch.zeros((ORBIT_N, n * 3), dtype=torch.float32, device="cuda")
    ctx.render_cameras_async(W, H, _settings(), cams, [lin[f].data_ptr() for f in range(ORBIT_N)], None,
                             seeds=[SEED + f for f in range(ORBIT_N)], stream=0)
    feat = [{k: torch.zeros(n * (3 if k in ("albedo", "normal") else 1),
                            dtype=torch.int32 if k == "object" else torch.float32, device="cuda")
             for k in ("albedo", "normal", "depth", "object")} for _ in range(2)]
    acc, cnt, mom = [f32(n * 3) for _ in range(2)], [f32(n) for _ in range(2)], [f32(n * 2) for _ in range(2)]
    var, dlin, fvar = f32(n), f32(n * 3), f32(n)
    rgba = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    nbytes = rtgo.denoise_var_workspace_bytes(W, H)
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    prev, frames = None, []
    for f in range(ORBIT_N):
        ft, i = feat[f & 1], f & 1
        ctx.render_aov_async(W, H, _settings(SEED + f),
                             rtgo.AovBuffers(ft["albedo"].data_ptr(), ft["normal"].data_ptr(), ft["depth"].data_ptr(),
                                             None, ft["object"].data_ptr()), camera=cams[f])
        cam_frame = rtgo.camera_frame(cams[f], "lookat", W, H)
        cur = rtgo.temporal_frame(cam_frame, lin[f].data_ptr(), ft["depth"].data_ptr(), ft["object"].data_ptr(),
                                  ft["normal"].data_ptr())
        rtgo.temporal_moments_async(W, H, cur, prev, ft["albedo"].data_ptr(),
                                    mom[i ^ 1].data_ptr() if prev is not None else None, acc[i].data_ptr(),
                                    cnt[i].data_ptr(), mom[i].data_ptr(), None)
        prev = rtgo.temporal_frame(cam_frame, acc[i].data_ptr(), ft["depth"].data_ptr(), ft["object"].data_ptr(),
                                   ft["normal"].data_ptr(), cnt[i].data_ptr())
        rtgo.variance_async(W, H, acc[i].data_ptr(), ft["normal"].data_ptr(), ft["depth"].data_ptr(),
                            ft["albedo"].data_ptr(), ft["object"].data_ptr(), mom[i].data_ptr(), cnt[i].data_ptr(),
                            var.data_ptr())
        rtgo.denoise_var_async(W, H, acc[i].data_ptr(), ft["normal"].data_ptr(), ft["depth"].data_ptr(), var.data_ptr(),
                               ft["albedo"].data_ptr(), ft["object"].data_ptr(), dlin.data_ptr(), rgba.data_ptr(),
                               fvar.data_ptr(), work.data_ptr(), nbytes)
        torch.cuda.synchronize()  # (download this frame before its buffers are reused)
        shape = lambda k: (H, W, 3) if k in ("albedo", "normal") else (H, W)
        frames.append(dict(
            {k: ft[k].cpu().numpy().reshape(shape(k)) for k in ft}, frame=cam_frame,
            raw=lin[f].cpu().numpy().reshape(H, W, 3), color=acc[i].cpu().numpy().reshape(H, W, 3),
            count=cnt[i].cpu().numpy().reshape(H, W), moments=mom[i].cpu().numpy().reshape(H, W, 2),
            var=var.cpu().numpy().reshape(H, W), lin=dlin.cpu().numpy().reshape(H, W, 3),
            fvar=fvar.cpu().numpy().reshape(H, W), rgba=rgba.cpu().numpy().reshape(H, W, 4)))
    ctx.close()
    return frames


def test_real_chain_equals_the_host_functions_of_the_downloaded_inputs():
    frames = _chain()
    state = None
    for f, fr in enumerate(frames):
        cur = dict(color=fr["raw"], depth=fr["depth"], object=fr["object"], normal=fr["normal"], albedo=fr["albedo"],
                   frame=fr["frame"])
        color, count, moments, _ = rtgo.temporal_moments_host(cur, state)
        _same(fr["color"], color, (f, "color"))
        _same(fr["count"], count, (f, "count"))
        _same(fr["moments"], moments, (f, "moments"))
        state = dict(cur, color=color, count=count, moments=moments)
        var = rtgo.variance_host(color, fr["normal"], fr["depth"], fr["albedo"], fr["object"], moments, count)
        _same(fr["var"], var, (f, "variance"))
        lin, rgba, fvar = rtgo.denoise_var_host(color, fr["normal"], fr["depth"], var, fr["albedo"], fr["object"])
        _same(fr["lin"], lin, (f, "filtered"))
        _same(fr["fvar"], fvar, (f, "filtered variance"))
        assert fr["rgba"].tobytes() == rgba.tobytes(), f
    valid = np.isfinite(frames[2]["depth"])
    assert 300 < valid.sum() < W * H and len(np.unique(frames[2]["object"][valid])) == 4
    assert (frames[2]["count"][valid] == 3).mean() > 0.5  # (histories of three frames: below min_history, spatial)
    assert (frames[2]["var"][valid] > 0).mean() > 0.9 and (frames[2]["var"][~valid] == 0).all()
    assert (bits(frames[2]["lin"]) != bits(frames[2]["color"])).any(axis=-1)[valid].mean() > 0.85


def _renderer():
    r = rtgo.ParallelRenderer(1)
    r.set_samples(SPP)
    r.set_seed(SEED)
    r.set_camera("lookat")
    return r


def test_render_sequence_variance_hands_out_the_chain_and_leaves_the_plain_call_alone():
    frames = _chain()
    scene = rtgo.Scene.from_json_text(S_CUBE)
    r = _renderer()
    before = r.render_sequence(scene, W, H, _cameras(), temporal=True)
    before_lin, before_hist = r.last_temporal_linear.copy(), r.last_history.copy()
    assert r.last_variance is None
    img = r.render_sequence(scene, W, H, _cameras(), temporal=True, variance=True)
    assert img.shape == (ORBIT_N, H, W, 4) and r.last_variance.shape == (ORBIT_N, H, W)
    assert r.last_denoised_linear.shape == (ORBIT_N, H, W, 3)
    for f, fr in enumerate(frames):
        assert img[f].tobytes() == fr["rgba"].tobytes(), f
        _same(r.last_temporal_linear[f], fr["color"], (f, "last_temporal_linear"))
        _same(r.last_history[f], fr["count"], (f, "last_history"))
        _same(r.last_variance[f], fr["var"], (f, "last_variance"))
        _same(r.last_denoised_linear[f], fr["lin"], (f, "last_denoised_linear"))
        _same(r.last_temporal_linear[f], before_lin[f], (f, "the accumulation is rt_temporal_async's"))
    # the fields of a dict reach the kernels: min_history 2 sends the pixels with a history to the temporal branch
    r.render_sequence(scene, W, H, _cameras(), temporal=True, variance={"sigma_lum": 1.0, "min_history": 2})
    fr = frames[2]
    var = rtgo.variance_host(fr["color"], fr["normal"], fr["depth"], fr["albedo"], fr["object"], fr["moments"],
                             fr["count"], {"min_history": 2})
    _same(r.last_variance[2], var, "min_history 2")
    assert (bits(var) != bits(fr["var"]))[np.isfinite(fr["depth"])].mean() > 0.5  # (of the valid pixels)
    want = rtgo.denoise_var_host(fr["color"], fr["normal"], fr["depth"], var, fr["albedo"], fr["object"],
                                 {"sigma_lum": 1.0})[0]
    _same(r.last_denoised_linear[2], want, "sigma_lum 1")
    # afterwards the plain call returns what it returned before, and no stale variance
    after = r.render_sequence(scene, W, H, _cameras(), temporal=True)
    assert after.tobytes() == before.tobytes() and r.last_variance is None and r.last_denoised_linear is None
    _same(r.last_temporal_linear, before_lin, "last_temporal_linear")
    _same(r.last_history, before_hist, "last_history")
    r.close()


def test_render_denoised_variance_is_the_spatial_chain_of_one_frame():
    scene = rtgo.Scene.from_json_text(S_CUBE)
    r = _renderer()
    plain = r.render_denoised(scene, W, H)
    plain_lin = r.last_denoised_linear.copy()
    assert r.last_variance is None
    img = r.render_denoised(scene, W, H, variance=True)
    feat = r.render_aov(scene, W, H)
    var = rtgo.variance_host(r.last_linear, feat["normal"], feat["depth"], feat["albedo"], feat["object"])
    _same(r.last_variance, var, "last_variance")
    lin, rgba, _ = rtgo.denoise_var_host(r.last_linear, feat["normal"], feat["depth"], var, feat["albedo"], feat["object"])
    _same(r.last_denoised_linear, lin, "last_denoised_linear")
    assert img.tobytes() == rgba.tobytes() and img.tobytes() != plain.tobytes()
    again = r.render_denoised(scene, W, H)
    assert again.tobytes() == plain.tobytes() and r.last_variance is None
    _same(r.last_denoised_linear, plain_lin, "the plain call is what it was")
    r.close()


def _ppm(path):
    toks = open(path).read().split()
    w, h = int(toks[1]), int(toks[2])
    assert toks[0] == "P3" and toks[3] == "255"
    return np.array(toks[4:], np.int64).reshape(h, w, 3)


def test_cli_denoise_variance_writes_the_python_result_and_refuses_bad_combinations(tmp_path):
    frames = _chain()
    scene = tmp_path / "s_cube.json"
    scene.write_text(S_CUBE)
    out = tmp_path / "o.ppm"
    base = [EXE, str(scene), str(out), str(W), str(H), "--samples", str(SPP), "--seed", str(SEED), "--camera", "lookat"]
    orbit = ["--orbit", f"{ORBIT_N},{ORBIT_DEG}", "--temporal", "default"]
    p = subprocess.run(base + orbit + ["--denoise-variance", "default"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    for f, fr in enumerate(frames):
        assert np.array_equal(_ppm(tmp_path / f"o_{f:04d}.ppm"), fr["rgba"][..., :3].astype(np.int64)), f
    # a SPEC with fields, and the single render, against the Python layer
    r = _renderer()
    want = r.render_sequence(rtgo.Scene.from_json_text(S_CUBE), W, H, _cameras(), temporal=True,
                             variance={"levels": 3, "sigma_lum": 1.0, "sigma_depth": 0.1, "normal_power": 16})
    single = r.render_denoised(rtgo.Scene.from_json_text(S_CUBE), W, H, variance={"levels": 2})
    r.close()
    p = subprocess.run(base + orbit + ["--denoise-variance", "3,1,0.1,16"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    for f in range(ORBIT_N):
        assert np.array_equal(_ppm(tmp_path / f"o_{f:04d}.ppm"), want[f][..., :3].astype(np.int64)), f
    for f in tmp_path.glob("o_*.ppm"):
        f.unlink()
    p = subprocess.run(base + ["--denoise-variance", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert np.array_equal(_ppm(out), single[..., :3].astype(np.int64))
    out.unlink()
    refused = {
        "with --denoise": base + orbit + ["--denoise-variance", "default", "--denoise", "default"],
        "--orbit without --temporal": base + ["--orbit", "3", "--denoise-variance", "default"],
        "a malformed SPEC": base + orbit + ["--denoise-variance", "4,abc"],
        "an empty field": base + orbit + ["--denoise-variance", "4,,0.05"],
        "a fifth field": base + orbit + ["--denoise-variance", "4,2,0.05,32,1"],
        "levels 0": base + orbit + ["--denoise-variance", "0"],
        "sigma_lum < 0": base + orbit + ["--denoise-variance", "4,-1"],
        "no SPEC": base + orbit + ["--denoise-variance"],
        "--pass-samples": base + ["--pass-samples", "1", "--denoise-variance", "default"],
    }
    for what, cmd in refused.items():
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0, what
        assert "--denoise-variance" in p.stderr, (what, p.stderr)
        assert not list(tmp_path.glob("o*.ppm")), what
