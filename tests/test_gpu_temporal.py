"""GPU: temporal accumulation (rt_temporal_async).

The kernel is held, bit for bit, to rt_temporal_host and to the numpy
restatement of the definition (tests/temporal_reference.py) on the cases of the
CPU tests: a partial wave and a partial block of rows (33x17), one pixel, two
waves per row (70x5), every test off in turn, no previous frame, no out_rgba.
One real chain renders a three-camera look-at orbit of S_CUBE, takes each
frame's feature buffers and accumulates by hand with ping-pong buffers; the
Python layer and the CLI must hand out the same bytes.  The rest pins what the
call promises around the image: a refused call touches nothing and nothing is
written behind an output.  Every case is at most 72x48 pixels; the references
are computed once (temporal_reference.case_reference caches) and shared."""
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
from temporal_reference import CASES, bits, case_inputs, case_reference

pytestmark = pytest.mark.gpu

RT_E_INVALID = -1
W, H, SPP, SEED, ORBIT_N, ORBIT_DEG = 72, 48, 2, 3, 3, 6.0
S_CUBE = scene_json("S_CUBE")
NAMES = ("color", "depth", "object", "normal", "count")
SENT_F, SENT_B, GUARD = -1234.5, 0xA5, 64
EXE = os.path.join(ROOT, "concurrent-raytracer-go_amd", "build", "raytracer")


class _Dev:
    """Device copies of a case's frames and sentinel-filled outputs, each with GUARD elements behind it
    that no call may touch."""

    def __init__(self, cur, prev, w, h):
        import torch

        self.torch, self.w, self.h = torch, w, h
        up = lambda d: {k: torch.from_numpy(np.array(d[k])).cuda() for k in NAMES if d.get(k) is not None}
        self.cur, self.prev = up(cur), (up(prev) if prev is not None else None)
        ptr = lambda t, k: t[k].data_ptr() if k in t else None
        self.fc = rtgo.temporal_frame(cur["frame"], *[ptr(self.cur, k) for k in NAMES])
        self.fp = rtgo.temporal_frame(prev["frame"], *[ptr(self.prev, k) for k in NAMES]) if prev is not None else None
        self.fill()

    def fill(self):
        t, n = self.torch, self.w * self.h
        self.color = t.full((n * 3 + GUARD,), SENT_F, dtype=t.float32, device="cuda")
        self.count = t.full((n + GUARD,), SENT_F, dtype=t.float32, device="cuda")
        self.rgba = t.full((n * 4 + GUARD,), SENT_B, dtype=t.uint8, device="cuda")

    def run(self, params, rgba=True):
        n = self.w * self.h
        rtgo.temporal_async(self.w, self.h, self.fc, self.fp, self.color.data_ptr(), self.count.data_ptr(),
                            self.rgba.data_ptr() if rgba else None, params, 0)
        self.torch.cuda.synchronize()
        # (nothing behind an output was written)
        assert (self.color[n * 3:] == SENT_F).all() and (self.count[n:] == SENT_F).all()
        assert (self.rgba[n * 4:] == SENT_B).all()
        return (self.color[:n * 3].cpu().numpy().reshape(self.h, self.w, 3),
                self.count[:n].cpu().numpy().reshape(self.h, self.w),
                self.rgba[:n * 4].cpu().numpy().reshape(self.h, self.w, 4))

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.color == SENT_F).all() and (self.count == SENT_F).all() and (self.rgba == SENT_B).all())


def _same(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert got.shape == want.shape and got.dtype == want.dtype and bad.size == 0, (what, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host_and_reference_bit_for_bit(name):
    cur, prev, params = case_inputs(name)
    ref_color, ref_count, _ = case_reference(name)
    h, w = cur["depth"].shape
    host_color, host_count, host_rgba = rtgo.temporal_host(cur, prev, params)
    color, count, rgba = _Dev(cur, prev, w, h).run(params)
    _same(color, ref_color, (name, "color, reference"))
    _same(count, ref_count, (name, "count, reference"))
    _same(color, host_color, (name, "color, host"))
    _same(count, host_count, (name, "count, host"))
    assert rgba.tobytes() == host_rgba.tobytes(), name
    if name == "33x17":  # (the comparison is of an accumulation that did something)
        assert (count > 1).mean() > 0.3 and (count == 1).mean() > 0.3 and (count == 0).mean() > 0.1


def test_without_out_rgba():
    cur, prev, params = case_inputs("33x17")
    ref_color, ref_count, _ = case_reference("33x17")
    color, count, rgba = _Dev(cur, prev, 33, 17).run(params, rgba=False)
    _same(color, ref_color, "color")
    _same(count, ref_count, "count")
    assert (rgba == SENT_B).all()


def test_refused_calls_touch_nothing_and_the_same_call_then_succeeds():
    lib = rtgo.lib()
    cur, prev, _ = case_inputs("33x17")
    h, w = cur["depth"].shape
    d = _Dev(cur, prev, w, h)
    T = rtgo.default_temporal

    def call(params=T(), w=w, h=h, cur_on=True, color=True, count=True, edit=None):
        fc, fp = rtgo.TemporalFrame.from_buffer_copy(d.fc), rtgo.TemporalFrame.from_buffer_copy(d.fp)
        if edit:
            edit(fc, fp)
        return lib.rt_temporal_async(ctypes.byref(params) if params is not None else None, w, h,
                                     ctypes.byref(fc) if cur_on else None, ctypes.byref(fp),
                                     d.color.data_ptr() if color else None, d.count.data_ptr() if count else None,
                                     d.rgba.data_ptr(), None)

    def setf(which, name, value):
        def edit(fc, fp):
            setattr(fc if which == "cur" else fp, name, value)
        return edit

    def frame(which, i, v):
        def edit(fc, fp):
            (fc if which == "cur" else fp).frame[i] = v
        return edit

    def zero_h(fc, fp):
        fp.frame[6] = fp.frame[7] = fp.frame[8] = 0.0

    cases = {
        "NULL params": dict(params=None), "NULL cur": dict(cur_on=False),
        "NULL cur.color": dict(edit=setf("cur", "color", None)), "NULL cur.depth": dict(edit=setf("cur", "depth", None)),
        "NULL prev.color": dict(edit=setf("prev", "color", None)), "NULL prev.count": dict(edit=setf("prev", "count", None)),
        "object in cur only": dict(edit=setf("prev", "object", None)),
        "normal in prev only": dict(edit=setf("cur", "normal", None)),
        "NULL out_color": dict(color=False), "NULL out_count": dict(count=False),
        "out_color == prev.color": dict(edit=setf("prev", "color", d.color.data_ptr())),
        "out_count == prev.count": dict(edit=setf("prev", "count", d.count.data_ptr())),
        "w = 0": dict(w=0), "h = 65537": dict(h=65537), "too many pixels": dict(w=65536, h=65536),
        "max_history 0": dict(params=T(max_history=0.0)), "max_history NaN": dict(params=T(max_history=float("nan"))),
        "depth_tol < 0": dict(params=T(depth_tol=-1.0)), "normal_min 2": dict(params=T(normal_min=2.0)),
        "min_weight 0": dict(params=T(min_weight=0.0)), "min_weight inf": dict(params=T(min_weight=float("inf"))),
        "NaN in cur.frame": dict(edit=frame("cur", 5, float("nan"))),
        "inf in prev.frame": dict(edit=frame("prev", 0, float("inf"))),
        "hh == 0": dict(edit=zero_h),
    }
    for what, kw in cases.items():
        assert call(**kw) == RT_E_INVALID, what
        assert lib.rt_last_error(), what
        assert d.untouched(), what
    assert call() == 0  # (the same call with nothing wrong)
    d.torch.cuda.synchronize()
    n = w * h
    _same(d.color[:n * 3].cpu().numpy().reshape(h, w, 3), case_reference("33x17")[0], "after the refused calls")
    _same(d.count[:n].cpu().numpy().reshape(h, w), case_reference("33x17")[1], "after the refused calls")


def _settings(seed=SEED):
    return make_settings(rtgo, {"samples": SPP, "max_depth": 50, "camera": rtgo.RT_CAMERA_LOOKAT}, seed)


def _cameras():
    return rtgo.camera_orbit(rtgo.Scene.from_json_text(S_CUBE), ORBIT_N, ORBIT_DEG)


@functools.lru_cache(maxsize=None)
def _chain():
    """The real chain at 72x48x2 on S_CUBE, by hand: one render_cameras_async of the three views (seed
    SEED + f), then per frame render_aov_async and rt_temporal_async with ping-pong buffers.  Returns, per
    frame, the downloaded inputs (raw colour and features) and outputs."""
    import torch

    cams = _cameras()
    ctx = rtgo.Context(0)
    ctx.set_scene(rtgo.Scene.from_json_text(S_CUBE))
    n = W * H
    lin = torch.zeros((ORBIT_N, n * 3), dtype=torch.float32, device="cuda")
    ctx.render_cameras_async(W, H, _settings(), cams, [lin[f].data_ptr() for f in range(ORBIT_N)], None,
                             seeds=[SEED + f for f in range(ORBIT_N)], stream=0)
    feat = [{k: torch.zeros(n * (3 if k in ("albedo", "normal") else 1),
                            dtype=torch.int32 if k == "object" else torch.float32, device="cuda")
             for k in ("albedo", "normal", "depth", "object")} for _ in range(2)]
    acc = [torch.zeros(n * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
    cnt = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(2)]
    rgba = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    prev, frames = None, []
    for f in range(ORBIT_N):
        ft = feat[f & 1]
        ctx.render_aov_async(W, H, _settings(SEED + f),
                             rtgo.AovBuffers(ft["albedo"].data_ptr(), ft["normal"].data_ptr(), ft["depth"].data_ptr(),
                                             None, ft["object"].data_ptr()), camera=cams[f])
        cam_frame = rtgo.camera_frame(cams[f], "lookat", W, H)
        cur = rtgo.temporal_frame(cam_frame, lin[f].data_ptr(), ft["depth"].data_ptr(), ft["object"].data_ptr(),
                                  ft["normal"].data_ptr())
        rtgo.temporal_async(W, H, cur, prev, acc[f & 1].data_ptr(), cnt[f & 1].data_ptr(), rgba.data_ptr())
        prev = rtgo.temporal_frame(cam_frame, acc[f & 1].data_ptr(), ft["depth"].data_ptr(), ft["object"].data_ptr(),
                                   ft["normal"].data_ptr(), cnt[f & 1].data_ptr())
        torch.cuda.synchronize()  # (download this frame before its buffers are reused)
        shape = lambda k: (H, W, 3) if k in ("albedo", "normal") else (H, W)
        frames.append(dict(
            {k: ft[k].cpu().numpy().reshape(shape(k)) for k in ft}, frame=cam_frame,
            raw=lin[f].cpu().numpy().reshape(H, W, 3), color=acc[f & 1].cpu().numpy().reshape(H, W, 3),
            count=cnt[f & 1].cpu().numpy().reshape(H, W), rgba=rgba.cpu().numpy().reshape(H, W, 4)))
    ctx.close()
    return frames


def test_real_chain_equals_the_host_function_of_the_downloaded_inputs():
    frames = _chain()
    state = None
    for f, fr in enumerate(frames):
        cur = dict(color=fr["raw"], depth=fr["depth"], object=fr["object"], normal=fr["normal"], frame=fr["frame"])
        color, count, rgba = rtgo.temporal_host(cur, state)
        _same(fr["color"], color, (f, "color"))
        _same(fr["count"], count, (f, "count"))
        assert fr["rgba"].tobytes() == rgba.tobytes(), f
        state = dict(cur, color=color, count=count)
    valid = np.isfinite(frames[2]["depth"])
    assert 300 < valid.sum() < W * H and len(np.unique(frames[2]["object"][valid])) == 4
    share = (frames[2]["count"][valid] > 1).mean()
    assert share >= 0.90, share
    assert (frames[2]["count"][valid] == 3).mean() > 0.5 and (frames[0]["count"][np.isfinite(frames[0]["depth"])] == 1).all()
    assert not np.array_equal(frames[0]["frame"], frames[1]["frame"])  # (the camera really moves)
    assert (bits(frames[2]["color"]) != bits(frames[2]["raw"])).any(axis=-1)[valid].mean() > 0.85


def _renderer():
    r = rtgo.ParallelRenderer(1)
    r.set_samples(SPP)
    r.set_seed(SEED)
    r.set_camera("lookat")
    return r


def test_render_sequence_temporal_hands_out_the_chain():
    frames = _chain()
    scene = rtgo.Scene.from_json_text(S_CUBE)
    cams = _cameras()
    r = _renderer()
    img = r.render_sequence(scene, W, H, cams, temporal=True)  # (seeds None: SEED + f)
    assert img.shape == (ORBIT_N, H, W, 4) and r.last_temporal_linear.shape == (ORBIT_N, H, W, 3)
    assert r.last_history.shape == (ORBIT_N, H, W) and r.last_denoised_linear is None
    for f, fr in enumerate(frames):
        assert img[f].tobytes() == fr["rgba"].tobytes(), f
        _same(r.last_temporal_linear[f], fr["color"], (f, "last_temporal_linear"))
        _same(r.last_history[f], fr["count"], (f, "last_history"))
        _same(r.last_linear[f], fr["raw"], (f, "last_linear stays the raw render"))
    raw_temporal = r.last_linear.copy()
    # the raw renders are those of the plain call with the same explicit seeds, and that call is what it was
    seeds = [SEED + f for f in range(ORBIT_N)]
    plain = r.render_sequence(scene, W, H, cams, seeds)
    assert r.last_linear.tobytes() == raw_temporal.tobytes()
    import torch

    ctx = rtgo.Context(0)
    ctx.set_scene(scene)
    lin = torch.zeros((ORBIT_N, W * H * 3), dtype=torch.float32, device="cuda")
    out = torch.zeros((ORBIT_N, W * H * 4), dtype=torch.uint8, device="cuda")
    ctx.render_cameras_async(W, H, r.settings, cams, [lin[f].data_ptr() for f in range(ORBIT_N)],
                             [out[f].data_ptr() for f in range(ORBIT_N)], seeds=seeds, stream=0)
    torch.cuda.synchronize()
    assert plain.tobytes() == out.cpu().numpy().tobytes() and r.last_linear.tobytes() == lin.cpu().numpy().tobytes()
    plain_none = r.render_sequence(scene, W, H, cams)  # (seeds None without temporal: the renderer's seed for all)
    ctx.render_cameras_async(W, H, r.settings, cams, [lin[f].data_ptr() for f in range(ORBIT_N)],
                             [out[f].data_ptr() for f in range(ORBIT_N)], stream=0)
    torch.cuda.synchronize()
    assert plain_none.tobytes() == out.cpu().numpy().tobytes()
    ctx.close()
    # other parameters reach the kernel
    r.render_sequence(scene, W, H, cams, temporal={"max_history": 2})
    assert r.last_history.max() == 2 and (r.last_history[2] == 2).any()
    r.close()


def test_render_sequence_temporal_and_denoise():
    frames = _chain()
    scene = rtgo.Scene.from_json_text(S_CUBE)
    r = _renderer()
    img = r.render_sequence(scene, W, H, _cameras(), temporal=rtgo.default_temporal(), denoise=True)
    assert r.last_denoised_linear.shape == (ORBIT_N, H, W, 3)
    for f, fr in enumerate(frames):
        # the unfiltered accumulation is what is fed back: it is the chain's
        _same(r.last_temporal_linear[f], fr["color"], (f, "last_temporal_linear"))
        want_lin, want_rgba = rtgo.denoise_host(r.last_temporal_linear[f], fr["normal"], fr["depth"], fr["albedo"],
                                                fr["object"])
        _same(r.last_denoised_linear[f], want_lin, (f, "last_denoised_linear"))
        assert img[f].tobytes() == want_rgba.tobytes(), f
        assert img[f].tobytes() != fr["rgba"].tobytes(), f
    # denoise alone is refused, as the CLI refuses --denoise --orbit without --temporal
    with pytest.raises(rtgo.RenderError, match="temporal"):
        r.render_sequence(scene, W, H, _cameras(), denoise=True)
    # a later call that computes neither leaves no stale result behind
    r.render_sequence(scene, W, H, _cameras())
    assert r.last_denoised_linear is None and r.last_temporal_linear is None and r.last_history is None
    r.close()


def _ppm(path):
    toks = open(path).read().split()
    w, h = int(toks[1]), int(toks[2])
    assert toks[0] == "P3" and toks[3] == "255"
    return np.array(toks[4:], np.int64).reshape(h, w, 3)


def test_cli_temporal_writes_the_python_result_and_refuses_bad_combinations(tmp_path):
    frames = _chain()
    scene = tmp_path / "s_cube.json"
    scene.write_text(S_CUBE)
    out = tmp_path / "o.ppm"
    base = [EXE, str(scene), str(out), str(W), str(H), "--samples", str(SPP), "--seed", str(SEED), "--camera", "lookat"]
    orbit = ["--orbit", f"{ORBIT_N},{ORBIT_DEG}"]
    p = subprocess.run(base + orbit + ["--temporal", "default"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    for f, fr in enumerate(frames):
        assert np.array_equal(_ppm(tmp_path / f"o_{f:04d}.ppm"), fr["rgba"][..., :3].astype(np.int64)), f
    # a SPEC with fields and --denoise, against the Python layer
    r = _renderer()
    want = r.render_sequence(rtgo.Scene.from_json_text(S_CUBE), W, H, _cameras(),
                             temporal={"max_history": 2, "depth_tol": 0.1, "normal_min": 0.5}, denoise=True)
    r.close()
    p = subprocess.run(base + orbit + ["--temporal", "2,0.1,0.5", "--denoise", "default"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    for f in range(ORBIT_N):
        assert np.array_equal(_ppm(tmp_path / f"o_{f:04d}.ppm"), want[f][..., :3].astype(np.int64)), f
    for f in tmp_path.glob("o_*.ppm"):
        f.unlink()
    refused = {
        "without --orbit": base + ["--temporal", "default"],
        "a malformed SPEC": base + orbit + ["--temporal", "32,abc"],
        "an empty field": base + orbit + ["--temporal", "32,,0.9"],
        "a fourth field": base + orbit + ["--temporal", "32,0.05,0.9,0.25"],
        "max_history 0": base + orbit + ["--temporal", "0"],
        "--samples 0": base[:5] + ["--samples", "0", "--camera", "lookat"] + orbit + ["--temporal", "default"],
        "no SPEC": base + orbit + ["--temporal"],
    }
    for what, cmd in refused.items():
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0, what
        assert "--temporal" in p.stderr, (what, p.stderr)
        assert not list(tmp_path.glob("o*.ppm")), what
