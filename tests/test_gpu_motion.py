"""GPU: temporal accumulation with per-object motion (rt_temporal_motion_async,
DESIGN.md §4.17).

The kernels (with and without moments) are held, bit for bit, to
rt_temporal_motion_host and to the numpy restatement (tests/motion_reference.py)
on a partial wave and a partial block of rows (33x17), two waves per row, the
second cut at the image edge (70x5), and one pixel; with a table of zeros they
are held to rt_temporal_async / rt_temporal_moments_async on the device.  A
refused call touches nothing and nothing is written behind an output.  One real
chain renders S_CUBE with its Lambertian sphere moved from frame to frame, by
hand from the public calls; the device result equals the host function of the
downloaded inputs, and render_sequence(offsets=...) and the CLI's --move must
hand out the same bytes, each frame's render being the oracle's render of the
moved scene.  Every case is at most 72x48 pixels; the references are computed
once and shared."""
import copy
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
import rtgo
from conftest import ROOT
from motion_reference import TABLE, bits, case_inputs, case_reference
from scene_cases import make_settings
from sequence_cases import SCENES, at, scene_json

pytestmark = pytest.mark.gpu

RT_E_INVALID = -1
W, H, SEED = 72, 48, 3
MOVE = (0.25, 0.06, 0.0)  # object 1 (the Lambertian sphere) per frame: about 2.5 pixels at 72x48
NAMES = ("color", "depth", "object", "normal", "count")
SENT_F, SENT_B, GUARD = -1234.5, 0xA5, 64
EXE = os.path.join(ROOT, "concurrent-raytracer-go_amd", "build", "raytracer")
KERNEL_CASES = ["33x17", "70x5", "1x1"]


class _Dev:
    """Device copies of a case's frames, the table and sentinel-filled outputs, each output with GUARD
    elements behind it that no call may touch."""

    def __init__(self, cur, prev, w, h, table=TABLE):
        import torch

        self.torch, self.w, self.h = torch, w, h
        up = lambda d: {k: torch.from_numpy(np.array(d[k])).cuda() for k in NAMES + ("albedo", "moments")
                        if d.get(k) is not None}
        self.cur, self.prev = up(cur), (up(prev) if prev is not None else None)
        ptr = lambda t, k: t[k].data_ptr() if k in t else None
        self.fc = rtgo.temporal_frame(cur["frame"], *[ptr(self.cur, k) for k in NAMES])
        self.fp = rtgo.temporal_frame(prev["frame"], *[ptr(self.prev, k) for k in NAMES]) if prev is not None else None
        self.table = torch.from_numpy(np.array(table, np.float64)).cuda()
        self.albedo = ptr(self.cur, "albedo")
        self.pmom = ptr(self.prev, "moments") if prev is not None else None
        self.fill()

    def fill(self):
        t, n = self.torch, self.w * self.h
        self.color = t.full((n * 3 + GUARD,), SENT_F, dtype=t.float32, device="cuda")
        self.count = t.full((n + GUARD,), SENT_F, dtype=t.float32, device="cuda")
        self.mom = t.full((n * 2 + GUARD,), SENT_F, dtype=t.float32, device="cuda")
        self.rgba = t.full((n * 4 + GUARD,), SENT_B, dtype=t.uint8, device="cuda")

    def download(self):
        n = self.w * self.h
        self.torch.cuda.synchronize()
        # (nothing behind an output was written)
        assert (self.color[n * 3:] == SENT_F).all() and (self.count[n:] == SENT_F).all()
        assert (self.mom[n * 2:] == SENT_F).all() and (self.rgba[n * 4:] == SENT_B).all()
        return (self.color[:n * 3].cpu().numpy().reshape(self.h, self.w, 3),
                self.count[:n].cpu().numpy().reshape(self.h, self.w),
                self.mom[:n * 2].cpu().numpy().reshape(self.h, self.w, 2),
                self.rgba[:n * 4].cpu().numpy().reshape(self.h, self.w, 4))

    def run(self, params, moments, rgba=True):
        m = dict(d_cur_albedo=self.albedo, d_prev_moments=self.pmom, d_out_moments=self.mom.data_ptr()) if moments else {}
        rtgo.temporal_motion_async(self.w, self.h, self.fc, self.fp, self.table.data_ptr(), self.table.shape[0],
                                   self.color.data_ptr(), self.count.data_ptr(), self.rgba.data_ptr() if rgba else None,
                                   params, 0, **m)
        return self.download()

    def run_existing(self, params, moments):
        if moments:
            rtgo.temporal_moments_async(self.w, self.h, self.fc, self.fp, self.albedo, self.pmom, self.color.data_ptr(),
                                        self.count.data_ptr(), self.mom.data_ptr(), self.rgba.data_ptr(), params, 0)
        else:
            rtgo.temporal_async(self.w, self.h, self.fc, self.fp, self.color.data_ptr(), self.count.data_ptr(),
                                self.rgba.data_ptr(), params, 0)
        return self.download()

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.color == SENT_F).all() and (self.count == SENT_F).all() and (self.mom == SENT_F).all()
                    and (self.rgba == SENT_B).all())


def _same(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert got.shape == want.shape and got.dtype == want.dtype and bad.size == 0, (what, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("moments", [False, True], ids=["colour", "moments"])
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_device_equals_host_and_reference_bit_for_bit(name, moments):
    cur, prev, params = case_inputs(name, moments)
    ref_color, ref_count, _, ref_mom = case_reference(name, moments)
    h, w = cur["depth"].shape
    host = rtgo.temporal_motion_host(cur, prev, TABLE, params, moments=moments)
    d = _Dev(cur, prev, w, h)
    color, count, mom, rgba = d.run(params, moments)
    _same(color, ref_color, (name, "color, reference"))
    _same(count, ref_count, (name, "count, reference"))
    _same(color, host[0], (name, "color, host"))
    _same(count, host[1], (name, "count, host"))
    assert rgba.tobytes() == host[-1].tobytes(), name
    if moments:
        _same(mom, ref_mom, (name, "moments, reference"))
        _same(mom, host[2], (name, "moments, host"))
    else:
        assert (mom == SENT_F).all()
    if name == "33x17":  # (the comparison is of an accumulation that did something, and the table of one that moved)
        assert (count > 1).mean() > 0.2 and (count == 1).mean() > 0.3 and (count == 0).mean() > 0.1
        zero = case_reference(name, moments, zero=True)
        assert (bits(color) != bits(zero[0])).any(axis=-1).sum() > 100
    # without out_rgba: the same floats, and the image stays what it was
    d.fill()
    color2, count2, mom2, rgba2 = d.run(params, moments, rgba=False)
    _same(color2, ref_color, (name, "color, no out_rgba"))
    _same(count2, ref_count, (name, "count, no out_rgba"))
    if moments:
        _same(mom2, ref_mom, (name, "moments, no out_rgba"))
    assert (rgba2 == SENT_B).all()


@pytest.mark.parametrize("moments", [False, True], ids=["colour", "moments"])
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_a_table_of_zeros_is_the_existing_kernels_bit_for_bit(name, moments):
    cur, prev, params = case_inputs(name, moments)
    h, w = cur["depth"].shape
    d = _Dev(cur, prev, w, h, np.zeros((3, 3)))
    got = d.run(params, moments)
    d.fill()
    want = d.run_existing(params, moments)
    for a, b, what in zip(got, want, ("color", "count", "moments", "rgba")):
        _same(a, b, (name, what))
    # a table that ends before id 2 is the three-row table, whose third row is zero
    d2 = _Dev(cur, prev, w, h, TABLE[:2])
    ref = case_reference(name, moments)
    short = d2.run(params, moments)
    _same(short[0], ref[0], (name, "two rows, color"))
    _same(short[1], ref[1], (name, "two rows, count"))


def test_refused_calls_touch_nothing_and_the_same_call_then_succeeds():
    lib = rtgo.lib()
    cur, prev, _ = case_inputs("33x17", True)
    h, w = cur["depth"].shape
    d = _Dev(cur, prev, w, h)
    T = rtgo.default_temporal

    def call(params=T(), w=w, h=h, cur_on=True, prev_on=True, color=True, count=True, moments=True, albedo=True,
             pmom=True, motion_on=True, table=True, rows=3, edit=None):
        fc, fp = rtgo.TemporalFrame.from_buffer_copy(d.fc), rtgo.TemporalFrame.from_buffer_copy(d.fp)
        if edit:
            edit(fc, fp)
        m = rtgo.Motion(d.table.data_ptr() if table else None, rows, 0)
        return lib.rt_temporal_motion_async(
            ctypes.byref(params) if params is not None else None, w, h, ctypes.byref(fc) if cur_on else None,
            ctypes.byref(fp) if prev_on else None, ctypes.byref(m) if motion_on else None, d.albedo if albedo else None,
            d.pmom if pmom else None, d.color.data_ptr() if color else None, d.count.data_ptr() if count else None,
            d.mom.data_ptr() if moments else None, d.rgba.data_ptr(), None)

    def setf(which, name, value):
        def edit(fc, fp):
            setattr(fc if which == "cur" else fp, name, value)
        return edit

    def zero_h(fc, fp):
        fp.frame[6] = fp.frame[7] = fp.frame[8] = 0.0

    def nan_frame(fc, fp):
        fc.frame[5] = float("nan")

    colour_only = dict(moments=False, albedo=False, pmom=False)
    cases = {
        "NULL motion": dict(motion_on=False), "NULL table": dict(table=False), "num_objects 0": dict(rows=0),
        "num_objects -3": dict(rows=-3),
        "NULL cur.object": dict(edit=setf("cur", "object", None)), "NULL prev.object": dict(edit=setf("prev", "object", None)),
        "albedo without out_moments": dict(colour_only, albedo=True),
        "prev_moments without out_moments": dict(colour_only, pmom=True),
        "prev without prev_moments": dict(pmom=False), "prev_moments without prev": dict(prev_on=False),
        "out_moments == prev_moments": dict(alias=True),
        "NULL params": dict(params=None), "NULL cur": dict(cur_on=False),
        "NULL cur.color": dict(edit=setf("cur", "color", None)), "NULL cur.depth": dict(edit=setf("cur", "depth", None)),
        "NULL prev.color": dict(edit=setf("prev", "color", None)), "NULL prev.count": dict(edit=setf("prev", "count", None)),
        "normal in prev only": dict(edit=setf("cur", "normal", None)),
        "NULL out_color": dict(color=False), "NULL out_count": dict(count=False),
        "out_color == prev.color": dict(edit=setf("prev", "color", d.color.data_ptr())),
        "out_count == prev.count": dict(edit=setf("prev", "count", d.count.data_ptr())),
        "w = 0": dict(w=0), "h = 65537": dict(h=65537), "too many pixels": dict(w=65536, h=65536),
        "max_history 0": dict(params=T(max_history=0.0)), "depth_tol < 0": dict(params=T(depth_tol=-1.0)),
        "normal_min 2": dict(params=T(normal_min=2.0)), "min_weight NaN": dict(params=T(min_weight=float("nan"))),
        "NaN in cur.frame": dict(edit=nan_frame), "hh == 0": dict(edit=zero_h),
    }
    for what, kw in cases.items():
        kw = dict(kw)
        if kw.pop("alias", False):  # out_moments is the previous frame's moments
            fc, fp = rtgo.TemporalFrame.from_buffer_copy(d.fc), rtgo.TemporalFrame.from_buffer_copy(d.fp)
            m = rtgo.Motion(d.table.data_ptr(), 3, 0)
            p = T()
            rc = lib.rt_temporal_motion_async(ctypes.byref(p), w, h, ctypes.byref(fc), ctypes.byref(fp), ctypes.byref(m),
                                              d.albedo, d.mom.data_ptr(), d.color.data_ptr(), d.count.data_ptr(),
                                              d.mom.data_ptr(), d.rgba.data_ptr(), None)
        else:
            rc = call(**kw)
        assert rc == RT_E_INVALID, what
        assert b"rt_temporal_motion_async" in lib.rt_last_error(), what
        assert d.untouched(), what
    assert call() == 0  # (the same call with nothing wrong)
    color, count, mom, _ = d.download()
    ref = case_reference("33x17", True)
    _same(color, ref[0], "after the refused calls")
    _same(count, ref[1], "after the refused calls")
    _same(mom, ref[3], "after the refused calls")


# ---- a real chain: S_CUBE, the reference camera stepping in x, the Lambertian sphere moving
def _offsets(n):
    off = np.zeros((n, 4, 3), np.float64)
    for f in range(n):
        off[f, 1] = [f * v for v in MOVE]
    return off


def _cams(n):
    return [at((0.05 * f, 0, 3)) for f in range(n)]


def _moved_json(f, cam):
    d = copy.deepcopy(SCENES["S_CUBE"])
    d["camera"] = dict(cam)
    d["objects"][1]["position"] = [float(d["objects"][1]["position"][k]) + f * MOVE[k] for k in range(3)]
    return json.dumps(d)


def _settings(spp, seed):
    return make_settings(rtgo, {"samples": spp, "max_depth": 50}, seed)


@functools.lru_cache(maxsize=None)
def _chain(spp, n, moments=False):
    """The chain by hand from the public calls at 72x48: per frame rt_context_set_scene of the moved scene, a
    one-camera render (seed SEED + f), render_aov_async, and rt_temporal_motion_async with
    scene_motion(frame f - 1's scene, frame f's) on the device; buffers ping-pong.  Returns, per frame, the
    downloaded inputs (raw colour and features), the table and the outputs."""
    import torch

    cams = _cams(n)
    base = rtgo.Scene.from_json_text(scene_json("S_CUBE"))
    off = _offsets(n)
    scenes = [base.translated(off[f]) for f in range(n)]
    ctx = rtgo.Context(0)
    npix = W * H
    lin = torch.zeros((n, npix * 3), dtype=torch.float32, device="cuda")
    raw_rgba = torch.zeros((n, npix * 4), dtype=torch.uint8, device="cuda")
    feat = [{k: torch.zeros(npix * (3 if k in ("albedo", "normal") else 1),
                            dtype=torch.int32 if k == "object" else torch.float32, device="cuda")
             for k in ("albedo", "normal", "depth", "object")} for _ in range(2)]
    acc = [torch.zeros(npix * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
    cnt = [torch.zeros(npix, dtype=torch.float32, device="cuda") for _ in range(2)]
    mom = [torch.zeros(npix * 2, dtype=torch.float32, device="cuda") for _ in range(2)]
    rgba = torch.zeros(npix * 4, dtype=torch.uint8, device="cuda")
    prev, frames = None, []
    for f in range(n):
        ft = feat[f & 1]
        ctx.set_scene(scenes[f])
        ctx.render_cameras_async(W, H, _settings(spp, SEED), [cams[f]], [lin[f].data_ptr()], [raw_rgba[f].data_ptr()],
                                 seeds=[SEED + f], stream=0)
        ctx.render_aov_async(W, H, _settings(spp, SEED + f),
                             rtgo.AovBuffers(ft["albedo"].data_ptr(), ft["normal"].data_ptr(), ft["depth"].data_ptr(),
                                             None, ft["object"].data_ptr()), camera=cams[f])
        table = rtgo.scene_motion(scenes[f - 1], scenes[f]) if f else np.zeros((4, 3))
        d_table = torch.from_numpy(table).cuda()
        cam_frame = rtgo.camera_frame(cams[f], "reference", W, H)
        cur = rtgo.temporal_frame(cam_frame, lin[f].data_ptr(), ft["depth"].data_ptr(), ft["object"].data_ptr(),
                                  ft["normal"].data_ptr())
        m = dict(d_cur_albedo=ft["albedo"].data_ptr(), d_prev_moments=mom[(f - 1) & 1].data_ptr() if f else None,
                 d_out_moments=mom[f & 1].data_ptr()) if moments else {}
        rtgo.temporal_motion_async(W, H, cur, prev, d_table.data_ptr(), 4, acc[f & 1].data_ptr(), cnt[f & 1].data_ptr(),
                                   rgba.data_ptr(), None, 0, **m)
        prev = rtgo.temporal_frame(cam_frame, acc[f & 1].data_ptr(), ft["depth"].data_ptr(), ft["object"].data_ptr(),
                                   ft["normal"].data_ptr(), cnt[f & 1].data_ptr())
        torch.cuda.synchronize()  # (download this frame before its buffers are reused)
        shape = lambda k: (H, W, 3) if k in ("albedo", "normal") else (H, W)
        frames.append(dict(
            {k: ft[k].cpu().numpy().reshape(shape(k)) for k in ft}, frame=cam_frame, table=table,
            raw=lin[f].cpu().numpy().reshape(H, W, 3), raw_rgba=raw_rgba[f].cpu().numpy().reshape(H, W, 4),
            color=acc[f & 1].cpu().numpy().reshape(H, W, 3), count=cnt[f & 1].cpu().numpy().reshape(H, W),
            moments=mom[f & 1].cpu().numpy().reshape(H, W, 2), rgba=rgba.cpu().numpy().reshape(H, W, 4)))
    ctx.close()
    return frames


@pytest.mark.parametrize("moments", [False, True], ids=["colour", "moments"])
def test_real_chain_equals_the_host_function_of_the_downloaded_inputs(moments):
    frames = _chain(1, 2, moments)
    state = None
    for f, fr in enumerate(frames):
        cur = dict(color=fr["raw"], depth=fr["depth"], object=fr["object"], normal=fr["normal"], albedo=fr["albedo"],
                   frame=fr["frame"])
        got = rtgo.temporal_motion_host(cur, state, fr["table"], moments=moments)
        _same(fr["color"], got[0], (f, "color"))
        _same(fr["count"], got[1], (f, "count"))
        assert fr["rgba"].tobytes() == got[-1].tobytes(), f
        state = dict(cur, color=got[0], count=got[1])
        if moments:
            _same(fr["moments"], got[2], (f, "moments"))
            state["moments"] = got[2]
    # ((position + offset) - position: the offset to within a rounding of the position, and only object 1's)
    table = frames[1]["table"]
    assert not table[[0, 2, 3]].any() and np.abs(table[1] - np.array(MOVE)).max() <= 2.0 ** -52 and table[1, 0] > 0
    # the sphere moved and kept its history; rt_temporal_host, which does not know that it moved, keeps less
    sphere = frames[1]["object"] == 1
    assert sphere.sum() > 60
    with_motion = (frames[1]["count"][sphere] > 1).mean()
    cur = dict(color=frames[1]["raw"], depth=frames[1]["depth"], object=frames[1]["object"], normal=frames[1]["normal"],
               frame=frames[1]["frame"])
    prev = dict(color=frames[0]["color"], depth=frames[0]["depth"], object=frames[0]["object"],
                normal=frames[0]["normal"], count=frames[0]["count"], frame=frames[0]["frame"])
    static = (rtgo.temporal_host(cur, prev)[1][sphere] > 1).mean()
    print(f"object 1: {int(sphere.sum())} pixels, with a history {with_motion:.3f} (static pass {static:.3f})")
    assert with_motion > 0.8 and with_motion > static + 0.1, (with_motion, static)


def _renderer(spp):
    r = rtgo.ParallelRenderer(1)
    r.set_samples(spp)
    r.set_seed(SEED)
    return r


def test_render_sequence_offsets_is_the_oracle_frame_by_frame_and_the_chain():
    n, spp = 3, 4
    cams, off = _cams(n), _offsets(n)
    scene = rtgo.Scene.from_json_text(scene_json("S_CUBE"))
    r = _renderer(spp)
    seeds = [SEED + f for f in range(n)]
    img = r.render_sequence(scene, W, H, cams, seeds, offsets=off)
    assert img.shape == (n, H, W, 4) and r.last_temporal_linear is None
    for f in range(n):
        moved = rtgo.Scene.from_json_text(_moved_json(f, cams[f]))
        lin, rgba, _ = oracle.render(moved, W, H, _settings(spp, seeds[f]))
        assert img[f].tobytes() == rgba.tobytes(), f
        assert r.last_linear[f].tobytes() == lin.astype(np.float32).tobytes(), f
    assert img[0].tobytes() != img[1].tobytes()
    # seeds None without temporal: the renderer's seed for every frame
    same_seed = r.render_sequence(scene, W, H, cams, offsets=off)
    assert same_seed[0].tobytes() == img[0].tobytes() and same_seed[1].tobytes() != img[1].tobytes()
    # temporal: the chain by hand
    frames = _chain(spp, n)
    acc = r.render_sequence(scene, W, H, cams, temporal=True, offsets=off)  # (seeds None: SEED + f)
    for f, fr in enumerate(frames):
        assert fr["raw_rgba"].tobytes() == img[f].tobytes(), f
        _same(r.last_linear[f], fr["raw"], (f, "last_linear"))
        _same(r.last_temporal_linear[f], fr["color"], (f, "last_temporal_linear"))
        _same(r.last_history[f], fr["count"], (f, "last_history"))
        assert acc[f].tobytes() == fr["rgba"].tobytes(), f
    sphere = frames[2]["object"] == 1
    assert (r.last_history[2][sphere] == 3).mean() > 0.6
    # zero offsets are the plain sequence
    r.render_sequence(scene, W, H, cams, temporal=True, offsets=np.zeros((n, 4, 3)))
    zero_lin, zero_hist = r.last_temporal_linear.copy(), r.last_history.copy()
    r.render_sequence(scene, W, H, cams, temporal=True)
    _same(zero_lin, r.last_temporal_linear, "zero offsets")
    _same(zero_hist, r.last_history, "zero offsets")
    # variance and denoise compose: the accumulation fed back is the chain's, the moments its own chain's
    mframes = _chain(spp, n, True)
    out = r.render_sequence(scene, W, H, cams, temporal=True, variance=True, offsets=off)
    for f, fr in enumerate(mframes):
        _same(r.last_temporal_linear[f], fr["color"], (f, "variance: last_temporal_linear"))
        want_var = rtgo.variance_host(fr["color"], fr["normal"], fr["depth"], fr["albedo"], fr["object"], fr["moments"],
                                      fr["count"])
        _same(r.last_variance[f], want_var, (f, "last_variance"))
    assert out.shape == (n, H, W, 4) and r.last_denoised_linear.shape == (n, H, W, 3)
    r.render_sequence(scene, W, H, cams, temporal=True, denoise=True, offsets=off)
    for f, fr in enumerate(frames):
        _same(r.last_temporal_linear[f], fr["color"], (f, "denoise: last_temporal_linear"))
        want_lin, _ = rtgo.denoise_host(fr["color"], fr["normal"], fr["depth"], fr["albedo"], fr["object"])
        _same(r.last_denoised_linear[f], want_lin, (f, "last_denoised_linear"))
    r.close()


def _ppm(path):
    toks = open(path).read().split()
    w, h = int(toks[1]), int(toks[2])
    assert toks[0] == "P3" and toks[3] == "255"
    return np.array(toks[4:], np.int64).reshape(h, w, 3)


def test_cli_move_writes_the_python_result_and_refuses_bad_combinations(tmp_path):
    n, spp, deg = 3, 2, 6.0
    text = scene_json("S_CUBE")
    scene_file = tmp_path / "s_cube.json"
    scene_file.write_text(text)
    out = tmp_path / "o.ppm"
    base = [EXE, str(scene_file), str(out), str(W), str(H), "--samples", str(spp), "--seed", str(SEED), "--camera", "lookat"]
    orbit = ["--orbit", f"{n},{deg}"]
    move = ["--move", "1:0.25,0.06,0"]
    scene = rtgo.Scene.from_json_text(text)
    cams = rtgo.camera_orbit(scene, n, deg)
    r = _renderer(spp)
    r.set_camera("lookat")
    want = r.render_sequence(scene, W, H, cams, temporal=True, offsets=_offsets(n))
    p = subprocess.run(base + orbit + move + ["--temporal", "default"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    for f in range(n):
        assert np.array_equal(_ppm(tmp_path / f"o_{f:04d}.ppm"), want[f][..., :3].astype(np.int64)), f
    # two objects, --denoise-variance, and no --temporal at all (the plain renders of the moved scenes)
    off2 = _offsets(n)
    for f in range(n):
        off2[f, 3] = [f * v for v in (-0.125, 0.0, 0.5)]
    want = r.render_sequence(scene, W, H, cams, temporal=True, variance=True, offsets=off2)
    p = subprocess.run(base + orbit + move + ["--move", "3:-0.125,0,0.5", "--temporal", "default", "--denoise-variance",
                                              "default"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    for f in range(n):
        assert np.array_equal(_ppm(tmp_path / f"o_{f:04d}.ppm"), want[f][..., :3].astype(np.int64)), f
    want = r.render_sequence(scene, W, H, cams, offsets=_offsets(n))
    p = subprocess.run(base + orbit + move, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    for f in range(n):
        assert np.array_equal(_ppm(tmp_path / f"o_{f:04d}.ppm"), want[f][..., :3].astype(np.int64)), f
    r.close()
    for f in tmp_path.glob("o_*.ppm"):
        f.unlink()
    tp = ["--temporal", "default"]
    refused = {
        "without --orbit": base + move,
        "an object outside the scene": base + orbit + tp + ["--move", "4:0.1,0,0"],
        "a negative object": base + orbit + tp + ["--move", "-1:0.1,0,0"],
        "no colon": base + orbit + tp + ["--move", "0.1,0,0"],
        "two fields": base + orbit + tp + ["--move", "1:0.1,0"],
        "four fields": base + orbit + tp + ["--move", "1:0.1,0,0,0"],
        "an empty field": base + orbit + tp + ["--move", "1:0.1,,0"],
        "a malformed field": base + orbit + tp + ["--move", "1:0.1,abc,0"],
        "a field that is not finite": base + orbit + tp + ["--move", "1:0.1,inf,0"],
        "a malformed object": base + orbit + tp + ["--move", "x:0.1,0,0"],
        "an object given twice": base + orbit + tp + move + ["--move", "1:0,0,0.5"],
        "no SPEC": base + orbit + tp + ["--move"],
    }
    for what, cmd in refused.items():
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0, what
        assert "--move" in p.stderr, (what, p.stderr)
        assert not list(tmp_path.glob("o*.ppm")), what
