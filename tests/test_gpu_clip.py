"""GPU: temporal accumulation with history rectification
(rt_temporal_clip_async).

Both kernel forms (plain and staged, chosen by RTGO_CLIP_FORM) are held, bit for
bit, to rt_temporal_clip_host and to the numpy restatement
(tests/clip_reference.py) at the sizes at which a 64x4 tile or a window can go
wrong: one pixel, an image smaller than the window (5x3, radius 3), exactly one
tile, one pixel more than a tile each way, three tiles across and three down
with both cut (130x9), and 72x48; each with and without moments, albedo, ids,
the table, out_clipped and a previous frame.  With radius 0 the call is held to
rt_temporal_motion_async / rt_temporal_async on the device.  A refused call
touches nothing.  One real chain renders C_FLOOR over three frames by hand from
the public calls; the device result equals the host function of the downloaded
inputs, and render_sequence(clip=...) and the CLI's --clip hand out the same
bytes.  Every case is at most 130x9 or 72x48 pixels; the references are
computed once and shared."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import rtgo
from clip_cases import CAMERA, FLOOR_MOVE, LIGHT_MOVE, frame_json
from clip_reference import SIZES, TABLE, VARIANTS, bits, clip_of, syn_inputs, syn_reference
from conftest import ROOT
from scene_cases import make_settings

pytestmark = pytest.mark.gpu

RT_E_INVALID = -1
W, H, SEED = 72, 48, 3
NAMES = ("color", "depth", "object", "normal", "count")
SENT_F, SENT_B, GUARD = -1234.5, 0xA5, 64
EXE = os.path.join(ROOT, "concurrent-raytracer-go_amd", "build", "raytracer")
FORMS = ["plain", "staged"]


@pytest.fixture
def form(request, monkeypatch):
    """The kernel form of the test's launches (the library reads RTGO_CLIP_FORM at every launch)."""
    monkeypatch.setenv("RTGO_CLIP_FORM", request.param)
    return request.param


class _Dev:
    """Device copies of a case's frames, the table and sentinel-filled outputs, each output with GUARD
    elements behind it that no call may touch."""

    def __init__(self, cur, prev, w, h, table):
        import torch

        self.torch, self.w, self.h = torch, w, h
        up = lambda d: {k: torch.from_numpy(np.array(d[k])).cuda() for k in NAMES + ("albedo", "moments")
                        if d.get(k) is not None}
        self.cur, self.prev = up(cur), (up(prev) if prev is not None else None)
        ptr = lambda t, k: t[k].data_ptr() if k in t else None
        self.fc = rtgo.temporal_frame(cur["frame"], *[ptr(self.cur, k) for k in NAMES])
        self.fp = rtgo.temporal_frame(prev["frame"], *[ptr(self.prev, k) for k in NAMES]) if prev is not None else None
        self.table = torch.from_numpy(np.array(table, np.float64)).cuda() if table is not None else None
        self.albedo = ptr(self.cur, "albedo")
        self.pmom = ptr(self.prev, "moments") if prev is not None else None
        self.fill()

    def fill(self):
        t, n = self.torch, self.w * self.h
        self.color = t.full((n * 3 + GUARD,), SENT_F, dtype=t.float32, device="cuda")
        self.count = t.full((n + GUARD,), SENT_F, dtype=t.float32, device="cuda")
        self.mom = t.full((n * 2 + GUARD,), SENT_F, dtype=t.float32, device="cuda")
        self.clp = t.full((n + GUARD,), SENT_F, dtype=t.float32, device="cuda")
        self.rgba = t.full((n * 4 + GUARD,), SENT_B, dtype=t.uint8, device="cuda")

    def download(self):
        n = self.w * self.h
        self.torch.cuda.synchronize()
        # (nothing behind an output was written)
        assert (self.color[n * 3:] == SENT_F).all() and (self.count[n:] == SENT_F).all()
        assert (self.mom[n * 2:] == SENT_F).all() and (self.rgba[n * 4:] == SENT_B).all()
        assert (self.clp[n:] == SENT_F).all()
        return dict(color=self.color[:n * 3].cpu().numpy().reshape(self.h, self.w, 3),
                    count=self.count[:n].cpu().numpy().reshape(self.h, self.w),
                    moments=self.mom[:n * 2].cpu().numpy().reshape(self.h, self.w, 2),
                    clipped=self.clp[:n].cpu().numpy().reshape(self.h, self.w),
                    rgba=self.rgba[:n * 4].cpu().numpy().reshape(self.h, self.w, 4))

    def run(self, clip, moments, clipped=True, params=None):
        rtgo.temporal_clip_async(self.w, self.h, self.fc, self.fp, self.color.data_ptr(), self.count.data_ptr(),
                                 self.rgba.data_ptr(), params, 0, clip=clip,
                                 d_motion=self.table.data_ptr() if self.table is not None else None,
                                 num_objects=self.table.shape[0] if self.table is not None else 0,
                                 d_cur_albedo=self.albedo, d_prev_moments=self.pmom if moments else None,
                                 d_out_moments=self.mom.data_ptr() if moments else None,
                                 d_out_clipped=self.clp.data_ptr() if clipped else None)
        return self.download()

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.color == SENT_F).all() and (self.count == SENT_F).all() and (self.mom == SENT_F).all()
                    and (self.clp == SENT_F).all() and (self.rgba == SENT_B).all())


def _same(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert got.shape == want.shape and got.dtype == want.dtype and bad.size == 0, (what, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_host_and_reference_bit_for_bit(size, variant, form):
    w, h = size
    v = VARIANTS[variant]
    cur, prev, table = syn_inputs(w, h, variant)
    ref = syn_reference(w, h, variant)
    host = rtgo.temporal_clip_host(cur, prev, table, moments=v["moments"], clip=clip_of(w, h))
    d = _Dev(cur, prev, w, h, table)
    got = d.run(clip_of(w, h), v["moments"], v["clipped"])
    what = (size, variant, form)
    _same(got["color"], ref["color"], what + ("color, reference",))
    _same(got["count"], ref["count"], what + ("count, reference",))
    _same(got["color"], host[0], what + ("color, host",))
    _same(got["count"], host[1], what + ("count, host",))
    assert got["rgba"].tobytes() == host[-1].tobytes(), what
    if v["moments"]:
        _same(got["moments"], ref["moments"], what + ("moments, reference",))
        _same(got["moments"], host[2], what + ("moments, host",))
    else:
        assert (got["moments"] == SENT_F).all()
    if v["clipped"]:
        _same(got["clipped"], ref["clipped"], what + ("clipped, reference",))
        _same(got["clipped"], host[-2], what + ("clipped, host",))
    else:
        assert (got["clipped"] == SENT_F).all()
    if size == (72, 48) and v["prev"]:  # (the comparison is of a clip that did something, and left something alone)
        assert ref["clipped"].sum() > 100 and (ref["has"] & (ref["channels"] == 0)).sum() > 30


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("size", [(65, 5), (72, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_radius_0_is_the_existing_kernels_bit_for_bit(size, form):
    w, h = size
    off = rtgo.default_history_clip(radius=0)
    for variant, moments in (("all", True), ("colour", False)):
        cur, prev, table = syn_inputs(w, h, variant)
        if not moments:
            cur = {k: a for k, a in cur.items() if k != "albedo"}
        d = _Dev(cur, prev, w, h, table)
        got = d.run(off, moments)
        assert (got["clipped"] == 0).all()
        d.fill()
        m = dict(d_cur_albedo=d.albedo, d_prev_moments=d.pmom, d_out_moments=d.mom.data_ptr()) if moments else {}
        rtgo.temporal_motion_async(w, h, d.fc, d.fp, d.table.data_ptr(), 3, d.color.data_ptr(), d.count.data_ptr(),
                                   d.rgba.data_ptr(), None, 0, **m)
        want = d.download()
        for k in ("color", "count", "moments", "rgba"):
            _same(got[k], want[k], (size, variant, k))
    # without a table: rt_temporal_async, with and without ids
    for variant in ("no ids", "moments, no table"):
        cur, prev, _ = syn_inputs(w, h, variant)
        cur = {k: a for k, a in cur.items() if k != "albedo"}
        d = _Dev(cur, prev, w, h, None)
        got = d.run(off, False)
        d.fill()
        rtgo.temporal_async(w, h, d.fc, d.fp, d.color.data_ptr(), d.count.data_ptr(), d.rgba.data_ptr(), None, 0)
        want = d.download()
        for k in ("color", "count", "rgba"):
            _same(got[k], want[k], (size, variant, k))


def test_refused_calls_enqueue_nothing_and_the_same_call_then_succeeds():
    lib = rtgo.lib()
    w, h = 65, 5
    cur, prev, table = syn_inputs(w, h, "all")
    d = _Dev(cur, prev, w, h, table)
    T, K = rtgo.default_temporal, rtgo.default_history_clip
    nan, inf = float("nan"), float("inf")

    def call(params=T(), clip=K(**clip_of(w, h)), w=w, h=h, prev_on=True, motion_on=True, rows=3, table_on=True,
             pmom=True, moments=True, clipped="own", edit=None):
        fc, fp = rtgo.TemporalFrame.from_buffer_copy(d.fc), rtgo.TemporalFrame.from_buffer_copy(d.fp)
        if edit:
            edit(fc, fp)
        m = rtgo.Motion(d.table.data_ptr() if table_on else None, rows, 0)
        out_clipped = {"own": d.clp.data_ptr(), "color": d.color.data_ptr(), "count": d.count.data_ptr(),
                       "moments": d.mom.data_ptr(), None: None}[clipped]
        return lib.rt_temporal_clip_async(
            ctypes.byref(params) if params is not None else None, w, h, ctypes.byref(fc),
            ctypes.byref(fp) if prev_on else None, ctypes.byref(m) if motion_on else None,
            ctypes.byref(clip) if clip is not None else None, d.albedo, d.pmom if pmom else None, d.color.data_ptr(),
            d.count.data_ptr(), d.mom.data_ptr() if moments else None, out_clipped, d.rgba.data_ptr(), None)

    def setf(which, name, value):
        def edit(fc, fp):
            setattr(fc if which == "cur" else fp, name, value)
        return edit

    cases = {
        "NULL clip": dict(clip=None), "radius -1": dict(clip=K(radius=-1)), "radius 5": dict(clip=K(radius=5)),
        "min_taps 0": dict(clip=K(min_taps=0)), "gamma < 0": dict(clip=K(gamma=-0.5)), "gamma NaN": dict(clip=K(gamma=nan)),
        "gamma inf": dict(clip=K(gamma=inf)), "min_half < 0": dict(clip=K(min_half=-1.0)),
        "min_half NaN": dict(clip=K(min_half=nan)),
        "out_clipped == out_color": dict(clipped="color"), "out_clipped == out_count": dict(clipped="count"),
        "out_clipped == out_moments": dict(clipped="moments"),
        "NULL table": dict(table_on=False), "num_objects 0": dict(rows=0),
        "a table without cur.object": dict(edit=setf("cur", "object", None)),
        "object in cur only, no table": dict(motion_on=False, edit=setf("prev", "object", None)),
        "prev_moments without out_moments": dict(moments=False),
        "prev without prev_moments": dict(pmom=False), "prev_moments without prev": dict(prev_on=False),
        "NULL params": dict(params=None), "NULL cur.depth": dict(edit=setf("cur", "depth", None)),
        "NULL prev.count": dict(edit=setf("prev", "count", None)),
        "out_color == prev.color": dict(edit=setf("prev", "color", d.color.data_ptr())),
        "w = 0": dict(w=0), "too many pixels": dict(w=65536, h=65536), "max_history 0": dict(params=T(max_history=0.0)),
    }
    for what, kw in cases.items():
        assert call(**kw) == RT_E_INVALID, what
        assert b"rt_temporal_clip_async" in lib.rt_last_error(), what
        assert d.untouched(), what
    assert call() == 0  # (the same call with nothing wrong)
    got = d.download()
    ref = syn_reference(w, h, "all")
    for k in ("color", "count", "moments", "clipped"):
        _same(got[k], ref[k], ("after the refused calls", k))


# ---- a real chain: C_FLOOR at 72x48, the sphere moving over the floor, three frames
def _settings(spp, seed):
    return make_settings(rtgo, {"samples": spp, "max_depth": 50}, seed)


def _offsets(n):
    off = np.zeros((n, 2, 3), np.float64)
    for f in range(n):
        off[f, 1] = [f * v for v in FLOOR_MOVE]
    return off


@functools.lru_cache(maxsize=None)
def _chain(spp, n, moments=False):
    """The chain by hand from the public calls: per frame rt_context_set_scene of the moved scene, a one-camera
    render (seed SEED + f), render_aov_async, and rt_temporal_clip_async with the defaults, the frame's albedo
    and scene_motion(frame f - 1's scene, frame f's) on the device; buffers ping-pong.  Returns, per frame, the
    downloaded inputs (raw colour and features), the table and the outputs."""
    import torch

    base = rtgo.Scene.from_json_text(frame_json("C_FLOOR", 0, CAMERA))
    off = _offsets(n)
    scenes = [base.translated(off[f]) for f in range(n)]
    ctx = rtgo.Context(0)
    npix = W * H
    lin = torch.zeros((n, npix * 3), dtype=torch.float32, device="cuda")
    feat = [{k: torch.zeros(npix * (3 if k in ("albedo", "normal") else 1),
                            dtype=torch.int32 if k == "object" else torch.float32, device="cuda")
             for k in ("albedo", "normal", "depth", "object")} for _ in range(2)]
    acc = [torch.zeros(npix * 3, dtype=torch.float32, device="cuda") for _ in range(2)]
    cnt = [torch.zeros(npix, dtype=torch.float32, device="cuda") for _ in range(2)]
    mom = [torch.zeros(npix * 2, dtype=torch.float32, device="cuda") for _ in range(2)]
    clp = torch.zeros(npix, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(npix * 4, dtype=torch.uint8, device="cuda")
    cam_frame = rtgo.camera_frame(CAMERA, "reference", W, H)
    prev, frames = None, []
    for f in range(n):
        ft = feat[f & 1]
        ctx.set_scene(scenes[f])
        ctx.render_cameras_async(W, H, _settings(spp, SEED), [CAMERA], [lin[f].data_ptr()], None, seeds=[SEED + f],
                                 stream=0)
        ctx.render_aov_async(W, H, _settings(spp, SEED + f),
                             rtgo.AovBuffers(ft["albedo"].data_ptr(), ft["normal"].data_ptr(), ft["depth"].data_ptr(),
                                             None, ft["object"].data_ptr()), camera=CAMERA)
        table = rtgo.scene_motion(scenes[f - 1], scenes[f]) if f else np.zeros((2, 3))
        d_table = torch.from_numpy(table).cuda()
        cur = rtgo.temporal_frame(cam_frame, lin[f].data_ptr(), ft["depth"].data_ptr(), ft["object"].data_ptr(),
                                  ft["normal"].data_ptr())
        rtgo.temporal_clip_async(W, H, cur, prev, acc[f & 1].data_ptr(), cnt[f & 1].data_ptr(),
                                 None if moments else rgba.data_ptr(), None, 0, clip=None, d_motion=d_table.data_ptr(),
                                 num_objects=2, d_cur_albedo=ft["albedo"].data_ptr(),
                                 d_prev_moments=mom[(f - 1) & 1].data_ptr() if moments and f else None,
                                 d_out_moments=mom[f & 1].data_ptr() if moments else None, d_out_clipped=clp.data_ptr())
        prev = rtgo.temporal_frame(cam_frame, acc[f & 1].data_ptr(), ft["depth"].data_ptr(), ft["object"].data_ptr(),
                                   ft["normal"].data_ptr(), cnt[f & 1].data_ptr())
        torch.cuda.synchronize()  # (download this frame before its buffers are reused)
        shape = lambda k: (H, W, 3) if k in ("albedo", "normal") else (H, W)
        frames.append(dict(
            {k: ft[k].cpu().numpy().reshape(shape(k)) for k in ft}, frame=cam_frame, table=table,
            raw=lin[f].cpu().numpy().reshape(H, W, 3), color=acc[f & 1].cpu().numpy().reshape(H, W, 3),
            count=cnt[f & 1].cpu().numpy().reshape(H, W), moments=mom[f & 1].cpu().numpy().reshape(H, W, 2),
            clipped=clp.cpu().numpy().reshape(H, W), rgba=rgba.cpu().numpy().reshape(H, W, 4)))
    ctx.close()
    return frames


@pytest.mark.parametrize("moments", [False, True], ids=["colour", "moments"])
def test_real_chain_equals_the_host_chain_bit_for_bit(moments):
    frames = _chain(1, 3, moments)
    state = None
    for f, fr in enumerate(frames):
        cur = dict(color=fr["raw"], depth=fr["depth"], object=fr["object"], normal=fr["normal"], albedo=fr["albedo"],
                   frame=fr["frame"])
        got = rtgo.temporal_clip_host(cur, state, fr["table"], moments=moments)
        _same(fr["color"], got[0], (f, "color"))
        _same(fr["count"], got[1], (f, "count"))
        _same(fr["clipped"], got[-2], (f, "clipped"))
        state = dict(cur, color=got[0], count=got[1])
        if moments:
            _same(fr["moments"], got[2], (f, "moments"))
            state["moments"] = got[2]
        else:
            assert fr["rgba"].tobytes() == got[-1].tobytes(), f
    # the clip did something on real frames, and left most histories alone
    last = frames[-1]
    kept = last["count"] > 1
    print(f"frame 2: {int(kept.sum())} pixels with a history, {int(last['clipped'].sum())} clipped")
    assert kept.sum() > 1000 and 0 < last["clipped"].sum() < kept.sum()
    assert not frames[0]["clipped"].any()


def _renderer(spp):
    r = rtgo.ParallelRenderer(1)
    r.set_samples(spp)
    r.set_seed(SEED)
    return r


def test_render_sequence_clip_is_the_manual_chain():
    n, spp = 3, 1
    scene = rtgo.Scene.from_json_text(frame_json("C_FLOOR", 0, CAMERA))
    cams = [CAMERA] * n
    r = _renderer(spp)
    frames = _chain(spp, n)
    img = r.render_sequence(scene, W, H, cams, temporal=True, offsets=_offsets(n), clip="default")
    for f, fr in enumerate(frames):
        _same(r.last_linear[f], fr["raw"], (f, "last_linear"))
        _same(r.last_temporal_linear[f], fr["color"], (f, "last_temporal_linear"))
        _same(r.last_history[f], fr["count"], (f, "last_history"))
        _same(r.last_clipped[f], fr["clipped"], (f, "last_clipped"))
        assert img[f].tobytes() == fr["rgba"].tobytes(), f
    # variance composes: the accumulation and moments fed back are the moments chain's
    mframes = _chain(spp, n, True)
    r.render_sequence(scene, W, H, cams, temporal=True, variance=True, offsets=_offsets(n), clip=True)
    for f, fr in enumerate(mframes):
        _same(r.last_temporal_linear[f], fr["color"], (f, "variance: last_temporal_linear"))
        want_var = rtgo.variance_host(fr["color"], fr["normal"], fr["depth"], fr["albedo"], fr["object"], fr["moments"],
                                      fr["count"])
        _same(r.last_variance[f], want_var, (f, "last_variance"))
    # clip=None changes nothing, and radius 0 is that pass too
    r.render_sequence(scene, W, H, cams, temporal=True, offsets=_offsets(n))
    plain_lin, plain_hist = r.last_temporal_linear.copy(), r.last_history.copy()
    assert r.last_clipped is None
    r.render_sequence(scene, W, H, cams, temporal=True, offsets=_offsets(n), clip=dict(radius=0))
    _same(r.last_temporal_linear, plain_lin, "radius 0")
    _same(r.last_history, plain_hist, "radius 0")
    assert (bits(plain_lin) != bits(np.stack([fr["color"] for fr in frames]))).any()
    # without offsets (no table), and a moving light: each frame's render is that of the relit scene
    r.render_sequence(scene, W, H, cams, temporal=True, clip=True)
    assert r.last_clipped.shape == (n, H, W)
    loff = np.zeros((n, 1, 3))
    for f in range(n):
        loff[f, 0] = [f * v for v in LIGHT_MOVE]
    r.render_sequence(scene, W, H, cams, temporal=True, clip=True, light_offsets=loff)
    relit = r.last_linear.copy()
    light_scene = rtgo.Scene.from_json_text(frame_json("C_LIGHT", 2, CAMERA))
    r2 = _renderer(spp)
    r2.set_seed(SEED + 2)
    r2.render(light_scene, W, H)
    _same(relit[2], np.asarray(r2.last_linear, np.float32).reshape(H, W, 3), "frame 2 of the moving light")
    assert r.last_clipped[2].sum() > 0
    r.close()
    r2.close()


def _ppm(path):
    toks = open(path).read().split()
    w, h = int(toks[1]), int(toks[2])
    assert toks[0] == "P3" and toks[3] == "255"
    return np.array(toks[4:], np.int64).reshape(h, w, 3)


def test_cli_clip_writes_the_python_result_and_refuses_bad_combinations(tmp_path):
    n, spp, deg = 3, 2, 6.0
    text = frame_json("C_FLOOR", 0)
    scene_file = tmp_path / "c_floor.json"
    scene_file.write_text(text)
    out = tmp_path / "o.ppm"
    base = [EXE, str(scene_file), str(out), str(W), str(H), "--samples", str(spp), "--seed", str(SEED), "--camera", "lookat"]
    orbit = ["--orbit", f"{n},{deg}"]
    move = ["--move", "1:0.25,0,0"]
    tp = ["--temporal", "default"]
    scene = rtgo.Scene.from_json_text(text)
    cams = rtgo.camera_orbit(scene, n, deg)
    r = _renderer(spp)
    r.set_camera("lookat")
    runs = {
        "default, with --move": (move + ["--clip", "default"], dict(offsets=_offsets(n), clip=True)),
        "four fields, no --move": (["--clip", "3,2,4,0.01"], dict(clip=dict(radius=3, gamma=2.0, min_taps=4, min_half=0.01))),
        "radius alone, --denoise-variance": (["--clip", "1", "--denoise-variance", "default"],
                                             dict(clip=dict(radius=1), variance=True)),
    }
    for what, (args, kw) in runs.items():
        want = r.render_sequence(scene, W, H, cams, temporal=True, **kw)
        p = subprocess.run(base + orbit + tp + args, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (what, p.stdout + p.stderr)
        for f in range(n):
            assert np.array_equal(_ppm(tmp_path / f"o_{f:04d}.ppm"), want[f][..., :3].astype(np.int64)), (what, f)
    r.close()
    for f in tmp_path.glob("o_*.ppm"):
        f.unlink()
    refused = {
        "without --temporal": base + orbit + ["--clip", "default"],
        "without --orbit": base + ["--clip", "default"],
        "radius 5": base + orbit + tp + ["--clip", "5"],
        "a negative gamma": base + orbit + tp + ["--clip", "2,-1"],
        "five fields": base + orbit + tp + ["--clip", "2,1.5,5,0,1"],
        "an empty field": base + orbit + tp + ["--clip", "2,,5"],
        "a malformed field": base + orbit + tp + ["--clip", "2,abc"],
        "a gamma that is not finite": base + orbit + tp + ["--clip", "2,nan"],
        "no SPEC": base + orbit + tp + ["--clip"],
    }
    for what, cmd in refused.items():
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0, what
        assert "--clip" in p.stderr, (what, p.stderr)
        assert not list(tmp_path.glob("o*.ppm")), what
