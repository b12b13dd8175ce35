"""GPU: the à-trous denoiser (rt_denoise_async).

The kernels are held, bit for bit, to rt_denoise_host and to the numpy
restatement of the definition (tests/denoise_reference.py) on the cases of the
CPU tests: a partial wave and a partial block of rows (33x17), one pixel, two
waves per row with steps that reach past the image (70x5, levels 8), every
mechanism off in turn, in place, and each output alone.  One real chain feeds
the filter a GPU render and the GPU feature buffers.  The rest pins what the
call promises around the image: a refused call touches nothing, the workspace
is never overrun, and the Python layer and the CLI hand out the same bytes.
Every case is at most 72x48 pixels; the references are computed once
(denoise_reference.case_reference caches) and shared."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import rtgo
from conftest import ROOT
from denoise_reference import CASES, bits, case_inputs, case_reference
from scene_cases import make_settings
from sequence_cases import scene_json

pytestmark = pytest.mark.gpu

RT_E_INVALID = -1
W, H, SPP, SEED = 72, 48, 4, 3
S_CUBE = scene_json("S_CUBE")
NAMES = ("color", "normal", "depth", "albedo", "object")
SENT_F, SENT_B, GUARD = -1234.5, 0xA5, 256
EXE = os.path.join(ROOT, "concurrent-raytracer-go_amd", "build", "raytracer")


class _Dev:
    """Device copies of a case's inputs, sentinel-filled outputs, and a sentinel-filled workspace
    with GUARD bytes behind it that no call may touch."""

    def __init__(self, inp, w, h):
        import torch

        self.torch, self.w, self.h = torch, w, h
        self.inp = {k: (torch.from_numpy(np.array(inp[k])).cuda() if inp[k] is not None else None) for k in NAMES}
        self.nbytes = rtgo.denoise_workspace_bytes(w, h)
        assert 0 < self.nbytes <= 64 * w * h + 256
        self.fill()

    def fill(self):
        t = self.torch
        self.lin = t.full((self.h, self.w, 3), SENT_F, dtype=t.float32, device="cuda")
        self.rgba = t.full((self.h, self.w, 4), SENT_B, dtype=t.uint8, device="cuda")
        self.work = t.full((self.nbytes + GUARD,), SENT_B, dtype=t.uint8, device="cuda")

    def ptr(self, k):
        return self.inp[k].data_ptr() if self.inp[k] is not None else None

    def run(self, params, lin=True, rgba=True, in_place=False):
        out_lin = self.ptr("color") if in_place else (self.lin.data_ptr() if lin else None)
        rtgo.denoise_async(self.w, self.h, self.ptr("color"), self.ptr("normal"), self.ptr("depth"), self.ptr("albedo"),
                           self.ptr("object"), out_lin, self.rgba.data_ptr() if rgba else None, self.work.data_ptr(),
                           self.nbytes, params, 0)
        self.torch.cuda.synchronize()
        assert (self.work[self.nbytes:] == SENT_B).all()  # (nothing behind the workspace was written)
        return (self.inp["color"] if in_place else self.lin).cpu().numpy(), self.rgba.cpu().numpy()

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool((self.lin == SENT_F).all() and (self.rgba == SENT_B).all() and (self.work == SENT_B).all())


def _host(inp, params):
    return rtgo.denoise_host(inp["color"], inp["normal"], inp["depth"], inp["albedo"], inp["object"], params)


def _same(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert got.shape == want.shape and bad.size == 0, (what, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host_and_reference_bit_for_bit(name):
    inp, params = case_inputs(name)
    ref = case_reference(name)
    h, w = inp["depth"].shape
    host_lin, host_rgba = _host(inp, params)
    lin, rgba = _Dev(inp, w, h).run(params)
    _same(lin, ref, (name, "reference"))
    _same(lin, host_lin, (name, "host"))
    assert rgba.tobytes() == host_rgba.tobytes(), name
    if name == "33x17 levels 3":  # (the comparison is of a filter that did something)
        valid = np.isfinite(inp["depth"])
        assert (bits(ref) != bits(inp["color"])).any(axis=-1)[valid].mean() >= 0.9


def test_in_place_and_each_output_alone():
    name = "33x17 levels 3"
    inp, params = case_inputs(name)
    ref = case_reference(name)
    h, w = inp["depth"].shape
    want_rgba = _host(inp, params)[1]
    d = _Dev(inp, w, h)
    lin, rgba = d.run(params, rgba=False)
    _same(lin, ref, "only linear")
    assert (rgba == SENT_B).all()
    d.fill()
    lin, rgba = d.run(params, lin=False)
    assert rgba.tobytes() == want_rgba.tobytes() and (lin == SENT_F).all()
    d.fill()
    lin, rgba = d.run(params, in_place=True)  # (last: it overwrites the device copy of color)
    _same(lin, ref, "in place")
    assert rgba.tobytes() == want_rgba.tobytes() and (d.lin == SENT_F).all()


@functools.lru_cache(maxsize=None)
def _chain():
    """The real chain at 72x48x4 on S_CUBE, by hand: the GPU render's d_linear, the GPU feature buffers
    and rt_denoise_async with the defaults.  Returns the downloaded inputs and outputs."""
    import torch

    st = make_settings(rtgo, {"samples": SPP, "max_depth": 50}, SEED)
    ctx = rtgo.Context(0)
    ctx.set_scene(rtgo.Scene.from_json_text(S_CUBE))
    n = W * H
    lin = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    f = {k: torch.zeros(n * (3 if k in ("albedo", "normal") else 1),
                        dtype=torch.int32 if k == "object" else torch.float32, device="cuda")
         for k in ("albedo", "normal", "depth", "object")}
    ctx.render_async(W, H, st, lin.data_ptr(), 0, 0)
    ctx.render_aov_async(W, H, st, rtgo.AovBuffers(f["albedo"].data_ptr(), f["normal"].data_ptr(),
                                                  f["depth"].data_ptr(), None, f["object"].data_ptr()))
    nbytes = rtgo.denoise_workspace_bytes(W, H)
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    out_lin = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    out_rgba = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    rtgo.denoise_async(W, H, lin.data_ptr(), f["normal"].data_ptr(), f["depth"].data_ptr(), f["albedo"].data_ptr(),
                       f["object"].data_ptr(), out_lin.data_ptr(), out_rgba.data_ptr(), work.data_ptr(), nbytes)
    torch.cuda.synchronize()
    ctx.close()
    shape = lambda k: (H, W, 3) if k in ("albedo", "normal", "color") else (H, W)
    inp = {k: f[k].cpu().numpy().reshape(shape(k)) for k in f}
    inp["color"] = lin.cpu().numpy().reshape(H, W, 3)
    return inp, out_lin.cpu().numpy().reshape(H, W, 3), out_rgba.cpu().numpy().reshape(H, W, 4)


def test_real_chain_equals_the_host_filter_of_the_downloaded_inputs():
    inp, lin, rgba = _chain()
    valid = np.isfinite(inp["depth"])
    assert 300 < valid.sum() < W * H and len(np.unique(inp["object"][valid])) == 4 and inp["color"].any()
    host_lin, host_rgba = _host(inp, None)
    assert np.isfinite(host_lin).all()
    _same(lin, host_lin, "chain")
    assert rgba.tobytes() == host_rgba.tobytes()
    assert (bits(lin) != bits(inp["color"])).any(axis=-1)[valid].mean() > 0.9
    assert np.array_equal(bits(lin)[~valid], bits(inp["color"])[~valid])


def test_refused_calls_touch_nothing_and_a_short_workspace_is_refused():
    lib = rtgo.lib()
    inp, _ = case_inputs("33x17 levels 3")
    h, w = inp["depth"].shape
    d = _Dev(inp, w, h)
    D = rtgo.default_denoise

    def call(params=D(), w=w, h=h, inputs=True, lin=True, rgba=True, work=True, nbytes=d.nbytes, **drop):
        di = rtgo.DenoiseInputs(*[None if drop.get(k) else d.ptr(k) for k in NAMES])
        return lib.rt_denoise_async(ctypes.byref(params) if params is not None else None, w, h,
                                    ctypes.byref(di) if inputs else None, d.lin.data_ptr() if lin else None,
                                    d.rgba.data_ptr() if rgba else None, d.work.data_ptr() if work else None, nbytes, None)

    cases = {
        "NULL params": dict(params=None), "NULL inputs": dict(inputs=False), "NULL color": dict(color=True),
        "NULL normal": dict(normal=True), "NULL depth": dict(depth=True), "both outputs NULL": dict(lin=False, rgba=False),
        "width 0": dict(w=0), "height 65537": dict(h=65537), "too many pixels": dict(w=65536, h=65536),
        "NULL workspace": dict(work=False), "workspace one byte short": dict(nbytes=d.nbytes - 1),
        "workspace 0 bytes": dict(nbytes=0),
        "levels 0": dict(params=D(levels=0)), "levels 9": dict(params=D(levels=9)),
        "normal_power 24": dict(params=D(normal_power=24)), "sigma_color NaN": dict(params=D(sigma_color=float("nan"))),
        "sigma_depth inf": dict(params=D(sigma_depth=float("inf"))), "sigma_depth < 0": dict(params=D(sigma_depth=-1.0)),
        "demodulate 2": dict(params=D(demodulate=2)),
    }
    for what, kw in cases.items():
        assert call(**kw) == RT_E_INVALID, what
        assert lib.rt_last_error(), what
        assert d.untouched(), what
    assert call() == 0  # (the same call with nothing wrong)
    d.torch.cuda.synchronize()
    _same(d.lin.cpu().numpy(), reference_default(), "after the refused calls")


@functools.lru_cache(maxsize=None)
def reference_default():
    inp, _ = case_inputs("33x17 levels 3")
    return _host(inp, None)[0]


def _renderer():
    r = rtgo.ParallelRenderer(1)
    r.set_samples(SPP)
    r.set_seed(SEED)
    return r


def test_render_denoised_equals_the_chain():
    inp, lin, rgba = _chain()
    r = _renderer()
    img = r.render_denoised(rtgo.Scene.from_json_text(S_CUBE), W, H)
    assert img.tobytes() == rgba.tobytes()
    _same(r.last_denoised_linear, lin, "last_denoised_linear")
    _same(r.last_linear, inp["color"], "last_linear stays the raw render")
    # other parameters reach the filter
    img2 = r.render_denoised(rtgo.Scene.from_json_text(S_CUBE), W, H, params={"levels": 2, "sigma_color": 0.25})
    want = _host(inp, {"levels": 2, "sigma_color": 0.25})
    _same(r.last_denoised_linear, want[0], "levels 2")
    assert img2.tobytes() == want[1].tobytes() and img2.tobytes() != img.tobytes()
    r.close()


def test_progressive_denoise_leaves_the_raw_progression_as_it_was():
    scene = rtgo.Scene.from_json_text(S_CUBE)
    runs = {}
    for dn in (None, {"levels": 3}):
        r = rtgo.ParallelRenderer(1)
        r.set_samples(5)  # (passes of 2, 2 and 1 samples)
        r.set_seed(SEED)
        seen = []
        img = r.render_progressive(scene, W, H, 2, on_pass=lambda n, im, ch: seen.append((n, ch, im.copy())),
                                   denoise=dn)
        runs[dn is not None] = (r, seen, img)
    (r0, seen0, img0), (r1, seen1, img1) = runs[False], runs[True]
    assert [(n, ch) for n, ch, _ in seen0] == [(n, ch) for n, ch, _ in seen1] == [(2, None), (4, seen0[1][1]), (5, seen0[2][1])]
    assert seen0[1][1] > 0  # (the raw stop criterion was really read)
    assert r1.last_linear.tobytes() == r0.last_linear.tobytes()
    assert r1.last_sample_counts.tobytes() == r0.last_sample_counts.tobytes() and r1.last_samples == r0.last_samples == 5
    assert r0.last_denoised_linear is None
    # the denoised last image: the host filter of the last raw image with the features of min(cap, pass) samples
    ra = rtgo.ParallelRenderer(1)
    ra.set_samples(2)
    ra.set_seed(SEED)
    f = ra.render_aov(scene, W, H)
    want_lin, want_rgba = rtgo.denoise_host(r0.last_linear, f["normal"], f["depth"], f["albedo"], f["object"],
                                            {"levels": 3})
    _same(r1.last_denoised_linear, want_lin, "last_denoised_linear")
    assert img1.tobytes() == want_rgba.tobytes() == seen1[-1][2].tobytes()
    assert img1.tobytes() != img0.tobytes() and seen1[0][2].tobytes() != seen0[0][2].tobytes()
    # an until_changed_pixels stop falls at the same pass with and without the filter
    stops = []
    for dn in (None, True):
        r = rtgo.ParallelRenderer(1)
        r.set_samples(5)
        r.set_seed(SEED)
        r.render_progressive(scene, W, H, 2, until_changed_pixels=W * H, denoise=dn)
        stops.append(r.last_samples)
        r.close()
    assert stops == [4, 4]
    for r in (r0, r1, ra):
        r.close()


def _ppm(path):
    toks = open(path).read().split()
    w, h = int(toks[1]), int(toks[2])
    assert toks[0] == "P3" and toks[3] == "255"
    return np.array(toks[4:], np.int64).reshape(h, w, 3)


def test_cli_denoise_writes_the_python_result_and_refuses_bad_combinations(tmp_path):
    _, _, rgba = _chain()
    scene = tmp_path / "s_cube.json"
    scene.write_text(S_CUBE)
    out = tmp_path / "o.ppm"
    base = [EXE, str(scene), str(out), str(W), str(H), "--samples", str(SPP), "--seed", str(SEED)]
    p = subprocess.run(base + ["--denoise", "default", "--aov", str(tmp_path / "f")], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert np.array_equal(_ppm(out), rgba[..., :3].astype(np.int64))
    assert (tmp_path / "f.depth.ppm").exists()  # (it combines with --aov)
    # a SPEC with fields, against the Python layer
    r = _renderer()
    want = r.render_denoised(rtgo.Scene.from_json_text(S_CUBE), W, H,
                             params={"levels": 2, "sigma_color": 0.25, "sigma_depth": 0.1, "normal_power": 8})
    p = subprocess.run(base + ["--denoise", "2,0.25,0.1,8"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert np.array_equal(_ppm(out), want[..., :3].astype(np.int64))
    # the last image of a progression
    want = r.render_progressive(rtgo.Scene.from_json_text(S_CUBE), W, H, 2, denoise=True)
    p = subprocess.run(base + ["--pass-samples", "2", "--denoise", "default"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert np.array_equal(_ppm(out), want[..., :3].astype(np.int64))
    r.close()
    out.unlink()
    refused = {
        "--orbit": base + ["--denoise", "default", "--orbit", "2"],
        "--samples 0": base[:5] + ["--samples", "0", "--denoise", "default"],
        "no pixels": [EXE, str(scene), str(out), "0", "8", "--denoise", "default"],
        "levels 9": base + ["--denoise", "9"],
        "a power that is no power of two": base + ["--denoise", "4,0.5,0.05,24"],
        "a fifth field": base + ["--denoise", "4,0.5,0.05,32,1"],
        "no SPEC": base + ["--denoise"],
    }
    for what, cmd in refused.items():
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0, what
        assert "--denoise" in p.stderr, (what, p.stderr)
        assert not out.exists(), what
