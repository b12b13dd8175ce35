"""GPU: matte layers and the edge resolve (rt_context_render_matte_async,
rt_matte_resolve_async).

The matte kernel is held, bit for bit, to the definition restated from the
oracle's parts (tests/matte_reference.py): one pixel, exactly one wave, one
wave and a lane, a partial wave, several blocks; fewer samples than slots and
more; a pixel whose samples overflow the sixteen slots; the linear scan, the
tree of a sphere field and the mixed tree, forced on and off; both levels (the
face ordinals of a cube); each output left out in turn; both camera models and a
camera argument; guard elements behind every output.  The call changes no later
render and no statistic.  The resolve kernel is held to the host twin and the
numpy restatement at every radius, with and without rest and out_rgba, at sizes
that leave partial blocks (finite colours here: the sign of a NaN that an
invalid operation makes is the processor's, and the CPU tests cover NaN and
Inf).  One real chain runs on the device from the public calls and equals the
host twin of its downloaded inputs; the Python layer and the CLI hand out the
same bytes.  Every case is at most 130x9 or 72x48; the references are computed
once and shared."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import rtgo
from clip_cases import CAMERA, frame_json
from conftest import ROOT
from matte_reference import bits, overflow_scene, parts_of, reference, resolve, syn_inputs
from mixed_cases import field70, spheres70
from scene_cases import make_settings
from sequence_cases import GENERAL, scene_json

pytestmark = pytest.mark.gpu

REF, LOOKAT = rtgo.RT_CAMERA_REFERENCE, rtgo.RT_CAMERA_LOOKAT
RT_E_INVALID = -1
W, H, SEED = 72, 48, 3
S_CUBE = scene_json("S_CUBE")
C_FLOOR = frame_json("C_FLOOR", 0, CAMERA)
GENERAL_TEXT = json.dumps(GENERAL)
EXE = os.path.join(ROOT, "concurrent-raytracer-go_amd", "build", "raytracer")
NAMES = ("id", "count", "rest")
GUARD, SENTINEL = 64, -77


@functools.lru_cache(maxsize=None)
def _text(name):
    return {"S_CUBE": S_CUBE, "C_FLOOR": C_FLOOR, "overflow": overflow_scene(),
            "spheres70": json.dumps(spheres70()), "field70": json.dumps(field70())}[name]


def _settings(samples, seed=SEED, camera=REF, **over):
    st = make_settings(rtgo, dict({"samples": samples, "max_depth": 50}, **over), seed)
    st.camera = camera
    return st


class _Matte:
    """One rt_context holding a scene, and sentinel-filled matte buffers with GUARD elements behind each."""

    def __init__(self, scene_text, w, h, ranks, force_bvh=0, set_scene=True):
        self.w, self.h, self.k = w, h, ranks
        self.ctx = rtgo.Context(0)
        if set_scene:
            self.ctx.set_scene(rtgo.Scene.from_json_text(scene_text), force_bvh=force_bvh)
        self.fill()

    def size(self, name):
        return (1 if name == "rest" else self.k) * self.w * self.h

    def fill(self):
        import torch

        self.buf = {n: torch.full((self.size(n) + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for n in NAMES}

    def pointers(self, names=NAMES):
        return rtgo.MatteBuffers(*[self.buf[n].data_ptr() if n in names else None for n in NAMES])

    def arrays(self):
        import torch

        torch.cuda.synchronize()
        out = {}
        for n in NAMES:
            a = self.buf[n].cpu().numpy()
            assert (a[self.size(n):] == SENTINEL).all(), ("the guard behind", n)
            out[n] = a[:self.size(n)].reshape((self.h, self.w) if n == "rest" else (self.k, self.h, self.w))
        return out

    def run(self, st, level="object", camera=None, names=NAMES):
        self.ctx.render_matte_async(self.w, self.h, st, self.pointers(names),
                                    params=rtgo.default_matte(ranks=self.k, level=level), camera=camera)
        return self.arrays()

    def untouched(self, names=NAMES):
        a = self.arrays()
        return all((a[n] == SENTINEL).all() for n in names)

    def close(self):
        self.ctx.close()


def _matte(scene_text, w, h, st, ranks=4, level="object", force_bvh=0, camera=None):
    m = _Matte(scene_text, w, h, ranks, force_bvh)
    out = m.run(st, level, camera)
    m.close()
    return out


def _same(got, want, what=""):
    for n in NAMES:
        assert got[n].dtype == want[n].dtype and got[n].shape == want[n].shape, (what, n)
        bad = np.argwhere(got[n] != want[n])
        assert bad.size == 0, (what, n, len(bad), bad[:4].tolist())


def _same_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


# ---- the matte kernel against the restatement
# (w, h, samples, ranks): one pixel; exactly one wave; a wave and one lane; a partial wave; 54 blocks.  Samples 1, 2
# and 17 (more samples than slots).
SIZES = [(1, 1, 17, 4), (64, 1, 2, 4), (65, 1, 1, 8), (5, 3, 17, 1), (72, 48, 17, 2)]


@pytest.mark.parametrize("level", ["object", "face"])
@pytest.mark.parametrize("w,h,n,ranks", SIZES, ids=lambda v: str(v))
def test_1_kernel_equals_the_restatement_at_every_size_and_level(w, h, n, ranks, level):
    ref = reference(S_CUBE, w, h, n, SEED, ranks, level)
    if (w, h) == (72, 48):
        assert (ref["hits"] > 0).sum() > 400 and ((ref["hits"] > 0) & (ref["hits"] < n)).sum() > 50
        if level == "face":  # three faces of the cube in a pixel, two ranks
            assert (ref["used"] > ranks).any() and (ref["rest"] > 0).any()
            assert len(np.unique(ref["id"][ref["id"] >= 48])) >= 4
    _same(_matte(S_CUBE, w, h, _settings(n), ranks, level, force_bvh=-1), ref, (w, h, n, ranks, level))


def test_2_ties_go_to_the_smaller_key_and_overflow_goes_to_rest():
    ref = reference(S_CUBE, W, H, 2, SEED, 2, "face", walk_samples=17)
    assert ref["tie"].any()
    _same(_matte(S_CUBE, W, H, _settings(2), 2, "face", force_bvh=-1), ref, "1 : 1 ties")
    for ranks in (4, 8):
        ref = reference(_text("overflow"), 2, 2, 64, SEED, ranks)
        assert (ref["overflow"] > 0).any() and (ref["used"] == 16).any() and ref["tie"].any()
        got = _matte(_text("overflow"), 2, 2, _settings(64), ranks)
        _same(got, ref, ("overflow", ranks))
        assert np.array_equal(got["count"].sum(axis=0) + got["rest"], ref["hits"])


@pytest.mark.parametrize("name", ["spheres70", "field70"])
def test_3_trees_find_the_linear_scans_hits(name):
    """More than 64 spheres: a tree by the automatic rule (spheres70: of spheres alone; field70: with leaves of cubes)."""
    w, h, n = 24, 16, 2
    for level in ("object", "face"):
        ref = reference(_text(name), w, h, n, SEED, 4, level)
        assert len(np.unique(ref["id"][0])) >= 8
        tree, scan = (_matte(_text(name), w, h, _settings(n), 4, level, force_bvh=f) for f in (0, -1))
        _same(tree, ref, (name, level, "tree"))
        _same(scan, ref, (name, level, "scan"))
    if name == "field70":
        assert (ref["id"][ref["id"] >= 0] % 16 > 0).any()  # (a cube's triangle other than its first)
    forced = _matte(S_CUBE, W, H, _settings(17), 2, "face", force_bvh=1)  # the mixed tree of a small scene
    _same(forced, reference(S_CUBE, W, H, 17, SEED, 2, "face"), "S_CUBE, a forced tree")


def test_4_both_camera_models_and_a_camera_argument():
    n = 3
    ref = reference(S_CUBE, W, H, n, SEED, 4, "face", GENERAL_TEXT, LOOKAT)
    assert (ref["hits"] > 0).sum() > 350 and (ref["used"] > 1).any()
    st = _settings(n, camera=LOOKAT)
    by_arg = _matte(S_CUBE, W, H, st, 4, "face", force_bvh=-1, camera=GENERAL)
    by_scene = _matte(scene_json("S_CUBE", GENERAL), W, H, st, 4, "face", force_bvh=-1)
    _same(by_arg, ref, "GENERAL as an argument")
    _same(by_scene, ref, "GENERAL as the scene's")
    # the reference model ignores lookAt: the frame of the scene's own camera
    moved = dict(json.loads(S_CUBE)["camera"], lookAt=[5.0, 5.0, 5.0])
    _same(_matte(S_CUBE, W, H, _settings(n), 4, "face", force_bvh=-1, camera=moved),
          reference(S_CUBE, W, H, n, SEED, 4, "face", walk_samples=17), "the reference model")


def test_5_each_output_left_out_in_turn_and_only_seed_size_and_samples_matter():
    ref = reference(S_CUBE, W, H, 17, SEED, 2, "face")
    for left_out in NAMES:
        m = _Matte(S_CUBE, W, H, 2, force_bvh=-1)
        names = tuple(n for n in NAMES if n != left_out)
        got = m.run(_settings(17), "face", names=names)
        for n in names:
            assert np.array_equal(got[n], ref[n]), (left_out, n)
        assert m.untouched((left_out,)), left_out
        m.close()
    for what, st in {"max_depth 0": _settings(17, max_depth=0), "hard shadows": _settings(17, soft_shadows=0),
                     "a sky": _settings(17, sky=1)}.items():
        _same(_matte(S_CUBE, W, H, st, 2, "face", force_bvh=-1), ref, what)
    other = _matte(S_CUBE, W, H, _settings(17, seed=SEED + 1), 2, "face", force_bvh=-1)
    assert (other["count"] != ref["count"]).any()


def test_6_no_side_effects_on_renders_and_statistics():
    import torch

    m = _Matte(S_CUBE, W, H, 4, force_bvh=-1)
    st = _settings(4)
    lin = torch.zeros((2, W * H * 3), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((2, W * H * 4), dtype=torch.uint8, device="cuda")
    m.ctx.render_async(W, H, st, lin[0].data_ptr(), rgba[0].data_ptr(), 0)
    s0 = m.ctx.stats()
    got = m.run(_settings(17))
    seconds = m.ctx.last_kernel_seconds()  # (its own events: the pass's device time)
    assert m.ctx.stats() == s0
    m.ctx.render_async(W, H, st, lin[1].data_ptr(), rgba[1].data_ptr(), 0)
    torch.cuda.synchronize()
    assert lin[0].cpu().numpy().tobytes() == lin[1].cpu().numpy().tobytes()
    assert rgba[0].cpu().numpy().tobytes() == rgba[1].cpu().numpy().tobytes() and rgba[0].any()
    _same(got, reference(S_CUBE, W, H, 17, SEED), "between two renders")
    assert 0 < seconds < 1
    # hits equals the first-hit pass's coverage * n
    cov = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    m.ctx.render_aov_async(W, H, _settings(17), rtgo.AovBuffers(None, None, None, cov.data_ptr(), None))
    torch.cuda.synchronize()
    hits = np.rint(cov.cpu().numpy().astype(np.float64).reshape(H, W) * 17).astype(np.int32)
    assert np.array_equal(got["count"].sum(axis=0) + got["rest"], hits)
    m.close()


def test_7_invalid_arguments_are_refused_and_touch_nothing():
    lib = rtgo.lib()
    m = _Matte(S_CUBE, W, H, 4, force_bvh=-1)
    st, out, none = _settings(4), m.pointers(), rtgo.MatteBuffers()
    M = rtgo.default_matte

    def call(ctx=m.ctx._h, w=W, h=H, st=st, cam=None, params=M(), out=out):
        return lib.rt_context_render_matte_async(ctx, w, h, ctypes.byref(st) if st is not None else None,
                                                 ctypes.byref(cam) if cam is not None else None,
                                                 ctypes.byref(params) if params is not None else None,
                                                 ctypes.byref(out) if out is not None else None, None)

    same_point = rtgo._as_camera({"position": [1, 1, 1], "lookAt": [1, 1, 1], "up": [0, 1, 0], "fov": 60})
    empty = _Matte(S_CUBE, W, H, 4, set_scene=False)
    cases = {
        "NULL ctx": dict(ctx=None), "NULL settings": dict(st=None), "NULL out": dict(out=None),
        "NULL params": dict(params=None), "all three NULL": dict(out=none),
        "no scene": dict(ctx=empty.ctx._h, out=empty.pointers()),
        "samples 0": dict(st=_settings(0)), "samples -1": dict(st=_settings(-1)),
        "width 0": dict(w=0), "height 65537": dict(h=65537), "samples past 2^24": dict(st=_settings((1 << 24) + 1)),
        "ranks 0": dict(params=M(ranks=0)), "ranks 9": dict(params=M(ranks=9)), "ranks -1": dict(params=M(ranks=-1)),
        "level 2": dict(params=M(level=2)), "level -1": dict(params=M(level=-1)),
        "an unknown camera model": dict(st=_settings(4, camera=7)),
        "a look-at camera without a direction": dict(st=_settings(4, camera=LOOKAT), cam=same_point),
    }
    for what, kw in cases.items():
        assert call(**kw) == RT_E_INVALID, what
        assert lib.rt_last_error(), what
        assert m.untouched() and empty.untouched(), what
    assert call() == 0  # (the same call with nothing wrong)
    _same(m.arrays(), reference(S_CUBE, W, H, 4, SEED, walk_samples=17), "after the refused calls")
    empty.close()
    m.close()


# ---- the resolve kernel = the host twin = the numpy restatement
def _device_resolve(color, obj, ids, count, rest, n, params=None, with_linear=True, with_rgba=True):
    """(linear or None, rgba or None) of rt_matte_resolve_async, with guard elements behind both outputs."""
    import torch

    h, w = obj.shape
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None
           for a in (color, obj, ids, count, rest)]
    lin = torch.full((w * h * 3 + GUARD,), -1234.5, dtype=torch.float32, device="cuda")
    rgba = torch.full((w * h * 4 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rtgo.matte_resolve_async(w, h, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                             dev[4].data_ptr() if rest is not None else None, count.shape[0], n,
                             lin.data_ptr() if with_linear else None, rgba.data_ptr() if with_rgba else None, params, 0)
    torch.cuda.synchronize()
    l, r = lin.cpu().numpy(), rgba.cpu().numpy()
    assert (l[w * h * 3:] == -1234.5).all() and (r[w * h * 4:] == 0xA5).all(), "the guards behind the outputs"
    if not with_linear:
        assert (l == -1234.5).all()
    if not with_rgba:
        assert (r == 0xA5).all()
    return (l[:w * h * 3].reshape(h, w, 3) if with_linear else None,
            r[:w * h * 4].reshape(h, w, 4) if with_rgba else None)


@pytest.mark.parametrize("with_rest", [True, False], ids=["rest", "no rest"])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (72, 48), (130, 9)], ids=lambda v: str(v))
def test_8_resolve_kernel_equals_host_and_numpy_bit_for_bit(w, h, with_rest):
    n, bg = 8, (0.25, 0.0, 1.5)
    radius = 4 if (w, h) == (5, 3) else 2
    color, obj, ids, count, rest = syn_inputs(w, h, special=False)
    rest = rest if with_rest else None
    params = dict(radius=radius, background=bg)
    want = resolve(color, obj, ids, count, rest, n, radius, bg)
    host, host_rgba = rtgo.matte_resolve_host(color, obj, ids, count, rest, n, params)
    _same_bits(host, want, "host = numpy")
    got, rgba = _device_resolve(color, obj, ids, count, rest, n, params)
    _same_bits(got, want, (w, h, with_rest))
    assert rgba.tobytes() == host_rgba.tobytes()
    mixed = parts_of(count, rest, n) >= 2
    _same_bits(got[~mixed], color[~mixed], "unmixed pixels keep their bits")
    if w * h > 1:
        assert mixed.any() and (bits(got[mixed]) != bits(color[mixed])).any()


def test_9_resolve_every_radius_single_outputs_and_refusals():
    w, h, n = 130, 9, 8
    color, obj, ids, count, rest = syn_inputs(w, h, special=False)
    for radius in (1, 2, 3, 4):
        want = resolve(color, obj, ids, count, rest, n, radius)
        got, _ = _device_resolve(color, obj, ids, count, rest, n, dict(radius=radius))
        _same_bits(got, want, radius)
    want = resolve(color, obj, ids, count, rest, n, 2)
    lin, none = _device_resolve(color, obj, ids, count, rest, n, with_rgba=False)
    _same_bits(lin, want, "out_linear alone")
    none, rgba = _device_resolve(color, obj, ids, count, rest, n, with_linear=False)
    assert rgba.tobytes() == rtgo.matte_resolve_host(color, obj, ids, count, rest, n)[1].tobytes()
    import torch

    d = [torch.from_numpy(a).cuda() for a in (color, obj, ids, count, rest)]
    out = torch.full((w * h * 3,), -1234.5, dtype=torch.float32, device="cuda")
    refused = {
        "radius 0": dict(params=dict(radius=0)), "radius 5": dict(params=dict(radius=5)),
        "a NaN background": dict(params=dict(background=(0, float("nan"), 0))),
        "ranks 9": dict(ranks=9), "samples 0": dict(samples=0), "out == color": dict(out=d[0].data_ptr()),
        "no output": dict(out=None), "width 0": dict(w=0),
    }
    for what, kw in refused.items():
        with pytest.raises(rtgo.RenderError, match="rt_matte_resolve_async"):
            rtgo.matte_resolve_async(kw.get("w", w), h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                     d[4].data_ptr(), kw.get("ranks", 3), kw.get("samples", n),
                                     kw.get("out", out.data_ptr()), None, kw.get("params"), 0)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == -1234.5).all(), what
        assert d[0].cpu().numpy().tobytes() == color.tobytes(), what


# ---- one real chain on the device, the Python layer and the CLI
MATTE_SPP, SPP = 16, 1


@functools.lru_cache(maxsize=None)
def _chain():
    """C_FLOOR at 72x48, 1 spp: render, first-hit pass, rt_denoise_async, matte pass and resolve from the public
    calls; everything downloaded."""
    import torch

    ctx = rtgo.Context(0)
    ctx.set_scene(rtgo.Scene.from_json_text(C_FLOOR))
    st, npix = _settings(SPP), W * H
    lin = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
    feat = {n: torch.zeros(npix * (3 if n in ("albedo", "normal") else 1),
                           dtype=torch.int32 if n == "object" else torch.float32, device="cuda")
            for n in ("albedo", "normal", "depth", "object")}
    nbytes = rtgo.denoise_workspace_bytes(W, H)
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    den = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
    ids, cnt = (torch.zeros(4 * npix, dtype=torch.int32, device="cuda") for _ in range(2))
    rest = torch.zeros(npix, dtype=torch.int32, device="cuda")
    out = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(npix * 4, dtype=torch.uint8, device="cuda")
    ctx.render_async(W, H, st, lin.data_ptr(), 0, 0)
    ctx.render_aov_async(W, H, st, rtgo.AovBuffers(feat["albedo"].data_ptr(), feat["normal"].data_ptr(),
                                                   feat["depth"].data_ptr(), None, feat["object"].data_ptr()))
    rtgo.denoise_async(W, H, lin.data_ptr(), feat["normal"].data_ptr(), feat["depth"].data_ptr(),
                       feat["albedo"].data_ptr(), feat["object"].data_ptr(), den.data_ptr(), None, work.data_ptr(), nbytes)
    ctx.render_matte_async(W, H, _settings(MATTE_SPP), rtgo.MatteBuffers(ids.data_ptr(), cnt.data_ptr(), rest.data_ptr()))
    rtgo.matte_resolve_async(W, H, den.data_ptr(), feat["object"].data_ptr(), ids.data_ptr(), cnt.data_ptr(),
                             rest.data_ptr(), 4, MATTE_SPP, out.data_ptr(), rgba.data_ptr())
    torch.cuda.synchronize()
    got = {"denoised": den.cpu().numpy().reshape(H, W, 3), "object": feat["object"].cpu().numpy().reshape(H, W),
           "id": ids.cpu().numpy().reshape(4, H, W), "count": cnt.cpu().numpy().reshape(4, H, W),
           "rest": rest.cpu().numpy().reshape(H, W), "out": out.cpu().numpy().reshape(H, W, 3),
           "rgba": rgba.cpu().numpy().reshape(H, W, 4)}
    ctx.close()
    return got


def test_10_a_real_chain_equals_the_host_twin_of_its_downloaded_inputs():
    c = _chain()
    _same({n: c[n] for n in NAMES}, reference(C_FLOOR, W, H, MATTE_SPP, SEED), "the chain's matte")
    host, host_rgba = rtgo.matte_resolve_host(c["denoised"], c["object"], c["id"], c["count"], c["rest"], MATTE_SPP)
    _same_bits(c["out"], host, "the chain's resolve")
    assert c["rgba"].tobytes() == host_rgba.tobytes()
    mixed = parts_of(c["count"], c["rest"], MATTE_SPP) >= 2
    two_objects = (c["count"][:2] > 0).all(axis=0)  # the sphere in front of the floor: two ranks, not a rank and a miss
    assert mixed.sum() > 40 and two_objects.sum() > 10
    assert (bits(c["out"][mixed]) != bits(c["denoised"][mixed])).any()
    _same_bits(c["out"][~mixed], c["denoised"][~mixed], "unmixed pixels")


def _ppm(path):
    toks = open(path).read().split()
    w, h = int(toks[1]), int(toks[2])
    assert toks[0] == "P3" and toks[3] == "255"
    return np.array(toks[4:], np.int64).reshape(h, w, 3)


def _renderer(samples=SPP, seed=SEED):
    r = rtgo.ParallelRenderer(1)
    r.set_samples(samples)
    r.set_seed(seed)
    return r


def test_11_render_denoised_and_the_cli_hand_out_the_chains_bytes(tmp_path):
    c = _chain()
    scene = rtgo.Scene.from_json_text(C_FLOOR)
    r = _renderer()
    plain = r.render_denoised(scene, W, H)
    assert r.last_resolved_linear is None
    img = r.render_denoised(scene, W, H, matte=True)
    _same_bits(r.last_denoised_linear, c["denoised"], "last_denoised_linear")
    _same_bits(r.last_resolved_linear, c["out"], "last_resolved_linear")
    assert img.tobytes() == c["rgba"].tobytes() and img.tobytes() != plain.tobytes()
    img8 = r.render_denoised(scene, W, H, matte=dict(samples=8, ranks=2, radius=3, background=(0.1, 0.2, 0.3)))
    m8 = reference(C_FLOOR, W, H, 8, SEED, 2, walk_samples=MATTE_SPP)
    host, host_rgba = rtgo.matte_resolve_host(c["denoised"], c["object"], m8["id"], m8["count"], m8["rest"], 8,
                                              dict(radius=3, background=(0.1, 0.2, 0.3)))
    _same_bits(r.last_resolved_linear, host, "a dict of options")
    assert img8.tobytes() == host_rgba.tobytes()
    # the specular guide looks through mirrors; the resolve still reads the first-hit ids
    r.render_denoised(scene, W, H, guide="specular", matte=True)
    spec_den = r.last_denoised_linear
    host, _ = rtgo.matte_resolve_host(spec_den, c["object"], c["id"], c["count"], c["rest"], MATTE_SPP)
    _same_bits(r.last_resolved_linear, host, "with the specular guide")
    r.close()
    scene_file, out = tmp_path / "c_floor.json", tmp_path / "o.ppm"
    scene_file.write_text(C_FLOOR)
    base = [EXE, str(scene_file), str(out), str(W), str(H), "--samples", str(SPP), "--seed", str(SEED)]
    p = subprocess.run(base + ["--denoise", "default", "--edge-resolve", "default"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert np.array_equal(_ppm(out), c["rgba"][..., :3].astype(np.int64))
    p = subprocess.run(base + ["--denoise", "default", "--edge-resolve", "8,3"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m8 = reference(C_FLOOR, W, H, 8, SEED, 4, walk_samples=MATTE_SPP)
    want = rtgo.matte_resolve_host(c["denoised"], c["object"], m8["id"], m8["count"], m8["rest"], 8, dict(radius=3))[1]
    assert np.array_equal(_ppm(out), want[..., :3].astype(np.int64))
    out.unlink()
    refused = {
        "with --orbit": base + ["--orbit", "2", "--edge-resolve", "default"],
        "radius 5": base + ["--edge-resolve", "16,5"], "samples 0": base + ["--edge-resolve", "0"],
        "a malformed field": base + ["--edge-resolve", "abc"], "no SPEC": base + ["--edge-resolve"],
        "--samples 0": base[:5] + ["--samples", "0", "--edge-resolve", "default"],
    }
    for what, cmd in refused.items():
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0, what
        assert "--edge-resolve" in p.stderr, (what, p.stderr)
        assert not list(tmp_path.glob("o*.ppm")), what


def test_12_render_matte_matte_mask_and_the_clis_matte_images(tmp_path):
    scene = rtgo.Scene.from_json_text(S_CUBE)
    r = _renderer()
    got = r.render_matte(scene, W, H, samples=17, ranks=2, level="face")
    ref = reference(S_CUBE, W, H, 17, SEED, 2, "face")
    _same(got, ref, "render_matte")
    assert got["coverage"].dtype == np.float32 and np.array_equal(
        got["coverage"], (ref["count"].astype(np.float64) / 17.0).astype(np.float32))
    obj = r.render_matte(scene, W, H)  # 16 samples, 4 ranks, object level
    _same(obj, reference(S_CUBE, W, H, 16, SEED, walk_samples=17), "the defaults")
    mask = rtgo.matte_mask(obj, 3)
    assert mask.shape == (H, W) and 0 < (mask > 0).sum() < W * H and ((mask > 0) & (mask < 1)).any()
    assert np.array_equal(mask > 0, (obj["id"] == 3).any(axis=0))
    r.set_camera("lookat")
    _same(r.render_matte(scene, W, H, samples=3, level="face", camera=GENERAL),
          reference(S_CUBE, W, H, 3, SEED, 4, "face", GENERAL_TEXT, LOOKAT), "a camera argument")
    r.close()
    scene_file, out = tmp_path / "s_cube.json", tmp_path / "o.ppm"
    scene_file.write_text(S_CUBE)
    prefix = tmp_path / "m"
    base = [EXE, str(scene_file), str(out), str(W), str(H), "--samples", "1", "--seed", str(SEED)]
    p = subprocess.run(base + ["--matte", f"{prefix},17,2,face"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    for k in range(2):
        cov = np.floor(np.clip(ref["count"][k] / 17.0, 0, 1) * 255 + 0.5).astype(np.int64)
        assert np.array_equal(_ppm(tmp_path / f"m.coverage{k}.ppm"), np.repeat(cov[..., None], 3, axis=-1)), k
        img = _ppm(tmp_path / f"m.id{k}.ppm")
        empty = ref["id"][k] < 0
        assert not img[empty].any() and img[~empty].all()
        hsh = ((ref["id"][k].astype(np.int64) + 1) * 2654435761) & 0xFFFFFFFF
        want = np.stack([((hsh >> (8 * c)) & 0xFF) | 0x80 for c in range(3)], axis=-1)
        assert np.array_equal(img[~empty], want[~empty])
    rest = np.floor(np.clip(ref["rest"] / 17.0, 0, 1) * 255 + 0.5).astype(np.int64)
    assert np.array_equal(_ppm(tmp_path / "m.rest.ppm"), np.repeat(rest[..., None], 3, axis=-1))
    assert not (tmp_path / "m.id2.ppm").exists()
    for what, spec in {"ranks 9": f"{prefix},16,9", "samples 0": f"{prefix},0", "a level": f"{prefix},16,4,edge",
                       "five fields": f"{prefix},16,4,face,1", "no prefix": ",16"}.items():
        p = subprocess.run(base + ["--matte", spec], capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and "--matte" in p.stderr, (what, p.stderr)


def test_13_sequences_and_progressions_show_the_resolved_frame_and_feed_nothing_back():
    scene = rtgo.Scene.from_json_text(C_FLOOR)
    cams = [dict(CAMERA, position=[0.05 * f, 0.6, 3]) for f in range(3)]
    r = _renderer()
    r.render_sequence(scene, W, H, cams, temporal=True, denoise=True)
    acc, den = r.last_temporal_linear.copy(), r.last_denoised_linear.copy()
    assert r.last_resolved_linear is None
    img = r.render_sequence(scene, W, H, cams, temporal=True, denoise=True, matte=True)
    _same_bits(r.last_temporal_linear, acc, "the history is the unresolved accumulation")
    _same_bits(r.last_denoised_linear, den, "the filter's frames")
    assert r.last_resolved_linear.shape == (3, H, W, 3)
    for f in range(3):
        r.set_seed(SEED + f)  # (frame f's seed: its first-hit ids and its matte)
        obj = r.render_aov(scene, W, H, camera=cams[f])["object"]
        m = r.render_matte(scene, W, H, camera=cams[f])
        host, host_rgba = rtgo.matte_resolve_host(den[f], obj, m["id"], m["count"], m["rest"], 16)
        _same_bits(r.last_resolved_linear[f], host, ("frame", f))
        assert img[f].tobytes() == host_rgba.tobytes(), f
    r.set_seed(SEED)
    # without a filter the accumulated frame is the one resolved
    r.render_sequence(scene, W, H, cams, temporal=True, matte=8)
    _same_bits(r.last_temporal_linear, acc, "no filter: the accumulation")
    assert (bits(r.last_resolved_linear) != bits(acc)).any()
    # a progression: the matte once, every pass's denoised image resolved
    r.set_samples(4)
    seen = []
    last = r.render_progressive(scene, W, H, 2, denoise=True, matte=True, on_pass=lambda n, im, ch: seen.append(im.copy()))
    r.set_samples(2)  # (the features of the first pass's samples)
    obj = r.render_aov(scene, W, H)["object"]
    m = r.render_matte(scene, W, H)
    host, host_rgba = rtgo.matte_resolve_host(r.last_denoised_linear, obj, m["id"], m["count"], m["rest"], 16)
    _same_bits(r.last_resolved_linear, host, "the progression's last image")
    assert last.tobytes() == host_rgba.tobytes() and len(seen) == 2 and seen[-1].tobytes() == last.tobytes()
    r.close()
