"""GPU: specular-through feature buffers (rt_context_render_aov_spec_async,
DESIGN.md §4.16).

The seven buffers are held, bit for bit, to the definition restated from the
oracle's own parts (tests/aov_spec_reference.py) on S_MIRROR
(tests/spec_cases.py): the reference camera and a general look-at camera, every
max_bounces and max_roughness at which a chain ends differently, sizes that
leave a partial wave, the linear scan, the mixed tree and the tree of a
70-sphere field with mirrors, and two mirrors facing each other, where every
chain runs to the cap.  With no bounce, or nothing to follow, the first five
buffers are the first-hit pass's byte for byte.  The other cases pin what the
call promises around the buffers, as tests/test_gpu_aov.py does for the
first-hit call: independence, no side effects, partial outputs, refusals, and
the Python layer and the CLI.  Every case is at most 72x48 pixels and 5
samples; the references are computed once (reference() caches) and shared."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import rtgo
from aov_spec_reference import bits, reference
from conftest import ROOT
from scene_cases import make_settings
from sequence_cases import GENERAL, scene_json
from spec_cases import (CUBE_1, FACING_CUBES, FACING_SPHERES, MIRROR_SPHERE, ROUGH_METAL_SPHERE, S_MIRROR,
                        SHINY_SPHERE, field70_mirrors, text)

pytestmark = pytest.mark.gpu

REF, LOOKAT = rtgo.RT_CAMERA_REFERENCE, rtgo.RT_CAMERA_LOOKAT
RT_E_INVALID = -1
W, H, SPP, SEED = 72, 48, 4, 3
NAMES = rtgo.AOV_SPEC_NAMES
FIRST = rtgo.AOV_NAMES
S_MIRROR_TEXT = text(S_MIRROR)
GENERAL_TEXT = json.dumps(GENERAL)


@functools.lru_cache(maxsize=None)
def _field_text():
    return json.dumps(field70_mirrors())


def _settings(samples=SPP, seed=SEED, camera=REF, **over):
    st = make_settings(rtgo, dict({"samples": samples, "max_depth": 50}, **over), seed)
    st.camera = camera
    return st


class _Spec:
    """One rt_context holding a scene, and sentinel-filled feature buffers."""

    SENTINEL_F, SENTINEL_I = -1234.5, -77

    def __init__(self, scene_text, w, h, force_bvh=0, tun=None, set_scene=True):
        self.w, self.h = w, h
        self.ctx = rtgo.Context(0)
        if tun is not None:
            self.ctx.set_tuning(rtgo.default_tuning(**tun))
        if set_scene:
            self.ctx.set_scene(rtgo.Scene.from_json_text(scene_text), force_bvh=force_bvh)
        self.fill()

    def fill(self):
        import torch

        n = self.w * self.h
        self.buf = {k: torch.full((n * (3 if k in ("albedo", "normal") else 1),),
                                  self.SENTINEL_I if k == "object" else self.SENTINEL_F,
                                  dtype=torch.int32 if k == "object" else torch.float32, device="cuda") for k in NAMES}

    def pointers(self, names=NAMES):
        return rtgo.AovSpecBuffers(*[self.buf[k].data_ptr() if k in names else None for k in NAMES])

    def arrays(self):
        import torch

        torch.cuda.synchronize()
        return {k: self.buf[k].cpu().numpy().reshape((self.h, self.w, 3) if k in ("albedo", "normal")
                                                     else (self.h, self.w)) for k in NAMES}

    def run(self, st, camera=None, names=NAMES, spec=None):
        self.ctx.render_aov_spec_async(self.w, self.h, st, self.pointers(names), spec=spec, camera=camera)
        return self.arrays()

    def first_hit(self, st, camera=None):
        """The first-hit pass of the same context into the first five buffers."""
        self.ctx.render_aov_async(self.w, self.h, st, rtgo.AovBuffers(*[self.buf[k].data_ptr() for k in FIRST]),
                                  camera=camera)
        return self.arrays()

    def untouched(self, names=NAMES):
        a = self.arrays()
        return all(np.all(a[k] == (self.SENTINEL_I if k == "object" else self.SENTINEL_F)) for k in names)

    def close(self):
        self.ctx.close()


def _spec(scene_text, w, h, st, force_bvh=0, tun=None, camera=None, spec=None):
    a = _Spec(scene_text, w, h, force_bvh, tun)
    out = a.run(st, camera, spec=spec)
    a.close()
    return out


def _first_hit(scene_text, w, h, st, force_bvh=0):
    a = _Spec(scene_text, w, h, force_bvh)
    out = a.first_hit(st)
    a.close()
    return out


def _same(got, want, what="", names=NAMES):
    for k in names:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert bad.size == 0, (what, k, len(bad), bad[:4].tolist())


def _bytes_equal(got, want, what, names=NAMES):
    for k in names:
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def _conditions():
    """Conditions on the reference alone: the comparisons cannot pass vacuously."""
    ref = reference(S_MIRROR_TEXT, W, H, SPP, SEED)
    assert int((ref["bounces"] > 0).sum()) >= 200, int((ref["bounces"] > 0).sum())
    assert ref["stats"]["first_k2"] >= 20, ref["stats"]
    assert ref["stats"]["mirror_miss"] >= 20, ref["stats"]
    assert reference(S_MIRROR_TEXT, W, H, SPP, SEED, max_bounces=2)["stats"]["cap"] >= 1
    partial = (ref["specular"] > 0) & (ref["specular"] < 1)
    assert int(partial.sum()) >= 30, int(partial.sum())
    assert set(range(7)) <= set(np.unique(ref["object"]).tolist())
    return ref


@functools.lru_cache(maxsize=None)
def _case1():
    """S_MIRROR at 72x48x4, seed 3, reference camera, linear scan, default parameters (shared)."""
    return _spec(S_MIRROR_TEXT, W, H, _settings(), force_bvh=-1)


def test_1_reference_camera_linear_scan_equals_the_definition():
    ref = _conditions()
    _same(_case1(), ref, "S_MIRROR")


def test_2_look_at_camera_as_argument_and_as_the_scenes():
    ref = reference(S_MIRROR_TEXT, W, H, SPP, SEED, GENERAL_TEXT, LOOKAT)
    assert int((ref["bounces"] > 0).sum()) >= 100 and int((ref["coverage"] > 0).sum()) >= 350
    st = _settings(camera=LOOKAT)
    by_arg = _spec(S_MIRROR_TEXT, W, H, st, force_bvh=-1, camera=GENERAL)
    by_scene = _spec(text(S_MIRROR, GENERAL), W, H, st, force_bvh=-1)
    _bytes_equal(by_arg, by_scene, "argument == scene's")
    _same(by_arg, ref, "GENERAL")


@pytest.mark.parametrize("max_bounces", [0, 1, 2, 16])
def test_3_max_bounces(max_bounces):
    ref = reference(S_MIRROR_TEXT, W, H, SPP, SEED, max_bounces=max_bounces)
    assert ref["bounces"].max() <= max_bounces
    if max_bounces:
        assert ref["stats"]["cap"] >= 1 or max_bounces == 16
        assert (ref["bounces"] == max_bounces).any() or max_bounces == 16
    got = _spec(S_MIRROR_TEXT, W, H, _settings(), force_bvh=-1, spec={"max_bounces": max_bounces})
    _same(got, ref, f"max_bounces {max_bounces}")
    if max_bounces == 0:  # the first five buffers are the first-hit pass's, and the flag is still set
        _bytes_equal(got, _first_hit(S_MIRROR_TEXT, W, H, _settings(), force_bvh=-1), "no bounce", FIRST)
        assert not got["bounces"].any() and (got["specular"] == 1).sum() >= 200


def test_3_nothing_followed_equals_the_first_hit_pass():
    """S has no roughness-0 metal: with max_roughness 0 nothing is followed."""
    s = scene_json("S")
    got = _spec(s, W, H, _settings(), force_bvh=-1, spec={"max_roughness": 0.0})
    _bytes_equal(got, _first_hit(s, W, H, _settings(), force_bvh=-1), "S, max_roughness 0", FIRST)
    assert not got["bounces"].any() and not got["specular"].any() and (got["coverage"] > 0).sum() >= 300


@pytest.mark.parametrize("max_roughness", [0.0, 0.1, 0.2])
def test_4_max_roughness(max_roughness):
    ref = reference(S_MIRROR_TEXT, W, H, SPP, SEED, max_roughness=max_roughness)
    first = reference(S_MIRROR_TEXT, W, H, SPP, SEED, max_bounces=0)  # (object: the first hits')
    for obj, threshold in ((ROUGH_METAL_SPHERE, 0.2), (SHINY_SPHERE, 0.1), (CUBE_1, 0.0), (MIRROR_SPHERE, 0.0)):
        seen = first["object"] == obj  # (the lowest hitting sample's first hit)
        assert seen.sum() >= 25, obj
        if max_roughness >= threshold:  # followed: that sample carries the flag
            assert (ref["specular"][seen] > 0).all(), (obj, max_roughness)
        else:  # not followed: no flag and no bounce wherever all the samples see it
            assert (seen & (ref["specular"] == 0) & (ref["bounces"] == 0)).sum() >= 20, (obj, max_roughness)
            assert (ref["specular"][seen] < 1).all(), (obj, max_roughness)
    got = _spec(S_MIRROR_TEXT, W, H, _settings(), force_bvh=-1, spec={"max_roughness": max_roughness})
    _same(got, ref, f"max_roughness {max_roughness}")


@pytest.mark.parametrize("w,h,spp", [(33, 17, 3), (1, 1, 5)])
def test_5_sizes_that_leave_stragglers(w, h, spp):
    """A partial wave (33 * 17 = 561 = 8 * 64 + 49 pixels), a single pixel."""
    _same(_spec(S_MIRROR_TEXT, w, h, _settings(samples=spp), force_bvh=-1),
          reference(S_MIRROR_TEXT, w, h, spp, SEED), (w, h, spp))


def test_6_trees_find_the_linear_scans_chains():
    mixed = _spec(S_MIRROR_TEXT, W, H, _settings(), force_bvh=1)
    _bytes_equal(mixed, _case1(), "S_MIRROR mixed tree")
    st2 = _settings(samples=2)
    tree, scan = _spec(_field_text(), W, H, st2), _spec(_field_text(), W, H, st2, force_bvh=-1)
    assert (tree["bounces"] > 0).sum() >= 30 and len(np.unique(tree["object"])) > 30  # (the field is in view)
    _bytes_equal(tree, scan, "field70 with mirrors")
    ref = reference(_field_text(), 24, 16, 2, SEED)
    assert len(np.unique(ref["object"])) > 10 and (ref["bounces"] > 0).sum() >= 5
    _same(_spec(_field_text(), 24, 16, st2), ref, "field70 with mirrors 24x16")


@pytest.mark.parametrize("name,scene,max_bounces", [("cubes", FACING_CUBES, 5), ("cubes", FACING_CUBES, 16),
                                                    ("spheres", FACING_SPHERES, 4)])
def test_7_facing_mirrors_run_every_chain_to_the_cap(name, scene, max_bounces):
    w, h, spp = 24, 16, 2
    ref = reference(text(scene), w, h, spp, SEED, max_bounces=max_bounces)
    assert (ref["coverage"] == 1).all() and (ref["specular"] == 1).all()
    assert (ref["bounces"] == max_bounces).all()
    assert ref["stats"]["cap"] == w * h * spp and ref["stats"]["mirror_miss"] == 0
    assert set(np.unique(ref["object"]).tolist()) == {max_bounces % 2}  # (the mirrors take turns)
    got = _spec(text(scene), w, h, _settings(samples=spp), spec={"max_bounces": max_bounces})
    assert (got["bounces"] == max_bounces).all()
    _same(got, ref, (name, max_bounces))


def test_8_only_scene_size_camera_samples_seed_and_spec_matter():
    want = _case1()
    cases = {"max_depth 0": dict(st=_settings(max_depth=0)), "hard shadows": dict(st=_settings(soft_shadows=0)),
             "no recursion": dict(st=_settings(recursive_reflections=0)), "a sky": dict(st=_settings(sky=1)),
             "stream tuning": dict(st=_settings(), tun={"stream": 1, "stream_chunk": 64, "stream_order": 0})}
    for what, kw in cases.items():
        _bytes_equal(_spec(S_MIRROR_TEXT, W, H, kw["st"], force_bvh=-1, tun=kw.get("tun")), want, what)
    other = _spec(S_MIRROR_TEXT, W, H, _settings(seed=SEED + 1), force_bvh=-1)
    partial = (want["coverage"] > 0) & (want["coverage"] < 1)
    changed = np.zeros((H, W), bool)
    for k in NAMES:
        changed |= (bits(other[k]) != bits(want[k])).reshape(H, W, -1).any(axis=-1)
    assert (changed & partial).any()


def test_8_no_side_effects_on_renders_statistics_and_progressions():
    import torch

    a = _Spec(S_MIRROR_TEXT, W, H, force_bvh=-1)
    st = _settings()
    lin = torch.zeros((2, W * H * 3), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((2, W * H * 4), dtype=torch.uint8, device="cuda")
    a.ctx.render_async(W, H, st, lin[0].data_ptr(), rgba[0].data_ptr(), 0)
    render_seconds = a.ctx.last_kernel_seconds()
    s0 = a.ctx.stats()
    got = a.run(st)
    spec_seconds = a.ctx.last_kernel_seconds()  # (its own events: the pass's device time)
    assert a.ctx.stats() == s0
    a.ctx.render_async(W, H, st, lin[1].data_ptr(), rgba[1].data_ptr(), 0)
    torch.cuda.synchronize()
    assert lin[0].cpu().numpy().tobytes() == lin[1].cpu().numpy().tobytes()
    assert rgba[0].cpu().numpy().tobytes() == rgba[1].cpu().numpy().tobytes()
    assert rgba[0].any()
    _bytes_equal(got, _case1(), "between two renders")
    assert 0 < spec_seconds < 1 and 0 < render_seconds < 1
    # a progression: two adds of two samples, with and without a pass between them
    imgs = []
    for interrupt in (False, True):
        a.ctx.progressive_begin(W, H, st)
        a.ctx.progressive_add(2, lin[0].data_ptr(), rgba[0].data_ptr(), 0)
        if interrupt:
            a.fill()
            mid = a.run(_settings(samples=3, seed=9))
            assert (mid["bounces"] > 0).any()
        assert a.ctx.progressive_samples() == 2
        a.ctx.progressive_add(2, lin[0].data_ptr(), rgba[0].data_ptr(), 0)
        torch.cuda.synchronize()
        imgs.append((lin[0].cpu().numpy().tobytes(), rgba[0].cpu().numpy().tobytes()))
        a.ctx.progressive_end()
    assert imgs[0] == imgs[1]
    assert imgs[0][0] == lin[1].cpu().numpy().tobytes()  # (and both are the one-call render)
    a.close()


def test_8_partial_output_writes_only_the_buffers_given():
    a = _Spec(S_MIRROR_TEXT, W, H, force_bvh=-1)
    got = a.run(_settings(), names=("depth", "bounces"))
    assert got["depth"].tobytes() == _case1()["depth"].tobytes()
    assert got["bounces"].tobytes() == _case1()["bounces"].tobytes()
    assert a.untouched(("albedo", "normal", "coverage", "object", "specular"))
    a.fill()
    got = a.run(_settings(), names=("specular",))
    assert got["specular"].tobytes() == _case1()["specular"].tobytes()
    assert a.untouched(("albedo", "normal", "depth", "coverage", "object", "bounces"))
    a.close()


def test_8_invalid_arguments_are_refused_and_touch_nothing():
    lib = rtgo.lib()
    a = _Spec(S_MIRROR_TEXT, W, H, force_bvh=-1)
    st, out, none, ok = _settings(), a.pointers(), rtgo.AovSpecBuffers(), rtgo.default_aov_spec()

    def call(ctx=a.ctx._h, w=W, h=H, st=st, cam=None, spec=ok, out=out):
        return lib.rt_context_render_aov_spec_async(ctx, w, h, ctypes.byref(st) if st is not None else None,
                                                    ctypes.byref(cam) if cam is not None else None,
                                                    ctypes.byref(spec) if spec is not None else None,
                                                    ctypes.byref(out) if out is not None else None, None)

    same_point = rtgo._as_camera({"position": [1, 1, 1], "lookAt": [1, 1, 1], "up": [0, 1, 0], "fov": 60})
    empty = _Spec(S_MIRROR_TEXT, W, H, set_scene=False)
    cases = {
        "NULL ctx": dict(ctx=None), "NULL settings": dict(st=None), "NULL out": dict(out=None),
        "all seven NULL": dict(out=none), "no scene": dict(ctx=empty.ctx._h, out=empty.pointers()),
        "samples 0": dict(st=_settings(samples=0)), "samples -1": dict(st=_settings(samples=-1)),
        "width 0": dict(w=0), "height 65537": dict(h=65537), "samples past 2^24": dict(st=_settings(samples=(1 << 24) + 1)),
        "an unknown camera model": dict(st=_settings(camera=7)),
        "a look-at camera without a direction": dict(st=_settings(camera=LOOKAT), cam=same_point),
        "NULL spec": dict(spec=None), "max_bounces -1": dict(spec=rtgo.AovSpec(-1, 0, 0.1)),
        "max_bounces 17": dict(spec=rtgo.AovSpec(17, 0, 0.1)), "max_roughness < 0": dict(spec=rtgo.AovSpec(4, 0, -0.5)),
        "max_roughness NaN": dict(spec=rtgo.AovSpec(4, 0, float("nan"))),
        "max_roughness Inf": dict(spec=rtgo.AovSpec(4, 0, float("inf"))),
    }
    for what, kw in cases.items():
        assert call(**kw) == RT_E_INVALID, what
        assert lib.rt_last_error(), what
        assert a.untouched() and empty.untouched(), what
    assert call() == 0  # (the same call with nothing wrong)
    assert a.arrays()["depth"].tobytes() == _case1()["depth"].tobytes()
    empty.close()
    a.close()


def _renderer():
    r = rtgo.ParallelRenderer(1)
    r.set_samples(SPP)
    r.set_seed(SEED)
    return r


def test_9_render_aov_specular_equals_the_definition():
    r = _renderer()
    scene = rtgo.Scene.from_json_text(S_MIRROR_TEXT)
    got = r.render_aov(scene, W, H, specular="default")
    assert list(got) == NAMES
    _same(got, reference(S_MIRROR_TEXT, W, H, SPP, SEED), "render_aov")
    got2 = r.render_aov(scene, W, H, specular={"max_bounces": 2, "max_roughness": 0.2})
    _same(got2, reference(S_MIRROR_TEXT, W, H, SPP, SEED, max_bounces=2, max_roughness=0.2), "render_aov, a dict")
    assert list(r.render_aov(scene, W, H)) == FIRST  # (without the argument: the five first-hit arrays)
    r.close()


def test_9_render_denoised_guides():
    scene = rtgo.Scene.from_json_text(S_MIRROR_TEXT)
    r = _renderer()
    plain = r.render_denoised(scene, W, H)
    plain_lin = r.last_denoised_linear.copy()
    first = r.render_denoised(scene, W, H, guide="first")
    assert first.tobytes() == plain.tobytes() and r.last_denoised_linear.tobytes() == plain_lin.tobytes()
    f = r.render_aov(scene, W, H)  # today's output: the host filter over the first-hit arrays
    want_lin, want_rgba = rtgo.denoise_host(r.last_linear, f["normal"], f["depth"], f["albedo"], f["object"], None)
    assert plain.tobytes() == want_rgba.tobytes() and bits(plain_lin).tobytes() == bits(want_lin).tobytes()
    img = r.render_denoised(scene, W, H, guide="specular")
    g = r.render_aov(scene, W, H, specular="default")
    want_lin, want_rgba = rtgo.denoise_host(r.last_linear, g["normal"], g["depth"], g["albedo"], g["object"], None)
    assert img.tobytes() == want_rgba.tobytes()
    assert bits(r.last_denoised_linear).tobytes() == bits(want_lin).tobytes()
    assert img.tobytes() != plain.tobytes()
    # the variance-guided filter takes the same guide
    v0 = r.render_denoised(scene, W, H, variance=True)
    v1 = r.render_denoised(scene, W, H, variance=True, guide="specular", specular={"max_bounces": 2})
    assert v0.tobytes() != v1.tobytes()
    # a progression's preview and a sequence's spatial filter
    p0 = r.render_progressive(scene, W, H, 2, denoise=True)
    p1 = r.render_progressive(scene, W, H, 2, denoise=True, guide="specular")
    r.set_samples(2)
    g2 = r.render_aov(scene, W, H, specular="default")  # (the features of the first pass's samples)
    r.set_samples(SPP)
    want_lin, want_rgba = rtgo.denoise_host(r.last_linear, g2["normal"], g2["depth"], g2["albedo"], g2["object"], None)
    assert p1.tobytes() == want_rgba.tobytes() and p1.tobytes() != p0.tobytes()
    cams = [dict(S_MIRROR["camera"], position=[0.1 * k, 0, 3]) for k in range(2)]
    s0 = r.render_sequence(scene, W, H, cams, temporal=True, denoise=True)
    acc0 = r.last_temporal_linear.copy()
    s1 = r.render_sequence(scene, W, H, cams, temporal=True, denoise=True, guide="specular")
    assert r.last_temporal_linear.tobytes() == acc0.tobytes()  # (the accumulation keeps the first-hit buffers)
    assert s1.tobytes() != s0.tobytes()
    r.set_seed(SEED + 1)  # frame 1 of the sequence: seed + 1, its own camera
    g3 = r.render_aov(scene, W, H, camera=cams[1], specular="default")
    want_lin, want_rgba = rtgo.denoise_host(acc0[1], g3["normal"], g3["depth"], g3["albedo"], g3["object"], None)
    assert s1[1].tobytes() == want_rgba.tobytes()
    r.close()


def test_9_cli_writes_the_seven_images(tmp_path):
    r = _renderer()
    got = r.render_aov(rtgo.Scene.from_json_text(S_MIRROR_TEXT), W, H, specular={"max_bounces": 3})
    scene = tmp_path / "s_mirror.json"
    scene.write_text(S_MIRROR_TEXT)
    exe = os.path.join(ROOT, "concurrent-raytracer-go_amd", "build", "raytracer")
    out, prefix = tmp_path / "o.ppm", tmp_path / "f"
    base = [exe, str(scene), str(out), str(W), str(H), "--samples", str(SPP), "--seed", str(SEED)]
    p = subprocess.run(base + ["--aov", str(prefix), "--aov-specular", "3"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    img = {}
    for k in NAMES:
        toks = (tmp_path / f"f.{k}.ppm").read_text().split()
        assert toks[:4] == ["P3", str(W), str(H), "255"], k
        img[k] = np.array(toks[4:], np.int64).reshape(H, W, 3)
    want = np.floor(np.clip(got["albedo"].astype(np.float64), 0, 1) * 255 + 0.5).astype(np.int64)
    assert np.array_equal(img["albedo"], want) and want.any()
    for k, div in (("coverage", 1.0), ("specular", 1.0), ("bounces", 3.0)):  # (bounces / max_bounces)
        grey = np.floor(np.clip(got[k].astype(np.float64) / div, 0, 1) * 255 + 0.5).astype(np.int64)
        assert np.array_equal(img[k], np.repeat(grey[..., None], 3, axis=-1)) and grey.any(), k
    miss = got["object"] < 0
    assert not img["object"][miss].any() and not img["depth"][miss].any() and img["object"][~miss].all()
    assert out.exists()
    # with --denoise the flag switches the guide: the Python layer's image
    want = r.render_denoised(rtgo.Scene.from_json_text(S_MIRROR_TEXT), W, H, guide="specular", specular={"max_bounces": 3})
    p = subprocess.run(base + ["--denoise", "default", "--aov-specular", "3"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    toks = out.read_text().split()
    assert np.array_equal(np.array(toks[4:], np.int64).reshape(H, W, 3), want[..., :3].astype(np.int64))
    # without the flag: the five files, as before
    p = subprocess.run(base + ["--aov", str(tmp_path / "g")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and (tmp_path / "g.depth.ppm").exists() and not (tmp_path / "g.specular.ppm").exists()
    r.close()


def test_10_specular_guide_lowers_the_mirror_cubes_error():
    """S_CUBE at 96x64, one sample, rt_denoise at its defaults; truth is the 256-spp render with seed 77.
    On the pixels whose first hit is the roughness-0 cube the filter guided by the specular-through
    buffers ends closer to the truth than the filter guided by the first hits, which sees one flat metal
    face and blurs what it shows (0.41 to 0.50 of its error at 144x96 over three seeds;
    asserted here as plain "lower"; measured at this size: 0.00417 and 0.00218)."""
    w, h = 96, 64
    scene = rtgo.Scene.from_json_text(scene_json("S_CUBE"))
    t = rtgo.ParallelRenderer(1)
    t.set_samples(256)
    t.set_seed(77)
    t.render(scene, w, h)
    truth = t.last_linear.astype(np.float64)
    t.close()
    r = rtgo.ParallelRenderer(1)
    r.set_samples(1)
    r.set_seed(SEED)
    cube = r.render_aov(scene, w, h)["object"] == CUBE_1
    assert cube.sum() >= 150
    err = {}
    for guide in ("first", "specular"):
        r.render_denoised(scene, w, h, guide=guide)
        err[guide] = float(np.sqrt(((r.last_denoised_linear.astype(np.float64) - truth)[cube] ** 2).mean()))
    r.close()
    print("cube RMSE after rt_denoise, first-hit guide / specular guide:", err)
    assert err["specular"] < err["first"], err
