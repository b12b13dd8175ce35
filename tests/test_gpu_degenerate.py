"""GPU: every kernel path against the oracle on the degenerate scenes
(tests/degenerate_cases.py), at the guards of the kernels' shortcuts.

The kernels are exact only through shortcuts (shadow-cone culling, self
exclusion, box slab pruning, inert lights, wide mode, the quantized BVH slab
test, the cone walk), each with a guard for the inputs it cannot handle;
DESIGN.md ("Guards and the scenes that reach them") maps every guard to the
scene here that reaches it.  Every comparison is the project's bar: the
float32 linear radiance and the RGBA8 image equal the oracle's byte for byte,
NaN in the same places (_same); no tolerance, since no sky is involved.

Why every loop these scenes reach terminates, whatever values flow through it
(read in the sources before any non-finite value ran on a device):
  - the rejection loops (rand_in_unit_sphere, the soft points) accept or
    reject on the raw 32-bit draws alone (unit_ball_accept): no scene value;
  - soft_coop's `while (need > 0)` and soft_queue's passes and ring lower
    `need` by the accepted tries of those same draws; the ring's positions are
    wave-uniform counts of accepted points and its capacity bounds what a pass
    can leave (kRing); what a shadow ray hits only changes a count;
  - the BVH walks (closest_hit / any_hit of rt_device.h, descend / descend_x /
    descend4 and the cone walk of rt_wavefront.hip) are depth-first walks of a
    finite tree that enter every node at most once; with "every box is hit"
    (ray_q's !ok, NaN slabs) they enter all of them, once.  The stack holds
    one pending sibling (three in the 4-wide tree) per level, and the builder
    refuses trees deeper than the stack (bvh.cpp: kStack, bvh4_stack is
    computed for the all-hit case);
  - a path's bounce loop counts depth up to max_depth (traceRay's cut-off
    comes before any hit test), in the megakernel, the stream kernels and the
    wavefront kernels alike; the wavefront host loop stops when the device
    reports no live path, and in any case after samples + max_depth + 8 rounds
    ("wavefront loop did not terminate").
Non-finite geometry is rendered for spheres alone (no BVH: the linear scan's
loops run over the primitive counts); with cubes it is refused (rt_api.h).

"""
import functools

import numpy as np
import pytest

import degenerate_cases as dc
import oracle
import rtgo
from gpu_util import render_dev
from scene_cases import make_settings

pytestmark = pytest.mark.gpu

W, H = 72, 48
PATH_KEYS = ("camera_rays", "bounce_rays", "shadow_rays", "shade_events", "light_evals", "rng_draws")

LINEAR = [n for n in dc.LINEAR if n not in dc.GEOMETRY]
SCHEDULED = [n for n in LINEAR if n in dc.FINITE or n.startswith(("nonfinite_lights", "nonfinite_materials"))]
SCHEDULES = [("one_pixel_blocks", {"block_work": 1}), ("no_frustum_no_stage", {"frustum": 0, "stage": 0}),
             ("one_block", {"block_work": 1e6})]
STREAM_TUNINGS = [("auto", {}), ("forced", {"stream": 1})]


@functools.lru_cache(maxsize=None)
def _scene(name, spheres=False):
    sc = dc.SCENES[name]
    return dc.load(rtgo, dc.spheres_only(sc) if spheres else sc)


@functools.lru_cache(maxsize=None)
def _oracle(name, spheres, spp, seed):
    """The oracle's (float32 linear (H*W, 3), RGBA8 (H*W, 4), counts), computed once."""
    ref, ref_rgba, counts = oracle.render(_scene(name, spheres), W, H, make_settings(rtgo, {"samples": spp}, seed),
                                          counts=True)
    return ref.astype(np.float32).reshape(-1, 3), ref_rgba.reshape(-1, 4), counts


def _same(lin, rgba, ref, ref_rgba, what):
    """NaN in the same places, every other value and the RGBA8 image byte for
    byte; the figures are printed first.  A NaN's sign is not compared: where
    the whole image is NaN (nonfinite_geometry_nan_first) gfx950 left
    0xffc00000 and the oracle's host 0x7fc00000 -- the sign of the NaN an
    invalid operation makes is the processor's, and neither the reference nor
    the tone map reads it; the NaNs of every other scene had equal bytes."""
    lin, rgba = np.asarray(lin, np.float32).reshape(-1, 3), np.asarray(rgba).reshape(-1, 4)
    nan, ref_nan = np.isnan(lin), np.isnan(ref)
    diff = (lin.view(np.uint32) != ref.view(np.uint32)) & ~nan & ~ref_nan
    print(what, "NaN values", int(nan.sum()), "of the oracle", int(ref_nan.sum()), "pattern differs at",
          int((nan != ref_nan).sum()), "; other values differ at", int(diff.sum()),
          "; RGBA pixels differ at", int((rgba != ref_rgba).any(axis=1).sum()))
    assert (nan == ref_nan).all(), what
    assert not diff.any(), what
    assert np.where(nan, np.float32(0), lin).tobytes() == np.where(ref_nan, np.float32(0), ref).tobytes(), what
    assert rgba.tobytes() == ref_rgba.tobytes(), what


def _st(spp, seed):
    return make_settings(rtgo, {"samples": spp}, seed)


# ------------------------------------------------------------ block kernel
@pytest.mark.parametrize("seed", (1, 2))
@pytest.mark.parametrize("name", LINEAR)
def test_block_kernel(name, seed):
    lin, rgba, _, _ = render_dev(_scene(name), W, H, _st(4, seed))
    _same(lin, rgba, *_oracle(name, False, 4, seed)[:2], (name, seed))


@pytest.mark.parametrize("tname,tun", SCHEDULES, ids=[t[0] for t in SCHEDULES])
@pytest.mark.parametrize("name", SCHEDULED)
def test_schedules(name, tname, tun):
    """One-pixel blocks, no frustum masks and no LDS staging, one block per tile."""
    lin, rgba, _, _ = render_dev(_scene(name), W, H, _st(5, 3), tuning=rtgo.default_tuning(**tun))
    _same(lin, rgba, *_oracle(name, False, 5, 3)[:2], (name, tname))


@pytest.mark.parametrize("name", LINEAR)
def test_path_counts(name):
    """A shadow ray wrongly culled or wrongly kept shows as 16 soft rays and their draws."""
    lin, rgba, _, counts = render_dev(_scene(name), W, H, _st(4, 1), count=True)
    ref, ref_rgba, want = _oracle(name, False, 4, 1)
    print(name, {k: (counts[k], want[k]) for k in PATH_KEYS})
    assert {k: counts[k] for k in PATH_KEYS} == {k: want[k] for k in PATH_KEYS}
    _same(lin, rgba, ref, ref_rgba, name)


@pytest.mark.parametrize("name", ("neg_zero_radius", "nonfinite_materials", "nonfinite_materials_inf_colour"))
def test_parallel_renderer_entry_point(name):
    """rt_renderer_render (rtgo.ParallelRenderer, host buffers) on one finite and one non-finite family."""
    r = rtgo.ParallelRenderer()
    r.set_samples(4)
    r.set_seed(2)
    rgba = r.render(_scene(name), W, H)
    _same(r.last_linear, rgba, *_oracle(name, False, 4, 2)[:2], name)
    r.close()


# ------------------------------------------------------------ stream kernels
def _batched(name, spheres, seeds, tun, spp=4):
    """One rt_context_render_frames_async launch of len(seeds) frames (the
    pattern of test_gpu_stream_spheres.py): every frame against the oracle;
    the launch must have streamed."""
    import torch

    n = len(seeds)
    lin = torch.full((n, W * H * 3), float("nan"), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((n, W * H * 4), dtype=torch.uint8, device="cuda")
    c = rtgo.Context(0)
    c.set_tuning(rtgo.default_tuning(**tun))
    c.set_scene(_scene(name, spheres))
    c.render_frames_async(W, H, _st(spp, 1), list(seeds), [lin[f].data_ptr() for f in range(n)],
                          [rgba[f].data_ptr() for f in range(n)], 0, 0, 1, rtgo.RT_LAYOUT_IMAGE)
    torch.cuda.synchronize()
    stats = c.stats()
    c.close()
    assert stats["stream_launches"] == 1 and stats["batched_launches"] == 1, stats
    lin, rgba = lin.cpu().numpy(), rgba.cpu().numpy()
    for f, seed in enumerate(seeds):
        _same(lin[f], rgba[f], *_oracle(name, spheres, spp, seed)[:2], (name, seed))


@pytest.mark.parametrize("tname,tun", STREAM_TUNINGS, ids=[t[0] for t in STREAM_TUNINGS])
@pytest.mark.parametrize("name", LINEAR)
def test_stream_sphere_kernels(name, tname, tun):
    """The family without its cubes: the spheres-only stream kernel."""
    _batched(name, True, (1, 2), tun)


@pytest.mark.parametrize("name", ("flat_cubes", "coincident"))
def test_generic_stream_kernel(name):
    """Flat cubes and the coincident cube pair through the stream kernel with triangles."""
    _batched(name, False, (1, 2), {"stream": 1})


# ------------------------------------------------------------ BVH
def _path(name, mega, spheres=False, force_bvh=0, **tun):
    t = rtgo.default_tuning(**tun)
    t.path = rtgo.RT_PATH_MEGAKERNEL if mega else rtgo.RT_PATH_AUTO
    lin, rgba, _, counts = render_dev(_scene(name, spheres), W, H, _st(4, 1), tuning=t, force_bvh=force_bvh, count=True)
    return lin, rgba, counts


@pytest.mark.parametrize("name", dc.FIELD)
def test_bvh_wavefront_and_megakernel(name):
    """More than 64 spheres: the BVH, through the wavefront kernels and through
    the megakernel, against the oracle and against each other."""
    ref, ref_rgba, want = _oracle(name, False, 4, 1)
    lw, rw, cw = _path(name, mega=False)
    _same(lw, rw, ref, ref_rgba, (name, "wavefront"))
    lm, rm, cm = _path(name, mega=True)
    _same(lm, rm, ref, ref_rgba, (name, "megakernel"))
    print(name, {k: (cw[k], cm[k], want[k]) for k in PATH_KEYS})
    assert {k: cw[k] for k in PATH_KEYS} == {k: want[k] for k in PATH_KEYS}
    assert {k: cm[k] for k in PATH_KEYS} == {k: want[k] for k in PATH_KEYS}


@pytest.mark.parametrize("tname,tun", [("binary_tree_walk", {"wf_lds_nodes": 0}), ("leaf1", {"bvh_leaf": 1})])
@pytest.mark.parametrize("name", dc.FIELD)
def test_bvh_wavefront_tunings(name, tname, tun):
    ref, ref_rgba, want = _oracle(name, False, 4, 1)
    lw, rw, cw = _path(name, mega=False, **tun)
    _same(lw, rw, ref, ref_rgba, (name, tname))
    assert {k: cw[k] for k in PATH_KEYS} == {k: want[k] for k in PATH_KEYS}


@pytest.mark.parametrize("mega", (False, True), ids=("wavefront", "megakernel"))
@pytest.mark.parametrize("name", ("neg_zero_radius", "coincident"))
def test_forced_bvh(name, mega):
    """The small sphere-only scenes through a forced BVH: the tie rule and the
    negative radii in the BVH's closest hit."""
    lin, rgba, counts = _path(name, mega=mega, spheres=True, force_bvh=1)
    ref, ref_rgba, want = _oracle(name, True, 4, 1)
    _same(lin, rgba, ref, ref_rgba, name)
    assert {k: counts[k] for k in PATH_KEYS} == {k: want[k] for k in PATH_KEYS}


# ------------------------------------------------------------ progression
@pytest.mark.parametrize("name", ("zero_neg_colour", "nonfinite_materials", "nonfinite_materials_inf_colour"))
def test_progression_of_two_adds(name):
    """2 + 2 samples equal the 4-sample render: negative and NaN sums carry across adds."""
    import torch

    lin = torch.full((W * H * 3,), float("nan"), dtype=torch.float32, device="cuda")
    rgba = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    c = rtgo.Context(0)
    c.set_scene(_scene(name))
    c.progressive_begin(W, H, _st(4, 1), 0, 1, rtgo.RT_LAYOUT_IMAGE)
    for done in (2, 4):
        c.progressive_add(2, lin.data_ptr(), rgba.data_ptr(), 0)
        torch.cuda.synchronize()
        _same(lin.cpu().numpy(), rgba.cpu().numpy(), *_oracle(name, False, done, 1)[:2], (name, done))
    c.progressive_end()
    c.close()


# ------------------------------------------------------------ non-finite geometry
@pytest.mark.parametrize("tname,tun", [("default", {}), ("no_frustum_no_stage", {"frustum": 0, "stage": 0})])
@pytest.mark.parametrize("name", dc.GEOMETRY)
def test_nonfinite_spheres(name, tname, tun):
    """The spheres of the non-finite geometry scenes (a NaN or Inf centre or
    radius among finite spheres; no cube): image and path counts.  Such a
    sphere is hit by every ray it cannot be compared with, camera and shadow
    rays alike, so the culling must keep it (in_cone, cone_meets_sphere)."""
    lin, rgba, _, counts = render_dev(_scene(name, True), W, H, _st(4, 1), tuning=rtgo.default_tuning(**tun), count=True)
    ref, ref_rgba, want = _oracle(name, True, 4, 1)
    _same(lin, rgba, ref, ref_rgba, (name, tname))
    assert {k: counts[k] for k in PATH_KEYS} == {k: want[k] for k in PATH_KEYS}


@pytest.mark.parametrize("name", ("nonfinite_geometry_nan_radius", "nonfinite_geometry_inf_centre"))
def test_nonfinite_spheres_get_no_bvh(name):
    """... over a field of 72 spheres, and with a forced BVH: the linear scan renders it."""
    sc = dc._field(dc.SCENES[name])
    scene = dc.load(rtgo, sc)
    st = _st(4, 1)
    ref, ref_rgba, want = oracle.render(scene, W, H, st, counts=True)
    for force in (0, 1):
        lin, rgba, _, counts = render_dev(scene, W, H, st, force_bvh=force, count=True)
        _same(lin, rgba, ref.astype(np.float32).reshape(-1, 3), ref_rgba.reshape(-1, 4), (name, force))
        assert {k: counts[k] for k in PATH_KEYS} == {k: want[k] for k in PATH_KEYS}


REFUSED = [("nonfinite_geometry_nan_radius", "object 6: sphere radius is not finite in a scene with cubes"),
           ("nonfinite_geometry_inf_centre", "object 6: sphere position is not finite in a scene with cubes"),
           ("nonfinite_geometry_nan_cube", "object 6: cube size is not finite"),
           ("nonfinite_geometry_inf_cube", "object 6: cube size is not finite"),
           ("nonfinite_geometry_nan_first", "object 0: sphere radius is not finite in a scene with cubes")]


@pytest.mark.parametrize("name,message", REFUSED, ids=[r[0] for r in REFUSED])
def test_nonfinite_geometry_with_cubes_is_refused(name, message):
    """Every entry point that takes a scene: rt_context_set_scene, rt_render, rt_renderer_render."""
    scene = _scene(name)
    c = rtgo.Context(0)
    with pytest.raises(rtgo.RenderError, match=message):
        c.set_scene(scene)
    c.close()
    with pytest.raises(rtgo.RenderError, match=message):
        rtgo.render(scene, W, H, _st(1, 1))
    r = rtgo.ParallelRenderer()
    r.set_samples(1)
    with pytest.raises(rtgo.RenderError, match=message):
        r.render(scene, W, H)
    with pytest.raises(rtgo.RenderError, match=message):
        r.render_progressive(scene, W, H, 1)
    r.close()
