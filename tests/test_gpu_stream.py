"""GPU: streamed launches do not change a single bit.

With rt_tuning.stream = 1 every eligible launch -- one-frame launches too --
renders through render_stream_kernel (persistent waves that pull (frame, live
pixel, sample) entries off one launch-wide queue and store each path's
radiance in its row) and resolve_rows_kernel (each pixel's rows summed in
sample order, mean, tone map, write).  Every image here must equal the
oracle's, float3 and RGBA8, byte for byte, and every case checks
rt_context_stats.stream_launches, so none passes by falling back to the block
kernel.  The launches that are not eligible (a sky, sample passes) must still
equal the oracle and must not count as streamed."""
import copy
import functools
import json
import os

import numpy as np
import pytest

import oracle
import rtgo
from scene_cases import SCENES, load_case, make_settings

pytestmark = pytest.mark.gpu

STREAM = {"stream": 1}
MIB = 1 << 20


class _Ctx:
    """One rt_context with a tuning and a scene; renders return numpy images."""

    def __init__(self, scene, tun):
        self.ctx = rtgo.Context(0)
        self.ctx.set_tuning(rtgo.default_tuning(**tun))
        self.ctx.set_scene(scene)

    def frames(self, w, h, st, seeds):
        """One rt_context_render_frames_async call: (n, h, w, 3) f32, (n, h, w, 4) u8."""
        import torch

        n = len(seeds)
        lin = torch.full((n, w * h * 3), float("nan"), dtype=torch.float32, device="cuda")
        rgba = torch.zeros((n, w * h * 4), dtype=torch.uint8, device="cuda")
        self.ctx.render_frames_async(w, h, st, list(seeds), [lin[f].data_ptr() for f in range(n)],
                                     [rgba[f].data_ptr() for f in range(n)], 0, 0, 1, rtgo.RT_LAYOUT_IMAGE)
        torch.cuda.synchronize()
        return lin.cpu().numpy().reshape(n, h, w, 3), rgba.cpu().numpy().reshape(n, h, w, 4)

    def one(self, w, h, st):
        """One rt_context_render_async call: (h, w, 3) f32, (h, w, 4) u8."""
        import torch

        lin = torch.full((w * h * 3,), float("nan"), dtype=torch.float32, device="cuda")
        rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
        self.ctx.render_async(w, h, st, lin.data_ptr(), rgba.data_ptr(), 0)
        torch.cuda.synchronize()
        return lin.cpu().numpy().reshape(h, w, 3), rgba.cpu().numpy().reshape(h, w, 4)

    def share(self, w, h, st, rank, world):
        """`rank`'s packed share: (slots, 3) f32, (slots, 4) u8."""
        import torch

        nb, off = rtgo.packed_bytes(w, h, world), rtgo.packed_rgba_offset(w, h, world)
        buf = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        self.ctx.render_async(w, h, st, buf.data_ptr(), buf.data_ptr() + off, 0, rank, world,
                              rtgo.RT_LAYOUT_PACKED_TILES)
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        return b[:off].view(np.float32).reshape(-1, 3), b[off:].reshape(-1, 4)

    def stats(self):
        return self.ctx.stats()

    def close(self):
        self.ctx.close()


_SCENES = {}


def _scene(loader):
    if loader not in _SCENES:
        _SCENES[loader] = _mirror_shell() if loader == ("shell", None) else load_case(rtgo, loader)
    return _SCENES[loader]


def _mirror_shell():
    """scripts/latency_probe.py's scene: the headline spheres inside a mirror
    shell, so every path bounces until the depth cut-off."""
    s = json.load(open(os.path.join(SCENES, "sphere_reflections_light_facing.json")))
    shell = {"type": "sphere", "position": [0, 0, 0], "radius": 30.0,
             "material": {"type": "metal", "color": [0.9, 0.9, 0.9], "roughness": 0.0}}
    s = copy.deepcopy(s)
    s["objects"] = [shell] + s["objects"]
    return rtgo.Scene.from_json_text(json.dumps(s))


@functools.lru_cache(maxsize=None)
def _oracle(loader, w, h, over, seed):
    """The oracle's (float32 linear bytes, RGBA8 bytes) of a case, computed once."""
    st = make_settings(rtgo, dict(over), seed)
    ref, ref_rgba, _ = oracle.render(_scene(loader), w, h, st)
    return ref.astype(np.float32), ref_rgba


def _check(loader, w, h, over, seed, lin, rgba):
    ref, ref_rgba = _oracle(loader, w, h, tuple(sorted(over.items())), seed)
    assert lin.tobytes() == ref.tobytes()
    assert rgba.tobytes() == ref_rgba.tobytes()


def _one_frame(loader, w, h, over, seed, tun=STREAM):
    c = _Ctx(_scene(loader), tun)
    lin, rgba = c.one(w, h, make_settings(rtgo, over, seed))
    stats = c.stats()
    c.close()
    return lin, rgba, stats


ALLM = ("json", None)
ONE_FRAME = [("56x40x3", 56, 40, 3), ("56x40x40", 56, 40, 40), ("40x24x130", 40, 24, 130)]


@pytest.mark.parametrize("name,w,h,spp", ONE_FRAME, ids=[c[0] for c in ONE_FRAME])
def test_one_frame_launches_through_the_stream_path(name, w, h, spp):
    """The shapes of test_schedule_does_not_change_the_image; 56x40 has
    partial tiles on both axes."""
    over = {"samples": spp, "max_depth": 12}
    lin, rgba, stats = _one_frame(ALLM, w, h, over, 4)
    assert stats["stream_launches"] == 1, stats
    _check(ALLM, w, h, over, 4, lin, rgba)


PARITY = [
    ("spheres_facing", ("file", "sphere_reflections_light_facing.json"), 96, 72, {"samples": 8}),
    ("silver_facing", ("file", "final_silver_prism_purple_cube_facing.json"), 96, 72, {"samples": 6}),
    ("all_materials_odd_size_spp", ALLM, 37, 29, {"samples": 3}),
    ("all_materials_depth0", ALLM, 20, 10, {"samples": 2, "max_depth": 0}),
    ("all_materials_hard_shadows", ALLM, 64, 48, {"samples": 4, "soft_shadows": 0}),
    ("all_materials_no_recursion", ALLM, 64, 48, {"samples": 4, "recursive_reflections": 0}),
]


@pytest.mark.parametrize("name,loader,w,h,over", PARITY, ids=[c[0] for c in PARITY])
@pytest.mark.parametrize("seed", [1, 2])
def test_parity_shapes(name, loader, w, h, over, seed):
    lin, rgba, stats = _one_frame(loader, w, h, over, seed)
    assert stats["stream_launches"] == 1, stats
    _check(loader, w, h, over, seed, lin, rgba)


BATCH = (ALLM, 64, 48, {"samples": 6})
BATCH_SEEDS = [(3, 4, 5, 6), (7, 8, 9, 10), (11, 12, 13, 14)]


def test_batched_launches_and_context_reuse():
    """4 frames per launch, three calls on one context: the cursor is reset
    and the row buffer reused between launches, the schedule (and its
    live-pixel list) built once."""
    loader, w, h, over = BATCH
    c = _Ctx(_scene(loader), STREAM)
    st = make_settings(rtgo, over, 1)
    built = None
    for k, seeds in enumerate(BATCH_SEEDS):
        before = c.stats()["stream_launches"]
        lin, rgba = c.frames(w, h, st, seeds)
        s = c.stats()
        assert s["stream_launches"] == before + 1, s
        assert s["batched_launches"] == k + 1 and s["frames"] == 4 * (k + 1), s
        built = s["schedules_built"] if built is None else built
        assert s["schedules_built"] == built, s
        for f, seed in enumerate(seeds):
            _check(loader, w, h, over, seed, lin[f], rgba[f])
    c.close()


def test_grouping_under_the_row_budget():
    """stream_max_mb holds two frames' rows but not three: the 4-frame launch
    runs as two stream + resolve pairs over frames 0-1 and 2-3."""
    loader, w, h, over = BATCH
    probe = _Ctx(_scene(loader), STREAM)
    probe.one(w, h, make_settings(rtgo, over, 1))
    nlive = probe.stats()["stream_live_pixels"]
    probe.close()
    assert nlive > 0
    per = nlive * over["samples"] * 24  # bytes of one frame's rows
    mb = 2.5 * per / MIB  # (rt_tuning.stream_max_mb takes fractions of a MiB)
    c = _Ctx(_scene(loader), dict(STREAM, stream_max_mb=mb))
    seeds = BATCH_SEEDS[0]
    lin, rgba = c.frames(w, h, make_settings(rtgo, over, 1), seeds)
    s = c.stats()
    c.close()
    assert s["stream_launches"] == 2 and s["batched_launches"] == 1, s
    for f, seed in enumerate(seeds):
        _check(loader, w, h, over, seed, lin[f], rgba[f])


def test_fewer_entries_than_lanes():
    """8x8 at one sample: 64 entries at most, so most waves find the queue
    empty on their first claim."""
    over = {"samples": 1}
    lin, rgba, stats = _one_frame(ALLM, 8, 8, over, 5)
    assert stats["stream_launches"] == 1 and 0 < stats["stream_live_pixels"] <= 64, stats
    _check(ALLM, 8, 8, over, 5, lin, rgba)


def test_no_live_pixel_and_an_empty_queue():
    """The as-committed scene (the camera faces away from it): no live pixel,
    no entry; the call returns and the image is black."""
    loader, over = ("file", "sphere_reflections_light.json"), {"samples": 4}
    lin, rgba, stats = _one_frame(loader, 64, 48, over, 1)
    assert stats["stream_launches"] == 1 and stats["stream_live_pixels"] == 0, stats
    assert not lin.any() and not rgba[..., :3].any() and (rgba[..., 3] == 255).all()
    _check(loader, 64, 48, over, 1, lin, rgba)


def test_long_chains_outlive_the_queue():
    """50-bounce paths inside the mirror shell, 70 samples of a few pixels:
    the queue runs out while paths are alive, and a wave holds fresh and deep
    paths together."""
    loader, over = ("shell", None), {"samples": 70, "max_depth": 50}
    lin, rgba, stats = _one_frame(loader, 6, 4, over, 3)
    assert stats["stream_launches"] == 1, stats
    _check(loader, 6, 4, over, 3, lin, rgba)
    # two frames, their entries claimed four at a time, in the frame-major order
    # (the default interleaves the frames of a launch)
    seeds = (3, 9)
    c = _Ctx(_scene(loader), dict(STREAM, stream_chunk=4, stream_order=0))
    lin2, rgba2 = c.frames(6, 4, make_settings(rtgo, over, 1), seeds)
    assert c.stats()["stream_launches"] == 1
    c.close()
    for f, seed in enumerate(seeds):
        _check(loader, 6, 4, over, seed, lin2[f], rgba2[f])


@pytest.mark.parametrize("world", [2, 3])
def test_packed_tiles(world):
    """Every rank's packed share (RT_LAYOUT_PACKED_TILES) against the
    oracle's pixels of its tiles t % world == rank."""
    loader, w, h, over, seed = ("file", "sphere_reflections_light_facing.json"), 96, 64, {"samples": 8}, 2
    ref, ref_rgba = _oracle(loader, w, h, tuple(sorted(over.items())), seed)
    tiles_x = (w + 31) // 32
    ntiles = tiles_x * ((h + 31) // 32)
    for rank in range(world):
        c = _Ctx(_scene(loader), STREAM)
        lin, rgba = c.share(w, h, make_settings(rtgo, over, seed), rank, world)
        stats = c.stats()
        c.close()
        assert stats["stream_launches"] == 1, (rank, stats)
        for lt, t in enumerate(range(rank, ntiles, world)):
            x0, y0 = (t % tiles_x) * 32, (t // tiles_x) * 32
            th, tw = min(32, h - y0), min(32, w - x0)
            got = lin[lt * 1024:(lt + 1) * 1024].reshape(32, 32, 3)[:th, :tw]
            got_rgba = rgba[lt * 1024:(lt + 1) * 1024].reshape(32, 32, 4)[:th, :tw]
            assert got.tobytes() == ref[y0:y0 + th, x0:x0 + tw].tobytes(), (rank, t)
            assert got_rgba.tobytes() == ref_rgba[y0:y0 + th, x0:x0 + tw].tobytes(), (rank, t)


def test_a_sky_falls_back_to_the_block_kernel():
    loader, w, h = ("file", "sphere_reflections_light_facing.json"), 48, 32
    st = make_settings(rtgo, {"samples": 4}, 3)
    st.sky = rtgo.SKIES["white"]
    c = _Ctx(_scene(loader), STREAM)
    lin, rgba = c.one(w, h, st)
    stats = c.stats()
    c.close()
    assert stats["stream_launches"] == 0, stats
    ref, ref_rgba, _ = oracle.render(_scene(loader), w, h, st)
    assert lin.tobytes() == ref.astype(np.float32).tobytes()
    assert rgba.tobytes() == ref_rgba.tobytes()


def test_sample_passes_fall_back_to_the_block_kernel():
    """1501 samples per pixel: two sample passes (750 + 751), not streamed."""
    loader, w, h, over = ("file", "final_silver_prism_purple_cube_facing.json"), 20, 14, {"samples": 1501}
    lin, rgba, stats = _one_frame(loader, w, h, over, 6)
    assert stats["stream_launches"] == 0, stats
    _check(loader, w, h, over, 6, lin, rgba)
