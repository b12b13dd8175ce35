"""GPU: the stream kernel's refill, entry decode and single hit record.

The stream kernels decode a queue entry by multiply-high with per-launch magic
numbers, read the launch's camera constants from LDS, and fill the hit record
of both closest-hit passes once behind them.  None of that may move a bit:
every case renders with rt_tuning.stream = 1, compares float3 and RGBA8 with
the oracle byte for byte and asserts rt_context_stats.stream_launches.  The
cases sit where the loop and the decode can go wrong: waves whose lanes all go
free while the queue still holds entries, waves with fewer than 16 free lanes
for many iterations, every combination of frames, samples and entry order that
changes the decode's divisors, a progression's add, a camera sequence, a scene
with cubes (the generic kernel), wide mode in the second pass, fewer entries
than lanes and an empty queue.  Oracle images are computed once per (scene,
size, settings, seed) and shared.
"""
import functools
import json

import numpy as np
import pytest

import oracle
import rtgo
from scene_cases import all_materials_json, make_settings, scene_path
from sequence_cases import POSITIONS, at, scene_json
from test_gpu_stream import _mirror_shell
from test_gpu_stream_spheres import _sixty_four

pytestmark = pytest.mark.gpu

D50 = (("max_depth", 50),)


@functools.lru_cache(maxsize=None)
def _scene(name, cam_key=None):
    if name == "headline":
        return rtgo.Scene.load_from_file(scene_path("sphere_reflections_light_facing.json"))
    if name == "as_committed":
        return rtgo.Scene.load_from_file(scene_path("sphere_reflections_light.json"))
    if name == "shell":
        return _mirror_shell()
    if name == "all_materials":
        return rtgo.Scene.from_json_text(all_materials_json())
    if name == "sixty_four":
        return rtgo.Scene.from_json_text(json.dumps(_sixty_four()))
    return rtgo.Scene.from_json_text(scene_json(name, json.loads(cam_key) if cam_key else None))


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, over, seed, cam_key=None):
    """The oracle's (float32 linear bytes, RGBA8 bytes), computed once."""
    ref, ref_rgba, _ = oracle.render(_scene(name, cam_key), w, h, make_settings(rtgo, dict(over), seed))
    return ref.astype(np.float32).tobytes(), ref_rgba.tobytes()


def _same(got, want, what):
    assert got[0].tobytes() == want[0], what
    assert got[1].tobytes() == want[1], what


class _Ctx:
    def __init__(self, name, tun):
        self.ctx = rtgo.Context(0)
        self.ctx.set_tuning(rtgo.default_tuning(**dict(tun, stream=1)))
        self.ctx.set_scene(_scene(name))

    def _buffers(self, n, w, h):
        import torch

        self.lin = torch.full((n, w * h * 3), float("nan"), dtype=torch.float32, device="cuda")
        self.rgba = torch.zeros((n, w * h * 4), dtype=torch.uint8, device="cuda")
        return [self.lin[f].data_ptr() for f in range(n)], [self.rgba[f].data_ptr() for f in range(n)]

    def _images(self, n, w, h):
        import torch

        torch.cuda.synchronize()
        lin, rgba = self.lin.cpu().numpy().reshape(n, h, w, 3), self.rgba.cpu().numpy().reshape(n, h, w, 4)
        return [(lin[f], rgba[f]) for f in range(n)]

    def frames(self, w, h, st, seeds):
        """One launch: rt_context_render_async for one seed, else rt_context_render_frames_async."""
        lp, rp = self._buffers(len(seeds), w, h)
        if len(seeds) == 1:
            st.seed = seeds[0]
            self.ctx.render_async(w, h, st, lp[0], rp[0], 0)
        else:
            self.ctx.render_frames_async(w, h, st, list(seeds), lp, rp, 0, 0, 1, rtgo.RT_LAYOUT_IMAGE)
        return self._images(len(seeds), w, h)

    def sequence(self, w, h, st, cams):
        lp, rp = self._buffers(len(cams), w, h)
        self.ctx.render_cameras_async(w, h, st, cams, lp, rp)
        return self._images(len(cams), w, h)

    def stats(self):
        return self.ctx.stats()

    def close(self):
        self.ctx.close()


def _launch(name, w, h, over, seeds, tun):
    """One streamed launch of len(seeds) frames, every frame against the oracle."""
    c = _Ctx(name, tun)
    got = c.frames(w, h, make_settings(rtgo, dict(over), seeds[0]), seeds)
    stats = c.stats()
    c.close()
    assert stats["stream_launches"] == 1, stats
    for f, seed in enumerate(seeds):
        _same(got[f], _oracle(name, w, h, tuple(sorted(dict(over).items())), seed), (name, tun, f))
    return stats


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("chunk", [64, 4])
def test_all_lanes_free_with_entries_left(chunk, order):
    """Without the frustum test every pixel is live and most camera rays miss:
    whole waves go free again and again while the queue holds entries, and
    must refill at the top of the loop instead of leaving.  64x48x5, two
    frames (so that the two orders differ), a chunk per wave refill and a chunk
    of 4 (every refill claims twice and still leaves lanes free)."""
    w, h = 64, 48
    stats = _launch("headline", w, h, D50 + (("samples", 5),), (3, 4),
                    {"frustum": 0, "stream_chunk": chunk, "stream_order": order})
    assert stats["stream_live_pixels"] == w * h, stats


@pytest.mark.parametrize("depth", [50, 2])
def test_few_free_lanes_for_many_iterations(depth):
    """Inside the mirror shell every path runs to the depth cut-off: at depth
    50 the lanes that end are fewer than 16 for many iterations in a row (the
    second-pass refill is skipped and they wait for the top of the loop); at
    depth 2 paths end in twos and threes all the time."""
    _launch("shell", 24, 16, (("max_depth", depth), ("samples", 3)), (5,), {})
    _launch("shell", 24, 16, (("max_depth", depth), ("samples", 3)), (5, 6), {"stream_chunk": 16})


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("spp", [1, 7])
@pytest.mark.parametrize("nframes", [1, 3])
def test_decode_divisors(nframes, spp, order):
    """frames x samples x order at 40x24: each changes a divisor of the decode."""
    _launch("headline", 40, 24, D50 + (("samples", spp),), (2, 3, 4)[:nframes], {"stream_order": order})


def test_decode_of_a_progression_add():
    """Adds of 3 and 4 samples: the second add's entries carry sample_base = 3
    (the sample_base twin of the kernel); the image after it is the 7-sample one."""
    import torch

    w, h, over = 40, 24, D50 + (("samples", 7),)
    c = _Ctx("headline", {})
    lin = torch.full((w * h * 3,), float("nan"), dtype=torch.float32, device="cuda")
    rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    c.ctx.progressive_begin(w, h, make_settings(rtgo, dict(over), 2))
    for n in (3, 4):
        c.ctx.progressive_add(n, lin.data_ptr(), rgba.data_ptr(), 0)
    torch.cuda.synchronize()
    assert c.ctx.progressive_samples() == 7
    c.ctx.progressive_end()
    stats = c.stats()
    c.close()
    assert stats["stream_launches"] == 2, stats
    _same((lin.cpu().numpy(), rgba.cpu().numpy()), _oracle("headline", w, h, tuple(sorted(over)), 2), "progression")


@pytest.mark.parametrize("order", [0, 1])
def test_decode_of_a_camera_sequence(order):
    """Three frames, each from a camera of its own (the per-entry camera stays)."""
    w, h, over, seed = 40, 24, D50 + (("samples", 3),), 3
    c = _Ctx("S", {"stream_order": order})
    got = c.sequence(w, h, make_settings(rtgo, dict(over), seed), [at(p) for p in POSITIONS[:3]])
    stats = c.stats()
    c.close()
    assert stats["stream_launches"] == 1, stats
    for f, p in enumerate(POSITIONS[:3]):
        key = json.dumps(at(p), sort_keys=True)
        _same(got[f], _oracle("S", w, h, tuple(sorted(over)), seed, key), (order, f))


@pytest.mark.parametrize("order", [0, 1])
def test_decode_in_the_generic_kernel(order):
    """Spheres and cubes: the generic stream kernel, three frames."""
    _launch("all_materials", 40, 24, (("max_depth", 12), ("samples", 3)), (4, 5, 6), {"stream_order": order})


def test_wide_mode_in_the_second_pass():
    """64 spheres reach wide mode (16 lanes or fewer share a closest hit).  A
    chunk of 4 makes every second pass that narrow while the first pass's
    hitters wait for their hit record: their hit must survive the helpers."""
    _launch("sixty_four", 32, 24, D50 + (("samples", 2),), (1, 2), {"stream_chunk": 4})


def test_fewer_entries_than_lanes():
    """8x8 at one sample on the spheres-only kernel: 64 entries at most."""
    stats = _launch("headline", 8, 8, D50 + (("samples", 1),), (5,), {})
    assert 0 < stats["stream_live_pixels"] <= 64, stats


def test_an_empty_queue():
    """The as-committed scene faces away from the camera: no live pixel, no entry."""
    for seeds in ((1,), (1, 2)):
        stats = _launch("as_committed", 64, 48, D50 + (("samples", 4),), seeds, {})
        assert stats["stream_live_pixels"] == 0, stats
