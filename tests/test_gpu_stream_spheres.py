"""GPU: the spheres-only stream kernels do not change a bit.

A streamed launch of a scene without triangles and cubes -- every scene the
auto rule streams -- takes render_stream_sph_kernel (a progression's later
adds its sample_base twin), whose bounce code has no triangle or cube test,
mask, hit field or select.  Every image here must equal the oracle's, float3
and RGBA8, byte for byte, in batched launches of 2-4 seeds under the auto rule
and with rt_tuning.stream = 1, and every case checks
rt_context_stats.stream_launches, so none passes through the block kernel.
The scenes sit where the specialisation could go wrong: empty shadow cones,
bit 63 of the sphere mask, no light, hard shadows, no recursion, and the same
spheres with one cube, which must stay on the generic stream kernel.  (Which
kernel ran is not visible through the API: the bench's committed kernel trace
shows the dispatch.)"""
import copy
import functools
import json
import os

import numpy as np
import pytest

import oracle
import rtgo
from scene_cases import SCENES, make_settings

pytestmark = pytest.mark.gpu

TUNINGS = [("auto", {}), ("forced", {"stream": 1})]
LAMB = {"type": "lambertian", "color": [0.6, 0.5, 0.4]}


def _sph(p, r, m):
    return {"type": "sphere", "position": list(p), "radius": r, "material": m}


def _headline():
    return json.load(open(os.path.join(SCENES, "sphere_reflections_light_facing.json")))


def _one_sphere():
    """One sphere and nothing else: every shadow cone is empty (its own
    sphere is left out where the light is on the hit's side)."""
    s = _headline()
    s["objects"] = s["objects"][:1]
    return s


def _no_light():
    s = _headline()
    s["lights"] = []
    return s


def _sixty_four():
    """Exactly 64 spheres, the most a staged linear scene holds: sphere 63 is
    bit 63 of the candidate mask, and 16 or more spheres reach wide mode.  An
    8 x 8 grid whose neighbours overlap on screen and in depth (two z layers,
    radii larger than half the spacing), so the closest hit has to choose;
    sphere 63 is the large one behind them all."""
    mats = [{"type": "metal", "color": [0.8, 0.8, 0.9], "roughness": 0.1},
            {"type": "glass", "color": [0.8, 0.2, 0.2]},
            LAMB,
            {"type": "metal", "color": [0.9, 0.9, 0.1], "roughness": 0.3}]
    objs = []
    for i in range(63):
        gx, gy = i % 8, i // 8
        objs.append(_sph((gx * 0.9 - 3.15, gy * 0.7 - 2.45, -0.8 * ((gx + gy) % 2)), 0.5 + 0.02 * (i % 5), mats[i % 4]))
    objs.append(_sph((0, 0, -9), 6.0, mats[0]))
    s = _headline()
    s["objects"] = objs
    assert len(s["objects"]) == 64
    return s


def _with_cube():
    s = _headline()
    s["objects"] = s["objects"] + [{"type": "cube", "position": [1.2, -0.9, 1.5], "size": [0.8, 0.8, 0.8],
                                    "material": {"type": "metal", "color": [0.7, 0.7, 0.9], "roughness": 0.0}}]
    return s


BUILDERS = {"headline": _headline, "one_sphere": _one_sphere, "no_light": _no_light, "sixty_four": _sixty_four,
            "with_cube": _with_cube}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return rtgo.Scene.from_json_text(json.dumps(copy.deepcopy(BUILDERS[name]())))


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, over, seed):
    """The oracle's (float32 linear, RGBA8) of a case, computed once."""
    ref, ref_rgba, _ = oracle.render(_scene(name), w, h, make_settings(rtgo, dict(over), seed))
    return ref.astype(np.float32), ref_rgba


def _check(name, w, h, over, seed, lin, rgba):
    ref, ref_rgba = _oracle(name, w, h, tuple(sorted(over.items())), seed)
    assert lin.tobytes() == ref.tobytes(), (name, seed)
    assert rgba.tobytes() == ref_rgba.tobytes(), (name, seed)


def _context(name, tun):
    c = rtgo.Context(0)
    c.set_tuning(rtgo.default_tuning(**tun))
    c.set_scene(_scene(name))
    return c


def _batched(name, w, h, over, seeds, tun):
    """One rt_context_render_frames_async launch of len(seeds) frames, every
    frame against the oracle; the launch must have streamed."""
    import torch

    n = len(seeds)
    lin = torch.full((n, w * h * 3), float("nan"), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((n, w * h * 4), dtype=torch.uint8, device="cuda")
    c = _context(name, tun)
    c.render_frames_async(w, h, make_settings(rtgo, over, 1), list(seeds), [lin[f].data_ptr() for f in range(n)],
                          [rgba[f].data_ptr() for f in range(n)], 0, 0, 1, rtgo.RT_LAYOUT_IMAGE)
    torch.cuda.synchronize()
    stats = c.stats()
    c.close()
    assert stats["stream_launches"] == 1 and stats["batched_launches"] == 1, stats
    lin, rgba = lin.cpu().numpy().reshape(n, h, w, 3), rgba.cpu().numpy().reshape(n, h, w, 4)
    for f, seed in enumerate(seeds):
        _check(name, w, h, over, seed, lin[f], rgba[f])
    return stats


# (id, scene, width, height, settings, seeds)
CASES = [
    # empty shadow cones everywhere
    ("one_sphere", "one_sphere", 56, 40, {"samples": 8, "max_depth": 50}, (1, 2)),
    # metal and glass scatter, two lights; 40 samples of neighbouring pixels
    # fill a wave with lit owners (soft_queue), the launch's end leaves few (soft_coop)
    ("headline_40spp", "headline", 64, 48, {"samples": 40, "max_depth": 50}, (3, 4, 5)),
    ("headline_3spp_4_seeds", "headline", 56, 40, {"samples": 3, "max_depth": 50}, (6, 7, 8, 9)),
    # bit 63, wide mode, overlapping spheres
    ("sixty_four_spheres", "sixty_four", 64, 48, {"samples": 6, "max_depth": 50}, (1, 2)),
    ("no_light", "no_light", 56, 40, {"samples": 5, "max_depth": 50}, (2, 3)),
    ("hard_shadows", "headline", 64, 48, {"samples": 8, "max_depth": 50, "soft_shadows": 0}, (4, 5)),
    ("no_recursion", "headline", 64, 48, {"samples": 8, "max_depth": 50, "recursive_reflections": 0}, (5, 6)),
]


@pytest.mark.parametrize("tname,tun", TUNINGS, ids=[t[0] for t in TUNINGS])
@pytest.mark.parametrize("cid,name,w,h,over,seeds", CASES, ids=[c[0] for c in CASES])
def test_sphere_scenes_batched(cid, name, w, h, over, seeds, tname, tun):
    stats = _batched(name, w, h, over, seeds, tun)
    if name != "no_light":
        assert stats["stream_live_pixels"] > 0, stats


def test_a_cube_keeps_the_generic_stream_kernel():
    """The headline spheres plus one cube, streamed by force (auto leaves
    triangles to the block kernel): still exact, so the dispatch sent it to the
    untouched generic instantiation (the spheres-only body has no triangle
    test and would miss the cube)."""
    over = {"samples": 8, "max_depth": 50}
    _batched("with_cube", 64, 48, over, (2, 3), {"stream": 1})
    # and under auto the same launch is not streamed at all
    import torch

    lin = torch.zeros((2, 64 * 48 * 3), dtype=torch.float32, device="cuda")
    rgba = torch.zeros((2, 64 * 48 * 4), dtype=torch.uint8, device="cuda")
    c = _context("with_cube", {})
    c.render_frames_async(64, 48, make_settings(rtgo, over, 1), [2, 3], [lin[f].data_ptr() for f in range(2)],
                          [rgba[f].data_ptr() for f in range(2)], 0, 0, 1, rtgo.RT_LAYOUT_IMAGE)
    torch.cuda.synchronize()
    stats = c.stats()
    c.close()
    assert stats["stream_launches"] == 0, stats
    for f, seed in enumerate((2, 3)):
        _check("with_cube", 64, 48, over, seed, lin[f].cpu().numpy().reshape(48, 64, 3),
               rgba[f].cpu().numpy().reshape(48, 64, 4))


def test_a_progression_of_two_adds():
    """5 then 7 samples of a sphere-only frame, streamed: the second add's
    samples start at sample_base = 5, the kBase twin of the spheres-only
    kernel; after each add the image is the oracle's at the samples so far."""
    import torch

    w, h, seed = 56, 40, 4
    lin = torch.full((w * h * 3,), float("nan"), dtype=torch.float32, device="cuda")
    rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    c = _context("headline", {"stream": 1})
    c.progressive_begin(w, h, make_settings(rtgo, {"samples": 12, "max_depth": 50}, seed), 0, 1, rtgo.RT_LAYOUT_IMAGE)
    done = 0
    for n in (5, 7):
        c.progressive_add(n, lin.data_ptr(), rgba.data_ptr(), 0)
        torch.cuda.synchronize()
        done += n
        assert c.stats()["stream_launches"] == (1 if done == 5 else 2), c.stats()
        _check("headline", w, h, {"samples": done, "max_depth": 50}, seed, lin.cpu().numpy().reshape(h, w, 3),
               rgba.cpu().numpy().reshape(h, w, 4))
    c.progressive_end()
    c.close()


def test_packed_tiles_of_two_ranks():
    """Each of two ranks' packed share (RT_LAYOUT_PACKED_TILES) of a
    sphere-only frame against the oracle's pixels of its tiles."""
    import torch

    name, w, h, over, seed, world = "headline", 96, 64, {"samples": 8, "max_depth": 50}, 2, 2
    ref, ref_rgba = _oracle(name, w, h, tuple(sorted(over.items())), seed)
    tiles_x = (w + 31) // 32
    ntiles = tiles_x * ((h + 31) // 32)
    nb, off = rtgo.packed_bytes(w, h, world), rtgo.packed_rgba_offset(w, h, world)
    for rank in range(world):
        buf = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        c = _context(name, {"stream": 1})
        c.render_async(w, h, make_settings(rtgo, over, seed), buf.data_ptr(), buf.data_ptr() + off, 0, rank, world,
                       rtgo.RT_LAYOUT_PACKED_TILES)
        torch.cuda.synchronize()
        stats = c.stats()
        c.close()
        assert stats["stream_launches"] == 1, (rank, stats)
        b = buf.cpu().numpy()
        lin, rgba = b[:off].view(np.float32).reshape(-1, 3), b[off:].reshape(-1, 4)
        for lt, t in enumerate(range(rank, ntiles, world)):
            x0, y0 = (t % tiles_x) * 32, (t // tiles_x) * 32
            th, tw = min(32, h - y0), min(32, w - x0)
            got = lin[lt * 1024:(lt + 1) * 1024].reshape(32, 32, 3)[:th, :tw]
            got_rgba = rgba[lt * 1024:(lt + 1) * 1024].reshape(32, 32, 4)[:th, :tw]
            assert got.tobytes() == ref[y0:y0 + th, x0:x0 + tw].tobytes(), (rank, t)
            assert got_rgba.tobytes() == ref_rgba[y0:y0 + th, x0:x0 + tw].tobytes(), (rank, t)
