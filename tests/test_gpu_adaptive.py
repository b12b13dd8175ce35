"""GPU: adaptive sampling stops every pixel of a progression
on its own, without changing a single bit of what it has rendered.

The random streams are keyed by (seed, pixel, sample) and a pixel's sum is
continued in sample order, so a pixel stopped after n samples is pixel p of
the oracle's render with samples = n, byte for byte; and the stop rule reads
the displayed RGBA8 previews only, so the oracle also predicts which pixel
stops when.  A numpy model simulates the rule from the oracle's images at the
cumulative sample counts (computed once per sample count and shared), and
AFTER EVERY ADD each case checks (a) the count map against the model's, (b)
rt_context_progressive_state against the model (in-image pixels, active
pixels, sum of counts) and (c) the float32 linear image and the RGBA8 image
of every pixel against the oracle's at samples = count[p], byte for byte.

Every case first asserts on the model alone that it is not trivial: once the
first pixels can stop there are both stopped and active pixels, and at least
three distinct count values occur.  (The first add at which the rule can stop
a pixel is add patience + 1 -- the first add has no earlier image -- which is
the second add for the rows with patience 1 and the third for the row with
patience 2, whose second add provably leaves every pixel active.)  The rows
and their active counts after each add were simulated with the CPU oracle,
seed 3, default settings otherwise; the model must reproduce them.
"""
import copy
import functools
import json

import numpy as np
import pytest

import oracle
import rtgo
from scene_cases import ALL_MATERIALS, scene_path

pytestmark = pytest.mark.gpu

SEED = 3
ALLM, ALLM_SPHERES, SILVER = "all_materials", "all_materials_spheres", "silver"

# (scene, W, H, pass, cap, tolerance, patience, min_samples, active pixels after each add (a prefix))
ROW_A = (ALLM, 64, 48, 2, 16, 1, 1, 4, (3072, 262, 200, 146, 108, 82, 60, 48))
ROW_B = (ALLM, 37, 29, 3, 15, 2, 1, 3, (1073, 109, 69, 45, 32))
ROW_C = (ALLM, 64, 48, 2, 16, 0, 2, 2, (3072, 3072, 579, 483))
ROW_SA = (ALLM_SPHERES, 64, 48, 2, 16, 1, 1, 4, (3072, 257, 191, 137, 100, 80, 61, 51))
ROW_SB = (ALLM_SPHERES, 37, 29, 3, 15, 2, 1, 3, (1073, 102, 65, 45, 32))
ROW_SILVER = (SILVER, 64, 48, 2, 16, 1, 1, 4, (3072, 11, 9, 5, 3, 2, 0))

_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        if name == ALLM:
            _SCENES[name] = rtgo.Scene.from_json_text(json.dumps(ALL_MATERIALS))
        elif name == ALLM_SPHERES:  # (a BVH takes spheres only)
            d = copy.deepcopy(ALL_MATERIALS)
            d["objects"] = [o for o in d["objects"] if o["type"] == "sphere"]
            _SCENES[name] = rtgo.Scene.from_json_text(json.dumps(d))
        else:
            _SCENES[name] = rtgo.Scene.load_from_file(scene_path("final_silver_prism_purple_cube_facing.json"))
    return _SCENES[name]


def _settings(spp, **over):
    st = rtgo.default_settings()
    st.seed = SEED
    st.samples = spp
    for k, v in over.items():
        setattr(st, k, v)
    return st


@functools.lru_cache(maxsize=None)
def _oracle(name, w, h, spp):
    """The oracle's (float32 linear (H,W,3), RGBA8 (H,W,4)) at `spp` samples, computed once."""
    ref, ref_rgba, _ = oracle.render(_scene(name), w, h, _settings(spp))
    return ref.astype(np.float32), ref_rgba


@functools.lru_cache(maxsize=None)
def _model(name, w, h, pas, cap, tol, pat, mn):
    """The rule simulated from the oracle's previews: per add, the count map, the active mask after it and
    the number of pixels active before it."""
    count = np.zeros((h, w), np.int64)
    streak = np.zeros((h, w), np.int64)
    active = np.ones((h, w), bool)
    old = np.zeros((h, w, 4), np.int64)
    steps, done = [], 0
    while done < cap:
        n = min(pas, cap - done)
        before = int(active.sum())
        done += n
        new = _oracle(name, w, h, done)[1].astype(np.int64)
        count[active] = done  # (every active pixel has every sample so far)
        if done - n > 0:
            d = np.abs(new - old).max(axis=2)
            streak = np.where(active, np.where(d <= tol, streak + 1, 0), streak)
        old[active] = new[active]
        active = active & ~((streak >= pat) & (count >= mn))
        steps.append({"counts": count.copy(), "active": active.copy(), "before": before, "done": done})
    return steps


def _guard(row):
    """The model reproduces the simulated row and is not trivial (nothing of the GPU is looked at)."""
    name, w, h, pas, cap, tol, pat, mn, table = row
    steps = _model(name, w, h, pas, cap, tol, pat, mn)
    got = [int(s["active"].sum()) for s in steps]
    assert tuple(got[:len(table)]) == table, got
    first = steps[pat]  # after add patience + 1: the first add at which a pixel can stop
    assert first["active"].any() and (~first["active"]).any(), got
    assert len(np.unique(steps[-1]["counts"])) >= 3
    return steps


def _expected(name, w, h, counts):
    """Pixel p of the oracle's render with samples = counts[p]."""
    lin = np.zeros((h, w, 3), np.float32)
    rgba = np.zeros((h, w, 4), np.uint8)
    for c in np.unique(counts):
        m = counts == c
        o_lin, o_rgba = _oracle(name, w, h, int(c))
        lin[m] = o_lin[m]
        rgba[m] = o_rgba[m]
    return lin, rgba


def _rank_mask(w, h, rank, world):
    """The image pixels of the tiles t % world == rank."""
    tx = (w + 31) // 32
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy // 32) * tx + xx // 32) % world == rank


def _scatter(packed, w, h, rank, world, out):
    """A packed share ([local tile][32 * 32] rows) into the (H, W, ...) image `out`."""
    tx, nt = (w + 31) // 32, rtgo.num_tiles(w, h)
    for lt, t in enumerate(range(rank, nt, world)):
        x0, y0 = (t % tx) * 32, (t // tx) * 32
        tile = packed[lt * 1024:(lt + 1) * 1024].reshape((32, 32) + packed.shape[1:])
        hh, ww = min(32, h - y0), min(32, w - x0)
        out[y0:y0 + hh, x0:x0 + ww] = tile[:hh, :ww]


class _AProg:
    """One rt_context with a scene; begin() starts an (adaptive) progression into buffers of its own; add()
    returns the images, the count map (all as (H, W, ...) arrays: a packed share is scattered into a zeroed
    image) and the state after the add."""

    def __init__(self, scene, tun=None, force_bvh=0):
        self.ctx = rtgo.Context(0)
        if tun is not None:
            self.ctx.set_tuning(rtgo.default_tuning(**tun))
        self.ctx.set_scene(scene, force_bvh=force_bvh)

    def begin(self, w, h, st, adaptive=None, rank=0, world=1):
        import torch

        self.w, self.h, self.rank, self.world = w, h, rank, world
        if world > 1:
            self.npx = rtgo.max_local_tiles(w, h, world) * 1024
            layout = rtgo.RT_LAYOUT_PACKED_TILES
        else:
            self.npx = w * h
            layout = rtgo.RT_LAYOUT_IMAGE
        self.lin = torch.full((self.npx * 3,), float("nan"), dtype=torch.float32, device="cuda")
        self.rgba = torch.zeros(self.npx * 4, dtype=torch.uint8, device="cuda")
        self.cnt = torch.full((self.npx,), -1, dtype=torch.int32, device="cuda")
        self.ctx.progressive_begin(w, h, st, rank, world, layout)
        if adaptive is not None:
            self.ctx.progressive_set_adaptive(*adaptive)

    def add(self, n):
        import torch

        self.ctx.progressive_add(n, self.lin.data_ptr(), self.rgba.data_ptr(), 0)
        self.ctx.progressive_counts(self.cnt.data_ptr(), 0)
        torch.cuda.synchronize()
        state = self.ctx.progressive_state()
        lin = self.lin.cpu().numpy().reshape(-1, 3)
        rgba = self.rgba.cpu().numpy().reshape(-1, 4)
        cnt = self.cnt.cpu().numpy().astype(np.int64)
        if self.world > 1:
            o_lin = np.zeros((self.h, self.w, 3), np.float32)
            o_rgba = np.zeros((self.h, self.w, 4), np.uint8)
            o_cnt = np.zeros((self.h, self.w), np.int64)
            for src, dst in ((lin, o_lin), (rgba, o_rgba), (cnt, o_cnt)):
                _scatter(src, self.w, self.h, self.rank, self.world, dst)
            return o_lin, o_rgba, o_cnt, state
        return lin.reshape(self.h, self.w, 3), rgba.reshape(self.h, self.w, 4), cnt.reshape(self.h, self.w), state

    def stats(self):
        return self.ctx.stats()

    def close(self):
        self.ctx.close()


def _check_add(row, step, k, lin, rgba, cnt, state, mask=None, what=None):
    """(a), (b) and (c) of the module docstring for add k (0-based), on the pixels of `mask` (a rank's)."""
    name, w, h = row[:3]
    m = np.ones((h, w), bool) if mask is None else mask
    want = np.where(m, step["counts"], 0)
    assert np.array_equal(cnt, want), (what, k, int((cnt != want).sum()))
    assert state == {"pixels": int(m.sum()), "active": int((step["active"] & m).sum()),
                     "samples": int(want.sum()), "adds": k + 1}, (what, k, state)
    e_lin, e_rgba = _expected(name, w, h, step["counts"])
    assert lin[m].tobytes() == e_lin[m].tobytes(), (what, k)
    assert rgba[m].tobytes() == e_rgba[m].tobytes(), (what, k)


def _run(row, tun=None, force_bvh=0, on_add=None):
    """The row's whole progression on a fresh context, checked after every add; returns the _AProg."""
    name, w, h, pas, cap, tol, pat, mn, _ = row
    steps = _guard(row)
    p = _AProg(_scene(name), tun, force_bvh)
    p.begin(w, h, _settings(cap), (tol, pat, mn))
    for k, step in enumerate(steps):
        lin, rgba, cnt, state = p.add(min(pas, cap - k * pas))
        _check_add(row, step, k, lin, rgba, cnt, state, what=tun)
        assert p.ctx.progressive_samples() == step["done"]
        if on_add is not None:
            on_add(p, k, step)
    return p


# ---------------------------------------------------------------- 1. the linear-scan paths
TUNINGS = [("block_kernel", {"stream": 0}), ("unstaged", {"stage": 0}), ("no_frustum", {"frustum": 0}),
           ("stream", {"stream": 1})]


@pytest.mark.parametrize("row", [ROW_A, ROW_B, ROW_C], ids=["64x48_tol1", "37x29_tol2", "64x48_patience2"])
@pytest.mark.parametrize("name,tun", TUNINGS, ids=[t[0] for t in TUNINGS])
def test_all_materials_on_every_linear_scan_path(row, name, tun):
    p = _run(row, tun)
    s = p.stats()
    p.close()
    if name == "stream":
        assert s["stream_launches"] > 0, s
    else:
        assert s["stream_launches"] == 0, s


# ---------------------------------------------------------------- 2. BVH scenes
@pytest.mark.parametrize("row", [ROW_SA, ROW_SB], ids=["64x48_tol1", "37x29_tol2"])
@pytest.mark.parametrize("name,tun", [("wavefront", None), ("megakernel", {"path": rtgo.RT_PATH_MEGAKERNEL})],
                         ids=["wavefront", "megakernel"])
def test_spheres_only_with_a_bvh(row, name, tun):
    _run(row, tun, force_bvh=1).close()


# ---------------------------------------------------------------- 3. every pixel stops
def test_silver_scene_stops_completely():
    """Triangles, block kernel.  Every pixel has stopped after 14 samples: the eighth add renders nothing
    (no launch), reports no active pixel and still writes the same image."""
    seen = {}

    def on_add(p, k, step):
        import torch

        seen[k] = (p.stats()["launches"], p.rgba.cpu().numpy().copy(), p.lin.cpu().numpy().copy(),
                   int(step["active"].sum()))
        if k == 6:  # (the eighth add must write its image itself: wipe the buffers before it)
            p.lin.fill_(float("nan"))
            p.rgba.zero_()
            torch.cuda.synchronize()

    p = _run(ROW_SILVER, {"stream": 0}, on_add=on_add)
    p.close()
    assert seen[6][3] == 0 and seen[7][3] == 0
    assert seen[7][0] == seen[6][0] and seen[6][0] == seen[5][0] + 1  # launches: the eighth add made none
    assert seen[7][1].tobytes() == seen[6][1].tobytes() and seen[7][2].tobytes() == seen[6][2].tobytes()


# ---------------------------------------------------------------- 4. packed shares
def test_packed_shares_of_three_ranks_equal_one_rank():
    """world = 3, each rank a progression of its own on device 0 (row A): images and counts reassembled
    from the packed shares equal the model, which the one-rank progression equals too (test 1)."""
    row = ROW_A
    name, w, h, pas, cap, tol, pat, mn, _ = row
    steps = _guard(row)
    world = 3
    progs = [_AProg(_scene(name), {"stream": 0}) for _ in range(world)]
    for r, p in enumerate(progs):
        p.begin(w, h, _settings(cap), (tol, pat, mn), rank=r, world=world)
    for k, step in enumerate(steps):
        whole_cnt = np.zeros((h, w), np.int64)
        whole_rgba = np.zeros((h, w, 4), np.uint8)
        for r, p in enumerate(progs):
            lin, rgba, cnt, state = p.add(min(pas, cap - k * pas))
            m = _rank_mask(w, h, r, world)
            _check_add(row, step, k, lin, rgba, cnt, state, mask=m, what=("rank", r))
            whole_cnt += cnt
            whole_rgba += rgba
        assert np.array_equal(whole_cnt, step["counts"])
        assert whole_rgba.tobytes() == _expected(name, w, h, step["counts"])[1].tobytes()
    for p in progs:
        p.close()


# ---------------------------------------------------------------- 5. stopped pixels are not traced
def test_stopped_pixels_leave_the_stream_queue_and_the_blocks():
    live, blocks = [], []
    p = _run(ROW_A, {"stream": 1}, on_add=lambda p, k, step: live.append((p.stats()["stream_live_pixels"],
                                                                           step["before"])))
    p.close()
    assert all(0 <= n <= before for n, before in live), live
    assert live[2][0] < live[0][0], live
    p = _run(ROW_A, {"stream": 0}, on_add=lambda p, k, step: blocks.append(p.stats()["blocks"]))
    p.close()
    assert all(b <= a for a, b in zip(blocks, blocks[1:])), blocks
    assert blocks[-1] < blocks[0], blocks


# ---------------------------------------------------------------- 6. a patience never reached
def test_patience_1000_never_stops_a_pixel():
    name, w, h, pas, cap = ALLM, 64, 48, 2, 16
    p = _AProg(_scene(name), {"stream": 0})
    p.begin(w, h, _settings(cap), (1, 1000, 0))
    for k in range(cap // pas):
        lin, rgba, cnt, state = p.add(pas)
        done = (k + 1) * pas
        ref, ref_rgba = _oracle(name, w, h, done)
        assert lin.tobytes() == ref.tobytes() and rgba.tobytes() == ref_rgba.tobytes(), done
        assert np.array_equal(cnt, np.full((h, w), done))
        assert state == {"pixels": w * h, "active": w * h, "samples": w * h * done, "adds": k + 1}
    p.close()


# ---------------------------------------------------------------- 7. ordinary renders in between
@pytest.mark.parametrize("tun", [{"stream": 0}, {"stream": 1}], ids=["block_kernel", "stream"])
def test_ordinary_renders_between_adaptive_adds(tun):
    """After the third add: a render of another sample count and one of the pass's count.  Each equals its
    oracle image (it did not pick up the active set) and the progression goes on matching the model."""
    import torch

    name, w, h, pas = ROW_A[:4]

    def on_add(p, k, step):
        if k != 2:
            return
        for spp in (5, pas):
            lin = torch.full((w * h * 3,), float("nan"), dtype=torch.float32, device="cuda")
            rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
            p.ctx.render_async(w, h, _settings(spp), lin.data_ptr(), rgba.data_ptr(), 0)
            torch.cuda.synchronize()
            ref, ref_rgba = _oracle(name, w, h, spp)
            assert lin.cpu().numpy().tobytes() == ref.tobytes(), spp
            assert rgba.cpu().numpy().tobytes() == ref_rgba.tobytes(), spp

    _run(ROW_A, tun, on_add=on_add).close()


# ---------------------------------------------------------------- 8. errors
def test_errors_and_resets():
    import torch

    name, w, h = ALLM, 64, 48
    p = _AProg(_scene(name), {"stream": 0})
    lib = rtgo.lib()

    def refused(f, *a):
        with pytest.raises(rtgo.RenderError) as e:
            f(*a)
        assert "librtgo error -1" in str(e.value) and len(str(e.value)) > len("librtgo error -1: "), str(e.value)

    refused(p.ctx.progressive_set_adaptive, 1, 1, 0)  # no progression
    refused(p.ctx.progressive_state)
    p.begin(w, h, _settings(16))
    for bad in ((-1, 1, 0), (256, 1, 0), (1, 0, 0), (1, 1, -1)):
        refused(p.ctx.progressive_set_adaptive, *bad)
    p.ctx.progressive_set_adaptive(255, 1, 0)
    p.ctx.progressive_set_adaptive(None)  # off again, then on: both before the first add
    p.ctx.progressive_set_adaptive(255, 1, 0)
    _, _, cnt, state = p.add(2)
    assert state["active"] == w * h and int(cnt.min()) == 2
    refused(p.ctx.progressive_set_adaptive, 1, 1, 0)  # after the first add
    refused(p.ctx.progressive_set_adaptive, None)
    _, _, cnt, state = p.add(2)  # (tolerance 255: every pixel stops at its second add)
    assert state == {"pixels": w * h, "active": 0, "samples": 4 * w * h, "adds": 2}
    # begin again: adaptive is off
    p.begin(w, h, _settings(16))
    for k in range(3):
        lin, rgba, cnt, state = p.add(2)
        ref, ref_rgba = _oracle(name, w, h, 2 * (k + 1))
        assert lin.tobytes() == ref.tobytes() and rgba.tobytes() == ref_rgba.tobytes()
        assert state == {"pixels": w * h, "active": w * h, "samples": 2 * (k + 1) * w * h, "adds": k + 1}
        assert np.array_equal(cnt, np.full((h, w), 2 * (k + 1)))
    # a sky is refused
    p.begin(w, h, _settings(16, sky=rtgo.SKIES["default"]))
    refused(p.ctx.progressive_set_adaptive, 1, 1, 0)
    # set_scene ends the progression
    p.begin(w, h, _settings(16), (1, 1, 4))
    p.add(2)
    p.ctx.set_scene(_scene(name))
    refused(p.ctx.progressive_state)
    refused(p.ctx.progressive_counts, p.cnt.data_ptr(), 0)
    assert lib.rt_context_progressive_samples(p.ctx._h) == -1
    torch.cuda.synchronize()
    p.close()


# ---------------------------------------------------------------- 9. the renderer object
def test_parallel_renderer_stops_by_itself():
    row = ROW_SILVER
    name, w, h, pas, cap, tol, pat, mn, _ = row
    steps = _guard(row)
    r = rtgo.ParallelRenderer()
    r.settings.seed = SEED
    r.set_samples(cap)
    r.set_tuning(rtgo.default_tuning(stream=0))
    passes = []
    img = r.render_progressive(_scene(name), w, h, pas, adaptive={"tolerance": tol, "patience": pat, "min_samples": mn},
                               on_pass=lambda done, rgba, changed: passes.append(done))
    stop = next(k for k, s in enumerate(steps) if not s["active"].any())
    assert passes == [pas * (k + 1) for k in range(stop + 1)] and passes[-1] < cap
    assert r.last_samples == passes[-1]
    assert np.array_equal(r.last_sample_counts.astype(np.int64), steps[stop]["counts"])
    assert r.last_progressive_state == {"pixels": w * h, "active": 0, "samples": int(steps[stop]["counts"].sum()),
                                        "adds": stop + 1}
    e_lin, e_rgba = _expected(name, w, h, steps[stop]["counts"])
    assert img.tobytes() == e_rgba.tobytes() and r.last_linear.tobytes() == e_lin.tobytes()
    assert r.benchmark_data["mean_samples_per_pixel"] == steps[stop]["counts"].sum() / (w * h)
