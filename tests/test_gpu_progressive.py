"""GPU: progressive rendering continues a frame's samples
across calls without changing a single bit.

The random streams are keyed by (seed, pixel, sample), so after adds
totalling n samples the image must be that of a render with samples = n:
the float32 linear image and the RGBA8 image are compared byte for byte with
the oracle's at the cumulative sample count AFTER EVERY ADD, on the block
kernel (every kind of block, sub-passes inside one add), the stream path, the
wavefront path, packed shares and (at the sky's own tolerance) with a sky.
Oracle images are computed once per (scene, size, settings) and shared.
"""
import ctypes
import functools
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import rtgo
import test_gpu_parity
from conftest import ROOT
from scene_cases import load_case, make_settings
from test_gpu_paths import _sphere_field
from test_gpu_schedules import SCHEDULES
from test_gpu_stream import _mirror_shell

pytestmark = pytest.mark.gpu

ALLM = ("json", None)
SPHERES = ("file", "sphere_reflections_light_facing.json")
RT_E_INVALID = -1

_SCENES = {}


def _scene(loader):
    if loader not in _SCENES:
        kind, arg = loader
        if kind == "shell":
            _SCENES[loader] = _mirror_shell()
        elif kind == "field":
            _SCENES[loader] = rtgo.Scene.from_json_text(json.dumps(_sphere_field(arg[0], seed=arg[1])))
        else:
            _SCENES[loader] = load_case(rtgo, loader)
    return _SCENES[loader]


def _settings(over, seed, spp):
    st = make_settings(rtgo, dict(over), seed)
    st.samples = spp
    return st


@functools.lru_cache(maxsize=None)
def _oracle(loader, w, h, over, seed, spp):
    """The oracle's (float32 linear (H,W,3), RGBA8 (H,W,4)) at `spp` samples, computed once."""
    ref, ref_rgba, _ = oracle.render(_scene(loader), w, h, _settings(over, seed, spp))
    return ref.astype(np.float32), ref_rgba


def _key(over):
    return tuple(sorted(over.items()))


class _Prog:
    """One rt_context with a scene; begin() starts a progression into buffers
    of its own, add() returns the images after the add as numpy arrays."""

    def __init__(self, scene, tun=None, force_bvh=0):
        self.ctx = rtgo.Context(0)
        if tun is not None:
            self.ctx.set_tuning(rtgo.default_tuning(**tun))
        self.ctx.set_scene(scene, force_bvh=force_bvh)

    def begin(self, w, h, st, rank=0, world=1):
        import torch

        self.w, self.h, self.world = w, h, world
        if world > 1:
            nb, self.off = rtgo.packed_bytes(w, h, world), rtgo.packed_rgba_offset(w, h, world)
            self.buf = torch.zeros(nb, dtype=torch.uint8, device="cuda")
            self.p_lin, self.p_rgba = self.buf.data_ptr(), self.buf.data_ptr() + self.off
            layout = rtgo.RT_LAYOUT_PACKED_TILES
        else:
            self.lin = torch.full((w * h * 3,), float("nan"), dtype=torch.float32, device="cuda")
            self.rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
            self.p_lin, self.p_rgba = self.lin.data_ptr(), self.rgba.data_ptr()
            layout = rtgo.RT_LAYOUT_IMAGE
        self.ctx.progressive_begin(w, h, st, rank, world, layout)

    def add(self, n):
        import torch

        self.ctx.progressive_add(n, self.p_lin, self.p_rgba, 0)
        torch.cuda.synchronize()
        if self.world > 1:
            b = self.buf.cpu().numpy()
            return b[:self.off].view(np.float32).reshape(-1, 3), b[self.off:].reshape(-1, 4)
        return (self.lin.cpu().numpy().reshape(self.h, self.w, 3),
                self.rgba.cpu().numpy().reshape(self.h, self.w, 4))

    def stats(self):
        return self.ctx.stats()

    def close(self):
        self.ctx.close()


def _run(loader, w, h, over, seed, adds, tun=None, cap=None, prog=None):
    """A progression of `adds` on a fresh context (or `prog`), the image checked
    against the oracle after every add; returns the _Prog (the caller closes it)."""
    p = prog or _Prog(_scene(loader), tun)
    p.begin(w, h, _settings(over, seed, cap or sum(adds)))
    done = 0
    for n in adds:
        lin, rgba = p.add(n)
        done += n
        assert p.ctx.progressive_samples() == done
        ref, ref_rgba = _oracle(loader, w, h, _key(over), seed, done)
        assert lin.tobytes() == ref.tobytes(), (done, tun)
        assert rgba.tobytes() == ref_rgba.tobytes(), (done, tun)
    return p


# ---------------------------------------------------------------- 1. block kernel
@pytest.mark.parametrize("name,tun", SCHEDULES, ids=[s[0] for s in SCHEDULES])
def test_block_kernel_every_kind_of_block(name, tun):
    """All materials, 56x40 (partial tiles on both axes), adds 1, 2, 5, 32 under
    every schedule; every_pixel_split and split_by_8 resolve split rows onto a
    carried sum."""
    p = _run(ALLM, 56, 40, {"max_depth": 12}, 4, [1, 2, 5, 32], tun=tun)
    s = p.stats()
    p.close()
    assert s["stream_launches"] == 0 and s["frames"] == 4 and s["launches"] == 4, s
    if name in ("every_pixel_split", "split_by_8"):
        assert s["split_pixels"] > 0, s  # (of the last add's schedule, 32 samples)


# ---------------------------------------------------------------- 2. sub-passes
def test_sub_passes_inside_one_add():
    """401 then 1100 samples (1501 in all): the second add holds more than a
    block does and renders as two sub-passes; only the last writes the image."""
    p = _run(("file", "final_silver_prism_purple_cube_facing.json"), 20, 14, {}, 6, [401, 1100])
    s = p.stats()
    p.close()
    assert s["frames"] == 2 and s["launches"] == 3, s


def test_sub_passes_of_an_add_never_stream():
    """The same adds with the stream path forced: the 401-sample add is one
    launch and streams; the 1100-sample add's last sub-pass has the acc_mode of
    a one-launch add, yet both of its sub-passes take the block kernel."""
    p = _run(("file", "final_silver_prism_purple_cube_facing.json"), 20, 14, {}, 6, [401, 1100], tun={"stream": 1})
    s = p.stats()
    p.close()
    assert s["frames"] == 2 and s["launches"] == 3 and s["stream_launches"] == 1, s


# ---------------------------------------------------------------- 3. stream path
def test_stream_path_continues_the_sum_and_reuses_the_schedule():
    over = {"max_depth": 12}
    p = _Prog(_scene(ALLM), {"stream": 1})
    p.begin(56, 40, _settings(over, 4, 18))
    done, built = 0, []
    for n in (3, 5, 5, 5):
        before = p.stats()["stream_launches"]
        lin, rgba = p.add(n)
        done += n
        s = p.stats()
        assert s["stream_launches"] == before + 1, (done, s)
        built.append(s["schedules_built"])
        ref, ref_rgba = _oracle(ALLM, 56, 40, _key(over), 4, done)
        assert lin.tobytes() == ref.tobytes(), done
        assert rgba.tobytes() == ref_rgba.tobytes(), done
    p.close()
    assert built[1] == built[2] == built[3], built  # equal adds share one schedule


STREAM_CASES = [
    ("long_chains", ("shell", None), 6, 4, {"max_depth": 50}, 3, [30, 40]),
    ("fewer_entries_than_lanes", ALLM, 8, 8, {}, 5, [1, 1]),
]


@pytest.mark.parametrize("name,loader,w,h,over,seed,adds", STREAM_CASES, ids=[c[0] for c in STREAM_CASES])
def test_stream_path_shapes(name, loader, w, h, over, seed, adds):
    p = _run(loader, w, h, over, seed, adds, tun={"stream": 1})
    s = p.stats()
    p.close()
    assert s["stream_launches"] == len(adds), s


def test_stream_path_without_a_live_pixel():
    """The as-committed scene: no live pixel, every add writes black."""
    loader = ("file", "sphere_reflections_light.json")
    p = _Prog(_scene(loader), {"stream": 1})
    p.begin(64, 48, _settings({}, 1, 4))
    for done in (2, 4):
        lin, rgba = p.add(2)
        assert not lin.any() and not rgba[..., :3].any() and (rgba[..., 3] == 255).all()
        ref, ref_rgba = _oracle(loader, 64, 48, (), 1, done)
        assert lin.tobytes() == ref.tobytes() and rgba.tobytes() == ref_rgba.tobytes()
    s = p.stats()
    p.close()
    assert s["stream_launches"] == 2 and s["stream_live_pixels"] == 0, s


# ---------------------------------------------------------------- 4. wavefront
@pytest.mark.parametrize("tun", [None, {"wf_paths": 128, "wf_chunk": 3000}], ids=["default", "chunks"])
def test_wavefront_path(tun):
    """A 200-sphere field (a BVH scene: the wavefront path), adds 2, 3, 2; with
    wf_chunk the frame is cut into several chunks of whole pixels."""
    _run(("field", (200, 9)), 50, 37, {}, 1, [2, 3, 2], tun=tun).close()


def test_wavefront_path_past_one_block_of_samples():
    _run(("field", (300, 5)), 16, 12, {"max_depth": 6}, 1, [500, 600]).close()


# ---------------------------------------------------------------- 5. packed shares
@pytest.mark.parametrize("tun", [None, {"stream": 1}], ids=["block", "stream"])
def test_packed_shares(tun):
    """World 2, both ranks: each rank's packed share against the oracle's
    pixels of its tiles, after each add."""
    w, h, world, seed, adds = 96, 64, 2, 2, [3, 5]
    tiles_x = (w + 31) // 32
    ntiles = tiles_x * ((h + 31) // 32)
    for rank in range(world):
        p = _Prog(_scene(SPHERES), tun)
        p.begin(w, h, _settings({}, seed, sum(adds)), rank, world)
        done = 0
        for n in adds:
            lin, rgba = p.add(n)
            done += n
            ref, ref_rgba = _oracle(SPHERES, w, h, (), seed, done)
            for lt, t in enumerate(range(rank, ntiles, world)):
                x0, y0 = (t % tiles_x) * 32, (t // tiles_x) * 32
                th, tw = min(32, h - y0), min(32, w - x0)
                got = lin[lt * 1024:(lt + 1) * 1024].reshape(32, 32, 3)[:th, :tw]
                got_rgba = rgba[lt * 1024:(lt + 1) * 1024].reshape(32, 32, 4)[:th, :tw]
                assert got.tobytes() == ref[y0:y0 + th, x0:x0 + tw].tobytes(), (rank, t, done)
                assert got_rgba.tobytes() == ref_rgba[y0:y0 + th, x0:x0 + tw].tobytes(), (rank, t, done)
        s = p.stats()
        p.close()
        assert s["stream_launches"] == (len(adds) if tun else 0), (rank, s)


# ---------------------------------------------------------------- 6. sky
def _sky_tolerance():
    """(rmse, max |d|, RGBA mismatch share) bounds of test_opt_in_sky_matches_oracle, read from it."""
    src = inspect.getsource(test_gpu_parity.test_opt_in_sky_matches_oracle)
    m = re.search(r"assert np\.all\(rmse < ([0-9.e+-]+)\) and maxd < ([0-9.e+-]+) and rgba_mis < ([0-9.e+-]+)", src)
    assert m, "the sky test's tolerance line changed"
    return tuple(float(g) for g in m.groups())


def test_sky():
    """A white sky (every camera sample counts, no culling): adds 2, 2, at
    the tolerance of test_opt_in_sky_matches_oracle (the sky's exp / pow)."""
    w, h = 48, 32
    rmse_tol, maxd_tol, mis_tol = _sky_tolerance()
    st = _settings({}, 3, 4)
    st.sky = rtgo.SKIES["white"]
    p = _Prog(_scene(SPHERES))
    p.begin(w, h, st)
    for done in (2, 4):
        lin, rgba = p.add(2)
        so = _settings({}, 3, done)
        so.sky = rtgo.SKIES["white"]
        ref, ref_rgba, _ = oracle.render(_scene(SPHERES), w, h, so)
        rmse, maxd, mis = test_gpu_parity._compare(lin.astype(np.float64), rgba, ref, ref_rgba)
        print(f"progressive sky, {done} samples: rmse={rmse} max|d|={maxd:.3e} rgba_mismatch={mis:.2e}")
        assert np.all(rmse < rmse_tol) and maxd < maxd_tol and mis < mis_tol
        assert (ref_rgba[..., :3] > 0).mean() > 0.9  # the sky is visible
    p.close()


# ---------------------------------------------------------------- 7. isolation and reuse
def test_ordinary_renders_between_adds_and_a_second_begin():
    import torch

    over, w, h = {"max_depth": 12}, 56, 40
    p = _run(ALLM, w, h, over, 4, [3], cap=7)
    # an ordinary render of more than a block's samples (it uses the context's
    # own sample-pass sums) and a 4-frame launch, on the same context
    lin = torch.zeros(8 * 8 * 3, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(8 * 8 * 4, dtype=torch.uint8, device="cuda")
    st_big = _settings(over, 9, 1030)
    p.ctx.render_async(8, 8, st_big, lin.data_ptr(), rgba.data_ptr(), 0)
    torch.cuda.synchronize()
    ref, ref_rgba = _oracle(ALLM, 8, 8, _key(over), 9, 1030)
    assert lin.cpu().numpy().tobytes() == ref.tobytes() and rgba.cpu().numpy().tobytes() == ref_rgba.tobytes()
    nf = 4
    flin = torch.zeros((nf, 24 * 16 * 3), dtype=torch.float32, device="cuda")
    p.ctx.render_frames_async(24, 16, _settings(over, 1, 2), [11, 12, 13, 14], [flin[f].data_ptr() for f in range(nf)])
    torch.cuda.synchronize()
    ref, _ = _oracle(ALLM, 24, 16, _key(over), 14, 2)
    assert flin[nf - 1].cpu().numpy().tobytes() == ref.tobytes()
    assert p.ctx.progressive_samples() == 3
    lin2, rgba2 = p.add(4)
    ref, ref_rgba = _oracle(ALLM, w, h, _key(over), 4, 7)
    assert lin2.tobytes() == ref.tobytes() and rgba2.tobytes() == ref_rgba.tobytes()
    # a second begin on the same context starts over, from sample 0
    _run(ALLM, w, h, over, 5, [2, 1], prog=p)
    p.close()


# ---------------------------------------------------------------- 8. errors
def test_errors_leave_the_progression_unchanged():
    import torch

    lib = rtgo.lib()
    scene = _scene(ALLM)
    ctx = rtgo.Context(0)
    ctx.set_scene(scene)
    w, h = 16, 8
    lin = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    rgba = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")

    def add(n):
        before = ctx.progressive_samples()
        rc = lib.rt_context_progressive_add_async(ctx._h, n, ctypes.c_void_p(lin.data_ptr()),
                                                  ctypes.c_void_p(rgba.data_ptr()), None)
        torch.cuda.synchronize()
        if rc != 0:
            assert lib.rt_last_error()
            assert ctx.progressive_samples() == before
        return rc

    assert ctx.progressive_samples() == -1
    assert add(1) == RT_E_INVALID  # before begin
    ctx.progressive_begin(w, h, _settings({"max_depth": 4}, 1, 5))
    assert ctx.progressive_samples() == 0
    assert add(0) == RT_E_INVALID and add(-3) == RT_E_INVALID
    assert add(3) == 0 and ctx.progressive_samples() == 3
    assert add(3) == RT_E_INVALID  # past the cap of 5
    assert add(2) == 0 and ctx.progressive_samples() == 5
    assert add(1) == RT_E_INVALID  # the cap is reached
    ctx.progressive_begin(w, h, _settings({"max_depth": 4}, 1, 5))
    assert add(1) == 0
    ctx.set_scene(scene)
    assert add(1) == RT_E_INVALID and ctx.progressive_samples() == -1  # set_scene ended it
    ctx.progressive_begin(w, h, _settings({"max_depth": 4}, 1, 5))
    assert add(1) == 0
    ctx.set_tuning(rtgo.default_tuning())
    assert add(1) == RT_E_INVALID  # set_tuning ended it
    ctx.progressive_begin(w, h, _settings({"max_depth": 4}, 1, 5))
    assert add(1) == 0
    ctx.progressive_end()
    assert add(1) == RT_E_INVALID and ctx.progressive_samples() == -1  # after end
    ctx.close()


# ---------------------------------------------------------------- 9. rgba_delta
def _delta(a, b):
    import torch

    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    out = torch.full((2,), 12345, dtype=torch.int32, device="cuda")  # (the call zeroes it)
    rtgo.rgba_delta_async(da.data_ptr(), db.data_ptr(), a.shape[0], out.data_ptr(), 0)
    torch.cuda.synchronize()
    return tuple(int(v) & 0xFFFFFFFF for v in out.cpu().numpy())


@pytest.mark.parametrize("npix", [1, 63, 64, 65, 4097, 2048 * 256 + 300])
def test_rgba_delta_against_numpy(npix):
    """(the last size is past the kernel's largest grid, 2048 workgroups of 256: lanes take a second step)"""
    rng = np.random.default_rng(npix)
    a = rng.integers(0, 256, (npix, 4), dtype=np.uint8)
    b = a.copy()
    change = rng.random(npix) < 0.5  # about half the pixels differ, in some of their bytes
    noise = rng.integers(0, 256, (npix, 4), dtype=np.uint8)
    b[change] = np.where(rng.random((int(change.sum()), 4)) < 0.5, noise[change], b[change])
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    assert _delta(a, b) == (int((d.max(axis=1) > 0).sum()), int(d.max()))
    assert _delta(a, a.copy()) == (0, 0)
    c = a.copy()
    c[-1, 3] = (int(c[-1, 3]) + 77) % 256  # one byte of the last pixel
    assert _delta(a, c) == (1, abs(int(a[-1, 3]) - int(c[-1, 3])))


# ---------------------------------------------------------------- 10. render_progressive
PROG = (SPHERES, 64, 48, 6, 12, 2)  # scene, size, seed, cap, pass size


def _prog_oracle():
    """The oracle's images at 2, 4, .., 12 samples and the pixels that change between consecutive ones."""
    loader, w, h, seed, cap, step = PROG
    imgs = [_oracle(loader, w, h, (), seed, n) for n in range(step, cap + 1, step)]
    changed = [int(np.any(imgs[k][1] != imgs[k - 1][1], axis=2).sum()) for k in range(1, len(imgs))]
    return imgs, changed


def _renderer(seed, cap):
    r = rtgo.ParallelRenderer()
    r.set_samples(cap)
    r.set_seed(seed)
    return r


def test_render_progressive_passes_and_previews():
    loader, w, h, seed, cap, step = PROG
    imgs, changed = _prog_oracle()
    seen = []
    r = _renderer(seed, cap)
    out = r.render_progressive(_scene(loader), w, h, step, on_pass=lambda n, img, c: seen.append((n, img.copy(), c)))
    assert [s[0] for s in seen] == list(range(step, cap + 1, step))
    assert [s[2] for s in seen] == [None] + changed
    for (n, img, _), (ref, ref_rgba) in zip(seen, imgs):
        assert img.tobytes() == ref_rgba.tobytes(), n
    assert out.tobytes() == imgs[-1][1].tobytes() and r.last_linear.tobytes() == imgs[-1][0].tobytes()
    assert r.last_samples == cap
    # a second call on the same renderer (it keeps its context)
    out = r.render_progressive(_scene(loader), w, h, 5)
    assert r.last_samples == cap and out.tobytes() == imgs[-1][1].tobytes()
    r.close()


def test_render_progressive_stop_rules():
    loader, w, h, seed, cap, step = PROG
    imgs, changed = _prog_oracle()
    r = _renderer(seed, cap)
    out = r.render_progressive(_scene(loader), w, h, step, time_budget=0)
    assert r.last_samples == step and out.tobytes() == imgs[0][1].tobytes()
    assert r.last_linear.tobytes() == imgs[0][0].tobytes()
    # the smallest count of the oracle's own sequence: the rule fires inside the cap
    thr = min(changed)
    stop = next(k for k, c in enumerate(changed) if c <= thr) + 2  # passes rendered (changed[0] is pass 2's)
    out = r.render_progressive(_scene(loader), w, h, step, until_changed_pixels=thr)
    assert r.last_samples == stop * step, (changed, thr)
    assert out.tobytes() == imgs[stop - 1][1].tobytes()
    r.close()
    with pytest.raises(rtgo.RenderError):
        rtgo.ParallelRenderer(num_devices=2).render_progressive(_scene(loader), w, h, step)


# ---------------------------------------------------------------- 11. CLI
def test_cli_progressive_equals_one_render(tmp_path):
    exe = os.path.join(ROOT, "concurrent-raytracer-go_amd", "build", "raytracer")
    scene_file = os.path.join(ROOT, "scenes", "sphere_reflections_light_facing.json")
    outs = []
    for sub, extra in (("plain", []), ("prog", ["--pass-samples", "3"])):
        d = tmp_path / sub
        d.mkdir()
        p = subprocess.run([exe, scene_file, str(d / "o.ppm"), "64", "48", "--samples", "8"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append((d, p.stdout))
    (plain, _), (prog, stdout) = outs
    assert (prog / "o.ppm").read_bytes() == (plain / "o.ppm").read_bytes()
    assert json.loads((prog / "benchmark_data.json").read_text())["samples"] == 8
    lines = [ln for ln in stdout.splitlines() if ln.startswith("Pass ")]
    assert len(lines) == 3, stdout
    assert lines[0] == "Pass 1: 3 samples" and lines[1].startswith("Pass 2: 6 samples, ")
    assert re.fullmatch(r"Pass 3: 8 samples, \d+ pixels changed", lines[2]), lines
