"""The scheduler probe's cases, held to the conditions that keep its GPU tests
from being vacuous, on the references alone (tests/sched_cases.py; DESIGN.md
§2.2), and the host half of the scheduler -- tile_primary_masks of
csrc/schedule.cpp, through the probe library -- against both mask references.
No GPU.
"""
import numpy as np
import pytest

import probe_cases as pc
import sched_cases as sc

MASK_SCENES = sorted(sc.mask_cases())


def _all_tiles(c):
    return sc.tiles_of(c["W"], c["H"])


@pytest.mark.parametrize("name", MASK_SCENES)
def test_host_tile_masks_are_sound_and_equal_the_definition(name):
    c = sc.mask_cases()[name]
    ref = sc.mask_reference(name)
    tiles = _all_tiles(c)
    host = sc.host_tile_masks(c["spheres"], c["tris"], c["frames"], c["model"], c["W"], c["H"], tiles)
    # equal to the restatement, bit for bit
    ok = (host == ref["tile"]).all(1)
    assert ok.all(), f"{name}: tile {np.flatnonzero(~ok)[0]}: host {host[~ok][0]} != restated {ref['tile'][~ok][0]}"
    # sound: a primitive that a sampled ray of a pixel hits is in the pixel's tile's mask
    ns = len(c["spheres"])
    tx = (c["W"] + 31) // 32
    Y, X = np.divmod(np.arange(c["W"] * c["H"]), c["W"])
    bits = np.concatenate([sc.unpack(host[:, 0], ns), sc.unpack(host[:, 1], len(c["verts"]))], 1)
    bad = np.argwhere(ref["hit"] & ~bits[(Y // 32) * tx + X // 32])
    assert len(bad) == 0, f"{name}: pixel {bad[0][0]} is hit by primitive {bad[0][1]}, cleared in its tile's mask"
    # and so is the restated pixel mask (what the device's must equal)
    pbits = np.concatenate([sc.unpack(ref["pixel"][:, 0], ns), sc.unpack(ref["pixel"][:, 1], len(c["verts"]))], 1)
    bad = np.argwhere(ref["hit"] & ~pbits)
    assert len(bad) == 0, f"{name}: pixel {bad[0][0]} is hit by primitive {bad[0][1]}, cleared in its own mask"
    assert not (ref["pixel"] & ~ref["tile"][(Y // 32) * tx + X // 32]).any()
    # tightness (printed, recorded in DESIGN.md §2.2): set pixel-mask bits that no sampled ray hits
    print(f"tightness[{name}]: {int((pbits & ~ref['hit']).sum())} of {int(pbits.sum())} set bits unhit "
          f"({(pbits & ~ref['hit']).sum() / max(1, pbits.sum()):.4f})")


def test_the_ray_reference_is_the_oracles():
    """The vectorised Sphere.Hit / Triangle.Hit that decide the sampled rays are the oracle's, on the rays that
    matter most (through each sub-pixel sphere's centre, through the cube's corner) and a seeded sample of grid rays."""
    rng = np.random.default_rng(5)
    for name in ("subpixel/rolled-8:1", "edges/fisheye", "cubes/pitched"):
        c = sc.mask_cases()[name]
        f, W, H = c["frames"], c["W"], c["H"]
        n = 400
        px, py = rng.integers(0, W, n) + rng.choice(sc.GRID, n), rng.integers(0, H, n) + rng.choice(sc.GRID, n)
        d = sc.ray_dirs(f, W, H, px, py)
        o = np.broadcast_to(f[0:3], d.shape)
        t0, t1 = np.full(n, sc.TMIN), np.full(n, sc.INF)
        for i in range(len(c["spheres"])):
            s = c["spheres"][i]
            ok, _ = pc.oracle_sphere_batch(np.broadcast_to(s["c"], d.shape), np.full(n, s["r"]), o, d, t0, t1)
            assert np.array_equal(ok, sc._sphere_hits(c["spheres"][i:i + 1], f[0:3], d[:, None, :])[:, 0])
        for i in range(0, len(c["verts"]), 5):
            v = np.broadcast_to(c["verts"][i], (n, 3, 3))
            ok, _ = pc.oracle_tri_batch(v[:, 0], v[:, 1], v[:, 2], o, d, t0, t1)
            assert np.array_equal(ok, sc._tri_hits(c["verts"][i:i + 1], f[0:3], d[:, None, :])[:, 0])


def test_rays_the_grid_misses():
    """At least 200 (pixel, primitive) pairs are hit only by a nearest-point ray: the grid alone would not
    notice their bit cleared.  Every sub-pixel sphere is one."""
    only = 0
    for name in MASK_SCENES:
        ref = sc.mask_reference(name)
        only += int((ref["near"] & ~ref["grid"]).sum())
        c = sc.mask_cases()[name]
        if "subpixel" in c:
            pix, prim = c["subpixel"]
            assert ref["near"][pix, prim].all(), f"{name}: a sub-pixel sphere is missed by the ray through its centre"
            assert not ref["grid"][pix, prim].any(), f"{name}: a sub-pixel sphere is hit by a grid ray"
    assert only >= 200, only


def test_corner_spheres_need_four_pixels():
    for name in MASK_SCENES:
        c = sc.mask_cases()[name]
        if "corners" not in c:
            continue
        ref, W = sc.mask_reference(name), c["W"]
        xs, ys = c["corners"]
        for i, (x, y) in enumerate(zip(xs, ys)):
            four = [yy * W + xx for yy in (y - 1, y) for xx in (x - 1, x)]
            assert ref["hit"][four, i].all(), f"{name}: sphere {i} at corner ({x}, {y})"
    c = sc.mask_cases()["cubes/reference"]
    x, y = c["cube_corner"]
    hit = sc.mask_reference("cubes/reference")["hit"]
    four = [yy * c["W"] + xx for yy in (y - 1, y) for xx in (x - 1, x)]
    assert hit[four][:, :12].any(1).sum() >= 3  # the cube's corner: three of the four pixels see the cube itself


def test_stepped_edges_have_both_answers_on_both_sides():
    c = sc.mask_cases()["stepped"]
    ref = sc.mask_reference("stepped")
    W, row = c["W"], c["H"] // 2
    for X in sc.STEP_EDGES:
        fam = [i for i, m in enumerate(c["steps"]) if m[0] == X]
        assert len(fam) == len(sc.STEP_PIXELS) + len(sc.STEP_ULPS)
        for col in (X - 1, X):  # the pixel column before the edge, and the one past it
            bits = sc.unpack(ref["pixel"][row * W + col, 0:1], 64)[0][fam]
            assert bits.any() and not bits.all(), (X, col, bits)
        # the tile past a tile edge, the same
        if X % 32 == 0:
            t = (row // 32) * ((W + 31) // 32) + X // 32
            bits = sc.unpack(ref["tile"][t, 0:1], 64)[0][fam]
            assert bits.any() and not bits.all(), (X, "tile", bits)
        # the ulp steps around the edge move no bit: they are far inside the margins
        k0 = [i for i in fam if c["steps"][i][1] == 0.0]
        assert len({tuple(ref["pixel"][:, 0] >> np.uint64(i) & np.uint64(1)) for i in k0}) == 1


def test_cone_boundaries_flip_inside_their_families():
    """A margin of cone_meets_sphere that changes moves the flip: it must lie inside each family."""
    n = len(sc.BOUNDARY_STEPS)
    for name in ("boundary/reference", "boundary/rolled"):
        c = sc.mask_cases()[name]
        ref = sc.mask_reference(name)
        tile = sc.unpack(ref["tile"][0, 0:1], 64)[0][:n]                       # the first tile's cone
        x0, _, y0, _ = c["boundary"][1]
        pixel = sc.unpack(ref["pixel"][y0 * c["W"] + x0, 0:1], 64)[0][n:2 * n]  # the pixel's
        for bits in (tile, pixel):
            flips = np.flatnonzero(np.diff(bits.astype(int)))
            assert bits[0] and not bits[-1] and len(flips) == 1 and 2 <= flips[0] <= n - 4, (name, bits)


def test_dropped_and_kept_everywhere():
    for name in MASK_SCENES:
        c = sc.mask_cases()[name]
        if "dropped" not in c:
            continue
        ref = sc.mask_reference(name)
        bits = sc.unpack(ref["tile"][:, 0], 64)
        for i in c["dropped"]:
            assert not bits[:, i].any(), f"{name}: sphere {i} ({c['named'][i]}) is entirely behind the camera"
        for i in (c["named"].index("NaN centre"), c["named"].index("NaN radius"), c["named"].index("camera inside")):
            assert bits[:, i].all() and sc.unpack(ref["pixel"][:, 0], 64)[:, i].all(), (name, c["named"][i])
        # bit 63: set in some tile and clear in another
        assert bits[:, 63].any() and (not bits[:, 63].all() or len(bits) == 1), name
    e = sc.unpack(sc.mask_reference("edges/reference")["tile"][:, 0], 64)
    assert e[:, 63].any() and not e[:, 63].all()
    # the sequences' turned-away camera sees nothing in any tile
    s = sc.all_mask_cases()["corners/seq-2"]
    assert not sc.case_tile_masks(s, _all_tiles(s), host=False)[2].any()
    assert sc.case_tile_masks(s, _all_tiles(s), host=False)[1].any()


def test_mask_scenes_cover_the_frames_the_issue_names():
    cs = sc.mask_cases().values()
    assert all(len(c["spheres"]) <= 64 and len(c["tris"]) <= 64 and c["W"] <= 96 and c["H"] <= 70 for c in cs)
    assert any(c["W"] == 1 for c in cs) and any(c["H"] == 1 for c in cs) and any(c["W"] == 8 * c["H"] for c in cs)
    assert {c["model"] for c in cs} == {sc.REFERENCE, sc.LOOKAT}
    fov = [sc.CAMERAS[c["cam"]][1].get("fov") for c in cs if c["model"] == sc.LOOKAT]
    assert min(fov) == 5.0 and max(fov) == 150.0
    assert any((c["W"], c["H"]) == (96, 70) for c in cs)  # 3 x 3 tiles, partial bottom tiles
    v = sc.all_mask_cases()
    assert v["edges/tile-list"]["tile_list"] == [7, 2, 4, 0]
    act = v["edges/adaptive"]["active"]
    assert act[1].sum() == 0 and 0 < act.sum() < act.size


SCHED = sorted(sc.sched_cases())


@pytest.mark.parametrize("name", SCHED)
def test_sched_case_is_exact_and_off_the_class_boundaries(name):
    r = sc.sched_reference(name)
    assert r["blocks"]["exact"], "a prefix sum of the weights is not exact in binary64"
    assert r["tile_work_exact"]
    for w in r["blocks"]["weights"]:
        # (w == 0: log2(1) is 0 in every implementation; black records carry no weight)
        assert w is None or w == 0 or sc.weight_class(w)[1] > 1e-9, f"{name}: weight {w!r} at a class boundary"
    for e in np.unique(np.abs(r["est"][r["live"]])):
        assert e == 0 or sc.weight_class(float(e) * 64.0)[1] > 1e-9, f"{name}: live weight {e!r}"
    assert sc.block_properties(r["case"], [rec for _, rec in _ordered(r)], r["est"], r["tiles"], r["tile_masks"]) is None


def _ordered(r):
    return sorted(r["blocks"]["records"], key=lambda kr: kr[0])


def test_block_kinds_per_case():
    kinds = {name: sc.sched_reference(name)["blocks"]["kinds"] for name in SCHED}
    for name, k in kinds.items():
        print(name, k)
    assert kinds["blocks/all-zero"] == {"multi": 64, "single": 0, "split": 0, "black": 0}
    assert kinds["blocks/every-pixel-heavy"] == {"multi": 0, "single": 0, "split": 1024, "black": 0}
    k = kinds["blocks/alternating"]
    assert k["split"] == 512 and k["multi"] == 0 and k["single"] == 512
    assert kinds["blocks/heavy-at-0-and-1023"]["split"] >= 2
    assert kinds["blocks/big-pixels-1"]["multi"] == 0 and kinds["blocks/big-pixels-1"]["single"] > 0
    assert kinds["blocks/big-pixels-64"] == {"multi": 16, "single": 0, "split": 0, "black": 0}
    for ss in (1, 8, 64):
        assert kinds[f"blocks/split-{ss}-spp-1"]["split"] == 0  # one sample is never split
        for spp in (2, 63, 64, 65, 130):
            assert kinds[f"blocks/split-{ss}-spp-{spp}"]["split"] >= 3
    k = kinds["blocks/spp-1-over-block-work"]
    assert k["split"] == 0 and k["single"] > 0 and k["multi"] > 0
    assert kinds["blocks/2-tiles-one-black"]["black"] == 16 and kinds["blocks/9-tiles"]["black"] == 32
    assert kinds["blocks/9-tiles-frustum-0"]["black"] == 0 and kinds["blocks/no-live-pixel"]["black"] == 16
    assert kinds["blocks/9-tiles"]["split"] >= 2
    # the two block_work cases differ in their first block only by the ninth pixel
    a = sc.sched_reference("blocks/sum-equals-block-work")["blocks"]["records"]
    b = sc.sched_reference("blocks/sum-over-block-work")["blocks"]["records"]
    first = lambda recs: [r for _, r in recs if r[1] == 0][0]
    assert first(a)[2] == 9 and first(b)[2] == 8


def test_est_cases_reach_every_branch():
    r = sc.sched_reference("est/pilot")
    g = r["est"].reshape(2, 32, 32)
    assert (g[0, 0, :] >= 60).all() and (g[0, 1, :-2] == np.float32(60.02)).all()  # the neighbour above holds the maximum
    assert (g[0, :, 31] == np.float32(61.02)).all() and (g[1, :, 0] >= np.float32(63.02)).all()
    # ... and never across the tile's border: tile 1's column 0 (63) does not reach tile 0's column 31 (61)
    assert (g[0, 2:, 31] == np.float32(61.02)).all()
    m = sc.sched_reference("est/measured-frame")
    assert m["est"][0, 5] > 0 and m["est"][0, 6] == np.float32(-17.0) and m["est"][0, 1023] == np.float32(-40.0)
    assert sc.sched_reference("est/spp-1")["blocks"]["kinds"]["split"] == 0
    n = sc.sched_reference("est/no-pilot")["est"]
    assert (n[0] == 0).all() and (n[1] > 0).all() and (n[5] == n[4]).all() and (n[6] > n[2]).all()
    a = sc.sched_reference("est/adaptive-stopped")
    off = np.asarray(a["case"]["active"]).reshape(1, 1024) == 0
    assert off.any() and (a["est"][off] == 0).all() and (a["est"][~off] != 0).all()
    assert not np.signbit(a["est"][off]).any()


def test_random_cases_are_not_exact():
    inexact = 0
    for name, c in sc.random_cases().items():
        local = len(sc.tiles_of(c["W"], c["H"]))
        e = np.abs(sc.est_reference(c, local)).astype(np.float64) * max(c["spp"], 1)
        inexact += not all(sc._prefix_exact(e[lt]) for lt in range(local))
    assert inexact >= 15, inexact
