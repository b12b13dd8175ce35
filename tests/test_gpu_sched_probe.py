"""The GPU work scheduler (csrc/rt_schedule.hip) against plain references, one
stage at a time (tests/sched_cases.py; the probe: tests/c/sched_probe.cpp,
built by `make probe` around the product's own rt_schedule.o and schedule.o;
DESIGN.md §2.2).

Every other GPU test of the scheduler renders an image, and the image does not
depend on how the work is cut and ordered: it cannot tell a schedule that is
valid but wrong.  Here the product's launch sequence runs on chosen inputs and
every buffer it writes is compared with the definition: the masks with camera
rays (one-sided) and with the cone test restated in binary64 (bit for bit),
the estimates in float32, the partition record by record, the live list and
the per-tile work.  Every run asserts that the 4-KiB guards behind the buffers
the kernels write came back untouched.
"""
import functools

import numpy as np
import pytest

import sched_cases as sc

pytestmark = pytest.mark.gpu

MASK_CASES = sorted(sc.all_mask_cases())
SCHED_CASES = sorted(sc.sched_cases())
RANDOM_CASES = sorted(sc.random_cases())
FIELDS = ["lt", "p0", "np", "s0", "ns", "slot", "nsub", "flags", "spheres.lo", "spheres.hi", "tris.lo", "tris.hi",
          "live.lo", "live.hi", "tile", "pad"]


@functools.cache
def _run(kind, name):
    c = {"mask": sc.all_mask_cases, "sched": sc.sched_cases, "random": sc.random_cases}[kind]()[name]
    out = sc.run(c)
    assert out["guards_written"] == 0, f"{name}: {out['guards_written']} guard regions were written"
    return c, out


def _first(bad, tiles=None):
    """tile, pixel (and field) of the first differing element"""
    i = np.argwhere(bad)[0]
    return f"local tile {i[0]}" + (f" (tile {tiles[i[0]]})" if tiles is not None else "") + \
        (f", pixel {i[1]}" if len(i) > 1 else "") + (f", field {i[2]}" if len(i) > 2 else "")


@pytest.mark.parametrize("name", MASK_CASES)
def test_pixel_masks(name):
    c, out = _run("mask", name)
    tiles, W, H = out["tiles"], c["W"], c["H"]
    want, hit = sc.expected_pixmask(c, tiles)
    got, tm = out["pixmask"], out["tile_masks"][0]
    ns, nt = len(c["spheres"]), len(c["verts"])
    # sound: what a sampled camera ray of the pixel hits is in the pixel's mask and in its tile's
    bits = np.concatenate([sc.unpack(got[..., 0], ns), sc.unpack(got[..., 1], nt)], -1)
    tbits = np.concatenate([sc.unpack(tm[:, 0], ns), sc.unpack(tm[:, 1], nt)], -1)
    bad = hit & ~bits
    assert not bad.any(), f"{name}: a ray hits a primitive cleared in the pixel's mask: {_first(bad, tiles)} (primitive)"
    bad = hit & ~tbits[:, None, :]
    assert not bad.any(), f"{name}: a ray hits a primitive cleared in the tile's mask: {_first(bad, tiles)} (primitive)"
    # within the tile's masks; zero outside the image
    bad = (got & ~tm[:, None, :]) != 0
    assert not bad.any(), f"{name}: pixel mask outside its tile's: {_first(bad, tiles)}"
    x, y, inimg = sc.local_xy(W, H, tiles)
    bad = (got != 0) & ~inimg[..., None]
    assert not bad.any(), f"{name}: a mask outside the image: {_first(bad, tiles)}"
    # equal to the definition, bit for bit
    bad = got != want
    assert not bad.any(), (f"{name}: {_first(bad, tiles)}: got {got[bad][0]:#x}, the cone test restated in binary64 "
                           f"gives {want[bad][0]:#x}")
    # the pilot's records
    pilot = sc.expected_pilot(tiles, want)
    bad = out["pilot_blocks"] != pilot
    assert not bad.any(), f"{name}: pilot record: {_first(bad, tiles)} (record, field)"
    # tightness (measured, not asserted): set bits that no sampled ray hits
    unhit = int((bits & ~hit).sum())
    print(f"tightness[{name}]: {unhit} of {int(bits.sum())} set pixel-mask bits are hit by no sampled ray "
          f"({unhit / max(1, int(bits.sum())):.4f})")


def test_masks_drop_what_no_ray_can_hit():
    """The test above cannot pass by keeping everything: the sphere behind the camera is in no pixel's mask, the
    sub-pixel spheres are in few, and a sequence's turned-away camera adds nothing."""
    for name in ("edges/reference", "edges/rolled", "edges/fisheye"):
        c, out = _run("mask", name)
        assert not sc.unpack(out["pixmask"][..., 0], 64)[..., c["dropped"]].any(), name
    c, out = _run("mask", "subpixel/reference")
    assert sc.unpack(out["pixmask"][..., 0], 64).sum() < 64 * 9
    one, two = _run("mask", "corners/seq-1")[1], _run("mask", "corners/seq-2")[1]
    assert np.array_equal(one["pixmask"], two["pixmask"]) and one["pixmask"].any()


@pytest.mark.parametrize("name", SCHED_CASES)
def test_estimates(name):
    c, out = _run("sched", name)
    want = sc.sched_reference(name)["est"]
    bad = out["est"].view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{name}: {_first(bad, out['tiles'])}: est {out['est'][bad][0]!r}, float32 restatement {want[bad][0]!r}"


def _class_ranges(records):
    hist = np.bincount([k for k, _ in records], minlength=sc.BUCKETS)
    return hist, np.concatenate([[0], np.cumsum(hist)])


def _canon(rows):
    """records as sorted tuples, a split slot reduced to 'has one' (the slots are checked as a bijection)"""
    r = np.array(rows, np.int64).reshape(-1, 16)
    r[:, 5] = np.where(r[:, 5] >= 0, 0, -1)
    return r[np.lexsort(r.T[::-1])]


@pytest.mark.parametrize("name", SCHED_CASES)
def test_blocks(name):
    c, out = _run("sched", name)
    ref = sc.sched_reference(name)
    B = ref["blocks"]
    hist, ends = _class_ranges(B["records"])
    tot = out["totals"]
    assert (tot[0], tot[1], tot[2]) == (len(B["records"]), B["nsplit"], B["nsplit"]), \
        f"{name}: totals {tot[:3]}, reference blocks {len(B['records'])}, split pixels {B['nsplit']}"
    bad = out["hist"] != hist
    assert not bad.any(), f"{name}: class {np.flatnonzero(bad)[0]}: {out['hist'][bad][0]} blocks, reference {hist[bad][0]}"
    bad = out["cursor"] != ends[1:]
    assert not bad.any(), f"{name}: cursor of class {np.flatnonzero(bad)[0]} after pass 2"
    got = out["blocks"]
    for k in np.flatnonzero(hist):
        a = _canon(got[ends[k]:ends[k + 1]])
        b = _canon([r for kk, r in B["records"] if kk == k])
        bad = a != b
        if bad.any():
            i, f = np.argwhere(bad)[0]
            raise AssertionError(f"{name}: class {k}: record of local tile {a[i, 0]}, pixel {a[i, 1]}, field "
                                 f"{FIELDS[f]}: {a[i, f]}, reference (tile {b[i, 0]}, pixel {b[i, 1]}) {b[i, f]}")
    # split slots: one per split pixel, shared by its sub-blocks, onto 0 .. nsplit - 1
    sp = got[got[:, 5] >= 0]
    slots = {}
    for r in sp:
        assert slots.setdefault((r[0], r[1]), r[5]) == r[5], f"{name}: tile {r[0]} pixel {r[1]}: two slots"
    assert sorted(slots.values()) == list(range(B["nsplit"])), f"{name}: split slots are no bijection"
    why = sc.block_properties(c, got, ref["est"], out["tiles"], ref["tile_masks"])
    assert why is None, f"{name}: {why}"


@pytest.mark.parametrize("name", RANDOM_CASES)
def test_block_properties_of_inexact_sums(name):
    c, out = _run("random", name)
    est = sc.est_reference(c, len(out["tiles"]))
    bad = out["est"].view(np.uint32) != est.view(np.uint32)
    assert not bad.any(), f"{name}: est: {_first(bad, out['tiles'])}"
    why = sc.block_properties(c, out["blocks"], est, out["tiles"], None)
    assert why is None, f"{name}: {why}"
    assert out["totals"][0] == len(out["blocks"]) == out["hist"].sum()
    assert out["totals"][1] == out["totals"][2] == len({(r[0], r[1]) for r in out["blocks"] if r[5] >= 0})


def _check_live(name, c, out, live, est):
    tiles, W = out["tiles"], c["W"]
    x, y, _ = sc.local_xy(W, c["H"], tiles)
    n = int(live.sum())
    assert out["totals"][3] == n == len(out["live"]), f"{name}: totals[3] {out['totals'][3]}, live pixels {n}"
    items = out["live"]
    idx = items[:, 3]
    assert ((idx >= 0) & (idx < live.size)).all(), f"{name}: a live item outside the rank's pixels"
    assert len(np.unique(idx)) == n and live.reshape(-1)[idx].all(), f"{name}: the list is not the set of live pixels"
    want = np.stack([x.reshape(-1)[idx], y.reshape(-1)[idx], y.reshape(-1)[idx] * W + x.reshape(-1)[idx], idx], 1)
    bad = items != want
    assert not bad.any(), f"{name}: live item {np.argwhere(bad)[0][0]}, field {np.argwhere(bad)[0][1]}"
    pos = np.full(live.size, -1, np.int32)
    pos[idx] = np.arange(n)
    bad = out["live_pos"].reshape(-1) != pos
    assert not bad.any(), f"{name}: live_pos of local pixel {np.flatnonzero(bad)[0]}"
    cls = np.array([sc.weight_class(float(abs(e)) * 64.0)[0] for e in est.reshape(-1)[idx]], np.int64)
    assert (np.diff(cls) >= 0).all(), f"{name}: list position {np.flatnonzero(np.diff(cls) < 0)[0] + 1}: a heavier class"
    assert np.array_equal(out["live_hist"], np.bincount(cls, minlength=sc.BUCKETS)), f"{name}: live class counts"


@pytest.mark.parametrize("name", SCHED_CASES)
def test_live_list(name):
    c, out = _run("sched", name)
    ref = sc.sched_reference(name)
    _check_live(name, c, out, ref["live"], ref["est"])


@pytest.mark.parametrize("name", MASK_CASES)
def test_live_list_of_culled_frames(name):
    c, out = _run("mask", name)
    want, _ = sc.expected_pixmask(c, out["tiles"])
    _, _, inimg = sc.local_xy(c["W"], c["H"], out["tiles"])
    culled = c["frustum"] or c.get("active") is not None
    live = inimg & ((want[..., 0] | want[..., 1]) != 0) if culled else inimg
    _check_live(name, c, out, live, np.zeros(live.shape, np.float32))  # (no work measured, no cost: every estimate 0)
    assert not out["est"].any()


def test_live_list_may_be_empty():
    c, out = _run("sched", "blocks/no-live-pixel")
    assert out["totals"][3] == 0 and (out["live_pos"] == -1).all()


@pytest.mark.parametrize("name", [n for n in SCHED_CASES if sc.sched_cases()[n].get("active") is None])
def test_tile_work(name):
    c, out = _run("sched", name)
    want = sc.sched_reference(name)["tile_work"]
    bad = out["tile_work"].view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{name}: {_first(bad, out['tiles'])}: {out['tile_work'][bad][0]!r}, reference {want[bad][0]!r}"


def test_the_probe_refuses_what_prepare_schedule_cannot_produce():
    """-1 and no launch: sizes, counts and array lengths outside what the product's host code makes."""
    base = sc.sched_cases()["blocks/all-zero"]
    for change in ({"spp": 0}, {"spp": 1025}, {"big_pixels": 0}, {"big_pixels": 65}, {"split_samples": 65},
                   {"block_work": 0.5}, {"block_work": float("nan")}, {"W": 0}, {"W": 32 * 17},
                   {"tile_cost": np.zeros(2, np.float32)}, {"tile_list": [1]}, {"rank": 1},
                   {"work_max": np.zeros(1024, np.uint32)},
                   {"tile_masks": np.array([[1, 0]], np.uint64)}):  # (a mask bit without its sphere)
        with pytest.raises(AssertionError, match=r"rtp_sched_run\(.*\): -1"):
            sc.run(dict(base, **change))
