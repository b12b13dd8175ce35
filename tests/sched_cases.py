"""Cases and references of the scheduler probe (tests/c/sched_probe.cpp,
tests/test_gpu_sched_probe.py, tests/test_sched_cases_cpu.py).

The GPU work scheduler (csrc/rt_schedule.hip, and csrc/schedule.cpp on the
host) only cuts and orders work, so no image shows whether it does so as its
definitions say.  This module restates each stage from the kernels' header
comments and DESIGN.md §4.1 / §4.7 / §4.10 / §4.11 in plain numpy and plain
loops -- no prefix-sum, doubling or counting-sort tricks -- never from the code
under test:

  masks      two references.  The binding one is one-sided: wherever a sampled
             camera ray of a pixel hits primitive i (Sphere.Hit / Triangle.Hit
             on [0.001, +inf), the numpy restatements of probe_cases.py, which
             the CPU tests hold to oracle.sphere_hit / oracle.triangle_hit),
             bit i is set in the pixel's mask and in its tile's.  The second is
             a binary64 restatement of rect_cone / pixel_cone /
             cone_meets_sphere in the code's operation order, which the masks
             equal bit for bit; it is what makes the tightness figure (set bits
             that no sampled ray hits) mean something.
  sched_est  its three branches in float32
  blocks     the greedy partition, per tile, with exact binary64 prefix sums
  live       the live-pixel list
  tile_work  (float)(max(spp, 1) * sum |est|) over a tile's image pixels

A case is a dict; a reference is computed once per process (functools.cache on
the case's name).
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np

import oracle
import probe_cases as pc
import rtgo

INF = float("inf")
NAN = float("nan")
TMIN = 0.001
LAST = 1.0 - 2.0 ** -32  # the largest jitter draw
REFERENCE, LOOKAT = 0, 1
KBLOCK_BLACK = 1
BUCKETS = 128
U64 = np.uint64


# =============================================================== the probe's entry points
class SchedArgs(ctypes.Structure):
    _fields_ = (
        [(n, ctypes.c_int32) for n in ("W", "H", "rank", "world", "spp", "big_pixels", "frustum", "split_samples",
                                       "split_depth", "work_n", "work_mean", "own_masks", "ncams", "model",
                                       "want_tile_work", "want_live")]
        + [("block_work", ctypes.c_double)]
        + [(n, ctypes.c_void_p) for n in ("frames", "spheres", "tris")]
        + [("ns", ctypes.c_int64), ("nt", ctypes.c_int64)]
        + [(n, ctypes.c_void_p) for n in ("tile_list", "tile_masks", "tile_cost", "work_max", "work_sum", "active")]
        + [(n, ctypes.c_int64) for n in ("n_tile_list", "n_tile_masks", "n_tile_cost", "n_work_max", "n_work_sum",
                                         "n_active")]
        + [(n, ctypes.c_void_p) for n in ("pixmask", "est", "pilot_blocks", "hist", "cursor", "totals", "blocks",
                                          "live_hist", "live_cursor", "live", "live_pos", "tile_work")]
        + [("cap_blocks", ctypes.c_int64), ("guards_written", ctypes.c_int32), ("local", ctypes.c_int32)])


@functools.cache
def sched_lib():
    L = pc.probe_lib()
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.rtp_flat_from_records.restype = vp
    L.rtp_flat_from_records.argtypes = [vp, i64, vp, i64]
    L.rtp_sched_tile_masks.restype = i32
    L.rtp_sched_tile_masks.argtypes = [vp, vp, i32, i32, i32, vp, i64, vp]
    L.rtp_sched_run.restype = i32
    L.rtp_sched_run.argtypes = [ctypes.POINTER(SchedArgs)]
    return L


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def host_tile_masks(spheres, tris, frame, model, W, H, tiles):
    """tile_primary_masks of the host (schedule.cpp): (len(tiles), 2) uint64.  No GPU."""
    L = sched_lib()
    h = L.rtp_flat_from_records(_ptr(spheres), len(spheres), _ptr(tris), len(tris))
    assert h, "rtp_flat_from_records refused the records"
    try:
        tl = np.ascontiguousarray(tiles, np.int32)
        out = np.zeros((len(tl), 2), U64)
        fr = np.ascontiguousarray(frame, np.float64)
        rc = L.rtp_sched_tile_masks(h, fr.ctypes.data, model, W, H, tl.ctypes.data, len(tl), out.ctypes.data)
        assert rc == 0, f"rtp_sched_tile_masks: {rc}"
    finally:
        L.rtp_free(h)
    return out


def tiles_of(W, H, rank=0, world=1, tile_list=None):
    """The rank's global tiles in local order (strided_tiles, or a partition's list)."""
    if tile_list is not None:
        return np.asarray(tile_list, np.int32)
    nt = ((W + 31) // 32) * ((H + 31) // 32)
    return np.arange(rank, nt, world, dtype=np.int32)


def local_xy(W, H, tiles):
    """Per local pixel (lt, q): image x, y and whether it is an image pixel."""
    tx = (W + 31) // 32
    q = np.arange(1024)
    x = (np.asarray(tiles)[:, None] % tx) * 32 + (q & 31)[None, :]
    y = (np.asarray(tiles)[:, None] // tx) * 32 + (q >> 5)[None, :]
    return x, y, (x < W) & (y < H)


def run(c, tile_masks="host", want_live=True, want_tile_work=None, cap_blocks=None):
    """rtp_sched_run of case `c` on the GPU: a dict of the arrays it copies back.
    tile_masks: "host" (the product's tile_primary_masks, per camera for a sequence, as
    prepare_schedule feeds them), None, or an explicit array."""
    L = sched_lib()
    W, H = c["W"], c["H"]
    tiles = tiles_of(W, H, c.get("rank", 0), c.get("world", 1), c.get("tile_list"))
    local = len(tiles)
    npx = local * 1024
    spheres = np.ascontiguousarray(c.get("spheres", np.zeros(0, pc.SPHERE_DT)))
    tris = np.ascontiguousarray(c.get("tris", np.zeros(0, pc.TRI_DT)))
    frames = np.ascontiguousarray(c["frames"], np.float64).reshape(-1, 12)
    ncams = c.get("ncams", 0)
    assert len(frames) == max(ncams, 1)
    if isinstance(tile_masks, str):  # (a case without geometry has no masks: no primary culling)
        tile_masks = (c["tile_masks"] if "tile_masks" in c else
                      case_tile_masks(c, tiles, host=True) if len(spheres) + len(tris) else None)
    if want_tile_work is None:  # (never with an adaptive add: the product plans partitions from plain pilots)
        want_tile_work = c.get("active") is None
    keep = {}

    def inp(name, dtype, value):
        if value is None:
            return None, 0
        a = np.ascontiguousarray(value, dtype).reshape(-1)
        keep[name] = a
        return a.ctypes.data, a.size

    a = SchedArgs()
    for k in ("W", "H", "spp", "big_pixels", "frustum", "split_samples", "split_depth"):
        setattr(a, k, int(c[k]))
    a.rank, a.world = c.get("rank", 0), c.get("world", 1)
    a.work_n, a.work_mean = c.get("work_n", 0), c.get("work_mean", 0)
    a.own_masks, a.ncams, a.model = c.get("own_masks", 0), ncams, c["model"]
    a.want_tile_work, a.want_live = int(want_tile_work), int(want_live)
    a.block_work = float(c["block_work"])
    a.frames, a.spheres, a.tris = frames.ctypes.data, _ptr(spheres), _ptr(tris)
    a.ns, a.nt = len(spheres), len(tris)
    a.tile_list, a.n_tile_list = inp("tile_list", np.int32, c.get("tile_list"))
    a.tile_masks, a.n_tile_masks = inp("tile_masks", U64, tile_masks)
    a.tile_cost, a.n_tile_cost = inp("tile_cost", np.float32, c.get("tile_cost", np.zeros(local, np.float32)))
    a.work_max, a.n_work_max = inp("work_max", np.uint32, c.get("work_max"))
    a.work_sum, a.n_work_sum = inp("work_sum", np.uint32, c.get("work_sum"))
    a.active, a.n_active = inp("active", np.uint32, c.get("active"))
    if cap_blocks is None:
        cap_blocks = npx * (-(-c["spp"] // c["split_samples"]))
    out = {"pixmask": np.zeros((local, 1024, 2), U64), "est": np.zeros((local, 1024), np.float32),
           "pilot_blocks": np.zeros((local, 16, 16), np.int32), "hist": np.zeros(BUCKETS, np.int32),
           "cursor": np.zeros(BUCKETS, np.int32), "totals": np.zeros(4, np.int32),
           "blocks": np.zeros((cap_blocks, 16), np.int32), "live_hist": np.zeros(BUCKETS, np.int32),
           "live_cursor": np.zeros(BUCKETS, np.int32), "live": np.zeros((npx, 4), np.int32),
           "live_pos": np.zeros((local, 1024), np.int32), "tile_work": np.zeros(local, np.float32)}
    for k, v in out.items():
        setattr(a, k, v.ctypes.data)
    a.cap_blocks = cap_blocks
    a.guards_written = -1
    rc = L.rtp_sched_run(ctypes.byref(a))
    assert rc == 0, f"rtp_sched_run({c['name']}): {rc}"
    assert a.local == local
    out["blocks"] = out["blocks"][:max(int(out["totals"][0]), 0)]
    out["live"] = out["live"][:max(0, min(int(out["totals"][3]), npx))] if want_live else out["live"][:0]
    out["guards_written"] = a.guards_written
    out["tiles"] = tiles
    out["tile_masks"] = None if tile_masks is None else np.asarray(tile_masks, U64).reshape(-1, local, 2)
    return out


# =============================================================== cameras and camera rays
def frame_of(camera, model, W, H):
    return rtgo.camera_frame(camera, model, W, H)


def ray_dirs(frame, W, H, px, py):
    """rt_camera_frame's ray through image point (px, py) = (x + du, y + dv):
    ((lower_left + horizontal u) + vertical v) - origin per component."""
    o, ll, h, v = frame[0:3], frame[3:6], frame[6:9], frame[9:12]
    u = np.asarray(px, np.float64) / W
    w = np.asarray(py, np.float64) / H
    return ((ll + h * u[..., None]) + v * w[..., None]) - o


def _project(frame, W, H, pts):
    """Image point (px, py) of each world point, and whether it lies in front of the camera."""
    o, ll, h, v = frame[0:3], frame[3:6], frame[6:9], frame[9:12]
    px = np.full(len(pts), 0.0)
    py = np.full(len(pts), 0.0)
    ok = np.zeros(len(pts), bool)
    for i, p in enumerate(pts):
        A = np.stack([h, v, -(p - o)], 1)
        with np.errstate(all="ignore"):
            try:
                s = np.linalg.solve(A, -(ll - o))
            except np.linalg.LinAlgError:
                continue
        if np.all(np.isfinite(s)) and s[2] > 0:
            px[i], py[i], ok[i] = s[0] * W, s[1] * H, True
    return px, py, ok


def _sphere_hits(spheres, o, d):
    """(rays, spheres) bool: Sphere.Hit on [TMIN, +inf)."""
    with np.errstate(all="ignore"):
        which = pc.ref_sphere(spheres["c"], spheres["r"], o, d, TMIN, INF)[0]
    return which != 0


def _tri_hits(verts, o, d):
    with np.errstate(all="ignore"):
        stage = pc.ref_tri(verts[:, 0], verts[:, 1], verts[:, 2], o, d, TMIN, INF)[0]
    return stage == 0


GRID = np.array([k / 8 for k in range(8)] + [LAST])  # 9 x 9 per pixel, the four extreme corners included


def ray_reference(spheres, verts, frame, W, H):
    """Which primitives the sampled camera rays of each image pixel hit:
    {"grid": (H*W, ns + nt) bool, hit by a ray of the 9 x 9 grid (the extreme
    corners are grid points), "near": by the ray through the pixel's point
    nearest the projection of the primitive's centre or of a triangle vertex}."""
    ns, nt = len(spheres), len(verts)
    o = frame[0:3]
    grid = np.zeros((H * W, ns + nt), bool)
    near = np.zeros((H * W, ns + nt), bool)
    gy, gx = np.meshgrid(GRID, GRID, indexing="ij")
    rows = max(1, 512 // W)
    for y0 in range(0, H, rows):
        ys = np.arange(y0, min(H, y0 + rows))
        X, Y = np.meshgrid(np.arange(W), ys)
        px = X.reshape(-1, 1) + gx.reshape(1, -1)
        py = Y.reshape(-1, 1) + gy.reshape(1, -1)
        d = ray_dirs(frame, W, H, px, py)[:, :, None, :]  # (pixels, 81, 1, 3)
        sl = slice(y0 * W, y0 * W + len(ys) * W)
        if ns:
            grid[sl, :ns] = _sphere_hits(spheres, o, d).any(1)
        if nt:
            grid[sl, ns:] = _tri_hits(verts, o, d).any(1)
    X, Y = np.meshgrid(np.arange(W), np.arange(H))
    X, Y = X.reshape(-1, 1).astype(np.float64), Y.reshape(-1, 1).astype(np.float64)

    def through(points):  # rays (pixels, prims, 3) through each pixel's point nearest each projection
        cx, cy, ok = _project(frame, W, H, points)
        qx = np.where(ok, np.clip(cx[None, :], X, X + LAST), X + 0.5)
        qy = np.where(ok, np.clip(cy[None, :], Y, Y + LAST), Y + 0.5)
        return ray_dirs(frame, W, H, qx, qy)

    if ns:
        with np.errstate(all="ignore"):
            finite = np.where(np.isfinite(spheres["c"]).all(1)[:, None], spheres["c"], 0.0)
            near[:, :ns] = pc.ref_sphere(spheres["c"], spheres["r"], o, through(finite), TMIN, INF)[0] != 0
    if nt:
        for pts in (verts[:, 0], verts[:, 1], verts[:, 2], verts.mean(1)):
            with np.errstate(all="ignore"):
                st = pc.ref_tri(verts[:, 0], verts[:, 1], verts[:, 2], o, through(pts), TMIN, INF)[0]
            near[:, ns:] |= st == 0
    return {"grid": grid, "near": near}


# =============================================================== the cone test, restated
def _len3(a0, a1, a2):
    return np.sqrt((a0 * a0 + a1 * a1) + a2 * a2)


def rect_cone(frame, model, W, H, x0, x1, y0, y1):
    """rect_cone (schedule.cpp) / pixel_cone (rt_schedule.hip) of the image
    rectangles [x0, x1) x [y0, y1) in binary64, the code's operation order:
    (axis (n, 3), cos, sin of the half-angle)."""
    o, ll, h, v = frame[0:3], frame[3:6], frame[6:9], frame[9:12]
    x0, x1, y0, y1 = (np.asarray(a, np.float64) for a in (x0, x1, y0, y1))
    with np.errstate(all="ignore"):
        if model != REFERENCE:
            u = [x0 / W, x1 / W]
            w = [y0 / H, y1 / H]
            cd = [[((ll[a] + h[a] * u[k & 1]) + v[a] * w[k >> 1]) - o[a] for a in range(3)] for k in range(4)]
            axis = [0.25 * ((cd[0][a] + cd[1][a]) + (cd[2][a] + cd[3][a])) for a in range(3)]
            al = _len3(*axis)
            axis = [a / al for a in axis]
            c = np.ones_like(x0)
            for k in range(4):
                cl = _len3(*cd[k])
                c = np.fmin(c, ((axis[0] * cd[k][0] + axis[1] * cd[k][1]) + axis[2] * cd[k][2]) / cl)
        else:
            vw = h[0]
            dx = [vw * (x0 / W - 0.5), vw * (x1 / W - 0.5)]
            dy = [2.0 * (y0 / H - 0.5), 2.0 * (y1 / H - 0.5)]
            axis = [0.5 * (dx[0] + dx[1]), 0.5 * (dy[0] + dy[1]), np.full_like(x0, -1.0)]
            al = _len3(*axis)
            axis = [a / al for a in axis]
            c = np.ones_like(x0)
            for k in range(4):
                cx, cy = dx[k & 1], dy[(k >> 1) & 1]
                cl = np.sqrt((cx * cx + cy * cy) + 1.0)
                c = np.fmin(c, ((axis[0] * cx + axis[1] * cy) - axis[2]) / cl)
        s = np.sqrt(np.fmax(0.0, 1.0 - c * c))
    return np.stack(axis, -1), c, s


def cone_meets(centres, radii, apex, axis, cos_t, sin_t):
    """cone_meets_sphere for every (cone, sphere): (cones, spheres) bool."""
    with np.errstate(all="ignore"):
        v = centres[None, :, :] - apex[None, None, :]
        v0, v1, v2 = v[..., 0], v[..., 1], v[..., 2]
        dc2 = (v0 * v0 + v1 * v1) + v2 * v2
        dc = np.sqrt(dc2)
        ra = (np.abs(radii)[None, :] * (1.0 + 1e-7) + 1e-7 * dc) + 1e-12
        near = ~(dc > ra)
        tl = np.sqrt(np.fmax(dc2 - ra * ra, 0.0))
        ax = axis[:, None, :]
        vd = (v0 * ax[..., 0] + v1 * ax[..., 1]) + v2 * ax[..., 2]
        miss = vd < ((cos_t[:, None] * (1.0 - 1e-9)) * tl - (sin_t[:, None] + 1e-9) * ra) - 1e-7 * dc
    return near | ~miss


def _pack(bits):
    """(n, k <= 64) bool -> (n,) uint64, bit i = column i."""
    out = np.zeros(bits.shape[0], U64)
    for i in range(bits.shape[1]):
        out |= bits[:, i].astype(U64) << U64(i)
    return out


def restated_masks(spheres, tris, frame, model, W, H):
    """The masks by definition: {"tile": (ntiles, 2) uint64 over all tiles of the
    image, "pixel": (H*W, 2) uint64, each pixel's cone test within its tile's masks}."""
    tx, ty = (W + 31) // 32, (H + 31) // 32
    t = np.arange(tx * ty)
    x0, y0 = (t % tx) * 32, (t // tx) * 32
    o = frame[0:3]

    def masks(x0, x1, y0, y1):
        axis, c, s = rect_cone(frame, model, W, H, x0, x1, y0, y1)
        ms = _pack(cone_meets(spheres["c"], spheres["r"], o, axis, c, s)) if len(spheres) else np.zeros(len(c), U64)
        mt = _pack(cone_meets(tris["bc"], tris["br"], o, axis, c, s)) if len(tris) else np.zeros(len(c), U64)
        return np.stack([ms, mt], 1)

    tile = masks(x0, np.minimum(x0 + 32, W), y0, np.minimum(y0 + 32, H))
    X, Y = np.meshgrid(np.arange(W), np.arange(H))
    X, Y = X.reshape(-1), Y.reshape(-1)
    pixel = masks(X, X + 1, Y, Y + 1) & tile[(Y // 32) * tx + X // 32]
    return {"tile": tile, "pixel": pixel}


def unpack(mask, n):
    """(..., ) uint64 -> (..., n) bool"""
    return ((mask[..., None] >> np.arange(n, dtype=U64)) & U64(1)).astype(bool)


# =============================================================== mask scenes
def spheres_of(centres, radii):
    s = np.zeros(len(radii), pc.SPHERE_DT)
    s["c"] = np.asarray(centres, np.float64).reshape(-1, 3)
    s["r"] = radii
    with np.errstate(all="ignore"):
        s["r2"] = s["r"] * s["r"]
    s["obj"] = np.arange(len(s))
    return s


CAMERAS = {
    # (model, camera dict): the reference model reads position and aspectRatio only
    "reference": (REFERENCE, {"position": (0.0, 1.0, 5.0), "aspectRatio": 1.25}),
    "rolled": (LOOKAT, {"position": (3.0, 2.0, 6.0), "lookAt": (0.2, 0.5, -1.0), "up": (0.4, 1.0, 0.1), "fov": 40.0}),
    "pitched": (LOOKAT, {"position": (0.0, 7.0, 3.0), "lookAt": (0.0, 0.0, -1.0), "up": (0.0, 1.0, 0.3), "fov": 70.0}),
    "tele": (LOOKAT, {"position": (1.0, 1.0, 30.0), "lookAt": (0.0, 1.0, 0.0), "up": (0.1, 1.0, 0.0), "fov": 5.0}),
    "fisheye": (LOOKAT, {"position": (0.0, 1.0, 4.0), "lookAt": (0.5, 0.5, 0.0), "up": (-0.3, 1.0, 0.2),
                         "fov": 150.0}),
}


def _case(name, cam, W, H, spheres=None, tris=None, verts=None, **kw):
    model, camera = CAMERAS[cam]
    c = {"name": name, "cam": cam, "model": model, "W": W, "H": H, "frames": frame_of(camera, model, W, H),
         "spheres": spheres if spheres is not None else np.zeros(0, pc.SPHERE_DT),
         "tris": tris if tris is not None else np.zeros(0, pc.TRI_DT),
         "verts": verts if verts is not None else np.zeros((0, 3, 3)),
         "spp": 4, "big_pixels": 16, "frustum": 1, "split_samples": 64, "split_depth": 16, "block_work": 384.0}
    c.update(kw)
    return c


def _subpixel(name, cam, W, H, seed):
    """64 spheres whose projection is below 1/20 pixel, at seeded sub-pixel
    positions half-way between the points of the 9 x 9 grid: the grid's rays
    miss them, the ray through the projected centre hits."""
    rng = np.random.default_rng(seed)
    model, camera = CAMERAS[cam]
    f = frame_of(camera, model, W, H)
    px = rng.integers(0, W, 64) + (rng.integers(0, 8, 64) + 0.5) / 8 + rng.uniform(-0.01, 0.01, 64)
    py = rng.integers(0, H, 64) + (rng.integers(0, 8, 64) + 0.5) / 8 + rng.uniform(-0.01, 0.01, 64)
    d = ray_dirs(f, W, H, px, py)
    depth = rng.uniform(2.0, 9.0, 64)
    # one pixel at unit distance along the view axis, shrunk by cos^2 of the ray's angle to it (the
    # projection of a sphere off the axis is stretched by that much)
    pix = min(np.sqrt((f[6:9] ** 2).sum()) / W, np.sqrt((f[9:12] ** 2).sum()) / H)
    r = 0.03 * pix * depth / (d ** 2).sum(1)
    c = _case(name, cam, W, H, spheres=spheres_of(f[0:3] + d * depth[:, None], r))
    c["subpixel"] = (np.floor(py).astype(int) * W + np.floor(px).astype(int), np.arange(64))
    return c


def _corners(name, cam, W, H):
    """Spheres centred on pixel corners with a silhouette of 0.3 pixel: the four
    pixels that meet there must all keep the bit."""
    model, camera = CAMERAS[cam]
    f = frame_of(camera, model, W, H)
    xs = np.array([1, 5, 31, 32, 33, W - 1, 17, 8][:max(1, min(8, W - 1))])
    ys = np.array([1, 32, 3, 32, 31, H - 1, 20, 9][:len(xs)])
    xs, ys = np.minimum(xs, W - 1), np.minimum(ys, H - 1)
    d = ray_dirs(f, W, H, xs.astype(float), ys.astype(float))
    depth = np.linspace(3.0, 8.0, len(xs))
    pix = min(np.sqrt((f[6:9] ** 2).sum()) / W, np.sqrt((f[9:12] ** 2).sum()) / H)
    r = 0.3 * pix * depth / (d ** 2).sum(1)
    c = _case(name, cam, W, H, spheres=spheres_of(f[0:3] + d * depth[:, None], r))
    c["corners"] = (xs, ys)
    return c


# (6 pixels: a tile's cone is the circle around its rectangle, 2.5 pixels wide of the edge at the spheres' row)
STEP_PIXELS = [-6.0, -1.5, -0.5, -1e-3, -1e-6, 0.0, 1e-6, 1e-3, 0.5, 1.5, 6.0]
STEP_ULPS = [1, -1, 2, -2, 4, -4, 2 ** 10, -2 ** 10, 2 ** 20, -2 ** 20, 2 ** 26, -2 ** 26]
STEP_EDGES = [10, 64]  # a pixel edge inside a tile, and a tile edge


def _stepped(name):
    """Reference camera, 96 x 70.  Spheres on the image's middle row whose right
    silhouette edge stands at image x = X + delta pixels, X a pixel edge and a
    tile edge: delta from +-6 pixels down to 1e-6, then the centre's x stepped
    by ulps from delta = 0."""
    W, H = 96, 70
    model, camera = CAMERAS["reference"]
    f = frame_of(camera, model, W, H)
    o, vw = f[0:3], f[6]
    depth, r = 6.0, 0.25
    cs, rs, meta = [], [], []

    def centre_x(edge_px):  # the sphere (cx, 0, -depth) seen from o whose right tangent ray passes image x edge_px
        T = vw * (edge_px / W - 0.5)  # tan of the tangent ray's angle
        lo, hi = -50.0, 50.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            ang = math.atan2(mid, depth) + math.asin(r / math.hypot(mid, depth))
            lo, hi = (mid, hi) if math.tan(ang) < T else (lo, mid)
        return 0.5 * (lo + hi)

    for X in STEP_EDGES:
        for dpx in STEP_PIXELS:
            cs.append((o[0] + centre_x(X + dpx), o[1], o[2] - depth))
            meta.append((X, dpx, 0))
        base = o[0] + centre_x(float(X))
        for k in STEP_ULPS:
            cs.append((float(pc.step(base, k)), o[1], o[2] - depth))
            meta.append((X, 0.0, k))
    c = _case(name, "reference", W, H, spheres=spheres_of(cs, np.full(len(cs), r)))
    c["steps"] = meta
    return c


def _edges(name, cam, W, H):
    """64 spheres: the guards of cone_meets_sphere and both ends of the mask word."""
    model, camera = CAMERAS[cam]
    f = frame_of(camera, model, W, H)
    o = f[0:3]
    view = ray_dirs(f, W, H, W / 2.0, H / 2.0)
    view = view / np.sqrt((view ** 2).sum())
    side = f[6:9] / np.sqrt((f[6:9] ** 2).sum())
    rng = np.random.default_rng(11)
    cs = [(0.0, -1000.0, 0.0), o + 0.1 * side, o + view * (0.5 + 1e-6), o + side * (0.5 + 1e-6),
          o - view * (0.5 + 1e-6), o + view * 5 + side, (NAN, 0.0, 0.0), o + view * 4, o - view * 10]
    rs = [1000.0, 2.0, 0.5, 0.5, 0.5, -0.7, 0.5, NAN, 1.0]
    names = ["ground", "camera inside", "1e-6 in front", "1e-6 beside", "1e-6 behind", "negative radius",
             "NaN centre", "NaN radius", "behind"]
    while len(cs) < 63:  # small spheres all over the view
        px, py = rng.uniform(0, W), rng.uniform(0, H)
        d = ray_dirs(f, W, H, px, py)
        cs.append(o + d * rng.uniform(2, 12))
        rs.append(rng.uniform(0.05, 0.6))
    d = ray_dirs(f, W, H, 1.5, 1.5)  # bit 63: a sphere a pixel wide in the first tile's corner
    cs.append(o + d * 6.0)
    rs.append(0.5 * 6.0 * np.sqrt((f[9:12] ** 2).sum()) / H)
    c = _case(name, cam, W, H, spheres=spheres_of(np.array([np.asarray(x, float) for x in cs]), np.array(rs)))
    c["named"] = names
    c["dropped"] = [8]  # entirely behind the camera: in no mask
    return c


BOUNDARY_STEPS = range(-12, 13)  # x 2e-7 rad: the margins of cone_meets_sphere move a narrow cone's boundary by up to 2e-6


def _boundary(name, cam, W, H):
    """Spheres stepped across the boundary of a cone itself -- the first tile's and one pixel's, which are
    circles around their rectangles, not the rectangles: sphere k of a family is tangent to the cone from
    outside but for k x 2e-7 rad, so the bit flips inside the family, where the code's margins put it."""
    model, camera = CAMERAS[cam]
    f = frame_of(camera, model, W, H)
    o = f[0:3]
    cs, fam = [], []
    d, r = 6.0, 0.3
    for rect in ((0, min(32, W), 0, min(32, H)), (13, 14, 9, 10)):
        axis, c, sn = rect_cone(f, model, W, H, *([v] for v in rect))
        axis = axis[0]
        perp = np.cross(axis, (0.3, 0.5, 0.8))
        perp /= np.sqrt((perp ** 2).sum())
        for k in BOUNDARY_STEPS:
            phi = math.atan2(sn[0], c[0]) + math.asin(r / d) + k * 2e-7
            cs.append(o + d * (math.cos(phi) * axis + math.sin(phi) * perp))
        fam.append(rect)
    c = _case(name, cam, W, H, spheres=spheres_of(np.array(cs), np.full(len(cs), r)))
    c["boundary"] = fam
    return c


def _cubes(name, cam, W, H):
    """Five cubes (60 triangles).  The first has its nearest vertex, and so three of its edges,
    on a pixel corner."""
    model, camera = CAMERAS[cam]
    f = frame_of(camera, model, W, H)
    o = f[0:3]
    boxes = [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((2.0, 0.5, -2.0), (1.0, 2.0, 1.0)), ((-2.5, 1.0, -1.0), (0.5, 0.5, 3.0)),
             ((0.5, 2.5, -4.0), (2.0, 0.3, 2.0)), ((-1.0, -0.5, 1.0), (0.2, 0.2, 0.2))]
    V = oracle.cube_triangles(*boxes[0]).reshape(-1, 3)
    nearest = V[np.argmin(((V - o) ** 2).sum(1))]
    xc, yc = min(13, W - 1), min(7, H - 1)
    d = ray_dirs(f, W, H, float(xc), float(yc))
    target = o + d * (np.sqrt(((nearest - o) ** 2).sum()) / np.sqrt((d ** 2).sum()))
    boxes[0] = (tuple(np.asarray(boxes[0][0]) + (target - nearest)), boxes[0][1])
    flat = pc.flatten(pc.make_scene([pc.cube_obj(p, s) for p, s in boxes]))
    verts = np.concatenate([oracle.cube_triangles(p, s) for p, s in boxes])
    assert len(flat["tris"]) == len(verts) and np.array_equal(flat["tris"]["v0"], verts[:, 0])
    c = _case(name, cam, W, H, tris=flat["tris"], verts=verts)
    c["cube_corner"] = (xc, yc)
    return c


@functools.cache
def mask_cases():
    cs = [
        _subpixel("subpixel/reference", "reference", 40, 36, 1),
        _subpixel("subpixel/rolled-8:1", "rolled", 64, 8, 2),
        _subpixel("subpixel/fisheye", "fisheye", 33, 34, 3),
        _subpixel("subpixel/tele", "tele", 36, 40, 4),
        _subpixel("subpixel/width-1", "pitched", 1, 70, 5),
        _subpixel("subpixel/height-1", "rolled", 70, 1, 6),
        _corners("corners/reference", "reference", 40, 36),
        _corners("corners/pitched", "pitched", 40, 36),
        _stepped("stepped"),
        _edges("edges/reference", "reference", 96, 70),
        _edges("edges/rolled", "rolled", 40, 36),
        _edges("edges/fisheye", "fisheye", 36, 40),
        _boundary("boundary/reference", "reference", 40, 36),
        _boundary("boundary/rolled", "rolled", 40, 36),
        _cubes("cubes/reference", "reference", 40, 36),
        _cubes("cubes/pitched", "pitched", 36, 34),
    ]
    return {c["name"]: c for c in cs}


def case_tile_masks(c, tiles, host):
    """The tile masks prepare_schedule uploads for the case's tiles: one camera's, or for a
    sequence [the OR][camera 0's][camera 1's]...; own_masks: every primitive."""
    local = len(tiles)
    if c.get("own_masks"):
        bits = lambda n: (1 << n) - 1 if n < 64 else 2 ** 64 - 1
        return np.tile(np.array([bits(len(c["spheres"])), bits(len(c["tris"]))], U64), (local, 1))
    frames = np.asarray(c["frames"]).reshape(-1, 12)
    per = []
    for f in frames:
        if host:
            per.append(host_tile_masks(c["spheres"], c["tris"], f, c["model"], c["W"], c["H"], tiles))
        else:
            per.append(restated_masks(c["spheres"], c["tris"], f, c["model"], c["W"], c["H"])["tile"][tiles])
    if c.get("ncams", 0) == 0:
        return per[0]
    return np.stack([np.bitwise_or.reduce(np.stack(per), 0)] + per)


@functools.cache
def mask_reference(name, cam=0):
    """Both references of mask case `name` under its camera `cam`, in image order."""
    c = all_mask_cases()[name]
    f = np.asarray(c["frames"]).reshape(-1, 12)[cam]
    rays = ray_reference(c["spheres"], c["verts"], f, c["W"], c["H"])
    rest = restated_masks(c["spheres"], c["tris"], f, c["model"], c["W"], c["H"])
    return {"grid": rays["grid"], "near": rays["near"], "hit": rays["grid"] | rays["near"], **rest}


def expected_pixmask(c, tiles):
    """(local, 1024, 2) uint64 by the restated definition, and (local, 1024, ns + nt) bool: hit by a sampled ray
    of any of the case's cameras."""
    W, H = c["W"], c["H"]
    x, y, inimg = local_xy(W, H, tiles)
    idx = np.where(inimg, y * W + x, 0)
    ncam = max(c.get("ncams", 0), 1)
    want = np.zeros((len(tiles), 1024, 2), U64)
    hit = np.zeros((len(tiles), 1024, len(c["spheres"]) + len(c["verts"])), bool)
    for k in range(ncam):
        ref = mask_reference(c["base"] if "base" in c else c["name"], k if "base" not in c else c["cams"][k])
        want |= np.where(inimg[..., None], ref["pixel"][idx], U64(0))
        hit |= ref["hit"][idx] & inimg[..., None]
    if c.get("own_masks"):
        want = np.where(inimg[..., None], case_tile_masks(c, tiles, host=False)[:, None, :], U64(0))
    if c.get("active") is not None:
        on = np.asarray(c["active"]).reshape(len(tiles), 1024) != 0
        want = np.where(on[..., None], want, U64(0))
        hit &= on[..., None]
    return want, hit


def expected_pilot(tiles, pixmask):
    """The pilot's records: per 64 pixels {lt, 64 w, 64, 0, 1, -1, 1, 0, OR of masks, live bits, t, 0}."""
    local = len(tiles)
    rec = np.zeros((local, 16, 16), np.int32)
    for lt in range(local):
        for w in range(16):
            m = pixmask[lt, w * 64:(w + 1) * 64]
            live = sum(1 << k for k in range(64) if m[k, 0] | m[k, 1])
            words = np.array([np.bitwise_or.reduce(m[:, 0]), np.bitwise_or.reduce(m[:, 1]), live], U64).view(np.int32)
            rec[lt, w] = [lt, w * 64, 64, 0, 1, -1, 1, 0, *words, tiles[lt], 0]
    return rec


# ---- instantiations of the mask scenes: tiles, sequences, adaptive adds
def _variant(base, name, **kw):
    c = dict(mask_cases()[base])
    c.update(name=name, base=base, cams=[0], **kw)
    return c


def _sequence(base, name, cams):
    """Cameras of a sequence on scene `base`: camera dicts under the scene's model."""
    b = mask_cases()[base]
    frames = np.stack([b["frames"]] + [frame_of(cam, b["model"], b["W"], b["H"]) for cam in cams[1:]])
    c = dict(b)
    c.update(name=name, frames=frames, ncams=len(cams))
    return c


@functools.cache
def all_mask_cases():
    """The mask scenes and what is instantiated on them."""
    cs = dict(mask_cases())
    rng = np.random.default_rng(21)

    def add(c):
        cs[c["name"]] = c

    e = "edges/reference"  # 96 x 70: 9 tiles
    add(_variant(e, "edges/world-2-rank-0", world=2, rank=0))
    add(_variant(e, "edges/world-2-rank-1", world=2, rank=1))
    add(_variant(e, "edges/world-3-rank-2", world=3, rank=2))
    add(_variant(e, "edges/tile-list", tile_list=[7, 2, 4, 0]))
    add(_variant(e, "edges/frustum-0", frustum=0))
    # adaptive adds: seeded active flags, the second local tile with no active pixel
    act = (rng.uniform(size=(9, 1024)) < 0.6).astype(np.uint32)
    act[1] = 0
    add(_variant(e, "edges/adaptive", active=act, own_masks=0))
    add(_variant(e, "edges/adaptive-own-masks", active=act, own_masks=1, frustum=0))
    # sequences: the corner spheres from 1, 2 and 5 cameras; the turned-away camera sees nothing anywhere
    ref = CAMERAS["pitched"][1]
    away = dict(ref, lookAt=(0.0, 14.0, 7.0))
    moved = [dict(ref, position=(0.5 * k, 7.0, 3.0 + 0.2 * k)) for k in range(1, 4)]
    add(_sequence("corners/pitched", "corners/seq-1", [ref]))
    add(_sequence("corners/pitched", "corners/seq-2", [ref, away]))
    add(_sequence("corners/pitched", "corners/seq-5", [ref, moved[0], away, moved[1], moved[2]]))
    return cs


# =============================================================== sched_est
F32 = np.float32


def est_reference(c, local):
    """sched_est in float32: (local, 1024) float32, the sign bit marking a pixel to split."""
    spp, n = c["spp"], c.get("work_n", 0)
    wm = c.get("work_max")
    if wm is not None:
        wm = np.asarray(wm, np.uint32).reshape(local, 32, 32)
        ws = np.asarray(c["work_sum"], np.uint32).reshape(local, 32, 32)
    heavy = np.zeros((local, 32, 32), bool)
    if wm is not None and n < spp and not c.get("work_mean", 0):
        m = wm.copy()  # the longest path among the pixel and its 4 neighbours inside the tile
        m[:, :, 1:] = np.maximum(m[:, :, 1:], wm[:, :, :-1])
        m[:, :, :-1] = np.maximum(m[:, :, :-1], wm[:, :, 1:])
        m[:, 1:, :] = np.maximum(m[:, 1:, :], wm[:, :-1, :])
        m[:, :-1, :] = np.maximum(m[:, :-1, :], wm[:, 1:, :])
        e = m.astype(F32) + F32(0.02)
    elif wm is not None:
        e = (ws.astype(np.float64) / np.float64(n)).astype(F32) + F32(0.02)
        heavy = wm.astype(np.int32) > c["split_depth"]
        e = np.where(heavy, np.fmax(e, wm.astype(F32)), e)
    else:
        cost = np.asarray(c.get("tile_cost", np.zeros(local)), F32)
        base = F32(np.float64(c["block_work"]) / (2.0 * max(1, spp)))
        e = np.where(cost > 0, base * (F32(1.0) + F32(1e-3) * np.fmin(cost, F32(100.0))), F32(0.0)).astype(F32)
        e = np.broadcast_to(e[:, None, None], (local, 32, 32)).copy()
    if c.get("active") is not None:
        off = np.asarray(c["active"]).reshape(local, 32, 32) == 0
        e = np.where(off, F32(0.0), e)
        heavy = heavy & ~off
    e = np.where(heavy, -e - F32(1e-30), e).astype(F32)
    return e.reshape(local, 1024)


# =============================================================== blocks
def weight_class(w):
    """(class, distance of 8 log2(1 + w) from the nearest integer)"""
    l = 8.0 * math.log2(1.0 + max(w, 0.0))
    return 127 - min(127, int(math.floor(l))), abs(l - round(l))


def blocks_reference(c, est, tiles, pixmask):
    """The partition by definition.  est: (local, 1024) float32 (the reference's);
    pixmask: (local, 1024, 2) or None (no tile masks).  Returns {"records": [(class, 16 ints)],
    "weights": [...], "kinds": counts, "nsplit", "exact": every prefix sum was exact}."""
    spp, S, bw = c["spp"], float(max(c["spp"], 1)), float(c["block_work"])
    big, ss = c["big_pixels"], c["split_samples"]
    tm = c.get("_tile_masks")
    recs, weights, exact = [], [], True
    kinds = {"multi": 0, "single": 0, "split": 0, "black": 0}
    nsplit = 0

    def record(lt, p0, n, s0, ns, slot, nsub, flags):
        ms = mt = live = 0
        if tm is not None:
            for k in range(n):
                a, b = int(pixmask[lt, p0 + k, 0]), int(pixmask[lt, p0 + k, 1])
                ms |= a
                mt |= b
                if a | b:
                    live |= 1 << k
        words = np.array([ms, mt, live], U64).view(np.int32)
        return (lt, p0, n, s0, ns, slot, nsub, flags, *[int(x) for x in words], int(tiles[lt]), 0)

    for lt in range(len(tiles)):
        if c["frustum"] and tm is not None and spp > 0 and not (int(tm[lt, 0]) | int(tm[lt, 1])):
            for k in range(16):
                recs.append((127, record(lt, 64 * k, 64, 0, spp, -1, 1, KBLOCK_BLACK)))
                weights.append(None)
            kinds["black"] += 16
            continue
        a = np.abs(est[lt]).astype(np.float64)
        w = S * a
        pre = [0.0]
        for q in range(1024):  # plain sums, in pixel order
            pre.append(pre[-1] + float(w[q]))
        exact = exact and _prefix_exact(w)
        heavy = [spp > 1 and (w[q] > bw or est[lt, q] < 0) for q in range(1024)]
        barrier = [w[q] > bw or heavy[q] for q in range(1024)]
        q = 0
        while q < 1024:
            if heavy[q]:
                nsub = -(-spp // ss)
                for j in range(nsub):
                    s0, s1 = spp * j // nsub, spp * (j + 1) // nsub
                    wt = (s1 - s0) * float(a[q])
                    recs.append((weight_class(wt)[0], record(lt, q, 1, s0, s1 - s0, nsplit, nsub, 0)))
                    weights.append(wt)
                nsplit += 1
                kinds["split"] += 1
                q += 1
                continue
            e = q + 1
            while (e + 1 <= min(q + big, 1024) and not barrier[e] and pre[e + 1] <= pre[q] + bw):
                e += 1
            wt = pre[e] - pre[q]
            recs.append((weight_class(wt)[0], record(lt, q, e - q, 0, spp, -1, 1, 0)))
            weights.append(wt)
            kinds["multi" if e - q > 1 else "single"] += 1
            q = e
    return {"records": recs, "weights": weights, "kinds": kinds, "nsplit": nsplit, "exact": exact}


def _prefix_exact(w):
    """Every partial sum of w, in any order, is exact in binary64: the values are
    multiples of one power of two u, and their sum is below 2^53 u."""
    nz = [float(x) for x in w if x != 0]
    if not nz:
        return True
    def low_bit(x):  # the exponent of the lowest set bit of a binary64
        m, e = math.frexp(x)
        k = int(math.ldexp(m, 53))
        return e - 53 + ((k & -k).bit_length() - 1)

    u = min(low_bit(x) for x in nz)
    return sum(int(math.ldexp(x, -u)) for x in nz) < 2 ** 53


def block_properties(c, blocks, est, tiles, tile_masks):
    """The properties every partition has, whatever the order of the sums: None, or what is wrong."""
    spp, bw, big, ss = c["spp"], float(c["block_work"]), c["big_pixels"], c["split_samples"]
    S = float(max(spp, 1))
    cover = np.zeros((len(tiles), 1024, spp), np.int32)
    last = -1
    for i, r in enumerate(blocks):
        lt, p0, n, s0, ns, slot, nsub, flags = (int(x) for x in r[:8])
        if not (0 <= lt < len(tiles) and 0 <= p0 and n >= 1 and p0 + n <= 1024 and 0 <= s0 and ns >= 1
                and s0 + ns <= spp):
            return f"record {i}: out of range {r[:8]}"
        if flags & KBLOCK_BLACK:
            k = 127
        else:
            cover[lt, p0:p0 + n, s0:s0 + ns] += 1
            if n > big:
                return f"record {i}: {n} pixels > big_pixels {big}"
            wsum = S * float(np.abs(est[lt, p0:p0 + n]).astype(np.float64).sum())
            if slot < 0 and n > 1 and wsum > bw * (1 + 2.0 ** -40):
                return f"record {i}: tile {lt} pixels [{p0}, {p0 + n}) weigh {wsum} > block_work {bw}"
            if slot >= 0 and (n != 1 or ns > ss):
                return f"record {i}: a split block of {n} pixels, {ns} samples (split_samples {ss})"
            if slot < 0 and (s0 != 0 or ns != spp):
                return f"record {i}: an unsplit block with samples [{s0}, {s0 + ns})"
            k, near = weight_class(ns * float(abs(est[lt, p0])) if slot >= 0 else wsum)
            if near < 1e-6 and k < last:  # at a class boundary the order of the sums decides: either class
                k = min((j for j in (k - 1, k, k + 1) if j >= last), default=k)
        if k < last:
            return f"record {i}: class {k} after class {last}"
        last = k
    black = np.array([c["frustum"] and tile_masks is not None and not (int(tile_masks[lt, 0]) | int(tile_masks[lt, 1]))
                      for lt in range(len(tiles))], bool)
    want = np.where(black[:, None, None], 0, 1)
    bad = np.argwhere(cover != want)
    if len(bad):
        lt, q, s = bad[0]
        return f"tile {lt} pixel {q} sample {s}: in {cover[lt, q, s]} records"
    return None


# ---- scheduler inputs
def _far_sphere():
    """One sphere around the camera: every image pixel keeps bit 0."""
    return spheres_of([(0.0, 1.0, 5.0)], np.array([50.0]))


def _sched_case(name, W=32, H=32, **kw):
    model, camera = CAMERAS["reference"]
    local = len(tiles_of(W, H, kw.get("rank", 0), kw.get("world", 1), kw.get("tile_list")))
    c = {"name": name, "model": model, "W": W, "H": H, "frames": frame_of(camera, model, W, H),
         "spp": 16, "big_pixels": 16, "frustum": 1, "split_samples": 8, "split_depth": 16, "block_work": 384.0,
         "tile_cost": np.zeros(local, np.float32)}
    c.update(kw)
    return c


def _measured(rng, local, lo=1, hi=51, n=16, heavy_at=()):
    """work_max in [lo, hi], work_sum = floor(n * (a multiple of 1/16 up to work_max))."""
    wm = rng.integers(lo, hi + 1, (local, 1024)).astype(np.uint32)
    ws = (rng.integers(1, 17, (local, 1024)) * wm * n // 16).astype(np.uint32)
    for lt, q, v in heavy_at:
        wm[lt, q] = v
        ws[lt, q] = max(1, min(v, 3)) * n
    return wm, ws


@functools.cache
def sched_cases():
    rng = np.random.default_rng(7)
    cs = []

    def add(name, **kw):
        cs.append(_sched_case(name, **kw))

    def measured(name, local=1, heavy_at=(), hi=15, **kw):
        n = min(16, kw.get("spp", 16))  # (the product measures at most spp samples)
        wm, ws = _measured(rng, local, 1, hi, n=n, heavy_at=heavy_at)
        add(name, work_max=wm, work_sum=ws, work_n=n, work_mean=1, **kw)

    # ---- sched_est: the pilot branch (rows and columns 0 and 31 hold the maximum), a measured frame
    wm = rng.integers(1, 52, (2, 1024)).astype(np.uint32)
    g = wm.reshape(2, 32, 32)
    g[0, 0, :], g[0, :, 31], g[1, 31, :], g[1, :, 0] = 60, 61, 62, 63
    add("est/pilot", W=64, H=32, work_max=wm, work_sum=wm, work_n=1, spp=16, block_work=1e6)
    wm, ws = _measured(rng, 1, 1, 51, n=16, heavy_at=[(0, 5, 16), (0, 6, 17), (0, 1023, 40)])
    add("est/measured-frame", work_max=wm, work_sum=ws, work_n=16, spp=16)          # work_n == spp
    add("est/work-mean", work_max=wm, work_sum=ws, work_n=16, work_mean=1, spp=64)
    add("est/spp-1", work_max=wm, work_sum=wm, work_n=1, spp=1, block_work=20.0)     # work_n == spp == 1
    add("est/no-pilot", W=90, H=70, tile_cost=np.array([0, 1, 3, 0, 100, 250, 7, 0, 2], np.float32), spp=7,
        block_work=384.0)
    act = (rng.uniform(size=(1, 1024)) < 0.5).astype(np.uint32)
    add("est/adaptive-stopped", work_max=wm, work_sum=ws, work_n=16, spp=16, active=act, own_masks=1, frustum=0,
        spheres=_far_sphere(), tile_masks=np.array([[1, 0]], U64))
    # ---- blocks
    add("blocks/all-zero", spp=4)
    heavy_all = [(0, q, 40) for q in range(1024)]
    measured("blocks/every-pixel-heavy", heavy_at=heavy_all, spp=130, split_samples=1)
    measured("blocks/alternating", heavy_at=[(0, q, 40) for q in range(0, 1024, 2)], spp=16, split_samples=8)
    measured("blocks/heavy-at-0-and-1023", heavy_at=[(0, 0, 17), (0, 1023, 17)], spp=63, split_samples=64)
    for big in (1, 64):
        measured(f"blocks/big-pixels-{big}", big_pixels=big, spp=2, block_work=1e6 if big == 64 else 384.0)
    for ss in (1, 8, 64):
        for spp in (1, 2, 63, 64, 65, 130):
            measured(f"blocks/split-{ss}-spp-{spp}", heavy_at=[(0, 7, 30), (0, 500, 17), (0, 501, 18)], spp=spp,
                     split_samples=ss, block_work=384.0)
    measured("blocks/spp-1-over-block-work", spp=1, block_work=5.0, hi=9)
    measured("blocks/block-work-1", spp=2, block_work=1.0, hi=3)
    measured("blocks/block-work-1e6", spp=64, block_work=1e6)
    # a block whose sum is block_work exactly, and the same block 2^-20 over: the first 9 pixels
    wm, ws = _measured(rng, 1, 1, 15, n=8)
    e = est_reference(_sched_case("tmp", work_max=wm, work_sum=ws, work_n=8, work_mean=1, spp=8), 1)
    exact_sum = float((8.0 * np.abs(e[0, :9]).astype(np.float64)).sum())
    add("blocks/sum-equals-block-work", work_max=wm, work_sum=ws, work_n=8, work_mean=1, spp=8,
        block_work=exact_sum)
    add("blocks/sum-over-block-work", work_max=wm, work_sum=ws, work_n=8, work_mean=1, spp=8,
        block_work=exact_sum - 2.0 ** -20)
    # tiles: 2 and 9 local tiles with partial and black ones (tile masks given: bit 0, the far sphere, or nothing)
    tm2 = np.array([[1, 0], [0, 0]], U64)
    measured("blocks/2-tiles-one-black", local=2, W=50, H=20, spheres=_far_sphere(), tile_masks=tm2, spp=16)
    tm9 = np.array([[1, 0]] * 9, U64)
    tm9[[2, 4]] = 0
    measured("blocks/9-tiles", local=9, W=90, H=70, heavy_at=[(3, 100, 20), (8, 0, 33)], spheres=_far_sphere(),
             tile_masks=tm9, spp=16)
    measured("blocks/9-tiles-frustum-0", local=9, W=90, H=70, spheres=_far_sphere(), tile_masks=tm9, spp=16, frustum=0)
    measured("blocks/no-live-pixel", local=1, W=20, H=20, spheres=_far_sphere(), tile_masks=np.zeros((1, 2), U64),
             spp=4)
    measured("blocks/tile-list", local=3, W=90, H=70, tile_list=[8, 1, 5], spp=16)
    return {c["name"]: c for c in cs}


@functools.cache
def random_cases():
    """20 seeded inputs whose sums are NOT exact (work sums over 30 binades): properties only."""
    rng = np.random.default_rng(99)
    cs = []
    for k in range(20):
        local = int(rng.integers(1, 4))
        W, H = [(32, 32), (50, 20), (90, 20)][local - 1]
        wm = rng.integers(1, 40, (local, 1024)).astype(np.uint32)
        ws = np.exp2(rng.uniform(0, 31, (local, 1024))).astype(np.uint32)
        spp = int(rng.integers(1, 65))
        cs.append(_sched_case(f"random/{k}", W=W, H=H, work_max=wm, work_sum=ws, work_n=min(3, spp), work_mean=1,
                              spp=spp, big_pixels=int(rng.integers(1, 65)),
                              split_samples=int(rng.integers(1, 65)), split_depth=int(rng.integers(4, 40)),
                              block_work=float(np.exp2(rng.uniform(0, 34)))))
    return {c["name"]: c for c in cs}


@functools.cache
def sched_reference(name):
    """est, pixel masks, blocks, live set and tile work of scheduler case `name`."""
    c = dict(sched_cases()[name])
    tiles = tiles_of(c["W"], c["H"], c.get("rank", 0), c.get("world", 1), c.get("tile_list"))
    local = len(tiles)
    x, y, inimg = local_xy(c["W"], c["H"], tiles)
    est = est_reference(c, local)
    tm = None if "tile_masks" not in c else np.asarray(c["tile_masks"], U64).reshape(local, 2)
    pixmask = None
    if tm is not None:  # the far sphere: a pixel keeps its tile's bit 0 (an adaptive add: while active)
        on = inimg if c.get("active") is None else inimg & (np.asarray(c["active"]).reshape(local, 1024) != 0)
        pixmask = np.where(on[..., None], tm[:, None, :], U64(0))
    c["_tile_masks"] = tm
    blocks = blocks_reference(c, est, tiles, pixmask)
    culled = (c["frustum"] or c.get("active") is not None) and tm is not None
    live = inimg & ((pixmask[..., 0] | pixmask[..., 1]) != 0) if culled else inimg
    a = np.abs(est).astype(np.float64)
    work = [float(max(c["spp"], 1)) * sum(float(v) for v in a[lt][inimg[lt]]) for lt in range(local)]
    return {"case": c, "tiles": tiles, "est": est, "tile_masks": tm, "pixmask": pixmask, "blocks": blocks,
            "live": live, "x": x, "y": y, "tile_work": np.array(work, np.float64).astype(np.float32),
            "tile_work_exact": all(_prefix_exact(a[lt][inimg[lt]]) for lt in range(local))}
