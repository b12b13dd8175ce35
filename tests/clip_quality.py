"""The quality set-up of history rectification, shared by
tests/test_clip_cpu.py and scripts/clip_grid.py: six one-sample frames of a
case of tests/clip_cases.py at 144x96 by the oracle, their first-hit features
by aov_reference, accumulated by rt_temporal_clip_host (the host twin) with and
without the clip, against a 512-sample render of the last frame.  No device."""
import functools

import numpy as np

import oracle
import rtgo
from aov_reference import reference as aov_reference
from clip_cases import CAMERA, FLOOR_ID, frame_json
from scene_cases import make_settings

QW, QH, QFRAMES, TRUTH_SPP = 144, 96, 6, 512
TRAIL_THRESHOLD = 0.02  # luminance of the 512-sample renders, last frame against the frame two before it


def lum(img):
    return (0.2126 * img[..., 0] + 0.7152 * img[..., 1]) + 0.0722 * img[..., 2]


@functools.lru_cache(maxsize=None)
def inputs(name, frames=QFRAMES):
    """Per frame the host call's `cur` dict (1-spp colour, depth, object, normal, albedo, frame) and the motion
    table from the frame before (None for frame 0); read-only."""
    frame = rtgo.camera_frame(CAMERA, "reference", QW, QH)
    out, last = [], None
    for f in range(frames):
        text = frame_json(name, f, CAMERA)
        scene = rtgo.Scene.from_json_text(text)
        noisy, _, _ = oracle.render(scene, QW, QH, make_settings(rtgo, {"samples": 1, "max_depth": 50}, 3 + f))
        feat = aov_reference(text, QW, QH, 1, 3 + f)
        cur = dict(color=noisy.astype(np.float32), depth=feat["depth"], object=feat["object"], normal=feat["normal"],
                   albedo=feat["albedo"], frame=frame)
        for a in cur.values():
            a.flags.writeable = False
        out.append((cur, None if last is None else rtgo.scene_motion(last, scene)))
        last = scene
    return out


@functools.lru_cache(maxsize=None)
def truth(name, f):
    """The 512-sample render of frame f, float64."""
    scene = rtgo.Scene.from_json_text(frame_json(name, f, CAMERA))
    img, _, _ = oracle.render(scene, QW, QH, make_settings(rtgo, {"samples": TRUTH_SPP, "max_depth": 50}, 77))
    return img.astype(np.float64)


def accumulate(name, clip, frames=QFRAMES):
    """The last frame's (color, count, clipped) after the frames; clip None: radius 0, the pass as it is."""
    state = None
    k = dict(clip) if clip is not None else dict(radius=0)
    for cur, table in inputs(name, frames):
        color, count, clipped, _ = rtgo.temporal_clip_host(cur, state, table if state is not None else None, clip=k)
        state = dict(cur, color=color, count=count)
    return color, count, clipped


def rmse(img, ref, mask=None):
    d = (img.astype(np.float64) - ref) ** 2
    return float(np.sqrt((d if mask is None else d[mask]).mean()))


def masks(name):
    """(floor, trail): the floor's pixels in the last frame, and those of them whose 512-sample luminance differs
    between the last frame and the frame two before it by more than TRAIL_THRESHOLD."""
    last = inputs(name)[-1][0]
    floor = last["object"] == FLOOR_ID
    moved = np.abs(lum(truth(name, QFRAMES - 1)) - lum(truth(name, QFRAMES - 3))) > TRAIL_THRESHOLD
    return floor, floor & moved


def figures(name, clip):
    """RMSE against the last frame's truth, with the clip / without: whole image, and for the floor cases the
    floor, the trail and the floor outside the trail.  {region: (with, without, pixels)}."""
    ref = truth(name, QFRAMES - 1)
    a, b = accumulate(name, clip)[0], accumulate(name, None)[0]
    out = {"image": (rmse(a, ref), rmse(b, ref), QW * QH)}
    if name != "S_CUBE":
        floor, trail = masks(name)
        for region, m in (("floor", floor), ("trail", trail), ("static", floor & ~trail)):
            out[region] = (rmse(a, ref, m), rmse(b, ref, m), int(m.sum()))
    return out
