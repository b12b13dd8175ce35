"""The quality set-up of the edge resolve, used by
tests/test_matte_cpu.py: a one-sample frame at
144x96 by the oracle, its first-hit features by aov_reference, rt_denoise_host,
a matte from the restatement (tests/matte_reference.py) and
rt_matte_resolve_host, against a 512-sample render of the same frame.  No
device.

S_CUBE and C_FLOOR are clip_cases' frame 0 under clip_cases' camera (the set-up
of tests/clip_quality.py).
sequence() is the same comparison at the end of render_sequence's chain on the
host twins: six one-sample frames from a moving camera accumulated by
rt_temporal_host, the last one denoised, then resolved."""
import functools

import numpy as np

import oracle
import rtgo
from aov_reference import reference as aov_reference
from clip_cases import CAMERA, frame_json
from matte_reference import matte_of, keys, parts_of
from scene_cases import make_settings
from sequence_cases import at, scene_json

QW, QH, TRUTH_SPP, MATTE_SPP = 144, 96, 512, 16
SEEDS = (3, 4, 5)
QFRAMES, QSTEP = 6, 0.05  # the camera moves 0.05 in x per frame, as in tests/test_temporal_cpu.py


def scene_text(name):
    return frame_json(name, 0, CAMERA)


def rmse(img, ref, mask=None):
    d = (np.asarray(img, np.float64) - ref) ** 2
    return float(np.sqrt((d if mask is None else d[mask]).mean()))


@functools.lru_cache(maxsize=None)
def truth(text):
    img, _, _ = oracle.render(rtgo.Scene.from_json_text(text), QW, QH,
                              make_settings(rtgo, {"samples": TRUTH_SPP, "max_depth": 50}, 77))
    return img.astype(np.float64)


def edge_mask(obj):
    """Pixels with a 4-neighbour of another object id."""
    e = np.zeros(obj.shape, bool)
    e[:, 1:] |= obj[:, 1:] != obj[:, :-1]
    e[:, :-1] |= obj[:, 1:] != obj[:, :-1]
    e[1:, :] |= obj[1:, :] != obj[:-1, :]
    e[:-1, :] |= obj[1:, :] != obj[:-1, :]
    return e


@functools.lru_cache(maxsize=None)
def denoised(name, seed):
    """(denoised (H, W, 3) float32, object (H, W) int32) of the one-sample frame."""
    text = scene_text(name)
    noisy, _, _ = oracle.render(rtgo.Scene.from_json_text(text), QW, QH,
                                make_settings(rtgo, {"samples": 1, "max_depth": 50}, seed))
    feat = aov_reference(text, QW, QH, 1, seed)
    den, _ = rtgo.denoise_host(noisy.astype(np.float32), feat["normal"], feat["depth"], feat["albedo"], feat["object"])
    return den, feat["object"]


def resolved(color, obj, text, seed, samples):
    """(rt_matte_resolve_host of color, the mask of the pixels with two parts or more)."""
    m = matte_of(keys(text, QW, QH, MATTE_SPP, seed), samples)
    out, _ = rtgo.matte_resolve_host(color, obj, m["id"], m["count"], m["rest"], samples)
    return out, parts_of(m["count"], m["rest"], samples) >= 2


def figures(name, seed, samples=MATTE_SPP):
    """RMSE against the truth: {"image": (denoised, resolved), "edge": (denoised, resolved, pixels)}, the mixed
    pixels' count and whether every other pixel kept its bits."""
    text = scene_text(name)
    den, obj = denoised(name, seed)
    out, mixed = resolved(den, obj, text, seed, samples)
    ref, e = truth(text), edge_mask(obj)
    same = np.array_equal(out.view(np.uint32)[~mixed], den.view(np.uint32)[~mixed])
    return {"image": (rmse(den, ref), rmse(out, ref)), "edge": (rmse(den, ref, e), rmse(out, ref, e), int(e.sum())),
            "mixed": int(mixed.sum()), "unmixed_same": same}


@functools.lru_cache(maxsize=None)
def sequence(samples=MATTE_SPP):
    """(denoised RMSE, resolved RMSE, mixed pixels) of the last of six accumulated frames of S_CUBE."""
    state = None
    for f in range(QFRAMES):
        cam = at((QSTEP * f, CAMERA["position"][1], CAMERA["position"][2]), CAMERA)
        text = scene_json("S_CUBE", cam)
        noisy, _, _ = oracle.render(rtgo.Scene.from_json_text(text), QW, QH,
                                    make_settings(rtgo, {"samples": 1, "max_depth": 50}, 3 + f))
        feat = aov_reference(text, QW, QH, 1, 3 + f)
        cur = dict(color=noisy.astype(np.float32), depth=feat["depth"], object=feat["object"], normal=feat["normal"],
                   frame=rtgo.camera_frame(cam, "reference", QW, QH))
        color, count, _ = rtgo.temporal_host(cur, state)
        state = dict(cur, color=color, count=count)
    den, _ = rtgo.denoise_host(color, feat["normal"], feat["depth"], feat["albedo"], feat["object"])
    out, mixed = resolved(den, feat["object"], text, 3 + QFRAMES - 1, samples)
    ref = truth(text)
    return rmse(den, ref), rmse(out, ref), int(mixed.sum())
