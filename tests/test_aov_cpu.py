"""First-hit feature buffers (rt_context_render_aov_async), CPU:
the declaration, its ctypes mirror, the Python layer's argument checks, and the
reference helper of the GPU tests (tests/aov_reference.py) held to the oracle's
render: on S_CUBE a pixel is hit by some sample exactly where the oracle's image
is not black (every hit adds at least the ambient term, and no material of the
scene has a zero albedo without emission)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import rtgo
from aov_reference import reference
from conftest import ROOT
from scene_cases import make_settings
from sequence_cases import ORACLE_NONZERO, scene_json

HEADER = os.path.join(ROOT, "include", "rt_api.h")
W, H, SPP, SEED = 72, 48, 4, 3


def test_declared_exported_and_version_stays_8():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"^int\s+rt_context_render_aov_async\s*\(", text, flags=re.M)
    assert re.search(r"\}\s*rt_aov_buffers\s*;", text)
    assert re.search(r"#define\s+RT_ABI_VERSION\s+8\b", text)
    assert rtgo.lib().rt_abi_version() == 8
    assert hasattr(ctypes.CDLL(rtgo.LIB_PATH), "rt_context_render_aov_async")
    assert "rt_context_render_aov_async" in rtgo.EXPORTED_SYMBOLS


def test_ctypes_signature_and_struct_layout_match_c(tmp_path):
    f = rtgo.lib().rt_context_render_aov_async
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == [vp, i32, i32, ctypes.POINTER(rtgo.Settings), ctypes.POINTER(rtgo.Camera),
                                ctypes.POINTER(rtgo.AovBuffers), vp]
    fields = ["d_albedo", "d_normal", "d_depth", "d_coverage", "d_object"]
    assert [n for n, _ in rtgo.AovBuffers._fields_] == fields
    inc = os.path.join(ROOT, "include")
    # the declaration has exactly this type (a mismatch does not compile; compiled only, not linked)
    typ = tmp_path / "aov_type.c"
    typ.write_text('#include "rt_api.h"\n'
                   "int (*const aov_fn)(rt_context*, int32_t, int32_t, const rt_settings*, const rt_camera*,\n"
                   "                    const rt_aov_buffers*, void*) = rt_context_render_aov_async;\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", inc, "-c", str(typ), "-o", str(tmp_path / "aov_type.o")],
                   check=True)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_api.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(rt_aov_buffers));']
    lines += [f'printf("{n} %zu\\n", offsetof(rt_aov_buffers, {n}));' for n in fields]
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "aov_layout.c", tmp_path / "aov_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", inc, str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                   check=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(rtgo.AovBuffers)
    for n in fields:
        assert int(got[n]) == getattr(rtgo.AovBuffers, n).offset, n


def test_null_arguments_are_refused_without_a_device():
    lib = rtgo.lib()
    st = rtgo.default_settings()
    out = rtgo.AovBuffers()
    assert lib.rt_context_render_aov_async(None, 8, 8, ctypes.byref(st), None, ctypes.byref(out), None) == -1
    assert lib.rt_last_error()


def test_render_aov_rejects_bad_arguments_before_a_context_is_made():
    r = rtgo.ParallelRenderer(1)
    r.set_samples(2)
    scene = rtgo.Scene.from_json_text(scene_json("S_CUBE"))
    for w, h in ((0, 8), (8, 0), (-3, 4)):
        with pytest.raises(rtgo.RenderError, match="image size"):
            r.render_aov(scene, w, h)
    with pytest.raises(rtgo.RenderError, match="position"):
        r.render_aov(scene, 8, 8, camera={"lookAt": [0, 0, 0], "fov": 60})
    with pytest.raises(rtgo.RenderError, match="camera"):
        r.render_aov(scene, 8, 8, camera=3)
    r.set_samples(0)
    with pytest.raises(rtgo.RenderError, match="samples"):
        r.render_aov(scene, 8, 8)
    r.set_samples(2)
    r.set_camera("lookat")  # a look-at camera that rt_camera_frame refuses: position == lookAt
    with pytest.raises(rtgo.RenderError):
        r.render_aov(scene, 8, 8, camera={"position": [1, 1, 1], "lookAt": [1, 1, 1], "up": [0, 1, 0], "fov": 60})
    assert r._prog_ctx is None and r._r is None  # nothing touched a device


def test_reference_helper_is_the_oracles_camera_and_hits():
    text = scene_json("S_CUBE")
    ref = reference(text, W, H, SPP, SEED)
    lin, _, _ = oracle.render(rtgo.Scene.from_json_text(text), W, H,
                              make_settings(rtgo, {"samples": SPP, "max_depth": 50}, SEED))
    lit = (lin != 0).any(axis=-1)
    cov = ref["coverage"]
    assert np.array_equal(cov > 0, lit)
    assert int((cov > 0).sum()) == ORACLE_NONZERO["S_CUBE"][0] == 490
    # the definition's own consistency: coverage is hits / n, misses carry the miss values
    assert set(np.unique(cov)) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    miss = cov == 0
    assert np.all(np.isposinf(ref["depth"][miss])) and np.all(ref["object"][miss] == -1)
    assert not ref["albedo"][miss].any() and not ref["normal"][miss].any()
    assert np.all(np.isfinite(ref["depth"][~miss])) and np.all(ref["depth"][~miss] > 0.001)
    assert int(((cov > 0) & (cov < 1)).sum()) >= 50
    assert set(np.unique(ref["object"][~miss])) == {0, 1, 2, 3}
