"""Progressive rendering, the parts that need no GPU: the
new C entry points resolve in librtgo.so with the signatures the Python
wrappers declare, and the CLI refuses bad progressive flags with exit 2
before any device state exists."""
import ctypes
import os
import subprocess

import pytest

import rtgo
from conftest import ROOT

EXE = os.path.join(ROOT, "concurrent-raytracer-go_amd", "build", "raytracer")
SCENE = os.path.join(ROOT, "scenes", "sphere_reflections_light_facing.json")

vp, i32 = ctypes.c_void_p, ctypes.c_int32
SIGNATURES = {
    "rt_context_progressive_begin": (ctypes.c_int, [vp, i32, i32, ctypes.POINTER(rtgo.Settings), i32, i32, i32]),
    "rt_context_progressive_add_async": (ctypes.c_int, [vp, i32, vp, vp, vp]),
    "rt_context_progressive_samples": (ctypes.c_int64, [vp]),
    "rt_context_progressive_end": (ctypes.c_int, [vp]),
    "rt_rgba_delta_async": (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp, vp]),
}


def test_new_symbols_resolve_with_their_signatures():
    lib = rtgo.lib()
    raw = ctypes.CDLL(rtgo.LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        assert hasattr(raw, name), name
        assert name in rtgo.EXPORTED_SYMBOLS, name
        f = getattr(lib, name)
        assert f.restype is res and list(f.argtypes) == args, name
    assert lib.rt_abi_version() >= 7
    for m in ("progressive_begin", "progressive_add", "progressive_samples", "progressive_end"):
        assert callable(getattr(rtgo.Context, m))
    assert callable(rtgo.rgba_delta_async) and callable(rtgo.ParallelRenderer.render_progressive)


def test_entry_points_refuse_null_arguments_without_a_device():
    lib = rtgo.lib()
    assert lib.rt_context_progressive_samples(None) == -1
    assert lib.rt_context_progressive_begin(None, 8, 8, None, 0, 1, 0) == -1
    assert lib.rt_context_progressive_add_async(None, 1, None, None, None) == -1
    assert lib.rt_context_progressive_end(None) == -1
    assert lib.rt_rgba_delta_async(None, None, 4, None, None) == -1
    assert lib.rt_last_error()


BAD_FLAGS = [
    ("pass_samples_zero", ["--pass-samples", "0"]),
    ("pass_samples_not_a_number", ["--pass-samples", "x"]),
    ("time_budget_not_a_number", ["--pass-samples", "2", "--time-budget", "x"]),
    ("time_budget_negative", ["--pass-samples", "2", "--time-budget", "-1"]),
    ("converge_negative", ["--pass-samples", "2", "--converge", "-1"]),
    ("two_devices", ["--pass-samples", "2", "--devices", "2"]),
    ("two_devices_flag_first", ["--devices", "2", "--pass-samples", "2"]),
    ("no_samples_to_render", ["--pass-samples", "2", "--samples", "0"]),
    ("time_budget_without_pass_samples", ["--time-budget", "1"]),
]


@pytest.mark.parametrize("name,flags", BAD_FLAGS, ids=[c[0] for c in BAD_FLAGS])
def test_cli_refuses_bad_progressive_flags(tmp_path, name, flags):
    out = tmp_path / "o.png"
    p = subprocess.run([EXE, SCENE, str(out), "8", "8"] + flags, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2, p.stdout + p.stderr
    assert p.stderr.strip()  # says why
    assert "Loading scene" not in p.stdout and not out.exists()  # refused before anything was done
