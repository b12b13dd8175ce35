#!/usr/bin/env python3
"""Writes tests/golden/degenerate_scenes.txt: the scenes of
tests/degenerate_cases.py as the C ABI sees them, for the sanitizer driver
(tests/c/sanitize_driver.cpp), which has no Python.  Regenerate when the
scenes change (tests/test_degenerate_cpu.py compares the file with them)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(ROOT, "concurrent-raytracer-go_amd")]
import degenerate_cases  # noqa: E402
import rtgo  # noqa: E402

text = degenerate_cases.fixture_text(rtgo)
with open(os.path.join(HERE, "degenerate_scenes.txt"), "w") as f:
    f.write(text)
print("wrote", len(degenerate_cases.SCENES), "scenes,", len(text), "bytes")
