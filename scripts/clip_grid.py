#!/usr/bin/env python3
"""The grid behind rt_history_clip_default, CPU only: radius
in {1, 2, 3} x gamma in {1, 1.5, 2, 3} (and min_taps, min_half as given) over
the cases of tests/clip_cases.py, six one-sample frames at 144x96 by the oracle
accumulated by the host twin, RMSE against 512 samples of the last frame as the
ratio with the clip / without (tests/clip_quality.py has the set-up).

    python scripts/clip_grid.py [--min-taps 5] [--min-half 0] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "concurrent-raytracer-go_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import clip_quality as q  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-taps", type=int, default=5)
    ap.add_argument("--min-half", type=float, default=0.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    for radius in (1, 2, 3):
        for gamma in (1.0, 1.5, 2.0, 3.0):
            clip = dict(radius=radius, gamma=gamma, min_taps=args.min_taps, min_half=args.min_half)
            row = dict(clip)
            for name in ("C_FLOOR", "C_LIGHT", "S_CUBE"):
                for region, (a, b, n) in q.figures(name, clip).items():
                    row[f"{name}.{region}"] = {"pixels": n, "clip": round(a, 5), "plain": round(b, 5),
                                               "ratio": round(a / b, 3)}
            lines.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
