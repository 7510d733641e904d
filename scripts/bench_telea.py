#!/usr/bin/env python3
"""Throughput of the Telea engine (--inpaint-mode opencv) on one GPU: 1080p frames resident in HBM under the benchmark's subtitle
mask (box (950, 1069, 288, 1632) widened by create_mask, plus a second overlapping line), one workgroup per frame.  Prints the
host plan-build time, the level histogram of that mask and one JSON line per batch size."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vsr_amd  # noqa: E402,F401
from vsr_amd._lib import lib  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import create_mask  # noqa: E402
from vsr_amd.engine import TeleaEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[50, 512])
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

H, W = args.height, args.width
s = H / 1080.
boxes = [(950, 1069, 288, 1632), (880, 960, 500, 1400)]                      # ymin, ymax, xmin, xmax at 1080p
mask = create_mask((H, W), [(int(x0 * s), int(x1 * s), int(y0 * s), int(y1 * s)) for y0, y1, x0, x1 in boxes])
eng = TeleaEngine(device=0)
t0 = time.perf_counter()
h = eng.plan(mask)
t_plan = time.perf_counter() - t0
P, L = int(lib.vsr_telea_plan_pixels(h)), int(lib.vsr_telea_plan_levels(h))
level = np.zeros(P, np.int32)
lib.vsr_telea_plan_read(h, None, None, None, level.ctypes.data)
hist = np.bincount(level)[1:]
print(json.dumps({"metric": "Telea plan (host, once per mask)", "build_plus_upload_s": round(t_plan, 3), "masked_pixels": P, "levels": L,
                  "pixels_per_level": {"mean": round(float(hist.mean()), 1), "median": float(np.median(hist)), "min": int(hist.min()),
                                       "max": int(hist.max())},
                  "share_of_levels_with_at_most_2_pixels": round(float((hist <= 2).mean()), 4)}))
g = torch.Generator(device="cuda").manual_seed(3)
for n in args.batches:
    frames = torch.randint(0, 256, (n, H, W, 3), device="cuda", generator=g, dtype=torch.uint8)
    for _ in range(args.warmup):
        eng.inpaint(frames, mask)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        eng.inpaint(frames, mask)                                            # in place again: same schedule, same work
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    print(json.dumps({"metric": f"Telea inpainted frames/s ({W}x{H}, batch {n})", "value": round(n / dt, 1), "unit": "frames/s",
                      "ms_per_call": round(dt * 1e3, 2), "us_per_level": round(dt * 1e6 / L, 2), "levels": L}))
    del frames
eng.close()
