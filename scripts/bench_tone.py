#!/usr/bin/env python3
"""What --tone-match costs next to its siblings.  One invocation, every leg `--rounds` times, interleaved; the lines go to
stdout and to --log (default profiles/tone.log).

  vsr_tone_apply (S = 100), vsr_regrain_measure + vsr_regrain_apply (P = 100) and the deflicker pass (R = 2) on the same 50-frame 1080p
  batch resident in HBM under the benchmark's subtitle-band mask, against a device-to-device copy_ of the batch timed in the same
  rounds.  The source is a smooth picture with Gaussian noise; the fill is the picture without the noise, nine levels darker and with a
  per-frame offset inside the band, so that every frame has a step to level, a deficit of grain and flicker.  The fill is put back before
  every timed call by a copy of the band's rows, timed as a leg of its own and subtracted.

    python scripts/bench_tone.py [--log FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_amd  # noqa: E402,F401
from vsr_amd._lib import check, lib  # noqa: E402
from vsr_amd.backend.tools import deflicker, regrain, tone_match  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import create_mask  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "tone.log"))
args = ap.parse_args()

os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
log = open(args.log, "w")


def say(obj):
    line = json.dumps(obj)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def timed(fn, steps, warmup):
    """ms per call by device events around `steps` calls"""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


H, W, n = args.height, args.width, args.batch
s = H / 1080.
box = (950, 1069, 288, 1632)                                                 # the benchmark's subtitle band at 1080p
mask = create_mask((H, W), [(int(box[2] * s), int(box[3] * s), int(box[0] * s), int(box[1] * s))])
cmask = (mask != 0).astype(np.uint8)
g = torch.Generator(device="cuda").manual_seed(3)
yy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None, None]
xx = torch.arange(W, device="cuda", dtype=torch.float32)[None, :, None]
plane = (60 + 0.05 * xx + 0.08 * yy).expand(H, W, 3)
src = (plane[None] + 6.0 * torch.randn((n, H, W, 3), device="cuda", generator=g)).round().clamp(0, 255).to(torch.uint8)
inside = torch.from_numpy(cmask).cuda().bool()
fill = src.clone()
for t in range(n):
    fill[t][inside] = (plane - 9 + (t % 5 - 2)).round().to(torch.uint8)[inside]
frames = fill.clone()
P = lambda t: C.c_void_p(t.data_ptr())                                        # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)          # noqa: E731

bands = tone_match.sets(cmask, (0, H), frames.device)
sets = regrain.sets(cmask, (0, H), frames.device)
say({"metric": "seam bands", "pixels": H * W, "C": int(cmask.sum()), "rows_of_C": [bands.c0, bands.c1], "cells_listed": bands.ncells,
     "cells": -(-H // 8) * -(-W // 8), "workspace_MiB": round(lib.vsr_tone_workspace_bytes(H, W, n) / 2 ** 20, 1)})
cm = torch.from_numpy(cmask).cuda()
tmp, cnt = torch.empty((H, W), dtype=torch.uint8, device="cuda"), torch.empty(3, dtype=torch.int64, device="cuda")
lst = torch.empty(-(-H // 8) * -(-W // 8), dtype=torch.int32, device="cuda")
a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
check(lib.vsr_tone_sets(P(cm), H, W, 0, H, P(tmp), P(cnt), P(lst), stream()))
a0.record()
check(lib.vsr_tone_sets(P(cm), H, W, 0, H, P(tmp), P(cnt), P(lst), stream()))
a1.record()
a1.synchronize()
say({"metric": "vsr_tone_sets (once per mask)", "ms": round(a0.elapsed_time(a1), 3)})

band = slice(bands.c0, bands.c1)


def restore():
    frames[:, band].copy_(fill[:, band])


def leg(fn):
    def run():
        restore()
        fn()
    return run


legs = {"copy": lambda: frames.copy_(src), "restore": restore,
        "restore+tone": leg(lambda: tone_match.apply(frames, src, bands, 100)),
        "restore+regrain": leg(lambda: regrain.apply(frames, src, sets, 100)),
        "restore+deflicker": leg(lambda: deflicker.apply(frames, src, sets, 2))}
times = {k: [] for k in legs}
for r in range(args.rounds):
    for name, fn in legs.items():
        ms = timed(fn, args.steps, args.warmup)
        times[name].append(ms)
        say({"metric": "kernel leg", "round": r, "leg": name, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / n, 5)})
for name, fn in list(legs.items())[2:]:
    fn()
    torch.cuda.synchronize()
    say({"metric": "bytes of the batch the pass changed", "leg": name[8:], "value": int((frames != fill).sum().item())})
copy_best, copy_worst = min(times["copy"]), max(times["copy"])
for name in ("tone", "regrain", "deflicker"):
    best = min(times["restore+" + name]) - min(times["restore"])
    say({"metric": f"{name} against copy_ ({W}x{H}, batch {n})", "ms_per_call": round(best, 4), "ms_per_frame": round(best / n, 5),
         "time_ratio_to_copy": round(best / copy_best, 3), "copy_ms_per_frame": round(copy_best / n, 5),
         "copy_min_max_spread": round(copy_worst / copy_best - 1, 4)})
log.close()
