#!/usr/bin/env python3
"""What --deflicker costs per plugin call.  One invocation, every leg --rounds times, interleaved; the lines go to
stdout and, with --log, to a file.

  vsr_regrain_measure + vsr_deflicker_pairs + the clone of the mask's rows + vsr_deflicker_apply (deflicker.apply, R = --radius) on a
  50-frame 1080p batch resident in HBM under a subtitle-band mask, against a device-to-device copy_ of the same batch timed in the same
  rounds.  The source is a still picture under fresh Gaussian noise per frame, the fill the picture without the noise plus a per-frame
  offset inside the band: every pair is open and every pixel of the band has 2 R neighbours to read.  The fill is put back before every
  timed call by a copy of the band's rows, timed as a leg of its own and subtracted.

    python scripts/bench_deflicker.py [--radius 2] [--log FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_amd  # noqa: E402,F401
from vsr_amd.backend.tools import deflicker, regrain  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import create_mask  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--radius", type=int, nargs="+", default=[2, 8])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log", default=None)
args = ap.parse_args()

log = open(args.log, "w") if args.log else None


def say(obj):
    line = json.dumps(obj)
    print(line, flush=True)
    if log:
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
offsets = torch.randint(-8, 9, (n, 1, 1), device="cuda", generator=g).to(torch.float32)
fill = src.clone()
fill[:, inside] = (plane[inside][None] + offsets).round().clamp(0, 255).to(torch.uint8)
frames = fill.clone()

sets = regrain.sets(cmask, (0, H), frames.device)
ne, _ = sets.counts.cpu().tolist()
say({"metric": "sample set", "pixels": H * W, "|E|": ne, "C": int(cmask.sum()), "rows_of_C": [sets.c0, sets.c1]})
band = slice(sets.c0, sets.c1)


def restore():
    frames[:, band].copy_(fill[:, band])


def leg(radius):
    def run():
        restore()
        deflicker.apply(frames, src, sets, radius)
    return run


legs = {"copy": lambda: frames.copy_(src), "restore": restore}
legs.update({f"restore+deflicker R={r}": leg(r) for r in args.radius})
times = {k: [] for k in legs}
for rnd in range(args.rounds):
    for name, fn in legs.items():
        ms = timed(fn, args.steps, args.warmup)
        times[name].append(ms)
        say({"metric": "kernel leg", "round": rnd, "leg": name, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / n, 5)})
copy_best, copy_worst = min(times["copy"]), max(times["copy"])
for r in args.radius:
    restore()
    deflicker.apply(frames, src, sets, r)
    torch.cuda.synchronize()
    changed = int((frames != fill).sum().item())
    best = min(times[f"restore+deflicker R={r}"]) - min(times["restore"])
    say({"metric": f"deflicker per call against copy_ ({W}x{H}, batch {n}, R = {r})", "ms_per_call": round(best, 4),
         "ms_per_frame": round(best / n, 5), "time_ratio_to_copy": round(best / copy_best, 3), "copy_ms_per_frame": round(copy_best / n, 5),
         "copy_min_max_spread": round(copy_worst / copy_best - 1, 4), "bytes_changed": changed})
if log:
    log.close()
