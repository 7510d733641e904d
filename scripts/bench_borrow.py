#!/usr/bin/env python3
"""What --borrow costs and what it borrows.  One invocation, every leg `--rounds` times, interleaved, device events; the
lines go to stdout and to --log (default profiles/borrow.log).

  borrow.apply (vsr_regrain_measure, vsr_deflicker_pairs, vsr_borrow_apply) at B = 2 and B = 8 with T = 12 on a 50-frame 1080p batch
  resident in HBM under the benchmark's subtitle-band mask, against a device-to-device copy_ of the batch and --glyph-key 12
  (vsr_key_apply) timed in the same rounds.  The source is a smooth picture that stands still, with Gaussian noise of sigma 2 and rows
  of strokes 100 levels brighter in the band that change place every ten frames (a caption that changes); the fill is the picture
  without the strokes, with another draw of the noise.  The fill is put back before every timed call by a copy of the band's rows,
  timed as a leg of its own and subtracted.

    python scripts/bench_borrow.py [--log FILE]
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
from vsr_amd._lib import lib  # noqa: E402
from vsr_amd.backend.tools import borrow, glyph_key, regrain  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import create_mask  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--key", type=int, default=12)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "borrow.log"))
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
inside = torch.from_numpy(cmask).cuda().bool()
rows_c = np.flatnonzero(cmask.any(axis=1))
cols_c = np.flatnonzero(cmask.any(axis=0))
mid = slice(int(rows_c[0] + len(rows_c) // 4), int(rows_c[0] + 3 * len(rows_c) // 4))
src = plane[None] + 2.0 * torch.randn((n, H, W, 3), device="cuda", generator=g)
for t in range(n):
    strokes = torch.zeros((H, W), dtype=torch.bool, device="cuda")           # 3 px wide, every 48 columns, moved by 16 every ten frames
    for x in range(int(cols_c[0]) + 40 + 16 * ((t // 10) % 3), int(cols_c[-1]) - 40, 48):
        strokes[mid, x:x + 3] = True
    src[t][strokes & inside] += 100
src = src.round().clamp(0, 255).to(torch.uint8)
fill = src.clone()
other = (plane[None] + 2.0 * torch.randn((n, H, W, 3), device="cuda", generator=g)).round().clamp(0, 255).to(torch.uint8)
fill[:, inside] = other[:, inside]
del other
frames = fill.clone()

m = glyph_key.mask(cmask, frames.device)
sets = regrain.sets(cmask, (0, H), frames.device)
say({"metric": "borrow", "pixels": H * W, "C": int(cmask.sum()), "rows_of_C": [m.c0, m.c1], "T": args.key,
     "workspace_MiB": round(lib.vsr_borrow_workspace_bytes(H, W, n) / 2 ** 20, 1)})
band = slice(m.c0, m.c1)


def restore():
    frames[:, band].copy_(fill[:, band])


def leg(fn):
    def run():
        restore()
        fn()
    return run


legs = {"copy": lambda: frames.copy_(src), "restore": restore,
        "restore+key": leg(lambda: glyph_key.apply(frames, src, m, args.key, hold=0)),
        "restore+borrow2": leg(lambda: borrow.apply(frames, src, sets, m, args.key, 2)),
        "restore+borrow8": leg(lambda: borrow.apply(frames, src, sets, m, args.key, 8))}
times = {k: [] for k in legs}
for r in range(args.rounds):
    for name, fn in legs.items():
        ms = timed(fn, args.steps, args.warmup)
        times[name].append(ms)
        say({"metric": "kernel leg", "round": r, "leg": name, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / n, 5)})
for b in (2, 8):
    legs[f"restore+borrow{b}"]()
    torch.cuda.synchronize()
    changed = (frames != fill).any(dim=-1)
    say({"metric": "what the borrow did", "B": b, "pixels borrowed (those that differ from the fill)": int(changed.sum().item()),
         "frames that borrowed": int(changed.flatten(1).any(dim=1).sum().item()), "pixels of C in the batch": int(cmask.sum()) * n})
copy_best, copy_worst = min(times["copy"]), max(times["copy"])
for name in ("key", "borrow2", "borrow8"):
    best = min(times["restore+" + name]) - min(times["restore"])
    worst = max(times["restore+" + name]) - min(times["restore"])
    say({"metric": f"{name} against copy_ ({W}x{H}, batch {n})", "ms_per_call": round(best, 4), "ms_per_frame": round(best / n, 5),
         "min_max_spread": round(worst / best - 1, 4), "time_ratio_to_copy": round(best / copy_best, 3),
         "copy_ms_per_frame": round(copy_best / n, 5), "copy_min_max_spread": round(copy_worst / copy_best - 1, 4)})
log.close()
