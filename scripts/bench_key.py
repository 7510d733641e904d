#!/usr/bin/env python3
"""What --glyph-key costs.  One invocation, every leg `--rounds` times, interleaved; the lines go to stdout and to --log
(default profiles/key.log).

  vsr_key_apply (T = 12) on a 50-frame 1080p batch resident in HBM under the benchmark's subtitle-band mask, against a device-to-device
  copy_ of the batch timed in the same rounds, and vsr_tone_apply (S = 100) on the same batch for scale.  The source is a smooth picture
  with Gaussian noise and, on four frames of five, rows of strokes 100 levels brighter in the band (a subtitle); the fill is the picture
  without the noise and without the strokes, so that the key has glyphs to fill, a band to hand back around them and whole frames to
  hand back.  The fill is put back before every timed call by a copy of the band's rows, timed as a leg of its own and subtracted.

    python scripts/bench_key.py [--log FILE]
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
from vsr_amd.backend.tools import glyph_key, tone_match  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import create_mask  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--key", type=int, default=12)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "key.log"))
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
strokes = torch.zeros((H, W), dtype=torch.bool, device="cuda")               # 3 px wide, every 16 columns, the middle half of the band
mid = slice(int(rows_c[0] + len(rows_c) // 4), int(rows_c[0] + 3 * len(rows_c) // 4))
for x in range(int(cols_c[0]) + 40, int(cols_c[-1]) - 40, 16):
    strokes[mid, x:x + 3] = True
strokes &= inside
src = plane[None] + 6.0 * torch.randn((n, H, W, 3), device="cuda", generator=g)
for t in range(n):
    if t % 5:
        src[t][strokes] += 100
src = src.round().clamp(0, 255).to(torch.uint8)
fill = src.clone()
for t in range(n):
    fill[t][inside] = plane.round().to(torch.uint8)[inside]
frames = fill.clone()

m = glyph_key.mask(cmask, frames.device)
bands = tone_match.sets(cmask, (0, H), frames.device)
say({"metric": "glyph key", "pixels": H * W, "C": int(cmask.sum()), "rows_of_C": [m.c0, m.c1], "T": args.key,
     "workspace_MiB": round(lib.vsr_key_workspace_bytes(H, W, n) / 2 ** 20, 1)})
band = slice(m.c0, m.c1)


def restore():
    frames[:, band].copy_(fill[:, band])


def leg(fn):
    def run():
        restore()
        fn()
    return run


legs = {"copy": lambda: frames.copy_(src), "restore": restore,
        "restore+key": leg(lambda: glyph_key.apply(frames, src, m, args.key)),
        "restore+tone": leg(lambda: tone_match.apply(frames, src, bands, 100))}
times = {k: [] for k in legs}
for r in range(args.rounds):
    for name, fn in legs.items():
        ms = timed(fn, args.steps, args.warmup)
        times[name].append(ms)
        say({"metric": "kernel leg", "round": r, "leg": name, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / n, 5)})
legs["restore+key"]()
torch.cuda.synchronize()
kept = (frames == src)[:, inside].all(dim=-1)
say({"metric": "what the key did", "bytes of the batch changed": int((frames != fill).sum().item()),
     "pixels of C handed back to the source": int(kept.sum().item()), "pixels of C": int(kept.numel()),
     "frames equal to their source": int((frames == src).flatten(1).all(dim=1).sum().item())})
copy_best, copy_worst = min(times["copy"]), max(times["copy"])
for name in ("key", "tone"):
    best = min(times["restore+" + name]) - min(times["restore"])
    say({"metric": f"{name} against copy_ ({W}x{H}, batch {n})", "ms_per_call": round(best, 4), "ms_per_frame": round(best / n, 5),
         "time_ratio_to_copy": round(best / copy_best, 3), "copy_ms_per_frame": round(copy_best / n, 5),
         "copy_min_max_spread": round(copy_worst / copy_best - 1, 4)})
log.close()
