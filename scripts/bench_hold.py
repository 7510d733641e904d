#!/usr/bin/env python3
"""What --glyph-hold costs and what it steadies.  The lines go to stdout and to --log (default profiles/hold.log).

  default    on the GPU, one invocation, every leg `--rounds` times, interleaved: glyph_key.apply at T = 12 with K = 0 (vsr_key_apply,
             the path without the option: the yardstick), K = 2 and K = 8 (vsr_key_apply_hold) on scripts/bench_key.py's 50-frame
             1080p batch and mask, against a device-to-device copy_ of the batch timed in the same rounds.  The fill is put back before
             every timed call by a copy of the band's rows, timed as a leg of its own and subtracted.
  --flicker  on the CPU, with the statement alone (tests/_hold_statement.py, on the rows of C): the same picture, band and strokes with
             the strokes' contrast alternating about T from frame to frame (14 and 10 levels at T = 12), without noise and with
             the bench's noise of sigma 6: the pixels of C whose weight a changes between consecutive frames, and the share of C handed
             back to the source, at K = 0 and K = 2.

    python scripts/bench_hold.py [--flicker] [--log FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--key", type=int, default=12)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--flicker", action="store_true")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "hold.log"))
args = ap.parse_args()

os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
log = open(args.log, "a" if args.flicker else "w")


def say(obj):
    line = json.dumps(obj)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


H, W, n = args.height, args.width, args.batch
s = H / 1080.
box = (950, 1069, 288, 1632)                                                 # the benchmark's subtitle band at 1080p


def band_and_strokes(cmask):
    """bench_key.py's strokes: 3 px wide, every 16 columns, the middle half of the band"""
    rows_c = np.flatnonzero(cmask.any(axis=1))
    cols_c = np.flatnonzero(cmask.any(axis=0))
    strokes = np.zeros((H, W), bool)
    mid = slice(int(rows_c[0] + len(rows_c) // 4), int(rows_c[0] + 3 * len(rows_c) // 4))
    for x in range(int(cols_c[0]) + 40, int(cols_c[-1]) - 40, 16):
        strokes[mid, x:x + 3] = True
    return strokes & (cmask != 0)


def flicker(cmask):
    from tests import _hold_statement as hs

    T = args.key
    c0, c1 = int(np.flatnonzero(cmask.any(axis=1))[0]), int(np.flatnonzero(cmask.any(axis=1))[-1]) + 1
    strokes = band_and_strokes(cmask)[c0:c1]
    inside = cmask[c0:c1] != 0
    yy, xx = np.mgrid[c0:c1, 0:W]
    plane = (60 + 0.05 * xx + 0.08 * yy)[None, :, :, None] + np.zeros((n, 1, 1, 3))
    hi, lo = T + 2, T - 2
    for sigma in (0.0, 6.0):
        rng = np.random.default_rng(3)
        src = plane + sigma * rng.standard_normal(plane.shape)
        for t in range(n):
            if t % 5:
                src[t][strokes] += hi if t % 2 else lo
        src = np.clip(np.rint(src), 0, 255).astype(np.uint8)
        fill = src.copy()
        fill[:, inside] = np.rint(plane).astype(np.uint8)[:, inside]
        for K in (0, 2):
            info = []
            out = hs.hold(fill, src, cmask, T, K, y0=c0, info=info)          # the rows of C: the full-frame result's
            S, Wk, Z, a = info[0]
            a = a[:, inside]
            back = (out == src).all(axis=-1)[:, inside]
            say({"metric": "flicker of the weight", "sigma": sigma, "T": T, "K": K, "stroke contrast": [hi, lo], "pixels of C": int(inside.sum()),
                 "frames": n, "strong seeds": int(S.sum()), "weak seeds": int(Wk.sum()), "held seeds": int(Z.sum()),
                 "pixels of C whose a changes between consecutive frames": int((a[1:] != a[:-1]).sum()),
                 "pixels of C that switch between a = 0 and a > 0": int(((a[1:] > 0) != (a[:-1] > 0)).sum()),
                 "share of C handed back to the source": round(float(back.mean()), 4),
                 "share of C with a = 0": round(float((a == 0).mean()), 4)})


import vsr_amd  # noqa: E402,F401
from vsr_amd.backend.tools.inpaint_tools import create_mask  # noqa: E402

mask = create_mask((H, W), [(int(box[2] * s), int(box[3] * s), int(box[0] * s), int(box[1] * s))])
cmask = (mask != 0).astype(np.uint8)
if args.flicker:
    flicker(cmask)
    log.close()
    sys.exit(0)

import torch  # noqa: E402

from vsr_amd._lib import lib  # noqa: E402
from vsr_amd.backend.tools import glyph_key  # noqa: E402


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


g = torch.Generator(device="cuda").manual_seed(3)
yy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None, None]
xx = torch.arange(W, device="cuda", dtype=torch.float32)[None, :, None]
plane = (60 + 0.05 * xx + 0.08 * yy).expand(H, W, 3)
inside = torch.from_numpy(cmask).cuda().bool()
strokes = torch.from_numpy(band_and_strokes(cmask)).cuda()
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
say({"metric": "glyph hold", "pixels": H * W, "C": int(cmask.sum()), "rows_of_C": [m.c0, m.c1], "T": args.key,
     "workspace_MiB": {"K = 0": round(lib.vsr_key_workspace_bytes(H, W, n) / 2 ** 20, 1),
                       "K > 0": round(lib.vsr_key_hold_workspace_bytes(H, W, n) / 2 ** 20, 1)},
     "used_MiB_of_three_bitmaps": round(3 * n * (m.c1 - m.c0 + 2) * ((W + 63) // 64) * 8 / 2 ** 20, 2)})
band = slice(m.c0, m.c1)


def restore():
    frames[:, band].copy_(fill[:, band])


def leg(k):
    def run():
        restore()
        glyph_key.apply(frames, src, m, args.key, hold=k)
    return run


legs = {"copy": lambda: frames.copy_(src), "restore": restore, "restore+K0": leg(0), "restore+K2": leg(2), "restore+K8": leg(8)}
times = {k: [] for k in legs}
for r in range(args.rounds):
    for name, fn in legs.items():
        ms = timed(fn, args.steps, args.warmup)
        times[name].append(ms)
        say({"metric": "kernel leg", "round": r, "leg": name, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / n, 5)})
copy_best, copy_worst = min(times["copy"]), max(times["copy"])
base = min(times["restore+K0"]) - min(times["restore"])
for k in (0, 2, 8):
    legs[f"restore+K{k}"]()
    torch.cuda.synchronize()
    kept = (frames == src)[:, inside].all(dim=-1)
    best = min(times[f"restore+K{k}"]) - min(times["restore"])
    say({"metric": f"K = {k} against K = 0 and copy_ ({W}x{H}, batch {n})", "ms_per_call": round(best, 4), "ms_per_frame": round(best / n, 5),
         "time_ratio_to_K0": round(best / base, 3), "time_ratio_to_copy": round(best / copy_best, 3),
         "copy_ms_per_call": round(copy_best, 4), "copy_min_max_spread": round(copy_worst / copy_best - 1, 4),
         "pixels of C handed back to the source": int(kept.sum().item()), "pixels of C": int(kept.numel())})
log.close()
