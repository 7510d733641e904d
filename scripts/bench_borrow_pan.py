#!/usr/bin/env python3
"""What --borrow-pan costs and what it borrows.  One invocation, every leg `--rounds` times, interleaved, device events;
the lines go to stdout and to --log (default profiles/borrow_pan.log).

  borrow.apply at B = 2 and B = 8 with T = 12 on scripts/bench_borrow.py's 50-frame 1080p batch resident in HBM under the benchmark's
  subtitle-band mask, plain (vsr_regrain_measure, vsr_deflicker_pairs, vsr_borrow_apply) and with P = 4 and P = 8 (vsr_regrain_measure,
  vsr_borrow_pan_search, vsr_borrow_pan_apply), and vsr_borrow_pan_search alone.  The frames are cut from a smooth textured canvas at
  `--pan` = 3 columns per frame, with Gaussian noise of sigma 2 and rows of strokes 100 levels brighter in the band that change place
  every ten frames (a caption that changes); the fill is the picture without the strokes, with another draw of the noise.  The fill is
  put back before every timed call by a copy of the band's rows, timed as a leg of its own and subtracted.

    python scripts/bench_borrow_pan.py [--log FILE]
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
from vsr_amd.backend.tools import borrow, glyph_key, regrain  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import create_mask  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--key", type=int, default=12)
ap.add_argument("--pan", type=int, default=3)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "borrow_pan.log"))
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
wide = W + args.pan * n
yy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None, None]
xx = torch.arange(wide, device="cuda", dtype=torch.float32)[None, :, None]
canvas = (110 + 40 * torch.sin(2 * np.pi * xx / 97 + yy / 31) + 30 * torch.sin(2 * np.pi * yy / 61 + xx / 43)).expand(H, wide, 3)
inside = torch.from_numpy(cmask).cuda().bool()
rows_c = np.flatnonzero(cmask.any(axis=1))
cols_c = np.flatnonzero(cmask.any(axis=0))
mid = slice(int(rows_c[0] + len(rows_c) // 4), int(rows_c[0] + 3 * len(rows_c) // 4))


def cut(t):
    """what frame t shows at column x, frame t + 1 shows at column x + pan"""
    x0 = args.pan * (n - 1 - t)
    return canvas[:, x0:x0 + W]


src = torch.stack([cut(t) for t in range(n)]) + 2.0 * torch.randn((n, H, W, 3), device="cuda", generator=g)
for t in range(n):
    strokes = torch.zeros((H, W), dtype=torch.bool, device="cuda")           # 3 px wide, every 48 columns, moved by 16 every ten frames
    for x in range(int(cols_c[0]) + 40 + 16 * ((t // 10) % 3), int(cols_c[-1]) - 40, 48):
        strokes[mid, x:x + 3] = True
    src[t][strokes & inside] += 100
src = src.round().clamp(0, 255).to(torch.uint8)
fill = src.clone()
for t in range(n):
    other = (cut(t) + 2.0 * torch.randn((H, W, 3), device="cuda", generator=g)).round().clamp(0, 255).to(torch.uint8)
    fill[t][inside] = other[inside]
del other
frames = fill.clone()

m = glyph_key.mask(cmask, frames.device)
sets = regrain.sets(cmask, (0, H), frames.device)
say({"metric": "borrow-pan", "pixels": H * W, "C": int(cmask.sum()), "rows_of_C": [m.c0, m.c1], "T": args.key, "pan": args.pan,
     "workspace_MiB": {f"B{b}P{p}": round(lib.vsr_borrow_pan_workspace_bytes(H, W, n, b, p) / 2 ** 20, 1) for b in (2, 8) for p in (4, 8)}})
band = slice(m.c0, m.c1)
work = torch.empty(lib.vsr_borrow_pan_workspace_bytes(H, W, n, 8, 8) // 8, dtype=torch.int64, device="cuda")


def restore():
    frames[:, band].copy_(fill[:, band])


def lend(b, p):
    def run():
        restore()
        os.environ[borrow.PAN_ENV] = str(p)
        borrow.apply(frames, src, sets, m, args.key, b)
    return run


def search(b, p):
    """vsr_borrow_pan_search alone: it reads src and the sets, and writes its table"""
    def run():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib.vsr_borrow_pan_search(C.c_void_p(src.data_ptr()), src.stride(0), C.c_void_p(sets.map.data_ptr()),
                                        C.c_void_p(sets.counts.data_ptr()), n, H, W, 0, H, sets.c0, sets.c1, b, p,
                                        C.c_void_p(work.data_ptr()), st))
    return run


legs = {"restore": restore}
for b in (2, 8):
    legs[f"restore+B{b}"] = lend(b, 0)
    for p in (4, 8):
        legs[f"restore+B{b}P{p}"] = lend(b, p)
        legs[f"search B{b}P{p}"] = search(b, p)
times = {k: [] for k in legs}
for r in range(args.rounds):
    for name, fn in legs.items():
        ms = timed(fn, args.steps, args.warmup)
        times[name].append(ms)
        say({"metric": "kernel leg", "round": r, "leg": name, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / n, 5)})
borrowed = {}
for b in (2, 8):
    for p in (0, 4, 8):
        lend(b, p)()
        torch.cuda.synchronize()
        changed = (frames != fill).any(dim=-1)
        borrowed[(b, p)] = int(changed.sum().item())
        say({"metric": "what the borrow did", "B": b, "P": p, "pixels borrowed (those that differ from the fill)": borrowed[(b, p)],
             "frames that borrowed": int(changed.flatten(1).any(dim=1).sum().item()), "pixels of C in the batch": int(cmask.sum()) * n})
base = min(times["restore"])
for b in (2, 8):
    plain = min(times[f"restore+B{b}"]) - base
    say({"metric": f"plain --borrow {b} ({W}x{H}, batch {n})", "ms_per_call": round(plain, 4),
         "min_max_spread": round((max(times[f"restore+B{b}"]) - base) / plain - 1, 4), "pixels_borrowed": borrowed[(b, 0)]})
    for p in (4, 8):
        best, worst = min(times[f"restore+B{b}P{p}"]) - base, max(times[f"restore+B{b}P{p}"]) - base
        find = min(times[f"search B{b}P{p}"])
        say({"metric": f"--borrow {b} --borrow-pan {p} ({W}x{H}, batch {n})", "ms_per_call": round(best, 4), "ms_per_frame": round(best / n, 5),
             "min_max_spread": round(worst / best - 1, 4), "search_ms": round(find, 4),
             "search_min_max_spread": round(max(times[f"search B{b}P{p}"]) / find - 1, 4), "measure_and_apply_ms": round(best - find, 4),
             "time_ratio_to_plain": round(best / plain, 2), "pixels_borrowed": borrowed[(b, p)]})
os.environ.pop(borrow.PAN_ENV, None)
log.close()
