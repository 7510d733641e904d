#!/usr/bin/env python3
"""What --text-detect strokes costs.  One invocation; the lines go to stdout and to --log (default profiles/strokes.log).

  StrokeTextDetection.predict_batch_device on 8 frames of 1080p resident in HBM: `--steps` timed calls after `--warmup`, each by a host
  clock around a call that ends in its read-back (min, median, max: the spread), per frame.  Then the legs of a call by device events,
  each `--steps` times after warm-up, `--rounds` rounds interleaved: vsr_strokes_cells (the bytes it needs: every frame byte once, the
  two count planes written once) against a device-to-device copy_ of as many frame bytes (a copy reads and writes every byte, so its
  rate counts both), vsr_strokes_text, the 8 labellings (vsr_det_launch_ccl), and the read-back (host clock).  One batch of 1080p is 50 MB
  and stays in the 256 MiB Infinity Cache from call to call, so the cells kernel and the copy are timed a second time over a clip larger
  than that cache, batch after batch: the rate from HBM.  The frames are a moving wave with noise and two lines of block text with an
  outline.

    python scripts/bench_strokes.py [--batch N] [--steps 10] [--warmup 3] [--rounds 3] [--clip-batches 16] [--log FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_amd  # noqa: E402,F401
from vsr_amd._lib import check, lazy, lib  # noqa: E402
from vsr_amd.backend.tools import stroke_det as sd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--clip-batches", type=int, default=16, help="batches of the clip of the from-HBM legs (16 x 8 frames of 1080p: 796 MB)")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "strokes.log"))
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


# (the 5 x 7 block font and the glyph painter of tests/_strokes_statement.py, FONT and glyph_mask, copied: a script imports no test)
FONT = {"E": "#####/#..../#..../####./#..../#..../#####", "H": "#...#/#...#/#...#/#####/#...#/#...#/#...#",
        "L": "#..../#..../#..../#..../#..../#..../#####", "O": ".###./#...#/#...#/#...#/#...#/#...#/.###.",
        "N": "#...#/##..#/#.#.#/#.#.#/#..##/#...#/#...#", "T": "#####/..#../..#../..#../..#../..#../..#..",
        "A": ".###./#...#/#...#/#####/#...#/#...#/#...#", "I": "#####/..#../..#../..#../..#../..#../#####"}


def glyphs(text, k, H, W, y0, x0):
    m = np.zeros((H, W), bool)
    for n, ch in enumerate(text):
        if ch != " ":
            g = np.array([[c == "#" for c in row] for row in FONT[ch].split("/")])
            g = np.repeat(np.repeat(g, k, axis=0), k, axis=1)
            xs = x0 + n * 6 * k
            m[y0:y0 + g.shape[0], xs:xs + g.shape[1]] |= g[:H - y0, :max(W - xs, 0)]
    return m


n, H, W = args.batch, args.height, args.width
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(5)
yy = torch.arange(H, device=dev)[:, None]
xx = torch.arange(W, device=dev)[None, :]
k = max(H // 180, 2)                                                         # 1080p: strokes of 6 pixels, 3 at the analysis scale
lines = [(glyphs("HELLO NATION", k, H, W, H - 16 * k, W // 2 - 36 * k), 235, 16), (glyphs("NOT A LINE", k, H, W, H - 26 * k, W // 2 - 30 * k), 20, 240)]
frames = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
for f in range(n):
    t = (xx + yy + 5 * f) % 256
    wave = torch.minimum(t, 256 - t).to(torch.float32)
    frames[f] = (wave[..., None] * 0.75 + 4.0 * torch.randn((H, W, 3), device=dev, generator=gen)).round().clamp(0, 255).to(torch.uint8)
    for m, fg, rim in lines:
        grown = torch.from_numpy(m).to(dev)[None, None].float()
        grown = torch.nn.functional.max_pool2d(grown, 2 * (k // 2) + 1, 1, k // 2)[0, 0] > 0
        frames[f][grown] = rim
        frames[f][torch.from_numpy(m).to(dev)] = fg
torch.cuda.synchronize()

det = sd.StrokeTextDetection(0)
first = det.predict_batch_device(frames)
b = det._buffers[(n, H, W)]
frame_bytes, plane_bytes = n * H * W * 3, 2 * n * b.hc * b.wc
say({"metric": "stroke text detector", "frames": [n, H, W], "F": b.F, "cells": [b.hc, b.wc], "frame_MB": round(frame_bytes / 1e6, 1),
     "count_planes_MB": round(plane_bytes / 1e6, 3), "read_back_MB": round(b.out.numel() / 1e6, 3), "boxes_per_frame": [len(r["dt_scores"]) for r in first],
     "boxes_frame_0": first[0]["dt_polys"][:, [0, 2]].reshape(-1, 4).tolist()})

calls = []
for i in range(args.warmup + args.steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    det.predict_batch_device(frames)
    calls.append((time.perf_counter() - t0) * 1e3)
calls = calls[args.warmup:]
say({"metric": f"predict_batch_device, {n} frames of {W}x{H} per call (host clock around a call that ends in its read-back)", "calls": len(calls),
     "ms_per_frame_min": round(min(calls) / n, 4), "ms_per_frame_median": round(statistics.median(calls) / n, 4),
     "ms_per_frame_max": round(max(calls) / n, 4), "ms_per_call_all": [round(c, 3) for c in calls]})

p = lambda t: C.c_void_p(t.data_ptr())                                          # noqa: E731
base, cells = b.out.data_ptr(), b.hc * b.wc
cv_p, ch_p = C.c_void_p(base), C.c_void_p(base + n * cells)
stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
dst = torch.empty_like(frames)


def leg_cells():
    check(lazy("vsr_strokes_cells")(p(frames), H * W * 3, n, H, W, b.F, sd.S, sd.CONTRAST, cv_p, ch_p, stream))


def leg_text():
    check(lazy("vsr_strokes_text")(cv_p, ch_p, n, b.hc, b.wc, sd.WX, sd.WY, sd.NV, sd.NH, p(b.text), stream))


def leg_label():
    for f in range(n):
        at = base + b.plane_bytes + 4 * f * b.frame_ints
        check(lib.vsr_det_launch_ccl(p(b.text[f]), b.hc, b.wc, C.c_float(0.5), p(b.labels), p(b.work), C.c_void_p(at + 16), b.cap, C.c_void_p(at), stream))


# the same kernel fed from HBM: a clip of `--clip-batches` batches, larger than the 256 MiB Infinity Cache, one batch after the other, so
# that no call finds its frames in a cache (the legs above run on one batch of 50 MB again and again, which stays in that cache)
clip = frames.repeat(args.clip_batches, 1, 1, 1)
dst_clip = torch.empty_like(clip)
turn = {"cells": 0, "copy": 0}


def leg_cells_clip():
    j = turn["cells"] = (turn["cells"] + 1) % args.clip_batches
    check(lazy("vsr_strokes_cells")(p(clip[j * n]), H * W * 3, n, H, W, b.F, sd.S, sd.CONTRAST, cv_p, ch_p, stream))


def leg_copy_clip():
    j = turn["copy"] = (turn["copy"] + 1) % args.clip_batches
    dst_clip[j * n:(j + 1) * n].copy_(clip[j * n:(j + 1) * n])


legs = {"copy": lambda: dst.copy_(frames), "cells": leg_cells, "text": leg_text, "labellings": leg_label, "copy, from HBM": leg_copy_clip,
        "cells, from HBM": leg_cells_clip}
times = {name: [] for name in legs}
for r in range(args.rounds):
    for name, fn in legs.items():
        ms = timed(fn, args.steps, args.warmup)
        times[name].append(ms)
        say({"metric": "leg", "round": r, "leg": name, "ms_per_call": round(ms, 4)})
back = []
for _ in range(args.warmup + args.steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b.out.cpu()
    back.append((time.perf_counter() - t0) * 1e3)
back = back[args.warmup:]
copy_ms, cells_ms = min(times["copy"]), min(times["cells"])
say({"metric": f"legs of one call ({n} frames of {W}x{H}), best of {args.rounds} rounds of {args.steps} calls", "cells_ms": round(cells_ms, 4),
     "cells_GB_per_s": round((frame_bytes + plane_bytes) / cells_ms / 1e6, 1), "cells_ms_per_frame": round(cells_ms / n, 4),
     "cells_ms_all": [round(t, 4) for t in times["cells"]], "copy_ms": round(copy_ms, 4),
     "copy_GB_per_s_read_plus_write": round(2 * frame_bytes / copy_ms / 1e6, 1), "text_ms": round(min(times["text"]), 4),
     "labellings_ms": round(min(times["labellings"]), 4), "read_back_ms_min": round(min(back), 4), "read_back_ms_median": round(statistics.median(back), 4),
     "sum_of_legs_ms_per_frame": round((cells_ms + min(times["text"]) + min(times["labellings"]) + min(back)) / n, 4)})
hbm_ms, hbm_copy = min(times["cells, from HBM"]), min(times["copy, from HBM"])
say({"metric": f"the cells kernel fed from HBM (a clip of {args.clip_batches * n} frames, {round(clip.numel() / 1e6)} MB, batch after batch)",
     "cells_ms": round(hbm_ms, 4), "cells_GB_per_s": round((frame_bytes + plane_bytes) / hbm_ms / 1e6, 1), "cells_ms_per_frame": round(hbm_ms / n, 4),
     "cells_ms_all": [round(t, 4) for t in times["cells, from HBM"]], "copy_ms": round(hbm_copy, 4),
     "copy_GB_per_s_read_plus_write": round(2 * frame_bytes / hbm_copy / 1e6, 1), "time_ratio_to_copy": round(hbm_ms / hbm_copy, 3)})
log.close()
