#!/usr/bin/env python3
"""Throughput of the exemplar fill (--inpaint-mode opencv --opencv-fill exemplar) on one GPU, in one process: 1080p frames resident in
HBM under a 1920 x 100 box near the bottom, as a 50-frame batch and as a 512-frame resident clip (Telea's published setting), Telea's
fill on the same batches beside it, and the time of every kernel of one call from HIP events (the call is replayed launch by launch
through vsr_exemplar_run_stage).  The frames are a striped texture with noise: on flat or on purely random frames the early exit of
k_ex_search would see an easier job than on a picture.  One JSON line per figure."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vsr_amd  # noqa: E402,F401
from vsr_amd import _lib  # noqa: E402
from vsr_amd.engine import ExemplarEngine, TeleaEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[50, 512])
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

H, W = args.height, args.width
ITERS, PASSES = 4, 4
mask = np.zeros((H, W), np.uint8)
mask[H - 130 * H // 1080:H - 30 * H // 1080] = 255                          # rows 950..1049 at 1080p, the whole width
ex, te = ExemplarEngine(device=0), TeleaEngine(device=0)
t0 = time.perf_counter()
ex.plan(mask)
t_plan = time.perf_counter() - t0
levels = ex.plan_levels(mask)
print(json.dumps({"metric": "exemplar plan (host, once per mask)", "build_plus_upload_s": round(t_plan, 3), "levels": len(levels),
                  "per_level": [{"H": l["H"], "W": l["W"], "sources": len(l["S"]), "targets": len(l["D"]), "tiles": len(l["tiles"])} for l in levels]}))


def texture(n, gen):
    y = torch.arange(H, device="cuda").view(1, H, 1)
    x = torch.arange(W, device="cuda").view(1, 1, W)
    base = 110 + 60 * (((x + y // 2) // 4) % 2) + 30 * ((y // 6) % 2)
    hole = torch.from_numpy(mask != 0).cuda()
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
    for f0 in range(0, n, 32):                                               # in pieces: the int64 intermediates of 512 frames are large
        noise = torch.randint(-8, 9, (min(32, n - f0), H, W), device="cuda", generator=gen)
        piece = torch.stack([base + noise, base // 2 + 60 + noise, 255 - base + noise], -1).clamp_(0, 255).to(torch.uint8)
        piece[:, hole] = 255
        out[f0:f0 + piece.shape[0]] = piece
    return out


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    each = []
    for _ in range(args.steps):                                              # every step on its own, so that the spread can be stated
        t0 = time.perf_counter()
        fn()                                                                 # in place again: the same plan, the same work
        torch.cuda.synchronize()
        each.append(time.perf_counter() - t0)
    return sum(each) / len(each), min(each), max(each)


def stages(nl):
    """the launches of one call, in order: (kernel, stage, level, iteration, pass, from_b)"""
    out = [("k_ex_down", _lib.EX_DOWN, l, 0, 0, 0) for l in range(1, nl)]
    for l in range(nl - 1, -1, -1):
        if l == nl - 1:
            out += [("k_ex_init", _lib.EX_INIT, l, 0, 0, 0), ("k_ex_up", _lib.EX_UP, l, 0, 0, 0)]
        else:
            out += [("k_ex_up", _lib.EX_UP, l, 0, 0, 0), ("k_ex_vote", _lib.EX_VOTE, l, 0, 0, 0)]
        for it in range(ITERS):
            out += [("k_ex_search", _lib.EX_SEARCH, l, it, ps, ps & 1) for ps in range(PASSES)]
            out.append(("k_ex_vote", _lib.EX_VOTE, l, 0, 0, 0))
    return out


gen = torch.Generator(device="cuda").manual_seed(3)
for n in args.batches:
    frames = texture(n, gen)
    keep = frames.clone()
    dt, lo, hi = timed(lambda: ex.inpaint(frames, mask))
    print(json.dumps({"metric": f"exemplar inpainted frames/s ({W}x{H}, batch {n})", "value": round(n / dt, 1), "unit": "frames/s",
                      "ms_per_call": round(dt * 1e3, 2), "ms_min": round(lo * 1e3, 2), "ms_max": round(hi * 1e3, 2), "steps": args.steps}))
    # the same call launch by launch, a pair of HIP events around each
    frames.copy_(keep)
    plan = stages(len(levels))
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in plan]
    handle = ex.plan(mask)
    ws = ex.workspace(handle, n)
    ptr, wptr, stream = C.c_void_p(frames.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (kernel, stage, l, it, ps, fb), (a, b) in zip(plan, events):
        a.record()                                                           # straight through the C-ABI: the host must not fall behind the GPU
        _lib.check(_lib.lib.vsr_exemplar_run_stage(handle, ptr, frames.stride(0), n, wptr, ws.numel(), stage, l, it, ps, fb, stream))
        b.record()
    torch.cuda.synchronize()
    per, search_level = {}, {}
    for (kernel, stage, l, it, ps, fb), (a, b) in zip(plan, events):
        ms = a.elapsed_time(b)
        per[kernel] = per.get(kernel, 0.0) + ms
        if kernel == "k_ex_search":
            search_level[l] = search_level.get(l, 0.0) + ms
    print(json.dumps({"metric": f"exemplar kernel times (batch {n})", "unit": "ms per call", "launches": len(plan),
                      **{k: round(v, 3) for k, v in per.items()},
                      "k_ex_search_by_level": {str(l): round(v, 3) for l, v in sorted(search_level.items())}}))
    frames.copy_(keep)
    dt_t, lo_t, hi_t = timed(lambda: te.inpaint(frames, mask))
    print(json.dumps({"metric": f"Telea inpainted frames/s on the same batch ({W}x{H}, batch {n})", "value": round(n / dt_t, 1), "unit": "frames/s",
                      "ms_per_call": round(dt_t * 1e3, 2), "ms_min": round(lo_t * 1e3, 2), "ms_max": round(hi_t * 1e3, 2), "steps": args.steps,
                      "exemplar_over_telea_rate": round(dt_t / dt, 4)}))
    del frames, keep
ex.close()
te.close()
