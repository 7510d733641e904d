#!/usr/bin/env python3
"""What --logo-scan costs.  One invocation, every leg `--rounds` times, interleaved; the lines go to stdout and to --log
(default profiles/logo_scan.log).

  vsr_static_accum over the 120 sampled frames of a 1 200-frame 1080p clip resident in HBM (one launch; the bytes it needs: the sampled
  frames once, the three state planes written once), against a device-to-device copy_ of as many frame bytes timed in the same rounds
  (a copy reads and writes every byte, so its rate counts both); then vsr_static_classify, the labelling (vsr_det_launch_ccl with its
  read-back) and the whole of find_areas on the resident clip.  The clip is a moving wave with noise and two static logos.

    python scripts/bench_logo_scan.py [--frames N] [--log FILE]
"""
import argparse
import json
import os
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_amd  # noqa: E402,F401
from vsr_amd.backend.tools import logo_scan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1200)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "logo_scan.log"))
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


N, H, W = args.frames, args.height, args.width
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(5)
yy = torch.arange(H, device=dev)[:, None]
xx = torch.arange(W, device=dev)[None, :]
clip = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
for f in range(N):                                                           # a frame at a time: the clip alone is N * H * W * 3 bytes
    t = (xx + yy + 5 * f) % 256
    wave = torch.minimum(t, 256 - t).to(torch.float32)
    frame = wave[..., None] + 4.0 * torch.randn((H, W, 3), device=dev, generator=g)
    clip[f] = frame.round().clamp(0, 255).to(torch.uint8)
sy, sx = H / 1080.0, W / 1920.0
logos = [(int(60 * sy), int(140 * sy), int(1660 * sx), int(1840 * sx)), (int(940 * sy), int(1000 * sy), int(80 * sx), int(300 * sx))]
for y0, y1, x0, x1 in logos:
    clip[:, y0:y1, x0:x1] = 255
    clip[:, y0 + 8:y1 - 8, x0 + 8:x1 - 8] = 20
torch.cuda.synchronize()

idx = logo_scan.sample_indices(N)
M = len(idx)
scan = logo_scan.Scan(H, W, dev)
sampled_bytes = M * H * W * 3
src, dst = clip[:M], torch.empty_like(clip[:M])                              # as many bytes as the scan reads
say({"metric": "logo scan", "clip": [N, H, W], "sampled_frames": M, "sampled_MB": round(sampled_bytes / 1e6, 1),
     "state_planes_MB": round(H * W * 4 / 1e6, 2)})


def accumulate():
    scan.fed = 0
    scan.feed(clip, idx)


accumulate()
grown, moving = scan.maps()
legs = {"copy": lambda: dst.copy_(src), "accumulate": accumulate, "classify": scan.maps}
times = {k: [] for k in legs}
for r in range(args.rounds):
    for name, fn in legs.items():
        ms = timed(fn, args.steps, args.warmup)
        times[name].append(ms)
        say({"metric": "kernel leg", "round": r, "leg": name, "ms_per_call": round(ms, 4)})
copy_ms, acc_ms = min(times["copy"]), min(times["accumulate"])
say({"metric": f"accumulate against copy_ ({W}x{H}, {M} of {N} frames)", "accumulate_ms": round(acc_ms, 3),
     "accumulate_GB_per_s": round((sampled_bytes + H * W * 4) / acc_ms / 1e6, 1), "copy_ms": round(copy_ms, 3),
     "copy_GB_per_s_read_plus_write": round(2 * sampled_bytes / copy_ms / 1e6, 1), "time_ratio_to_copy": round(acc_ms / copy_ms, 3),
     "copy_min_max_spread": round(max(times["copy"]) / copy_ms - 1, 4), "classify_ms": round(min(times["classify"]), 4)})

torch.cuda.synchronize()
t0 = time.time()
comps = scan.components(grown)
torch.cuda.synchronize()
label_ms = (time.time() - t0) * 1e3
resident = types.SimpleNamespace(frames=clip, windowed=False)
whole = []
for _ in range(args.rounds):
    torch.cuda.synchronize()
    t0 = time.time()
    areas = logo_scan.find_areas(None, clip=resident)
    torch.cuda.synchronize()
    whole.append((time.time() - t0) * 1e3)
say({"metric": "find_areas on the resident clip (host clock, ends in a synchronise)", "ms_min": round(min(whole), 2), "ms_all": [round(w, 2) for w in whole],
     "labelling_with_read_back_ms_first_call": round(label_ms, 2), "components": int(len(comps)), "areas": [list(a) for a in areas],
     "logos_drawn_ymin_ymax_xmin_xmax": [list(b) for b in logos]})
log.close()
