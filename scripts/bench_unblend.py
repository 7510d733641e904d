#!/usr/bin/env python3
"""What --logo-unblend costs.  One invocation, every kernel leg `--rounds` times, interleaved; the lines go to stdout
and to --log (default profiles/unblend.log).

  A 1 200-frame 1080p clip resident in HBM, a moving wave with noise, with one 300 x 500 area blended toward white at a = 96.
  vsr_unmix_accum over the 120 sampled frames inside the grown area (one launch; the bytes it needs: the grown area of every sampled
  frame once, the two moment planes written once), beside vsr_static_accum over the whole sampled frames timed in the same rounds;
  vsr_unmix_apply on a 50-frame batch; then, by the host clock, make_plans as a whole (accumulate, read-back, solve, upload, gate),
  find_areas on the resident clip (the "logo scan" phase) and one opencv plugin call on a 50-frame batch masked with the area.

    python scripts/bench_unblend.py [--frames N] [--log FILE]
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
from vsr_amd.backend.tools import logo_scan, unblend  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1200)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "unblend.log"))
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


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    return (time.time() - t0) * 1e3, out


N, H, W = args.frames, args.height, args.width
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(5)
yy = torch.arange(H, device=dev)[:, None]
xx = torch.arange(W, device=dev)[None, :]
sy, sx = H / 1080.0, W / 1920.0
logo = (int(80 * sy), int(80 * sy) + int(292 * sy), int(1340 * sx), int(1340 * sx) + int(492 * sx))      # the scan grows it by 1 + D + PAD
clip = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
for f in range(N):                                                           # a frame at a time: the clip alone is N * H * W * 3 bytes
    t = (xx + yy + 5 * f) % 256
    wave = torch.minimum(t, 256 - t).to(torch.float32)
    frame = (wave[..., None] + 4.0 * torch.randn((H, W, 3), device=dev, generator=g)).round().clamp(0, 255).to(torch.int32)
    y0, y1, x0, x1 = logo
    frame[y0:y1, x0:x1] = ((256 - 96) * frame[y0:y1, x0:x1] + 96 * 255 + 128) >> 8
    clip[f] = frame.to(torch.uint8)
torch.cuda.synchronize()

idx = logo_scan.sample_indices(N)
M = len(idx)
resident = types.SimpleNamespace(frames=clip, windowed=False)
scan_ms, scan = host_ms(lambda: logo_scan.run_scan(None, clip=resident, keep=True))
say({"metric": "logo scan of the resident clip, frames kept (host clock, first call)", "ms": round(scan_ms, 2), "areas": [list(a) for a in scan.found],
     "logo_drawn": list(logo)})
area = scan.found[0] if scan.found else (logo[0] - 11, logo[1] + 11, logo[2] - 11, logo[3] + 11)
gbox = unblend.grown_box(area, H, W)
gbytes = (gbox[1] - gbox[0]) * (gbox[3] - gbox[2]) * 3
rows_bytes = (gbox[1] - gbox[0]) * W * 3
say({"metric": "area", "area": list(area), "grown": list(gbox), "grown_MB_per_frame": round(gbytes / 1e6, 3), "sampled_frames": M,
     "grown_MB_all_samples": round(M * gbytes / 1e6, 1), "whole_rows_of_the_grown_area_MB_all_samples": round(M * rows_bytes / 1e6, 1)})

mom = unblend.Moments(H, W, gbox, dev)
whole = logo_scan.Scan(H, W, dev)


def accumulate():
    mom.fed = 0
    mom.feed(clip, idx)


def static_accumulate():
    whole.fed = 0
    whole.feed(clip, idx)


plans, refusals = unblend.make_plans(scan, [area])
say({"metric": "plans", "accepted": [[list(p.box), p.level] for p in plans], "refused": [[list(a), r] for a, r in refusals]})
batch = clip[:args.batch].clone()
src = clip[:args.batch].clone()
legs = {"unmix_accum": accumulate, "static_accum": static_accumulate}
if plans:
    legs["unmix_apply"] = lambda: unblend.apply(batch, src, plans, H=H)
times = {k: [] for k in legs}
for r in range(args.rounds):
    for name, fn in legs.items():
        ms = timed(fn, args.steps, args.warmup)
        times[name].append(ms)
        say({"metric": "kernel leg", "round": r, "leg": name, "ms_per_call": round(ms, 4)})
acc, stat = min(times["unmix_accum"]), min(times["static_accum"])
say({"metric": f"accumulate ({W}x{H}, {M} of {N} frames)", "unmix_accum_ms": round(acc, 4),
     "unmix_accum_GB_per_s_on_the_grown_area": round((M * gbytes + 8 * gbytes) / acc / 1e6, 1),
     "static_accum_ms": round(stat, 4), "static_accum_GB_per_s_on_whole_frames": round((M * H * W * 3 + H * W * 4) / stat / 1e6, 1),
     "static_accum_rate_on_the_rows_of_the_grown_area_would_take_ms": round(stat * rows_bytes / (H * W * 3), 4)})
if plans:
    bh, bw = area[1] - area[0], area[3] - area[2]
    say({"metric": f"apply per {args.batch}-frame batch", "ms": round(min(times["unmix_apply"]), 4),
         "GB_per_s_read_plus_write_of_the_box": round(2 * args.batch * bh * bw * 3 / min(times["unmix_apply"]) / 1e6, 1)})

whole_ms = [host_ms(lambda: unblend.make_plans(scan, [area]))[0] for _ in range(args.rounds)]
say({"metric": "make_plans as a whole, one area (host clock, ends in a synchronise)", "ms_min": round(min(whole_ms), 2),
     "ms_all": [round(w, 2) for w in whole_ms]})
find_ms = [host_ms(lambda: logo_scan.find_areas(None, clip=resident))[0] for _ in range(args.rounds)]
say({"metric": "find_areas on the resident clip: the logo scan phase (host clock)", "ms_min": round(min(find_ms), 2),
     "ms_all": [round(w, 2) for w in find_ms]})

from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import create_mask  # noqa: E402

plugin = OpenCVInpaint("cuda:0")
mask = create_mask((H, W), [(area[2], area[3], area[0], area[1])])
for name, registered in (("scan alone", []), ("with the plans", plans)):
    unblend.register(registered)
    ms = []
    for _ in range(args.rounds + 1):
        work = clip[:args.batch].clone()
        ms.append(host_ms(lambda: plugin(work, mask))[0])
    say({"metric": f"opencv plugin call on a {args.batch}-frame batch, {name} (host clock, first call dropped)", "ms_min": round(min(ms[1:]), 2),
         "ms_all": [round(w, 2) for w in ms]})
unblend.clear()
plugin.close()
log.close()
