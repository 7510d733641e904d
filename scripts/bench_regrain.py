#!/usr/bin/env python3
"""What --regrain costs.  One invocation, every leg three times, interleaved; the lines go to stdout and to
profiles/regrain.log.

  kernel   vsr_regrain_measure + vsr_regrain_apply (P = 100) on a 50-frame 1080p batch resident in HBM under a subtitle-band mask,
           against a device-to-device copy_ of the same batch timed in the same rounds.  The source is a smooth picture with Gaussian
           noise, the fill the same picture without it inside the band, so every frame has a deficit and gets grain.  The fill is put
           back before every timed call by a copy of the band's rows, timed as a leg of its own and subtracted.
  e2e      (--e2e) scripts/bench_e2e.py file to file, 1080p x --frames frames, opencv and sttn-det, P = 0 / 100 at this commit, each run
           a fresh process; --parent DIR adds a run with P unset from a built checkout of the parent commit (P = 0 runs the old path:
           the difference must lie inside the parent's own min-max spread).

    python scripts/bench_regrain.py [--e2e [--frames 1200] [--parent DIR]]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_amd  # noqa: E402,F401
from vsr_amd._lib import check, lib  # noqa: E402
from vsr_amd.backend.tools import regrain  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import create_mask  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--e2e", action="store_true")
ap.add_argument("--frames", type=int, default=1200)
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its scripts/bench_e2e.py is run with P unset)")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "regrain.log"))
args = ap.parse_args()

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
fill[:, inside] = plane.round().to(torch.uint8)[inside]
frames = fill.clone()
frame_bytes = H * W * 3
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
P = lambda t: C.c_void_p(t.data_ptr())

sets = regrain.sets(cmask, (0, H), frames.device)
ne, ni = sets.counts.cpu().tolist()
say({"metric": "sample sets", "pixels": H * W, "|E|": ne, "|I|": ni, "C": int(cmask.sum()), "rows_of_C": [sets.c0, sets.c1]})
a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
cm = torch.from_numpy(cmask).cuda()
tmp, cnt = torch.empty((H, W), dtype=torch.uint8, device="cuda"), torch.empty(2, dtype=torch.int64, device="cuda")
check(lib.vsr_regrain_sets(P(cm), H, W, 0, H, P(tmp), P(cnt), stream()))
a0.record()
check(lib.vsr_regrain_sets(P(cm), H, W, 0, H, P(tmp), P(cnt), stream()))
a1.record()
a1.synchronize()
say({"metric": "vsr_regrain_sets (once per mask)", "ms": round(a0.elapsed_time(a1), 3)})

band = slice(sets.c0, sets.c1)


def restore():
    frames[:, band].copy_(fill[:, band])


def regrain_leg():
    restore()
    regrain.apply(frames, src, sets, 100)


legs = {"copy": lambda: frames.copy_(src), "restore": restore, "restore+regrain": regrain_leg}
times = {k: [] for k in legs}
for r in range(args.rounds):
    for name, fn in legs.items():
        ms = timed(fn, args.steps, args.warmup)
        times[name].append(ms)
        say({"metric": "kernel leg", "round": r, "leg": name, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / n, 5)})
restore()
regrain.apply(frames, src, sets, 100)
torch.cuda.synchronize()
say({"metric": "bytes of the batch the grain changed", "value": int((frames != fill).sum().item())})
copy_best, copy_worst = min(times["copy"]), max(times["copy"])
best = min(times["restore+regrain"]) - min(times["restore"])
say({"metric": f"measure + apply against copy_ ({W}x{H}, batch {n}, P = 100)", "ms_per_frame": round(best / n, 5),
     "time_ratio_to_copy": round(best / copy_best, 3), "copy_ms_per_frame": round(copy_best / n, 5),
     "copy_min_max_spread": round(copy_worst / copy_best - 1, 4)})
del fill, src, frames
torch.cuda.empty_cache()

if args.e2e:
    import tempfile

    with tempfile.TemporaryDirectory() as tmpdir:
        for mode in ("opencv", "sttn-det"):
            clip = os.path.join(tmpdir, f"clip_{mode}.y4m")
            runs = [("this P=0", ROOT, "0"), ("this P=100", ROOT, "100")]
            if args.parent:
                runs.insert(0, ("parent", args.parent, None))
            got = {name: [] for name, _, _ in runs}
            for r in range(args.rounds):
                for name, root, p in runs:
                    env = dict(os.environ)
                    env.pop("VSR_REGRAIN", None)
                    if p is not None:
                        env["VSR_REGRAIN"] = p
                    out = subprocess.run([sys.executable, os.path.join(root, "scripts", "bench_e2e.py"), "--mode", mode, "--frames",
                                          str(args.frames), "--cycle", "50", "--clip", clip], env=env, cwd=root, check=True,
                                         stdout=subprocess.PIPE, text=True).stdout
                    line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
                    got[name].append(line["value"])
                    say({"metric": "e2e leg", "mode": mode, "round": r, "leg": name, "frames_per_s": line["value"]})
            for name in got:
                say({"metric": f"e2e {mode} 1080p x {args.frames}", "leg": name, "frames_per_s_min": min(got[name]),
                     "frames_per_s_max": max(got[name])})
log.close()
