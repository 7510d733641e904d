#!/usr/bin/env python3
"""What --seam-feather costs.  One invocation, every leg three times, interleaved; the lines go to stdout and to
profiles/seam_feather.log.

  kernel   vsr_feather_composite on a 50-frame 1080p batch resident in HBM under a subtitle-band mask, F = 1 and F = 8, against a
           device-to-device copy_ of the same batch timed in the same rounds.  The bytes the kernel has to move are counted from d:
           a pixel with d == 0 reads src and writes (2 x 3 bytes), 0 < d < F also reads the fill (3 x 3), d == F nothing; every pixel
           reads its d (1 byte) -- at most 3 1/3 frame-sized streams against the copy's 2.
  e2e      (--e2e) scripts/bench_e2e.py file to file, 1080p x --frames frames, opencv and sttn-det, F = 0 / 1 / 8 at this commit, each
           run a fresh process; --parent DIR adds F = 0 from a built checkout of the parent commit (F = 0 runs the old path: the
           difference must lie inside the parent's own min-max spread).

    python scripts/bench_seam_feather.py [--e2e [--frames 1200] [--parent DIR]]
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
from vsr_amd.backend.tools import seam_feather  # noqa: E402
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
ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its scripts/bench_e2e.py is run with F unset)")
ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "seam_feather.log"))
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
fill = torch.randint(0, 256, (n, H, W, 3), device="cuda", generator=g, dtype=torch.uint8)
src = torch.randint(0, 256, (n, H, W, 3), device="cuda", generator=g, dtype=torch.uint8)
frames = fill.clone()
frame_bytes = H * W * 3
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
P = lambda t: C.c_void_p(t.data_ptr())

legs = {"copy": lambda: frames.copy_(src)}
moved = {"copy": 2 * frame_bytes}
for F in (1, 8):
    d = seam_feather.alpha(cmask, F, frames.device)
    dh = d.cpu().numpy()
    zero, full = int((dh == 0).sum()), int((dh == F).sum())
    ramp = dh.size - zero - full
    moved[f"F={F}"] = 3 * (2 * zero + 3 * ramp) + dh.size
    # the frames are composited again and again: after the first call the ramp blends a blend, the traffic is the same
    legs[f"F={F}"] = (lambda d=d, F=F: check(lib.vsr_feather_composite(P(frames), frame_bytes, P(src), frame_bytes, P(d), n, H, W, F, stream())))
    say({"metric": "composite mask", "F": F, "pixels": dh.size, "d==0": zero, "0<d<F": ramp, "d==F": full,
         "bytes_per_frame": moved[f"F={F}"], "frame_sized_streams": round(moved[f"F={F}"] / frame_bytes, 3)})
    a0 = torch.cuda.Event(enable_timing=True)
    a1 = torch.cuda.Event(enable_timing=True)
    tmp = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    cm = torch.from_numpy(cmask).cuda()
    check(lib.vsr_feather_alpha(P(cm), H, W, F, P(tmp), stream()))
    a0.record()
    check(lib.vsr_feather_alpha(P(cm), H, W, F, P(tmp), stream()))
    a1.record()
    a1.synchronize()
    say({"metric": "vsr_feather_alpha (once per mask)", "F": F, "ms": round(a0.elapsed_time(a1), 3)})

times = {k: [] for k in legs}
for r in range(args.rounds):
    for name, fn in legs.items():
        ms = timed(fn, args.steps, args.warmup)
        times[name].append(ms)
        say({"metric": "kernel leg", "round": r, "leg": name, "ms_per_call": round(ms, 4), "ms_per_frame": round(ms / n, 5),
             "TB_per_s": round(moved[name] * n / (ms * 1e-3) / 1e12, 3)})
copy_best, copy_worst = min(times["copy"]), max(times["copy"])
for name in legs:
    if name == "copy":
        continue
    best = min(times[name])
    say({"metric": f"composite {name} against copy_ ({W}x{H}, batch {n})", "ms_per_frame": round(best / n, 5),
         "time_ratio_to_copy": round(best / copy_best, 3), "byte_ratio_to_copy": round(moved[name] / moved["copy"], 3),
         "copy_min_max_spread": round(copy_worst / copy_best - 1, 4), "TB_per_s": round(moved[name] * n / (best * 1e-3) / 1e12, 3),
         "copy_TB_per_s": round(moved["copy"] * n / (copy_best * 1e-3) / 1e12, 3)})
del fill, src, frames
torch.cuda.empty_cache()

if args.e2e:
    import tempfile

    with tempfile.TemporaryDirectory() as tmpdir:
        for mode in ("opencv", "sttn-det"):
            clip = os.path.join(tmpdir, f"clip_{mode}.y4m")
            runs = [("this F=0", ROOT, "0"), ("this F=1", ROOT, "1"), ("this F=8", ROOT, "8")]
            if args.parent:
                runs.insert(0, ("parent", args.parent, None))
            got = {name: [] for name, _, _ in runs}
            for r in range(args.rounds):
                for name, root, F in runs:
                    env = dict(os.environ)
                    env.pop("VSR_SEAM_FEATHER", None)
                    if F is not None:
                        env["VSR_SEAM_FEATHER"] = F
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
