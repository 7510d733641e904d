#!/usr/bin/env python3
"""What look-ahead context frames cost both STTN modes: SttnEngine.auto_chunk on a chunk of 50 frames and
SttnEngine.det_batch on BASELINE config 3's batch of 47 frames, with N context frames in front and M behind.

    python scripts/bench_sttn_lookahead.py [--res 1080p] [--legs 0:0,10:0,0:10,10:10] [--rounds 3] [--reps 3] [--modes auto,det] [--flops-only]

The legs (N:M) are interleaved --rounds times in ONE process, every visit --reps calls after one untimed call.  Reported per leg: fps
of the written frames as median [min - max] over the rounds, next to the FLOPs of the plan that ran (vsr_sttn_flops_ctx2 with the
decoder box of the bench's mask; context frames of either kind go through the encoder and seven of the eight blocks, not through the
decoder), the ratios to the first leg, and that leg's own min - max spread.  --flops-only needs no device.

One JSON line per mode."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import vsr_amd  # noqa: E402,F401
from bench import RES  # noqa: E402
from vsr_amd import _lib, switches, synth  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import create_mask, get_inpaint_area_by_mask, threshold_mask  # noqa: E402
from vsr_amd.engine import SttnEngine  # noqa: E402

WRITTEN = {"auto": 50, "det": 47}      # the reference's chunk; batch_generator(1200 frames, 50): 25 x 47 + 25 (scripts/bench_configs.py)


def plan_flops(eng, n_list, n_ctx, n_after, mask, areas, frame_w):
    """FLOPs of the plans the call runs for this mask: per area, the decoder box its mask rows / columns are resized to / from"""
    ar = np.asarray(areas, dtype=np.int32).reshape(-1, 4)
    cols = eng.mask_cols(mask, ar) if switches.on("VSR_DECODE_COLS") else np.zeros((ar.shape[0], 2), np.int32)
    total = 0.0
    for (ymin, ymax, _, _), (lo, hi), (c0, c1) in zip(ar, eng.mask_rows(mask, ar), cols):
        a, b, ca, cb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        if hi > lo and os.environ.get("VSR_DECODE_ROWS", "1") != "0":
            _lib.check(_lib.lib.vsr_sttn_decode_rows(eng.handle, int(ymax - ymin), int(lo), int(hi), C.byref(a), C.byref(b)))
            if c1 > c0:
                _lib.check(_lib.lib.vsr_sttn_decode_cols(eng.handle, int(frame_w), int(c0), int(c1), C.byref(ca), C.byref(cb)))
        total += eng.context_flops(n_list, n_ctx, (a.value, b.value), (ca.value, cb.value), n_after=n_after)
    return total


def run_mode(mode, args, H, W, box, legs_nm):
    L = WRITTEN[mode]
    raw = create_mask((H, W), [(box[2], box[3], box[0], box[1])])
    if mode == "auto":
        m3 = threshold_mask(raw)
        areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), m3)
        mask = np.ascontiguousarray(m3[:, :, 0])
    else:
        areas = get_inpaint_area_by_mask(W, H, int(W * 5 / 18), raw[:, :, None])
        mask = np.ascontiguousarray(raw)
    eng = SttnEngine(synth.make_state_dict(0, mode), mode, device=None if args.flops_only else 0)
    legs = {}
    for n, m in legs_nm:
        fl = plan_flops(eng, n + L + m, n, m, mask, areas, W)
        plain = plan_flops(eng, n + L + m, 0, 0, mask, areas, W)
        legs[f"{n}:{m}"] = {"plan_gflops": round(fl / 1e9, 1), "plain_plan_of_all_frames_gflops": round(plain / 1e9, 1),
                            "saved_by_read_only": round(1.0 - fl / plain, 4)}
    first = f"{legs_nm[0][0]}:{legs_nm[0][1]}"
    for k in legs:
        legs[k]["flop_ratio"] = round(legs[k]["plan_gflops"] / legs[first]["plan_gflops"], 4)
    if not args.flops_only:
        import torch

        assert torch.cuda.is_available(), "the timing legs need a GPU"
        top_n, top_m = max(n for n, _ in legs_nm), max(m for _, m in legs_nm)
        src = torch.from_numpy(synth.make_clip(top_n + L + top_m, H, W, box, seed=3)).cuda()
        dmask = torch.from_numpy(mask).cuda()
        work = torch.empty((L, H, W, 3), dtype=torch.uint8, device="cuda")
        call = eng.auto_chunk if mode == "auto" else eng.det_batch
        fps = {k: [] for k in legs}
        for _ in range(args.rounds):
            for n, m in legs_nm:
                ctx = src[top_n - n:top_n].contiguous() if n else None
                after = src[top_n + L:top_n + L + m].contiguous() if m else None
                for rep in range(args.reps + 1):
                    work.copy_(src[top_n:top_n + L])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call(work, dmask, areas, mask_host=mask, context=ctx, lookahead=after)
                    torch.cuda.synchronize()
                    if rep:
                        fps[f"{n}:{m}"].append(L / (time.perf_counter() - t0))
        for k in legs:
            per_round = [statistics.median(fps[k][r * args.reps:(r + 1) * args.reps]) for r in range(args.rounds)]
            legs[k].update({"fps_median": round(statistics.median(per_round), 2), "fps_min": round(min(per_round), 2),
                            "fps_max": round(max(per_round), 2)})
        for k in legs:
            legs[k]["time_ratio"] = round(legs[first]["fps_median"] / legs[k]["fps_median"], 4)
        legs["spread_of_first_leg"] = round(legs[first]["fps_max"] / legs[first]["fps_min"] - 1.0, 4)
    eng.close()
    print(json.dumps({"metric": f"sttn-{mode}: cost of look-back (N) and look-ahead (M) context frames", "res": args.res,
                      "written_frames": L, "timed": not args.flops_only, "legs_by_N:M": legs}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1080p", choices=sorted(RES))
    ap.add_argument("--legs", default="0:0,10:0,0:10,10:10")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="auto,det")
    ap.add_argument("--flops-only", action="store_true")
    args = ap.parse_args()
    H, W, box = RES[args.res]
    legs_nm = [tuple(int(x) for x in leg.split(":")) for leg in args.legs.split(",")]
    for mode in args.modes.split(","):
        run_mode(mode, args, H, W, box, legs_nm)


if __name__ == "__main__":
    main()
