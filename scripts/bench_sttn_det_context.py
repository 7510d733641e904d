#!/usr/bin/env python3
"""What look-back context frames cost sttn-det: SttnEngine.det_batch on BASELINE config 3's batch of L = 47 frames with N
context frames in front.

    python scripts/bench_sttn_det_context.py [--res 1080p] [--contexts 0,5,10] [--rounds 3] [--reps 3] [--flops-only]

The legs are interleaved --rounds times in ONE process (N0 N5 N10 N0 N5 N10 ...), every visit --reps calls after one untimed call.
Reported per N: fps of the 47 written frames as median [min - max] over the rounds, next to the FLOPs of the plan that ran (the decoder
box of the bench's mask; context frames go through the encoder and seven of the eight blocks, not through the decoder), the ratio to
N = 0 and what the read-only marking saves against the plain plan of 47 + N frames.  --flops-only needs no device.

One JSON line."""
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
from vsr_amd.backend.tools.inpaint_tools import create_mask, get_inpaint_area_by_mask  # noqa: E402
from vsr_amd.engine import SttnEngine  # noqa: E402

L = 47          # batch_generator(1200 frames, 50): 25 x 47 + 25 (scripts/bench_configs.py run_det)


def plan_flops(eng, n_list, n_ctx, mask, areas):
    """FLOPs of the plans det_batch runs for this mask: per area, the decoder box its mask rows / columns are resized to"""
    ar = np.asarray(areas, dtype=np.int32).reshape(-1, 4)
    cols = eng.mask_cols(mask, ar) if switches.on("VSR_DECODE_COLS") else np.zeros((ar.shape[0], 2), np.int32)
    total = 0.0
    for (ymin, ymax, _, _), (lo, hi), (c0, c1) in zip(ar, eng.mask_rows(mask, ar), cols):
        a, b, ca, cb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        if hi > lo and os.environ.get("VSR_DECODE_ROWS", "1") != "0":
            _lib.check(_lib.lib.vsr_sttn_decode_rows(eng.handle, int(ymax - ymin), int(lo), int(hi), C.byref(a), C.byref(b)))
            if c1 > c0:
                _lib.check(_lib.lib.vsr_sttn_decode_cols(eng.handle, int(mask.shape[1]), int(c0), int(c1), C.byref(ca), C.byref(cb)))
        total += eng.context_flops(n_list, n_ctx, (a.value, b.value), (ca.value, cb.value))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1080p", choices=sorted(RES))
    ap.add_argument("--contexts", default="0,5,10")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--flops-only", action="store_true")
    args = ap.parse_args()
    H, W, box = RES[args.res]
    contexts = [int(x) for x in args.contexts.split(",")]
    mask = create_mask((H, W), [(box[2], box[3], box[0], box[1])])
    areas = get_inpaint_area_by_mask(W, H, int(W * 5 / 18), mask[:, :, None])
    eng = SttnEngine(synth.make_state_dict(0, "det"), "det", device=None if args.flops_only else 0)
    legs = {}
    for n in contexts:
        fl, plain = plan_flops(eng, L + n, n, mask, areas), plan_flops(eng, L + n, 0, mask, areas)
        legs[str(n)] = {"plan_gflops": round(fl / 1e9, 1), "plain_plan_of_all_frames_gflops": round(plain / 1e9, 1),
                        "saved_by_read_only": round(1.0 - fl / plain, 4)}
    base = legs[str(contexts[0])]
    for n in contexts:
        legs[str(n)]["flop_ratio"] = round(legs[str(n)]["plan_gflops"] / base["plan_gflops"], 4)
    if not args.flops_only:
        import torch

        assert torch.cuda.is_available(), "the timing legs need a GPU"
        top = max(contexts)
        clip = synth.make_clip(L + top, H, W, box, seed=3)
        dmask = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
        src = torch.from_numpy(clip).cuda()
        work = torch.empty((L, H, W, 3), dtype=torch.uint8, device="cuda")
        fps = {n: [] for n in contexts}
        for _ in range(args.rounds):
            for n in contexts:
                ctx = src[top - n:top].contiguous() if n else None
                for rep in range(args.reps + 1):
                    work.copy_(src[top:])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    eng.det_batch(work, dmask, areas, mask_host=mask, context=ctx)
                    torch.cuda.synchronize()
                    if rep:
                        fps[n].append(L / (time.perf_counter() - t0))
        for n in contexts:
            per_round = [statistics.median(fps[n][r * args.reps:(r + 1) * args.reps]) for r in range(args.rounds)]
            legs[str(n)].update({"fps_median": round(statistics.median(per_round), 2), "fps_min": round(min(per_round), 2),
                                 "fps_max": round(max(per_round), 2)})
        for n in contexts:
            legs[str(n)]["time_ratio"] = round(base["fps_median"] / legs[str(n)]["fps_median"], 4)
        legs["spread_of_first_leg"] = round(base["fps_max"] / base["fps_min"] - 1.0, 4)
    eng.close()
    print(json.dumps({"metric": "sttn-det: cost of look-back context frames", "res": args.res, "batch_frames": L,
                      "timed": not args.flops_only, "legs_by_context": legs}), flush=True)


if __name__ == "__main__":
    main()
