#!/usr/bin/env python3
"""What the two sttn-auto options that are not the reference's cost: look-back context frames and the scene pass.

    python scripts/bench_sttn_context.py [--res 1080p] [--contexts 0,5,10] [--rounds 3] [--reps 4] [--frames 1200]

Leg 1, the engine: SttnEngine.auto_chunk on a chunk of L = 50 frames with N context frames in front, N from --contexts, the legs
interleaved --rounds times in ONE process (N0 N5 N10 N0 N5 N10 ...), every visit --reps calls after one untimed call.  Reported per N:
fps of the 50 written frames as median [min - max] over the rounds, next to the FLOPs of the plan that ran (the decoder box of this
mask; context frames go through the encoder and seven of the eight blocks, not through the decoder).

Leg 2, the plugin: a synthetic --frames-frame *.y4m (4:2:0, the first 50 frames repeated: every stage's cost is content-independent)
file to file through SubtitleRemover.run() in sttn-auto mode, once as the reference runs it and once with --scene-split
--sttn-context 5; the seconds of the scene pass are SubtitleRemover.phase_seconds["scene cuts"].

One JSON line."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import vsr_amd  # noqa: E402,F401
from bench import RES  # noqa: E402
from bench_e2e import write_clip  # noqa: E402
from vsr_amd import _lib, switches, synth  # noqa: E402
from vsr_amd.backend.config import config  # noqa: E402
from vsr_amd.backend.main import SubtitleRemover  # noqa: E402
from vsr_amd.backend.tools.constant import InpaintMode  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import get_inpaint_area_by_mask, threshold_mask  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import create_mask  # noqa: E402
from vsr_amd.engine import SttnEngine  # noqa: E402


def plan_flops(eng, L, n_ctx, mask01, areas):
    """FLOPs of the plans auto_chunk runs for this mask: per area, the decoder box its mask rows / columns are resized from"""
    ar = np.asarray(areas, dtype=np.int32).reshape(-1, 4)
    cols = eng.mask_cols(mask01, ar) if switches.on("VSR_DECODE_COLS") else np.zeros((ar.shape[0], 2), np.int32)
    total = 0.0
    for (ymin, ymax, _, _), (lo, hi), (c0, c1) in zip(ar, eng.mask_rows(mask01, ar), cols):
        a, b, ca, cb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        if hi > lo and os.environ.get("VSR_DECODE_ROWS", "1") != "0":
            _lib.check(_lib.lib.vsr_sttn_decode_rows(eng.handle, int(ymax - ymin), int(lo), int(hi), C.byref(a), C.byref(b)))
            if c1 > c0:
                _lib.check(_lib.lib.vsr_sttn_decode_cols(eng.handle, int(mask01.shape[1]), int(c0), int(c1), C.byref(ca), C.byref(cb)))
        total += eng.context_flops(L + n_ctx, n_ctx, (a.value, b.value), (ca.value, cb.value))
    return total


def engine_legs(args, H, W, box):
    L = 50
    contexts = [int(x) for x in args.contexts.split(",")]
    eng = SttnEngine(synth.make_state_dict(0, "auto"), "auto", device=0)
    clip = synth.make_clip(L + max(contexts), H, W, box, seed=3)
    mask = threshold_mask(create_mask((H, W), [(box[2], box[3], box[0], box[1])]))
    areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), mask)
    mask01 = np.ascontiguousarray(mask[:, :, 0])
    dmask = torch.from_numpy(mask01).cuda()
    src = torch.from_numpy(clip).cuda()
    work = torch.empty((L, H, W, 3), dtype=torch.uint8, device="cuda")
    fps = {n: [] for n in contexts}
    for _ in range(args.rounds):
        for n in contexts:
            ctx = src[max(contexts) - n:max(contexts)].contiguous() if n else None
            for rep in range(args.reps + 1):
                work.copy_(src[max(contexts):])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.auto_chunk(work, dmask, areas, mask_host=mask01, context=ctx)
                torch.cuda.synchronize()
                if rep:
                    fps[n].append(L / (time.perf_counter() - t0))
    legs = {}
    for n in contexts:
        per_round = [statistics.median(fps[n][r * args.reps:(r + 1) * args.reps]) for r in range(args.rounds)]
        legs[str(n)] = {"fps_median": round(statistics.median(per_round), 2), "fps_min": round(min(per_round), 2), "fps_max": round(max(per_round), 2),
                        "plan_gflops": round(plan_flops(eng, L, n, mask01, areas) / 1e9, 1)}
    base = legs[str(contexts[0])]
    for n in contexts:
        legs[str(n)]["time_ratio"] = round(base["fps_median"] / legs[str(n)]["fps_median"], 4)
        legs[str(n)]["flop_ratio"] = round(legs[str(n)]["plan_gflops"] / base["plan_gflops"], 4)
    eng.close()
    return legs


def plugin_legs(args, H, W, box):
    tmp = tempfile.mkdtemp(prefix="vsr_ctx_")
    src = os.path.join(tmp, "in.y4m")
    write_clip(src, args.frames, H, W, box, lambda i: True, cycle=50)
    ck = os.path.join(tmp, "infer_model.pth")
    torch.save({"netG": {k: torch.from_numpy(v) for k, v in synth.make_state_dict(0, "auto").items()}}, ck)
    config.inpaintMode.value = InpaintMode.STTN_AUTO
    out = {}
    for name, env in (("reference grid", {"VSR_SCENE_SPLIT": "0", "VSR_STTN_CONTEXT": "0"}),
                      ("scene split + context 5", {"VSR_SCENE_SPLIT": "1", "VSR_STTN_CONTEXT": "5"})):
        os.environ.update(env)
        sr = SubtitleRemover(src, device="cuda:0", model_path=ck)
        sr.sub_areas = [box]
        sr.video_out_path = os.path.join(tmp, "out.y4m")
        torch.cuda.synchronize()
        t0 = time.time()
        sr.run()
        torch.cuda.synchronize()
        wall = time.time() - t0
        out[name] = {"fps": round(args.frames / wall, 2), "wall_s": round(wall, 2), "phases_s": {k: round(v, 3) for k, v in sr.phase_seconds.items()}}
    shutil.rmtree(tmp, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="1080p", choices=sorted(RES))
    ap.add_argument("--contexts", default="0,5,10")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--frames", type=int, default=1200, help="frames of the plugin leg's clip (0: skip that leg)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sttn_context.py needs a GPU"
    H, W, box = RES[args.res]
    res = {"metric": "sttn-auto: cost of look-back context frames and of the scene pass", "res": args.res, "chunk_frames": 50,
           "engine_legs_by_context": engine_legs(args, H, W, box)}
    if args.frames > 0:
        res["frames"] = args.frames
        res["plugin_runs"] = plugin_legs(args, H, W, box)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
