"""Child process of tests/test_gpu_pad_taps.py: one sttn-auto chunk or one sttn-det batch on the GPU with the VSR_SKIP_PAD_TAPS of this
process's environment (the library reads it once); prints the SHA-256 of the written frames and the model rows the decoder was asked for."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vsr_amd  # noqa: E402,F401
from vsr_amd import _lib, synth  # noqa: E402
from vsr_amd.backend.tools.inpaint_tools import create_mask, get_inpaint_area_by_mask, threshold_mask  # noqa: E402
from vsr_amd.engine import SttnEngine  # noqa: E402

case = sys.argv[1]
if case == "det":
    L, H, W, box, strip = 5, 240, 432, (150, 230, 60, 380), int(432 * 5 / 18)
else:
    L, H, W, strip = 6, 720, 1280, int(1280 * 3 / 16)
    # none / bottom: the mask reaches the last row of the frame, so of its strip; middle: it sits in the middle of its strip
    box = (300, 340, W // 8, W * 7 // 8) if case == "middle" else (H * 5 // 6, H, W // 8, W * 7 // 8)
variant = "det" if case == "det" else "auto"
eng = SttnEngine(synth.make_state_dict(1, variant), variant, device=0)
frames = torch.from_numpy(synth.make_clip(L, H, W, box, seed=23)).cuda()
if case == "det":
    mask = create_mask((H, W), [(box[2], box[3], box[0], box[1])])
    areas = get_inpaint_area_by_mask(W, H, strip, mask[:, :, None])
    dmask = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
else:
    m01 = threshold_mask(create_mask((H, W), [(box[2], box[3], box[0], box[1])]))
    areas = get_inpaint_area_by_mask(W, H, strip, m01)
    dmask = torch.from_numpy(np.ascontiguousarray(m01[:, :, 0])).cuda()
assert len(areas) == 1
promise = case != "none"
lo, hi = C.c_int32(0), C.c_int32(0)
if promise:
    (r0, r1), = eng.mask_rows(dmask, areas)
    _lib.check(_lib.lib.vsr_sttn_decode_rows(eng.handle, int(areas[0][1] - areas[0][0]), int(r0), int(r1), C.byref(lo), C.byref(hi)))
before = frames.clone()
if case == "det":
    eng.det_batch(frames, dmask, areas, decode_rows=promise)
else:
    eng.auto_chunk(frames, dmask, areas, decode_rows=promise)
torch.cuda.synchronize()
assert not torch.equal(frames, before)
print("DIGEST", hashlib.sha256(frames.cpu().numpy().tobytes()).hexdigest(), _lib.lib.vsr_switch_state(b"VSR_SKIP_PAD_TAPS"), lo.value, hi.value)
