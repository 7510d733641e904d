"""--inpaint-mode opencv with the reference's signature, running on the MI355X engine.

Mirrors backend/inpaint/opencv_inpaint.py:
  OpenCVInpaint()
      inpaint(frame, mask) -> uint8 HxWx3            :8-10   cv2.inpaint(frame, mask, 3, cv2.INTER_LINEAR): the flag's value is
                                                             1 = INPAINT_TELEA, radius 3
      __call__(input_frames, input_mask) -> frames   :12-16  (the generic plugin contract of main.py:326)
OpenCV's Telea fill is restated (tests/_telea_statement.py): the fast-marching order depends on the mask alone, so
the engine builds it once per mask on the host and replays it on every frame in a HIP kernel.  Parity with cv2 itself is
pinned only where cv2 can be imported (tests/test_gpu_telea.py).  The reference's own pass-through survives as an explicit
choice, VSR_OPENCV_BACKEND=cv2, honoured only where cv2 imports; the default is the GPU path everywhere and has no CPU path.

--opencv-fill exemplar (VSR_OPENCV_FILL; default telea) swaps the fill itself: a PatchMatch exemplar fill, coarse to fine, that copies
real texture from the picture around the hole (engine.ExemplarEngine, tests/_exemplar_statement.py).  Everything
around the fill -- the plugin contract, composite_mask, sample_rows, the cosmetic passes of tools/seam_feather.py -- is the same.
"""
import os

import numpy as np
import torch

from ...engine import ExemplarEngine, TeleaEngine
from ..tools import seam_feather
from .sttn_auto_inpaint import _device_index

RADIUS = 3                                                                   # opencv_inpaint.py:9
FILLS = ("telea", "exemplar")


def fill_option(value=None):
    """--opencv-fill / VSR_OPENCV_FILL -> "telea" or "exemplar"; None reads the environment, unset or empty is telea.  ValueError otherwise."""
    if value is None:
        value = os.environ.get("VSR_OPENCV_FILL", "")
    text = str(value).strip().lower()
    if text == "":
        return "telea"
    if text not in FILLS:
        raise ValueError(f"the opencv fill must be one of {', '.join(FILLS)}, not {value!r}")
    return text


def available():
    """whether opencv-python can be imported (only VSR_OPENCV_BACKEND=cv2 needs it)"""
    try:
        import cv2  # noqa: F401
        return True
    except ImportError:
        return False


def _mask2d(mask):
    m = np.asarray(mask)
    if m.ndim == 3:                                                          # [H,W,1], as the other plugins' callers may pass
        m = m[:, :, 0]
    return np.ascontiguousarray(m, dtype=np.uint8)


class OpenCVInpaint:
    accepts_device_frames = True      # __call__ also takes a uint8 [n,H,W,3] device tensor and inpaints it in place (tools/resident.py)

    def __init__(self, device="cuda:0", engine=None, fill=None):
        self.device = device
        self._cv2 = None
        if engine is not None:
            # a passed engine is the fill: the option is not read, and an explicit `fill` that names the other one is refused
            self.fill = "exemplar" if isinstance(engine, ExemplarEngine) else "telea"
            if fill is not None and fill_option(fill) != self.fill:
                raise ValueError(f"fill={fill!r} does not match the engine that was passed, which fills by {self.fill}")
        else:
            self.fill = fill_option(fill)
        wants_cv2 = os.environ.get("VSR_OPENCV_BACKEND", "").lower() == "cv2"
        if self.fill == "exemplar" and engine is None:
            if wants_cv2:
                raise ValueError("VSR_OPENCV_BACKEND=cv2 hands the fill to cv2.inpaint, which has no exemplar fill: drop one of the two")
            self.engine = ExemplarEngine(device=_device_index(device))
        elif engine is None and wants_cv2 and available():
            import cv2

            self._cv2 = cv2
            self.accepts_device_frames = False
            self.engine = None
        else:
            self.engine = engine if engine is not None else TeleaEngine(device=_device_index(device), radius=RADIUS)

    def clone(self):
        """a second instance on the same device: its own engine and plan cache (tools/batch_lanes.py)"""
        return OpenCVInpaint(self.device, fill=self.fill)

    def close(self):
        if self.engine is not None:
            self.engine.close()

    def inpaint(self, frame, mask):
        return self([frame], mask)[0]

    def composite_mask(self, input_mask):
        """uint8 [H,W]: the pixels this plugin fills (--seam-feather, tools/seam_feather.py): mask != 0"""
        return (_mask2d(input_mask) != 0).astype(np.uint8)

    def sample_rows(self, input_mask):
        """(r0, r1): the rows --regrain samples the source's grain in (tools/regrain.py): the whole frame"""
        return 0, int(np.asarray(input_mask).shape[0])

    def __call__(self, input_frames, input_mask):
        """input_frames: the reference's list of HxWx3 uint8 BGR arrays (fresh arrays come back, inputs untouched), or -- the
        HBM-resident loop of main.SubtitleRemover, tools/resident.py -- a uint8 [n,H,W,3] device tensor, which is inpainted IN
        PLACE and returned.  (--seam-feather: the call ends with the feathered composite, tools/seam_feather.py.)"""
        return seam_feather.plugin_call(self, self._call, input_frames, input_mask, self.device)

    def _call(self, input_frames, input_mask):
        mask = _mask2d(input_mask)
        if self._cv2 is not None:
            return [self._cv2.inpaint(f, mask, RADIUS, self._cv2.INPAINT_TELEA) for f in input_frames]
        if isinstance(input_frames, torch.Tensor):
            if input_frames.shape[0]:
                self.engine.inpaint(input_frames, mask)
            return input_frames
        if len(input_frames) == 0:
            return []
        if not mask.any():
            return [np.array(f, copy=True) for f in input_frames]
        frames = torch.from_numpy(np.ascontiguousarray(np.stack(input_frames))).to(self.engine.device)
        out = self.engine.inpaint(frames, mask).cpu().numpy()
        return [out[i] for i in range(out.shape[0])]
