"""--text-detect strokes: a text detector that needs no weights, on the GPU (not in the reference, whose detector is PP-OCRv5; opt-in,
DESIGN 4.22; the numpy statement is tests/_strokes_statement.py).

It finds stroke-like text -- bright or dark thin strokes with strong contrast against their surroundings, in both orientations, packed
densely along a line: the burnt-in subtitle with an outline or a shadow.  Per frame, at the analysis scale F = clamp(ceil(min(H, W) /
720), 1, 8) (the rounded mean of F x F lumas, so stroke widths land in 2..6 analysis pixels): a pixel is a V-stroke pixel when it is a
ridge along its row -- brighter by C than the minimum of the S pixels on either side, or darker by C than their maxima -- and an H-stroke
pixel when it is one along its column; a step edge is no ridge; a bar wider than S loses its rim, one of 2 S or more is none at all.
The stroke pixels are counted per 4 x 4 cell; a cell is a text cell when the (2 WX + 1) x (2 WY + 1) cells around it hold at least NV V-stroke and NH H-stroke pixels (text has
strokes both ways; a fence, blinds or a bar code has them one way).  An 8-connected component of text cells gives a box: the bounding
box of its cells with at least MINC stroke pixels, kept when it is at least MIN_H analysis pixels high, at least twice as wide as high and
at least a quarter of its cells are such cells.

What it cannot tell: text without contrast against its background, strokes wider than 6 F pixels, a single very short word (narrower
than twice its height), vertical text; and dense fine texture with strokes both ways (a brick wall at the right scale, a printed page
in the shot) is taken for text.  Parity with PP-OCRv5 and the behaviour on real footage are unmeasured.

    1. vsr_strokes_cells: one launch over all frames of a call, the two count planes,
    2. vsr_strokes_text: one launch, the text maps,
    3. vsr_det_launch_ccl: the components of every frame's map (the model detector's labeller), then ONE read-back of all component
       lists and the count planes; the choice among the components (select_boxes) is host arithmetic on a handful of boxes.  (A frame
       with more than COMPONENT_CAP components is labelled once more with room for all and read back on its own: stats["relabelled"].)

Off (the default, or `model`): nothing here is called but detect_option, no symbol of the library is looked up, no launch.  The option is
read here and nowhere else (detect_option: --text-detect sets VSR_TEXT_DETECT).
"""
import ctypes as C
import os

import numpy as np

ENV = "VSR_TEXT_DETECT"
S, CONTRAST, CELL, WX, WY, NV, NH, MINC, MIN_H = 6, 48, 4, 5, 3, 64, 40, 2, 8
COMPONENT_CAP = 1024                        # components of a frame read back at first; a map with more is labelled again with room for all

stats = {"calls": 0, "frames": 0, "launches": 0, "boxes": 0, "relabelled": 0}     # relabelled: frames with more components than COMPONENT_CAP


def detect_option(value=None, env=None):
    """which text detector this run uses: `value`, None = the environment (VSR_TEXT_DETECT; unset, empty or `model` = the PP-OCRv5
    network configured through VSR_DET_MODEL_DIR, `strokes` = the detector of this module).  The one reading of the option.  ValueError
    for anything else."""
    env = os.environ if env is None else env
    if value is None:
        value = env.get(ENV, "")
    value = str(value).strip().lower()
    if value in ("", "model"):
        return "model"
    if value == "strokes":
        return "strokes"
    raise ValueError(f"text detector: {value!r} is neither model nor strokes")


def refuse(dist, runs_detector, injected, value=None):
    """-> whether this run detects strokes.  With `strokes`, a run that cannot use it raises before any work: a mode that runs no
    detector (sttn-auto), an injected detector (a contradiction, as --opencv-fill refuses a contradicting engine), more than one rank
    (the precedent of --logo-scan: the peers' loops have not been taught the option)."""
    if detect_option(value) != "strokes":
        return False
    if not runs_detector:
        raise RuntimeError(f"--text-detect strokes / {ENV} = strokes: --inpaint-mode sttn-auto runs no text detector (it masks the -c boxes on "
                           "every frame); run it without the option, or choose a mode that detects")
    if injected is not None:
        raise RuntimeError(f"--text-detect strokes / {ENV} = strokes contradicts the text detector this run was given "
                           f"({type(injected).__name__}): give one or the other")
    if dist is not None and dist.get_world_size() > 1:
        raise RuntimeError(f"--text-detect strokes / {ENV} = strokes runs in one process (world size {dist.get_world_size()}): "
                           "run without it or on one GPU")
    return True


def scale(H, W):
    """the analysis scale of an H x W frame: 720p -> 1, 1080p -> 2, 2160p -> 3"""
    return min(max(-(-min(int(H), int(W)) // 720), 1), 8)


def select_boxes(comps, cv, ch, F, H, W):
    """the choice among the components -> ([(ymin, ymax, xmin, xmax)] in source pixels, float32 scores), sorted by (ymin, xmin).  comps:
    rows (label, area, xmin, xmax, ymin, ymax) of vsr_det_launch_ccl in cells (inclusive boxes); cv, ch: host [hc,wc] count planes"""
    ink = (np.asarray(cv, np.int64) + np.asarray(ch, np.int64)) >= MINC
    kept = []
    for _, _, xmin, xmax, ymin, ymax in np.asarray(comps, dtype=np.int64).reshape(-1, 6).tolist():
        sub = ink[ymin:ymax + 1, xmin:xmax + 1]
        rows, cols = np.nonzero(sub.any(axis=1))[0], np.nonzero(sub.any(axis=0))[0]
        if len(rows) == 0:
            continue
        y0, y1, x0, x1 = ymin + int(rows[0]), ymin + int(rows[-1]) + 1, xmin + int(cols[0]), xmin + int(cols[-1]) + 1
        hh, ww = (y1 - y0) * CELL, (x1 - x0) * CELL
        inked, count = int(ink[y0:y1, x0:x1].sum()), (y1 - y0) * (x1 - x0)
        if hh >= MIN_H and ww >= 2 * hh and 4 * inked >= count:
            kept.append((y0 * CELL * F, min(y1 * CELL * F, H), x0 * CELL * F, min(x1 * CELL * F, W), np.float32(inked) / np.float32(count)))
    kept.sort(key=lambda b: (b[0], b[2], b[1], b[3]))
    return [b[:4] for b in kept], np.array([b[4] for b in kept], np.float32)


def result(found, scores):
    """one frame's result in the model detector's format: quads [[x0,y0],[x1,y0],[x1,y1],[x0,y1]], so tools/ocr.get_coordinates gives
    back (x0, x1, y0, y1)"""
    polys = np.array([[[x0, y0], [x1, y0], [x1, y1], [x0, y1]] for y0, y1, x0, x1 in found], np.int32).reshape(-1, 4, 2)
    return {"dt_polys": polys, "dt_scores": np.asarray(scores, np.float32)}


class _Buffers:
    """the device buffers of calls of n frames of H x W: everything that is read back lies in `out` -- the two count planes uint8
    [2][n][hc][wc], then per frame int32 [4 + cap * 6]: the component count and the component rows"""

    def __init__(self, n, H, W, device):
        import torch

        self.F = scale(H, W)
        h, w = H // self.F, W // self.F
        self.hc, self.wc = -(-h // CELL), -(-w // CELL)
        cells = self.hc * self.wc
        self.cap = min(COMPONENT_CAP, -(-self.hc // 2) * -(-self.wc // 2))      # (no map has more 8-connected components than that)
        self.plane_bytes = -(-2 * n * cells // 16) * 16
        self.frame_ints = 4 + self.cap * 6
        self.out = torch.zeros(self.plane_bytes + 4 * n * self.frame_ints, dtype=torch.uint8, device=device)
        self.text = torch.empty((n, self.hc, self.wc), dtype=torch.float32, device=device)
        self.labels = torch.empty(cells, dtype=torch.int32, device=device)
        self.work = torch.empty(cells * 5, dtype=torch.int32, device=device)


class StrokeTextDetection:
    """the surface of the model detector (tools/ocr_det.TextDetection) that SubtitleDetect uses -- predict, predict_batch,
    predict_batch_device, batch_size -- without clone(): it runs on one lane, as an injected detector does"""
    batch_size = 8

    def __init__(self, device=0):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("the stroke text detector runs on the MI355X path only: no HIP device available")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self._buffers = {}

    def predict_batch_device(self, frames_dev):
        """frames_dev: uint8 [n,H,W,3] BGR on the device -> n dicts {"dt_polys": int32 [k,4,2], "dt_scores": float32 [k]}.  2 + n
        launches on the current stream, one read-back; a frame whose map has more components than the rows read back (COMPONENT_CAP,
        counted in stats["relabelled"]) costs one more labelling and a read-back of its own."""
        import torch

        from ..._lib import check, lazy, lib

        n = int(frames_dev.shape[0])
        if n == 0:
            return []
        assert frames_dev.dtype == torch.uint8 and frames_dev.dim() == 4 and frames_dev.shape[3] == 3 and frames_dev.device == self.device
        H, W = int(frames_dev.shape[1]), int(frames_dev.shape[2])
        if not (frames_dev.stride(3) == 1 and frames_dev.stride(2) == 3 and frames_dev.stride(1) == 3 * W and (n == 1 or frames_dev.stride(0) >= H * W * 3)):
            frames_dev = frames_dev.contiguous()
        stride = frames_dev.stride(0) if n > 1 else H * W * 3
        key = (n, H, W)
        if key not in self._buffers:
            self._buffers[key] = _Buffers(n, H, W, self.device)
        b = self._buffers[key]
        cells, base = b.hc * b.wc, b.out.data_ptr()
        cv_p, ch_p = C.c_void_p(base), C.c_void_p(base + n * cells)
        launches = 2
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(lazy("vsr_strokes_cells")(C.c_void_p(frames_dev.data_ptr()), stride, n, H, W, b.F, S, CONTRAST, cv_p, ch_p, stream))
            check(lazy("vsr_strokes_text")(cv_p, ch_p, n, b.hc, b.wc, WX, WY, NV, NH, C.c_void_p(b.text.data_ptr()), stream))
            for k in range(n):
                at = base + b.plane_bytes + 4 * k * b.frame_ints
                check(lib.vsr_det_launch_ccl(C.c_void_p(b.text[k].data_ptr()), b.hc, b.wc, C.c_float(0.5), C.c_void_p(b.labels.data_ptr()),
                                             C.c_void_p(b.work.data_ptr()), C.c_void_p(at + 16), b.cap, C.c_void_p(at), stream))
            launches += n
            host = b.out.cpu().numpy()                                   # the one read-back (it waits for the stream)
            planes = host[:2 * n * cells].reshape(2, n, b.hc, b.wc)
            lists = host[b.plane_bytes:].view(np.int32).reshape(n, b.frame_ints)
            results = []
            for k in range(n):
                found = int(lists[k, 0])
                comps = lists[k, 4:4 + 6 * min(found, b.cap)]
                if found > b.cap:                                        # more components than rows: this frame again, with room for all
                    count = torch.zeros(4, dtype=torch.int32, device=self.device)
                    rows = torch.empty(found * 6, dtype=torch.int32, device=self.device)
                    check(lib.vsr_det_launch_ccl(C.c_void_p(b.text[k].data_ptr()), b.hc, b.wc, C.c_float(0.5), C.c_void_p(b.labels.data_ptr()),
                                                 C.c_void_p(b.work.data_ptr()), C.c_void_p(rows.data_ptr()), found, C.c_void_p(count.data_ptr()),
                                                 stream))
                    launches += 1
                    stats["relabelled"] += 1
                    comps = rows.cpu().numpy()
                results.append(result(*select_boxes(comps, planes[0, k], planes[1, k], b.F, H, W)))
        stats["calls"] += 1
        stats["frames"] += n
        stats["launches"] += launches
        stats["boxes"] += sum(len(r["dt_scores"]) for r in results)
        return results

    def predict_batch(self, imgs):
        """[predict(img)[0] for img in imgs] with one call for all frames (independent per frame: the same results)"""
        import torch

        if len(imgs) == 0:
            return []
        with torch.cuda.device(self.device):
            frames = torch.from_numpy(np.ascontiguousarray(np.stack(imgs))).to(self.device)
        return self.predict_batch_device(frames)

    def predict(self, img):
        return self.predict_batch([img])
