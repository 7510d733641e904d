"""CPU statement of --seam-feather: the mask-exact, feathered composite a plugin call ends with.  Plain numpy, written to
be read; the tests use it, the product never imports it.  All integer arithmetic.

For one plugin call on frames [n,H,W,3] with mask M and the option F (1 <= F <= 64; 0 is off and is not stated here):

  src   the frames as they came in
  fill  what the call returns with the option off
  C     the composite mask, uint8 [H,W]: the pixels under which the plugin blends its prediction (composite_mask below, per mode)
  d(p)  min(F, Chebyshev distance from p to the nearest pixel q INSIDE THE FRAME with C[q] == 0); 0 outside C.  The frame border is
        no zero: a band that touches the bottom edge is not feathered there; a mask that covers the whole frame has d = F everywhere.
  out[p] = (d(p) * fill[p] + (F - d(p)) * src[p] + F // 2) // F          per channel

(a) `distance_brute(C, F)`: d by its definition, one pixel at a time: the largest k <= F such that the (2k-1) x (2k-1) window around p,
    cut at the frame, holds no zero.
(b) `distance_separable(C, F)`: the two passes the kernel runs -- h(y,x) = min(F, distance along the row to the nearest zero), then
    d(y,x) = min over |dy| < F of max(|dy|, h(y+dy,x)), rows outside the frame counting as h = F.
(c) `blend(fill, src, d, F)`, `composite(fill, src, C, F)`: the integer blend.
(d) `composite_mask(mode, M, ...)`: C per mode, restated from the plugin code it mirrors.
"""
import numpy as np

MAX_FEATHER = 64


def distance_brute(C, F):
    C = np.asarray(C)
    H, W = C.shape
    zero = C == 0
    d = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            k = 0
            # the window of Chebyshev radius k (cut at the frame) holds no zero  <=>  the distance is > k
            while k < F and not zero[max(0, y - k):y + k + 1, max(0, x - k):x + k + 1].any():
                k += 1
            d[y, x] = k
    return d


def distance_separable(C, F):
    C = np.asarray(C)
    H, W = C.shape
    h = np.full((H, W), F, dtype=np.int64)
    for y in range(H):
        zeros = np.flatnonzero(C[y] == 0)
        if zeros.size:
            h[y] = np.minimum(F, np.abs(np.arange(W)[:, None] - zeros[None, :]).min(axis=1))
    padded = np.full((H + 2 * F, W), F, dtype=np.int64)           # rows outside the frame: h = F
    padded[F:F + H] = h
    d = np.full((H, W), F, dtype=np.int64)
    for dy in range(-(F - 1), F):
        d = np.minimum(d, np.maximum(abs(dy), padded[F + dy:F + dy + H]))
    return d.astype(np.uint8)


def blend(fill, src, d, F):
    """fill, src uint8 [..., H, W, 3]; d uint8 [H, W] with 0 <= d <= F -> uint8"""
    d = np.asarray(d).astype(np.int64)[..., None]
    assert d.min() >= 0 and d.max() <= F
    out = (d * np.asarray(fill).astype(np.int64) + (F - d) * np.asarray(src).astype(np.int64) + F // 2) // F
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def composite(fill, src, C, F, distance=distance_separable):
    return blend(fill, src, distance(C, F), F)


# ---- C per mode ------------------------------------------------------------------------------------------------------------------
def _strips(M, split_h, multiple=1):
    from vsr_amd.backend.tools.inpaint_tools import get_inpaint_area_by_mask

    H, W = M.shape[:2]
    return get_inpaint_area_by_mask(W, H, split_h, M.reshape(H, W, 1), multiple=multiple)


def composite_mask(mode, M, mask_dilation=4):
    """M: the uint8 [H,W] mask the plugin call gets.
    sttn-det, lama, opencv   M != 0 (sttn_det_inpaint.py / lama_inpaint.py: the prediction is blended under the mask; opencv fills it)
    sttn-auto                the thresholded mask (M > 127, sttn_auto_inpaint.py:224-225) inside the rows of its inpaint areas
                             (strips of height int(W * 3 / 16))
    propainter               per strip of get_inpaint_area_by_mask(..., int(W * 3 / 16), multiple=8): the mask it blends under, the
                             `mask_dilation`-iteration scipy binary_dilation of the strip's mask, bounded by the strip
                             (propainter_inpaint.py read_mask, :32-77), put back at the strip's position; the union over the strips"""
    M = np.asarray(M)
    if M.ndim == 3:
        M = M[:, :, 0]
    H, W = M.shape
    if mode in ("sttn-det", "lama", "opencv"):
        return (M != 0).astype(np.uint8)
    if mode == "sttn-auto":
        T = (M > 127).astype(np.uint8)
        out = np.zeros((H, W), dtype=np.uint8)
        for y0, y1, _, _ in _strips(T, int(W * 3 / 16)):
            out[y0:y1] = T[y0:y1]
        return out
    if mode == "propainter":
        import scipy.ndimage

        out = np.zeros((H, W), dtype=np.uint8)
        for y0, y1, x0, x1 in _strips(M, int(W * 3 / 16), multiple=8):
            out[y0:y1, x0:x1] |= scipy.ndimage.binary_dilation(M[y0:y1, x0:x1], iterations=mask_dilation).astype(np.uint8)
        return out
    raise ValueError(mode)
