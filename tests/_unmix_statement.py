"""The definition of --logo-unblend in plain numpy: a translucent overlay I = (1 - a) B + a L found by --logo-scan is
un-mixed, B = (I - o) / g with the gain g = 1 - a and the offset o = a L estimated per pixel of the area from the scan's M sampled frames.
The kernels of csrc/unmix_kernels.hip are held to `moments` and `unmix` bit for bit, backend/tools/unblend.solve to `solve`.  All
arithmetic is in integers: g in Q8 (256 = no overlay), means and offsets in Q4.

For one area box = (y0, y1, x0, x1) and the sampled frames F_k (uint8 [H,W,3], BGR), Gbox = the box grown by RING = 24 and clipped to the
frame, ring = Gbox less the box (nr pixels).  Per pixel of Gbox and channel c:
    S1_c = sum_k F,   S2_c = sum_k F^2,   V = sum_c (M S2_c - S1_c^2)                       (M^2 times the variance over time)
    vbar = (sum_ring V) // nr,   mr_c = (16 sum_ring S1_c + (nr M) // 2) // (nr M)         vbar < 16 M^2: refused as "still"
Per pixel of the box:
    g = min(512, isqrt((V << 16) // vbar)),   mI_c = (16 S1_c + M // 2) // M
The level (one opacity per overlay): hist[v] = #(g == v) for v < 232 (none: refused as "none"); c[v] = sum of hist over |u - v| <= 24;
lvl_c = the smallest v at the maximum of c; lvl = element [count // 2] of the sorted g over the pixels with |g - lvl_c| <= 24;
lvl > 216: refused as "faint".  Classes: level |g - lvl| <= 24; clear |g - 256| <= 24 and not level; rim: the rest.
    level   gt = lvl,  ot_c = element [count // 2] of the sorted mI_c - ((lvl mr_c + 128) >> 8) over the level pixels
    clear   gt = 256,  ot = 0
    rim     gt = g,    ot_c = mI_c - ((g mr_c + 128) >> 8)
Un-mixing a pixel with gt >= GMIN = 64: num = 256 (16 I_c - ot_c), den = 16 gt, out_c = 0 if num < 0 else min(255, (num + den // 2) // den);
a pixel with gt < 64 is opaque and keeps what it holds.
The gate: the M sampled frames un-mixed (opaque pixels keep the source) go through the scan's `accumulate`; a pixel of the box that still
has e >= M - M // 8 refuses the area as "shows"."""
import numpy as np

from tests import _static_statement as st

RING, GMIN, GMAX = 24, 64, 512
BAND, HIST_BELOW, FAINT = 24, 232, 216
STILL = 16                                      # vbar below STILL * M^2: a ring that stands still


def grown_box(box, H, W):
    y0, y1, x0, x1 = box
    return max(y0 - RING, 0), min(y1 + RING, H), max(x0 - RING, 0), min(x1 + RING, W)


def moments(frames, gbox, state=None):
    """(S1, S2): int64 [gh,gw,3] each over `frames` (an iterable of uint8 [H,W,3]); state: the pair of the frames before them"""
    gy0, gy1, gx0, gx1 = gbox
    S1, S2 = (None, None) if state is None else (s.copy() for s in state)
    for fr in frames:
        f = fr[gy0:gy1, gx0:gx1].astype(np.int64)
        S1, S2 = (f, f * f) if S1 is None else (S1 + f, S2 + f * f)
    return S1, S2


def isqrt(x):
    """floor(sqrt(x)) of an int64 array, exactly"""
    x = np.asarray(x, np.int64)
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > x, r - 1, r)
    return np.where((r + 1) * (r + 1) <= x, r + 1, r)


def middle(values):
    v = np.sort(np.asarray(values, np.int64).ravel())
    return int(v[len(v) // 2])


def solve(S1, S2, M, box, gbox, info=None):
    """-> (gt int64 [bh,bw], ot int64 [bh,bw,3]) or the reason of the refusal, a string.  S1, S2: the moments over Gbox;
    info, if a dict, receives vbar, mr, lvl and the sizes of the classes"""
    y0, y1, x0, x1 = box
    gy0, gy1, gx0, gx1 = gbox
    S1, S2, M = np.asarray(S1, np.int64), np.asarray(S2, np.int64), int(M)
    V = (M * S2 - S1 * S1).sum(axis=2)
    inner = (slice(y0 - gy0, y1 - gy0), slice(x0 - gx0, x1 - gx0))
    nr = V.size - V[inner].size
    if nr == 0:
        return "still"
    vbar = int(V.sum() - V[inner].sum()) // nr
    mr = (16 * (S1.sum(axis=(0, 1)) - S1[inner].sum(axis=(0, 1))) + (nr * M) // 2) // (nr * M)
    if info is not None:
        info.update(vbar=vbar, mr=[int(m) for m in mr])
    if vbar < STILL * M * M:
        return "still"
    g = np.minimum(GMAX, isqrt(np.minimum((V[inner] << 16) // vbar, GMAX * GMAX)))
    mI = (16 * S1[inner] + M // 2) // M
    hist = np.bincount(g[g < HIST_BELOW], minlength=GMAX + 1)
    if hist.sum() == 0:
        return "none"
    cum = np.concatenate(([0], np.cumsum(hist)))
    v = np.arange(GMAX + 1)
    c = cum[np.minimum(v + BAND, GMAX) + 1] - cum[np.maximum(v - BAND, 0)]
    lvl_c = int(np.argmax(c))
    lvl = middle(g[np.abs(g - lvl_c) <= BAND])
    if info is not None:
        info.update(lvl=lvl)
    if lvl > FAINT:
        return "faint"
    level = np.abs(g - lvl) <= BAND
    clear = (np.abs(g - 256) <= BAND) & ~level
    gt = np.where(level, lvl, np.where(clear, 256, g))
    ot = mI - ((g[..., None] * mr + 128) >> 8)
    flat = mI[level] - ((lvl * mr + 128) >> 8)
    ot[level] = [middle(flat[:, ch]) for ch in range(3)]
    ot[clear] = 0
    if info is not None:
        info.update(level=int(level.sum()), clear=int(clear.sum()), rim=int(g.size - level.sum() - clear.sum()),
                    opaque=int((gt < GMIN).sum()))
    return gt, ot


def unmix(frame, src, gt, ot, box, y0=0):
    """in place on `frame` (uint8 [h,W,3], the rows [y0, y0 + h) of the picture) from `src` (the same rows): every pixel of the box in
    these rows with gt >= GMIN gets the un-mixed source"""
    by0, by1, bx0, bx1 = box
    h = frame.shape[0]
    lo, hi = max(by0, y0), min(by1, y0 + h)
    if lo >= hi:
        return frame
    g = np.asarray(gt, np.int64)[lo - by0:hi - by0]
    o = np.asarray(ot, np.int64)[lo - by0:hi - by0]
    I = src[lo - y0:hi - y0, bx0:bx1].astype(np.int64)
    den = 16 * np.maximum(g, 1)[..., None]
    num = 256 * (16 * I - o)
    out = np.where(num < 0, 0, np.minimum(255, (np.maximum(num, 0) + den // 2) // den))
    into = frame[lo - y0:hi - y0, bx0:bx1]
    into[...] = np.where((g >= GMIN)[..., None], out, into).astype(np.uint8)
    return frame


def gate(frames, gt, ot, box):
    """the seeds the un-mixed sampled frames leave inside the box (0: the overlay is gone)"""
    M = len(frames)
    y0, y1, x0, x1 = box
    _, _, e = st.accumulate(unmix(fr.copy(), fr, gt, ot, box) for fr in frames)
    return int((e[y0:y1, x0:x1] >= M - M // 8).sum())


def plan(frames, box, info=None):
    """the whole definition for one area on the sampled frames (a sequence of uint8 [H,W,3]) -> (gt, ot) or the refusal's reason"""
    H, W = frames[0].shape[:2]
    gbox = grown_box(box, H, W)
    S1, S2 = moments(frames, gbox)
    solved = solve(S1, S2, len(frames), box, gbox, info)
    if isinstance(solved, str):
        return solved
    left = gate(frames, solved[0], solved[1], box)
    if info is not None:
        info.update(seeds=left)
    return "shows" if left else solved


def meets(box, other):
    """whether two (ymin, ymax, xmin, xmax) rectangles share a pixel"""
    return max(box[0], other[0]) < min(box[1], other[1]) and max(box[2], other[2]) < min(box[3], other[3])


# ---- the clips of the design's table -------------------------------------------------------------------------------------------------
def blend(clip, a, rect=st.LOGO, white=255):
    """the rectangle blended toward `white` at opacity a / 256"""
    y0, y1, x0, x1 = rect
    c = clip.copy()
    c[:, y0:y1, x0:x1] = ((256 - a) * clip[:, y0:y1, x0:x1].astype(np.int64) + a * white + 128) >> 8
    return c


def texture(size=1024, seed=7):
    """one smooth grey texture uint8 [size,size]: white noise blurred twice by a 9-pixel box, stretched to the whole range"""
    t = np.random.default_rng(seed).random((size, size))
    for _ in range(2):
        for axis in (0, 1):
            t = sum(np.roll(t, s, axis) for s in range(-4, 5)) / 9.0
    t = (t - t.min()) / (t.max() - t.min())
    return np.round(255 * t).astype(np.uint8)


def crops(tex, offsets, H=st.CLIP_H, W=st.CLIP_W):
    return np.stack([np.repeat(tex[y:y + H, x:x + W, None], 3, axis=2) for y, x in offsets])
