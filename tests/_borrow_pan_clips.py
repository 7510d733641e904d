"""The clips of the borrow-pan GPU tests, made on the CPU so that the statement alone (tests/_borrow_pan_statement.py) shows what a case
is for: frames cut from a larger smooth canvas along a path of whole-pixel offsets, independent grain of sigma 2 per frame, white glyph
blocks that change place every `period` frames, a few source pixels 40 levels off (no seed at T = 12, but beyond every threshold) and
one stroke of fill 100 levels off per frame (a seed that nothing can lend to)."""
import numpy as np

from tests.test_gpu_glyph_key import rows_of

MARGIN = 136                                                 # the canvas around the frame: 17 frames of 8 pixels


def canvas(h, w):
    """smooth, with periods beyond 2 P + 1: a shift by a pixel moves a sample by several levels, Immerkaer's operator sees little"""
    y, x = np.mgrid[0:h, 0:w]
    return 120 + 40 * np.sin(2 * np.pi * x / 23.0 + y / 9.0) + 30 * np.sin(2 * np.pi * y / 29.0 + x / 7.0)


def path(n, step, still=()):
    """the offset of every frame: `step` per frame, none in front of the frames of `still`"""
    at, out = np.zeros(2, np.int64), []
    for t in range(n):
        if t and t not in still:
            at = at + np.asarray(step)
        out.append(at.copy())
    return out


def spots(H, W, cmask, group):
    """the upper left corners of the glyph blocks (2 rows x 4 columns) of the frames of `group`: at either end of the mask's first and
    last rows, in its middle, and on either side of column 64"""
    c0, c1 = rows_of(cmask)
    first, last = np.flatnonzero(cmask[c0]), np.flatnonzero(cmask[c1 - 1])
    mid = (c0 + c1) // 2
    if group == 0:
        out = [(c0, int(first[0])), (c1 - 2, int(last[-1]) - 3), (mid, 58)]
    else:
        out = [(c0, int(first[-1]) - 3), (c1 - 2, int(last[0])), (mid, 62)]
    out = [(max(min(y, H - 2), 0), max(min(x, W - 4), 0)) for y, x in out]
    return [(y, x) for y, x in out if cmask[y:y + 2, x:x + 4].any()]


def clip(H, W, cmask, n, step, seed, period=2, still=(), cut=None, extras=True):
    """fill, src uint8 [n,H,W,3]; what frame t shows at p, frame t + 1 shows at p + step (not in front of the frames of `still`);
    cut: from this frame on another scene"""
    rng = np.random.default_rng(seed)
    big = canvas(H + 2 * MARGIN, W + 2 * MARGIN)
    offs = path(n, step, still)
    clean = np.stack([big[MARGIN - o[0]:MARGIN - o[0] + H, MARGIN - o[1]:MARGIN - o[1] + W] for o in offs])[..., None] + np.zeros((1, 1, 1, 3))
    if cut is not None:
        clean[cut:] = 255 - clean[cut:, ::-1, ::-1]
    src = np.rint(clean + rng.normal(0, 2, clean.shape))
    other = np.rint(clean + rng.normal(0, 2, clean.shape))
    inside = cmask != 0
    ys, xs = np.nonzero(inside)
    if extras:
        for f in range(n):
            for i in rng.choice(len(ys), max(len(ys) // 60, 1), replace=False):
                src[f, ys[i], xs[i]] += 40                   # alone in its 3 x 3: no seed, and no lender either
    fill = src.copy()
    fill[:, inside] = other[:, inside]
    for f in range(n):
        for yy, xx in spots(H, W, cmask, (f // period) % 2):
            block = np.zeros((H, W), bool)
            block[yy:yy + 2, xx:xx + 4] = True
            src[f][block] = 255
            fill[f][block & ~inside] = 255                   # outside C the fill is the source
        if extras:
            i = int(rng.integers(0, len(ys)))
            fill[f, ys[i], xs[i]:xs[i] + 3][inside[ys[i], xs[i]:xs[i] + 3]] -= 100
    return np.clip(fill, 0, 255).astype(np.uint8), np.clip(src, 0, 255).astype(np.uint8)


def events(info):
    """what the statement did, the counts by name"""
    lender, q = info["lender"], info["q"]
    n, h, W = lender.shape
    taken = lender >= 0
    xx = np.broadcast_to(np.arange(W)[None, None, :], lender.shape)
    C_at_q = np.zeros(lender.shape, bool)
    C_at_q[taken] = info["Cnz"][q[taken][:, 0], q[taken][:, 1]]
    return dict(shifted_pairs=sum(d != (0, 0) for d in info["D"].values()),
                full_pairs=sum(b == 16 for b in info["b0"].values()),
                crosses_word=int((taken & (q[..., 1] // 64 != xx // 64)).sum()),
                lent_from_outside=int((taken & ~C_at_q).sum()),
                off_frame=info["refused_offframe"], own_glyph=info["refused_near"], threshold=info["refused_threshold"],
                left=int((info["borrowers"] & ~taken).sum()), taken=int(taken.sum()))
