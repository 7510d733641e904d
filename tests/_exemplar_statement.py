"""The definition of --opencv-fill exemplar in plain numpy: the kernels of csrc/exemplar_kernels.hip and the plan of
csrc/exemplar_plan.cpp are held to it byte for byte.  Plain numpy, written to be read; the tests use it, the product never imports it.
All arithmetic is in integers.

A PatchMatch exemplar fill, coarse to fine.  R = 3: patches are 7 x 7 x 3 bytes, their distance is the sum of the 147 absolute differences.

pyramid   level 0 is the frame and the hole mask != 0.  Level l + 1 is the 2 x 2 mean (a + b + c + d + 2) >> 2 per channel of level l, odd
          sizes padded by repeating the last row / column; a coarse pixel is hole if one of its four is.  A level is added while the
          hole's depth (4-neighbour erosions until it is empty, outside the frame = hole) exceeds 2, the smaller side is at least 28, the
          next level has a valid source, and there are at most 6.
plan      per level, from the mask alone.  S: the centres whose patch lies inside the frame, holds no hole pixel and lies within
          Chebyshev distance G_l = max(8, 32 >> l) of a hole pixel, in raster order.  D (targets): the centres whose patch lies inside
          the frame and meets the hole.  The tiles are the 16 x 16 cells of the level's grid that hold a target, in raster order; the
          box is the bounding box of D.
hash      hash32(level, iteration, pass, slot, y, x): a fixed 32-bit mix (below).  It never sees the frame index or a pixel.

What the issue leaves open and this file fixes:
  * the mix itself (hash32), and the slots: iteration 255, pass 0, slot 0 is the "any source" draw of the initial state; in a search pass
    slot 2k / 2k + 1 are the row / column offset of the k-th random candidate and slot 63 is the pass's "any source" draw;
  * a random offset is hash % (2 rho + 1) - rho; a candidate outside the frame does not count (it is not clamped);
  * an iteration is 4 search passes and then one vote, so a level votes 4 times after its initial state;
  * a finer level's initial content is ONE vote with the upsampled field: pixels are never upsampled, only the field is, and the vote
    reads known pixels alone;
  * the coarse cell of q is q // 2 clamped to the coarse centres; if it is no coarse target, q takes the "any source" draw;
  * a hole pixel of the coarsest level with no known pixel in its row nor its column starts at 128;
  * e = left means the neighbour to the left of q, whose match is shifted one to the right.

One thing the kernel has and this file has not: k_ex_vote does not follow a field entry that is no valid source, and writes nothing to
a pixel left without a contribution.  Every field that up_field and search_pass produce holds valid sources only, so the guard cannot
be reached from vsr_exemplar_inpaint and there is no rule here for it; it keeps a caller of the stage runner who votes on a workspace
it never filled from reading outside the frames.  A broken field from the searches would still show as a mismatch in the per-launch
tests of the search and of up, which compare the fields themselves.
"""
import numpy as np

R = 3
P = 2 * R + 1
MAX_LEVELS = 6
MIN_SIDE = 28
ITERS = 4
PASSES = 4
TILE = 16
INIT_ITER = 255
ANY_SLOT = 63
NEIGHBOURS = ((0, 1), (1, 0), (0, -1), (-1, 0))        # e: q - e is the left, upper, right, lower neighbour
_M = np.uint64(0xFFFFFFFF)


def hash32(*args):
    """uint32 (as numpy uint64 holding 32 bits): arguments are non-negative ints or arrays of them, broadcast together"""
    h = np.uint64(0x811C9DC5)
    for a in args:
        h = h ^ (np.asarray(a).astype(np.uint64) & _M)
        h = (h * np.uint64(0x9E3779B1)) & _M
        h = h ^ (h >> np.uint64(15))
    h = (h * np.uint64(0x85EBCA6B)) & _M
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M
    return h ^ (h >> np.uint64(16))


def gap(level):
    return max(8, 32 >> level)


# ---------------------------------------------------------------------------------------------------------------------------------------
# pyramid
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pad_even(a):
    H, W = a.shape[:2]
    return np.pad(a, ((0, H & 1), (0, W & 1)) + ((0, 0),) * (a.ndim - 2), mode="edge")


def down(img):
    """uint8 [H,W,3] -> uint8 [(H+1)//2, (W+1)//2, 3]"""
    a = _pad_even(img).astype(np.int32)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def down_hole(hole):
    a = _pad_even(hole)
    return a[0::2, 0::2] | a[0::2, 1::2] | a[1::2, 0::2] | a[1::2, 1::2]


def depth_exceeds(hole, k):
    """whether the hole survives k 4-neighbour erosions (outside the frame counts as hole)"""
    h = np.pad(hole, 1, constant_values=True)
    for _ in range(k):
        h[1:-1, 1:-1] = h[1:-1, 1:-1] & h[:-2, 1:-1] & h[2:, 1:-1] & h[1:-1, :-2] & h[1:-1, 2:]
    return bool(h[1:-1, 1:-1].any())


def _dilate(hole, k):
    """square dilation by k, clipped to the frame"""
    H, W = hole.shape
    c = np.zeros((H + 1, W + 1), np.int64)
    c[1:, 1:] = hole.astype(np.int64).cumsum(0).cumsum(1)
    y0, y1 = np.clip(np.arange(H) - k, 0, H), np.clip(np.arange(H) + k + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - k, 0, W), np.clip(np.arange(W) + k + 1, 0, W)
    return (c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]) > 0


def plan_level(hole, level):
    """the plan of one level: a dict of H, W, hole, valid, target (bool [H,W]), S, D (int [.,2], raster order), tiles (int [.,2]: ty, tx),
    box (y0, x0, h, w: the bounding box of D; zeros without a target)"""
    H, W = hole.shape
    centre = np.zeros((H, W), bool)
    if H >= P and W >= P:
        centre[R:H - R, R:W - R] = True
    meets = _dilate(hole, R)
    valid = centre & ~meets & _dilate(hole, gap(level))
    target = centre & meets
    S, D = np.argwhere(valid), np.argwhere(target)
    tiles = np.unique(D // TILE, axis=0) if len(D) else np.zeros((0, 2), np.int64)
    box = (0, 0, 0, 0)
    if len(D):
        y0, x0 = D.min(0)
        y1, x1 = D.max(0)
        box = (int(y0), int(x0), int(y1 - y0 + 1), int(x1 - x0 + 1))
    return dict(level=level, H=H, W=W, hole=hole, valid=valid, target=target, S=S, D=D, tiles=tiles, box=box)


def init_table(hole):
    """int [nh, 6] per hole pixel in raster order: y, x and the distances to the nearest known pixel to the left, to the right, above and
    below (0: there is none)"""
    H, W = hole.shape
    rows = []
    for y, x in np.argwhere(hole):
        d = [0, 0, 0, 0]
        for k, (dy, dx) in enumerate(((0, -1), (0, 1), (-1, 0), (1, 0))):
            yy, xx, s = y + dy, x + dx, 1
            while 0 <= yy < H and 0 <= xx < W:
                if not hole[yy, xx]:
                    d[k] = s
                    break
                yy, xx, s = yy + dy, xx + dx, s + 1
        rows.append([y, x] + d)
    return np.array(rows, np.int64).reshape(-1, 6)


def plan(mask):
    """mask uint8 [H,W] -> (levels, table): the list of plan_level dicts, finest first, and init_table of the coarsest.  An empty mask gives
    ([], None).  ValueError: no valid source at level 0."""
    hole = np.asarray(mask) != 0
    assert hole.ndim == 2
    if not hole.any():
        return [], None
    levels = [plan_level(hole, 0)]
    if len(levels[0]["S"]) == 0:
        raise ValueError("exemplar: the mask leaves no 7x7 patch of known pixels near the hole to copy from")
    while len(levels) < MAX_LEVELS and depth_exceeds(hole, 2) and min(hole.shape) >= MIN_SIDE:
        nxt = plan_level(down_hole(hole), len(levels))
        if len(nxt["S"]) == 0:
            break
        levels.append(nxt)
        hole = nxt["hole"]
    return levels, init_table(levels[-1]["hole"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the stages (one kernel launch each)
# ---------------------------------------------------------------------------------------------------------------------------------------
def init_pixels(img, table):
    """the coarsest level's initial hole content -> a new uint8 image"""
    out = img.copy()
    a = img.astype(np.int64)
    for y, x, dl, dr, du, dd in table:
        axes = []
        for lo, hi, (ay, ax) in ((dl, dr, (0, 1)), (du, dd, (1, 0))):
            if lo and hi:
                axes.append((hi * a[y - lo * ay, x - lo * ax] + lo * a[y + hi * ay, x + hi * ax] + (lo + hi) // 2) // (lo + hi))
            elif lo:
                axes.append(a[y - lo * ay, x - lo * ax])
            elif hi:
                axes.append(a[y + hi * ay, x + hi * ax])
        out[y, x] = (axes[0] + axes[1] + 1) >> 1 if len(axes) == 2 else axes[0] if axes else 128
    return out


def any_source(lp, it, ps, slot, D):
    """S[hash % |S|] for the targets D [.,2]"""
    h = hash32(lp["level"], it, ps, slot, D[:, 0], D[:, 1])
    return lp["S"][(h % np.uint64(len(lp["S"]))).astype(np.int64)]


def up_field(lp, coarse=None, coarse_lp=None):
    """the initial field of a level, int32 [H,W,2] ((-1,-1) where there is no target): from the coarser level's field, or -- coarse=None,
    the coarsest level -- the "any source" draw for every target"""
    H, W, D = lp["H"], lp["W"], lp["D"]
    nnf = np.full((H, W, 2), -1, np.int32)
    cand = any_source(lp, INIT_ITER, 0, 0, D)
    if coarse is not None:
        Hc, Wc = coarse_lp["H"], coarse_lp["W"]
        cy, cx = np.clip(D[:, 0] // 2, R, Hc - R - 1), np.clip(D[:, 1] // 2, R, Wc - R - 1)
        c = coarse[cy, cx].astype(np.int64)
        uy = np.clip(2 * c[:, 0] + (D[:, 0] & 1), R, H - R - 1)
        ux = np.clip(2 * c[:, 1] + (D[:, 1] & 1), R, W - R - 1)
        ok = (c[:, 0] >= 0) & lp["valid"][uy, ux]
        cand = np.where(ok[:, None], np.stack([uy, ux], 1), cand)
    nnf[D[:, 0], D[:, 1]] = cand
    return nnf


def _patches(img):
    return np.lib.stride_tricks.sliding_window_view(img, (P, P), axis=(0, 1))       # [H-6, W-6, 3, 7, 7], indexed by centre - R


def search_pass(img, nnf, lp, it, ps):
    """one synchronous pass: reads nnf, returns the next field"""
    H, W, D, level = lp["H"], lp["W"], lp["D"], lp["level"]
    y, x = D[:, 0], D[:, 1]
    cur = nnf[y, x].astype(np.int64)
    cands = [cur]
    for ey, ex in NEIGHBOURS:
        ny, nx = y - ey, x - ex
        inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
        nb = nnf[np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)].astype(np.int64)
        nb = np.where((inside & (nb[:, 0] >= 0))[:, None], nb + (ey, ex), -1)
        cands.append(nb)
    rho, k = max(H, W) // 2, 0
    while rho >= 1:
        oy = (hash32(level, it, ps, 2 * k, y, x) % np.uint64(2 * rho + 1)).astype(np.int64) - rho
        ox = (hash32(level, it, ps, 2 * k + 1, y, x) % np.uint64(2 * rho + 1)).astype(np.int64) - rho
        cands.append(cur + np.stack([oy, ox], 1))
        rho, k = rho // 2, k + 1
    cands.append(any_source(lp, it, ps, ANY_SLOT, D))
    pat = _patches(img)
    tgt = pat[y - R, x - R].astype(np.int32)
    best, best_d = cur.copy(), np.full(len(D), np.iinfo(np.int64).max)
    for c in cands:
        cy, cx = c[:, 0], c[:, 1]
        ok = (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
        ok &= lp["valid"][np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)]
        d = np.full(len(D), np.iinfo(np.int64).max)
        if ok.any():
            d[ok] = np.abs(pat[cy[ok] - R, cx[ok] - R].astype(np.int32) - tgt[ok]).sum(axis=(1, 2, 3))
        win = d < best_d                                 # strictly smaller: among equals the earliest candidate stays
        best[win], best_d[win] = c[win], d[win]
    out = nnf.copy()
    out[y, x] = best
    return out


def vote(img, nnf, lp):
    """every hole pixel becomes the rounded mean of what the targets around it propose -> a new uint8 image"""
    H, W = lp["H"], lp["W"]
    a = img.astype(np.int64)
    out = img.copy()
    py, px = np.nonzero(lp["hole"])
    s = np.zeros((len(py), 3), np.int64)
    n = np.zeros(len(py), np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            qy, qx = py + dy, px + dx
            ok = (qy >= R) & (qy < H - R) & (qx >= R) & (qx < W - R)          # an in-frame centre this close to a hole pixel is a target
            m = nnf[qy[ok], qx[ok]].astype(np.int64)
            s[ok] += a[m[:, 0] - dy, m[:, 1] - dx]
            n[ok] += 1
    out[py, px] = (s + (n // 2)[:, None]) // n[:, None]
    return out


def fill(frame, mask, trace=None):
    """one frame uint8 [H,W,3] -> the filled frame.  trace: a list that receives (stage, level, iteration, pass, image, field) after
    every stage, for the per-launch tests."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    levels, table = plan(mask)
    if not levels:
        return frame.copy()
    assert frame.shape[:2] == (levels[0]["H"], levels[0]["W"])
    note = (lambda *a: trace.append(a)) if trace is not None else (lambda *a: None)
    imgs = [frame.copy()]
    for _ in levels[1:]:
        imgs.append(down(imgs[-1]))
        note("down", len(imgs) - 1, 0, 0, imgs[-1], None)
    nnf = None
    for l in range(len(levels) - 1, -1, -1):
        lp = levels[l]
        if nnf is None:
            imgs[l] = init_pixels(imgs[l], table)
            note("init", l, 0, 0, imgs[l], None)
            nnf = up_field(lp)
            note("up", l, 0, 0, imgs[l], nnf)
        else:
            nnf = up_field(lp, nnf, levels[l + 1])
            note("up", l, 0, 0, imgs[l], nnf)
            imgs[l] = vote(imgs[l], nnf, lp)
            note("vote", l, INIT_ITER, 0, imgs[l], nnf)
        for it in range(ITERS):
            for ps in range(PASSES):
                nnf = search_pass(imgs[l], nnf, lp, it, ps)
                note("search", l, it, ps, imgs[l], nnf)
            imgs[l] = vote(imgs[l], nnf, lp)
            note("vote", l, it, 0, imgs[l], nnf)
    out = frame.copy()
    hole = levels[0]["hole"]
    out[hole] = imgs[0][hole]
    return out


def exemplar(frames, mask):
    """frames uint8 [n,H,W,3] -> uint8, the same shape: every frame filled on its own"""
    frames = np.asarray(frames)
    return np.stack([fill(f, mask) for f in frames]) if len(frames) else frames.copy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the test texture and cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def texture(H, W, seed=0):
    y, x = np.mgrid[0:H, 0:W]
    base = 110 + 60 * (((x + y // 2) // 4) % 2) + 30 * ((y // 6) % 2)
    noise = (hash32(seed, y, x) % np.uint64(17)).astype(np.int64) - 8
    return np.clip(np.stack([base + noise, base // 2 + 60 + noise, 255 - base + noise], -1), 0, 255).astype(np.uint8)


def box_mask(H, W, *boxes):
    m = np.zeros((H, W), np.uint8)
    for y0, y1, x0, x1 in boxes:
        m[y0:y1, x0:x1] = 255
    return m


CASES = {
    "48x64": (48, 64, [(18, 30, 12, 52)]),
    "37x53": (37, 53, [(25, 37, 8, 53)]),
    "96x160": (96, 160, [(36, 60, 20, 140)]),
    "64x96_two": (64, 96, [(10, 22, 8, 40), (38, 52, 50, 90)]),
    "thin": (40, 56, [(20, 23, 10, 46)]),
}


def case(name, seed=0):
    """(clean texture, input with the hole at 255, mask)"""
    H, W, boxes = CASES[name]
    clean, mask = texture(H, W, seed), box_mask(H, W, *boxes)
    img = clean.copy()
    img[mask != 0] = 255
    return clean, img, mask
