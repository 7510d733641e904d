"""The definition of --logo-scan in plain numpy: the rectangles of a clip that hold a static overlay -- an edge pattern
that stays put while the picture around it moves.  The kernels of csrc/static_kernels.hip are held to `accumulate` and `classify` bit for
bit, backend/tools/logo_scan.find_areas to `areas`.  All arithmetic is in integers.

Of an N-frame clip (N >= 16) M = min(N, 120) frames are sampled, i_k = (k N) // M.  Per sampled frame (uint8 [H,W,3], BGR):
    Y = (29 B + 150 G + 77 R + 128) >> 8
    g = |Y[y, x + 1] - Y[y, x - 1]| + |Y[y + 1, x] - Y[y - 1, x]|            indices clamped to the frame
Per pixel over the samples:  lo = min Y,  hi = max Y,  e = the number of samples with g >= GE = 24.
    seed   = e >= M - M // 8
    moving = hi - lo >= MV = 48
    grown  = seed dilated by D = 6 pixels of Chebyshev distance (pixels outside the frame are no seeds)
A component of grown (8-connected) with the box [y0, y1) x [x0, x1) is kept when
    its area is at least 400 pixels                                            (one stray seed grows to 169),
    x1 - x0 <= W // 3 and y1 - y0 <= H // 3                                    (an overlay, not a letterbox or the set),
    2 * (moving pixels of its ring) >= the ring's pixels                       (a static shot tells nothing),
the ring being the box grown by 24 and clipped to the frame, less the box.  The result: the kept boxes grown by PAD = 4 and clipped, as
(ymin, ymax, xmin, xmax), the at most 8 of the largest area (ties: the smaller (y0, x0) first), sorted by (ymin, xmin)."""
import numpy as np

GE, MV, D = 24, 48, 6
MAX_SAMPLES, MIN_FRAMES = 120, 16
MIN_AREA, RING, PAD, MAX_AREAS = 400, 24, 4, 8


def sample_indices(N):
    if N < MIN_FRAMES:
        raise ValueError(f"{N} frames: a scan needs at least {MIN_FRAMES}")
    M = min(N, MAX_SAMPLES)
    return [(k * N) // M for k in range(M)]


def luma(frame):
    f = frame.astype(np.int64)
    return (29 * f[..., 0] + 150 * f[..., 1] + 77 * f[..., 2] + 128) >> 8


def gradient(Y):
    p = np.pad(Y, 1, mode="edge")
    return np.abs(p[1:-1, 2:] - p[1:-1, :-2]) + np.abs(p[2:, 1:-1] - p[:-2, 1:-1])


def accumulate(frames, ge=GE, state=None):
    """(lo, hi, e): int64 [H,W] each, over `frames` (an iterable of uint8 [H,W,3]); state: the triple of the frames before them"""
    lo, hi, e = (None, None, None) if state is None else (s.copy() for s in state)
    for fr in frames:
        Y = luma(fr)
        edge = (gradient(Y) >= ge).astype(np.int64)
        if lo is None:
            lo, hi, e = Y.copy(), Y.copy(), edge
        else:
            lo, hi, e = np.minimum(lo, Y), np.maximum(hi, Y), e + edge
    return lo, hi, e


def dilate(seed, d):
    H, W = seed.shape
    p = np.zeros((H + 2 * d, W + 2 * d), bool)
    p[d:d + H, d:d + W] = seed
    out = np.zeros((H, W), bool)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def classify(lo, hi, e, need, mv=MV, grow=D):
    """(grown, moving): bool [H,W] each"""
    return dilate(e >= need, grow), (hi - lo) >= mv


def components(grown):
    """[(area, y0, y1, x0, x1)] of the 8-connected components of a bool map, boxes half-open: a flood fill, nothing borrowed"""
    H, W = grown.shape
    seen = np.zeros((H, W), bool)
    out = []
    for sy, sx in zip(*np.nonzero(grown)):
        if seen[sy, sx]:
            continue
        seen[sy, sx] = True
        stack, area, y0, y1, x0, x1 = [(int(sy), int(sx))], 0, int(sy), int(sy), int(sx), int(sx)
        while stack:
            y, x = stack.pop()
            area += 1
            y0, y1, x0, x1 = min(y0, y), max(y1, y), min(x0, x), max(x1, x)
            for ny in range(max(y - 1, 0), min(y + 2, H)):
                for nx in range(max(x - 1, 0), min(x + 2, W)):
                    if grown[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
        out.append((area, y0, y1 + 1, x0, x1 + 1))
    return out


def select(comps, moving, info=None):
    """the areas [(ymin, ymax, xmin, xmax)] of the components [(area, y0, y1, x0, x1)].  info, if a list, receives per component
    (box, verdict, moving pixels of the ring, ring pixels), and ("dropped", k) when more than MAX_AREAS were kept"""
    H, W = moving.shape
    kept = []
    for area, y0, y1, x0, x1 in comps:
        ry0, ry1, rx0, rx1 = max(y0 - RING, 0), min(y1 + RING, H), max(x0 - RING, 0), min(x1 + RING, W)
        ring = (ry1 - ry0) * (rx1 - rx0) - (y1 - y0) * (x1 - x0)
        mov = int(moving[ry0:ry1, rx0:rx1].sum()) - int(moving[y0:y1, x0:x1].sum())
        if area < MIN_AREA:
            verdict = "small"
        elif x1 - x0 > W // 3 or y1 - y0 > H // 3:
            verdict = "large"
        elif 2 * mov < ring:
            verdict = "still"
        else:
            verdict = "kept"
            kept.append((area, y0, y1, x0, x1))
        if info is not None:
            info.append(((y0, y1, x0, x1), verdict, mov, ring))
    kept.sort(key=lambda c: (-c[0], c[1], c[3]))
    if len(kept) > MAX_AREAS and info is not None:
        info.append(("dropped", len(kept) - MAX_AREAS))
    boxes = [(max(y0 - PAD, 0), min(y1 + PAD, H), max(x0 - PAD, 0), min(x1 + PAD, W)) for _, y0, y1, x0, x1 in kept[:MAX_AREAS]]
    return sorted(boxes, key=lambda b: (b[0], b[2]))


def areas(clip, info=None):
    """the whole definition on a clip uint8 [N,H,W,3]"""
    idx = sample_indices(len(clip))
    M = len(idx)
    lo, hi, e = accumulate(clip[i] for i in idx)
    grown, moving = classify(lo, hi, e, M - M // 8)
    return select(components(grown), moving, info)


# ---- the clips of the design's table: 40 frames of 144 x 256, a grey diagonal triangle wave that moves 5 pixels a frame ----------------
CLIP_N, CLIP_H, CLIP_W = 40, 144, 256
LOGO = (12, 36, 200, 240)                       # rows [12, 36), columns [200, 240): opaque, 255
LOGO_AREA = (1, 47, 189, 251)                   # the logo's box grown by 1 (the gradient's reach) + D + PAD


def wave(n=CLIP_N, H=CLIP_H, W=CLIP_W, still=False):
    """grey uint8 [n,H,W,3]: t = (x + y + 5 f) % 64, Y = 3 min(t, 64 - t), so g <= 12 everywhere and hi - lo = 96; still: f = 0 throughout"""
    y, x = np.mgrid[0:H, 0:W]
    f = np.zeros(n, np.int64) if still else np.arange(n)
    t = (x[None] + y[None] + 5 * f[:, None, None]) % 64
    return np.repeat((3 * np.minimum(t, 64 - t)).astype(np.uint8)[..., None], 3, axis=3)


def put_logo(clip):
    clip[:, LOGO[0]:LOGO[1], LOGO[2]:LOGO[3]] = 255
    return clip


def clip_logo():
    return put_logo(wave())


def clip_still_logo():
    return put_logo(wave(still=True))


def clip_letterbox_logo():
    c = wave()
    c[:, :16] = 0
    c[:, -16:] = 0
    return put_logo(c)


def clip_plain():
    return wave()


DESK = (60, 100, 30, 90)                        # 40 rows of vertical stripes: its seeds grow to 40 + 2 + 2 D = 54 rows > 144 // 3


def clip_desk_logo():
    c = wave()
    c[:, :, :CLIP_W // 2] = wave(still=True)[:, :, :CLIP_W // 2]
    stripes = np.where((np.arange(DESK[2], DESK[3]) // 4) % 2 == 0, 255, 0).astype(np.uint8)
    c[:, DESK[0]:DESK[1], DESK[2]:DESK[3]] = stripes[None, None, :, None]
    return put_logo(c)
