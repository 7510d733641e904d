"""CPU statement of --regrain P: the source's grain, measured next to the mask, put back inside the inpainted pixels.
Plain numpy, written to be read; the tests use it, the product never imports it.  All integer arithmetic.

For one plugin call on frames [n,H,W,3] with mask M and the option P (1 <= P <= 200, a percentage; 0 is off and is the identity):

  src   the frames as they came in
  fill  what the call's body returns
  C     the composite mask, uint8 [H,W] of the FULL frame (tests/_feather_statement.composite_mask, per mode)
  R     [r0, r1): the plugin's sample rows (sample_rows below): the rows every one of its loops holds

All coordinates are full-frame coordinates.  A loop that holds the rows [y0, y0 + h) of the frames only (sttn-auto's strip rows: y0 = r0,
h = r1 - r0) states the same thing about those rows: `regrain(fill, src, C, R, P, y0=y0)` with fill, src of h rows.  Pixels of C outside
the rows held take no part (no plugin has any: sttn-auto's C lies inside its strips).

  N      the 3x3 kernel [[1,-2,1],[-2,4,-2],[1,-2,1]] (Immerkaer's noise operator: blind to planes and straight edges)
  L(x)(p) = sum over the three channels of |(N * x_c)(p)|
  inner  r0 + 1 <= y < r1 - 1 and 1 <= x < W - 1
  I      the pixels of inner whose whole 3x3 neighbourhood has C != 0
  E      the pixels of inner whose whole 3x3 neighbourhood has C == 0 and that lie within Chebyshev distance 16 of a pixel with C != 0

per frame t:   A_src = sum over E of L(src_t), A_fill = sum over I of L(fill_t)
               E or I empty, or fill_t == src_t on every pixel of C: the frame is fill_t, untouched
               q_src = (A_src << 8) // (3 |E|), q_fill = (A_fill << 8) // (3 |I|), r = isqrt(max(0, q_src^2 - q_fill^2))
               seed = low32(A_src) xor high32(A_src)
per pixel:     h = mix(mix((y * W + x) xor seed) + 0x9e3779b9), z = (sum of the four bytes of h) - 510
               g = (r * P * GAIN * z + 2^39) >> 40 (floor), the same value on all three channels
               out = clamp(fill + g, 0, 255) where C != 0, fill elsewhere

(a) `sets_brute`: E and I by their definition, one pixel at a time; (b) `sets`: the separable passes the kernel runs; `sets_map`: the
byte map the kernel writes (bit 0 = E, bit 1 = I, bit 2 = C != 0).  (c) `measure`, `deficit`, `grain`, `regrain`: the rest.
"""
import math

import numpy as np

MAX_REGRAIN = 200
RING = 16                           # E reaches this far (Chebyshev) from C
GAIN = 60701                        # round(2^40 * (sqrt(pi / 2) / 6) / (sqrt(65535 / 3) * 100 * 256))
assert GAIN == round(2 ** 40 * (math.sqrt(math.pi / 2) / 6) / (math.sqrt(65535 / 3) * 100 * 256))


def sample_rows(mode, M):
    """R per mode: sttn-auto the hull of its inpaint areas' rows, every other mode the whole frame"""
    M = np.asarray(M)
    H, W = M.shape[:2]
    if mode != "sttn-auto":
        return 0, H
    from vsr_amd.backend.tools.inpaint_tools import get_inpaint_area_by_mask

    T = (M.reshape(H, W) > 127).astype(np.uint8)
    areas = get_inpaint_area_by_mask(W, H, int(W * 3 / 16), T.reshape(H, W, 1))
    return (min(a[0] for a in areas), max(a[1] for a in areas)) if areas else (0, 0)


def sets_brute(C, R):
    C = np.asarray(C)
    H, W = C.shape
    nz = C != 0
    E, I = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for y in range(max(R[0] + 1, 1), min(R[1] - 1, H - 1)):
        for x in range(1, W - 1):
            hood = nz[y - 1:y + 2, x - 1:x + 2]
            I[y, x] = hood.all()
            E[y, x] = not hood.any() and nz[max(0, y - RING):y + RING + 1, max(0, x - RING):x + RING + 1].any()
    return E, I


def _along(a, radius, axis, op, outside):
    """op over the window of `radius` along `axis`, positions outside the array counting as `outside`"""
    pad = [(0, 0), (0, 0)]
    pad[axis] = (radius, radius)
    p = np.pad(a, pad, constant_values=outside)
    out = np.zeros(a.shape, bool) if op is np.logical_or else np.ones(a.shape, bool)
    for k in range(2 * radius + 1):
        out = op(out, p[k:k + a.shape[0]] if axis == 0 else p[:, k:k + a.shape[1]])
    return out


def sets(C, R):
    """-> (E, I) bool [H,W]: rows then columns, as the kernel: 3-wide erosions of C != 0 and of C == 0, a 33-wide dilation of C != 0"""
    C = np.asarray(C)
    H, W = C.shape
    nz = C != 0
    inner = np.zeros((H, W), bool)
    inner[max(R[0] + 1, 1):max(min(R[1] - 1, H - 1), 0), 1:W - 1] = True
    all_nz = _along(_along(nz, 1, 1, np.logical_and, False), 1, 0, np.logical_and, False)
    all_z = _along(_along(~nz, 1, 1, np.logical_and, False), 1, 0, np.logical_and, False)
    near = _along(_along(nz, RING, 1, np.logical_or, False), RING, 0, np.logical_or, False)
    return all_z & near & inner, all_nz & inner


def sets_map(C, R):
    E, I = sets(C, R)
    return (E.astype(np.uint8) | (I.astype(np.uint8) << 1) | ((np.asarray(C) != 0).astype(np.uint8) << 2)).astype(np.uint8)


def noise_level(x):
    """L(x): int64 [..., H, W], zero on the one-pixel border of the rows held (where N does not fit)"""
    x = np.asarray(x).astype(np.int64)
    h = x[..., :, :-2, :] - 2 * x[..., :, 1:-1, :] + x[..., :, 2:, :]                 # along the row
    v = h[..., :-2, :, :] - 2 * h[..., 1:-1, :, :] + h[..., 2:, :, :]                 # down the column
    out = np.zeros(x.shape[:-1], np.int64)
    out[..., 1:-1, 1:-1] = np.abs(v).sum(axis=-1)
    return out


def isqrt(v):
    return math.isqrt(int(v))


def measure(fill_t, src_t, E, I, Cnz):
    """one frame (the rows held) -> (A_src, A_fill, changed)"""
    a_src = int(noise_level(src_t)[E].sum())
    a_fill = int(noise_level(fill_t)[I].sum())
    changed = bool((np.asarray(fill_t)[Cnz] != np.asarray(src_t)[Cnz]).any())
    return a_src, a_fill, changed


def deficit(a_src, a_fill, n_e, n_i):
    """-> (r, seed)"""
    q_src = (a_src << 8) // (3 * n_e)
    q_fill = (a_fill << 8) // (3 * n_i)
    return isqrt(max(0, q_src * q_src - q_fill * q_fill)), (a_src & 0xffffffff) ^ ((a_src >> 32) & 0xffffffff)


def mix(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x7feb352d)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x846ca68b)
    h ^= h >> np.uint32(16)
    return h


def grain(H, W, seed, r, P, y0=0, rows=None):
    """g int64 [rows, W] for the rows [y0, y0 + rows) of an H x W frame"""
    rows = H - y0 if rows is None else rows
    with np.errstate(over="ignore"):
        idx = ((np.arange(y0, y0 + rows, dtype=np.int64)[:, None] * W + np.arange(W, dtype=np.int64)[None, :]) & 0xffffffff).astype(np.uint32)
        h = mix(mix(idx ^ np.uint32(seed)) + np.uint32(0x9e3779b9))
    z = ((h & 0xff) + ((h >> 8) & 0xff) + ((h >> 16) & 0xff) + (h >> 24)).astype(np.int64) - 510
    k = int(r) * int(P) * GAIN
    assert k * 510 + 2 ** 39 < 2 ** 63
    return (k * z + 2 ** 39) >> 40


def regrain(fill, src, C, R, P, y0=0, info=None):
    """fill, src uint8 [n, h, W, 3]: the rows [y0, y0 + h) of the frames (the whole frames: y0 = 0, h = H) -> uint8, the same shape.
    info: a list that receives (A_src, A_fill, changed, r, seed, touched) per frame."""
    fill, src, C = np.asarray(fill), np.asarray(src), np.asarray(C)
    H, W = C.shape
    n, h = fill.shape[:2]
    assert fill.shape == src.shape == (n, h, W, 3) and 0 <= y0 and y0 + h <= H and 0 <= P <= MAX_REGRAIN
    assert 0 <= R[0] <= R[1] <= H
    E, I = sets(C, R)
    # the rows held: a sample needs its 3x3 neighbourhood in them (always so when they are R's or the frame's)
    E, I, Cnz = E[y0:y0 + h].copy(), I[y0:y0 + h].copy(), (C != 0)[y0:y0 + h]
    assert not (E[[0, -1]].any() or I[[0, -1]].any()), "the rows held must cover R"
    n_e, n_i = int(E.sum()), int(I.sum())
    out = fill.copy()
    for t in range(n):
        a_src, a_fill, changed = measure(fill[t], src[t], E, I, Cnz)
        touched = bool(P and n_e and n_i and changed)
        r, seed = deficit(a_src, a_fill, n_e, n_i) if (n_e and n_i) else (0, 0)
        if touched:
            g = grain(H, W, seed, r, P, y0, h)
            out[t] = np.where(Cnz[:, :, None], np.clip(fill[t].astype(np.int64) + g[:, :, None], 0, 255), fill[t]).astype(np.uint8)
        if info is not None:
            info.append((a_src, a_fill, changed, r, seed, touched))
    return out
