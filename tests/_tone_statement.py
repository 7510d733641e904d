"""CPU statement of --tone-match S: the fill's tone levelled to the picture across the seam of the composite mask.
Plain numpy, written to be read; the tests use it, the product never imports it.  All integer arithmetic.

For one plugin call on frames [n,h,W,3] that hold the picture rows [y0, y0 + h) of an H x W picture, with the option S (1 <= S <= 100,
a percentage; 0 is off and is the identity):

  src   the frames as they came in
  fill  what the call's body returns
  C     the composite mask, uint8 [H,W] of the FULL picture (tests/_feather_statement.composite_mask, per mode)
  R     [r0, r1): the plugin's sample rows (tests/_regrain_statement.sample_rows)

All coordinates are picture coordinates.

  E      the pixels with C == 0 within Chebyshev distance 2 of a pixel (of the picture) with C != 0        } both only in the rows
  M      the pixels with C != 0 within Chebyshev distance 2 of a pixel (of the picture) with C == 0        } [r0, r1) and the rows held
  cells  a level-k cell (Y, X) covers the picture rows [Y 2^k, (Y + 1) 2^k) and the same columns; the grid at level k is
         ceil(H / 2^k) x ceil(W / 2^k); the finest level is 3, the top level K = max(3, ceil(log2(max(H, W)))) is one cell

per frame, for each of the two sets (the samples are src over E, fill over M) and each channel:
  pull   level 3: N = the number, Sum = the sum of the cell's samples; above: the sum of the 2 x 2 children that exist
  push   mean_k = (64 Sum + N // 2) // N (0 where N == 0), in 1/64 levels;  V_K = mean_K;  for k = K - 1 ... 3:
             U   = the 2x bilinear upsample of V_{k+1} at the cell centres: 9/3/3/1 sixteenths, indices clamped (a numerator over 16)
             T   = 2 * 2^k,  w = min(N, T)
             V_k = (16 w mean_k + (T - w) U + 8 T) // (16 T)
  h3     clamp(V^E_3 - V^M_3, -24 * 64, 24 * 64) per cell and channel
  h(p)   the bilinear interpolation of h3 between the four nearest cell centres (cell X's centre lies at 8 X + 3.5: the per-axis
         weights are the odd sixteenths, indices clamped): a numerator over 256
  out    clamp(fill + (S h + d // 2) // d, 0, 255) with d = 100 * 64 * 256 (floor division) where C != 0, fill elsewhere
  the frame is fill, untouched, where fill == src on all of C in the rows held, or E is empty, or M is empty

(a) `bands_brute`: E and M by their definition, one pixel at a time; (b) `bands`: the separable form; `sets_map`: the byte map the
kernel writes (bit 0 = E, bit 1 = M, bit 2 = C != 0), `cells`: the level-3 cells with a non-zero byte of the map, ascending;
(c) `pull`, `push`, `offset_field`, `tone`: the rest.
"""
import numpy as np

MAX_TONE = 100
BAND = 2                            # E and M reach this far (Chebyshev) across the seam
FINEST = 3                          # 8 x 8 cells
CLAMP = 24 * 64                     # of h3, in 1/64 levels
DEN = 100 * 64 * 256


def bands_brute(C, R):
    C = np.asarray(C)
    H, W = C.shape
    nz = C != 0
    E, M = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for y in range(max(R[0], 0), min(R[1], H)):
        for x in range(W):
            hood = nz[max(0, y - BAND):y + BAND + 1, max(0, x - BAND):x + BAND + 1]        # the frame border is no zero of C
            E[y, x] = (not nz[y, x]) and hood.any()
            M[y, x] = nz[y, x] and not hood.all()
    return E, M


def _any_along(a, axis):
    """a non-zero within BAND along `axis`, positions outside the array counting as none"""
    pad = [(0, 0), (0, 0)]
    pad[axis] = (BAND, BAND)
    p = np.pad(a, pad, constant_values=False)
    out = np.zeros(a.shape, bool)
    for k in range(2 * BAND + 1):
        out |= p[k:k + a.shape[0]] if axis == 0 else p[:, k:k + a.shape[1]]
    return out


def bands(C, R):
    """-> (E, M) bool [H,W]: rows then columns, two 5-wide dilations (of C != 0 and of C == 0)"""
    C = np.asarray(C)
    H, W = C.shape
    nz = C != 0
    rows = np.zeros((H, W), bool)
    rows[max(R[0], 0):max(min(R[1], H), 0)] = True
    near_nz = _any_along(_any_along(nz, 1), 0)
    near_z = _any_along(_any_along(~nz, 1), 0)
    return ~nz & near_nz & rows, nz & near_z & rows


def sets_map(C, R):
    E, M = bands(C, R)
    return (E.astype(np.uint8) | (M.astype(np.uint8) << 1) | ((np.asarray(C) != 0).astype(np.uint8) << 2)).astype(np.uint8)


def grid(H, W, k):
    return -(-H // (1 << k)), -(-W // (1 << k))


def top_level(H, W):
    K = FINEST
    while (1 << K) < max(H, W):
        K += 1
    return K


def cells(C, R):
    """the level-3 cells (Y * ceil(W / 8) + X) that hold a non-zero byte of the map, ascending"""
    m = sets_map(C, R)
    H, W = m.shape
    gh, gw = grid(H, W, FINEST)
    p = np.zeros((gh * 8, gw * 8), bool)
    p[:H, :W] = m != 0
    return np.flatnonzero(p.reshape(gh, 8, gw, 8).any(axis=(1, 3))).astype(np.int32)


def pull(values, where, H, W, y0=0):
    """values uint8 [h,W,3] (the picture rows [y0, y0 + h)), where bool [h,W] -> per level 3..K the pair (N int64 [gh,gw],
    Sum int64 [gh,gw,3])"""
    h = values.shape[0]
    K = top_level(H, W)
    gh, gw = grid(H, W, FINEST)
    wp = np.zeros((gh * 8, gw * 8), np.int64)
    vp = np.zeros((gh * 8, gw * 8, 3), np.int64)
    wp[y0:y0 + h, :W] = where
    vp[y0:y0 + h, :W] = np.asarray(values).astype(np.int64) * where[:, :, None]
    levels = [(wp.reshape(gh, 8, gw, 8).sum(axis=(1, 3)), vp.reshape(gh, 8, gw, 8, 3).sum(axis=(1, 3)))]
    for k in range(FINEST + 1, K + 1):
        N, S = levels[-1]
        gh, gw = grid(H, W, k)
        Np = np.zeros((2 * gh, 2 * gw), np.int64)
        Sp = np.zeros((2 * gh, 2 * gw, 3), np.int64)
        Np[:N.shape[0], :N.shape[1]] = N                     # children that do not exist count as zero
        Sp[:S.shape[0], :S.shape[1]] = S
        levels.append((Np.reshape(gh, 2, gw, 2).sum(axis=(1, 3)), Sp.reshape(gh, 2, gw, 2, 3).sum(axis=(1, 3))))
    return levels


def mean64(N, S):
    """(64 Sum + N // 2) // N, 0 where N == 0: int64 [gh,gw,3]"""
    n = np.maximum(N, 1)[:, :, None]
    return np.where(N[:, :, None] > 0, (64 * S + n // 2) // n, 0)


def upsample(V, gh, gw):
    """V int64 [ph,pw,3] of the level above -> its 2x bilinear upsample at the gh x gw cell centres, a numerator over 16"""
    ph, pw = V.shape[:2]
    Y, X = np.arange(gh), np.arange(gw)
    ya, xa = Y >> 1, X >> 1                                           # the parent: 3 of 4 per axis
    yb = np.clip(ya + np.where(Y & 1, 1, -1), 0, ph - 1)              # the neighbour on the cell's side of it: 1 of 4
    xb = np.clip(xa + np.where(X & 1, 1, -1), 0, pw - 1)
    return (9 * V[ya][:, xa] + 3 * V[ya][:, xb] + 3 * V[yb][:, xa] + V[yb][:, xb])


def push(levels, H, W):
    """the levels of `pull` -> V_3, int64 [gh,gw,3] in 1/64 levels"""
    K = top_level(H, W)
    V = mean64(*levels[K - FINEST])
    for k in range(K - 1, FINEST - 1, -1):
        N, S = levels[k - FINEST]
        gh, gw = grid(H, W, k)
        U = upsample(V, gh, gw)
        T = 2 << k
        w = np.minimum(N, T)[:, :, None]
        V = (16 * w * mean64(N, S) + (T - w) * U + 8 * T) // (16 * T)
    return V


def offset_field(h3, H, W, y0, rows):
    """h3 int64 [gh,gw,3] -> h int64 [rows,W,3] on the picture rows [y0, y0 + rows): a numerator over 256"""
    gh, gw = h3.shape[:2]

    def axis(p, g):
        a = (p - 4) >> 3                                              # the cell whose centre lies before p (-1: none, clamped)
        w1 = 2 * ((p - 4) & 7) + 1
        return np.clip(a, 0, g - 1), np.clip(a + 1, 0, g - 1), 16 - w1, w1

    ya, yb, wya, wyb = axis(np.arange(y0, y0 + rows), gh)
    xa, xb, wxa, wxb = axis(np.arange(W), gw)
    wya, wyb, wxa, wxb = wya[:, None, None], wyb[:, None, None], wxa[None, :, None], wxb[None, :, None]
    return wya * (wxa * h3[ya][:, xa] + wxb * h3[ya][:, xb]) + wyb * (wxa * h3[yb][:, xa] + wxb * h3[yb][:, xb])


def tone(fill, src, C, R, S, y0=0, info=None):
    """fill, src uint8 [n, h, W, 3]: the rows [y0, y0 + h) of the frames (the whole frames: y0 = 0, h = H) -> uint8, the same shape.
    info: a list that receives (N_E, N_M, changed, touched, h3) per frame."""
    fill, src, C = np.asarray(fill), np.asarray(src), np.asarray(C)
    H, W = C.shape
    n, h = fill.shape[:2]
    assert fill.shape == src.shape == (n, h, W, 3) and 0 <= y0 and y0 + h <= H and 0 <= S <= MAX_TONE
    assert 0 <= R[0] <= R[1] <= H
    E, M = bands(C, R)
    E, M, Cnz = E[y0:y0 + h], M[y0:y0 + h], (C != 0)[y0:y0 + h]
    n_e, n_m = int(E.sum()), int(M.sum())
    out = fill.copy()
    for t in range(n):
        changed = bool((fill[t][Cnz] != src[t][Cnz]).any())
        touched = bool(S and n_e and n_m and changed)
        h3 = None
        if touched:
            v_e = push(pull(src[t], E, H, W, y0), H, W)
            v_m = push(pull(fill[t], M, H, W, y0), H, W)
            h3 = np.clip(v_e - v_m, -CLAMP, CLAMP)
            g = (S * offset_field(h3, H, W, y0, h) + DEN // 2) // DEN
            out[t] = np.where(Cnz[:, :, None], np.clip(fill[t].astype(np.int64) + g, 0, 255), fill[t]).astype(np.uint8)
        if info is not None:
            info.append((n_e, n_m, changed, touched, h3))
    return out
