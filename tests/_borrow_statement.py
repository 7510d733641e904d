"""The definition of --borrow B in plain numpy: the kernels of csrc/borrow_kernels.hip are held to it byte for byte.
Plain numpy, written to be read; the tests use it, the product never imports it.  All arithmetic is in integers.

For one plugin call on frames [n,h,W,3] that hold the rows [y0, y0 + h) of the picture, the options T of --glyph-key (1 <= T <= 128)
and B (1 <= B <= 8, a radius in frames; 0, or fewer than two frames, is off and is the identity):
    src   the frames as they came in          fill  the frames as they stand when the pass runs
    C     the composite mask of the whole picture, uint8 [H,W]
    rows  [r0, r1): the plugin's sample rows (tests/_regrain_statement.sample_rows)
    E     the ring set of --regrain over those rows (tests/_regrain_statement.sets), m = 3 |E|
    G = R = 4 the key's constants (tests/_key_statement.py), TH = 24 deflicker's (tests/_deflicker_statement.py)

    Z(t,p)   the key's seeds at T on fill against src: _key_statement.seeds, called
    N(t,p)   = 1 iff e(t,p) < G + R, e the key's Chebyshev distance to the nearest seed of frame t among the rows held: the 15 x 15
             square around p holds a seed.  These are the pixels where the key's weight a > 0.  --glyph-hold does not enter.
    b(t,k)   in 0..16 for 1 <= k <= B, t + k < n: deflicker's pair weight WITHOUT its "changed" rule (a frame the call did not inpaint has
             no glyph anywhere and is the best lender there is):
             b = 0 if m == 0, else floor = (15447 (A[t] + A[t+k])) >> 17, X = max(0, S[t][k] - floor),
             b = clamp((16 (4 m - X)) // (3 m), 0, 16); A[t] = the sum over E of Immerkaer's operator on src_t, S deflicker's pair sums
    borrower a pixel p of C in the rows held with N(t,p) = 1
    lenders  tried in the order t-1, t+1, t-2, t+2, .. t-B, t+B, those inside [0, n): frame s lends iff N(s,p) = 0 and
             max_c |src_s[p][c] - fill_t[p][c]| < (TH b(min(t,s), |t-s|)) >> 4
             the first that passes wins: out_t[p] = src_s[p], all three channels; none: the fill stays
Everything else is the fill, bit for bit.  One lender, not an average: the borrowed pixel keeps its own grain.
"""
import numpy as np

from tests import _deflicker_statement as ds
from tests import _key_statement as ks
from tests import _regrain_statement as rs

MAX_BORROW = 8
TH = ds.TH
FULL = ds.FULL


def near(Z):
    """N: bool [n,h,W], the pixels within G + R - 1 of a seed of their own frame"""
    return ks.distance(Z) < ks.G + ks.R


def near_words(words):
    """N from the seed bitmap, bit-parallel as the kernel forms it: every row's words dilated by G + R - 1 bits, then the OR over the
    rows y - (G + R - 1) .. y + (G + R - 1), clipped"""
    k = ks.G + ks.R - 1
    Hk = ks.dilate_words(words, k)
    h = words.shape[1]
    out = np.zeros_like(Hk)
    for y in range(h):
        out[:, y] = np.bitwise_or.reduce(Hk[:, max(y - k, 0):min(y + k, h - 1) + 1], axis=1)
    return out


def pair_weight(S_tk, A_t, A_u, m):
    if m == 0:
        return 0
    X = max(0, int(S_tk) - ((ds.GRAIN * (int(A_t) + int(A_u))) >> 17))
    return min(FULL, max(0, (FULL * (4 * m - X)) // (3 * m)))


def threshold(b):
    return (TH * b) >> 4


def lenders(t, n, B):
    """the frames tried for frame t, in order"""
    out = []
    for k in range(1, B + 1):
        out += [s for s in (t - k, t + k) if 0 <= s < n]
    return out


def borrow(fill, src, C, rows, T, B, y0=0, info=None):
    """fill, src uint8 [n, h, W, 3]: the rows [y0, y0 + h) of the frames (the whole frames: y0 = 0, h = H) -> uint8, the same shape.
    info: a dict that receives "Z", "N" (bool [n,h,W]), "S", "A", "m", "b" ({(t, k): weight}), "lender" (int64 [n,h,W]: the frame a pixel
    was taken from, -1 = none), "borrowers" (bool [n,h,W]) and the counts "refused_near" (lenders passed over for their own glyph),
    "refused_threshold" (passed over by an open pair's threshold) and "refused_closed" (by a closed pair)."""
    fill, src, C = np.asarray(fill), np.asarray(src), np.asarray(C)
    assert fill.dtype == np.uint8 and src.dtype == np.uint8
    H, W = C.shape
    n, h = fill.shape[:2]
    assert fill.shape == src.shape == (n, h, W, 3) and 0 <= y0 and y0 + h <= H and 0 <= B <= MAX_BORROW
    assert 0 <= rows[0] <= rows[1] <= H
    out = fill.copy()
    if n < 2 or B == 0:
        return out
    E, _ = rs.sets(C, rows)
    m = 3 * int(E.sum())
    E, Cnz = E[y0:y0 + h].copy(), (C != 0)[y0:y0 + h]
    assert m == 3 * int(E.sum()), "the rows held must cover E"
    Z = ks.seeds(fill, src, C, T, y0)
    N = near(Z)
    A = [int(rs.noise_level(src[t])[E].sum()) for t in range(n)]
    S = ds.pair_sums(src, E, B)
    b = {(t, k): pair_weight(S[t, k - 1], A[t], A[t + k], m) for t in range(n) for k in range(1, B + 1) if t + k < n}
    f, s64 = fill.astype(np.int64), src.astype(np.int64)
    lender = np.full((n, h, W), -1, np.int64)
    counts = dict(refused_near=0, refused_threshold=0, refused_closed=0)
    for t in range(n):
        want = Cnz & N[t]                                   # the borrowers still without a lender
        for s in lenders(t, n, B):
            th = threshold(b[(min(t, s), abs(t - s))])
            D = np.abs(s64[s] - f[t]).max(axis=-1)
            counts["refused_near"] += int((want & N[s]).sum())
            if th == 0:
                counts["refused_closed"] += int((want & ~N[s]).sum())
                continue
            counts["refused_threshold"] += int((want & ~N[s] & (D >= th)).sum())
            take = want & ~N[s] & (D < th)
            out[t][take] = src[s][take]
            lender[t][take] = s
            want = want & ~take
    if info is not None:
        info.update(Z=Z, N=N, S=S, A=A, m=m, b=b, lender=lender, borrowers=Cnz[None] & N, **counts)
    return out


def workspace_bytes(H, W, n):
    """the documented size of vsr_borrow_apply's workspace: two bitmaps of the key's size"""
    return 2 * ks.workspace_bytes(H, W, n)
