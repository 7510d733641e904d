"""CPU statement of --deflicker R: the fill steadied over time inside the inpainted pixels, gated by how much the real
picture around them moved.  Plain numpy, written to be read; the tests use it, the product never imports it.  All integer arithmetic.

For one plugin call on frames [n,H,W,3] with mask M and the option R (1 <= R <= 8, a radius in frames; 0 is off and is the identity):

  src   the frames as they came in
  fill  what the call's body returns
  C     the composite mask, uint8 [H,W] of the FULL frame (tests/_feather_statement.composite_mask, per mode)
  rows  [r0, r1): the plugin's sample rows (tests/_regrain_statement.sample_rows)
  E     the ring set of --regrain over those rows (tests/_regrain_statement.sets), m = 3 |E|

All coordinates are full-frame coordinates; a loop that holds the rows [y0, y0 + h) of the frames only states the same thing about those
rows (`deflicker(fill, src, C, rows, R, y0=y0)`), as tests/_regrain_statement.py does.

per frame t:     changed[t] = the number of pixels of C with fill_t != src_t, A[t] = the sum over E of Immerkaer's operator on src_t:
                 words 2 and 0 of vsr_regrain_measure (tests/_regrain_statement.measure)
per pair (t, k), 1 <= k <= R, t + k < n:
                 S[t][k] = sum over E and the channels of |src_t - src_{t+k}|            how much the real picture around the band moved
                 a(t, k) = 0 if m == 0 or changed[t] == 0 or changed[t+k] == 0, else
                           floor = (15447 (A[t] + A[t+k])) >> 17        what the source's own grain contributes to S
                           X = max(0, S[t][k] - floor)
                           a = clamp((16 (4 m - X)) // (3 m), 0, 16)    full up to 1 level of real change per sample, none from 4 on
per pixel p of C in a frame t with changed[t] > 0 (TH = 24):
                 num_c = 16 TH fill_t[p][c], den = 16 TH
                 every s in [t - R, t + R], 0 <= s < n, s != t, with a = a(min(t, s), |t - s|) > 0 and
                 D = max_c |fill_s[p][c] - fill_t[p][c]| < TH adds w = a (TH - D): num_c += w fill_s[p][c], den += w
                 out_t[p][c] = (num_c + den // 2) // den
The neighbours are always the unsmoothed fill.  Everything else -- pixels outside C, frames with changed == 0 -- is fill, bit for bit.
"""
import math

import numpy as np

from tests import _regrain_statement as rs

MAX_DEFLICKER = 8
TH = 24                             # a fill that differs by this much at a pixel is other content there, not flicker
FULL = 16                           # the pair weight's scale
GRAIN = 15447                       # round(2^16 * sqrt(2) / 6): 2^-16 GRAIN * (mean Immerkaer response) = mean |frame difference| of pure grain
assert GRAIN == round(2 ** 16 * math.sqrt(2) / 6)


def pair_sums(src, E, R):
    """S: int64 [n][R], S[t][k-1] for t + k < n, 0 elsewhere"""
    src = np.asarray(src).astype(np.int64)
    n = src.shape[0]
    S = np.zeros((n, R), np.int64)
    for t in range(n):
        for k in range(1, R + 1):
            if t + k < n:
                S[t, k - 1] = int(np.abs(src[t][E] - src[t + k][E]).sum())
    return S


def pair_weight(S_tk, A_t, A_u, changed_t, changed_u, m):
    if m == 0 or not changed_t or not changed_u:
        return 0
    X = max(0, int(S_tk) - ((GRAIN * (int(A_t) + int(A_u))) >> 17))
    return min(FULL, max(0, (FULL * (4 * m - X)) // (3 * m)))


def deflicker(fill, src, C, rows, R, y0=0, info=None):
    """fill, src uint8 [n, h, W, 3]: the rows [y0, y0 + h) of the frames (the whole frames: y0 = 0, h = H) -> uint8, the same shape.
    info: a dict that receives "S" (int64 [n][R]), "A", "changed" (per frame) and "a" ({(t, k): weight})."""
    fill, src, C = np.asarray(fill), np.asarray(src), np.asarray(C)
    H, W = C.shape
    n, h = fill.shape[:2]
    assert fill.shape == src.shape == (n, h, W, 3) and 0 <= y0 and y0 + h <= H and 0 <= R <= MAX_DEFLICKER
    assert 0 <= rows[0] <= rows[1] <= H
    E, I = rs.sets(C, rows)
    m = 3 * int(E.sum())
    E, I, Cnz = E[y0:y0 + h].copy(), I[y0:y0 + h].copy(), (C != 0)[y0:y0 + h]
    assert m == 3 * int(E.sum()), "the rows held must cover E"
    out = fill.copy()
    A, changed = [], []
    for t in range(n):
        a_src, _, ch = rs.measure(fill[t], src[t], E, I, Cnz)
        A.append(a_src)
        changed.append(ch)
    S = pair_sums(src, E, R)
    a = {(t, k): pair_weight(S[t, k - 1], A[t], A[t + k], changed[t], changed[t + k], m)
         for t in range(n) for k in range(1, R + 1) if t + k < n}
    if info is not None:
        info.update(S=S, A=A, changed=changed, a=a, m=m)
    f = fill.astype(np.int64)
    for t in range(n):
        if not changed[t]:
            continue
        num = FULL * TH * f[t]
        den = np.full((h, W), FULL * TH, np.int64)
        for s in range(max(0, t - R), min(n, t + R + 1)):
            w_pair = a[(min(t, s), abs(t - s))] if s != t else 0
            if w_pair <= 0:
                continue
            D = np.abs(f[s] - f[t]).max(axis=-1)
            w = np.where(D < TH, w_pair * (TH - D), 0)
            num = num + w[:, :, None] * f[s]
            den = den + w
        res = (num + (den // 2)[:, :, None]) // den[:, :, None]
        out[t] = np.where(Cnz[:, :, None], res, fill[t]).astype(np.uint8)
    return out
