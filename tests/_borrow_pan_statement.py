"""The definition of --borrow-pan P in plain numpy: --borrow B (tests/_borrow_statement.py) made to follow a camera
that pans by a whole number of pixels per frame.  The kernels of csrc/borrow_pan_kernels.hip are held to it byte for byte.  Plain
numpy, written to be read; the tests use it, the product never imports it.  All arithmetic is in integers.

src, fill, C, rows, E, m = 3 |E|, A[t], Z, N, T, B, TH = 24, GRAIN are 4.18's.  P (1 <= P <= 8; 0 is off and is 4.18 itself) is a search
radius in pixels per frame step.  p = (y, x) is a position in the rows held [0, h) x [0, W), d = (dy, dx) a shift.

    V(q)        q lies inside [0, h) x [0, W) and C[y0 + q.y, q.x] == 0 (E is a subset of V)
    E_d         the p of E with V(p + d); cnt(d) = |E_d| (the mask alone decides both)
    S(t,k,d)    the sum over E_d and the channels of |src_t[p] - src_{t+k}[p + d]|; d = 0 gives 4.13's S[t][k] and cnt = |E|
    eligible    |E| > 0 and 2 cnt(d) >= |E|
    d beats e   S_d cnt(e) < S_e cnt(d); a tie goes to the earlier in the order of ascending (max(|dy|,|dx|), |dy|+|dx|, dy, dx)
    candidates  k = 1: every d with |dy|, |dx| <= P, slot (dy + P)(2 P + 1) + dx + P
                k >= 2: the centre c = R(t,k-1) + R(t+k-1,1); slots 0..8 hold c + (ey, ex), slot 3 (ey + 1) + ex + 1, those with
                |.|inf <= k P and != (0,0); slot 9 holds (0,0)
    R(t,k)      the raw best: the eligible candidate that no other beats ((0,0) where |E| = 0)
    b_d         m_d = 3 cnt(d), floor_d = (((GRAIN (A[t] + A[t+k])) >> 17) cnt(d)) // |E|, X = max(0, S - floor_d),
                b_d = clamp((16 (4 m_d - X)) // (3 m_d), 0, 16); b_0 is 4.18's b(t,k)
    D(t,k)      0 if b_0 == 16, R == 0 or b_R <= b_0, else R(t,k); the pair's weight w(t,k) = b_D
    lender      of a borrower p of frame t, tried in 4.18's order: s = t + k looks at q = p + D(t,k), s = t - k at q = p - D(s,k); s
                lends iff q lies inside the rows held, C[q] == 0 or N(s,q) == 0, and max_c |src_s[q] - fill_t[p]| < (TH w) >> 4;
                the first wins: out_t[p] = src_s[q]; none: the fill stays
"""
import numpy as np

from tests import _borrow_statement as bs
from tests import _deflicker_statement as ds
from tests import _key_statement as ks
from tests import _regrain_statement as rs

MAX_PAN = 8
TH, FULL, GRAIN = ds.TH, ds.FULL, ds.GRAIN
LATER = 10                                                   # the slots of a level k >= 2


def slots(P):
    """the slots of a table row"""
    return max((2 * P + 1) ** 2, LATER)


def order(d):
    return max(abs(d[0]), abs(d[1])), abs(d[0]) + abs(d[1]), d[0], d[1]


def candidates(k, P, centre=(0, 0)):
    """the shift of every slot of level k, None: the slot is empty"""
    if k == 1:
        return [(dy, dx) for dy in range(-P, P + 1) for dx in range(-P, P + 1)]
    out = []
    for ey in (-1, 0, 1):
        for ex in (-1, 0, 1):
            d = (centre[0] + ey, centre[1] + ex)
            out.append(d if max(abs(d[0]), abs(d[1])) <= k * P and d != (0, 0) else None)
    return out + [(0, 0)]


def shift_sums(a, u, E, V, d):
    """(S, cnt) of the shift d between the frames a and u (int64 [h,W,3])"""
    h, W = E.shape
    ys, xs = np.nonzero(E)
    qy, qx = ys + d[0], xs + d[1]
    ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < W)
    ok[ok] = V[qy[ok], qx[ok]]
    return int(np.abs(a[ys[ok], xs[ok]] - u[qy[ok], qx[ok]]).sum()), int(ok.sum())


def raw_best(cands, S, cnt, n_e):
    """R: the eligible candidate that no other beats"""
    best = None
    for i in sorted((i for i, d in enumerate(cands) if d is not None), key=lambda i: order(cands[i])):
        if n_e <= 0 or 2 * cnt[i] < n_e:
            continue
        if best is None or int(S[i]) * int(cnt[best]) < int(S[best]) * int(cnt[i]):
            best = i
    return (0, 0) if best is None else cands[best]


def weight(S, cnt, A_t, A_u, n_e):
    """b_d"""
    if n_e == 0 or cnt == 0:
        return 0
    m = 3 * int(cnt)
    X = max(0, int(S) - (((GRAIN * (int(A_t) + int(A_u))) >> 17) * int(cnt)) // n_e)
    return min(FULL, max(0, (FULL * (4 * m - X)) // (3 * m)))


def search(src, E, V, A, B, P):
    """the tables and what follows from them: dict of S, cnt (int64 [n][B][slots]), cands, R, D, w, b0, bR ({(t, k): ..})"""
    s64 = np.asarray(src).astype(np.int64)
    n, n_e, nc = s64.shape[0], int(E.sum()), slots(P)
    S, cnt = np.zeros((n, B, nc), np.int64), np.zeros((n, B, nc), np.int64)
    cands, R, D, w, b0, bR = {}, {}, {}, {}, {}, {}
    for k in range(1, B + 1):
        for t in range(n - k):
            c = (0, 0)
            if k > 1:
                c = (R[(t, k - 1)][0] + R[(t + k - 1, 1)][0], R[(t, k - 1)][1] + R[(t + k - 1, 1)][1])
            cs = candidates(k, P, c)
            for i, d in enumerate(cs):
                if d is not None:
                    S[t, k - 1, i], cnt[t, k - 1, i] = shift_sums(s64[t], s64[t + k], E, V, d)
            r = raw_best(cs, S[t, k - 1], cnt[t, k - 1], n_e)
            i0, ir = cs.index((0, 0)), cs.index(r)
            z = weight(S[t, k - 1, i0], cnt[t, k - 1, i0], A[t], A[t + k], n_e)
            br = weight(S[t, k - 1, ir], cnt[t, k - 1, ir], A[t], A[t + k], n_e)
            d = (0, 0) if (z == FULL or r == (0, 0) or br <= z) else r
            cands[(t, k)], R[(t, k)], D[(t, k)], b0[(t, k)], bR[(t, k)] = cs, r, d, z, br
            w[(t, k)] = br if d != (0, 0) else z
    return dict(S=S, cnt=cnt, cands=cands, R=R, D=D, w=w, b0=b0, bR=bR)


def borrow_pan(fill, src, C, rows, T, B, P, y0=0, info=None):
    """fill, src uint8 [n, h, W, 3]: the rows [y0, y0 + h) of the frames -> uint8, the same shape.  info: a dict that receives Z, N, A,
    m, the tables "S" and "cnt" (int64 [n][B][slots(P)]), "cands", "R", "D", "w", "b0", "bR" ({(t, k): ..}), "lender" (int64 [n,h,W],
    -1 = none), "q" (int64 [n,h,W,2], the lender's pixel), "borrowers", "Cnz" (C != 0 in the rows held) and the counts "refused_offframe" (q outside the rows held),
    "refused_near" (the lender's own glyph at q), "refused_threshold" and "refused_closed"."""
    fill, src, C = np.asarray(fill), np.asarray(src), np.asarray(C)
    assert 0 <= P <= MAX_PAN
    if P == 0:
        return bs.borrow(fill, src, C, rows, T, B, y0=y0, info=info)
    assert fill.dtype == np.uint8 and src.dtype == np.uint8
    H, W = C.shape
    n, h = fill.shape[:2]
    assert fill.shape == src.shape == (n, h, W, 3) and 0 <= y0 and y0 + h <= H and 0 <= B <= bs.MAX_BORROW
    out = fill.copy()
    if n < 2 or B == 0:
        return out
    E, _ = rs.sets(C, rows)
    n_e = int(E.sum())
    E, Cnz = E[y0:y0 + h].copy(), (C != 0)[y0:y0 + h]
    assert n_e == int(E.sum()), "the rows held must cover E"
    Z = ks.seeds(fill, src, C, T, y0)
    N = bs.near(Z)
    A = [int(rs.noise_level(src[t])[E].sum()) for t in range(n)]
    found = search(src, E, ~Cnz, A, B, P)
    f, s64 = fill.astype(np.int64), src.astype(np.int64)
    lender = np.full((n, h, W), -1, np.int64)
    where = np.full((n, h, W, 2), -1, np.int64)
    counts = dict(refused_offframe=0, refused_near=0, refused_threshold=0, refused_closed=0)
    yy, xx = np.mgrid[0:h, 0:W]
    for t in range(n):
        want = Cnz & N[t]                                   # the borrowers still without a lender
        for s in bs.lenders(t, n, B):
            k = abs(s - t)
            d = found["D"][(t, k)] if s > t else tuple(-v for v in found["D"][(s, k)])
            th = bs.threshold(found["w"][(min(t, s), k)])
            qy, qx = yy + d[0], xx + d[1]
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < W)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, W - 1)
            free = inside & ~(Cnz[qy, qx] & N[s][qy, qx])
            theirs = s64[s][qy, qx]
            dist = np.abs(theirs - f[t]).max(axis=-1)
            counts["refused_offframe"] += int((want & ~inside).sum())
            counts["refused_near"] += int((want & inside & ~free).sum())
            if th == 0:
                counts["refused_closed"] += int((want & free).sum())
                continue
            counts["refused_threshold"] += int((want & free & (dist >= th)).sum())
            take = want & free & (dist < th)
            out[t][take] = theirs[take].astype(np.uint8)
            lender[t][take] = s
            where[t][take] = np.stack([qy, qx], axis=-1)[take]
            want = want & ~take
    if info is not None:
        info.update(Z=Z, N=N, A=A, m=3 * n_e, lender=lender, q=where, borrowers=Cnz[None] & N, Cnz=Cnz, **found, **counts)
    return out


def table_words(n, B, P):
    """the 64-bit words of the table at the front of the workspace: [n][B][slots(P) + 1][2], (S, cnt) per slot; the last pair of a row
    is the kernels' own (the centre of the level)"""
    return n * B * (slots(P) + 1) * 2


def workspace_bytes(H, W, n, B, P):
    """the documented size of the workspace: the table, one word per (t, k) of chosen shifts, two bitmaps of the key's size"""
    return 8 * (table_words(n, B, P) + n * B) + 2 * ks.workspace_bytes(H, W, n)
