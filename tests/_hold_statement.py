"""The definition of --glyph-hold K in plain numpy: hysteresis in time for --glyph-key T.  The kernels of
csrc/key_kernels.hip are held to it byte for byte.  All arithmetic is in integers; D, A, G, R, the rows held and C are those of
tests/_key_statement.py, which this file imports and leaves as it is.

For one plugin call on frames [n,h,W,3] that hold the rows [y0, y0 + h) of the picture:
    T_lo    = (T + 1) // 2
    S(f,p)  = A(f,p) >= 9 T                                                                   the strong seeds: the plain key's Z
    Wk(f,p) = A(f,p) >= 9 T_lo                                                                the weak seeds, S <= Wk
    U(f,p)  = the OR of S(g,p) over the frames g != f of the call with |g - f| <= K             one-sided at the ends of the call
    N(f,p)  = U(f) dilated by one pixel of Chebyshev distance, among the pixels of the picture in the rows held
    Z'(f,p) = S(f,p) or (Wk(f,p) and N(f,p))                                                  the held seeds
    e, a, out: tests/_key_statement.py's, with Z' in place of Z

Nothing is carried from one call to another.  `hold_words` is the bit-parallel form the kernel uses, written once on uint64 words, and
tests/test_glyph_hold.py shows it equal."""
import numpy as np

from tests import _key_statement as ks

G, R = ks.G, ks.R
MAX_HOLD = 8


def low(T):
    return (T + 1) // 2


def strong_weak(fill, src, C, T, y0=0):
    """S, Wk: bool [n,h,W]"""
    assert 1 <= T <= ks.MAX_KEY
    A = ks.box_sum(ks.difference(fill, src, C, y0))
    return A >= 9 * T, A >= 9 * low(T)


def neighbours(S, K):
    """U: bool [n,h,W]"""
    n = S.shape[0]
    U = np.zeros_like(S)
    for f in range(n):
        for g in range(max(f - K, 0), min(f + K, n - 1) + 1):
            if g != f:
                U[f] |= S[g]
    return U


def nearby(U):
    """N: U dilated by one pixel to every side, clipped to the array"""
    n, h, W = U.shape
    p = np.zeros((n, h + 2, W + 2), bool)
    p[:, 1:-1, 1:-1] = U
    N = np.zeros_like(U)
    for dy in range(3):
        for dx in range(3):
            N |= p[:, dy:dy + h, dx:dx + W]
    return N


def held(S, Wk, K):
    """Z' from the strong and the weak seeds of a call"""
    assert 0 <= K <= MAX_HOLD
    return S | (Wk & nearby(neighbours(S, K)))


def seeds(fill, src, C, T, K, y0=0):
    """Z': bool [n,h,W]"""
    S, Wk = strong_weak(fill, src, C, T, y0)
    return held(S, Wk, K)


def hold_words(s_words, w_words, K):
    """Z' on the bitmaps (uint64 [n,h,nw], tests/_key_statement.pack_words; no bit at or beyond column W), as the kernel takes it: the
    OR of the neighbouring frames' words, dilated by one bit with carries across the word boundaries, the OR of the rows y - 1 .. y + 1
    (rows beyond the bitmap read as 0)"""
    n, h, nw = s_words.shape
    U = np.zeros_like(s_words)
    for f in range(n):
        for g in range(max(f - K, 0), min(f + K, n - 1) + 1):
            if g != f:
                U[f] |= s_words[g]
    H1 = ks.dilate_words(U, 1)
    V = np.zeros_like(H1)
    for y in range(h):
        V[:, y] = np.bitwise_or.reduce(H1[:, max(y - 1, 0):min(y + 1, h - 1) + 1], axis=1)
    return s_words | (w_words & V)


def hold(fill, src, C, T, K, y0=0, info=None):
    """out: uint8 [n,h,W,3].  info, if a list, receives (S, Wk, Z', a) of the call"""
    assert fill.dtype == np.uint8 and src.dtype == np.uint8 and fill.shape == src.shape
    n, h, W, _ = fill.shape
    S, Wk = strong_weak(fill, src, C, T, y0)
    Z = held(S, Wk, K)
    a = ks.weight(ks.distance(Z))
    if info is not None:
        info.append((S, Wk, Z, a))
    mix = (a[..., None] * fill.astype(np.int64) + (R - a[..., None]) * src.astype(np.int64) + R // 2) // R
    inside = np.asarray(C)[y0:y0 + h] != 0
    return np.where(inside[None, :, :, None], mix, fill).astype(np.uint8)


def workspace_bytes(H, W, n):
    """the documented size of vsr_key_apply_hold's workspace: three bitmaps of vsr_key_apply's size (S, Wk, Z')"""
    return 3 * ks.workspace_bytes(H, W, n)
