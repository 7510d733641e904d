"""The definition of --glyph-key T in plain numpy: the kernels of csrc/key_kernels.hip are held to it byte for byte.
All arithmetic is in integers.

For one plugin call on frames [n,h,W,3] that hold the rows [y0, y0 + h) of the picture:
    src   the frames as they came in          fill  the frames as they stand when the pass runs
    C     the composite mask of the whole picture, uint8 [H,W]

    D(f,p) = max over the channels of |src - fill|   where C[p] != 0 and p lies in the rows held, 0 elsewhere
    A(f,p) = the sum of D(f,q) over the 3 x 3 neighbourhood of p (outside the picture or the rows held: 0)        A <= 2295
    Z(f,p) = A(f,p) >= 9 T                                                                                          the seeds
    e(f,p) = min(G + R, Chebyshev distance from p to the nearest seed of frame f in the rows held)
    a      = clamp(G + R - e, 0, R)
    out    = (a * fill + (R - a) * src + R // 2) // R    on the pixels of C in the rows held; every other byte is the fill's

Nothing is carried from one frame to another.  The box sum is taken by padded slices, the distance by brute-force square dilation;
`distance_words` is the bit-parallel form the kernel uses, written once on uint64 words, and tests/test_glyph_key.py shows it equal."""
import numpy as np

G, R = 4, 4                 # grow: full fill within G pixels of a seed; ramp: back to the source over the next R
MAX_KEY = 128
A_MAX = 9 * 255


def difference(fill, src, C, y0=0):
    """D: int64 [n,h,W]"""
    n, h, W, _ = fill.shape
    inside = np.asarray(C)[y0:y0 + h] != 0
    d = np.abs(src.astype(np.int64) - fill.astype(np.int64)).max(axis=3)
    return np.where(inside[None], d, 0)


def box_sum(D):
    """A: the 3 x 3 sum of D [n,h,W], zeros beyond its edges"""
    n, h, W = D.shape
    p = np.zeros((n, h + 2, W + 2), np.int64)
    p[:, 1:-1, 1:-1] = D
    return sum(p[:, dy:dy + h, dx:dx + W] for dy in range(3) for dx in range(3))


def seeds(fill, src, C, T, y0=0):
    """Z: bool [n,h,W]"""
    assert 1 <= T <= MAX_KEY
    return box_sum(difference(fill, src, C, y0)) >= 9 * T


def distance(Z):
    """e: int64 [n,h,W], by brute force: e <= k iff the (2k+1)^2 square around p, clipped to the array, holds a seed"""
    n, h, W = Z.shape
    e = np.full(Z.shape, G + R, np.int64)
    pad = G + R
    p = np.zeros((n, h + 2 * pad, W + 2 * pad), bool)
    p[:, pad:pad + h, pad:pad + W] = Z
    for k in range(G + R - 1, -1, -1):
        hit = np.zeros(Z.shape, bool)
        for dy in range(-k, k + 1):
            for dx in range(-k, k + 1):
                hit |= p[:, pad + dy:pad + dy + h, pad + dx:pad + dx + W]
        e[hit] = k
    return e


def pack_words(Z):
    """bool [n,h,W] -> uint64 [n,h,ceil(W / 64)]: bit i of word w is column 64 w + i"""
    n, h, W = Z.shape
    nw = -(-W // 64)
    bits = np.zeros((n, h, nw * 64), np.uint64)
    bits[:, :, :W] = Z
    shifts = np.arange(64, dtype=np.uint64)
    return (bits.reshape(n, h, nw, 64) << shifts).sum(axis=3, dtype=np.uint64)


def unpack_words(words, W):
    n, h, nw = words.shape
    shifts = np.arange(64, dtype=np.uint64)
    bits = (words[..., None] >> shifts) & np.uint64(1)
    return bits.reshape(n, h, nw * 64)[:, :, :W].astype(bool)


def dilate_words(words, k):
    """H_k: every row's words dilated by k bits to either side, with carries across the word boundaries"""
    out = words.copy()
    zero = np.zeros_like(words[..., :1])
    left = np.concatenate([zero, words[..., :-1]], axis=-1)       # the word of the 64 columns before
    right = np.concatenate([words[..., 1:], zero], axis=-1)       # the word of the 64 columns after
    for j in range(1, k + 1):
        s, t = np.uint64(j), np.uint64(64 - j)
        out |= (words << s) | (left >> t) | (words >> s) | (right << t)
    return out


def distance_words(words, W):
    """e from the seed bitmap, bit-parallel: e <= k iff the OR of H_k over the rows y - k .. y + k (clipped) has the bit"""
    n, h, nw = words.shape
    e = np.full((n, h, W), G + R, np.int64)
    for k in range(G + R - 1, -1, -1):
        Hk = dilate_words(words, k)
        V = np.zeros_like(Hk)
        for y in range(h):
            V[:, y] = np.bitwise_or.reduce(Hk[:, max(y - k, 0):min(y + k, h - 1) + 1], axis=1)
        e[unpack_words(V, W)] = k
    return e


def weight(e):
    return np.clip(G + R - e, 0, R)


def key(fill, src, C, T, y0=0, info=None):
    """out: uint8 [n,h,W,3].  info, if a list, receives (Z, a) of the call"""
    assert fill.dtype == np.uint8 and src.dtype == np.uint8 and fill.shape == src.shape
    n, h, W, _ = fill.shape
    Z = seeds(fill, src, C, T, y0)
    a = weight(distance(Z))
    if info is not None:
        info.append((Z, a))
    mix = (a[..., None] * fill.astype(np.int64) + (R - a[..., None]) * src.astype(np.int64) + R // 2) // R
    inside = np.asarray(C)[y0:y0 + h] != 0
    return np.where(inside[None, :, :, None], mix, fill).astype(np.uint8)


def workspace_bytes(H, W, n):
    """the documented size of vsr_key_apply's workspace: a seed bitmap of 64-bit words, a row per picture row"""
    return n * H * -(-W // 64) * 8
