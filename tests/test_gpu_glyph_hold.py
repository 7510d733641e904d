"""The glyph-hold kernels through the C-ABI (vsr_key_hold_workspace_bytes, vsr_key_apply_hold; csrc/key_kernels.hip) against the numpy
statement (tests/_hold_statement.py): exact equality of the frames, no tolerance.  Shapes, masks and buffers are those of
tests/test_gpu_glyph_key.py; the clips carry strokes whose contrast changes from frame to frame about T, and the placed cases put a
strong seed of one frame next to weak pixels of another where the kernel can go wrong: either side of a word boundary (columns 63 and
64), either side of a row tile (bitmap rows 31 and 32), the picture's corners, the first and last rows of C, the frames on either side
of the grid's z limit."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _hold_statement as hs
from tests import _key_statement as ks
from tests.test_gpu_glyph_key import SHAPES, P, _buffers, masks, noisy, rows_of

pytestmark = pytest.mark.gpu

T = 12


def hovering(H, W, cmask, seed, n, t=T):
    """noisy(): noise and strokes that are seeds on every frame; on top, six strokes at fixed places (one on the first and one on the
    last row of C) that move by a pixel and change contrast from frame to frame: strong, weak, weak, none, strong; frame 1 not inpainted"""
    rng = np.random.default_rng(seed)
    fill, src = noisy(rng, H, W, n, cmask)
    c0, c1 = rows_of(cmask)
    contrast = [min(2 * t, 255), (6 * t) // 5, (9 * t + 9) // 10, 0, min(3 * t, 255)]
    places = [(c0, int(np.flatnonzero(cmask[c0])[0])), (c1 - 1, int(np.flatnonzero(cmask[c1 - 1])[-1]) - 5)]
    places += [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(4)]
    for f in range(n):
        for j, (y, x) in enumerate(places):
            c = contrast[(f + j) % 5]
            x = max(x + f % 3 - 1, 0)
            src[f, y:y + 2, x:x + 6] = 255
            fill[f, y:y + 2, x:x + 6] = 255 - c
    if n > 2:
        fill[1] = src[1]
    return fill, src


def gpu_hold(lib, dev, fill, src, cmask, t, k, y0=0, **kw):
    H, W = cmask.shape
    n, h = fill.shape[:2]
    lead, src_lead = kw.get("lead", 5), kw.get("src_lead", 3)
    c0, c1 = rows_of(cmask) if cmask.any() else (0, 0)
    cbuf = torch.full((H * W + 128,), 0, dtype=torch.uint8, device=dev)
    cbuf[64:64 + H * W] = torch.from_numpy(np.ascontiguousarray(cmask).ravel()).to(dev)
    cbuf[:64], cbuf[64 + H * W:] = 255, 255                         # a read beyond the mask would find pixels of it
    ft, st, fstride, sstride, fbuf, sbuf = _buffers(dev, fill, src, **kw)
    nbytes = lib.lib.vsr_key_hold_workspace_bytes(H, W, n)
    assert nbytes == hs.workspace_bytes(H, W, n) == 3 * lib.lib.vsr_key_workspace_bytes(H, W, n) and nbytes % 8 == 0
    work = torch.full((nbytes // 8 + 2,), -1, dtype=torch.int64, device=dev)        # garbage: the call writes what it reads
    fp, sp = C.c_void_p(ft.data_ptr() + lead), C.c_void_p(st.data_ptr() + src_lead)
    rc = lib.lib.vsr_key_apply_hold(fp, fstride, sp, sstride, C.c_void_p(cbuf.data_ptr() + 64), n, H, W, y0, h, c0, c1, t, k,
                                    C.c_void_p(work.data_ptr() + 8), None)
    assert rc == 0, lib.last_error()
    torch.cuda.synchronize()
    got = ft.cpu().numpy()
    assert np.array_equal(st.cpu().numpy(), sbuf), "src was written"
    assert int(work[0]) == -1 and int(work[-1]) == -1, "a word in front of or behind the workspace was written"
    size = h * W * 3
    out = np.stack([got[lead + f * fstride:lead + f * fstride + size].reshape(h, W, 3) for f in range(n)])
    untouched = np.ones(got.size, bool)
    for f in range(n):
        untouched[lead + f * fstride:lead + f * fstride + size] = False
    assert np.array_equal(got[untouched], fbuf[untouched]), "bytes in front of, between or behind the frames were written"
    return out


def check(lib, dev, fill, src, cmask, t=T, k=2, y0=0, **kw):
    info = []
    want = hs.hold(fill, src, cmask, t, k, y0=y0, info=info)
    out = gpu_hold(lib, dev, fill, src, cmask, t, k, y0=y0, **kw)
    assert np.array_equal(out, want), f"{int((out != want).sum())} bytes differ from the statement, by up to " \
                                      f"{int(np.abs(out.astype(int) - want).max())}, first at {np.argwhere(out != want)[0].tolist()}"
    return out, info[0]


NK = [(5, 1), (5, 2), (3, 8), (2, 2)]                               # per mask of a shape: frames and K, K >= n among them


@pytest.mark.parametrize("shape", SHAPES)
def test_the_kernels_equal_the_statement(built_lib, gpu_device, shape):
    H, W = shape
    held = 0
    for i, (name, cmask) in enumerate(masks(H, W).items()):
        n, k = NK[i]
        fill, src = hovering(H, W, cmask, seed=H + i, n=n)
        out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, k=k)
        assert not (Z & ~Wk).any() and not (S & ~Z).any(), "S <= Z' <= Wk"
        if n > 2:
            assert np.array_equal(out[1], src[1]) and not Z[1].any(), "the frame with fill == src comes back bit-identical"
        assert np.array_equal(out[:, cmask == 0], fill[:, cmask == 0]), name
        held += int((Z & ~S).sum())
        print(shape, name, "n", n, "K", k, "strong", int(S.sum()), "weak", int(Wk.sum()), "held", int(Z.sum()))
    assert held > 0, "the hold kept seeds the plain key had not"


@pytest.mark.parametrize("n,k", [(1, 1), (1, 8), (18, 8), (18, 1)])
def test_one_frame_and_eighteen(built_lib, gpu_device, n, k):
    H, W = SHAPES[3]                                                # 20 x 65: one bit in a second word
    cmask = masks(H, W)["whole picture"]
    fill, src = hovering(H, W, cmask, seed=n + k, n=n)
    out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, k=k)
    if n == 1:
        assert np.array_equal(Z, S) and np.array_equal(out, ks.key(fill, src, cmask, T)), "one frame has no neighbour: the plain key"
    else:
        assert (Z & ~S).any()


@pytest.mark.parametrize("t", [2, 12, 128])
def test_thresholds(built_lib, gpu_device, t):
    H, W = SHAPES[0]
    cmask = masks(H, W)["two boxes"]
    fill, src = hovering(H, W, cmask, seed=t, n=5, t=t)
    out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, t=t, k=2)
    assert S.any() and (Wk & ~S).any()
    assert (Z & ~S).any() or t == 2, "at T = 2 the noise is a strong seed wherever the fill was written"


def placed(H, W, n, spots, t=T):
    """a black clip under the whole picture as mask; spots: (frame, y, x, 'S' | 'W' | 'w') puts one pixel off by 9 T (a strong seed on
    the 3 x 3 pixels around it), by 9 T_lo (a weak one) or by 9 T_lo - 1 (none)"""
    src = np.zeros((n, H, W, 3), np.uint8)
    fill = src.copy()
    level = {"S": 9 * t, "W": 9 * hs.low(t), "w": 9 * hs.low(t) - 1}
    for f, y, x, kind in spots:
        assert level[kind] <= 255
        fill[f, y, x, (y + x) % 3] = level[kind]
    return fill, src, np.full((H, W), 255, np.uint8)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] > 64])
def test_either_side_of_a_word_boundary(built_lib, gpu_device, shape):
    """a strong seed whose last column is 63 against weak pixels from column 64 on, and mirrored, on the first, a middle and the last row"""
    H, W = shape
    right = min(65, W - 1)                                          # centre of the pixel placed right of the boundary (20 x 65: on it)
    for y in (0, H // 2, H - 1):
        fill, src, cmask = placed(H, W, 2, [(0, y, 62, "S"), (1, y, right, "W"), (1, y, 10, "W")])
        out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, k=1)
        assert S[0, y, 63] and not S[0, y, 64] and Wk[1, y, 64] and not S[1].any()
        assert Z[1, y, 64], "column 64 of frame 1 is one pixel off column 63 of frame 0"
        assert (not Z[1, y, 65] if W > 65 else True) and not Z[1, y, 10] and (out[1] != src[1]).any()
        # mirrored: strong from column 64 on in frame 0, weak up to column 63 in frame 1
        fill, src, cmask = placed(H, W, 2, [(0, y, right, "S"), (1, y, 62, "W")])
        out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, k=1)
        assert S[0, y, 64] and Wk[1, y, 61:64].all() and not Wk[1, y, 64] and Z[1, y, 63]
        if right == 65:
            assert not S[0, y, 63] and not Z[1, y, 62], "column 63 is held, column 62 is two pixels off column 64"


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] >= 34])
def test_either_side_of_a_row_tile(built_lib, gpu_device, shape):
    """the whole picture as mask: bitmap row = picture row.  A strong seed whose last row is 31 against weak pixels from row 32 on, and
    mirrored"""
    H, W = shape
    x = min(63, W - 2)
    fill, src, cmask = placed(H, W, 2, [(0, 30, x, "S"), (1, 33, x, "W")])
    out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, k=1)
    assert S[0, 31, x] and not S[0, 32, x] and Wk[1, 32, x] and not Wk[1, 31, x]
    assert Z[1, 32, x - 1:x + 2].all() and not Z[1, 33].any()
    fill, src, cmask = placed(H, W, 2, [(1, 33, x, "S"), (0, 30, x, "W")])
    out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, k=1)
    assert S[1, 32, x] and not S[1, 31, x]
    assert Z[0, 31, x - 1:x + 2].all() and not Z[0, 30].any()


@pytest.mark.parametrize("shape", SHAPES)
def test_the_four_corners(built_lib, gpu_device, shape):
    """a strong seed in a corner of one frame against a weak pixel two pixels in on the next; the top corners on frames 0 and 1, the
    bottom ones on 2 and 3 (on seven rows their weak pixels would add up to a strong one)"""
    H, W = shape
    corners = [(0, 0, 0, 2, 2), (0, 0, W - 1, 2, W - 3), (2, H - 1, 0, H - 3, 2), (2, H - 1, W - 1, H - 3, W - 3)]
    spots = [(f, y, x, "S") for f, y, x, _, _ in corners] + [(f + 1, y, x, "W") for f, _, _, y, x in corners]
    fill, src, cmask = placed(H, W, 4, spots)
    out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, k=1)
    for (f, y, x, wy, wx) in corners:
        assert S[f, y, x] and Z[f, y, x]
        iy, ix = (y + wy) // 2, (x + wx) // 2                       # the pixel the strong and the weak square share
        assert Z[f + 1, iy, ix] and Z[f + 1, wy, wx] and not Z[f + 1, 2 * wy - iy, 2 * wx - ix], (y, x)
    assert not S[1].any() and not S[3].any() and (out[1] != src[1]).any() and (out[3] != src[3]).any()


def test_a_lone_pixel_under_the_weak_threshold(built_lib, gpu_device):
    """A = 9 T_lo - 1 next to a neighbour frame's strong seed is not held: the frame comes back as its source; A = 9 T_lo is"""
    H, W = SHAPES[0]
    for t in (3, 12, 28):
        fill, src, cmask = placed(H, W, 2, [(0, 20, 62, "S"), (1, 20, 64, "w")], t=t)
        out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, t=t, k=1)
        assert S[0].sum() == 9 and not Wk[1].any() and np.array_equal(out[1], src[1])
        fill, src, cmask = placed(H, W, 2, [(0, 20, 62, "S"), (1, 20, 64, "W")], t=t)
        out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, t=t, k=1)
        assert Wk[1].sum() == 9 and Z[1].sum() == 6 and out[1, 20, 64].max() == 9 * hs.low(t)


def test_three_frames_the_middle_one_unchanged(built_lib, gpu_device):
    H, W = SHAPES[1]
    cmask = masks(H, W)["bottom box"]
    fill, src = hovering(H, W, cmask, seed=77, n=3)
    out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, k=2)
    assert np.array_equal(out[1], src[1]) and S[0].any() and S[2].any() and not Wk[1].any()
    assert (Z & ~S).any(), "frames 0 and 2 hold each other's weak pixels across the unchanged one"


def test_more_frames_than_the_grid_has_planes(built_lib, gpu_device):
    """n = 1030 at 9 x 8: the frames from 1024 on are a workgroup's second round, and their windows reach back across the stride"""
    H, W = SHAPES[5]
    n = 1030
    spots = [(f, 4, 3, "S" if f % 7 == 0 else "W") for f in range(n) if f % 7 == 0 or f % 3]
    fill, src, cmask = placed(H, W, n, spots)
    out, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, k=2)
    assert S[1022].any() and not S[1023:1029].any() and not Z[1023].any() and Z[1024].any() and not Z[1025].any()
    assert S[1029].any() and Z[1027].any() and Z[1028].any() and not Z[1026].any() and Z[5].any() and not Z[4].any()


@pytest.mark.parametrize("lead,src_lead", [(0, 0), (1, 16), (15, 15)])
def test_every_alignment(built_lib, gpu_device, lead, src_lead):
    H, W = SHAPES[0]
    cmask = masks(H, W)["two boxes"]
    fill, src = hovering(H, W, cmask, seed=21, n=5)
    check(built_lib, gpu_device, fill, src, cmask, k=2, lead=lead, src_lead=src_lead, gap=lead % 5, src_gap=0 if lead else 29)


def test_strip_rows(built_lib, gpu_device):
    """y0 = 5, h = 33 of H = 45: with the mask inside the rows they come back as the rows of the full-frame result; with a box in front
    of the rows and one they cut, as the statement's for the rows"""
    H, W = SHAPES[0]
    y0, h = 5, 33
    cmask = np.zeros((H, W), np.uint8)
    cmask[14:30, 6:W - 11] = 255
    cmask[5:8, W // 3:W // 2] = 255
    fill, src = hovering(H, W, cmask, seed=H, n=5)
    whole, (S, Wk, Z, a) = check(built_lib, gpu_device, fill, src, cmask, k=2)
    assert (Z & ~S).any()
    rows, _ = check(built_lib, gpu_device, fill[:, y0:y0 + h], src[:, y0:y0 + h], cmask, k=2, y0=y0)
    assert np.array_equal(rows, whole[:, y0:y0 + h])
    cmask[1:4, 3:40] = 255                                          # c0 < y0
    cmask[36:44, 20:70] = 9                                         # c1 > y0 + h
    fill, src = hovering(H, W, cmask, seed=H + 1, n=5)
    rows, (S, Wk, Z, a) = check(built_lib, gpu_device, fill[:, y0:y0 + h], src[:, y0:y0 + h], cmask, k=2, y0=y0)
    assert Z.shape[1] == h and (Z & ~S).any()


def test_nothing_to_do_is_success(built_lib, gpu_device):
    t = torch.full((64,), 3, dtype=torch.int64, device=gpu_device)
    lib = built_lib.lib
    assert lib.vsr_key_hold_workspace_bytes(3, 3, 0) == 0 and lib.vsr_key_hold_workspace_bytes(1080, 1920, 50) == 3 * 50 * 1080 * 30 * 8
    assert lib.vsr_key_apply_hold(P(t), 27, P(t), 27, P(t), 0, 3, 3, 0, 3, 0, 3, T, 2, P(t), None) == 0, "n = 0"
    assert lib.vsr_key_apply_hold(P(t), 27, P(t), 27, P(t), 2, 3, 3, 0, 3, 2, 2, T, 2, P(t), None) == 0, "c0 == c1"
    assert lib.vsr_key_apply_hold(P(t), 27, P(t), 27, P(t), 2, 9, 3, 0, 3, 5, 8, T, 2, P(t), None) == 0, "the rows held lie beside C's"
    torch.cuda.synchronize()
    assert (t == 3).all()


def test_argument_errors(built_lib, gpu_device):
    lib = built_lib.lib
    frames = torch.full((4096,), 9, dtype=torch.uint8, device=gpu_device)
    src = torch.full((4096,), 7, dtype=torch.uint8, device=gpu_device)
    cm = torch.full((4096,), 4, dtype=torch.uint8, device=gpu_device)
    words = torch.full((4096,), 5, dtype=torch.int64, device=gpu_device)
    size = 8 * 8 * 3
    ok = dict(frames=P(frames), fs=size, src=P(src), ss=size, cm=P(cm), n=2, H=8, W=8, y0=0, rows=8, c0=2, c1=6, T=T, K=2, work=P(words))

    def apply(**kw):
        a = dict(ok, **kw)
        return lib.vsr_key_apply_hold(a["frames"], a["fs"], a["src"], a["ss"], a["cm"], a["n"], a["H"], a["W"], a["y0"], a["rows"], a["c0"],
                                      a["c1"], a["T"], a["K"], a["work"], None)

    bad = [dict(frames=None), dict(src=None), dict(cm=None), dict(work=None), dict(H=0), dict(W=-1), dict(n=-1), dict(fs=size - 1),
           dict(ss=size - 1), dict(y0=-1), dict(y0=1), dict(rows=0), dict(rows=-3), dict(rows=9), dict(c0=-1), dict(c0=7, c1=6), dict(c1=9),
           dict(H=32768, W=32768, rows=1), dict(T=0), dict(T=-1), dict(T=129), dict(work=C.c_void_p(words.data_ptr() + 4)),
           dict(K=0), dict(K=-1), dict(K=9)]
    for kw in bad:
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "glyph key" in built_lib.last_error(), kw
    for args in ((0, 8, 1), (8, -1, 1), (8, 8, -1), (32768, 32768, 1)):
        assert lib.vsr_key_hold_workspace_bytes(*args) == built_lib.VSR_ERR_ARG, args
        assert "glyph key" in built_lib.last_error(), args
    torch.cuda.synchronize()
    assert (frames == 9).all() and (src == 7).all() and (cm == 4).all() and (words == 5).all(), "a refused call wrote something"
