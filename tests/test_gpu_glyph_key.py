"""The glyph-key kernels through the C-ABI (vsr_key_workspace_bytes, vsr_key_apply; csrc/key_kernels.hip) against the numpy statement
(tests/_key_statement.py): exact equality of the frames, no tolerance; unaligned and strided frames, guard bytes, a workspace of
garbage, the strip-row form, uninpainted frames, argument errors.  The shapes are the smallest at which the kernels can go wrong:
45 x 75 (one full word and 11 bits), 130 x 260 (five words, a partial last one, five row tiles), 20 x 64 and 20 x 65 (exactly one word,
and one bit in a second), 7 x 130 (fewer rows than G + R: the vertical window is clipped on both sides), 9 x 8 (one partial word)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _key_statement as ks

pytestmark = pytest.mark.gpu

SHAPES = [(45, 75), (130, 260), (20, 64), (20, 65), (7, 130), (9, 8)]
T = 12


def P(t):
    return C.c_void_p(t.data_ptr())


def masks(H, W):
    out = {"whole picture": np.full((H, W), 255, np.uint8)}         # touches every border: the corners are pixels of C
    bottom = np.zeros((H, W), np.uint8)
    bottom[H - max(H // 4, 2):, W // 6:W - W // 5] = 255            # touches the bottom border
    out["bottom box"] = bottom
    two = np.zeros((H, W), np.uint8)
    two[1:3, 1:W // 2] = 255
    two[H // 2:H - 1, W // 2 + 1:W - 1] = 7                         # any non-zero value is inside
    out["two boxes"] = two
    one = np.zeros((H, W), np.uint8)
    one[H // 2 + 1, min(W // 3, W - 1)] = 255
    out["one pixel"] = one
    return out


def rows_of(cmask):
    held = np.flatnonzero(cmask.any(axis=1))
    return int(held[0]), int(held[-1]) + 1


def noisy(rng, H, W, n, cmask):
    """src: a plane with noise of sigma 2; fill: another draw of the noise inside the mask, src outside it, and strokes 100 levels off"""
    y, x = np.mgrid[0:H, 0:W]
    base = (70 + 0.4 * x + 0.6 * y)[None, :, :, None] + np.zeros((n, 1, 1, 3))
    src = np.clip(np.rint(base + rng.normal(0, 2, base.shape)), 0, 255).astype(np.uint8)
    fill = src.copy()
    inside = cmask != 0
    other = np.clip(np.rint(base + rng.normal(0, 2, base.shape)), 0, 255).astype(np.uint8)
    fill[:, inside] = other[:, inside]
    for f in range(n):
        for _ in range(3):
            yy, xx = int(rng.integers(0, H)), int(rng.integers(0, W))
            fill[f, yy:yy + 1 + f % 2, xx:xx + 6] = np.clip(src[f, yy:yy + 1 + f % 2, xx:xx + 6].astype(int) - 100, 0, 255)   # (inside C or not)
    return fill, src


def spots_a(H, W, c0, c1, cmask):
    """the corners of the picture, column 63, the first row of C"""
    ys, xs = np.nonzero(cmask[c0:c0 + 1])
    out = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (c0, int(xs[len(xs) // 2]))]
    if W > 63:
        out.append((H // 2, 63))
    return out


def spots_b(H, W, c0, c1, cmask):
    """column 64, the last row of C, and a pixel of C at its left edge, whose difference makes the pixel outside C a seed"""
    xs = np.flatnonzero(cmask[c1 - 1])
    out = [(c1 - 1, int(xs[len(xs) // 2]))]
    if W > 64:
        out.append((H // 2 - 1, 64))
    ys, xe = np.nonzero(cmask)
    out.append((int(ys[0]), int(xe[0])))
    return out


def exact(rng, src, spots, delta=200):
    """fill: src with at most one level of difference per byte, everywhere, and `delta` at the spots (the source white or black there)"""
    fill = np.clip(src.astype(int) + rng.integers(-1, 2, src.shape), 0, 255).astype(np.uint8)
    src = src.copy()
    for i, (y, x) in enumerate(spots):
        src[y, x] = 255 if i % 2 else 0
        fill[y, x] = 255 - delta if i % 2 else delta
    return fill, src


def clip(H, W, cmask, seed, n=5):
    """n = 5: 0 noisy, 1 not inpainted, 2 the spots of spots_a, 3 the spots of spots_b, 4 noisy"""
    rng = np.random.default_rng(seed)
    fill, src = noisy(rng, H, W, n, cmask)
    c0, c1 = rows_of(cmask)
    if n > 1:
        fill[1] = src[1]
    if n > 3:
        fill[2], src[2] = exact(rng, src[2], spots_a(H, W, c0, c1, cmask))
        fill[3], src[3] = exact(rng, src[3], spots_b(H, W, c0, c1, cmask))
    return fill, src


def _buffers(dev, fill, src, lead=5, gap=7, src_lead=3, src_gap=13):
    """frames: a slice of a larger tensor (odd start `lead`, stride = frame + gap); src: another stride and start"""
    n, size = fill.shape[0], fill[0].size
    fstride, sstride = size + gap, size + src_gap
    fbuf = np.full(lead + n * fstride + 32, 0x5A, np.uint8)
    sbuf = np.full(src_lead + n * sstride + 32, 0xC3, np.uint8)
    for f in range(n):
        fbuf[lead + f * fstride:lead + f * fstride + size] = fill[f].ravel()
        sbuf[src_lead + f * sstride:src_lead + f * sstride + size] = src[f].ravel()
    return torch.from_numpy(fbuf).to(dev), torch.from_numpy(sbuf).to(dev), fstride, sstride, fbuf, sbuf


def gpu_key(lib, dev, fill, src, cmask, t, y0=0, **kw):
    H, W = cmask.shape
    n, h = fill.shape[:2]
    lead, src_lead = kw.get("lead", 5), kw.get("src_lead", 3)
    c0, c1 = rows_of(cmask) if cmask.any() else (0, 0)
    cbuf = torch.full((H * W + 128,), 0, dtype=torch.uint8, device=dev)
    cbuf[64:64 + H * W] = torch.from_numpy(np.ascontiguousarray(cmask).ravel()).to(dev)
    cbuf[:64], cbuf[64 + H * W:] = 255, 255                         # a read beyond the mask would find pixels of it
    ft, st, fstride, sstride, fbuf, sbuf = _buffers(dev, fill, src, **kw)
    nbytes = lib.lib.vsr_key_workspace_bytes(H, W, n)
    assert nbytes == ks.workspace_bytes(H, W, n) and nbytes % 8 == 0
    work = torch.full((nbytes // 8 + 2,), -1, dtype=torch.int64, device=dev)        # garbage: the call writes what it reads
    fp, sp = C.c_void_p(ft.data_ptr() + lead), C.c_void_p(st.data_ptr() + src_lead)
    rc = lib.lib.vsr_key_apply(fp, fstride, sp, sstride, C.c_void_p(cbuf.data_ptr() + 64), n, H, W, y0, h, c0, c1, t,
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


def check(lib, dev, fill, src, cmask, t=T, y0=0, **kw):
    info = []
    want = ks.key(fill, src, cmask, t, y0=y0, info=info)
    out = gpu_key(lib, dev, fill, src, cmask, t, y0=y0, **kw)
    assert np.array_equal(out, want), f"{int((out != want).sum())} bytes differ from the statement, by up to " \
                                      f"{int(np.abs(out.astype(int) - want).max())}, first at {np.argwhere(out != want)[0].tolist()}"
    return out, info[0]


@pytest.mark.parametrize("shape", SHAPES)
def test_the_kernels_equal_the_statement(built_lib, gpu_device, shape):
    H, W = shape
    for k, (name, cmask) in enumerate(masks(H, W).items()):
        fill, src = clip(H, W, cmask, seed=H + k)
        out, (Z, a) = check(built_lib, gpu_device, fill, src, cmask)
        inside = cmask != 0
        c0, c1 = rows_of(cmask)
        assert np.array_equal(out[1], src[1]) and not Z[1].any(), "the frame with fill == src comes back bit-identical"
        assert np.array_equal(out[:, ~inside], fill[:, ~inside]), name
        # the spots: a seed at every one that is a pixel of C, and the fill there
        for f, spots in ((2, spots_a(H, W, c0, c1, cmask)), (3, spots_b(H, W, c0, c1, cmask))):
            for y, x in spots:
                if inside[y, x]:
                    assert Z[f, y, x] and a[f, y, x] == ks.R and np.array_equal(out[f, y, x], fill[f, y, x]), (name, f, y, x)
            at = np.zeros((1, H, W), bool)
            at[0][tuple(np.array(spots).T)] = True
            assert not Z[f][ks.distance(at)[0] > 1].any(), "no seed but around the spots"
        if name == "whole picture":
            assert Z[2, 0, 0] and Z[2, 0, W - 1] and Z[2, H - 1, 0] and Z[2, H - 1, W - 1], "the four corners"
            if W > 64:
                assert Z[2, H // 2, 63] and Z[3, H // 2 - 1, 64] and not Z[3, H // 2 - 1, 62], "either side of the word boundary"
            if W > 65:
                assert not Z[2, H // 2, 65]
        if name in ("bottom box", "two boxes"):
            y, x = spots_b(H, W, c0, c1, cmask)[-1]                 # the first pixel of C: its left neighbour lies outside C
            assert x > 0 and not inside[y, x - 1] and Z[3, y, x - 1], "a seed outside C, from its neighbour's difference"
        assert Z[2, c0].any() and Z[3, c1 - 1].any(), "seeds on the first and the last row of C"


def test_a_lone_pixel_under_the_threshold(built_lib, gpu_device):
    """A = 9 T - 1 in the pixel's 3 x 3 neighbourhood is no seed: the frame comes back as its source; A = 9 T is one"""
    H, W = SHAPES[0]
    cmask = masks(H, W)["whole picture"]
    src = np.zeros((2, H, W, 3), np.uint8)
    for t in (1, 12, 28):
        fill = src.copy()
        fill[0, 20, 63, 2] += 9 * t - 1
        fill[1, 20, 64, 0] += 9 * t
        out, (Z, a) = check(built_lib, gpu_device, fill, src, cmask, t=t)
        assert not Z[0].any() and np.array_equal(out[0], src[0]) and Z[1].sum() == 9 and out[1, 20, 64, 0] == 9 * t


@pytest.mark.parametrize("t", [1, 12, 128])
def test_thresholds(built_lib, gpu_device, t):
    H, W = SHAPES[0]
    cmask = masks(H, W)["two boxes"]
    fill, src = clip(H, W, cmask, seed=t)
    src[0, 24:29, 40:45], fill[0, 24:29, 40:45] = 255, 0           # a block that is a seed at every T
    out, (Z, a) = check(built_lib, gpu_device, fill, src, cmask, t=t)
    assert Z[0].any() and not Z[0].all() and (out[0] != src[0]).any()
    assert (out[0] != fill[0]).any() or t == 1, "at T = 1 the noise is a seed wherever the fill was written"


def test_bytes_at_the_ends_of_the_range(built_lib, gpu_device):
    """src and fill 127 levels apart with a byte at 0 or 255 in every channel (no seed at T = 128), around a block 255 apart: the ramp
    mixes the extreme bytes at every weight"""
    H, W = SHAPES[0]
    cmask = masks(H, W)["whole picture"]
    src = np.empty((2, H, W, 3), np.uint8)
    fill = np.empty_like(src)
    src[:], fill[:] = (255, 0, 128), (128, 127, 255)
    src[0, 20:25, 60:66], fill[0, 20:25, 60:66] = (255, 0, 0), (0, 255, 255)
    out, (Z, a) = check(built_lib, gpu_device, fill, src, cmask, t=128)
    assert sorted(np.unique(a[0]).tolist()) == [0, 1, 2, 3, 4] and not Z[1].any() and np.array_equal(out[1], src[1])
    assert out[0, 22, 49:56, 0].tolist() == [255, 255, 255, 223, 192, 160, 128]


@pytest.mark.parametrize("lead,src_lead", [(0, 0), (1, 16), (15, 15)])
def test_every_alignment(built_lib, gpu_device, lead, src_lead):
    H, W = SHAPES[0]
    cmask = masks(H, W)["two boxes"]
    fill, src = clip(H, W, cmask, seed=21)
    check(built_lib, gpu_device, fill, src, cmask, lead=lead, src_lead=src_lead, gap=lead % 5, src_gap=0 if lead else 29)


def test_strip_rows(built_lib, gpu_device):
    """y0 = 5, h = 33 of H = 45: a box inside the rows, one that touches their first row, one in front of them and one they cut.  The
    rows come back as the statement's for the rows; with the mask inside the rows, as the rows of the full-frame result"""
    H, W = SHAPES[0]
    y0, h = 5, 33
    cmask = np.zeros((H, W), np.uint8)
    cmask[14:30, 6:W - 11] = 255
    cmask[5:8, W // 3:W // 2] = 255
    fill, src = clip(H, W, cmask, seed=H)
    whole, _ = check(built_lib, gpu_device, fill, src, cmask)
    rows, _ = check(built_lib, gpu_device, fill[:, y0:y0 + h], src[:, y0:y0 + h], cmask, y0=y0)
    assert np.array_equal(rows, whole[:, y0:y0 + h])
    cmask[1:4, 3:40] = 255                                          # c0 < y0
    cmask[36:44, 20:70] = 9                                         # c1 > y0 + h
    fill, src = clip(H, W, cmask, seed=H + 1)
    rows, (Z, a) = check(built_lib, gpu_device, fill[:, y0:y0 + h], src[:, y0:y0 + h], cmask, y0=y0)
    assert Z.shape[1] == h and Z.any()


def test_three_frames_the_middle_one_unchanged(built_lib, gpu_device):
    H, W = SHAPES[1]
    cmask = masks(H, W)["bottom box"]
    fill, src = clip(H, W, cmask, seed=77, n=3)
    fill[0, 110, 100:106] = src[0, 110, 100:106] // 4                   # strokes inside the box, one on the picture's last row
    fill[2, H - 1, 60:70] = src[2, H - 1, 60:70] // 4
    out, (Z, a) = check(built_lib, gpu_device, fill, src, cmask)
    assert np.array_equal(out[1], src[1]) and Z[0].any() and Z[2].any() and not Z[1].any()


def test_nothing_to_do_is_success(built_lib, gpu_device):
    t = torch.full((64,), 3, dtype=torch.int64, device=gpu_device)
    lib = built_lib.lib
    assert lib.vsr_key_workspace_bytes(3, 3, 0) == 0 and lib.vsr_key_workspace_bytes(1080, 1920, 50) == 50 * 1080 * 30 * 8
    assert lib.vsr_key_apply(P(t), 27, P(t), 27, P(t), 0, 3, 3, 0, 3, 0, 3, T, P(t), None) == 0, "n = 0"
    assert lib.vsr_key_apply(P(t), 27, P(t), 27, P(t), 2, 3, 3, 0, 3, 2, 2, T, P(t), None) == 0, "c0 == c1"
    # the rows held lie beside the rows of C: nothing is launched
    assert lib.vsr_key_apply(P(t), 27, P(t), 27, P(t), 2, 9, 3, 0, 3, 5, 8, T, P(t), None) == 0
    torch.cuda.synchronize()
    assert (t == 3).all()


def test_argument_errors(built_lib, gpu_device):
    lib = built_lib.lib
    frames = torch.full((4096,), 9, dtype=torch.uint8, device=gpu_device)
    src = torch.full((4096,), 7, dtype=torch.uint8, device=gpu_device)
    cm = torch.full((4096,), 4, dtype=torch.uint8, device=gpu_device)
    words = torch.full((4096,), 5, dtype=torch.int64, device=gpu_device)
    size = 8 * 8 * 3
    ok = dict(frames=P(frames), fs=size, src=P(src), ss=size, cm=P(cm), n=2, H=8, W=8, y0=0, rows=8, c0=2, c1=6, T=T, work=P(words))

    def apply(**kw):
        a = dict(ok, **kw)
        return lib.vsr_key_apply(a["frames"], a["fs"], a["src"], a["ss"], a["cm"], a["n"], a["H"], a["W"], a["y0"], a["rows"], a["c0"],
                                 a["c1"], a["T"], a["work"], None)

    bad = [dict(frames=None), dict(src=None), dict(cm=None), dict(work=None), dict(H=0), dict(W=-1), dict(n=-1), dict(fs=size - 1),
           dict(ss=size - 1), dict(y0=-1), dict(y0=1), dict(rows=0), dict(rows=-3), dict(rows=9), dict(c0=-1), dict(c0=7, c1=6), dict(c1=9),
           dict(H=32768, W=32768, rows=1), dict(T=0), dict(T=-1), dict(T=129), dict(work=C.c_void_p(words.data_ptr() + 4))]
    for kw in bad:
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "glyph key" in built_lib.last_error(), kw
    for args in ((0, 8, 1), (8, -1, 1), (8, 8, -1), (32768, 32768, 1)):
        assert lib.vsr_key_workspace_bytes(*args) == built_lib.VSR_ERR_ARG, args
        assert "glyph key" in built_lib.last_error(), args
    torch.cuda.synchronize()
    assert (frames == 9).all() and (src == 7).all() and (cm == 4).all() and (words == 5).all(), "a refused call wrote something"
