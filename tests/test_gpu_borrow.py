"""The borrow kernels through the C-ABI (vsr_borrow_workspace_bytes, vsr_borrow_apply; csrc/borrow_kernels.hip) against the numpy
statement (tests/_borrow_statement.py): exact equality of the frames, no tolerance; unaligned and strided frames, guard bytes, a
workspace of garbage, the strip-row form, a cut, a half-open pair, an uninpainted frame, argument errors.  The shapes are the key's
(tests/test_gpu_glyph_key.py): 45 x 75 (one full word and 11 bits), 130 x 260 (five words, five row tiles), 20 x 64 and 20 x 65 (exactly
one word, and one bit in a second), 7 x 130 (fewer rows than G + R: the vertical window is clipped on both sides).

The clips: a dark plane with grain of sigma 2 that stands still; the fill is the plane with another draw of the grain inside the mask;
the source carries white glyph blocks that change place every `period` frames, among them blocks whose reach N ends at column 63 and
at column 64 from either side, blocks in the picture's corners and on the first and last row of C.  Every case asserts from the
statement's info that it is not vacuous, as far as its mask allows: the whole-picture mask has no ring (m = 0), so every pair is closed
and the frames must come back as the fill; a mask of fewer than 50 pixels (one pixel) cannot show every kind of event at once and
must show that a borrower was judged.  Every other case shows all five: a pixel taken at distance 1, one from farther away, a lender
passed over for its own glyph, one passed over by the threshold, a borrower left with its fill.  Glyph blocks that touch no pixel of C
are left out: they make no seed and would only move the ring."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _borrow_statement as bs
from tests import _key_statement as ks
from tests.test_gpu_glyph_key import masks, rows_of

pytestmark = pytest.mark.gpu

SHAPES = [(45, 75), (20, 64), (20, 65), (7, 130), (130, 260)]
T = 12


def P(t):
    return C.c_void_p(t.data_ptr())


def spots(H, W, cmask, group):
    """the upper left corners of the glyph blocks (2 rows x 4 columns, clipped) of the frames of `group`"""
    c0, c1 = rows_of(cmask)
    mid = H // 2
    ys, xs = np.nonzero(cmask)
    if group == 0:
        out = [(0, 0), (H - 2, W - 4), (c0, int(np.flatnonzero(cmask[c0])[0])), (int(ys[0]), int(xs[0]))]
        out += [(mid, 52)] + ([(mid - 20, 72)] if H >= 40 else [])      # N ends at column 63 on the right, starts at column 64 on the left
    else:
        out = [(0, W - 4), (H - 2, 0)]
        if len(ys) >= 50:                                    # (a mask of a few pixels stays free of glyphs on these frames: it has lenders)
            out += [(c1 - 2, int(np.flatnonzero(cmask[c1 - 1])[-1]) - 3), (int(ys[-1]) - 1, int(xs[-1]) - 3)]
        out += [(mid, 53)] + ([(mid - 20, 71)] if H >= 40 else [])      # N ends at column 64, starts at column 63
    out = [(max(y, 0), max(x, 0)) for y, x in out if x < W]
    return [(y, x) for y, x in out if cmask[y:y + 2, x:x + 4].any()]       # (a block beside C makes no seed; it would only move the ring)


def clip(H, W, cmask, n, seed, period=3, exact=False, cut=None, dim=None, plain=None, far=None):
    """src, fill uint8 [n,H,W,3].  exact: the fill is the source away from the glyphs (no seed from grain, whatever T); cut: from this
    frame on another scene; dim: this frame's source is 5 levels brighter (a half-open pair); plain: this frame is not inpainted;
    far: (frame, y, x): the source of that frame is 40 levels off at one pixel (no seed at T = 12, passed over by the threshold)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = (30 + 0.1 * x + 0.2 * y)[None, :, :, None] + np.zeros((n, 1, 1, 3))
    if cut is not None:
        base[cut:] += 90
    if dim is not None:
        base[dim] += 5
    src = np.rint(base + rng.normal(0, 2, base.shape))
    other = np.rint(base + rng.normal(0, 2, base.shape))
    if far is not None:
        src[far[0], far[1], far[2]] += 40
    fill = src.copy()
    inside = cmask != 0
    if not exact:
        fill[:, inside] = other[:, inside]
    for f in range(n):
        for yy, xx in spots(H, W, cmask, (f // period) % 2):
            block = np.zeros((H, W), bool)
            block[yy:yy + 2, xx:xx + 4] = True
            src[f][block] = 255
            fill[f][block & inside] = other[f][block & inside]
            fill[f][block & ~inside] = 255                   # outside C the fill is the source
    src, fill = np.clip(src, 0, 255).astype(np.uint8), np.clip(fill, 0, 255).astype(np.uint8)
    if plain is not None:
        fill[plain] = src[plain]
    return fill, src


def gpu_borrow(lib, dev, fill, src, cmask, rows, t, b, y0=0, lead=5, gap=7, src_lead=3, src_gap=13):
    H, W = cmask.shape
    n, h = fill.shape[:2]
    size = h * W * 3
    c0, c1 = rows_of(cmask) if cmask.any() else (0, 0)
    cbuf = torch.full((H * W + 128,), 255, dtype=torch.uint8, device=dev)         # a read beyond the mask would find pixels of it
    cbuf[64:64 + H * W] = torch.from_numpy(np.ascontiguousarray(cmask).ravel()).to(dev)
    cp = C.c_void_p(cbuf.data_ptr() + 64)
    fstride, sstride = size + gap, size + src_gap
    fbuf = np.full(lead + n * fstride + 32, 0x5A, np.uint8)
    sbuf = np.full(src_lead + n * sstride + 32, 0xC3, np.uint8)
    for f in range(n):
        fbuf[lead + f * fstride:lead + f * fstride + size] = fill[f].ravel()
        sbuf[src_lead + f * sstride:src_lead + f * sstride + size] = src[f].ravel()
    ft, st = torch.from_numpy(fbuf).to(dev), torch.from_numpy(sbuf).to(dev)
    fp, sp = C.c_void_p(ft.data_ptr() + lead), C.c_void_p(st.data_ptr() + src_lead)
    map_ = torch.empty((H, W), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    stats = torch.empty((n, 4), dtype=torch.int64, device=dev)
    pairs = torch.empty((n, b), dtype=torch.int64, device=dev)
    L = lib.lib
    assert L.vsr_regrain_sets(cp, H, W, rows[0], rows[1], P(map_), P(counts), None) == 0, lib.last_error()
    assert L.vsr_regrain_measure(fp, fstride, sp, sstride, P(map_), n, H, W, y0, h, c0, c1, P(stats), None) == 0, lib.last_error()
    assert L.vsr_deflicker_pairs(sp, sstride, P(map_), n, H, W, y0, h, c0, c1, b, P(pairs), None) == 0, lib.last_error()
    nbytes = L.vsr_borrow_workspace_bytes(H, W, n)
    assert nbytes == bs.workspace_bytes(H, W, n) == 2 * L.vsr_key_workspace_bytes(H, W, n) and nbytes % 8 == 0
    work = torch.full((nbytes // 8 + 2,), -1, dtype=torch.int64, device=dev)      # garbage: the call writes what it reads
    rc = L.vsr_borrow_apply(fp, fstride, sp, sstride, cp, P(counts), P(stats), P(pairs), n, H, W, y0, h, c0, c1, t, b,
                            C.c_void_p(work.data_ptr() + 8), None)
    assert rc == 0, lib.last_error()
    torch.cuda.synchronize()
    got = ft.cpu().numpy()
    assert np.array_equal(st.cpu().numpy(), sbuf), "src was written"
    assert int(work[0]) == -1 and int(work[-1]) == -1, "a word in front of or behind the workspace was written"
    guard = cbuf.cpu().numpy()
    assert (guard[:64] == 255).all() and (guard[64 + H * W:] == 255).all() and np.array_equal(guard[64:64 + H * W], cmask.ravel())
    out = np.stack([got[lead + f * fstride:lead + f * fstride + size].reshape(h, W, 3) for f in range(n)])
    untouched = np.ones(got.size, bool)
    for f in range(n):
        untouched[lead + f * fstride:lead + f * fstride + size] = False
    assert np.array_equal(got[untouched], fbuf[untouched]), "bytes in front of, between or behind the frames were written"
    return out


def check(lib, dev, fill, src, cmask, b, t=T, rows=None, y0=0, **kw):
    rows = (0, cmask.shape[0]) if rows is None else rows
    info = {}
    want = bs.borrow(fill, src, cmask, rows, t, b, y0=y0, info=info)
    out = gpu_borrow(lib, dev, fill, src, cmask, rows, t, b, y0=y0, **kw)
    assert np.array_equal(out, want), f"{int((out != want).sum())} bytes differ from the statement, by up to " \
                                      f"{int(np.abs(out.astype(int) - want).max())}, first at {np.argwhere(out != want)[0].tolist()}"
    return out, info


def events(info):
    """what the statement did: (taken at distance 1, taken from farther, refused by N_s, refused by the threshold, left with the fill)"""
    lender = info["lender"]
    t = np.arange(lender.shape[0])[:, None, None]
    dist = np.where(lender >= 0, np.abs(lender - t), 0)
    return (int((dist == 1).sum()), int((dist > 1).sum()), info["refused_near"], info["refused_threshold"],
            int((info["borrowers"] & (lender < 0)).sum()))


def not_vacuous(info, cmask, name):
    ev = events(info)
    print(name, "m =", info["m"], "weights:", sorted(set(info["b"].values())), "taken at 1 / farther, refused by N / threshold, left:", ev)
    if info["m"] == 0:
        assert ev[0] == ev[1] == 0 and ev[4] > 0, "no ring: every pair is closed"
    elif int((cmask != 0).sum()) >= 50:
        assert all(v > 0 for v in ev), (name, ev)
    else:
        assert ev[2] + ev[4] > 0, (name, ev)                 # a borrower there is, and a lender was judged


@pytest.mark.parametrize("shape", SHAPES)
def test_the_kernels_equal_the_statement(built_lib, gpu_device, shape):
    """n = 5, B = 2: the glyphs change place behind frame 2, frame 3 is 5 levels brighter, frame 4 is not inpainted"""
    H, W = shape
    for k, (name, cmask) in enumerate(masks(H, W).items()):
        ys, xs = np.nonzero(cmask)
        far = (3, int(ys[0]), int(xs[0]) + (1 if xs[0] + 1 < W and cmask[ys[0], min(xs[0] + 1, W - 1)] else 0))
        fill, src = clip(H, W, cmask, 5, seed=H + k, plain=4, dim=3, far=far)
        out, info = check(built_lib, gpu_device, fill, src, cmask, 2)
        not_vacuous(info, cmask, f"{H}x{W} {name}")
        inside = cmask != 0
        assert np.array_equal(out[:, ~inside], fill[:, ~inside]), name
        assert not info["Z"][4].any() and np.array_equal(out[4], fill[4]), "the frame with fill == src borrows nothing"
        if info["m"] and int(inside.sum()) >= 50:
            assert (info["lender"] == 4).any(), "and lends"
        if info["m"]:
            assert any(0 < v < 16 for v in info["b"].values()), "a half-open pair"
            assert np.abs(out.astype(int) - fill).max() < 24
        if name == "two boxes" and cmask[H // 2, 52:66].all():
            # here the ring is there (m > 0), so that k_borrow_near's carries across the word boundary are seen in the frames
            N, mid = info["N"], H // 2
            assert N[0, mid, 63] and not N[0, mid, 64] and N[3, mid, 64] and not N[3, mid, 65], "N ends on either side of the boundary"
            assert (info["lender"][:, mid - 1:mid + 3, 56:66] >= 0).any() and (out != fill)[:, mid - 1:mid + 3, 56:66].any()
        if name == "whole picture" and W > 72:
            # (m = 0: every threshold is 0 and k_borrow_take leaves every frame whole, so these look at the statement's N alone -- what
            # the clip was planned to hold; the kernel's N is observed under the masks that have a ring, above)
            N = info["N"]
            mid = H // 2
            assert N[0, mid, 63] and not N[0, mid, 64] and N[3, mid, 64] and not N[3, mid, 65], "N ends on either side of the boundary"
            if H >= 40:
                assert N[0, mid - 20, 64] and not N[0, mid - 20, 63] and N[3, mid - 20, 63] and not N[3, mid - 20, 62]
            assert N[0, 0, 0] and N[0, H - 1, W - 1] and N[3, 0, W - 1] and N[3, H - 1, 0], "the corners"


@pytest.mark.parametrize("n,b", [(2, 1), (2, 8), (5, 1), (5, 8), (17, 8)])
def test_windows(built_lib, gpu_device, n, b):
    """n = 17, B = 8: a full two-sided window, and a cut behind frame 8 that nothing is lent across"""
    H, W = SHAPES[0]
    cmask = masks(H, W)["two boxes"]
    period = 1 if n == 2 else 3
    fill, src = clip(H, W, cmask, n, seed=n + b, period=period, cut=9 if n == 17 else None, dim=12 if n == 17 else None)
    out, info = check(built_lib, gpu_device, fill, src, cmask, b)
    ev = events(info)
    print(n, b, ev, sorted(set(info["b"].values())))
    assert ev[0] > 0
    if n == 17:
        assert all(v > 0 for v in ev), "frame 12 is 5 levels brighter: half-open pairs, and lenders passed over by their threshold"
        lender = info["lender"]
        assert not (lender[:9] >= 9).any() and not ((lender[9:] >= 0) & (lender[9:] < 9)).any(), "a cut lends nothing across it"
        assert all(info["b"][(t, k)] == 0 for (t, k) in info["b"] if t < 9 <= t + k)
        assert (lender[8] >= 0).any() and (lender[9] >= 0).any(), "the windows at the cut are one-sided"


@pytest.mark.parametrize("t", [1, 12, 128])
def test_thresholds(built_lib, gpu_device, t):
    """the fill is the source away from the glyphs, so that the grain is no seed even at T = 1"""
    H, W = SHAPES[0]
    cmask = masks(H, W)["two boxes"]
    fill, src = clip(H, W, cmask, 5, seed=t, exact=True)
    out, info = check(built_lib, gpu_device, fill, src, cmask, 2, t=t)
    ev = events(info)
    print(t, ev)
    assert info["Z"].any() and ev[0] > 0 and ev[2] > 0 and (out != fill).any()


@pytest.mark.parametrize("lead,src_lead", [(0, 0), (1, 16), (15, 15)])
def test_every_alignment(built_lib, gpu_device, lead, src_lead):
    H, W = SHAPES[0]
    cmask = masks(H, W)["bottom box"]
    fill, src = clip(H, W, cmask, 5, seed=21)
    out, info = check(built_lib, gpu_device, fill, src, cmask, 2, lead=lead, src_lead=src_lead, gap=lead % 5, src_gap=0 if lead else 29)
    assert events(info)[0] > 0


def test_strip_rows(built_lib, gpu_device):
    """y0 = 5, h = 33 of H = 45 with the sample rows [5, 38): a mask inside the rows comes back as the rows of the full-frame result;
    one that the rows cut states its own rows"""
    H, W = SHAPES[0]
    y0, h = 5, 33
    cmask = np.zeros((H, W), np.uint8)
    cmask[14:30, 6:W - 11] = 255
    fill, src = clip(H, W, cmask, 5, seed=H)
    whole, info = check(built_lib, gpu_device, fill, src, cmask, 2, rows=(y0, y0 + h))
    rows, _ = check(built_lib, gpu_device, fill[:, y0:y0 + h], src[:, y0:y0 + h], cmask, 2, rows=(y0, y0 + h), y0=y0)
    assert np.array_equal(rows, whole[:, y0:y0 + h]) and events(info)[0] > 0
    cmask[6:9, W // 3:W // 2] = 255                                 # N's window is clipped by the first row held
    cmask[34:37, 20:70] = 9
    fill, src = clip(H, W, cmask, 5, seed=H + 1)
    rows, info = check(built_lib, gpu_device, fill[:, y0:y0 + h], src[:, y0:y0 + h], cmask, 2, rows=(y0, y0 + h), y0=y0)
    assert info["N"].shape[1] == h and events(info)[0] > 0


def test_nothing_to_do_is_success(built_lib, gpu_device):
    t = torch.full((64,), 3, dtype=torch.int64, device=gpu_device)
    lib = built_lib.lib
    assert lib.vsr_borrow_workspace_bytes(3, 3, 0) == 0 and lib.vsr_borrow_workspace_bytes(1080, 1920, 50) == 2 * 50 * 1080 * 30 * 8
    assert lib.vsr_borrow_apply(P(t), 27, P(t), 27, P(t), P(t), P(t), P(t), 1, 3, 3, 0, 3, 0, 3, T, 2, P(t), None) == 0, "n = 1"
    assert lib.vsr_borrow_apply(P(t), 27, P(t), 27, P(t), P(t), P(t), P(t), 0, 3, 3, 0, 3, 0, 3, T, 2, P(t), None) == 0, "n = 0"
    assert lib.vsr_borrow_apply(P(t), 27, P(t), 27, P(t), P(t), P(t), P(t), 2, 3, 3, 0, 3, 2, 2, T, 2, P(t), None) == 0, "c0 == c1"
    # the rows held lie beside the rows of C: nothing is launched
    assert lib.vsr_borrow_apply(P(t), 27, P(t), 27, P(t), P(t), P(t), P(t), 2, 9, 3, 0, 3, 5, 8, T, 2, P(t), None) == 0
    torch.cuda.synchronize()
    assert (t == 3).all()


def test_argument_errors(built_lib, gpu_device):
    lib = built_lib.lib
    frames = torch.full((4096,), 9, dtype=torch.uint8, device=gpu_device)
    src = torch.full((4096,), 7, dtype=torch.uint8, device=gpu_device)
    cm = torch.full((4096,), 4, dtype=torch.uint8, device=gpu_device)
    words = torch.full((4096,), 5, dtype=torch.int64, device=gpu_device)
    size = 8 * 8 * 3
    ok = dict(frames=P(frames), fs=size, src=P(src), ss=size, cm=P(cm), counts=P(words), stats=P(words), pairs=P(words), n=2, H=8, W=8,
              y0=0, rows=8, c0=2, c1=6, T=T, B=2, work=P(words))

    def apply(**kw):
        a = dict(ok, **kw)
        return lib.vsr_borrow_apply(a["frames"], a["fs"], a["src"], a["ss"], a["cm"], a["counts"], a["stats"], a["pairs"], a["n"], a["H"],
                                    a["W"], a["y0"], a["rows"], a["c0"], a["c1"], a["T"], a["B"], a["work"], None)

    bad = [dict(frames=None), dict(src=None), dict(cm=None), dict(work=None), dict(counts=None), dict(stats=None), dict(pairs=None),
           dict(H=0), dict(W=-1), dict(n=-1), dict(fs=size - 1), dict(ss=size - 1), dict(y0=-1), dict(y0=1), dict(rows=0), dict(rows=-3),
           dict(rows=9), dict(c0=-1), dict(c0=7, c1=6), dict(c1=9), dict(H=32768, W=32768, rows=1), dict(T=0), dict(T=-1), dict(T=129),
           dict(B=0), dict(B=-1), dict(B=9), dict(work=C.c_void_p(words.data_ptr() + 4))]
    for kw in bad:
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "borrow" in built_lib.last_error(), kw
    for args in ((0, 8, 1), (8, -1, 1), (8, 8, -1), (32768, 32768, 1)):
        assert lib.vsr_borrow_workspace_bytes(*args) == built_lib.VSR_ERR_ARG, args
        assert "borrow" in built_lib.last_error(), args
    torch.cuda.synchronize()
    assert (frames == 9).all() and (src == 7).all() and (cm == 4).all() and (words == 5).all(), "a refused call wrote something"
