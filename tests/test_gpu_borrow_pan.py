"""The borrow-pan kernels through the C-ABI (vsr_borrow_pan_workspace_bytes, vsr_borrow_pan_search, vsr_borrow_pan_apply;
csrc/borrow_pan_kernels.hip) against the numpy statement (tests/_borrow_pan_statement.py): the search table equals the statement's S and
cnt for every (t, k, slot), the levels k >= 2 included, and the frames equal the statement's byte for byte; unaligned and strided
frames, guard bytes round the frames, the mask and the workspace, a workspace of garbage, the strip-row form, a cut, a still clip
(vsr_borrow_apply's bytes), pans in the four directions and a diagonal one, argument errors.  The shapes are the key's
(tests/test_gpu_glyph_key.py): 45 x 75, 130 x 260 (five words, row tiles of every kernel), 20 x 64 and 20 x 65 (exactly one word, and
one bit in a second), 7 x 130 (fewer rows than any tile).

The clips are tests/_borrow_pan_clips.py's.  Under the mask "two boxes" (it touches the picture's left side and spans column 64) a pan
along the rows shows every kind of event at once, and the case asserts each from the statement's info: a pair with D != 0, a pair kept
at 0 by b_0 = 16 (the camera rests between frames 0 and 1), a lender pixel in another 64-column word than its borrower, a lender pixel
outside C, a q off the frame, a lender passed over for its own glyph at q, one passed over by the threshold, a borrower left with its
fill.  A picture of 64 columns has one word per row and cannot show the third; the whole-picture mask has no ring (|E| = 0), every pair
is closed and the frames must come back as the fill."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _borrow_pan_clips as pc
from tests import _borrow_pan_statement as ps
from tests.test_gpu_glyph_key import masks, rows_of

pytestmark = pytest.mark.gpu

SHAPES = [(45, 75), (20, 64), (20, 65), (7, 130), (130, 260)]
T = 12
ALL = ("shifted_pairs", "full_pairs", "crosses_word", "lent_from_outside", "off_frame", "own_glyph", "threshold", "left")


def P(t):
    return C.c_void_p(t.data_ptr())


def gpu_pan(lib, dev, fill, src, cmask, rows, t, b, p, y0=0, lead=5, gap=7, src_lead=3, src_gap=13):
    """-> (frames, S, cnt): the frames after vsr_borrow_pan_apply and the table vsr_borrow_pan_search left"""
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
    L = lib.lib
    assert L.vsr_regrain_sets(cp, H, W, rows[0], rows[1], P(map_), P(counts), None) == 0, lib.last_error()
    assert L.vsr_regrain_measure(fp, fstride, sp, sstride, P(map_), n, H, W, y0, h, c0, c1, P(stats), None) == 0, lib.last_error()
    nbytes = L.vsr_borrow_pan_workspace_bytes(H, W, n, b, p)
    assert nbytes == ps.workspace_bytes(H, W, n, b, p) and nbytes % 8 == 0
    work = torch.full((nbytes // 8 + 2,), -1, dtype=torch.int64, device=dev)      # garbage: the calls write what they read
    wp = C.c_void_p(work.data_ptr() + 8)
    assert L.vsr_borrow_pan_search(sp, sstride, P(map_), P(counts), n, H, W, y0, h, c0, c1, b, p, wp, None) == 0, lib.last_error()
    assert L.vsr_borrow_pan_apply(fp, fstride, sp, sstride, cp, P(counts), P(stats), n, H, W, y0, h, c0, c1, t, b, p, wp, None) == 0, \
        lib.last_error()
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
    nc = ps.slots(p)
    table = work[1:1 + ps.table_words(n, b, p)].cpu().numpy().reshape(n, b, nc + 1, 2)
    return out, table[:, :, :nc, 0], table[:, :, :nc, 1]


def check(lib, dev, fill, src, cmask, b, p, t=T, rows=None, y0=0, **kw):
    rows = (0, cmask.shape[0]) if rows is None else rows
    info = {}
    want = ps.borrow_pan(fill, src, cmask, rows, t, b, p, y0=y0, info=info)
    out, S, cnt = gpu_pan(lib, dev, fill, src, cmask, rows, t, b, p, y0=y0, **kw)
    assert np.array_equal(cnt, info["cnt"]), f"cnt differs first at (t, k - 1, slot) = {np.argwhere(cnt != info['cnt'])[0].tolist()}"
    assert np.array_equal(S, info["S"]), f"S differs first at (t, k - 1, slot) = {np.argwhere(S != info['S'])[0].tolist()}"
    assert np.array_equal(out, want), f"{int((out != want).sum())} bytes differ from the statement, by up to " \
                                      f"{int(np.abs(out.astype(int) - want).max())}, first at {np.argwhere(out != want)[0].tolist()}"
    return out, info


def show(info, name, need):
    ev = pc.events(info)
    print(name, "m =", info["m"], "R:", sorted(set(info["R"].values())), "w:", sorted(set(info["w"].values())), ev)
    assert all(ev[key] > 0 for key in need), (name, {key: ev[key] for key in need})
    return ev


@pytest.mark.parametrize("shape", SHAPES)
def test_the_kernels_equal_the_statement(built_lib, gpu_device, shape):
    """n = 5, B = 2, P = 3: two columns per frame to the right, the camera rests between frames 0 and 1, the glyphs change place
    every second frame"""
    H, W = shape
    for k, (name, cmask) in enumerate(masks(H, W).items()):
        if name == "one pixel":
            continue
        fill, src = pc.clip(H, W, cmask, 5, (0, 2), seed=H + W + k, still=(1,))
        out, info = check(built_lib, gpu_device, fill, src, cmask, 2, 3)
        inside = cmask != 0
        assert np.array_equal(out[:, ~inside], fill[:, ~inside]), name
        if name == "whole picture":
            ev = show(info, f"{H}x{W} {name}", ("left",))
            assert info["m"] == 0 and ev["taken"] == 0 and np.array_equal(out, fill), "no ring: every pair is closed"
        elif name == "two boxes":
            show(info, f"{H}x{W} {name}", [key for key in ALL if key != "crosses_word" or W > 64])
            assert info["D"][(0, 1)] == (0, 0) and info["b0"][(0, 1)] == 16 and info["D"][(1, 1)] == (0, 2) and info["D"][(1, 2)] == (0, 4)
            assert np.abs(out.astype(int) - fill).max() < 24
        else:
            show(info, f"{H}x{W} {name}", ("shifted_pairs", "full_pairs", "lent_from_outside", "own_glyph", "threshold", "left"))


@pytest.mark.parametrize("n,b,p,step", [(2, 1, 1, (0, 1)), (2, 8, 3, (0, -3)), (5, 1, 8, (0, 7)), (5, 8, 8, (-1, 8)), (17, 8, 3, (0, 2)),
                                        (17, 2, 8, (1, -6)), (5, 8, 1, (0, 1))])
def test_windows(built_lib, gpu_device, n, b, p, step):
    """B > n - 1 included; n = 17: a cut behind frame 8 that nothing is lent across, and levels up to k = 8 whose centres move on"""
    H, W = SHAPES[0]
    cmask = masks(H, W)["two boxes"]
    fill, src = pc.clip(H, W, cmask, n, step, seed=n + b + p, period=1 if n == 2 else 3, cut=9 if n == 17 else None)
    out, info = check(built_lib, gpu_device, fill, src, cmask, b, p)
    ev = show(info, f"n = {n} B = {b} P = {p}", ("shifted_pairs", "taken"))
    assert info["R"][(0, 1)] == step
    if b > 1 and n > 2:
        assert any(max(abs(d[0]), abs(d[1])) > p for d in info["D"].values()), "a shift beyond P, reached along the chain"
    if n == 17:
        lender = info["lender"]
        assert not (lender[:9] >= 9).any() and not ((lender[9:] >= 0) & (lender[9:] < 9)).any(), "a cut lends nothing across it"
        assert all(info["w"][(t, k)] == 0 for (t, k) in info["w"] if t < 9 <= t + k)
        assert (lender[8] >= 0).any() and (lender[9] >= 0).any(), "the windows at the cut are one-sided"


@pytest.mark.parametrize("step", [(0, 3), (0, -3), (2, 0), (-2, 0), (2, -3)])
def test_directions(built_lib, gpu_device, step):
    H, W = SHAPES[4]
    cmask = masks(H, W)["two boxes"]
    fill, src = pc.clip(H, W, cmask, 4, step, seed=20 + step[0] * 5 + step[1])
    out, info = check(built_lib, gpu_device, fill, src, cmask, 3, 3)
    show(info, f"step {step}", ("shifted_pairs", "taken", "own_glyph", "left"))
    assert all(info["D"][(t, k)] == (k * step[0], k * step[1]) for (t, k) in info["D"]), info["D"]
    moved = (info["lender"] >= 0) & ((info["q"] != np.stack(np.mgrid[0:H, 0:W], axis=-1)[None]).any(axis=-1))
    assert moved.any() and (out != fill).any()


@pytest.mark.parametrize("t", [1, 12, 128])
def test_thresholds(built_lib, gpu_device, t):
    H, W = SHAPES[0]
    cmask = masks(H, W)["two boxes"]
    fill, src = pc.clip(H, W, cmask, 5, (0, 2), seed=t)
    out, info = check(built_lib, gpu_device, fill, src, cmask, 2, 3, t=t)
    ev = show(info, f"T = {t}", ("shifted_pairs",) if t > 12 else ("shifted_pairs", "taken", "left"))
    assert info["Z"].any()


@pytest.mark.parametrize("lead,src_lead", [(0, 0), (1, 16), (15, 15)])
def test_every_alignment(built_lib, gpu_device, lead, src_lead):
    H, W = SHAPES[0]
    cmask = masks(H, W)["bottom box"]
    fill, src = pc.clip(H, W, cmask, 5, (0, -2), seed=21)
    out, info = check(built_lib, gpu_device, fill, src, cmask, 2, 3, lead=lead, src_lead=src_lead, gap=lead % 5, src_gap=0 if lead else 29)
    show(info, f"lead {lead}", ("shifted_pairs", "taken"))


def test_strip_rows(built_lib, gpu_device):
    """y0 = 5, h = 33 of H = 45 with the sample rows [5, 38): along the rows the strip is the rows of the full-frame result; down the
    columns V and q end at the rows held, and the strip states its own rows"""
    H, W = SHAPES[0]
    y0, h = 5, 33
    cmask = np.zeros((H, W), np.uint8)
    cmask[14:30, 6:W - 11] = 255
    fill, src = pc.clip(H, W, cmask, 5, (0, 2), seed=H)
    whole, info = check(built_lib, gpu_device, fill, src, cmask, 2, 3, rows=(y0, y0 + h))
    rows, _ = check(built_lib, gpu_device, fill[:, y0:y0 + h], src[:, y0:y0 + h], cmask, 2, 3, rows=(y0, y0 + h), y0=y0)
    assert np.array_equal(rows, whole[:, y0:y0 + h])
    show(info, "strip, along the rows", ("shifted_pairs", "taken"))
    cmask[6:9, W // 3:W // 2] = 255                                 # N's window and q are clipped by the first row held
    cmask[34:37, 20:70] = 9
    fill, src = pc.clip(H, W, cmask, 5, (2, 1), seed=H + 1)
    rows, info = check(built_lib, gpu_device, fill[:, y0:y0 + h], src[:, y0:y0 + h], cmask, 2, 3, rows=(y0, y0 + h), y0=y0)
    assert info["N"].shape[1] == h
    show(info, "strip, down the columns", ("shifted_pairs", "taken", "off_frame"))


def test_a_still_clip_gives_the_plain_pass_bytes(built_lib, gpu_device):
    from tests import _borrow_statement as bs
    from tests.test_gpu_borrow import gpu_borrow

    H, W = SHAPES[0]
    cmask = masks(H, W)["two boxes"]
    fill, src = pc.clip(H, W, cmask, 5, (0, 0), seed=3)
    out, info = check(built_lib, gpu_device, fill, src, cmask, 2, 8)
    assert set(info["b0"].values()) == {16} and set(info["D"].values()) == {(0, 0)} and pc.events(info)["taken"] > 0
    plain = gpu_borrow(built_lib, gpu_device, fill, src, cmask, (0, H), T, 2)
    assert np.array_equal(out, plain) and np.array_equal(out, bs.borrow(fill, src, cmask, (0, H), T, 2))


def test_nothing_to_do_is_success(built_lib, gpu_device):
    t = torch.full((4096,), 3, dtype=torch.int64, device=gpu_device)
    lib = built_lib.lib
    assert lib.vsr_borrow_pan_workspace_bytes(3, 3, 0, 2, 1) == 0
    for n, c0, c1, H in ((1, 0, 3, 3), (0, 0, 3, 3), (2, 2, 2, 3)):
        assert lib.vsr_borrow_pan_search(P(t), 27, P(t), P(t), n, H, 3, 0, 3, c0, c1, 2, 1, P(t), None) == 0, (n, c0, c1)
        assert lib.vsr_borrow_pan_apply(P(t), 27, P(t), 27, P(t), P(t), P(t), n, H, 3, 0, 3, c0, c1, T, 2, 1, P(t), None) == 0, (n, c0, c1)
    # the rows held lie beside the rows of C: the apply launches nothing
    assert lib.vsr_borrow_pan_apply(P(t), 27, P(t), 27, P(t), P(t), P(t), 2, 60, 3, 0, 3, 50, 58, T, 2, 1, P(t), None) == 0
    torch.cuda.synchronize()
    assert (t == 3).all()


def test_argument_errors(built_lib, gpu_device):
    lib = built_lib.lib
    frames = torch.full((4096,), 9, dtype=torch.uint8, device=gpu_device)
    src = torch.full((4096,), 7, dtype=torch.uint8, device=gpu_device)
    cm = torch.full((4096,), 4, dtype=torch.uint8, device=gpu_device)
    words = torch.full((4096,), 5, dtype=torch.int64, device=gpu_device)
    size = 8 * 8 * 3
    ok = dict(frames=P(frames), fs=size, src=P(src), ss=size, cm=P(cm), map=P(cm), counts=P(words), stats=P(words), n=2, H=8, W=8, y0=0,
              rows=8, c0=2, c1=6, T=T, B=2, P=1, work=P(words))

    def apply(**kw):
        a = dict(ok, **kw)
        return lib.vsr_borrow_pan_apply(a["frames"], a["fs"], a["src"], a["ss"], a["cm"], a["counts"], a["stats"], a["n"], a["H"], a["W"],
                                        a["y0"], a["rows"], a["c0"], a["c1"], a["T"], a["B"], a["P"], a["work"], None)

    def search(**kw):
        a = dict(ok, **kw)
        return lib.vsr_borrow_pan_search(a["src"], a["ss"], a["map"], a["counts"], a["n"], a["H"], a["W"], a["y0"], a["rows"], a["c0"],
                                         a["c1"], a["B"], a["P"], a["work"], None)

    shared = [dict(src=None), dict(counts=None), dict(work=None), dict(H=0), dict(W=-1), dict(n=-1), dict(ss=size - 1), dict(y0=-1),
              dict(y0=1), dict(rows=0), dict(rows=-3), dict(rows=9), dict(c0=-1), dict(c0=7, c1=6), dict(c1=9),
              dict(H=32768, W=32768, rows=1), dict(B=0), dict(B=-1), dict(B=9), dict(P=0), dict(P=-1), dict(P=9),
              dict(work=C.c_void_p(words.data_ptr() + 4))]
    for kw in shared + [dict(frames=None), dict(cm=None), dict(stats=None), dict(fs=size - 1), dict(T=0), dict(T=-1), dict(T=129)]:
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "borrow-pan" in built_lib.last_error(), kw
    for kw in shared + [dict(map=None)]:
        assert search(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "borrow-pan" in built_lib.last_error(), kw
    for args in ((0, 8, 1, 2, 1), (8, -1, 1, 2, 1), (8, 8, -1, 2, 1), (32768, 32768, 1, 2, 1), (8, 8, 1, 0, 1), (8, 8, 1, 9, 1),
                 (8, 8, 1, 2, 0), (8, 8, 1, 2, 9)):
        assert lib.vsr_borrow_pan_workspace_bytes(*args) == built_lib.VSR_ERR_ARG, args
        assert "borrow-pan" in built_lib.last_error(), args
    torch.cuda.synchronize()
    assert (frames == 9).all() and (src == 7).all() and (cm == 4).all() and (words == 5).all(), "a refused call wrote something"
