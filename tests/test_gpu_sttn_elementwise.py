"""The kernels of csrc/elementwise.hip one launch at a time, through the launchers the STTN engine calls, against the float64 / exact
references of tests/_sttn_ew_ref.py at edge shapes.

Conventions (those of tests/test_gpu_flow_kernels.py): one launch per case; every output buffer is pre-filled with a sentinel (-7.0,
0xA5 for u8) and compared WHOLE, so cells outside the kernel's store set must still hold it; the inputs of a launch stay alive until
after the synchronisation (_KEEP); split-format buffers start 128-byte aligned (asserted).  No launch leaves its kernel's contract:
invalid arguments are tried only where the launcher refuses them before launching.  Each tolerance is derived beside its assertion
(or in _sttn_ew_ref) before anything was measured; `RATIO got/bound` lines go to profiles/sttn_elementwise_errors.md.

tests/test_sttn_ew_reference.py checks the prototypes bound here against the headers without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import _sttn_ew_ref as R
from oracle import cv2_restate as cv2r

pytestmark = pytest.mark.gpu

U32, SENT, SENT_U8 = R.U32, R.SENT, R.SENT_U8
_CT = {"p": C.c_void_p, "i": C.c_int, "l": C.c_int64}


@pytest.fixture(scope="module")
def K(built_lib, gpu_device):
    lib = C.CDLL(built_lib.LIB_PATH)
    for name, sig in R.PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = [_CT[ch] for ch in sig]
    lib.ERR_ARG = built_lib.VSR_ERR_ARG
    return lib


_KEEP = []         # inputs of the next launch (see test_gpu_flow_kernels._KEEP); launch() releases them after synchronising


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off * t.element_size())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(fn, *args, want=0):
    rc = fn(*args, _stream())
    torch.cuda.synchronize()
    _KEEP.clear()
    assert rc == want, f"launcher returned {rc}, expected {want}"


def refused(K, fn, *args):
    """the launcher returns VSR_ERR_ARG; the caller checks that its output buffer still holds what it held"""
    rc = fn(*args, _stream())
    torch.cuda.synchronize()
    assert rc == K.ERR_ARG, f"launcher returned {rc}, expected VSR_ERR_ARG"


def ratio(what, err, bound):
    """err, bound: arrays of one shape.  Prints the largest err / bound and asserts err <= bound everywhere."""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    worst = np.unravel_index(np.argmax(q), q.shape) if q.size else ()
    print(f"RATIO | {what} | max err {err.max():.3e} | bound there {bound[worst]:.3e} | got/bound {q.max():.3f}")
    assert np.all(err <= bound), f"{what}: |got - ref64| = {err[worst]:.3e} > bound {bound[worst]:.3e} at {worst}"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def aligned128(t):
    assert t.data_ptr() % 128 == 0, "split-format buffers start 128-byte aligned"
    return t


# =====================================================================================================================================
# 2. k_upsample2x_nhwc through vsr_launch_upsample2x_rows
# =====================================================================================================================================
UPSAMPLE = [(1, 1, 4, 0, 0, 1), (1, 5, 4, 1, 0, 1), (5, 1, 8, 0, 2, 1), (2, 3, 36, 2, 1, 2), (7, 9, 32, 1, 1, 2), (3, 4, 64, 0, 1, 1)]
UPSAMPLE_RUNS = [(c, 0) for c in UPSAMPLE] + [(c, 1) for c in UPSAMPLE[-2:]]


def _upsample(K, rng, H, W, Cc, hs, hd, n, split, lo=None, hi=None):
    """one launch of output rows [lo, hi) (default: all); every cell outside them must hold the sentinel (checked here on the whole
    buffer).  Returns (the written cells as float64 [n][hi - lo][2W][C], the reference of those rows, A = the largest |source|)"""
    x = rng.standard_normal((n, H, W, Cc)).astype(np.float32) * np.float32(3.0)
    src = R.with_halo(x, hs, R.HALO_POISON).reshape(-1)
    before = np.full(n * (2 * H + 2 * hd) * (2 * W + 2 * hd) * Cc, SENT, np.float32)
    if split:
        assert src.size % 32 == 0 and before.size % 32 == 0 and Cc % 32 == 0
        hi16, lo16 = R.split_halves(x)
        x = (hi16.astype(np.float32) + lo16.astype(np.float32))             # what the kernel reads: hi + lo, exact in fp32
        R.to_split_whole(src)
    dsrc, ddst = dev(src), torch.from_numpy(before).cuda()
    if split:
        aligned128(dsrc), aligned128(ddst)
    lo, hi = (0, 2 * H) if lo is None else (lo, hi)
    launch(K.vsr_launch_upsample2x_rows, ptr(dsrc), H, W, Cc, hs, ptr(ddst), hd, n, split, lo, hi)
    got = ddst.cpu().numpy()
    Hd, Wd = 2 * H + 2 * hd, 2 * W + 2 * hd
    written = np.zeros((n, Hd, Wd, Cc), dtype=bool)
    written[:, hd + lo:hd + hi, hd:hd + 2 * W] = True
    cells = np.flatnonzero(written.reshape(-1))
    if split:
        assert R.split_untouched(got, before, cells), "halo or rows outside the range were written"
        vals = R.split_decode(got, cells)
    else:
        assert np.all(got[~written.reshape(-1)] == SENT), "halo or rows outside the range were written"
        vals = got[cells].astype(np.float64)
    ref = R.upsample_ref(x)[:, lo:hi]
    return vals.reshape(ref.shape), ref, float(np.abs(x).max())


@pytest.mark.parametrize("case,split", UPSAMPLE_RUNS, ids=[f"{'x'.join(map(str, c))}{'-split' if s else ''}" for c, s in UPSAMPLE_RUNS])
def test_upsample2x(K, case, split):
    """F.interpolate(x.double(), scale_factor=2, bilinear, align_corners=True) on the interior, inside the destination halo; the
    source halo holds 1e30 (inf / -inf halves in split format), the destination halo the sentinel"""
    H, W, Cc, hs, hd, n = case
    got, ref, A = _upsample(K, np.random.default_rng(200 + H * 10 + W), H, W, Cc, hs, hd, n, split)
    assert np.isfinite(got).all(), "a halo cell of the source was read"
    bound = R.upsample_bound(H, W, A)                   # derived there
    if split:
        bound = bound + R.split_term(np.abs(ref) + bound)       # the stored value's two halves (derived there)
    ratio(f"upsample2x {case} split{split}", np.abs(got - ref), bound)


@pytest.mark.parametrize("lo,hi", [(0, 0), (11, 12), (3, 8), (0, 12)])
def test_upsample2x_row_range(K, lo, hi):
    """output rows [lo, hi) only; [0, 0) launches nothing; rows outside keep the sentinel (checked on the whole buffer)"""
    H, W, Cc, hs, hd, n = 6, 5, 4, 1, 1, 2
    got, ref, A = _upsample(K, np.random.default_rng(260), H, W, Cc, hs, hd, n, 0, lo, hi)
    assert got.shape == (n, hi - lo, 2 * W, Cc)
    if hi > lo:
        ratio(f"upsample2x rows [{lo}, {hi})", np.abs(got - ref), R.upsample_bound(H, W, A))


def test_upsample2x_refusals(K):
    H, W, hs, hd, n = 6, 5, 1, 1, 2
    src = dev(np.zeros(n * (H + 2 * hs) * (W + 2 * hs) * 64, np.float32))
    dst = torch.full((n * (2 * H + 2 * hd) * (2 * W + 2 * hd) * 64,), float(SENT), device="cuda")
    for Cc, split, lo, hi in [(4, 0, -1, 4), (4, 0, 0, 13), (4, 0, 5, 4),            # oyLo < 0, oyHi > 2H, oyLo > oyHi
                              (6, 0, 0, 12), (3, 0, 0, 12), (1, 0, 0, 12),            # C % 4
                              (36, 1, 0, 12), (16, 1, 0, 12)]:                        # split and C % 32
        refused(K, K.vsr_launch_upsample2x_rows, ptr(src), H, W, Cc, hs, ptr(dst), hd, n, split, lo, hi)
    _KEEP.clear()
    assert bool((dst == float(SENT)).all())


# =====================================================================================================================================
# 3. k_decode_out through vsr_launch_decode_out_rows: bit-exact, no exempted cells
# =====================================================================================================================================
def _comp_preset(rng, L, pix, kind):
    if kind == "u8":
        return rng.integers(0, 256, size=(L, pix, 3)).astype(np.float32)
    return (rng.integers(0, 1021, size=(L, pix, 3)) / 4.0).astype(np.float32)          # averaged twice already: multiples of 1/4


def _decode(K, rng, rows, W, blkW, ldy, frame_idx, first, L, preset, pLo, pCnt, det=False, want=0):
    """one launch of n = len(frame_idx) slots on a rows x W image; returns (got comp [L][pix][3], comp0, s, in_bgr, mask)"""
    n, pix = len(frame_idx), rows * W
    s = R.decode_inputs(rng, (n, pix, 3))
    y = R.to_blocked(s, rows, blkW, ldy, R.HALO_POISON) if blkW else R.to_plain(s, ldy, R.HALO_POISON)
    comp0 = _comp_preset(rng, L, pix, preset)
    in_bgr = mask = None
    if det:
        in_bgr = rng.integers(0, 256, size=(L, pix, 3), dtype=np.uint8)
        assert all(not np.array_equal(in_bgr[a], in_bgr[b]) for a in range(L) for b in range(a))
        mask = rng.choice(np.array([0, 0, 1, 127, 128, 255], np.uint8), size=(L, pix))
        assert all(not np.array_equal(mask[a], mask[b]) for a in range(L) for b in range(a))
    dy, dcomp = dev(y), torch.from_numpy(comp0.copy()).cuda()
    dfi, dfirst = dev(np.asarray(frame_idx, np.int32)), dev(np.asarray(first, np.int32))
    dbgr, dmask = (dev(in_bgr), dev(mask)) if det else (None, None)
    launch(K.vsr_launch_decode_out_rows, ptr(dy), ldy, pix, n, ptr(dfi), ptr(dfirst), ptr(dcomp), ptr(dbgr) if det else None,
           ptr(dmask) if det else None, blkW, pLo, pCnt, want=want)
    return dcomp.cpu().numpy(), comp0, s, in_bgr, mask


def _decode_check(got, comp0, s, frame_idx, first, pLo, pCnt, in_bgr, mask, what):
    """every cell of comp: frames addressed once equal the reference; a frame addressed by two slots of the launch holds, cell by
    cell, one of the values two unordered updates can leave (decode_outcomes); everything else keeps its bits"""
    frame_idx = [int(i) for i in frame_idx]
    once = [f for f, i in enumerate(frame_idx) if frame_idx.count(i) == 1]
    ref = R.decode_ref(s[once], comp0, [frame_idx[f] for f in once], [first[f] for f in once], pLo, pCnt, in_bgr, mask)
    twice = sorted({i for i in frame_idx if frame_idx.count(i) == 2})
    assert all(frame_idx.count(i) <= 2 for i in frame_idx)
    g = got.astype(np.float64)
    sl = slice(pLo, pLo + pCnt)
    for L_ in range(comp0.shape[0]):
        if L_ in twice:
            a, b = [f for f, i in enumerate(frame_idx) if i == L_]
            imgs = [R.decode_slot_image(s[f], None if mask is None else in_bgr[L_], None if mask is None else mask[L_])[sl] for f in (a, b)]
            outs = R.decode_outcomes(comp0[L_, sl].astype(np.float64), imgs[0], first[a], imgs[1], first[b])
            ok = np.zeros(g[L_, sl].shape, dtype=bool)
            for o in outs:
                ok |= g[L_, sl] == o
            assert ok.all(), f"{what}: frame {L_} (two slots): {int((~ok).sum())} cells hold none of the possible values"
            keep = np.ones(comp0.shape[1], dtype=bool)
            keep[sl] = False
            assert same_bits(got[L_, keep], comp0[L_, keep]), f"{what}: frame {L_}: pixels outside the range changed"
        elif L_ in frame_idx:
            bad = np.flatnonzero((g[L_] != ref[L_]).any(-1))
            assert bad.size == 0, f"{what}: frame {L_}: {bad.size} pixels differ, first {bad[:4]}: got {g[L_, bad[:2]]} want {ref[L_, bad[:2]]}"
        else:
            assert same_bits(got[L_], comp0[L_]), f"{what}: frame {L_} is in no slot and changed"
    return ref


# (rows, W, blkW, ldy): pix 8 = one 2 x 4 block, 2 x 12, and 2 x 64 (384 values per slot: every level in slot 0)
DECODE_SHAPES = [(2, 4, 0, 3), (2, 12, 0, 24), (2, 64, 0, 32), (2, 4, 4, 24), (2, 12, 12, 40), (4, 12, 12, 24), (2, 64, 4, 40)]


@pytest.mark.parametrize("rows,W,blkW,ldy", DECODE_SHAPES, ids=[f"{r}x{w}-blk{b}-ld{l}" for r, w, b, l in DECODE_SHAPES])
@pytest.mark.parametrize("frame_idx", [[4, 1, 1], [4, 1, 2]], ids=["idx411", "idx412"])
@pytest.mark.parametrize("first,preset", [([1, 0, 1], "u8"), ([0, 0, 0], "quarter")], ids=["first101-u8", "first000-quarters"])
def test_decode_out(K, rows, W, blkW, ldy, frame_idx, first, preset):
    """tanh -> level -> first visit or average, plain and blocked layouts, whole frames.  The inputs keep the float64 value 1/128
    at least from an integer (test_sttn_ew_reference), so a correct tanhf cannot cross a truncation boundary and every cell must be
    equal; u8-valued and quarter-valued presets average exactly in fp32.  frameIdx [4, 1, 1] addresses frame 1 from two slots of
    one launch -- two unordered read-modify-writes per cell -- so that frame is held to the set of values they can leave;
    [4, 1, 2] holds every frame to the one reference."""
    if blkW == 4 and W == 64:
        rows, W = 2 * 16, 4                  # 2 x 64 pixels as a 4-wide image: sixteen block rows of one block
    rng = np.random.default_rng(300 + rows + W + blkW + ldy)
    pix = rows * W
    got, comp0, s, _, _ = _decode(K, rng, rows, W, blkW, ldy, frame_idx, first, 5, preset, 0, pix)
    if pix == 128:
        assert np.array_equal(np.unique(R.decode_levels(s[0])), np.arange(256))
    _decode_check(got, comp0, s, frame_idx, first, 0, pix, None, None, f"decode {rows}x{W} blk{blkW} ld{ldy}")


@pytest.mark.parametrize("blkW,ldy", [(0, 32), (12, 40)], ids=["plain", "blocked"])
@pytest.mark.parametrize("which", ["whole", "middle-pair", "last-pair", "none"])
def test_decode_out_pixel_range(K, blkW, ldy, which):
    """pLo / pCnt: pixels outside the range and frames in no slot keep their bits; pCnt = 0 launches nothing"""
    rows, W = 6, 12
    pix = rows * W
    pLo, pCnt = {"whole": (0, pix), "middle-pair": (2 * W, 2 * W), "last-pair": (4 * W, 2 * W), "none": (2 * W, 0)}[which]
    rng = np.random.default_rng(330 + blkW)
    frame_idx, first = [4, 1, 2], [1, 0, 0]
    got, comp0, s, _, _ = _decode(K, rng, rows, W, blkW, ldy, frame_idx, first, 5, "quarter", pLo, pCnt)
    ref = _decode_check(got, comp0, s, frame_idx, first, pLo, pCnt, None, None, f"decode range {which} blk{blkW}")
    keep = np.ones(pix, dtype=bool)
    keep[pLo:pLo + pCnt] = False
    assert same_bits(got[:, keep], comp0[:, keep])
    assert pCnt == 0 or not np.array_equal(ref[[4, 1, 2]], comp0[[4, 1, 2]].astype(np.float64))


@pytest.mark.parametrize("blkW,ldy", [(0, 3), (12, 24)], ids=["plain", "blocked"])
@pytest.mark.parametrize("frame_idx", [[4, 1, 1], [2, 0, 3]], ids=["idx411", "idx203"])
def test_decode_out_keeps_input_under_a_zero_mask(K, blkW, ldy, frame_idx):
    """sttn-det: where the mask (values 0, 1, 127, 128, 255) is 0 the slot contributes the input frame with B and R swapped; mask
    and input are those of frame frameIdx[f] -- the frames differ, so slot f's would show"""
    rows, W = 4, 12
    pix = rows * W
    rng = np.random.default_rng(350 + blkW)
    first = [1, 0, 1]
    got, comp0, s, in_bgr, mask = _decode(K, rng, rows, W, blkW, ldy, frame_idx, first, 5, "u8", 0, pix, det=True)
    assert all((mask[i] == 0).sum() >= 4 and (mask[i] != 0).sum() >= 4 for i in frame_idx)
    _decode_check(got, comp0, s, frame_idx, first, 0, pix, in_bgr, mask, f"decode det blk{blkW}")
    if frame_idx == [2, 0, 3]:          # a first visit under a zero mask IS the swapped input
        z = mask[2] == 0
        assert np.array_equal(got[2][z], in_bgr[2][z][:, ::-1].astype(np.float32))


def test_decode_out_refusals(K):
    pix = 6 * 12
    y = dev(np.zeros(3 * pix * 40, np.float32))
    comp = torch.full((5 * pix * 3,), float(SENT), device="cuda")
    fi, first = dev(np.array([4, 1, 2], np.int32)), dev(np.array([1, 0, 0], np.int32))
    for ldy, pix_, blkW, pLo, pCnt in [(40, 72, 6, 0, 72),            # blkW % 4
                                       (40, 72, 16, 0, 64),           # pix % blkW
                                       (40, 36, 12, 0, 24),           # an odd number of rows
                                       (23, 72, 12, 0, 72),           # ldy < 24 in the blocked layout
                                       (40, 72, 0, 60, 13), (40, 72, 12, 48, 48),          # pLo + pCnt > pix
                                       (40, 72, 12, 12, 24), (40, 72, 12, 24, 12),         # pLo, pCnt off the 2-row blocks
                                       (40, 72, -4, 0, 72), (40, 72, 0, -1, 4)]:
        refused(K, K.vsr_launch_decode_out_rows, ptr(y), ldy, pix_, 3, ptr(fi), ptr(first), ptr(comp), None, None, blkW, pLo, pCnt)
    _KEEP.clear()
    assert bool((comp == float(SENT)).all())


# =====================================================================================================================================
# 4. k_norm_im2col_s2 through vsr_launch_norm_im2col_fmt
# =====================================================================================================================================
def _norm_im2col(K, img, mask, premask, out_split):
    n, ih, iw, _ = img.shape
    rows = n * (ih // 2) * (iw // 2)
    before = np.full(rows * 32 + 64, SENT, np.float32)
    dimg, dmask, dout = dev(img), (dev(mask) if mask is not None else None), torch.from_numpy(before).cuda()
    if out_split:
        aligned128(dout)
    launch(K.vsr_launch_norm_im2col_fmt, ptr(dimg), ih, iw, n, ptr(dout), premask, ptr(dmask) if mask is not None else None, out_split)
    got = dout.cpu().numpy()
    assert np.all(got[rows * 32:] == SENT), "cells behind the last row were written"
    return got[:rows * 32]


def _check_norm_im2col(got, img, mask, out_split, what):
    ref64 = R.norm_im2col_ref(img, mask)
    ref32 = R.norm_im2col_ref(img, mask, np.float32)
    if out_split:
        # 2^-22 relative of the fp32 value, no floor: hi = fp16(v) leaves r = v - hi <= 2^-11 |v|, lo = fp16(r) leaves 2^-11 |r|; below
        # 1/8, where r is an fp16 subnormal, v is a multiple of 2^-24 (the exact last subtraction of (u / 255) * 2 - 1) and so is r
        vals = R.split_decode(got, np.arange(got.size)).reshape(ref32.shape)
        ratio(f"{what} split-format vs fp32", np.abs(vals - ref32.astype(np.float64)), 2.0 ** -22 * np.abs(ref32.astype(np.float64)))
        want = ref32.reshape(-1).copy()
        R.to_split_whole(want)
        assert same_bits(got, want), f"{what}: not the split-format image of the fp32 values"
    else:
        assert same_bits(got.reshape(ref32.shape) + np.float32(0.0), ref32 + np.float32(0.0)), f"{what}: differs from float32(u) / 255, * 2, - 1"
        # |.| <= 1: the quotient rounds once (u), doubling is exact, the difference rounds once (u / 2 at most below 1): 3u covers it
        ratio(f"{what} vs float64", np.abs(got.reshape(ref64.shape).astype(np.float64) - ref64), 3 * U32)


@pytest.mark.parametrize("ih,iw,n", [(2, 2, 1), (4, 6, 2), (5, 7, 1), (6, 10, 3)])
@pytest.mark.parametrize("out_split", [0, 1], ids=["fp32", "split"])
def test_norm_im2col(K, ih, iw, n, out_split):
    rng = np.random.default_rng(400 + ih + iw)
    img = rng.integers(0, 256, size=(n, ih, iw, 3), dtype=np.uint8)
    img.reshape(-1)[:4] = (0, 255, 127, 128)
    got = _norm_im2col(K, img, None, 0, out_split)
    _check_norm_im2col(got, img, None, out_split, f"norm_im2col {ih}x{iw} n{n}")


@pytest.mark.parametrize("premask", [1, 0])
def test_norm_im2col_premask(K, premask):
    """premask = 1: a pixel whose mask is >= 128 counts as 0 (127 keeps it), each frame under its own mask; premask = 0 ignores a
    mask that is handed over"""
    rng = np.random.default_rng(420)
    n, ih, iw = 3, 6, 10
    img = rng.integers(0, 256, size=(n, ih, iw, 3), dtype=np.uint8)
    mask = rng.choice(np.array([0, 127, 128, 255], np.uint8), size=(n, ih, iw))
    assert all(not np.array_equal(mask[a], mask[b]) for a in range(n) for b in range(a))
    assert ((mask == 127).sum() > 5) and ((mask == 128).sum() > 5)
    got = _norm_im2col(K, img, mask, premask, 0)
    _check_norm_im2col(got, img, mask if premask else None, 0, f"norm_im2col premask{premask}")
    assert not np.array_equal(R.norm_im2col_ref(img, mask), R.norm_im2col_ref(img))


# =====================================================================================================================================
# 5. k_reduce_scatter through vsr_launch_reduce_scatter_fmt
# =====================================================================================================================================
def _reduce_scatter(K, rng, M, N, ns, out_split, with_lsum, what):
    ncc = N // 32
    gap = 40                                                  # sentinel floats between the planes
    stride = M * N + gap
    part = rng.standard_normal((ns, M, N)).astype(np.float32)
    phys = np.full(ns * stride, R.HALO_POISON, np.float32)
    for s in range(ns):
        phys[s * stride:s * stride + M * N] = part[s].reshape(-1)
    colC = (rng.permutation(ncc + 2)[:ncc] * 32).astype(np.int32)
    rowC = (rng.permutation(M + 3)[:M] * ((ncc + 2) * 32)).astype(np.int32)
    before = np.full((M + 3) * (ncc + 2) * 32, SENT, np.float32)
    ldL = M + 3
    lsum = R.lsum_planes(rng, ns, M, ldL) if with_lsum else None
    dpart, drow, dcol, dout = dev(phys), dev(rowC), dev(colC), torch.from_numpy(before).cuda()
    dl = dev(lsum) if with_lsum else None
    if out_split:
        aligned128(dout)
    launch(K.vsr_launch_reduce_scatter_fmt, ptr(dpart), ns, stride, M, N, ptr(drow), ptr(dcol), ptr(dout), out_split,
           ptr(dl) if with_lsum else None, ldL if with_lsum else 0)
    got = dout.cpu().numpy()
    cells = R.scatter_cells(rowC, colC, N)
    ref, mag = R.reduce_scatter_ref(part, lsum[:, :M] if with_lsum else None)
    if out_split:
        assert R.split_untouched(got, before, cells), f"{what}: cells outside the scatter were written"
        vals = R.split_decode(got, cells)
    else:
        untouched = np.ones(got.size, dtype=bool)
        untouched[cells.reshape(-1)] = False
        assert np.all(got[untouched] == SENT), f"{what}: cells outside the scatter were written"
        vals = got[cells].astype(np.float64)
    assert np.isfinite(vals).all(), f"{what}: the gap between the planes or the tail of lsum was read"
    ratio(what, np.abs(vals - ref), R.reduce_scatter_bound(ref, mag, ns, with_lsum, out_split))       # derived there
    if ns == 1 and not with_lsum and not out_split:
        assert same_bits(got[cells], part[0]), f"{what}: one plane is a copy"


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("N", [32, 96])
@pytest.mark.parametrize("ns", [1, 2, 5])
@pytest.mark.parametrize("out_split", [0, 1], ids=["fp32", "split"])
@pytest.mark.parametrize("with_lsum", [0, 1], ids=["plain", "lsum"])
def test_reduce_scatter(K, M, N, ns, out_split, with_lsum):
    """float64 sum of the planes (splitStride > M N, 1e30 between them), divided by the float64 sum of the lsum planes (ldL > M, row
    sums over 2^-10 .. 2^10), scattered through permuted, gapped row and chunk tables"""
    rng = np.random.default_rng(500 + 7 * M + N + 3 * ns)
    _reduce_scatter(K, rng, M, N, ns, out_split, with_lsum, f"reduce_scatter {M}x{N} ns{ns} split{out_split} lsum{with_lsum}")


def test_reduce_scatter_refusals(K):
    part, tab = dev(np.zeros(5 * 96, np.float32)), dev(np.zeros(8, np.int32))
    out = torch.full((5 * 96,), float(SENT), device="cuda")
    for N, out_split in [(6, 0), (3, 0), (33, 0), (36, 1), (16, 1), (4, 1)]:               # N % 4; split and N % 32
        refused(K, K.vsr_launch_reduce_scatter_fmt, ptr(part), 1, 5 * 96, 5, N, ptr(tab), ptr(tab), ptr(out), out_split, None, 0)
    _KEEP.clear()
    assert bool((out == float(SENT)).all())


# =====================================================================================================================================
# 6. k_resize_u8: bit-exact with cv2_restate.resize_linear
# =====================================================================================================================================
def _resize(K, rng, sw, sh, dw, dh, ch, frame_idx, nsrc, row_gap, shared_source=False):
    """frame_idx None: the n = nsrc source frames in order; shared_source: srcFrameStride = 0 (every output frame reads frame 0)"""
    row_stride = sw * ch + row_gap
    frames = rng.integers(0, 256, size=(nsrc, sh + 2, row_stride), dtype=np.uint8)          # a row above and below the strip
    n = len(frame_idx) if frame_idx is not None else nsrc
    xo, xa, _ = R.lib_tables(K, sw, dw, 1)               # the clamp flags of the engine's strip tables
    yo, ya, _ = R.lib_tables(K, sh, dh, 0)
    tail = 32
    dsrc, ddst = dev(frames), torch.full((n * dh * dw * ch + tail,), SENT_U8, dtype=torch.uint8, device="cuda")
    dt = [dev(t) for t in (xo, xa, yo, ya)]
    dfi = dev(np.asarray(frame_idx, np.int32)) if frame_idx is not None else None
    launch(K.vsr_launch_resize_u8, ptr(dsrc, row_stride), 0 if shared_source else frames[0].size, row_stride, sw, sh, ptr(ddst), dw, dh, n, ch,
           ptr(dfi) if dfi is not None else None, *[ptr(t) for t in dt])
    got = ddst.cpu().numpy()
    assert np.all(got[n * dh * dw * ch:] == SENT_U8), "bytes behind the last frame were written"
    got = got[:n * dh * dw * ch].reshape(n, dh, dw, ch)
    for o in range(n):
        f = 0 if shared_source else (frame_idx[o] if frame_idx is not None else o)
        strip = frames[f, 1:1 + sh, :sw * ch].reshape(sh, sw, ch)
        ref = cv2r.resize_linear(strip, (dw, dh))
        assert np.array_equal(got[o], ref.reshape(dh, dw, ch)), f"output frame {o} (source {f}): {int((got[o] != ref.reshape(dh, dw, ch)).sum())} bytes differ"


RESIZE = [(3, 2, 2, 1), (7, 5, 3, 2), (5, 3, 13, 7), (6, 4, 6, 4)]


@pytest.mark.parametrize("sw,sh,dw,dh", RESIZE, ids=[f"{a}x{b}-to-{c}x{d}" for a, b, c, d in RESIZE])
@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("how", ["in-order", "gathered", "shared-source"])
def test_resize_u8(K, sw, sh, dw, dh, ch, how):
    """tiny strips down, up and at identity, both channel counts; frameIdx NULL / permuted with a repeat, a row stride beyond the
    strip's width, frame stride 0"""
    rng = np.random.default_rng(600 + sw + dw + ch)
    if how == "in-order":
        _resize(K, rng, sw, sh, dw, dh, ch, None, 3, 0)
    elif how == "gathered":
        _resize(K, rng, sw, sh, dw, dh, ch, [2, 0, 2, 1], 3, 7)
    else:
        _resize(K, rng, sw, sh, dw, dh, ch, None, 3, 5, shared_source=True)


# =====================================================================================================================================
# 7. k_upscale_blend: bit-exact with STTNInpaintOracle.blend_strip
# =====================================================================================================================================
BLEND = [(6, 4, 13, 7), (4, 2, 4, 2)]


@pytest.mark.parametrize("mw,mh,W,sh", BLEND, ids=[f"{a}x{b}-to-{c}x{d}" for a, b, c, d in BLEND])
@pytest.mark.parametrize("is_float", [[0, 1], [1, 0]], ids=["u8-float", "float-u8"])
@pytest.mark.parametrize("masked", [0, 1], ids=["whole-strip", "masked"])
@pytest.mark.parametrize("gather", [0, 1], ids=["in-order", "frameIdx20"])
def test_upscale_blend(K, mw, mh, W, sh, is_float, masked, gather):
    """u8 and float comps in one launch (the float frames hold multiples of 1/4), frameIdx [2, 0] into three frames or NULL, mask
    NULL (sttn-det: the whole strip) or with a row stride of W + 5, rows 3W + 9 bytes apart and a gap between the frames; the
    frame no slot names, the row gaps and the rows outside the strip keep every byte"""
    rng = np.random.default_rng(700 + mw + W + masked)
    n, nfr = 2, 3
    row_stride, rows_alloc = 3 * W + 9, sh + 3
    frame_stride = rows_alloc * row_stride + 11
    buf = rng.integers(0, 256, size=nfr * frame_stride, dtype=np.uint8)
    comp = rng.integers(0, 256, size=(n, mh, mw, 3)).astype(np.float32)
    for f in range(n):
        if is_float[f]:
            comp[f] = (rng.integers(0, 1021, size=(mh, mw, 3)) / 4.0).astype(np.float32)
            assert (comp[f] % 1 != 0).any()
    mrs = W + 5
    mask = np.zeros((sh, mrs), np.uint8)
    mask[:, :W] = rng.random((sh, W)) < 0.6
    mask[:, W:] = 1                                           # the row gap of the mask must not count
    frame_idx = [2, 0] if gather else None
    xo, xa, xf = R.lib_tables(K, mw, W, 1)
    yo, ya, yf = R.lib_tables(K, mh, sh, 0)
    dt = [dev(t) for t in (xo, xa, xf, yo, ya, yf)]
    dcomp, disf, dbuf = dev(comp), dev(np.asarray(is_float, np.int32)), torch.from_numpy(buf.copy()).cuda()
    dmask = dev(mask) if masked else None
    dfi = dev(np.asarray(frame_idx, np.int32)) if gather else None
    ymin = 2                                                   # the strip starts two rows into each frame
    launch(K.vsr_launch_upscale_blend, ptr(dcomp), mw, mh, ptr(disf), ptr(dbuf, ymin * row_stride), frame_stride, row_stride,
           ptr(dfi) if gather else None, ptr(dmask) if masked else None, mrs, W, sh, n, *[ptr(t) for t in dt])
    got = dbuf.cpu().numpy()
    want = buf.copy()
    for f in range(n):
        fd = frame_idx[f] if gather else f
        rows = want[fd * frame_stride:fd * frame_stride + rows_alloc * row_stride].reshape(rows_alloc, row_stride)
        strip = rows[ymin:ymin + sh, :3 * W].reshape(sh, W, 3)
        rows[ymin:ymin + sh, :3 * W] = R.blend_ref(strip, comp[f], bool(is_float[f]), mask[:, :W] if masked else None).reshape(sh, 3 * W)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:6]} (frame stride {frame_stride}, row stride {row_stride})"
    assert not np.array_equal(want, buf)


# =====================================================================================================================================
# 8. converters, and the second trip of every grid-stride loop
# =====================================================================================================================================
@pytest.mark.parametrize("n", [32, 64])
def test_to_split(K, n):
    rng = np.random.default_rng(800 + n)
    x = R.to_split_values(rng, n)
    before = np.full(n + 32, SENT, np.float32)
    dx, dout = aligned128(dev(x)), aligned128(torch.from_numpy(before).cuda())
    launch(K.vsr_launch_to_split, ptr(dx), ptr(dout), n)
    want = before.copy()
    want[:n] = R.to_split_whole(x.copy())
    assert same_bits(dout.cpu().numpy(), want)
    for bad in (31, 33, 48):
        refused(K, K.vsr_launch_to_split, ptr(dx), ptr(dout), bad)
    assert same_bits(dout.cpu().numpy(), want)


@pytest.mark.parametrize("ld", [32, 96])
def test_kn_to_nk_split(K, ld):
    rng = np.random.default_rng(810 + ld)
    Kk = N = 32
    rowB = (rng.permutation(Kk + 3)[:Kk] * 96).astype(np.int32)
    colB = np.array([32], np.int32)
    src = rng.integers(0, 2 ** 32, size=(Kk + 3) * 96, dtype=np.uint32)
    before = np.full(N * ld + 32, SENT, np.float32)
    dsrc, dout = aligned128(dev(src.view(np.float32))), aligned128(torch.from_numpy(before).cuda())
    drow, dcol = dev(rowB), dev(colB)
    launch(K.vsr_launch_kn_to_nk_split, ptr(dsrc), ptr(drow), ptr(dcol), Kk, N, ld, ptr(dout))
    want = R.kn_to_nk_ref(src.view(np.uint16), rowB, colB, Kk, N, ld, before.view(np.uint16))
    assert np.array_equal(dout.cpu().numpy().view(np.uint16), want)
    for k_, n_, ld_ in [(31, 32, 96), (32, 48, 96), (64, 32, 32)]:                 # K % 32, N % 32, ld < K
        refused(K, K.vsr_launch_kn_to_nk_split, ptr(dsrc), ptr(drow), ptr(dcol), k_, n_, ld_, ptr(dout))
    assert np.array_equal(dout.cpu().numpy().view(np.uint16), want)


# Just over 4096 x 256 = 1 048 576 work items: the launchers cap the grid there, so the last items are a second trip of the grid-stride
# loop.  The totals are no multiple of 256 or of a row; everything is compared.
def test_second_trip_resize_u8(K):
    assert 1031 * 1021 > 1048576 and (1031 * 1021) % 256
    _resize(K, np.random.default_rng(900), 37, 29, 1031, 1021, 3, None, 1, 3)


def test_second_trip_norm_im2col(K):
    ih, iw = 726, 730
    assert (ih // 2) * (iw // 2) * 8 > 1048576 and ((ih // 2) * (iw // 2) * 8) % 256
    img = np.random.default_rng(901).integers(0, 256, size=(1, ih, iw, 3), dtype=np.uint8)
    _check_norm_im2col(_norm_im2col(K, img, None, 0, 0), img, None, 0, "norm_im2col 726x730")


def test_second_trip_decode_out(K):
    rows, W = 2, 525_001
    assert rows * W > 1048576 and (rows * W) % 256
    frame_idx, first = [1], [0]
    got, comp0, s, _, _ = _decode(K, np.random.default_rng(902), rows, W, 0, 4, frame_idx, first, 2, "u8", 0, rows * W)
    _decode_check(got, comp0, s, frame_idx, first, 0, rows * W, None, None, "decode 1 050 002 pixels")


def test_second_trip_reduce_scatter(K):
    M, N = 4100, 1056
    assert M * N // 4 > 1048576 and (M * N // 4) % 256
    _reduce_scatter(K, np.random.default_rng(903), M, N, 2, 0, 1, "reduce_scatter 4100x1056 ns2 lsum")


def test_second_trip_to_split(K):
    n = 32 * 131_101
    assert n // 4 > 1048576 and (n // 4) % 256
    x = R.to_split_values(np.random.default_rng(904), n)
    before = np.full(n + 32, SENT, np.float32)
    dx, dout = aligned128(dev(x)), aligned128(torch.from_numpy(before).cuda())
    launch(K.vsr_launch_to_split, ptr(dx), ptr(dout), n)
    want = before.copy()
    want[:n] = R.to_split_whole(x.copy())
    assert same_bits(dout.cpu().numpy(), want)
