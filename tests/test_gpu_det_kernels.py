"""The text detector's forward kernels (csrc/det_kernels.hip) one launch at a time against float64 references.

Every vsr_det_launch_* of the forward pass is called alone through vsr_amd._lib (ccl and db_boxes have their tests in
tests/test_gpu_ocr_det.py), in the forms include/vsr_hip.h documents and not only the ones the two shipped programs compile to:
asymmetric padding, kh != kw, bias and activation on the direct conv, Cout % 8 != 0, N > 1, the depthwise direct and transposed
convs, all eight binary forms, views with halos, channel slices and gaps.

Conventions (those of tests/test_gpu_flow_kernels.py): every output buffer, and every buffer a view points into, is filled with a
sentinel; one launch; the WHOLE buffer is compared, so a cell outside the documented store set must still hold the sentinel bit for
bit.  A reference restates the operation (torch.nn.functional in float64, np.pad, repeat), never the kernel's loop.

Bars.  Pure data movement is bit-equal.  An arithmetic kernel gets a per-element bound derived next to its assertion:
a K-term fp32 sum of products with separate multiply and add (the file is compiled with fp contract off) is within
(K + e) * 2^-24 * S of the exact value, S being the same operation on the absolute values of inputs, weights, bias and residual and e
the roundings of the epilogue.  Sigmoid's bar is calibrated inside the test by the float32 numpy statement of the same formula.  Every
case prints its error beside its bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _det_bounds import SENT, U32, act_ref_bound, hswish_exact_input, sigmoid_ref_bar  # noqa: E402

ERR_ARG = -1            # VSR_ERR_ARG


@pytest.fixture(scope="module")
def L(built_lib, gpu_device):
    assert built_lib.VSR_ERR_ARG == ERR_ARG
    return built_lib.lib


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
_KEEP = []         # device tensors of the next launch (a pointer into a temporary would be handed to the next allocation at once)


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


def sent(n, extra=64):
    """an output buffer of n floats and `extra` more behind them, all sentinel"""
    t = torch.full((int(n) + extra,), SENT, dtype=torch.float32, device="cuda")
    _KEEP.append(t)
    return t


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + int(off) * t.element_size()) if t is not None else None


def launch(fn, *args, rc=0):
    got = fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert got == rc, f"{fn.__name__} returned {got}, expected {rc}"


def host(t):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    _KEEP.clear()
    return a


def expected(size, extra=64):
    return np.full(int(size) + extra, SENT, np.float32)


def bits_equal(what, got, want):
    """bit for bit over the whole buffer (the sentinel cells included)"""
    want = np.ascontiguousarray(want, dtype=np.float32).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print(f"{what}: {got.size} cells, {bad.size} differ (bit-equal required)")
    assert bad.size == 0, f"{what}: {bad.size} cells differ, first at {bad[0]}: got {got[bad[0]]!r} want {want[bad[0]]!r}"


def within(what, got, ref, bound, idx=None):
    """|got - ref| <= bound per element on the cells idx of the buffer (all cells when None); every other cell holds the sentinel"""
    got = got.reshape(-1)
    if idx is not None:
        idx = np.asarray(idx).reshape(-1)
        rest = np.ones(got.size, bool)
        rest[idx] = False
        stray = np.flatnonzero(rest & (got.view(np.uint32) != np.float32(SENT).view(np.uint32)))
        assert stray.size == 0, f"{what}: {stray.size} cells outside the store set were written, first at {stray[0]}: {got[stray[0]]!r}"
        got = got[idx]
    ref, bound = np.asarray(ref, np.float64).reshape(-1), np.broadcast_to(np.asarray(bound, np.float64), np.shape(ref)).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = np.abs(got.astype(np.float64) - ref)
    k = int(np.argmax(err - bound))
    print(f"{what}: max err {err.max():.3e} (bound there {bound[int(np.argmax(err))]:.3e}); tightest cell err {err[k]:.3e} bound {bound[k]:.3e}")
    assert err[k] <= bound[k], f"{what}: cell {k}: got {got[k]!r} ref {ref[k]!r} err {err[k]:.3e} > bound {bound[k]:.3e}"


def vidx(off, n, H, W, Cc, img, row, cs):
    """flat indices [n][H][W][Cc] of a view"""
    return (off + np.arange(n, dtype=np.int64)[:, None, None, None] * img + np.arange(H, dtype=np.int64)[None, :, None, None] * row
            + np.arange(W, dtype=np.int64)[None, None, :, None] * cs + np.arange(Cc, dtype=np.int64)[None, None, None, :])


class ViewBuf:
    """a haloed NHWC buffer [n][H + 2 hy][W + 2 hx][Cs] (+ `gap` floats between images) and the view at channel c0 of its interior"""

    def __init__(self, n, H, W, Cs, c0, halo, gap=0, fill=SENT):
        hy, hx = halo
        self.n, self.H, self.W, self.Cs, self.c0 = n, H, W, Cs, c0
        self.row = (W + 2 * hx) * Cs
        self.img = (H + 2 * hy) * self.row + gap
        self.off = hy * self.row + hx * Cs + c0
        self.a = np.full(n * self.img, fill, np.float32)

    def idx(self, Cc):
        return vidx(self.off, self.n, self.H, self.W, Cc, self.img, self.row, self.Cs)

    def put(self, x_nhwc):
        self.a[self.idx(x_nhwc.shape[-1])] = x_nhwc
        return self


def rnd(seed, *shape, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# =====================================================================================================================================
# conv2d: dense (k_det_conv<8>) and depthwise (k_det_dwconv)
# =====================================================================================================================================
def _conv_ref(x, w, bias, sh, sw, pt, pl, Ho, Wo, groups):
    """F.conv2d in float64 with the launcher's padding: (pt, pl) before, whatever Ho x Wo needs after (zero) -- value and S"""
    H, W = x.shape[2:]
    kh, kw = w.shape[2:]
    pb, pr = max(0, (Ho - 1) * sh + kh - pt - H), max(0, (Wo - 1) * sw + kw - pl - W)

    def run(x_, w_, b_):
        y = F.conv2d(F.pad(t64(x_), (pl, pr, pt, pb)), t64(w_), None if b_ is None else t64(b_), stride=(sh, sw), groups=groups)
        return y[:, :, :Ho, :Wo].numpy()
    return run(x, w, bias), run(np.abs(x), np.abs(w), None if bias is None else np.abs(bias))


CONV_CASES = [
    # N, Cin, H, W, Cout, kh, kw, sh, sw, pt, pl, Ho, Wo, bias, act
    (2, 3, 17, 19, 13, 3, 3, 1, 1, 1, 1, 17, 19, True, 2),     # CO = 8 tail, blockIdx.z, 323 pixels: two blocks, the second partial
    (1, 5, 9, 11, 3, 3, 3, 2, 2, 0, 0, 5, 6, False, 1),        # "SAME" padding only at the bottom and right: the window overhangs
    (1, 4, 7, 5, 8, 9, 9, 1, 1, 4, 4, 7, 5, True, 0),          # the kernel is larger than the map
    (1, 2, 6, 10, 9, 1, 3, 2, 1, 0, 1, 3, 10, False, 2),       # kh != kw, asymmetric padding and stride
    (1, 2, 6, 10, 9, 3, 1, 1, 2, 1, 0, 6, 5, True, 1),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "N%d_Cin%d_%dx%d_Cout%d_k%dx%d_s%d%d_p%d%d_o%dx%d_b%d_a%d" % c)
def test_conv2d_dense(L, case):
    N, Cin, H, W, Cout, kh, kw, sh, sw, pt, pl, Ho, Wo, has_bias, act = case
    x, w = rnd(1, N, Cin, H, W), rnd(2, Cout, Cin, kh, kw, scale=2.0 / np.sqrt(Cin * kh * kw))
    bias = rnd(3, Cout) if has_bias else None
    out = sent(N * Cout * Ho * Wo)
    launch(L.vsr_det_launch_conv2d, ptr(dev(x)), ptr(dev(w)), ptr(dev(bias)) if has_bias else None, N, Cin, H, W, Cout, kh, kw, sh, sw, pt, pl,
           Ho, Wo, 0, act, ptr(out))
    pre, S = _conv_ref(x, w, bias, sh, sw, pt, pl, Ho, Wo, 1)
    # K = Cin*kh*kw products, each rounded, added one by one to an accumulator that starts at the bias: K multiplies and K adds, every
    # partial sum bounded by S -> (K + 1) * u * S covers them (the standard gamma_K of a K-term inner product, plus the bias term)
    K = Cin * kh * kw
    ref, bound = act_ref_bound(pre, (K + 1) * U32 * S, S, act)
    within(f"conv2d dense {case}", host(out), ref, bound, np.arange(ref.size))


DW_CASES = [
    # N, C, H, W, k, s, p, Ho, Wo, bias, act
    (2, 5, 7, 9, 3, 1, 1, 7, 9, True, 2),
    (2, 5, 9, 7, 5, 2, 2, 5, 4, False, 1),                     # odd sizes: Ho, Wo are ceils
    (2, 5, 9, 7, 5, 2, 2, 5, 4, True, 0),
]


@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "N%d_C%d_%dx%d_k%d_s%d_p%d_o%dx%d_b%d_a%d" % c)
def test_conv2d_depthwise(L, case):
    N, Cc, H, W, k, s, p, Ho, Wo, has_bias, act = case
    x, w = rnd(4, N, Cc, H, W), rnd(5, Cc, 1, k, k, scale=2.0 / k)
    bias = rnd(6, Cc) if has_bias else None
    out = sent(N * Cc * Ho * Wo)
    launch(L.vsr_det_launch_conv2d, ptr(dev(x)), ptr(dev(w)), ptr(dev(bias)) if has_bias else None, N, Cc, H, W, Cc, k, k, s, s, p, p, Ho, Wo, 1, act,
           ptr(out))
    pre, S = _conv_ref(x, w, bias, s, s, p, p, Ho, Wo, Cc)
    ref, bound = act_ref_bound(pre, (k * k + 1) * U32 * S, S, act)      # as the dense conv with K = k*k taps
    within(f"conv2d depthwise {case}", host(out), ref, bound, np.arange(ref.size))


def test_conv2d_depthwise_refuses_cin_ne_cout(L):
    out = sent(2 * 6 * 7 * 9)
    launch(L.vsr_det_launch_conv2d, ptr(dev(rnd(4, 2, 5, 7, 9))), ptr(dev(rnd(5, 6, 1, 3, 3))), None, 2, 5, 7, 9, 6, 3, 3, 1, 1, 1, 1, 7, 9, 1, 0, ptr(out),
           rc=ERR_ARG)
    bits_equal("depthwise Cin != Cout leaves the output alone", host(out), expected(2 * 6 * 7 * 9))


# =====================================================================================================================================
# deconv2x2 (k_det_deconv2): dense and depthwise
# =====================================================================================================================================
@pytest.mark.parametrize("N,Cin,Cout,H,W,dw", [(2, 5, 3, 3, 5, 0), (2, 6, 6, 3, 5, 1)], ids=["dense", "depthwise"])
def test_deconv2x2(L, N, Cin, Cout, H, W, dw):
    x, w = rnd(7, N, Cin, H, W), rnd(8, Cin, 1 if dw else Cout, 2, 2)
    out = sent(N * Cout * 4 * H * W)
    launch(L.vsr_det_launch_deconv2x2, ptr(dev(x)), ptr(dev(w)), N, Cin, H, W, Cout, dw, ptr(out))
    g = Cin if dw else 1
    ref = F.conv_transpose2d(t64(x), t64(w), stride=2, groups=g).numpy()
    S = F.conv_transpose2d(t64(np.abs(x)), t64(np.abs(w)), stride=2, groups=g).numpy()
    K = 1 if dw else Cin                              # stride = kernel: each output is ONE tap, a K-term sum over the input channels
    within(f"deconv2x2 dw={dw}", host(out), ref, K * U32 * S, np.arange(ref.size))


# =====================================================================================================================================
# binary, affine, unary, the grid-stride second trip
# =====================================================================================================================================
def _bmode_operand(rng, bmode, N, Cc, HW):
    b = rng.standard_normal({0: N * Cc * HW, 1: Cc, 2: N * Cc, 3: 1}[bmode]).astype(np.float32)
    full = {0: lambda: b.reshape(N, Cc, HW), 1: lambda: b.reshape(1, Cc, 1), 2: lambda: b.reshape(N, Cc, 1), 3: lambda: b.reshape(1, 1, 1)}[bmode]()
    return b, np.broadcast_to(full, (N, Cc, HW))


@pytest.mark.parametrize("op", [0, 1], ids=["add", "mul"])
@pytest.mark.parametrize("bmode", [0, 1, 2, 3])
def test_binary(L, op, bmode):
    N, Cc, HW = 2, 3, 35
    rng = np.random.default_rng(10 + bmode)
    a = rng.standard_normal((N, Cc, HW)).astype(np.float32)
    b, bfull = _bmode_operand(rng, bmode, N, Cc, HW)
    out = sent(a.size)
    launch(L.vsr_det_launch_binary, ptr(dev(a)), ptr(dev(b)), op, a.size, Cc, HW, bmode, ptr(out))
    # ONE correctly rounded fp32 operation: the float64 result of two float32 operands (exact for the product, and for the sum of
    # operands this close) rounded to float32 IS the answer -- bit-equal
    r = (a.astype(np.float64) + bfull) if op == 0 else (a.astype(np.float64) * bfull)
    want = expected(a.size)
    want[:a.size] = r.astype(np.float32).reshape(-1)
    bits_equal(f"binary op {op} bmode {bmode}", host(out), want)


def test_affine(L):
    N, Cc, HW = 2, 3, 35
    x, sc, sf = rnd(20, N, Cc, HW), rnd(21, Cc), rnd(22, Cc)
    out = sent(x.size)
    launch(L.vsr_det_launch_affine, ptr(dev(x)), ptr(dev(sc)), ptr(dev(sf)), x.size, Cc, HW, ptr(out))
    ref = x.astype(np.float64) * sc[None, :, None] + sf[None, :, None]
    S = np.abs(x).astype(np.float64) * np.abs(sc)[None, :, None] + np.abs(sf)[None, :, None]
    within("affine", host(out), ref, 2 * U32 * S, np.arange(x.size))      # one multiply and one add: 2 roundings, each <= u * S


def _unary_inputs():
    f = np.float32
    up, dn = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    special = [f(-3), f(3), f(0.0), f(-0.0), up(-3), dn(-3), up(3), dn(3), up(-2.5), dn(-2.5), f(-2.5), f(2.5), up(2.5), dn(2.5), f(100), f(-100),
               f(4), f(5), f(6), f(7), f(12), f(3.5), f(1), f(-1), f(1.5), f(-1.5)]       # integers >= 3: hardswish(v) = v with no rounding at all
    return np.concatenate([np.array(special, np.float32), rnd(30, 230, scale=2.5)])


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4], ids=["relu", "hardswish", "hardsigmoid", "sigmoid", "scale"])
def test_unary(L, kind):
    v = _unary_inputs()
    p0, p1 = (np.float32(0.2), np.float32(0.5)) if kind == 2 else (np.float32(1.7), np.float32(-0.3))     # hardsigmoid: knees at -2.5 and 2.5
    out = sent(v.size)
    launch(L.vsr_det_launch_unary, ptr(dev(v)), v.size, kind, C.c_float(p0), C.c_float(p1), ptr(out))
    got = host(out)
    v64 = v.astype(np.float64)
    idx = np.arange(v.size)
    if kind == 0:                                      # pure selection: the value, bit for bit (relu(-0) may be either zero: compared as a value)
        want = expected(v.size)
        want[:v.size] = np.maximum(v, np.float32(0))
        neg0 = np.flatnonzero(np.signbit(v) & (v == 0))
        assert (got[neg0] == 0).all()
        want[neg0] = got[neg0]
        bits_equal("unary relu", got, want)
    elif kind == 1:
        ref, bound = hswish_exact_input(v)
        within("unary hardswish", got, ref, bound, idx)
        assert got[list(v).index(np.float32(100))] == np.float32(100) and got[list(v).index(np.float32(-100))] == 0
    elif kind in (2, 4):                               # v * p0 + p1: a multiply and an add, 2 roundings of at most u * S; the clip has slope 1
        lin = v64 * float(p0) + float(p1)
        S = np.abs(v64) * abs(float(p0)) + abs(float(p1))
        within(f"unary kind {kind}", got, np.clip(lin, 0.0, 1.0) if kind == 2 else lin, 2 * U32 * S, idx)
        if kind == 2:
            assert got[:v.size].min() == 0.0 and got[:v.size].max() == 1.0
    else:
        ref, bar = sigmoid_ref_bar(v)
        within("unary sigmoid", got, ref, bar, idx)
        lo, hi = got[list(v).index(np.float32(-100))], got[list(v).index(np.float32(100))]
        assert lo == 0.0 and hi == 1.0, f"sigmoid(-100) = {lo!r}, sigmoid(100) = {hi!r}: must saturate to finite 0 and 1"


SECOND_TRIP = 2_097_152 + 300       # grid_for caps the grid at 8192 blocks of 256: element 2,097,152 is the first of a second trip


def test_grid_stride_second_trip_unary(L):
    v = rnd(40, SECOND_TRIP)
    out = sent(v.size)
    launch(L.vsr_det_launch_unary, ptr(dev(v)), v.size, 0, C.c_float(0), C.c_float(0), ptr(out))
    want = expected(v.size)
    want[:v.size] = np.maximum(v, np.float32(0))
    bits_equal("unary relu, second trip", host(out), want)


def test_grid_stride_second_trip_binary(L):
    Cc, HW = 7, 1000
    a, b = rnd(41, SECOND_TRIP), rnd(42, Cc)
    out = sent(a.size)
    launch(L.vsr_det_launch_binary, ptr(dev(a)), ptr(dev(b)), 0, a.size, Cc, HW, 1, ptr(out))
    want = expected(a.size)
    want[:a.size] = (a.astype(np.float64) + b[(np.arange(a.size) // HW) % Cc]).astype(np.float32)     # one correctly rounded add (test_binary)
    bits_equal("binary add per channel, second trip", host(out), want)


# =====================================================================================================================================
# gap, maxpool, nearest, normalize, copy
# =====================================================================================================================================
@pytest.mark.parametrize("HW", [1, 63, 64, 65, 1000])
def test_gap(L, HW):
    planes = 5                                         # four planes per block: the second block is partial
    x = rnd(50 + HW, planes, HW) + np.float32(0.5)
    out = sent(planes)
    launch(L.vsr_det_launch_gap, ptr(dev(x)), planes, HW, ptr(out))
    ref, S = x.astype(np.float64).mean(axis=1), np.abs(x).astype(np.float64).mean(axis=1)
    # a sum of HW numbers in any order is within (HW - 1) * u * sum|x| of the exact sum; the divide is one more rounding: HW * u * S
    within(f"gap HW={HW}", host(out), ref, HW * U32 * S, np.arange(planes))


@pytest.mark.parametrize("H,W,k,s,pt,pl,Ho,Wo", [(5, 7, 2, 1, 0, 0, 5, 7), (7, 9, 3, 2, 1, 1, 4, 5)], ids=["2x2_s1_overhang", "3x3_s2_p1"])
def test_maxpool(L, H, W, k, s, pt, pl, Ho, Wo):
    planes = 3
    x = -np.abs(rnd(60, planes, H, W)) - np.float32(0.25)          # all negative: padding with 0 instead of -inf would win every border window
    out = sent(planes * Ho * Wo)
    launch(L.vsr_det_launch_maxpool, ptr(dev(x)), planes, H, W, k, k, s, s, pt, pl, Ho, Wo, ptr(out))
    pb, pr = max(0, (Ho - 1) * s + k - pt - H), max(0, (Wo - 1) * s + k - pl - W)
    y = F.max_pool2d(F.pad(torch.from_numpy(x)[None], (pl, pr, pt, pb), value=float("-inf")), k, stride=s)[0, :, :Ho, :Wo].numpy()
    want = expected(planes * Ho * Wo)
    want[:y.size] = y.reshape(-1)
    bits_equal(f"maxpool {k}x{k} s{s}", host(out), want)


@pytest.mark.parametrize("s", [2, 3])
def test_nearest(L, s):
    planes, H, W = 4, 3, 5
    x = rnd(61, planes, H, W)
    out = sent(x.size * s * s)
    launch(L.vsr_det_launch_nearest, ptr(dev(x)), planes, H, W, s, ptr(out))
    want = expected(x.size * s * s)
    want[:x.size * s * s] = x.repeat(s, axis=1).repeat(s, axis=2).reshape(-1)
    bits_equal(f"nearest s={s}", host(out), want)


def test_normalize(L):
    H, W = 7, 111                                      # 777 pixels: four blocks, the last partial; every byte value in every channel
    rng = np.random.default_rng(62)
    img = np.stack([rng.permutation(np.arange(H * W) % 256) for _ in range(3)], axis=-1).astype(np.uint8).reshape(H, W, 3)
    assert all(len(np.unique(img[..., c])) == 256 for c in range(3))
    out = sent(3 * H * W)
    launch(L.vsr_det_launch_normalize, ptr(dev(img)), H, W, ptr(out))
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    b = img.astype(np.float64).transpose(2, 0, 1)
    ref = (b / 255.0 - mean[:, None, None]) / std[:, None, None]
    S = (b / 255.0 + mean[:, None, None]) / std[:, None, None]
    # (byte * (1/255) - mean) / std in fp32: three constants rounded to fp32 (1/255, mean, std) and three operations (multiply, subtract,
    # divide), each a relative 2^-24 of a quantity bounded by S: 6 * u * S
    within("normalize", host(out), ref, 6 * U32 * S, np.arange(ref.size))


def test_copy(L):
    width, sp, dp, rows = 13, 16, 20, 3                # 52 bytes a row, pitches 64 and 80 bytes
    src = rnd(63, rows * sp)
    dst = sent(rows * dp)
    launch(L.vsr_det_launch_copy, ptr(dev(src)), 4 * sp, ptr(dst), 4 * dp, 4 * width, rows)
    want = expected(rows * dp)
    for r in range(rows):
        want[r * dp:r * dp + width] = src[r * sp:r * sp + width]
    bits_equal("copy", host(dst), want)
    dst, s = sent(rows * dp), dev(src)
    for args in [(None, 4 * sp, ptr(dst), 4 * dp, 4 * width, rows), (ptr(s), 4 * sp, None, 4 * dp, 4 * width, rows),
                 (ptr(s), 4 * sp, ptr(dst), 4 * dp, -4, rows), (ptr(s), 4 * sp, ptr(dst), 4 * dp, 4 * width, -1),
                 (ptr(s), 4 * width - 4, ptr(dst), 4 * dp, 4 * width, rows), (ptr(s), 4 * sp, ptr(dst), 4 * width - 4, 4 * width, rows)]:
        launch(L.vsr_det_launch_copy, *args, rc=ERR_ARG)
    launch(L.vsr_det_launch_copy, ptr(s), 4 * sp, ptr(dst), 4 * dp, 0, rows)                 # nothing to copy: accepted, nothing written
    bits_equal("copy refusals leave the destination alone", host(dst), expected(rows * dp))


# =====================================================================================================================================
# layout kernels around the GEMM convs
# =====================================================================================================================================
@pytest.mark.parametrize("Cc,Cp", [(5, 32), (40, 64)])
def test_nchw_to_nhwc(L, Cc, Cp):
    n, H, W, pt, pl, Hp, Wp = 2, 5, 7, 2, 1, 10, 10
    x = rnd(70, n, Cc, H, W)
    out = sent(n * Hp * Wp * Cp)
    launch(L.vsr_det_launch_nchw_to_nhwc, ptr(dev(x)), n, Cc, H, W, pt, pl, Hp, Wp, Cp, ptr(out))
    ref = np.zeros((n, Hp, Wp, Cp), np.float32)        # the WHOLE padded image is written: zero padding and zero channels included
    ref[:, pt:pt + H, pl:pl + W, :Cc] = x.transpose(0, 2, 3, 1)
    want = expected(ref.size)
    want[:ref.size] = ref.reshape(-1)
    bits_equal(f"nchw_to_nhwc C={Cc}", host(out), want)


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_nhwc_to_nchw(L, affine, act):
    n, Cc, Np, P = 2, 40, 64, 37
    x = rnd(71, n, P, Np, scale=2.5)
    x[0, :12, :3] = np.array([3, 4, 5, 6, 7, 12, -3, -4, 2.5, 1.5, 100, -100], np.float32)[:, None]     # hardswish without a rounding
    sc, sf = rnd(72, Cc), rnd(73, Cc)
    out = sent(n * Cc * P)
    launch(L.vsr_det_launch_nhwc_to_nchw, ptr(dev(x)), n, Cc, P, Np, ptr(dev(sc)) if affine else None, ptr(dev(sf)) if affine else None, act, ptr(out))
    got = host(out)
    v = np.ascontiguousarray(x[:, :, :Cc].transpose(0, 2, 1))               # [n][C][P]
    if not affine and act in (0, 1):
        want = expected(v.size)
        want[:v.size] = (v if act == 0 else np.maximum(v, np.float32(0))).reshape(-1)
        bits_equal(f"nhwc_to_nchw act {act}", got, want)
    elif not affine:
        ref, bound = hswish_exact_input(v)
        within("nhwc_to_nchw hardswish", got, ref, bound, np.arange(v.size))
    else:
        pre = v.astype(np.float64) * sc[None, :, None] + sf[None, :, None]
        S = np.abs(v).astype(np.float64) * np.abs(sc)[None, :, None] + np.abs(sf)[None, :, None]
        ref, bound = act_ref_bound(pre, 2 * U32 * S, S, act)                   # multiply and add: 2 roundings of at most u * S
        within(f"nhwc_to_nchw affine act {act}", got, ref, bound, np.arange(v.size))


def test_nhwc_to_nchw_refusals(L):
    n, Cc, Np, P = 2, 40, 64, 37
    x, sc, out = dev(rnd(71, n, P, Np)), dev(rnd(72, Cc)), sent(n * Cc * P)
    for args in [(None, n, Cc, P, Np, None, None, 0, ptr(out)), (ptr(x), n, Cc, P, Np, None, None, 0, None), (ptr(x), 0, Cc, P, Np, None, None, 0, ptr(out)),
                 (ptr(x), 65536, Cc, P, Np, None, None, 0, ptr(out)), (ptr(x), n, 0, P, Np, None, None, 0, ptr(out)),
                 (ptr(x), n, Cc, P, Cc - 1, None, None, 0, ptr(out)), (ptr(x), n, Cc, 0, Np, None, None, 0, ptr(out)),
                 (ptr(x), n, Cc, P, Np, ptr(sc), None, 0, ptr(out))]:
        launch(L.vsr_det_launch_nhwc_to_nchw, *args, rc=ERR_ARG)
    bits_equal("nhwc_to_nchw refusals leave the output alone", host(out), expected(n * Cc * P))


# =====================================================================================================================================
# the NHWC-resident plan's view kernels
# =====================================================================================================================================
def test_to_view(L):
    n, Cc, Cw, H, W = 2, 5, 32, 5, 7
    x = rnd(80, n, Cc, H, W)
    vb = ViewBuf(n, H, W, Cs=96, c0=32, halo=(2, 3), gap=192)
    out = dev(vb.a)
    launch(L.vsr_det_launch_to_view, ptr(dev(x)), n, Cc, H, W, Cw, ptr(out, vb.off), vb.img, vb.row, vb.Cs)
    ref = np.zeros((n, H, W, Cw), np.float32)          # channels [5, 32) of the slice become 0
    ref[..., :Cc] = x.transpose(0, 2, 3, 1)
    vb.put(ref)                                        # halo, the other two slices and the gap between the images keep the sentinel
    bits_equal("to_view", host(out), vb.a)


def test_from_view(L):
    n, Cc, H, W = 2, 40, 5, 7
    x = rnd(81, n, H, W, 64)
    vb = ViewBuf(n, H, W, Cs=64, c0=0, halo=(1, 2), gap=64).put(x)
    stride = Cc * H * W + 24
    out = sent(n * stride, extra=0)
    launch(L.vsr_det_launch_from_view, ptr(dev(vb.a), vb.off), vb.img, vb.row, vb.Cs, n, Cc, H, W, ptr(out), stride)
    want = expected(n * stride, extra=0)
    for b in range(n):
        want[b * stride:b * stride + Cc * H * W] = x[b, :, :, :Cc].transpose(2, 0, 1).reshape(-1)
    bits_equal("from_view", host(out), want)


DWV_CASES = [
    # H, W, k, s, p, affine, act
    (5, 7, 3, 1, 1, True, 2),
    (5, 7, 3, 1, 1, False, 0),
    (5, 7, 3, 2, 1, False, 1),
    (7, 9, 5, 2, 2, True, 0),
    (5, 7, 5, 1, 2, False, 2),
    (5, 7, 5, 1, 2, True, 1),
]


@pytest.mark.parametrize("case", DWV_CASES, ids=lambda c: "%dx%d_k%d_s%d_p%d_aff%d_act%d" % c)
def test_dwconv_view(L, case):
    H, W, k, s, p, affine, act = case
    N, Cc = 2, 8
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = rnd(82, N, H, W, Cc)
    w = rnd(83, Cc, 1, k, k, scale=2.0 / k)
    sc, sf = rnd(84, Cc), rnd(85, Cc)
    vin = ViewBuf(N, H, W, Cs=32, c0=4, halo=(3, 3))                      # the halo a tap outside the image reads is zero in the slice's
    vin.a.reshape(N, H + 6, W + 6, 32)[..., 4:12] = 0.0                    # channels; the other channels hold the sentinel: a read outside
    vin.put(x)                                                            # the slice shows as a 7 in the sum
    vout = ViewBuf(N, Ho, Wo, Cs=16, c0=8, halo=(1, 2), gap=48)           # other strides than the input; its halo is sentinel and stays so
    out = dev(vout.a)
    wt = np.ascontiguousarray(w.reshape(Cc, k * k).T)                     # tap-major [kh*kw][C]
    launch(L.vsr_det_launch_dwconv_view, ptr(dev(vin.a), vin.off), vin.img, vin.row, vin.Cs, ptr(dev(wt)), ptr(dev(sc)) if affine else None,
           ptr(dev(sf)) if affine else None, N, Cc, k, k, s, s, p, p, Ho, Wo, act, ptr(out, vout.off), vout.img, vout.row, vout.Cs)
    xc = x.transpose(0, 3, 1, 2)
    acc = F.conv2d(t64(xc), t64(w), stride=s, padding=p, groups=Cc).numpy()
    Sa = F.conv2d(t64(np.abs(xc)), t64(np.abs(w)), stride=s, padding=p, groups=Cc).numpy()
    assert acc.shape == (N, Cc, Ho, Wo)
    K = k * k                                          # K products and K adds from a zero accumulator: K * u * Sa; the affine adds a multiply
    if affine:                                         # and an add, (K + 2) * u * S with S = Sa * |scale| + |shift|
        pre, S = acc * sc[None, :, None, None] + sf[None, :, None, None], Sa * np.abs(sc)[None, :, None, None] + np.abs(sf)[None, :, None, None]
        pre_err = (K + 2) * U32 * S
    else:
        pre, S, pre_err = acc, Sa, K * U32 * Sa
    ref, bound = act_ref_bound(pre, pre_err, S, act)
    within(f"dwconv_view {case}", host(out), ref.transpose(0, 2, 3, 1), bound.transpose(0, 2, 3, 1), vout.idx(Cc))


def test_dwconv_view_refuses_unaligned_slice(L):
    vin = ViewBuf(2, 5, 7, Cs=32, c0=2, halo=(3, 3), fill=0.0)
    vout = ViewBuf(2, 5, 7, Cs=16, c0=8, halo=(1, 2))
    out = dev(vout.a)
    launch(L.vsr_det_launch_dwconv_view, ptr(dev(vin.a), vin.off), vin.img, vin.row, vin.Cs, ptr(dev(rnd(83, 9, 8))), None, None, 2, 8, 3, 3, 1, 1, 1, 1, 5, 7,
           0, ptr(out, vout.off), vout.img, vout.row, vout.Cs, rc=ERR_ARG)
    bits_equal("dwconv_view at c0 = 2 leaves the output alone", host(out), vout.a)


@pytest.mark.parametrize("s", [2, 3])
def test_nearest_view(L, s):
    N, Cc, h, w = 2, 8, 3, 5
    x = rnd(86, N, h, w, Cc)
    vin = ViewBuf(N, h, w, Cs=16, c0=4, halo=(1, 1)).put(x)
    vout = ViewBuf(N, h * s, w * s, Cs=24, c0=8, halo=(1, 2), gap=24)
    out = dev(vout.a)
    launch(L.vsr_det_launch_nearest_view, ptr(dev(vin.a), vin.off), vin.img, vin.row, vin.Cs, N, Cc, h * s, w * s, s, ptr(out, vout.off), vout.img, vout.row,
           vout.Cs)
    vout.put(x.repeat(s, axis=1).repeat(s, axis=2))
    bits_equal(f"nearest_view s={s}", host(out), vout.a)


@pytest.mark.parametrize("Cc,kh,kw,pt,pl", [(1, 3, 3, 1, 1), (3, 3, 3, 1, 1), (2, 4, 4, 1, 2), (2, 3, 5, 1, 2)])
def test_im2col_view(L, Cc, kh, kw, pt, pl):
    N, H, W = 2, 5, 7
    x = rnd(87, N, Cc, H, W)
    vout = ViewBuf(N, H, W, Cs=64, c0=32, halo=(1, 1), gap=64)
    out = dev(vout.a)
    launch(L.vsr_det_launch_im2col_view, ptr(dev(x)), N, Cc, H, W, kh, kw, pt, pl, ptr(out, vout.off), vout.img, vout.row, vout.Cs)
    xp = np.pad(x, ((0, 0), (0, 0), (pt, kh - 1 - pt), (pl, kw - 1 - pl)))
    ref = np.zeros((N, H, W, 32), np.float32)          # channels beyond C*kh*kw are zero
    for c in range(Cc):
        for ky in range(kh):
            for kx in range(kw):
                ref[..., (c * kh + ky) * kw + kx] = xp[:, c, ky:ky + H, kx:kx + W]
    vout.put(ref)
    bits_equal(f"im2col_view C={Cc} {kh}x{kw}", host(out), vout.a)


def test_im2col_view_refuses_33_taps(L):
    vout = ViewBuf(2, 5, 7, Cs=64, c0=32, halo=(1, 1))
    out = dev(vout.a)
    launch(L.vsr_det_launch_im2col_view, ptr(dev(rnd(87, 2, 3, 5, 7))), 2, 3, 5, 7, 1, 11, 0, 5, ptr(out, vout.off), vout.img, vout.row, vout.Cs, rc=ERR_ARG)
    bits_equal("im2col_view with 33 taps leaves the output alone", host(out), vout.a)


def _dots_case(L, N, H, W, Cc, n_out, has_bias, act, seed):
    x = rnd(seed, N, H, W, Cc)
    w = rnd(seed + 1, n_out, Cc, scale=2.0 / np.sqrt(Cc))
    bias = np.array([0.37], np.float32) if has_bias else None
    vin = ViewBuf(N, H, W, Cs=Cc + 8, c0=4, halo=(1, 1)).put(x)           # the channels around the slice hold the sentinel: a read beyond C shows
    out = sent(N * n_out * H * W)
    launch(L.vsr_det_launch_dots_view, ptr(dev(vin.a), vin.off), vin.img, vin.row, vin.Cs, N, Cc, H, W, ptr(dev(w)), ptr(dev(bias)) if has_bias else None,
           n_out, act, ptr(out))
    xc = x.transpose(0, 3, 1, 2)
    b0 = float(bias[0]) if has_bias else 0.0
    if n_out == 1:
        wk = w.reshape(1, Cc, 1, 1)
        pre, S = F.conv2d(t64(xc), t64(wk)).numpy() + b0, F.conv2d(t64(np.abs(xc)), t64(np.abs(wk))).numpy() + abs(b0)
    else:                                              # the four dots are the taps (dy, dx) of a 2x2 / stride 2 transposed conv to one channel
        wk = w.reshape(2, 2, Cc).transpose(2, 0, 1)[:, None]
        pre = F.conv_transpose2d(t64(xc), t64(wk), stride=2).numpy() + b0
        S = F.conv_transpose2d(t64(np.abs(xc)), t64(np.abs(wk)), stride=2).numpy() + abs(b0)
    # C products and C adds in some order (lanes, then a shuffle tree), then the bias: (C + 1) * u * S whatever the order
    pre_err = (Cc + 1) * U32 * S
    if act == 3:                                       # sigmoid has slope at most 1/4; its own evaluation is held to the calibrated bar
        ref, bar = sigmoid_ref_bar(pre.astype(np.float32))
        ref, bound = 1.0 / (1.0 + np.exp(-pre)), 0.25 * pre_err + bar
    else:
        ref, bound = act_ref_bound(pre, pre_err, S, act)
    within(f"dots_view N={N} {H}x{W} C={Cc} n_out={n_out} bias={has_bias} act={act}", host(out), ref, bound, np.arange(ref.size))


@pytest.mark.parametrize("n_out", [1, 4])
@pytest.mark.parametrize("Cc,has_bias,act", [(4, True, 3), (24, False, 0), (64, True, 1), (68, False, 2), (68, True, 3), (24, True, 2)])
def test_dots_view(L, n_out, Cc, has_bias, act):
    _dots_case(L, 2, 5, 7, Cc, n_out, has_bias, act, 90 + Cc)             # 70 pixels: four groups of 16 lanes and a partial one


def test_dots_view_second_round(L):
    _dots_case(L, 1, 363, 362, 4, 1, True, 0, 99)                         # 131406 pixels > 8192 blocks x 16: the `rounds` loop runs twice
