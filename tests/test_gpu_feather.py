"""The two seam-feather kernels through the C-ABI (vsr_feather_alpha, vsr_feather_composite; csrc/feather_kernels.hip) against the numpy
statement (tests/_feather_statement.py): exact equality, unaligned and strided frames, untouched gaps, argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _feather_statement as fs

pytestmark = pytest.mark.gpu

FEATHERS = [1, 2, 3, 8, 64]             # 64 exceeds every half-width of the shapes below: the clip at F
H, W, N = 37, 53, 3                      # W * 3 = 159: no row start but the first is aligned to anything


def P(t):
    return C.c_void_p(t.data_ptr())


def masks(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    out = {"empty": np.zeros((H, W), np.uint8), "full": np.full((H, W), 255, np.uint8)}
    one = np.zeros((H, W), np.uint8)
    one[H // 2, W // 2] = 1
    out["one pixel"] = one
    edge = np.zeros((H, W), np.uint8)
    edge[H // 2:, W // 3:] = 255                                   # touches the bottom and the right frame edge
    out["edge rectangle"] = edge
    two = np.zeros((H, W), np.uint8)
    two[2:max(3, H - 2), 2:W // 2] = 255
    two[2:max(3, H - 2), W // 2 + 1:max(W // 2 + 2, W - 1)] = 7    # one pixel apart; any non-zero value is inside
    out["two rectangles"] = two
    out["random blob"] = (rng.random((H, W)) < 0.97).astype(np.uint8) * 255
    return out


def gpu_alpha(lib, dev, cmask, F):
    h, w = cmask.shape
    c = torch.from_numpy(np.ascontiguousarray(cmask)).to(dev)
    pad = 64
    buf = torch.full((h * w + 2 * pad,), 0xA5, dtype=torch.uint8, device=dev)
    rc = lib.lib.vsr_feather_alpha(P(c), h, w, F, C.c_void_p(buf.data_ptr() + pad), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.last_error()
    got = buf.cpu().numpy()
    assert (got[:pad] == 0xA5).all() and (got[pad + h * w:] == 0xA5).all(), "bytes around alpha were written"
    return got[pad:pad + h * w].reshape(h, w)


@pytest.mark.parametrize("shape", [(H, W), (1, 9), (9, 1)])
@pytest.mark.parametrize("F", FEATHERS)
def test_alpha_equals_the_statement(built_lib, gpu_device, shape, F):
    for name, cmask in masks(*shape).items():
        want = fs.distance_separable(cmask, F)
        got = gpu_alpha(built_lib, gpu_device, cmask, F)
        assert np.array_equal(got, want), f"{name} {shape} F={F}: {int((got != want).sum())} pixels differ"


def test_alpha_more_than_one_tile_each_way(built_lib, gpu_device):
    """the kernel's tile is 32 x 64 pixels with a halo of F - 1 rows: 70 x 150 has three tiles each way and ragged last ones"""
    rng = np.random.default_rng(11)
    cmask = np.full((70, 150), 255, np.uint8)
    cmask[rng.integers(0, 70, 6), rng.integers(0, 150, 6)] = 0
    cmask[31:33, 60:70] = 0
    for F in (8, 64):
        assert np.array_equal(gpu_alpha(built_lib, gpu_device, cmask, F), fs.distance_separable(cmask, F))


def _buffers(dev, fill, src, lead=5, gap=7, src_lead=2, src_gap=13):
    """frames: a slice of a larger tensor (unaligned start `lead`, stride = frame + gap); src: another stride and start"""
    n = fill.shape[0]
    size = fill[0].size
    fstride, sstride = size + gap, size + src_gap
    fbuf = np.full(lead + n * fstride + 32, 0x5A, np.uint8)
    sbuf = np.full(src_lead + n * sstride + 32, 0xC3, np.uint8)
    for f in range(n):
        fbuf[lead + f * fstride:lead + f * fstride + size] = fill[f].ravel()
        sbuf[src_lead + f * sstride:src_lead + f * sstride + size] = src[f].ravel()
    return torch.from_numpy(fbuf).to(dev), torch.from_numpy(sbuf).to(dev), fstride, sstride, fbuf, sbuf


def _composite(lib, dev, fill, src, d, F, **kw):
    n, h, w, _ = fill.shape
    lead, src_lead = kw.get("lead", 5), kw.get("src_lead", 2)
    ft, st, fstride, sstride, fbuf, sbuf = _buffers(dev, fill, src, **kw)
    dt = torch.from_numpy(np.ascontiguousarray(d)).to(dev)
    rc = lib.lib.vsr_feather_composite(C.c_void_p(ft.data_ptr() + lead), fstride, C.c_void_p(st.data_ptr() + src_lead), sstride, P(dt),
                                       n, h, w, F, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.last_error()
    got = ft.cpu().numpy()
    assert np.array_equal(st.cpu().numpy(), sbuf), "src was written"
    size = h * w * 3
    out = np.stack([got[lead + f * fstride:lead + f * fstride + size].reshape(h, w, 3) for f in range(n)])
    untouched = np.ones(got.size, bool)
    for f in range(n):
        untouched[lead + f * fstride:lead + f * fstride + size] = False
    assert np.array_equal(got[untouched], fbuf[untouched]), "bytes in front of, between or behind the frames were written"
    return out


@pytest.fixture(scope="module")
def pixels():
    rng = np.random.default_rng(2024)
    fill = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    src = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    # planted extremes: every (0 | 255, 0 | 255) pair inside the ramp of the masks below
    fill[:, 18:22, 20:24], src[:, 18:22, 20:24] = 0, 255
    fill[:, 18:22, 24:28], src[:, 18:22, 24:28] = 255, 0
    fill[:, 22:26, 20:24], src[:, 22:26, 20:24] = 255, 255
    fill[:, 22:26, 24:28], src[:, 22:26, 24:28] = 0, 0
    return fill, src


@pytest.mark.parametrize("F", FEATHERS)
def test_composite_equals_the_statement(built_lib, gpu_device, pixels, F):
    fill, src = pixels
    for name, cmask in masks(H, W).items():
        d = fs.distance_separable(cmask, F)
        want = fs.blend(fill, src, d, F)
        got = _composite(built_lib, gpu_device, fill, src, d, F)
        assert np.array_equal(got, want), f"{name} F={F}: {int((got != want).sum())} bytes differ"
        if F == 1:
            assert np.array_equal(got, np.where(cmask[None, :, :, None] != 0, fill, src))


@pytest.mark.parametrize("lead,src_lead", [(0, 0), (16, 1), (3, 16), (15, 15)])
def test_composite_every_alignment(built_lib, gpu_device, pixels, lead, src_lead):
    fill, src = pixels
    cmask = masks(H, W)["edge rectangle"]
    d = fs.distance_separable(cmask, 3)
    got = _composite(built_lib, gpu_device, fill, src, d, 3, lead=lead, src_lead=src_lead, gap=lead % 5, src_gap=0)
    assert np.array_equal(got, fs.blend(fill, src, d, 3))


def test_composite_frames_shorter_than_a_chunk(built_lib, gpu_device):
    """1 x 3 and 2 x 5 pixel frames: head and tail only, or a single chunk"""
    rng = np.random.default_rng(3)
    for h, w in ((1, 3), (2, 5), (1, 11)):
        fill = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        src = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        cmask = np.ones((h, w), np.uint8)
        cmask[0, 0] = 0
        d = fs.distance_separable(cmask, 2)
        assert np.array_equal(_composite(built_lib, gpu_device, fill, src, d, 2), fs.blend(fill, src, d, 2))


@pytest.mark.parametrize("F", FEATHERS)
def test_identity(built_lib, gpu_device, pixels, F):
    """fill == src gives src for every d"""
    _, src = pixels
    for cmask in masks(H, W).values():
        d = fs.distance_separable(cmask, F)
        assert np.array_equal(_composite(built_lib, gpu_device, src, src, d, F), src)


def test_composite_frame_stride_past_2_to_31(built_lib, gpu_device):
    """two small frames 2^31 + 21 bytes apart (a batch is a slice of a large tensor): the second frame's start needs 64-bit arithmetic"""
    rng = np.random.default_rng(8)
    fill = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    src = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    cmask = masks(H, W)["edge rectangle"]
    d = fs.distance_separable(cmask, 3)
    size, stride, lead = H * W * 3, 2 ** 31 + 21, 3
    big = torch.empty(lead + stride + size + 64, dtype=torch.uint8, device=gpu_device)
    guard = 64
    for f in range(2):
        at = lead + f * stride
        big[at - min(at, guard):at + size + guard] = 0x5A
        big[at:at + size] = torch.from_numpy(fill[f].ravel()).to(gpu_device)
    st = torch.from_numpy(src).to(gpu_device)
    dt = torch.from_numpy(d).to(gpu_device)
    rc = built_lib.lib.vsr_feather_composite(C.c_void_p(big.data_ptr() + lead), stride, P(st), size, P(dt), 2, H, W, 3, None)
    torch.cuda.synchronize()
    assert rc == 0, built_lib.last_error()
    want = fs.blend(fill, src, d, 3)
    for f in range(2):
        at = lead + f * stride
        assert np.array_equal(big[at:at + size].cpu().numpy().reshape(H, W, 3), want[f]), f"frame {f}"
        assert (big[at - min(at, guard):at] == 0x5A).all() and (big[at + size:at + size + guard] == 0x5A).all()


def test_n_zero_is_success(built_lib, gpu_device):
    t = torch.zeros(64, dtype=torch.uint8, device=gpu_device)
    assert built_lib.lib.vsr_feather_composite(P(t), 27, P(t), 27, P(t), 0, 3, 3, 2, None) == 0


def test_argument_errors(built_lib, gpu_device):
    lib = built_lib.lib
    frames = torch.full((4096,), 9, dtype=torch.uint8, device=gpu_device)
    src = torch.full((4096,), 7, dtype=torch.uint8, device=gpu_device)
    al = torch.full((4096,), 1, dtype=torch.uint8, device=gpu_device)
    size = 8 * 8 * 3
    bad_composite = [
        (None, size, P(src), size, P(al), 2, 8, 8, 2), (P(frames), size, None, size, P(al), 2, 8, 8, 2),
        (P(frames), size, P(src), size, None, 2, 8, 8, 2), (P(frames), size, P(src), size, P(al), 2, 0, 8, 2),
        (P(frames), size, P(src), size, P(al), 2, 8, -1, 2), (P(frames), size, P(src), size, P(al), 2, 8, 8, 0),
        (P(frames), size, P(src), size, P(al), 2, 8, 8, 65), (P(frames), size - 1, P(src), size, P(al), 2, 8, 8, 2),
        (P(frames), size, P(src), size - 1, P(al), 2, 8, 8, 2), (P(frames), size, P(src), size, P(al), -1, 8, 8, 2),
        (P(frames), 2 ** 40, P(src), 2 ** 40, P(al), 1, 32768, 32768, 2),
    ]
    for args in bad_composite:
        assert lib.vsr_feather_composite(*args, None) == built_lib.VSR_ERR_ARG, args
        assert "feather" in built_lib.last_error()
    bad_alpha = [(None, 8, 8, 2, P(al)), (P(src), 8, 8, 2, None), (P(src), 0, 8, 2, P(al)), (P(src), 8, 0, 2, P(al)),
                 (P(src), 8, 8, 0, P(al)), (P(src), 8, 8, 65, P(al))]
    for args in bad_alpha:
        assert lib.vsr_feather_alpha(*args, None) == built_lib.VSR_ERR_ARG, args
        assert "feather" in built_lib.last_error()
    torch.cuda.synchronize()
    assert (frames == 9).all() and (src == 7).all() and (al == 1).all(), "a refused call wrote something"
