"""The two deflicker kernels through the C-ABI (vsr_deflicker_pairs, vsr_deflicker_apply; csrc/deflicker_kernels.hip), behind
vsr_regrain_sets and vsr_regrain_measure as the product runs them, against the numpy statement (tests/_deflicker_statement.py): exact
equality of the pair sums and the frames; unaligned and strided frames, source and snapshot, the strip-row form, masks without a ring,
an uninpainted frame, a cut, a window wider than the batch, argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _deflicker_statement as ds
from tests import _regrain_statement as rs
from tests.test_gpu_regrain import SHAPES, P, gpu_sets, masks, rows_of

pytestmark = pytest.mark.gpu

N = 5
SAME, CUT = 1, 3


def clip(H, W, cmask, seed, n=N, same=SAME, cut=CUT, drift=6):
    """src: a still plane with grain; from frame `cut` on its negative (a cut), the last frame `drift` levels up (a pair that is
    neither open nor closed).  fill: src outside the mask; inside it one smooth picture plus a per-frame offset and a few levels of
    per-pixel noise, so that D falls on both sides of TH; frame `same` was not inpainted"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = (60 + 0.5 * x + 0.7 * y)[None, :, :, None] + np.zeros((n, 1, 1, 3))
    if cut is not None:
        base[cut:] = 255 - base[cut:]
    if drift:
        base[n - 1] += drift
    src = np.clip(np.rint(base + rng.normal(0, 4, base.shape)), 0, 255).astype(np.uint8)
    smooth = 128 + 60 * np.sin(x / 5.0 + y / 7.0)[None, :, :, None] + rng.integers(-ds.TH + 1, ds.TH, n)[:, None, None, None]
    flat = np.clip(np.rint(smooth) + rng.integers(-12, 13, base.shape), 0, 255).astype(np.uint8)
    fill = src.copy()
    inside = cmask != 0
    fill[:, inside] = flat[:, inside]
    if same is not None and same < n:
        fill[same] = src[same]
    return fill, src


def _strided(dev, frames, lead, gap, byte):
    """the frames in a larger buffer: odd start `lead`, stride = frame + gap, `byte` everywhere else"""
    n, size = frames.shape[0], frames[0].size
    stride = size + gap
    buf = np.full(lead + n * stride + 32, byte, np.uint8)
    for f in range(n):
        buf[lead + f * stride:lead + f * stride + size] = frames[f].ravel()
    return torch.from_numpy(buf).to(dev), stride, buf


def gpu_deflicker(lib, dev, fill, src, cmask, rows, R, y0=0, lead=5, gap=7, src_lead=3, src_gap=13, snap_lead=1, snap_gap=11):
    """sets, measure, pairs and apply on one stream with no host synchronisation between them -> (frames, pairs [n][R])"""
    H, W = cmask.shape
    n, h = fill.shape[:2]
    _, cnt, map_dev, counts = gpu_sets(lib, dev, cmask, rows)
    c0, c1 = rows_of(cmask) if cmask.any() else (0, 0)
    la, lb = max(c0 - y0, 0), min(c1 - y0, h)
    assert lb > la
    snap = np.ascontiguousarray(fill[:, la:lb])
    ft, fstride, fbuf = _strided(dev, fill, lead, gap, 0x5A)
    st, sstride, sbuf = _strided(dev, src, src_lead, src_gap, 0xC3)
    nt, nstride, nbuf = _strided(dev, snap, snap_lead, snap_gap, 0x3C)
    stats = torch.full((n + 1, 4), -1, dtype=torch.int64, device=dev)
    pairs = torch.full((n * R + 2,), -1, dtype=torch.int64, device=dev)
    fp, sp, np_ = C.c_void_p(ft.data_ptr() + lead), C.c_void_p(st.data_ptr() + src_lead), C.c_void_p(nt.data_ptr() + snap_lead)
    rc = lib.lib.vsr_regrain_measure(fp, fstride, sp, sstride, P(map_dev), n, H, W, y0, h, c0, c1, P(stats), None)
    assert rc == 0, lib.last_error()
    rc = lib.lib.vsr_deflicker_pairs(sp, sstride, P(map_dev), n, H, W, y0, h, c0, c1, R, P(pairs), None)
    assert rc == 0, lib.last_error()
    rc = lib.lib.vsr_deflicker_apply(fp, fstride, np_, nstride, P(map_dev), P(counts), P(stats), P(pairs), n, H, W, y0, h, c0, c1, R, None)
    assert rc == 0, lib.last_error()
    torch.cuda.synchronize()
    got = ft.cpu().numpy()
    assert np.array_equal(st.cpu().numpy(), sbuf), "src was written"
    assert np.array_equal(nt.cpu().numpy(), nbuf), "the snapshot was written"
    size = h * W * 3
    out = np.stack([got[lead + f * fstride:lead + f * fstride + size].reshape(h, W, 3) for f in range(n)])
    untouched = np.ones(got.size, bool)
    for f in range(n):
        untouched[lead + f * fstride:lead + f * fstride + size] = False
    assert np.array_equal(got[untouched], fbuf[untouched]), "bytes in front of, between or behind the frames were written"
    pr = pairs.cpu().numpy()
    assert (pr[n * R:] == -1).all(), "the words behind the last frame's were written"
    return out, pr[:n * R].reshape(n, R), cnt


def check(lib, dev, fill, src, cmask, rows, R, y0=0, **kw):
    info = {}
    want = ds.deflicker(fill, src, cmask, rows, R, y0=y0, info=info)
    out, pairs, cnt = gpu_deflicker(lib, dev, fill, src, cmask, rows, R, y0=y0, **kw)
    assert 3 * cnt[0] == info["m"]
    assert np.array_equal(pairs, info["S"]), f"pair sums: {pairs.tolist()} vs {info['S'].tolist()}"
    assert np.array_equal(out, want), f"{int((out != want).sum())} bytes differ from the statement"
    return out, info


@pytest.mark.parametrize("R", [1, 2, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_kernels_equal_the_statement(built_lib, gpu_device, shape, R):
    H, W = shape
    for k, (name, cmask) in enumerate(masks(H, W).items()):
        fill, src = clip(H, W, cmask, seed=H + k)
        out, info = check(built_lib, gpu_device, fill, src, cmask, (0, H), R)
        if name == "full":
            assert info["m"] == 0 and np.array_equal(out, fill), "no ring: the identity"
            continue
        assert info["changed"] == [True, False, True, True, True], name
        for (t, j), a in info["a"].items():
            if SAME in (t, t + j) or t < CUT <= t + j:
                assert a == 0, (name, t, j, a)
        assert 0 < info["a"][(3, 1)] < 16, (name, "the drifting pair is half open", info["a"][(3, 1)])
        assert np.array_equal(out[SAME], fill[SAME]), "the frame with fill == src comes back bit-identical"
        assert np.array_equal(out[:, cmask == 0], fill[:, cmask == 0])
        assert (out[3] != fill[3]).any() and (out[4] != fill[4]).any(), name
        if R == 1:
            assert np.array_equal(out[:3], fill[:3]), "frames 0 and 2 have the uninpainted frame and the cut for neighbours"
        else:
            assert info["a"][(0, 2)] == 16 and (out[0] != fill[0]).any() and (out[2] != fill[2]).any(), name


@pytest.mark.parametrize("lead,src_lead,snap_lead", [(0, 0, 0), (16, 1, 2), (1, 16, 3), (15, 15, 16), (2, 3, 0)])
def test_every_alignment(built_lib, gpu_device, lead, src_lead, snap_lead):
    H, W = SHAPES[0]
    cmask = masks(H, W)["two rectangles"]
    fill, src = clip(H, W, cmask, seed=21)
    check(built_lib, gpu_device, fill, src, cmask, (0, H), 2, lead=lead, src_lead=src_lead, snap_lead=snap_lead, gap=lead % 5, src_gap=0,
          snap_gap=snap_lead % 3)


@pytest.mark.parametrize("shape", SHAPES)
def test_strip_rows(built_lib, gpu_device, shape):
    """sample rows a proper sub-range of the frame, once with whole frames and once with frames that hold those rows only"""
    H, W = shape
    rows = (H // 4, H - 3)
    cmask = np.zeros((H, W), np.uint8)
    cmask[H // 2:H - 8, 4:W - 6] = 255
    cmask[rows[0]:rows[0] + 4, W // 3:W // 2] = 255                # touches the first sample row
    fill, src = clip(H, W, cmask, seed=H)
    whole, info = check(built_lib, gpu_device, fill, src, cmask, rows, 2)
    assert not np.array_equal(whole, fill)
    strip, _ = check(built_lib, gpu_device, fill[:, rows[0]:rows[1]], src[:, rows[0]:rows[1]], cmask, rows, 2, y0=rows[0])
    assert np.array_equal(strip, whole[:, rows[0]:rows[1]])
    assert rs.sets(cmask, (0, H))[0].sum() > info["m"] // 3, "the sample rows cut samples off"


def test_more_than_one_column_tile_and_many_frames(built_lib, gpu_device):
    """W = 600 > the 256 columns one workgroup of the pairs kernel covers; 40 frames, R = 8: interior frames have 16 neighbours"""
    H, W, n = 8, 600, 40
    cmask = np.zeros((H, W), np.uint8)
    cmask[3:5, 10:W - 10] = 255
    fill, src = clip(H, W, cmask, seed=77, n=n, same=17, cut=29, drift=0)
    out, info = check(built_lib, gpu_device, fill, src, cmask, (0, H), 8)
    assert info["m"] > 3 * 512 and sum(a == 16 for a in info["a"].values()) > 150
    assert all((out[t] != fill[t]).any() for t in range(n) if t != 17) and np.array_equal(out[17], fill[17])


def test_n_zero_and_r_zero_are_success_and_write_nothing(built_lib, gpu_device):
    t = torch.full((4096,), 0x33, dtype=torch.uint8, device=gpu_device)
    lib = built_lib.lib
    for n, R in ((0, 2), (3, 0), (0, 0)):
        assert lib.vsr_deflicker_pairs(P(t), 27, P(t), n, 3, 3, 0, 3, 0, 3, R, P(t), None) == 0
        assert lib.vsr_deflicker_apply(P(t), 27, P(t), 27, P(t), P(t), P(t), P(t), n, 3, 3, 0, 3, 0, 3, R, None) == 0
    torch.cuda.synchronize()
    assert (t == 0x33).all()


def test_argument_errors(built_lib, gpu_device):
    lib = built_lib.lib
    frames = torch.full((4096,), 9, dtype=torch.uint8, device=gpu_device)
    src = torch.full((4096,), 7, dtype=torch.uint8, device=gpu_device)
    snap = torch.full((4096,), 3, dtype=torch.uint8, device=gpu_device)
    mp = torch.full((4096,), 4, dtype=torch.uint8, device=gpu_device)
    words = torch.full((64,), 5, dtype=torch.int64, device=gpu_device)
    size = 8 * 8 * 3
    ok = dict(frames=P(frames), fs=size, src=P(src), ss=size, snap=P(snap), ns=4 * 8 * 3, map=P(mp), n=2, H=8, W=8, y0=0, rows=8, c0=2, c1=6,
              R=2)

    def pairs(**kw):
        a = dict(ok, **kw)
        return lib.vsr_deflicker_pairs(a["src"], a["ss"], a["map"], a["n"], a["H"], a["W"], a["y0"], a["rows"], a["c0"], a["c1"], a["R"],
                                       kw.get("pairs", P(words)), None)

    def apply(**kw):
        a = dict(ok, **kw)
        return lib.vsr_deflicker_apply(a["frames"], a["fs"], a["snap"], a["ns"], a["map"], kw.get("counts", P(words)),
                                       kw.get("stats", P(words)), kw.get("pairs", P(words)), a["n"], a["H"], a["W"], a["y0"], a["rows"],
                                       a["c0"], a["c1"], a["R"], None)

    both = [dict(map=None), dict(pairs=None), dict(H=0), dict(W=-1), dict(n=-1), dict(y0=-1), dict(y0=1), dict(rows=0), dict(rows=9),
            dict(c0=-1), dict(c0=7, c1=6), dict(c1=9), dict(H=32768, W=32768, rows=1), dict(R=-1), dict(R=9)]
    for kw in both:
        assert pairs(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "deflicker" in built_lib.last_error()
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "deflicker" in built_lib.last_error()
    for kw in (dict(src=None), dict(ss=size - 1)):
        assert pairs(**kw) == built_lib.VSR_ERR_ARG, kw
    for kw in (dict(frames=None), dict(snap=None), dict(counts=None), dict(stats=None), dict(fs=size - 1), dict(ns=4 * 8 * 3 - 1)):
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
    torch.cuda.synchronize()
    assert (frames == 9).all() and (src == 7).all() and (snap == 3).all() and (mp == 4).all() and (words == 5).all(), \
        "a refused call wrote something"
