"""The three regrain kernels through the C-ABI (vsr_regrain_sets, vsr_regrain_measure, vsr_regrain_apply; csrc/regrain_kernels.hip)
against the numpy statement (tests/_regrain_statement.py): exact equality of the map, the counts, the per-frame sums and the frames;
unaligned and strided frames, the strip-row form, masks without a ring or without an interior, an uninpainted frame, argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _regrain_statement as rs

pytestmark = pytest.mark.gpu

N = 3
SHAPES = [(37, 53), (64, 200)]           # W * 3 = 159: no row start but the first is aligned to anything; 64 x 200: 2 x 4 tiles of the sets
PAD = 64


def P(t):
    return C.c_void_p(t.data_ptr())


def masks(H, W):
    out = {}
    band = np.zeros((H, W), np.uint8)
    band[H - H // 3:, :] = 255                                     # touches the bottom, left and right frame edges
    out["bottom band"] = band
    two = np.zeros((H, W), np.uint8)
    two[3:H // 3, 2:W // 2] = 255
    two[H // 2:H - 4, W // 2 + 3:W - 1] = 7                        # any non-zero value is inside
    out["two rectangles"] = two
    line = np.zeros((H, W), np.uint8)
    line[2:H - 2, W // 2] = 255
    out["line"] = line                                             # I is empty: the frames come back untouched
    out["full"] = np.full((H, W), 255, np.uint8)                   # E is empty: the frames come back untouched
    return out


def clip(H, W, cmask, seed, n=N, same=1):
    """src: a plane with noise; fill: src outside the mask, a flatter picture inside it with a column stripe one level under white and
    one a level over black (straight edges: the noise operator does not see them); frame `same` was not inpainted"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = (60 + 0.5 * x + 0.7 * y)[None, :, :, None] + np.zeros((n, 1, 1, 3))
    src = np.clip(np.rint(base + rng.normal(0, 9, base.shape)), 0, 255).astype(np.uint8)
    fill = src.copy()
    inside = cmask != 0
    flat = np.clip(np.rint(base + rng.normal(0, 1.5, base.shape)), 0, 255).astype(np.uint8)
    flat[:, :, W // 8:W // 4], flat[:, :, W // 2 + 6:W // 2 + 6 + W // 8] = 254, 1
    fill[:, inside] = flat[:, inside]
    if same is not None and same < n:
        fill[same] = src[same]
    return fill, src


def gpu_sets(lib, dev, cmask, R):
    H, W = cmask.shape
    c = torch.from_numpy(np.ascontiguousarray(cmask)).to(dev)
    buf = torch.full((H * W + 2 * PAD,), 0xA5, dtype=torch.uint8, device=dev)
    counts = torch.full((4,), -1, dtype=torch.int64, device=dev)   # the call zeroes its two words, not more
    rc = lib.lib.vsr_regrain_sets(P(c), H, W, R[0], R[1], C.c_void_p(buf.data_ptr() + PAD), P(counts), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.last_error()
    got = buf.cpu().numpy()
    assert (got[:PAD] == 0xA5).all() and (got[PAD + H * W:] == 0xA5).all(), "bytes around the map were written"
    cnt = counts.cpu().numpy()
    assert cnt[2] == -1 and cnt[3] == -1
    map_dev = buf[PAD:PAD + H * W]                                 # (an odd start is as good as any)
    return got[PAD:PAD + H * W].reshape(H, W), cnt[:2].tolist(), map_dev, counts


def rows_of(cmask):
    held = np.flatnonzero(cmask.any(axis=1))
    return int(held[0]), int(held[-1]) + 1


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


def gpu_regrain(lib, dev, fill, src, cmask, R, percent, y0=0, **kw):
    """sets, measure and apply on one stream, no host synchronisation between measure and apply -> (frames, stats [n,3], map, counts)"""
    H, W = cmask.shape
    n, h = fill.shape[:2]
    lead, src_lead = kw.get("lead", 5), kw.get("src_lead", 3)
    got_map, cnt, map_dev, counts = gpu_sets(lib, dev, cmask, R)
    c0, c1 = rows_of(cmask) if cmask.any() else (0, 0)
    ft, st, fstride, sstride, fbuf, sbuf = _buffers(dev, fill, src, **kw)
    stats = torch.full((n + 1, 4), -1, dtype=torch.int64, device=dev)
    fp, sp = C.c_void_p(ft.data_ptr() + lead), C.c_void_p(st.data_ptr() + src_lead)
    rc = lib.lib.vsr_regrain_measure(fp, fstride, sp, sstride, P(map_dev), n, H, W, y0, h, c0, c1, P(stats), None)
    assert rc == 0, lib.last_error()
    rc = lib.lib.vsr_regrain_apply(fp, fstride, P(map_dev), P(counts), P(stats), n, H, W, y0, h, c0, c1, percent, None)
    assert rc == 0, lib.last_error()
    torch.cuda.synchronize()
    got = ft.cpu().numpy()
    assert np.array_equal(st.cpu().numpy(), sbuf), "src was written"
    size = h * W * 3
    out = np.stack([got[lead + f * fstride:lead + f * fstride + size].reshape(h, W, 3) for f in range(n)])
    untouched = np.ones(got.size, bool)
    for f in range(n):
        untouched[lead + f * fstride:lead + f * fstride + size] = False
    assert np.array_equal(got[untouched], fbuf[untouched]), "bytes in front of, between or behind the frames were written"
    s = stats.cpu().numpy()
    assert (s[n] == -1).all(), "the words behind the last frame's were written"
    return out, s[:n, :3], got_map, cnt


def check(lib, dev, fill, src, cmask, R, percent=100, y0=0, **kw):
    info = []
    want = rs.regrain(fill, src, cmask, R, percent, y0=y0, info=info)
    out, stats, got_map, cnt = gpu_regrain(lib, dev, fill, src, cmask, R, percent, y0=y0, **kw)
    E, I = rs.sets(cmask, R)
    assert np.array_equal(got_map, rs.sets_map(cmask, R)), f"{int((got_map != rs.sets_map(cmask, R)).sum())} bytes of the map differ"
    assert cnt == [int(E.sum()), int(I.sum())]
    for t, (a_src, a_fill, changed, _r, _seed, _touched) in enumerate(info):
        assert stats[t, 0] == a_src and stats[t, 1] == a_fill and (stats[t, 2] != 0) == changed, f"frame {t}: {stats[t]} vs {info[t]}"
    assert np.array_equal(out, want), f"{int((out != want).sum())} bytes differ from the statement"
    return out, info


@pytest.mark.parametrize("shape", SHAPES)
def test_the_three_kernels_equal_the_statement(built_lib, gpu_device, shape):
    H, W = shape
    for k, (name, cmask) in enumerate(masks(H, W).items()):
        fill, src = clip(H, W, cmask, seed=H + k)
        out, info = check(built_lib, gpu_device, fill, src, cmask, (0, H))
        touched = [i[5] for i in info]
        if name in ("line", "full"):
            assert touched == [False] * N and np.array_equal(out, fill), name
        else:
            assert touched == [True, False, True], name
            assert all(i[3] > 0 for i in info if i[5]) and (out[0] != fill[0]).any() and (out[2] != fill[2]).any(), name
            assert np.array_equal(out[1], fill[1]), "the frame with fill == src comes back bit-identical"
            assert np.array_equal(out[:, cmask == 0], fill[:, cmask == 0])
            assert ((out == 0) & (fill == 1)).any() and ((out == 255) & (fill == 254)).any(), "both clamps were reached"


@pytest.mark.parametrize("percent", [1, 37, 200])
def test_other_percentages(built_lib, gpu_device, percent):
    H, W = SHAPES[0]
    cmask = masks(H, W)["two rectangles"]
    fill, src = clip(H, W, cmask, seed=percent)
    check(built_lib, gpu_device, fill, src, cmask, (0, H), percent=percent)


def test_percent_zero_launches_nothing_and_changes_nothing(built_lib, gpu_device):
    H, W = SHAPES[0]
    cmask = masks(H, W)["bottom band"]
    fill, src = clip(H, W, cmask, seed=1)
    out, _ = check(built_lib, gpu_device, fill, src, cmask, (0, H), percent=0)
    assert np.array_equal(out, fill)


@pytest.mark.parametrize("lead,src_lead", [(0, 0), (16, 1), (1, 16), (15, 15)])
def test_every_alignment(built_lib, gpu_device, lead, src_lead):
    H, W = SHAPES[0]
    cmask = masks(H, W)["two rectangles"]
    fill, src = clip(H, W, cmask, seed=21)
    check(built_lib, gpu_device, fill, src, cmask, (0, H), lead=lead, src_lead=src_lead, gap=lead % 5, src_gap=0)


@pytest.mark.parametrize("shape", SHAPES)
def test_strip_rows(built_lib, gpu_device, shape):
    """R a proper sub-range of the rows, once with whole frames and once with frames that hold R's rows only: the same rows come back"""
    H, W = shape
    R = (H // 4, H - 3)
    cmask = np.zeros((H, W), np.uint8)
    cmask[H // 2:H - 8, 4:W - 6] = 255
    cmask[R[0]:R[0] + 4, W // 3:W // 2] = 255                      # touches the first sample row
    fill, src = clip(H, W, cmask, seed=H)
    whole, info = check(built_lib, gpu_device, fill, src, cmask, R)
    assert [i[5] for i in info] == [True, False, True]
    rows, _ = check(built_lib, gpu_device, fill[:, R[0]:R[1]], src[:, R[0]:R[1]], cmask, R, y0=R[0])
    assert np.array_equal(rows, whole[:, R[0]:R[1]])
    E_all = rs.sets(cmask, (0, H))[0]
    assert E_all.sum() > rs.sets(cmask, R)[0].sum(), "R cut samples off"


def test_more_than_one_column_tile_and_many_frames(built_lib, gpu_device):
    """W = 300 > the 256 columns one workgroup of the measure covers; 40 rows: five row tiles; n = 5 with two uninpainted frames"""
    H, W = 40, 300
    cmask = np.zeros((H, W), np.uint8)
    cmask[18:34, 1:W - 1] = 255
    cmask[2:7, 250:262] = 255                                      # straddles column 256
    fill, src = clip(H, W, cmask, seed=77, n=5, same=0)
    fill[3] = src[3]
    _, info = check(built_lib, gpu_device, fill, src, cmask, (0, H))
    assert [i[5] for i in info] == [False, True, True, False, True]


def test_identical_frames_get_identical_grain(built_lib, gpu_device):
    H, W = SHAPES[0]
    cmask = masks(H, W)["bottom band"]
    fill, src = clip(H, W, cmask, seed=5, n=1, same=None)
    out, _ = check(built_lib, gpu_device, np.concatenate([fill] * 3), np.concatenate([src] * 3), cmask, (0, H))
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


def test_n_zero_is_success(built_lib, gpu_device):
    t = torch.zeros(64, dtype=torch.int64, device=gpu_device)
    assert built_lib.lib.vsr_regrain_measure(P(t), 27, P(t), 27, P(t), 0, 3, 3, 0, 3, 0, 3, P(t), None) == 0
    assert built_lib.lib.vsr_regrain_apply(P(t), 27, P(t), P(t), P(t), 0, 3, 3, 0, 3, 0, 3, 100, None) == 0


def test_argument_errors(built_lib, gpu_device):
    lib = built_lib.lib
    frames = torch.full((4096,), 9, dtype=torch.uint8, device=gpu_device)
    src = torch.full((4096,), 7, dtype=torch.uint8, device=gpu_device)
    mp = torch.full((4096,), 4, dtype=torch.uint8, device=gpu_device)
    words = torch.full((64,), 5, dtype=torch.int64, device=gpu_device)
    size = 8 * 8 * 3
    ok = dict(frames=P(frames), fs=size, src=P(src), ss=size, map=P(mp), n=2, H=8, W=8, y0=0, rows=8, c0=2, c1=6)

    def measure(**kw):
        a = dict(ok, **kw)
        return lib.vsr_regrain_measure(a["frames"], a["fs"], a["src"], a["ss"], a["map"], a["n"], a["H"], a["W"], a["y0"], a["rows"], a["c0"],
                                       a["c1"], kw.get("stats", P(words)), None)

    def apply(**kw):
        a = dict(ok, **kw)
        return lib.vsr_regrain_apply(a["frames"], a["fs"], a["map"], kw.get("counts", P(words)), kw.get("stats", P(words)), a["n"], a["H"],
                                     a["W"], a["y0"], a["rows"], a["c0"], a["c1"], kw.get("percent", 100), None)

    bad = [dict(frames=None), dict(map=None), dict(stats=None), dict(H=0), dict(W=-1), dict(n=-1), dict(fs=size - 1), dict(y0=-1),
           dict(y0=1), dict(rows=0), dict(rows=9), dict(c0=-1), dict(c0=7, c1=6), dict(c1=9), dict(H=32768, W=32768, rows=1)]
    for kw in bad:
        assert measure(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "regrain" in built_lib.last_error()
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "regrain" in built_lib.last_error()
    for kw in (dict(src=None), dict(ss=size - 1)):
        assert measure(**kw) == built_lib.VSR_ERR_ARG, kw
    for kw in (dict(counts=None), dict(percent=-1), dict(percent=201)):
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
    bad_sets = [(None, 8, 8, 0, 8, P(mp), P(words)), (P(src), 8, 8, 0, 8, None, P(words)), (P(src), 8, 8, 0, 8, P(mp), None),
                (P(src), 0, 8, 0, 0, P(mp), P(words)), (P(src), 8, 0, 0, 8, P(mp), P(words)), (P(src), 8, 8, -1, 8, P(mp), P(words)),
                (P(src), 8, 8, 5, 4, P(mp), P(words)), (P(src), 8, 8, 0, 9, P(mp), P(words))]
    for args in bad_sets:
        assert lib.vsr_regrain_sets(*args, None) == built_lib.VSR_ERR_ARG, args
        assert "regrain" in built_lib.last_error()
    torch.cuda.synchronize()
    assert (frames == 9).all() and (src == 7).all() and (mp == 4).all() and (words == 5).all(), "a refused call wrote something"
