"""The tone-match kernels through the C-ABI (vsr_tone_sets, vsr_tone_workspace_bytes, vsr_tone_apply; csrc/tone_kernels.hip) against the
numpy statement (tests/_tone_statement.py): exact equality of the map, the counts, the cell list and the frames, no tolerance;
unaligned and strided frames, the strip-row form, an uninpainted frame, masks without one of the bands, the clamp, argument errors.
The shapes are the smallest at which the kernels can go wrong: 45 x 75 (neither side a multiple of 8, K = 7), 130 x 260 (K = 9,
partial cells on two edges), 7 x 8 (K = 3: the pyramid is one cell)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _tone_statement as ts

pytestmark = pytest.mark.gpu

N = 3
SHAPES = [(45, 75), (130, 260)]
PAD = 64


def P(t):
    return C.c_void_p(t.data_ptr())


def masks(H, W):
    out = {}
    bottom = np.zeros((H, W), np.uint8)
    bottom[H - H // 4:, W // 6:W - W // 5] = 255                    # touches the bottom border: no seam there
    out["bottom box"] = bottom
    two = np.zeros((H, W), np.uint8)
    two[4:7, 3:W // 2] = 255                                        # 3 px high: M is the whole box
    two[H // 2:H - 6, W // 2 + 3:W - 2] = 7                         # any non-zero value is inside
    out["two boxes"] = two
    one = np.zeros((H, W), np.uint8)
    one[H // 2 + 1, W // 3] = 255
    out["one pixel"] = one
    deep = np.zeros((H, W), np.uint8)
    deep[2:42, 5:W - 9] = 255                                       # 40 px deep: the interior lies beyond the bands, the push reaches it
    out["deep box"] = deep
    aligned = np.zeros((H, W), np.uint8)
    aligned[16:32, 8:W // 8 * 8 - 8] = 255                          # the seam on multiples of 8: E and M in different level-3 cells
    out["aligned seam"] = aligned
    return out


def clip(H, W, cmask, seed, n=N, same=1, step=(9, -6, 14)):
    """src: a plane with noise; fill: src outside the mask, inside it a flatter picture `step` levels off; frame `same` was not inpainted"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = (70 + 0.4 * x + 0.6 * y)[None, :, :, None] + np.zeros((n, 1, 1, 3))
    src = np.clip(np.rint(base + rng.normal(0, 9, base.shape)), 0, 255).astype(np.uint8)
    fill = src.copy()
    inside = cmask != 0
    flat = np.clip(np.rint(base + rng.normal(0, 2, base.shape) - np.array(step)), 0, 255).astype(np.uint8)
    fill[:, inside] = flat[:, inside]
    if same is not None and same < n:
        fill[same] = src[same]
    return fill, src


def gpu_sets(lib, dev, cmask, R):
    """-> (map, [|E|, |M|, cells], the sorted cell list, map_dev, cells_dev)"""
    H, W = cmask.shape
    g3 = -(-H // 8) * -(-W // 8)
    c = torch.from_numpy(np.ascontiguousarray(cmask)).to(dev)
    buf = torch.full((H * W + 2 * PAD,), 0xA5, dtype=torch.uint8, device=dev)
    counts = torch.full((5,), -1, dtype=torch.int64, device=dev)    # the call zeroes its three words, not more
    cells = torch.full((g3 + 4,), -7, dtype=torch.int32, device=dev)
    rc = lib.lib.vsr_tone_sets(P(c), H, W, R[0], R[1], C.c_void_p(buf.data_ptr() + PAD), P(counts), P(cells), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.last_error()
    got = buf.cpu().numpy()
    assert (got[:PAD] == 0xA5).all() and (got[PAD + H * W:] == 0xA5).all(), "bytes around the map were written"
    cnt = counts.cpu().numpy()
    assert cnt[3] == -1 and cnt[4] == -1
    listed = cells.cpu().numpy()
    assert 0 <= cnt[2] <= g3 and (listed[cnt[2]:] == -7).all(), "words behind the list were written"
    return got[PAD:PAD + H * W].reshape(H, W), cnt[:3].tolist(), np.sort(listed[:cnt[2]]), buf[PAD:PAD + H * W], cells


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


def gpu_tone(lib, dev, fill, src, cmask, R, S, y0=0, **kw):
    """sets, then the one per-call entry point on the same stream -> (frames, map, counts, cells)"""
    H, W = cmask.shape
    n, h = fill.shape[:2]
    lead, src_lead = kw.get("lead", 5), kw.get("src_lead", 3)
    got_map, cnt, listed, map_dev, cells_dev = gpu_sets(lib, dev, cmask, R)
    c0, c1 = rows_of(cmask) if cmask.any() else (0, 0)
    ft, st, fstride, sstride, fbuf, sbuf = _buffers(dev, fill, src, **kw)
    nbytes = lib.lib.vsr_tone_workspace_bytes(H, W, n)
    assert nbytes > 0 and nbytes % 4 == 0
    work = torch.full((nbytes // 8 + 2,), -1, dtype=torch.int64, device=dev)       # garbage: the call initialises what it reads
    fp, sp = C.c_void_p(ft.data_ptr() + lead), C.c_void_p(st.data_ptr() + src_lead)
    rc = lib.lib.vsr_tone_apply(fp, fstride, sp, sstride, P(map_dev), P(cells_dev), cnt[2], n, H, W, y0, h, c0, c1, S, P(work), None)
    assert rc == 0, lib.last_error()
    torch.cuda.synchronize()
    got = ft.cpu().numpy()
    assert np.array_equal(st.cpu().numpy(), sbuf), "src was written"
    assert int(work[-1]) == -1, "the word behind the workspace was written"
    size = h * W * 3
    out = np.stack([got[lead + f * fstride:lead + f * fstride + size].reshape(h, W, 3) for f in range(n)])
    untouched = np.ones(got.size, bool)
    for f in range(n):
        untouched[lead + f * fstride:lead + f * fstride + size] = False
    assert np.array_equal(got[untouched], fbuf[untouched]), "bytes in front of, between or behind the frames were written"
    return out, got_map, cnt, listed


def check(lib, dev, fill, src, cmask, R, S=100, y0=0, **kw):
    info = []
    want = ts.tone(fill, src, cmask, R, S, y0=y0, info=info)
    out, got_map, cnt, listed = gpu_tone(lib, dev, fill, src, cmask, R, S, y0=y0, **kw)
    E, M = ts.bands(cmask, R)
    assert np.array_equal(got_map, ts.sets_map(cmask, R)), f"{int((got_map != ts.sets_map(cmask, R)).sum())} bytes of the map differ"
    assert np.array_equal(listed, ts.cells(cmask, R)), "the cell list"
    assert cnt == [int(E.sum()), int(M.sum()), len(ts.cells(cmask, R))]
    assert np.array_equal(out, want), f"{int((out != want).sum())} bytes differ from the statement, by up to " \
                                      f"{int(np.abs(out.astype(int) - want).max())}"
    return out, info


@pytest.mark.parametrize("shape", SHAPES)
def test_the_kernels_equal_the_statement(built_lib, gpu_device, shape):
    H, W = shape
    for k, (name, cmask) in enumerate(masks(H, W).items()):
        fill, src = clip(H, W, cmask, seed=H + k)
        out, info = check(built_lib, gpu_device, fill, src, cmask, (0, H))
        assert [i[3] for i in info] == [True, False, True], name
        assert np.array_equal(out[1], fill[1]), "the frame with fill == src comes back bit-identical"
        assert np.array_equal(out[:, cmask == 0], fill[:, cmask == 0])
        assert (out[0] != fill[0]).any() and (out[2] != fill[2]).any(), name
        if name == "two boxes":
            assert np.array_equal(ts.bands(cmask, (0, H))[1][4:7], cmask[4:7] != 0), "M is the whole of the thin box"
        if name == "deep box":
            beyond = np.zeros((H, W), bool)
            beyond[12:32, 15:W - 19] = True                         # ten pixels from the seam: no sample in these cells
            assert not (ts.sets_map(cmask, (0, H))[beyond] & 3).any() and (out[0][beyond] != fill[0][beyond]).any()
        if name == "aligned seam":
            E, M = ts.bands(cmask, (0, H))
            cell = lambda s: set(map(tuple, (np.argwhere(s) // 8).tolist()))          # noqa: E731
            assert not (cell(E) & cell(M)), "no level-3 cell holds samples of both sets"


@pytest.mark.parametrize("S", [1, 37, 100])
def test_strengths(built_lib, gpu_device, S):
    H, W = SHAPES[0]
    cmask = masks(H, W)["two boxes"]
    fill, src = clip(H, W, cmask, seed=S)
    out, _ = check(built_lib, gpu_device, fill, src, cmask, (0, H), S=S)
    assert (out != fill).any() or S == 1


def test_a_step_beyond_the_clamp(built_lib, gpu_device):
    """a fill 60 levels off: h3 sits on the clamp of 24 levels; and one next to white and black so that the bytes clamp too"""
    H, W = SHAPES[0]
    cmask = masks(H, W)["bottom box"]
    for step in ((60, -60, 40), (-30, 30, 0)):
        fill, src = clip(H, W, cmask, seed=3, step=step)
        out, info = check(built_lib, gpu_device, fill, src, cmask, (0, H))
        assert any((np.abs(i[4]) == ts.CLAMP).any() for i in info if i[3]), "the clamp was not reached"
    fill, src = clip(H, W, cmask, seed=4, step=(0, 0, 0))
    src[:, cmask == 0] = np.array([255, 0, 128], np.uint8)
    fill[:, cmask == 0] = src[:, cmask == 0]
    fill[:, cmask != 0] = np.array([245, 8, 128], np.uint8)
    fill[:, :, ::2][:, cmask[:, ::2] != 0] = np.array([255, 0, 128], np.uint8)       # every other column is white / black already
    fill[1] = src[1]
    out, info = check(built_lib, gpu_device, fill, src, cmask, (0, H))
    assert info[0][4][..., 0].max() >= 3 * 64 and info[0][4][..., 1].min() <= -3 * 64, "the field pushes white up and black down"
    assert (out[0] != fill[0]).any() and np.array_equal(out[0][:, ::2], fill[0][:, ::2]), "the bytes at the ends of the range stayed"


def test_s_zero_launches_nothing_and_changes_nothing(built_lib, gpu_device):
    H, W = SHAPES[0]
    cmask = masks(H, W)["bottom box"]
    fill, src = clip(H, W, cmask, seed=1)
    out, _ = check(built_lib, gpu_device, fill, src, cmask, (0, H), S=0)
    assert np.array_equal(out, fill)


@pytest.mark.parametrize("lead,src_lead", [(0, 0), (1, 16), (15, 15)])
def test_every_alignment(built_lib, gpu_device, lead, src_lead):
    H, W = SHAPES[0]
    cmask = masks(H, W)["two boxes"]
    fill, src = clip(H, W, cmask, seed=21)
    check(built_lib, gpu_device, fill, src, cmask, (0, H), lead=lead, src_lead=src_lead, gap=lead % 5, src_gap=0 if lead else 29)


def test_strip_rows(built_lib, gpu_device):
    """y0 = 5, h = 33, [r0, r1) = [5, 38) of H = 45, once with whole frames and once with frames that hold those rows only: the same
    rows come back; a second box outside the rows takes no part"""
    H, W = SHAPES[0]
    R = (5, 38)
    cmask = np.zeros((H, W), np.uint8)
    cmask[14:30, 6:W - 11] = 255
    cmask[5:8, W // 3:W // 2] = 255                                 # touches the first sample row
    fill, src = clip(H, W, cmask, seed=H)
    whole, info = check(built_lib, gpu_device, fill, src, cmask, R)
    assert [i[3] for i in info] == [True, False, True]
    rows, _ = check(built_lib, gpu_device, fill[:, R[0]:R[1]], src[:, R[0]:R[1]], cmask, R, y0=R[0])
    assert np.array_equal(rows, whole[:, R[0]:R[1]])
    assert ts.bands(cmask, (0, H))[0].sum() > ts.bands(cmask, R)[0].sum(), "R cut samples off"


def test_a_band_missing_leaves_the_frames(built_lib, gpu_device):
    """C everywhere: E is empty; C everywhere in the sample rows and the rows held: both are; sample rows away from the mask: both are"""
    H, W = SHAPES[0]
    full = np.full((H, W), 255, np.uint8)
    fill, src = clip(H, W, full, seed=8)
    out, info = check(built_lib, gpu_device, fill, src, full, (0, H))
    assert np.array_equal(out, fill) and not any(i[3] for i in info)
    box = masks(H, W)["deep box"]
    fill, src = clip(H, W, box, seed=9)
    out, info = check(built_lib, gpu_device, fill, src, box, (H - 1, H))
    assert np.array_equal(out, fill) and info[0][0] == 0 and info[0][1] == 0
    out, _ = check(built_lib, gpu_device, fill[:, 10:20], src[:, 10:20], box, (0, H), y0=10)       # the rows held: M's columns only, E too
    assert (out != fill[:, 10:20]).any()


def test_a_picture_of_one_cell(built_lib, gpu_device):
    """7 x 8: K = 3, no level above the finest; and 9 x 8: two cells under one"""
    for H, W in ((7, 8), (9, 8)):
        cmask = np.zeros((H, W), np.uint8)
        cmask[2:5, 1:6] = 255
        fill, src = clip(H, W, cmask, seed=H, step=(12, -8, 5))
        out, info = check(built_lib, gpu_device, fill, src, cmask, (0, H))
        assert [i[3] for i in info] == [True, False, True] and (out[0] != fill[0]).any()


def test_many_frames_and_more_cells_than_threads(built_lib, gpu_device):
    """n = 5 with two uninpainted frames on the wide picture; every frame has its own workgroup and part of the workspace"""
    H, W = SHAPES[1]
    cmask = masks(H, W)["deep box"]
    fill, src = clip(H, W, cmask, seed=77, n=5, same=0)
    fill[3] = src[3]
    out, info = check(built_lib, gpu_device, fill, src, cmask, (0, H), S=80)
    assert [i[3] for i in info] == [False, True, True, False, True]


def test_n_zero_is_success(built_lib, gpu_device):
    t = torch.zeros(64, dtype=torch.int64, device=gpu_device)
    assert built_lib.lib.vsr_tone_workspace_bytes(3, 3, 0) == 0
    assert built_lib.lib.vsr_tone_apply(P(t), 27, P(t), 27, P(t), P(t), 1, 0, 3, 3, 0, 3, 0, 3, 100, P(t), None) == 0


def test_argument_errors(built_lib, gpu_device):
    lib = built_lib.lib
    frames = torch.full((4096,), 9, dtype=torch.uint8, device=gpu_device)
    src = torch.full((4096,), 7, dtype=torch.uint8, device=gpu_device)
    mp = torch.full((4096,), 4, dtype=torch.uint8, device=gpu_device)
    words = torch.full((4096,), 5, dtype=torch.int64, device=gpu_device)
    cells = torch.zeros((16,), dtype=torch.int32, device=gpu_device)
    size = 8 * 8 * 3
    ok = dict(frames=P(frames), fs=size, src=P(src), ss=size, map=P(mp), cells=P(cells), ncells=1, n=2, H=8, W=8, y0=0, rows=8, c0=2, c1=6,
              S=100, work=P(words))

    def apply(**kw):
        a = dict(ok, **kw)
        return lib.vsr_tone_apply(a["frames"], a["fs"], a["src"], a["ss"], a["map"], a["cells"], a["ncells"], a["n"], a["H"], a["W"], a["y0"],
                                  a["rows"], a["c0"], a["c1"], a["S"], a["work"], None)

    bad = [dict(frames=None), dict(src=None), dict(map=None), dict(cells=None), dict(work=None), dict(H=0), dict(W=-1), dict(n=-1),
           dict(fs=size - 1), dict(ss=size - 1), dict(y0=-1), dict(y0=1), dict(rows=0), dict(rows=9), dict(c0=-1), dict(c0=7, c1=6),
           dict(c1=9), dict(H=32768, W=32768, rows=1), dict(S=-1), dict(S=101), dict(ncells=-1), dict(ncells=2),
           dict(work=C.c_void_p(words.data_ptr() + 4))]
    for kw in bad:
        assert apply(**kw) == built_lib.VSR_ERR_ARG, kw
        assert "tone match" in built_lib.last_error()
    assert apply(S=0) == 0 and apply(n=0) == 0, "nothing to do is success"
    bad_sets = [(None, 8, 8, 0, 8, P(mp), P(words), P(cells)), (P(src), 8, 8, 0, 8, None, P(words), P(cells)),
                (P(src), 8, 8, 0, 8, P(mp), None, P(cells)), (P(src), 8, 8, 0, 8, P(mp), P(words), None),
                (P(src), 0, 8, 0, 0, P(mp), P(words), P(cells)), (P(src), 8, 0, 0, 8, P(mp), P(words), P(cells)),
                (P(src), 8, 8, -1, 8, P(mp), P(words), P(cells)), (P(src), 8, 8, 5, 4, P(mp), P(words), P(cells)),
                (P(src), 8, 8, 0, 9, P(mp), P(words), P(cells)), (P(src), 32768, 32768, 0, 1, P(mp), P(words), P(cells))]
    for args in bad_sets:
        assert lib.vsr_tone_sets(*args, None) == built_lib.VSR_ERR_ARG, args
        assert "tone match" in built_lib.last_error()
    for args in ((0, 8, 1), (8, -1, 1), (8, 8, -1), (32768, 32768, 1)):
        assert lib.vsr_tone_workspace_bytes(*args) == built_lib.VSR_ERR_ARG, args
    torch.cuda.synchronize()
    assert (frames == 9).all() and (src == 7).all() and (mp == 4).all() and (words == 5).all() and (cells == 0).all(), \
        "a refused call wrote something"
