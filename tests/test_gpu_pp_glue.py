"""The ProPainter plugin's glue kernels (csrc/pp_kernels.hip: k_pp_prepare, k_pp_compose, k_pp_blend) and the scene detector's
difference sums (csrc/scene_kernels.hip: k_absdiff_sums) one launch at a time through the public calls of vsr_amd._lib, against the
numpy restatements of tests/_pp_glue_ref.py (held against the reference wrapper's own lines by tests/test_pp_glue_reference.py).

Outputs are prefilled with a sentinel and carry guard cells around them; what a call must not write still holds the sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

import _pp_glue_ref as R

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
SENT = -7.0
SENT_U8 = 0xA5
GUARD = 64
SIZES = [(5, 7), (37, 53)]


@pytest.fixture(scope="module")
def lib(built_lib, gpu_device):
    return built_lib.lib


def P(t, off=0):
    return C.c_void_p(t.data_ptr() + off * t.element_size())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(n, dtype, fill):
    """a device buffer of GUARD + n + GUARD cells of `fill`; the call gets the cell GUARD"""
    return torch.full((int(n) + 2 * GUARD,), fill, dtype=dtype, device="cuda")


def payload(buf, n, fill, what):
    """the n cells between the guards; the guards must still hold `fill`"""
    a = buf.cpu().numpy()
    assert np.all(a[:GUARD] == fill) and np.all(a[GUARD + n:] == fill), f"{what}: cells around the output were written"
    return a[GUARD:GUARD + n]


def frames_and_mask(seed, n, h, w):
    """uint8 BGR frames whose three channels differ at every pixel (g = b + 85, r = b + 170 mod 256) and a mask of the bytes
    {0, 1, 7, 255}.  The b values run through a permutation of 0..255 separately over the hole pixels and over the others: with 256
    or more pixels of each kind in the batch, every byte value occurs in every channel inside and outside the mask."""
    rng = np.random.default_rng(seed)
    mask = rng.choice(np.array([0, 0, 0, 1, 7, 255], dtype=np.uint8), (h, w))
    hole = np.broadcast_to(mask != 0, (n, h, w))
    b = np.empty((n, h, w), dtype=np.int64)
    for kind in (True, False):
        perm = rng.permutation(256)
        b[hole == kind] = perm[np.arange(int((hole == kind).sum())) % 256]
    bgr = np.stack([b, b + 85, b + 170], axis=-1) % 256
    return bgr.astype(np.uint8), mask


def covers_every_byte(bgr, mask):
    hole = np.broadcast_to((mask != 0)[None, :, :, None], bgr.shape)
    return all(len(np.unique(bgr[..., c][hole[..., c] == kind])) == 256 for c in range(3) for kind in (True, False))


# =====================================================================================================================================
# vsr_pp_prepare_frames / vsr_pp_compose_frames
# =====================================================================================================================================
@pytest.mark.parametrize("h,w", SIZES)
def test_prepare_and_compose(lib, h, w):
    """Planar RGB in [-1, 1] from packed BGR bytes, one [h, w] mask for the n = 3 frames.  x / 255 * 2 - 1 is three correctly
    rounded IEEE operations on both sides (no contraction in the kernel), so the result equals numpy's float32 expression exactly;
    against float64 it is within 2 u: the quotient (<= 1) is rounded once (u / 2), doubled (exact), and the difference (<= 1) is
    rounded once more.  compose gives x outside the mask and prop inside it, exactly (x * 1 + prop * 0 and x * 0 + prop * 1).
    37x53 holds every byte value in every channel on both sides of the mask; 5x7 (105 pixels in all) cannot and checks the rest."""
    n = 3
    bgr, mask = frames_and_mask(10 * h + w, n, h, w)
    assert set(np.unique(mask)) == {0, 1, 7, 255}
    assert h * w < 1000 or covers_every_byte(bgr, mask)
    assert (bgr[..., 0] != bgr[..., 1]).all() and (bgr[..., 1] != bgr[..., 2]).all() and (bgr[..., 0] != bgr[..., 2]).all()
    N = n * 3 * h * w
    d_bgr, d_mask = dev(bgr), dev(mask)
    out = guarded(N, torch.float32, SENT)
    assert lib.vsr_pp_prepare_frames(P(d_bgr), P(d_mask), n, h, w, P(out, GUARD), stream()) == 0
    torch.cuda.synchronize()
    got = payload(out, N, SENT, "prepare").reshape(n, 3, h, w)
    want = R.prepare(bgr, mask, np.float32)
    err = float(np.abs(got - R.prepare(bgr, mask, np.float64)).max())
    print(f"prepare {h}x{w}: {int((got != want).sum())} cells differ from the float32 expression (bound 0); vs float64 {err:.3e} bound {2 * U32:.3e}")
    assert np.array_equal(got, want)
    assert err <= 2 * U32
    hole = mask != 0
    assert np.all(got[:, :, hole] == 0) and np.array_equal(got[:, 0][:, ~hole], (bgr[..., 2].astype(np.float32) / 255 * 2 - 1)[:, ~hole])

    prop = np.random.default_rng(h).uniform(-1, 1, (n, 3, h, w)).astype(np.float32)
    out = guarded(N, torch.float32, SENT)
    d_prop = dev(prop)
    assert lib.vsr_pp_compose_frames(P(d_bgr), P(d_mask), P(d_prop), n, h, w, P(out, GUARD), stream()) == 0
    torch.cuda.synchronize()
    got = payload(out, N, SENT, "compose").reshape(n, 3, h, w)
    x = R.prepare(bgr, np.zeros_like(mask), np.float32)
    print(f"compose {h}x{w}: {int((got != np.where(hole, prop, x)).sum())} cells differ (bound 0)")
    assert np.array_equal(got, np.where(hole, prop, x)) and np.array_equal(got, R.compose(bgr, mask, prop, np.float32))


def test_prepare_and_compose_empty_and_past_the_grid_cap(lib):
    """n = 0 returns 0 and writes nothing; n h w = 3 x 700 x 1000 > 2 097 152 threads of the capped grid: the stride loop's second
    turn, where the frame index and the pixel index come from the same running index"""
    out = guarded(16, torch.float32, SENT)
    byte = guarded(16, torch.uint8, SENT_U8)
    assert lib.vsr_pp_prepare_frames(P(byte), P(byte), 0, 5, 7, P(out, GUARD), stream()) == 0
    assert lib.vsr_pp_compose_frames(P(byte), P(byte), P(out), 0, 5, 7, P(out, GUARD), stream()) == 0
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == SENT)
    n, h, w = 3, 700, 1000
    assert n * h * w > 8192 * 256
    rng = np.random.default_rng(9)
    bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    mask = rng.choice(np.array([0, 0, 1, 7, 255], dtype=np.uint8), (h, w))
    prop = rng.uniform(-1, 1, (n, 3, h, w)).astype(np.float32)
    N = n * 3 * h * w
    d_bgr, d_mask, d_prop = dev(bgr), dev(mask), dev(prop)
    out = guarded(N, torch.float32, SENT)
    assert lib.vsr_pp_prepare_frames(P(d_bgr), P(d_mask), n, h, w, P(out, GUARD), stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(payload(out, N, SENT, "prepare").reshape(n, 3, h, w), R.prepare(bgr, mask, np.float32))
    out = guarded(N, torch.float32, SENT)
    assert lib.vsr_pp_compose_frames(P(d_bgr), P(d_mask), P(d_prop), n, h, w, P(out, GUARD), stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(payload(out, N, SENT, "compose").reshape(n, 3, h, w), R.compose(bgr, mask, prop, np.float32))


# =====================================================================================================================================
# vsr_pp_blend_window
# =====================================================================================================================================
def _blend(lib, pred, d_bgr, d_mask, frame_idx, first, comp, h, w):
    d_pred = dev(pred)
    d_idx, d_first = dev(np.asarray(frame_idx, dtype=np.int32)), dev(np.asarray(first, dtype=np.int32))
    assert lib.vsr_pp_blend_window(P(d_pred), P(d_bgr), P(d_mask), P(d_idx), P(d_first), len(frame_idx), h, w, P(comp, GUARD), stream()) == 0
    torch.cuda.synchronize()


def test_blend_truncation_boundaries(lib):
    """pred = +-1 and float32(2k/255 - 1), k = 0..255, with both fp32 neighbours, in every channel inside the mask: (pred + 1) / 2 *
    255 lands on and next to the integers, where a cast that rounds differs from the reference's truncation (95 of the 256 centre
    values truncate below k in fp32).  Division by 2 is exact and the sum and the product are single roundings: compared bit for bit
    with the float32 restatement.  A second window averages other boundary values onto the first (truncation again)."""
    h, w, n = 37, 53, 2
    v = R.boundary_preds()
    assert len(v) <= h * w and np.abs(v).max() == 1.0
    rng = np.random.default_rng(4)
    bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    mask = rng.choice(np.array([0, 1, 7, 255], dtype=np.uint8), h * w)
    mask[:len(v)] = np.tile(np.array([1, 7, 255], dtype=np.uint8), len(v))[:len(v)]          # the boundary values sit inside the mask
    mask = mask.reshape(h, w)
    preds = []
    for shift in (0, 331):
        p = np.tanh(rng.standard_normal((1, 3, h * w)) * 2).astype(np.float32)               # the rest stays in [-1, 1] as well
        for c in range(3):
            p[0, c, :len(v)] = np.roll(v, shift + 257 * c)
        preds.append(p.reshape(1, 3, h, w))
    d_bgr, d_mask = dev(bgr), dev(mask)
    comp = guarded(n * h * w * 3, torch.uint8, SENT_U8)
    want = np.full((n, h, w, 3), SENT_U8, dtype=np.uint8)
    for p, fst in zip(preds, (1, 0)):
        _blend(lib, p, d_bgr, d_mask, [1], [fst], comp, h, w)
        R.blend_window(p, bgr, mask, [1], [fst], want, np.float32)
        got = payload(comp, n * h * w * 3, SENT_U8, "blend").reshape(n, h, w, 3)
        print(f"blend boundaries first={fst}: {int((got != want).sum())} bytes differ from the float32 restatement (bound 0)")
        assert np.array_equal(got, want)
    rounded = np.rint(R.blend_values(preds[0], np.float32)).astype(np.uint8)[0].transpose(1, 2, 0)[..., ::-1]       # [h, w, BGR]
    trunc = R.blend_window(preds[0], bgr, mask, [0], [1], np.zeros_like(bgr), np.float32)[0]
    share = float((rounded != trunc).reshape(-1, 3)[:len(v)].mean())
    print(f"blend boundaries: a rounding cast would differ on {share:.3f} of the boundary bytes")
    assert share > 0.25, "the boundary values must tell truncation from rounding"


@pytest.mark.parametrize("h,w", SIZES)
def test_blend_three_windows(lib, h, w):
    """Three launches over 6 frames: slots [4, 0, 2] (all first visits, not in frame order), [2, 4, 3] (second visits of 2 and 4 and a
    first visit of 3 in one launch), [4, 1] (frame 4 a third time: ((a + b) // 2 + c) // 2, truncated after each average).  Frame 5
    is never visited.  After every launch the whole of comp -- visited frames inside and outside the mask, unvisited frames, the
    guards -- is compared with the float64 restatement run on a sentinel-filled comp.
    pred = tanh(...) stays in [-1, 1]: the float -> uint8 cast of the kernel (and numpy's astype) is defined only for values in
    [0, 256).  v = (pred + 1) / 2 * 255 carries three fp32 roundings of values <= 255, the first of them scaled by 255 / 2: below
    4 * 255 u; a byte whose |v - rint(v)| is below that is undecided between the two neighbouring integers, and so is what later
    averages make of it (within 1 of the reference).  Their share is capped at 0.1 %."""
    n = 6
    rng = np.random.default_rng(100 + h)
    bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    assert all((bgr[i] != bgr[j]).mean() > 0.9 for i in range(n) for j in range(i))           # indexing by slot instead of frame fails
    mask = rng.choice(np.array([0, 0, 1, 7, 255], dtype=np.uint8), (h, w))
    hole = mask != 0
    d_bgr, d_mask = dev(bgr), dev(mask)
    comp = guarded(n * h * w * 3, torch.uint8, SENT_U8)
    want = np.full((n, h, w, 3), SENT_U8, dtype=np.uint8)
    und = np.zeros((n, h, w, 3), dtype=bool)
    singles = {}
    for launch_no, (idx, first) in enumerate((([4, 0, 2], [1, 1, 1]), ([2, 4, 3], [0, 0, 1]), ([4, 1], [0, 1]))):
        pred = np.tanh(rng.standard_normal((len(idx), 3, h, w)) * 2).astype(np.float32)
        assert np.abs(pred).max() <= 1.0
        _blend(lib, pred, d_bgr, d_mask, idx, first, comp, h, w)
        R.blend_window(pred, bgr, mask, idx, first, want, np.float64)
        v = R.blend_values(pred, np.float64).transpose(0, 2, 3, 1)[..., ::-1]                # [slot, h, w, BGR]
        for k, f in enumerate(idx):
            und[f] |= (np.abs(v[k] - np.rint(v[k])) < 255 * 4 * U32) & hole[:, :, None]
            if f == 4:
                singles[launch_no] = np.where(hole[:, :, None], v[k].astype(np.uint8), bgr[4]).astype(np.int64)
        got = payload(comp, n * h * w * 3, SENT_U8, "blend").reshape(n, h, w, 3)
        d = np.abs(got.astype(np.int64) - want)
        print(f"blend {h}x{w} launch {launch_no}: {int((d != 0)[~und].sum())} decided bytes differ (bound 0), undecided share {und.mean():.2e} "
              f"(cap 1e-3), max |d| on them {int(d[und].max()) if und.any() else 0} (bound 1)")
        assert und.mean() <= 1e-3
        assert np.array_equal(got[~und], want[~und]) and (d[und] <= 1).all()
        assert np.all(got[5] == SENT_U8)
        for k, f in enumerate(idx):
            if first[k]:
                assert np.array_equal(got[f][~hole], bgr[f][~hole]), "outside the mask a first visit copies the frame's own bytes"
    a, b, c = singles[0], singles[1], singles[2]
    ok = ~und[4]
    assert np.array_equal(got[4][ok], (((a + b) // 2 + c) // 2)[ok])


# =====================================================================================================================================
# vsr_launch_absdiff_sums_u8x3
# =====================================================================================================================================
GARBAGE = 0x5A5A5A5A5A5A5A5A
PIX = (1, 63, 255, 257, 2048 * 3 + 5, 1024 * 2048 + 5)       # below a wave, around a block, several blocks, past the 1024-block cap


@pytest.fixture(scope="module")
def absdiff_frames():
    """four frames of the largest size, cut down per case: all 0, all 255 (the largest sums), a copy of it, random"""
    pix = max(PIX)
    f = np.zeros((4, pix, 3), dtype=np.uint8)
    f[1] = 255
    f[2] = 255
    f[3] = np.random.default_rng(12).integers(0, 256, (pix, 3), dtype=np.uint8)
    return f


@pytest.mark.parametrize("pix", PIX)
@pytest.mark.parametrize("npairs", [1, 3])
def test_absdiff_sums(lib, absdiff_frames, npairs, pix):
    """integer sums against int64 numpy.  npairs = 3: all-0 against all-255 (255 pix per plane, the largest sum), two identical
    frames (0), 255 against random; npairs = 1: random against all-255.  sums_dev holds garbage before the call, which zeroes its
    3 npairs words itself; the two words behind them survive."""
    f = absdiff_frames[:4, :pix] if npairs == 3 else absdiff_frames[[3, 1], :pix]
    f = np.ascontiguousarray(f)
    sums = torch.full((npairs * 3 + 2,), GARBAGE, dtype=torch.int64, device="cuda")
    d_f = dev(f)
    assert lib.vsr_launch_absdiff_sums_u8x3(P(d_f), npairs, pix, P(sums), stream()) == 0
    torch.cuda.synchronize()
    got = sums.cpu().numpy()
    want = R.absdiff_sums(f)
    print(f"absdiff sums npairs={npairs} pix={pix}: got {got[:npairs * 3].tolist()} want {want.reshape(-1).tolist()}")
    assert np.array_equal(got[:npairs * 3].reshape(npairs, 3), want)
    assert np.all(got[npairs * 3:] == GARBAGE), "guard words behind the sums were written"
    if npairs == 3:
        assert want[0].tolist() == [255 * pix] * 3 and want[1].tolist() == [0, 0, 0]


def test_absdiff_sums_arguments(lib, built_lib):
    """npairs = 0 returns 0; npairs = 65536 (the grid's y limit), a null pointer and pix = 0 return VSR_ERR_ARG; none of them
    writes"""
    f = dev(np.full((4, 16, 3), 9, dtype=np.uint8))
    sums = torch.full((16,), GARBAGE, dtype=torch.int64, device="cuda")
    null = C.c_void_p(0)
    assert lib.vsr_launch_absdiff_sums_u8x3(P(f), 0, 16, P(sums), stream()) == 0
    for args in ((P(f), 65536, 16, P(sums)), (null, 3, 16, P(sums)), (P(f), 3, 16, null), (P(f), 3, 0, P(sums))):
        assert lib.vsr_launch_absdiff_sums_u8x3(*args, stream()) == built_lib.VSR_ERR_ARG
    torch.cuda.synchronize()
    assert np.all(sums.cpu().numpy() == GARBAGE)
