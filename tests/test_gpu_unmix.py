"""--logo-unblend on the MI355X: the two kernels of csrc/unmix_kernels.hip against tests/_unmix_statement.py byte for
byte, and backend/tools/unblend.make_plans against the statement's `plan` on the clips of the design's table."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import _static_statement as st
from tests import _unmix_statement as us

pytestmark = pytest.mark.gpu

SLACK = 5                                                  # bytes between two frames: every frame at another alignment
K = 19
# (H, W, box): a 40 x 70 frame with the box in a corner, so the ring is clipped at the top and at the right; a grown box of 69 rows
# (no multiple of the 4 a workgroup owns) and 208 columns = 624 bytes a row (two runs of 256 and a rest)
SHAPES = {"corner": (40, 70, (2, 14, 50, 68)), "wide": (90, 300, (30, 51, 40, 200))}


def p(t):
    return C.c_void_p(t.data_ptr())


class Case:
    def __init__(self, H, W, box, device):
        self.H, self.W, self.box, self.gbox = H, W, box, us.grown_box(box, H, W)
        self.host = np.random.default_rng(H * 1000 + W).integers(0, 256, size=(K, H, W, 3), dtype=np.uint8)
        self.order = [int(i) for i in np.random.default_rng(7).permutation(K)]      # unordered
        self.host[self.order[0]] = 255                     # the largest square there is, in every byte of a frame every call takes
        self.stride = H * W * 3 + SLACK
        flat = np.zeros(K * self.stride, np.uint8)
        for f in range(K):
            flat[f * self.stride:f * self.stride + H * W * 3] = self.host[f].ravel()
        self.dev = torch.from_numpy(flat).to(device)

    def planes(self):
        gy0, gy1, gx0, gx1 = self.gbox
        return tuple(torch.full((gy1 - gy0, gx1 - gx0, 3), v, dtype=torch.int32, device=self.dev.device) for v in (7, 9))

    def accum(self, lib, idx, first, state):
        from vsr_amd._lib import check

        idx_dev = torch.tensor(idx, dtype=torch.int32, device=self.dev.device)
        check(lib.vsr_unmix_accum(p(self.dev), self.stride, p(idx_dev), len(idx), self.H, self.W, *self.gbox, first, p(state[0]), p(state[1]), None))
        torch.cuda.synchronize()
        return tuple(s.cpu().numpy().view(np.uint32).astype(np.int64) for s in state)


@pytest.fixture(scope="module")
def cases(built_lib, gpu_device):
    return {name: Case(*shape, gpu_device) for name, shape in SHAPES.items()}


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("n", [1, 2, 17])
def test_accumulate_equals_the_statement(built_lib, gpu_device, cases, name, n):
    case = cases[name]
    if name == "corner":
        assert case.gbox == (0, 38, 26, 70), "clipped at two sides"
    idx = case.order[:n]
    assert n < 3 or idx != sorted(idx), "unordered frame numbers"
    got = case.accum(built_lib.lib, idx, 1, case.planes())           # (first = 1 overwrites whatever the planes held)
    want = us.moments((case.host[i] for i in idx), case.gbox)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", list(SHAPES))
def test_two_calls_equal_one(built_lib, gpu_device, cases, name):
    case = cases[name]
    idx = case.order[:17]
    state = case.planes()
    case.accum(built_lib.lib, idx[:9], 1, state)
    got = case.accum(built_lib.lib, idx[9:], 0, state)
    want = us.moments((case.host[i] for i in idx), case.gbox)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    one = case.accum(built_lib.lib, idx, 1, case.planes())
    assert np.array_equal(one[0], got[0]) and np.array_equal(one[1], got[1])


def test_the_moments_object_refuses_more_than_65535_frames(built_lib, gpu_device):
    from vsr_amd.backend.tools import unblend

    frames = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=gpu_device)
    mom = unblend.Moments(8, 8, (0, 8, 0, 8), frames.device)
    mom.feed(frames)
    mom.fed = unblend.MAX_TOTAL - 1
    with pytest.raises(ValueError, match="65535"):
        mom.feed(frames)


# ---- vsr_unmix_apply ------------------------------------------------------------------------------------------------------------------
GAINS = (63, 64, 65, 255, 256, 257, 512)
AH, AW, ABOX, AN = 50, 90, (7, 38, 11, 80), 3


@pytest.fixture(scope="module")
def apply_case(built_lib, gpu_device):
    rng = np.random.default_rng(21)
    bh, bw = ABOX[1] - ABOX[0], ABOX[3] - ABOX[2]
    gt = rng.choice(GAINS, size=(bh, bw)).astype(np.int64)
    ot = rng.integers(-8160, 4081, size=(bh, bw, 3)).astype(np.int64)
    ot[rng.random((bh, bw)) < 0.2] = -8160
    ot[rng.random((bh, bw)) < 0.2] = 4080
    ot[rng.random((bh, bw)) < 0.2] = 0
    src = rng.integers(0, 256, size=(AN, AH, AW, 3), dtype=np.uint8)
    src[0][rng.random((AH, AW)) < 0.5] = 0
    src[1][rng.random((AH, AW)) < 0.5] = 255
    fill = rng.integers(0, 256, size=(AN, AH, AW, 3), dtype=np.uint8)
    want = np.stack([us.unmix(f.copy(), s, gt, ot, ABOX) for f, s in zip(fill, src)])
    inside = want[:, ABOX[0]:ABOX[1], ABOX[2]:ABOX[3]]
    assert (inside[:, gt >= 64] == 0).any() and (inside[:, gt >= 64] == 255).any(), "both clamps fire"
    for g in GAINS:
        assert (gt == g).sum() > 50
    g16 = torch.from_numpy(gt.astype(np.uint16).view(np.int16)).to(gpu_device)
    o16 = torch.from_numpy(ot.astype(np.int16)).to(gpu_device)
    return types.SimpleNamespace(gt=gt, ot=ot, src=src, fill=fill, want=want, g16=g16, o16=o16, box=(C.c_int32 * 4)(*ABOX))


def run_apply(lib, case, frames, src, y0, rows, H=AH, g16=None, o16=None):
    from vsr_amd._lib import check

    n = frames.shape[0]
    check(lib.vsr_unmix_apply(p(frames), frames.stride(0), p(src), src.stride(0), p(case.g16 if g16 is None else g16),
                              p(case.o16 if o16 is None else o16), n, H, AW, y0, rows, case.box, None))
    torch.cuda.synchronize()
    return frames.cpu().numpy()


def test_apply_equals_the_statement(built_lib, gpu_device, apply_case):
    c = apply_case
    frames, src = torch.from_numpy(c.fill).to(gpu_device), torch.from_numpy(c.src).to(gpu_device)
    got = run_apply(built_lib.lib, c, frames, src, 0, AH)
    assert np.array_equal(got, c.want), f"{int((got != c.want).sum())} bytes differ from the statement"
    opaque = np.zeros((AH, AW), bool)
    opaque[ABOX[0]:ABOX[1], ABOX[2]:ABOX[3]] = c.gt < 64
    assert opaque.any() and np.array_equal(got[:, opaque], c.fill[:, opaque]), "an opaque pixel keeps the fill"
    outside = np.ones((AH, AW), bool)
    outside[ABOX[0]:ABOX[1], ABOX[2]:ABOX[3]] = False
    assert np.array_equal(got[:, outside], c.fill[:, outside]), "nothing outside the box is written"
    assert np.array_equal(src.cpu().numpy(), c.src), "the source is read only"


def test_gain_256_and_offset_0_is_the_identity(built_lib, gpu_device, apply_case):
    c = apply_case
    bh, bw = ABOX[1] - ABOX[0], ABOX[3] - ABOX[2]
    g16 = torch.full((bh, bw), 256, dtype=torch.int16, device=gpu_device)
    o16 = torch.zeros((bh, bw, 3), dtype=torch.int16, device=gpu_device)
    frames, src = torch.from_numpy(c.fill).to(gpu_device), torch.from_numpy(c.src).to(gpu_device)
    got = run_apply(built_lib.lib, c, frames, src, 0, AH, g16=g16, o16=o16)
    want = c.fill.copy()
    want[:, ABOX[0]:ABOX[1], ABOX[2]:ABOX[3]] = c.src[:, ABOX[0]:ABOX[1], ABOX[2]:ABOX[3]]
    assert np.array_equal(got, want), "the box holds the source's bytes"


@pytest.mark.parametrize("rows", [(5, 20), (20, 45), (10, 30), (37, 50), (0, 8)])
def test_strips_that_cut_the_box(built_lib, gpu_device, apply_case, rows):
    c = apply_case
    lo, hi = rows
    frames = torch.from_numpy(np.ascontiguousarray(c.fill[:, lo:hi])).to(gpu_device)
    src = torch.from_numpy(np.ascontiguousarray(c.src[:, lo:hi])).to(gpu_device)
    got = run_apply(built_lib.lib, c, frames, src, lo, hi - lo)
    assert np.array_equal(got, c.want[:, lo:hi]), "the rows of the full-frame result"
    own = np.stack([us.unmix(f.copy(), s, c.gt, c.ot, ABOX, y0=lo) for f, s in zip(c.fill[:, lo:hi], c.src[:, lo:hi])])
    assert np.array_equal(got, own), "and the strip's own statement"


@pytest.mark.parametrize("rows", [(0, 7), (38, 50)])
def test_a_box_outside_the_rows_writes_nothing(built_lib, gpu_device, apply_case, rows):
    c = apply_case
    lo, hi = rows
    frames = torch.from_numpy(np.ascontiguousarray(c.fill[:, lo:hi])).to(gpu_device)
    src = torch.from_numpy(np.ascontiguousarray(c.src[:, lo:hi])).to(gpu_device)
    got = run_apply(built_lib.lib, c, frames, src, lo, hi - lo)
    assert np.array_equal(got, c.fill[:, lo:hi])


def test_in_place_on_the_source(built_lib, gpu_device, apply_case):
    c = apply_case
    frames = torch.from_numpy(c.src).to(gpu_device)
    got = run_apply(built_lib.lib, c, frames, frames, 0, AH)
    want = np.stack([us.unmix(s.copy(), s, c.gt, c.ot, ABOX) for s in c.src])
    assert np.array_equal(got, want), "src == frames: opaque pixels keep the source, the others are un-mixed from it"


# ---- make_plans ---------------------------------------------------------------------------------------------------------------------------
def scan_of(clip, device, batch=16):
    """a scan that kept its sampled frames, fed as the reading pass feeds it (batches) or as a resident clip does (batch = None)"""
    from vsr_amd.backend.tools import logo_scan

    idx = st.sample_indices(len(clip))
    scan = logo_scan.Scan(clip.shape[1], clip.shape[2], device, keep=True)
    if batch is None:
        scan.feed(torch.from_numpy(clip).to(device), idx)
    else:
        for i in range(0, len(idx), batch):
            scan.feed(torch.from_numpy(np.ascontiguousarray(clip[idx[i:i + batch]])).to(device))
    scan.found = scan.areas()
    return scan


@pytest.mark.parametrize("name", ["a64", "a128 resident", "a224", "opaque", "still", "plain", "texture"])
def test_make_plans_equals_the_statement(built_lib, gpu_device, name):
    from vsr_amd.backend.tools import unblend

    if name == "texture":
        rng = np.random.default_rng(11)
        off = [(int(rng.integers(0, 1024 - st.CLIP_H)), int(rng.integers(0, 1024 - st.CLIP_W))) for _ in range(120)]
        clip = us.blend(us.crops(us.texture(), off), 96)
    else:
        clip = {"a64": lambda: us.blend(st.wave(), 64), "a128 resident": lambda: us.blend(st.wave(), 128),
                "a224": lambda: us.blend(st.wave(), 224), "opaque": st.clip_logo, "still": lambda: us.blend(st.wave(still=True), 128),
                "plain": st.wave}[name]()
    scan = scan_of(clip, gpu_device, batch=None if "resident" in name else 16)
    areas = [st.LOGO_AREA]
    if name not in ("still", "plain"):
        assert scan.found == areas
    before = dict(unblend.stats)
    plans, refusals = unblend.make_plans(scan, areas)
    want = us.plan([clip[i] for i in st.sample_indices(len(clip))], st.LOGO_AREA)
    if isinstance(want, str):
        assert plans == [] and refusals == [(st.LOGO_AREA, want)]
        assert want == {"a224": "shows", "opaque": "shows", "still": "still", "plain": "none"}[name]
    else:
        assert refusals == [] and len(plans) == 1 and plans[0].box == st.LOGO_AREA and plans[0].seeds == 0
        assert np.array_equal(plans[0].g16.cpu().numpy().view(np.uint16), want[0])
        assert np.array_equal(plans[0].o16.cpu().numpy(), want[1])
        pieces = 1 if "resident" in name else -(-len(st.sample_indices(len(clip))) // 16)
        assert unblend.stats["accum_launches"] == before["accum_launches"] + pieces
        # the pass of a plugin call on these plans: the statement's frames
        t = torch.from_numpy(clip[:3].copy()).to(gpu_device)
        fill = torch.full_like(t, 9)
        unblend.apply(fill, t, plans, H=clip.shape[1])
        torch.cuda.synchronize()
        y0, y1, x0, x1 = st.LOGO_AREA
        want_frames = np.full_like(clip[:3], 9)
        for f, s in zip(want_frames, clip[:3]):
            us.unmix(f, s, want[0], want[1], st.LOGO_AREA)
        assert np.array_equal(fill.cpu().numpy(), want_frames)
