"""--logo-unblend: the translucent overlays --logo-scan found are un-mixed instead of inpainted (not in the reference; opt-in, DESIGN
4.20; the numpy statement is tests/_unmix_statement.py).

A station logo is mostly translucent: I = (1 - a) B + a L, and the picture B is still in the pixel.  Per pixel of a found area the gain
g = 1 - a (Q8, 256 = no overlay) and the offset o = a L (Q4) are estimated from the M frames the scan sampled: the variance of I over time
is g^2 times the variance of the moving picture, which the ring around the area shows unmixed, and the mean of I is g times the ring's
mean plus o.  One level is pooled over the area (a logo has one opacity), the scan's own measure checks that the un-mixed samples show no
overlay any more, and every plugin call then ends by writing B = (I - o) / g of its source into the pixels of the accepted areas with
g >= 64 / 256; the fill stays only under the opaque part.  An area that is refused -- "still" (the ring does not move), "none" (no pixel
with g < 232), "faint" (level above 216), "shows" (the gate), "text" (it meets a box of the text detector or of -c) -- is inpainted as
without the option.

    1. vsr_unmix_accum: one launch per piece of the sampled frames the scan kept on the device, two uint32 planes over the grown area,
    2. solve(): histogram, level and medians on the host, on planes of at most a ninth of a frame, once per run,
    3. vsr_unmix_apply + vsr_static_accum on the grown area cut out of the sampled frames: the gate,
    4. vsr_unmix_apply in every plugin call (tools/seam_feather.py), behind every other pass: an un-mixed pixel is real picture.

Off (the default): nothing here is called but unblend_option, no launch, no clone, no byte written that was not before.  The option is
read here and nowhere else (unblend_option: --logo-unblend sets VSR_LOGO_UNBLEND=1).  It needs --logo-scan (refuse), which refuses
several ranks.  The plans of a run live in a process-wide registry that SubtitleRemover.run() sets and clears and the pass reads.
"""
import ctypes as C
import os

import numpy as np

from . import logo_scan

ENV = "VSR_LOGO_UNBLEND"
RING = logo_scan.RING
GMIN, GMAX = 64, 512                        # gains below GMIN are opaque; the estimate is capped at GMAX
BAND, HIST_BELOW, FAINT, STILL = 24, 232, 216, 16
MAX_TOTAL = 65535                           # frames a sum of squares takes in 32 bits

stats = {"plans": 0, "refused": 0, "accum_launches": 0, "applies": 0}


def unblend_option(value=None, env=None):
    """whether this run un-mixes: `value`, None = the environment (VSR_LOGO_UNBLEND, unset, empty or 0 = off, 1 = on).  The one reading
    of the option.  ValueError for anything else."""
    env = os.environ if env is None else env
    if value is None:
        value = env.get(ENV, "0") or "0"
    if isinstance(value, bool):
        return value
    if str(value).strip() in ("0", "1"):
        return str(value).strip() == "1"
    raise ValueError(f"logo unblend: {value!r} is neither 0 nor 1")


def refuse(unblend=None, scan=None):
    """-> whether this run un-mixes.  On without --logo-scan raises ValueError before any work: there is no area to un-mix (several ranks
    are refused by the scan)."""
    on = unblend_option(unblend)
    if on and not logo_scan.scan_option(scan):
        raise ValueError(f"--logo-unblend / {ENV} = 1 un-mixes the areas --logo-scan / {logo_scan.ENV} finds, and that is off: "
                         "give both or neither")
    return on


def grown_box(box, H, W):
    y0, y1, x0, x1 = box
    return max(y0 - RING, 0), min(y1 + RING, H), max(x0 - RING, 0), min(x1 + RING, W)


def meets(box, other):
    """whether two (ymin, ymax, xmin, xmax) rectangles share a pixel"""
    return max(box[0], other[0]) < min(box[1], other[1]) and max(box[2], other[2]) < min(box[3], other[3])


def _isqrt(x):
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > x, r - 1, r)
    return np.where((r + 1) * (r + 1) <= x, r + 1, r)


def _middle(values):
    v = np.sort(np.asarray(values, np.int64).ravel())
    return int(v[len(v) // 2])


def solve(S1, S2, M, box, gbox):
    """the host part: the moments over Gbox ([gh,gw,3] each, any integer type) -> (g uint16 [bh,bw], o int16 [bh,bw,3], level) or the
    reason of the refusal, a string"""
    y0, y1, x0, x1 = box
    gy0, _, gx0, _ = gbox
    S1, S2, M = np.asarray(S1).astype(np.int64), np.asarray(S2).astype(np.int64), int(M)
    V = (M * S2 - S1 * S1).sum(axis=2)
    inner = (slice(y0 - gy0, y1 - gy0), slice(x0 - gx0, x1 - gx0))
    nr = V.size - V[inner].size
    if nr == 0:
        return "still"
    vbar = int(V.sum() - V[inner].sum()) // nr
    if vbar < STILL * M * M:
        return "still"
    mr = (16 * (S1.sum(axis=(0, 1)) - S1[inner].sum(axis=(0, 1))) + (nr * M) // 2) // (nr * M)
    g = _isqrt(np.minimum((V[inner] << 16) // vbar, GMAX * GMAX))
    mI = (16 * S1[inner] + M // 2) // M
    hist = np.bincount(g[g < HIST_BELOW], minlength=GMAX + 1)
    if hist.sum() == 0:
        return "none"
    cum = np.concatenate(([0], np.cumsum(hist)))
    v = np.arange(GMAX + 1)
    pooled = cum[np.minimum(v + BAND, GMAX) + 1] - cum[np.maximum(v - BAND, 0)]
    first = int(np.argmax(pooled))
    lvl = _middle(g[np.abs(g - first) <= BAND])
    if lvl > FAINT:
        return "faint"
    level = np.abs(g - lvl) <= BAND
    clear = (np.abs(g - 256) <= BAND) & ~level
    gt = np.where(level, lvl, np.where(clear, 256, g))
    ot = mI - ((g[..., None] * mr + 128) >> 8)
    flat = mI[level] - ((lvl * mr + 128) >> 8)
    ot[level] = [_middle(flat[:, ch]) for ch in range(3)]
    ot[clear] = 0
    return gt.astype(np.uint16), ot.astype(np.int16), lvl


class Plan:
    """one accepted area: box (ymin, ymax, xmin, xmax) in a picture of H x W, the gain (uint16 [bh,bw], kept as int16 storage) and the
    offset (int16 [bh,bw,3]) on the device, and the level"""

    def __init__(self, box, H, W, g16, o16, level):
        self.box, self.H, self.W, self.g16, self.o16, self.level = tuple(int(b) for b in box), int(H), int(W), g16, o16, int(level)
        self.box_c = (C.c_int32 * 4)(*self.box)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stride(frames):
    return frames.stride(0) if frames.shape[0] > 1 else int(np.prod(frames.shape[1:]))


def unmix(frames, src, plan, y0=0, H=None):
    """in place on `frames` (uint8 [n,h,W,3] on the GPU, every frame contiguous: the rows [y0, y0 + h) of a picture of H rows, None: of
    the plan's) from `src` (same shape, its own frame stride; `frames` itself is allowed): one vsr_unmix_apply on the current stream"""
    import torch

    from ..._lib import check, lib

    n, h, W, _ = frames.shape
    H = plan.H if H is None else int(H)
    for t in (frames, src):
        assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (n, h, W, 3)
        assert t.stride(3) == 1 and t.stride(2) == 3 and t.stride(1) == 3 * W, "every frame must be contiguous [h,W,3]"
    assert plan.g16.device == frames.device == src.device and 0 <= y0 and y0 + h <= H
    bh, bw = plan.box[1] - plan.box[0], plan.box[3] - plan.box[2]
    assert tuple(plan.g16.shape) == (bh, bw) and tuple(plan.o16.shape) == (bh, bw, 3)
    with torch.cuda.device(frames.device):
        stream = torch.cuda.current_stream(frames.device)
        for t in (plan.g16, plan.o16):
            t.record_stream(stream)          # (made once per run, on whichever stream made the plans)
        check(lib.vsr_unmix_apply(_p(frames), _stride(frames), _p(src), _stride(src), _p(plan.g16), _p(plan.o16), n, H, W, int(y0), h,
                                  plan.box_c, C.c_void_p(stream.cuda_stream)))
    stats["applies"] += 1
    return frames


def apply(frames, src, plans, y0=0, H=None):
    """the pass of a plugin call: every plan's area un-mixed from `src` into `frames` (the rows [y0, y0 + h) of a picture of H rows)"""
    n, h, W, _ = frames.shape
    for plan in plans:
        assert plan.W == W and (H is None or plan.H == H), \
            f"a plan for a picture of {plan.H} x {plan.W} in a call on one of {H} x {W}"
        if n and min(plan.box[1], y0 + h) > max(plan.box[0], y0):
            unmix(frames, src, plan, y0=y0, H=H)
    return frames


class Moments:
    """S1 = sum F and S2 = sum F^2 over Gbox on one device; feed() takes sampled frames in any pieces"""

    def __init__(self, H, W, gbox, device):
        import torch

        self.H, self.W, self.gbox, self.fed = int(H), int(W), tuple(int(b) for b in gbox), 0
        shape = (self.gbox[1] - self.gbox[0], self.gbox[3] - self.gbox[2], 3)
        self.S1 = torch.empty(shape, dtype=torch.int32, device=device)       # (uint32 to the kernel)
        self.S2 = torch.empty(shape, dtype=torch.int32, device=device)

    def feed(self, frames, idx=None):
        """frames: uint8 [k,H,W,3] on the device, every frame contiguous; idx: the numbers (into `frames`) of the frames to take, None =
        all of them.  One launch on the current stream.  More than 65535 frames in all are refused: S2 could overflow."""
        import torch

        from ..._lib import check, lib

        k = int(frames.shape[0])
        idx = list(range(k)) if idx is None else [int(i) for i in idx]
        if not idx:
            return
        if self.fed + len(idx) > MAX_TOTAL:
            raise ValueError(f"logo unblend: {self.fed + len(idx)} frames in one sum, at most {MAX_TOTAL} are possible")
        assert frames.dtype == torch.uint8 and frames.device == self.S1.device and tuple(frames.shape[1:]) == (self.H, self.W, 3)
        assert frames.stride(3) == 1 and frames.stride(2) == 3 and frames.stride(1) == 3 * self.W, "every frame must be contiguous [H,W,3]"
        assert min(idx) >= 0 and max(idx) < k, "a sampled frame outside the frames given"
        with torch.cuda.device(frames.device):
            idx_dev = torch.tensor(idx, dtype=torch.int32, device=frames.device)
            stream = C.c_void_p(torch.cuda.current_stream(frames.device).cuda_stream)
            check(lib.vsr_unmix_accum(_p(frames), _stride(frames), _p(idx_dev), len(idx), self.H, self.W, *self.gbox,
                                      0 if self.fed else 1, _p(self.S1), _p(self.S2), stream))
        self.fed += len(idx)
        stats["accum_launches"] += 1

    def host(self):
        """-> (S1, S2) uint32 [gh,gw,3] on the host"""
        return self.S1.cpu().numpy().view(np.uint32), self.S2.cpu().numpy().view(np.uint32)


def seeds_left(pieces, plan, gbox):
    """the gate: the grown area cut out of the sampled frames, un-mixed in place (opaque pixels keep the source) and run through the
    scan's vsr_static_accum -> the pixels of the box that still have an edge in M - M // 8 of the M samples.  (The gradient reaches one
    pixel, the ring 24: the cut's border is the frame's or lies outside the gradient's reach from the box.)"""
    import torch

    gy0, gy1, gx0, gx1 = gbox
    y0, y1, x0, x1 = plan.box
    cut_plan = Plan((y0 - gy0, y1 - gy0, x0 - gx0, x1 - gx0), gy1 - gy0, gx1 - gx0, plan.g16, plan.o16, plan.level)
    state = logo_scan.Scan(gy1 - gy0, gx1 - gx0, plan.g16.device)
    for frames, idx in pieces:
        with torch.cuda.device(frames.device):
            cut = frames[torch.tensor(idx, dtype=torch.long, device=frames.device), gy0:gy1, gx0:gx1].contiguous()
        unmix(cut, cut, cut_plan)
        state.feed(cut)
    M = state.fed
    e = state.edges.cpu().numpy().view(np.uint16)[y0 - gy0:y1 - gy0, x0 - gx0:x1 - gx0]
    return int((e >= M - M // 8).sum())


def make_plans(scan, areas, text_boxes=()):
    """-> (plans, refusals): the accepted areas as Plan objects and [(area, reason)] of the others.  scan: a logo_scan.Scan that kept
    its sampled frames on the device (keep=True); areas, text_boxes: (ymin, ymax, xmin, xmax) rectangles -- an area that meets a text
    box is refused as "text" without any work."""
    import torch

    plans, refusals = [], []
    text_boxes = [tuple(int(v) for v in b) for b in text_boxes]
    for area in areas:
        area = tuple(int(v) for v in area)
        if any(meets(area, b) for b in text_boxes):
            refusals.append((area, "text"))
            continue
        gbox = grown_box(area, scan.H, scan.W)
        mom = Moments(scan.H, scan.W, gbox, scan.device)
        for frames, idx in scan.pieces:
            mom.feed(frames, idx)
        solved = solve(*mom.host(), mom.fed, area, gbox) if mom.fed else "still"
        if isinstance(solved, str):
            refusals.append((area, solved))
            continue
        g, o, lvl = solved
        plan = Plan(area, scan.H, scan.W, torch.from_numpy(g.view(np.int16)).to(scan.device), torch.from_numpy(o).to(scan.device), lvl)
        plan.seeds = seeds_left(scan.pieces, plan, gbox)
        if plan.seeds:
            refusals.append((area, "shows"))
            continue
        plans.append(plan)
    stats["plans"] += len(plans)
    stats["refused"] += len(refusals)
    return plans, refusals


# ---- the plans of the run: set and cleared by SubtitleRemover.run(), read by the pass (tools/seam_feather.py) ---------------------
_plans = []


def register(plans):
    _plans[:] = list(plans)


def clear():
    del _plans[:]


def active():
    """the plans the pass of a plugin call un-mixes: none with the option off or outside a run"""
    return list(_plans)
