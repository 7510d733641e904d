"""Plain numpy restatements of ProPainter's image propagation step, of the plugin's glue around the generator and of the scene
detector's difference sums, and the seeded inputs the CPU and GPU tests share.  Host only.

Sources: oracle/propainter.py (flow_warp, fb_check, binary_mask, propagate :85-102 with interp="nearest") and
oracle/propainter_wrapper.py (:49, :67, :82, :94-101).  Every function takes the dtype it computes in: float64 is the reference of the
GPU tests, float32 is what the reference program itself computes in (tests/test_pp_glue_reference.py holds both against the torch
oracle bit for bit).  None of this restates a kernel's loop: sampling is written as whole-array gathers of a zero-padded picture."""
import numpy as np

U32 = 2.0 ** -24            # unit roundoff of fp32


# ---- flow_warp / grid_sample(align_corners=True, padding_mode="zeros") ------------------------------------------------------------------
def warp_coords(flow, dtype):
    """flow [2,h,w] (x, y displacement) -> sampling positions (iy, ix) in pixels, through flow_warp's normalisation to [-1, 1]
    (divided by max(size - 1, 1)) and grid_sample's un-normalisation ((g + 1) / 2 * (size - 1)), each step rounded in `dtype`"""
    dt = np.dtype(dtype).type
    _, h, w = flow.shape
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = []
    for grid, f, size in ((gy, flow[1], h), (gx, flow[0], w)):
        pos = grid.astype(dtype) + f.astype(dtype)
        g = dt(2) * pos / dt(max(size - 1, 1)) - dt(1)
        out.append((g + dt(1)) / dt(2) * dt(size - 1))
    return out[0], out[1]


def _padded(img, pad):
    return np.pad(img, [(0, 0)] * (img.ndim - 2) + [(pad, pad), (pad, pad)])


def gather(img, yy, xx):
    """img [...,h,w] at integer positions (zeros outside)"""
    h, w = img.shape[-2:]
    inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
    v = img[..., np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
    return np.where(inside, v, 0).astype(img.dtype)


def sample_bilinear(img, iy, ix):
    """img [...,h,w] at (iy, ix): the four neighbours weighted by the opposite areas, zeros outside; computes in img's dtype"""
    dt = img.dtype.type
    y0, x0 = np.floor(iy), np.floor(ix)
    ay, ax = (iy - y0).astype(img.dtype), (ix - x0).astype(img.dtype)
    y0, x0 = y0.astype(np.int64), x0.astype(np.int64)
    nw, ne = gather(img, y0, x0), gather(img, y0, x0 + 1)
    sw, se = gather(img, y0 + 1, x0), gather(img, y0 + 1, x0 + 1)
    one = dt(1)
    return nw * ((one - ax) * (one - ay)) + ne * (ax * (one - ay)) + sw * ((one - ax) * ay) + se * (ax * ay)


def sample_nearest(img, iy, ix):
    """grid_sample(mode="nearest"): the position rounded half to even (np.rint), zeros outside"""
    return gather(img, np.rint(iy).astype(np.int64), np.rint(ix).astype(np.int64))


# ---- one step of the non-learnable propagation --------------------------------------------------------------------------------------
def imgprop_step(prev_prop, prev_mask, cur, mcur, fprop, fcheck, first, dtype=np.float64):
    """propagate() :85-102, interp="nearest", learnable=False: prev_prop / cur [C,h,w], prev_mask / mcur [h,w] in {0,1}, flows
    [2,h,w] -> (prop [C,h,w], mprop [h,w], info).  first: prop, mprop = cur, mcur and nothing else is read.

    info: the three decisions (valid, mvalid, union), the sampling positions, and per pixel the margins of every thresholded
    decision: `fb` = |lhs - rhs| of the forward-backward test lhs < rhs with its terms, `mask` = |warped mask - 0.1|, `tie` = the
    distance of the nearest warp's positions from a .5 tie (the smaller of x and y)."""
    dt = np.dtype(dtype).type
    if first:
        return np.array(cur, dtype=dtype), np.array(mcur, dtype=dtype), None
    prev_prop, prev_mask, cur, mcur, fprop, fcheck = (np.asarray(a).astype(dtype) for a in (prev_prop, prev_mask, cur, mcur, fprop, fcheck))
    iy, ix = warp_coords(fprop, dtype)
    # fb_check: the check flow warped by the propagation flow, |f + b|^2 < 0.01 (|f|^2 + |b|^2) + 0.5
    back = sample_bilinear(fcheck, iy, ix)
    diff = fprop + back
    lhs = np.sum(np.square(diff), axis=0)
    rhs = dt(0.01) * (np.sum(np.square(fprop), axis=0) + np.sum(np.square(back), axis=0)) + dt(0.5)
    valid = (lhs < rhs).astype(dtype)
    warped = sample_nearest(prev_prop, iy, ix)
    wmask = sample_bilinear(prev_mask, iy, ix)
    mvalid = (wmask > dt(0.1)).astype(dtype)
    union = (mcur * valid * (dt(1) - mvalid) > dt(0.1)).astype(dtype)
    prop = union * warped + (dt(1) - union) * cur
    mprop = (mcur * (dt(1) - valid * (dt(1) - mvalid)) > dt(0.1)).astype(dtype)
    fy, fx = iy - np.floor(iy), ix - np.floor(ix)
    info = dict(valid=valid, mvalid=mvalid, union=union, warped=warped, iy=iy, ix=ix, back=back, diff=diff, lhs=lhs, rhs=rhs,
                fb=np.abs(lhs - rhs), mask=np.abs(wmask - dt(0.1)), tie=np.minimum(np.abs(fx - 0.5), np.abs(fy - 0.5)),
                tie_x=np.abs(fx - 0.5) == 0, tie_y=np.abs(fy - 0.5) == 0)
    return prop, mprop, info


def _window_stats(img, iy, ix):
    """per pixel: (max - min, max |.|) of the zero-padded img [h,w] over the 4x4 pixels around the bilinear cell of (iy, ix) -- the
    cell and its eight neighbouring cells, which is where a position moved by less than a pixel can land"""
    h, w = img.shape
    pad = 4
    win = np.lib.stride_tricks.sliding_window_view(_padded(img, pad), (4, 4))        # window [i, j] covers padded rows i .. i + 3
    rng_, amax = win.max((2, 3)) - win.min((2, 3)), np.abs(win).max((2, 3))
    yy = np.clip(np.floor(iy).astype(np.int64) - 1 + pad, 0, h + pad)                # clipped far outside: an all-zero window
    xx = np.clip(np.floor(ix).astype(np.int64) - 1 + pad, 0, w + pad)
    return rng_[yy, xx], amax[yy, xx]


def imgprop_bounds(info, prev_mask, fprop, fcheck):
    """How far an fp32 evaluation may move each thresholded expression of imgprop_step away from the float64 one in `info`: a pixel
    whose float64 margin is below its bound is undecided.  Derivation, u = 2^-24:
      * position: x + f, 2 pos / d, - 1, + 1, * (size - 1) are five roundings (/ 2 is exact); in pixel units four of them round a
        value of |pos| and the third one of |pos - (size - 1) / 2| <= |pos| + size: dpos = u (5 |pos| + size) per axis; this is the
        bound of `tie`;
      * a bilinear sample is continuous and piecewise bilinear; its slope per axis inside a cell is a difference of two of the
        cell's corner values, so moving the position by dpos per axis moves it by at most 2 dpos R, R = max - min over the cell and
        its neighbours (_window_stats); the weights (two products) and the four-term sum add 8 u of the largest corner value A:
        eb = 2 dpos R + 8 u A;  with mask values in [0, 1] this is the bound of `mask`;
      * lhs = |f + b|^2 moves by 2 (|dx| + |dy|) eb + 2 eb^2 and rhs by 0.01 (2 (|bx| + |by|) eb + 2 eb^2); the squares, sums, the
        product with 0.01f (itself rounded) and the sum with 0.5 are fewer than 8 roundings of at most lhs + rhs."""
    h, w = info["ix"].shape
    dpos = U32 * np.maximum(5 * np.abs(info["ix"]) + w, 5 * np.abs(info["iy"]) + h)
    rm, am = _window_stats(np.asarray(prev_mask, np.float64), info["iy"], info["ix"])
    bmask = 2 * dpos * rm + 8 * U32 * am
    eb = np.zeros_like(dpos)
    for c in range(2):
        r, a = _window_stats(np.asarray(fcheck[c], np.float64), info["iy"], info["ix"])
        eb = np.maximum(eb, 2 * dpos * r + 8 * U32 * a)
    bfb = (2 * np.abs(info["diff"]).sum(0) * eb + 2 * eb * eb + 0.01 * (2 * np.abs(info["back"]).sum(0) * eb + 2 * eb * eb)
           + 8 * U32 * (info["lhs"] + info["rhs"]))
    return dict(tie=dpos, mask=bmask, fb=bfb)


def imgprop_undecided(info, bounds):
    return (info["tie"] < bounds["tie"]) | (info["mask"] < bounds["mask"]) | (info["fb"] < bounds["fb"])


def imgprop_chain(masked_frames, flows_f, flows_b, masks, dtype=np.float64):
    """img_propagation: backward_1 over the input frames (last frame first, flows_f propagate / flows_b check, flow index = frame
    index), then forward_1 over backward_1's results (flow index = frame index - 1, roles swapped) -> (frames, masks) [t,...]"""
    t = masked_frames.shape[0]
    x, m = [masked_frames[i] for i in range(t)], [masks[i, 0] for i in range(t)]
    for order, fp, fc, shift in ((range(t - 1, -1, -1), flows_f, flows_b, 0), (range(t), flows_b, flows_f, -1)):
        outx, outm = [None] * t, [None] * t
        prop = mprop = None
        for i, idx in enumerate(order):
            k = idx + shift
            prop, mprop, _ = imgprop_step(prop, mprop, x[idx], m[idx], None if i == 0 else fp[k], None if i == 0 else fc[k], i == 0, dtype)
            outx[idx], outm[idx] = prop, mprop
        x, m = outx, outm
    return np.stack(x), np.stack(m)[:, None]


# ---- seeded inputs of one step -------------------------------------------------------------------------------------------------------
DYADIC_SIZES = [(9, 17), (17, 33), (2, 9)]        # h - 1 and w - 1 powers of two: every position and weight is exact in fp32
GENERAL_SIZES = [(13, 22), (45, 75), (2, 3)]
LARGE_SIZE = (1449, 1448)                         # h w = 2 097 152 + 1000: one pixel more than 8192 blocks of 256 threads hold


def step_seed(h, w):
    """the seed of the (h, w) case: the CPU test of the input conditions and the GPU test build the same step (15: also the 18 and
    6 pixels of 2x9 and 2x3 hold ties, in-picture and out-of-picture targets and union pixels, one of them on a tie)"""
    return 15


def _blocks(rng, h, w, size, draw):
    bh, bw = -(-h // size), -(-w // size)
    return np.repeat(np.repeat(draw((bh, bw)), size, axis=0), size, axis=1)[:h, :w], (bh, bw)


def imgprop_inputs(seed, h, w, C, noise, far=True, bad=0.3, check_noise=True):
    """Flows constant on 3x3 blocks, multiples of 1/4 in [-2.5, 2.5]: one draw in [0.75, 2] for the picture, pointing outwards in each
    quadrant (none along an axis shorter than 6), plus one in [-0.5, 0.5] per block, so that neighbouring blocks stay consistent
    often enough.  far: about 8 % of the blocks (where there are 12 or more) are sent w + 1 / h + 1 out of the picture, the sides in
    turn.  fcheck = -fprop, with +2 in x on a share `bad` of the blocks (the forward-backward test fails there).  noise: N(0, noise)
    per pixel on both flows, which leaves no exact tie (check_noise=False: on fprop only).  prev_mask is constant on 2x2 blocks (its
    bilinear warp crosses 0.1 between them), mcur is per pixel; the pictures are uniform in [-1, 1] with no two pixels alike."""
    rng = np.random.default_rng(seed)
    base = rng.integers(3, 9, 2) / 4.0 * (np.array([w, h]) >= 6)              # points out of the picture in every quadrant
    sx = lambda s: np.where(np.arange(s[1]) * 2 >= s[1], 1.0, -1.0)[None, :]
    sy = lambda s: np.where(np.arange(s[0]) * 2 >= s[0], 1.0, -1.0)[:, None]
    bh, bw = -(-h // 3), -(-w // 3)
    bfx = base[0] * sx((bh, bw)) + rng.integers(-2, 3, (bh, bw)) / 4.0
    bfy = base[1] * sy((bh, bw)) + rng.integers(-2, 3, (bh, bw)) / 4.0
    # half of the blocks along the border step 3/4 of a pixel across it and at most 1/4 along it: their outermost pixels have a
    # nearest target outside the picture and still pass the forward-backward test, so the union branch reads the zero padding
    gentle = rng.random((bh, bw)) < 0.5
    along = rng.integers(-1, 2, (bh, bw)) / 4.0
    for rows, cols, nx_, ny_ in ((slice(None), 0, -0.75, None), (slice(None), -1, 0.75, None), (0, slice(None), None, -0.75),
                                 (-1, slice(None), None, 0.75)):
        g = gentle[rows, cols]
        bfx[rows, cols] = np.where(g, along[rows, cols] if nx_ is None else nx_, bfx[rows, cols])
        bfy[rows, cols] = np.where(g, along[rows, cols] if ny_ is None else ny_, bfy[rows, cols])
    fx = np.repeat(np.repeat(bfx, 3, axis=0), 3, axis=1)[:h, :w]
    fy = np.repeat(np.repeat(bfy, 3, axis=0), 3, axis=1)[:h, :w]
    nb = bh * bw
    bx, by = np.zeros(nb), np.zeros(nb)
    for j, b in enumerate(rng.permutation(nb)[:max(1, int(round(0.08 * nb)))] if far and nb >= 12 else ()):
        side = (j + seed) % 4
        bx[b] = (w + 1) * (1 - side) if side in (0, 2) else 0.0            # right, left
        by[b] = (h + 1) * (2 - side) if side in (1, 3) else 0.0            # down, up
    up = lambda v: np.repeat(np.repeat(v.reshape(bh, bw), 3, axis=0), 3, axis=1)[:h, :w]
    fprop = np.stack([fx + up(bx), fy + up(by)])
    bad_blocks, _ = _blocks(rng, h, w, 3, lambda s: rng.random(s) < bad)
    fcheck = -fprop
    fcheck[0] += 2.0 * bad_blocks
    if noise:
        fprop = fprop + rng.normal(0, noise, fprop.shape)
        fcheck = fcheck + rng.normal(0, noise if check_noise else 0.0, fcheck.shape)
    prev_mask, _ = _blocks(rng, h, w, 2, lambda s: (rng.random(s) < 0.3).astype(np.float64))
    mcur = (rng.random((h, w)) < 0.5).astype(np.float64)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(prev_prop=f32(rng.uniform(-1, 1, (C, h, w))), prev_mask=f32(prev_mask), cur=f32(rng.uniform(-1, 1, (C, h, w))),
                mcur=f32(mcur), fprop=f32(fprop), fcheck=f32(fcheck))


def imgprop_shares(inp, info, prop):
    """measured shares of the conditions the tests set on a step's inputs"""
    h, w = inp["mcur"].shape
    ny, nx = np.rint(info["iy"]), np.rint(info["ix"])
    y0, x0 = np.floor(info["iy"]), np.floor(info["ix"])
    tie = info["tie_x"] | info["tie_y"]
    low = np.where(info["tie_x"], np.floor(info["ix"]), np.floor(info["iy"])).astype(np.int64)
    # a tie where rounding half away from zero picks another pixel than half to even does, on a pixel that shows the warped value
    away = lambda v: np.sign(v) * np.floor(np.abs(v) + 0.5)
    tie_union = (info["union"] == 1) & ((away(info["ix"]) != nx) | (away(info["iy"]) != ny))
    combos = {(a, b, c): float(((inp["mcur"] == a) & (info["valid"] == b) & (info["mvalid"] == c)).mean())
              for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    return dict(tie=float(tie.mean()), tie_even=int((tie & (low % 2 == 0)).sum()), tie_odd=int((tie & (low % 2 == 1)).sum()),
                near_out=float(((nx < 0) | (nx > w - 1) | (ny < 0) | (ny > h - 1)).mean()),
                near_sides=[int((nx < 0).sum()), int((nx > w - 1).sum()), int((ny < 0).sum()), int((ny > h - 1).sum())],
                foot_out=float(((x0 < 0) | (x0 + 1 > w - 1) | (y0 < 0) | (y0 + 1 > h - 1)).mean()),
                foot_sides=[int((x0 < 0).sum()), int((x0 + 1 > w - 1).sum()), int((y0 < 0).sum()), int((y0 + 1 > h - 1).sum())],
                combos=combos, union=float(info["union"].mean()), tie_union=int(tie_union.sum()),
                union_out=int(((info["union"] == 1) & ((nx < 0) | (nx > w - 1) | (ny < 0) | (ny > h - 1))).sum()),
                changed=float((np.asarray(prop) != inp["cur"]).any(0).mean()))


def step_conditions(inp, dyadic, oob=True):
    """the conditions the GPU cases of test_gpu_flow_kernels.py set on the inputs of a step, printed and asserted on the float64
    restatement (on the CPU by test_pp_glue_reference.py, and again where the kernel is launched); returns (prop, mprop, info,
    undecided)"""
    h, w = inp["mcur"].shape
    prop, mprop, info = imgprop_step(first=0, dtype=np.float64, **inp)
    s = imgprop_shares(inp, info, prop)
    und = imgprop_undecided(info, imgprop_bounds(info, inp["prev_mask"], inp["fprop"], inp["fcheck"]))
    if dyadic:
        und = und & ~(info["tie_x"] | info["tie_y"])          # an exact tie is decided on this grid: positions carry no rounding
    print(f"imgprop inputs {h}x{w}: ties {s['tie']:.3f} (even {s['tie_even']}, odd {s['tie_odd']}, shown by the union branch "
          f"{s['tie_union']}), nearest out {s['near_out']:.3f} {s['near_sides']}, footprint out {s['foot_out']:.3f} {s['foot_sides']}, "
          f"union {s['union']:.3f} (with its nearest target outside: {s['union_out']}), changed {s['changed']:.3f}, "
          f"undecided {und.mean():.4f}, min margins fb {info['fb'].min():.2e} (rel {(info['fb'] / (info['lhs'] + info['rhs'])).min():.2e}) "
          f"mask {info['mask'].min():.2e}; combos " + " ".join(f"{k}:{v:.3f}" for k, v in s["combos"].items()))
    assert not oob or (s["near_out"] >= 0.05 and s["foot_out"] >= 0.05)
    assert und.mean() <= 0.005, "undecided share"
    if dyadic:
        assert s["tie"] >= 0.20 and s["tie_even"] > 0 and s["tie_odd"] > 0
        assert s["tie_union"] > 0, "no pixel shows which way a tie was rounded"
        assert not und.any(), "a dyadic-grid input has a decision within fp32 rounding of its threshold"
    if h * w > 100:
        assert min(s["near_sides"]) > 0 and min(s["foot_sides"]) > 0, "every side of the picture"
        assert min(s["combos"].values()) >= 0.02, s["combos"]
        assert s["changed"] >= 0.05, "the union branch must change the picture"
        assert s["union_out"] >= 3, "the union branch must read the nearest warp's zero padding"
    return prop, mprop, info, und


def imgprop_clip(seed, t, h, w):
    """a clip for the whole bidirectional propagation on a dyadic grid: frames * (1 - masks) [t,3,h,w], masks [t,1,h,w], flows
    [t-1,2,h,w] from imgprop_inputs (block-constant quarter-pixel flows, no noise)"""
    rng = np.random.default_rng(seed)
    steps = [imgprop_inputs(seed * 100 + i, h, w, 3, 0.0) for i in range(max(t - 1, 1))]
    masks = np.stack([_blocks(rng, h, w, 2, lambda s: (rng.random(s) < 0.45).astype(np.float32))[0] for _ in range(t)])[:, None]
    frames = rng.uniform(-1, 1, (t, 3, h, w)).astype(np.float32)
    ff = np.stack([s["fprop"] for s in steps])[:t - 1]
    fb = np.stack([s["fcheck"] for s in steps])[:t - 1]
    return np.ascontiguousarray(frames * (1 - masks)), np.ascontiguousarray(masks), np.ascontiguousarray(ff), np.ascontiguousarray(fb)


# ---- the plugin's glue (oracle/propainter_wrapper.py) ------------------------------------------------------------------------------
def prepare(bgr, mask, dtype=np.float32):
    """:46, :49, :67: uint8 BGR [n,h,w,3], mask [h,w] (non-zero = hole) -> masked planar RGB frames [n,3,h,w] in [-1, 1]"""
    dt = np.dtype(dtype).type
    rgb = bgr[..., ::-1].transpose(0, 3, 1, 2).astype(dtype)
    frames = rgb / dt(255) * dt(2) - dt(1)
    m = (np.asarray(mask) != 0).astype(dtype)[None, None]
    return frames * (dt(1) - m)


def compose(bgr, mask, prop, dtype=np.float32):
    """:82: frames * (1 - masks_dilated) + prop * masks_dilated"""
    dt = np.dtype(dtype).type
    rgb = bgr[..., ::-1].transpose(0, 3, 1, 2).astype(dtype)
    frames = rgb / dt(255) * dt(2) - dt(1)
    m = (np.asarray(mask) != 0).astype(dtype)[None, None]
    return frames * (dt(1) - m) + np.asarray(prop).astype(dtype) * m


def blend_window(pred, bgr, mask, frame_idx, first, comp, dtype=np.float32):
    """:94-101 for one window: pred [lt,3,h,w] in [-1, 1] (planar RGB), bgr [n,h,w,3] uint8, comp [n,h,w,3] uint8 in BGR (changed in
    place, as the wrapper's list is).  Slot k goes to frame frame_idx[k]; first[k]: the slot's picture replaces the frame, else
    comp = (comp.astype(f32) * 0.5 + img.astype(f32) * 0.5).astype(uint8) -- truncation after every average.  The wrapper works in
    RGB and swaps back at the end (:102); so does this."""
    dt = np.dtype(dtype).type
    binary = (np.asarray(mask) != 0).astype(np.uint8)[:, :, None]
    p = ((np.asarray(pred).astype(dtype) + dt(1)) / dt(2)).transpose(0, 2, 3, 1) * dt(255)
    for k, idx in enumerate(frame_idx):
        img = p[k].astype(np.uint8) * binary + bgr[idx][:, :, ::-1] * (1 - binary)
        if first[k]:
            out = img
        else:
            out = (comp[idx][:, :, ::-1].astype(np.float32) * np.float32(0.5) + img.astype(np.float32) * np.float32(0.5)).astype(np.uint8)
        comp[idx] = out[:, :, ::-1]
    return comp


def blend_values(pred, dtype=np.float64):
    """(pred + 1) / 2 * 255 before the cast, for the undecided band of the GPU test"""
    dt = np.dtype(dtype).type
    return (np.asarray(pred).astype(dtype) + dt(1)) / dt(2) * dt(255)


def boundary_preds():
    """exactly +-1 and, for k = 0..255, float32(2k/255 - 1) with both fp32 neighbours, kept inside [-1, 1]"""
    c = (2.0 * np.arange(256) / 255.0 - 1.0).astype(np.float32)
    v = np.concatenate([[-1.0, 1.0], c, np.nextafter(c, np.float32(-2)), np.nextafter(c, np.float32(2))]).astype(np.float32)
    return v[np.abs(v) <= 1.0]


def absdiff_sums(frames):
    """uint8 [n,pix,3] -> int64 [n-1,3]: per consecutive pair and plane the sum of |difference|"""
    f = np.asarray(frames).astype(np.int64)
    return np.abs(f[1:] - f[:-1]).sum(axis=1)
