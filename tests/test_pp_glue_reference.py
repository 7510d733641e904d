"""tests/_pp_glue_ref.py against the torch oracle and the reference wrapper's own lines, on the CPU: the restatements the GPU tests
(test_gpu_flow_kernels.py, test_gpu_pp_glue.py, test_gpu_pp.py) compare the kernels with are the reference's operations, and the
seeded inputs of those tests reach every branch they are meant to reach -- a generator that stops doing so fails here."""
import numpy as np
import pytest
import torch

import _pp_glue_ref as R
from oracle.make_golden import propainter_inputs
from oracle.propainter import ProPainterOracle, binary_mask, fb_check, flow_warp

IMGPROP_CASES = [(h, w, 0.0) for h, w in R.DYADIC_SIZES] + [(h, w, 0.2) for h, w in R.GENERAL_SIZES] + [(13, 22, 0.0), (37, 53, 0.0),
                                                                                                       (37, 53, 0.2), (45, 75, 0.0)]


def oracle_step(inp, tdtype):
    """propagate() :92-102 with interp="nearest", from the oracle's own functions"""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(tdtype)
    prop, mprop, cur, mcur = t(inp["prev_prop"])[None], t(inp["prev_mask"])[None, None], t(inp["cur"])[None], t(inp["mcur"])[None, None]
    fp, fc = t(inp["fprop"])[None], t(inp["fcheck"])[None]
    valid = fb_check(fp, fc)
    warped = flow_warp(prop, fp.permute(0, 2, 3, 1), "nearest")
    mvalid = binary_mask(flow_warp(mprop, fp.permute(0, 2, 3, 1)))
    union = binary_mask(mcur * valid * (1 - mvalid))
    return (union * warped + (1 - union) * cur)[0].numpy(), binary_mask(mcur * (1 - (valid * (1 - mvalid))))[0, 0].numpy()


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("h,w,noise", IMGPROP_CASES)
def test_imgprop_step_equals_the_oracle(h, w, noise, C):
    """float32 and float64 restatements equal the oracle's step in the same dtype bit for bit; and each other where no position
    sits within rounding of a tie"""
    inp = R.imgprop_inputs(1000 + 10 * h + w + C, h, w, C, noise)
    outs = {}
    for dt, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        prop, mprop, _ = R.imgprop_step(first=0, dtype=dt, **inp)
        want, wantm = oracle_step(inp, tdt)
        dp, dm = int((prop != want).any(0).sum()), int((mprop != wantm).sum())
        print(f"imgprop step {h}x{w} C={C} noise {noise} {np.dtype(dt).name}: {dp} pixels, {dm} mask cells differ from the oracle")
        assert prop.dtype == dt and dp == 0 and dm == 0
        outs[dt] = (prop, mprop)
    if noise or (h, w) in R.DYADIC_SIZES:      # quarter-pixel flows on another grid sit on .5 ties that rounding of the positions decides
        assert np.array_equal(outs[np.float32][0], outs[np.float64][0]) and np.array_equal(outs[np.float32][1], outs[np.float64][1])


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("h,w", R.DYADIC_SIZES + R.GENERAL_SIZES)
def test_imgprop_inputs_reach_every_branch(h, w, C):
    dyadic = (h, w) in R.DYADIC_SIZES
    R.step_conditions(R.imgprop_inputs(R.step_seed(h, w), h, w, C, 0.0 if dyadic else 0.2), dyadic)


def test_imgprop_large_input_conditions():
    """the 1449 x 1448 launch of the GPU test (second turn of the grid-stride loop): its share of undecided pixels and of every
    branch; no block is sent a picture's width away here (next to such a block the check flow has a slope of 1449 per pixel, and
    fp32 positions at x = 1448 are 1e-4 wide), so the picture is left only across its borders"""
    h, w = R.LARGE_SIZE
    inp = R.imgprop_inputs(R.step_seed(h, w), h, w, 3, 0.2, far=False, bad=0.1, check_noise=False)
    R.step_conditions(inp, False, oob=False)


def test_imgprop_first_step_ignores_the_rest():
    inp = R.imgprop_inputs(5, 9, 17, 3, 0.0)
    nan = {k: np.full_like(v, np.nan) for k, v in inp.items() if k not in ("cur", "mcur")}
    prop, mprop, _ = R.imgprop_step(first=1, **dict(inp, **nan))
    assert np.array_equal(prop, inp["cur"]) and np.array_equal(mprop, inp["mcur"])


@pytest.mark.parametrize("t,H,W", [(2, 32, 40), (4, 48, 64)])
def test_chain_equals_img_propagation(t, H, W):
    """the bidirectional chain of steps (frame, flow and role indexing of both directions) on the smooth-flow inputs of
    test_gpu_pp.py, in float32 as the oracle computes"""
    frames, masks, ff, fb = propainter_inputs(60 + t, t, t, H, W)
    masked = frames * (1 - masks)
    ref, rm = ProPainterOracle({}).img_propagation(torch.from_numpy(masked), torch.from_numpy(ff), torch.from_numpy(fb),
                                                   torch.from_numpy(masks).clone())
    got, gm = R.imgprop_chain(masked, ff, fb, masks, np.float32)
    dp, dm = float((got != ref.numpy()).mean()), float((gm != rm.numpy()).mean())
    print(f"chain {t}x{H}x{W}: pixel mismatches {dp:.2e}, mask mismatches {dm:.2e}")
    assert dp == 0 and dm == 0


@pytest.mark.parametrize("t", [4, 1])
def test_chain_on_the_dyadic_clip(t):
    """the clip of test_gpu_pp.py's zero-mismatch case: float32 and float64 chains and the oracle agree bit for bit, and the
    propagation fills holes in both directions"""
    masked, masks, ff, fb = R.imgprop_clip(70 + t, t, 17, 33)
    ref, rm = ProPainterOracle({}).img_propagation(torch.from_numpy(masked), torch.from_numpy(ff), torch.from_numpy(fb),
                                                   torch.from_numpy(masks).clone())
    for dt in (np.float32, np.float64):
        got, gm = R.imgprop_chain(masked, ff, fb, masks, dt)
        assert np.array_equal(got, ref.numpy()) and np.array_equal(gm, rm.numpy())
    if t > 1:
        filled = 1 - rm.sum().item() / masks.sum()
        print(f"dyadic clip t={t}: filled {filled:.3f} of the holes")
        assert filled > 0.1 and (ref.numpy() != masked).any(axis=1).mean() > 0.05


# ---- the plugin's glue -----------------------------------------------------------------------------------------------------------------
def test_prepare_and_compose_equal_the_wrapper_lines():
    rng = np.random.default_rng(3)
    n, h, w = 3, 5, 7
    bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    mask = rng.choice(np.array([0, 0, 1, 7, 255], dtype=np.uint8), (h, w))
    # oracle/propainter_wrapper.py:46-51, 67, 82 (the mask enters as {0, 1} after dilate_masks; any non-zero byte is a hole)
    frames_inp = [np.ascontiguousarray(f[:, :, ::-1]) for f in bgr]
    frames = torch.from_numpy(np.stack(frames_inp)).permute(0, 3, 1, 2).float().div(255) * 2 - 1
    md = torch.from_numpy((mask != 0).astype(np.uint8)).float()[None, None].repeat(n, 1, 1, 1)
    masked = frames * (1 - md)
    assert np.array_equal(R.prepare(bgr, mask, np.float32), masked.numpy())
    prop = torch.from_numpy(rng.uniform(-1, 1, (n, 3, h, w)).astype(np.float32))
    assert np.array_equal(R.compose(bgr, mask, prop.numpy(), np.float32), (frames * (1 - md) + prop * md).numpy())
    err = np.abs(R.prepare(bgr, mask, np.float64) - masked.numpy()).max()
    print(f"prepare float32 vs float64: {err:.3e} (bound {2 * R.U32:.3e})")
    assert err <= 2 * R.U32


def test_truncation_boundaries_are_real():
    """at the fp32 images of k / 255 the cast truncates below k for some k: the boundary values of the GPU test discriminate
    truncation from rounding, and the float32 and float64 evaluations differ there (the kernel is held to float32)"""
    c = (2.0 * np.arange(256) / 255.0 - 1.0).astype(np.float32)
    cast = lambda p: ((p + np.float32(1)) / np.float32(2) * np.float32(255)).astype(np.uint8)
    below = int((cast(c) != np.arange(256)).sum())
    below_n = int((cast(np.nextafter(c[1:], np.float32(-2))) != np.arange(1, 256)).sum())
    print(f"float32(2k/255 - 1) truncating below k: {below} of 256; their lower neighbours: {below_n} of 255")
    assert below >= 50 and below_n >= 150
    v = R.boundary_preds()
    assert v.min() == -1.0 and v.max() == 1.0 and len(v) >= 256 * 3
    f32, f64 = R.blend_values(v, np.float32), R.blend_values(v, np.float64)
    assert (np.rint(f32) != f32.astype(np.uint8)).mean() > 0.2, "rounding and truncation must differ on these values"
    assert f32.min() >= 0 and f32.max() <= 255


def test_blend_window_equals_the_wrapper_loop():
    """three overlapping windows through blend_window against the wrapper's loop :88-101 written out (comp list of None, RGB)"""
    rng = np.random.default_rng(11)
    n, h, w = 6, 5, 7
    bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    mask = rng.choice(np.array([0, 1, 7, 255], dtype=np.uint8), (h, w))
    windows = [[4, 0, 2], [2, 4, 3], [4, 1]]
    preds = [np.tanh(rng.standard_normal((len(nb), 3, h, w)) * 2).astype(np.float32) for nb in windows]
    frames_inp = [np.ascontiguousarray(f[:, :, ::-1]) for f in bgr]
    binary = (mask != 0)[:, :, None].astype(np.uint8)
    comp = [None] * n
    for nb, pred in zip(windows, preds):
        pred = ((torch.from_numpy(pred) + 1) / 2).permute(0, 2, 3, 1).numpy() * 255
        for i, idx in enumerate(nb):
            img = np.array(pred[i]).astype(np.uint8) * binary + frames_inp[idx] * (1 - binary)
            if comp[idx] is None:
                comp[idx] = img
            else:
                comp[idx] = comp[idx].astype(np.float32) * 0.5 + img.astype(np.float32) * 0.5
            comp[idx] = comp[idx].astype(np.uint8)
    got = np.full((n, h, w, 3), 0xA5, dtype=np.uint8)
    seen = set()
    for nb, pred in zip(windows, preds):
        R.blend_window(pred, bgr, mask, nb, [i not in seen for i in nb], got, np.float32)
        seen |= set(nb)
    for idx in range(n):
        if comp[idx] is None:
            assert np.all(got[idx] == 0xA5)
        else:
            assert np.array_equal(got[idx], comp[idx][:, :, ::-1]), f"frame {idx}"
    a, b, c = (R.blend_window(p[k:k + 1], bgr, mask, [4], [1], np.zeros_like(bgr), np.float32)[4].astype(np.int64)
               for p, k in ((preds[0], 0), (preds[1], 1), (preds[2], 0)))
    assert np.array_equal(got[4], ((a + b) // 2 + c) // 2), "truncation after every average"


def test_absdiff_sums_reference():
    f = np.array([[[0, 5, 255]], [[255, 5, 0]], [[250, 0, 0]]], dtype=np.uint8)
    assert R.absdiff_sums(f).tolist() == [[255, 0, 255], [5, 5, 0]] and R.absdiff_sums(f).dtype == np.int64
