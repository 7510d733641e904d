"""--deflicker R: the fill steadied over time inside the inpainted pixels (not in the reference; opt-in; the numpy statement
is tests/_deflicker_statement.py).

For one plugin call on frames [n,H,W,3]:   src   the frames as they came in
                                           fill  what the call's body returns
                                           C     the plugin's composite mask, uint8 [H,W]: plugin.composite_mask(input_mask)
                                           E     the ring of --regrain around C (tools/regrain.py) in the plugin's sample rows, m = 3 |E|
    per pair    S = the sum over E of |src_t - src_{t+k}|, 1 <= k <= R: how much the real picture around the band moved; less what the
                source's own grain accounts for, it sets the pair's weight a in 0..16: full up to 1 level per sample, none from 4 on
    per pixel   out_t = the mean of fill_t (weight 16 * 24) and of the fills fill_s, |s - t| <= R, that differ from it by D < 24 there
                (weight a * (24 - D)), on C
R is the radius of the window in frames, 0 <= R <= 8.  A frame the call did not inpaint (fill == src on C) comes back untouched and lends
nothing; one frame, or a mask without a ring, is the identity.  The window is the call: nothing is carried from one call to the next.

R = 0 (the default) is OFF: no clone, no launch, no byte written that was not before.  The option is read here and nowhere else
(deflicker_option: --deflicker sets VSR_DEFLICKER).  The call sits inside tools/seam_feather.plugin_call / device_call, between the
plugin's body and --regrain, and uses the source clone those make and the sample sets regrain caches:

    1. vsr_regrain_measure (the changed counts and the ring's noise sums), vsr_deflicker_pairs,
    2. one clone of the rows of C (the unsmoothed fill every frame's neighbours are read from), vsr_deflicker_apply,

all on the caller's stream; the sums and the weights never visit the host.  Several ranks are refused (refuse_ranks) before any work,
as --regrain refuses them.
"""
import ctypes as C
import os

MAX_DEFLICKER = 8
ENV = "VSR_DEFLICKER"


def deflicker_option(value=None, env=None):
    """R of this run: `value`, None = the environment (VSR_DEFLICKER, unset or empty = 0 = off).  The one reading of the option.
    ValueError for anything that is no integer in [0, 8]."""
    env = os.environ if env is None else env
    if value is None:
        value = env.get(ENV, "0") or "0"
    try:
        r = int(value)
        if isinstance(value, float) and r != value:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"deflicker: {value!r} is not an integer") from None
    if r < 0 or r > MAX_DEFLICKER:
        raise ValueError(f"deflicker: R = {r} asked for, 0 <= R <= {MAX_DEFLICKER} are possible (0 = off)")
    return r


def refuse_ranks(dist, deflicker=None):
    """-> R.  With R > 0, more than one rank raises before any work: the frames of a call and its source clone live on the rank that
    runs the call, and the ranks' writers have not been taught the option (the precedent of --regrain)."""
    r = deflicker_option(deflicker)
    if r and dist is not None and dist.get_world_size() > 1:
        raise RuntimeError(f"--deflicker / {ENV} = {r} runs in one process (world size {dist.get_world_size()}): "
                           "run without it or on one GPU")
    return r


stats = {"calls": 0}


def apply(frames, src, s, radius, y0=0):
    """in place on `frames` (uint8 [n,h,W,3] on the GPU, every frame contiguous; it holds the fill: the rows [y0, y0 + h) of the
    picture) with the source frames `src` (same shape, its own frame stride) under the regrain.Sets `s`: vsr_regrain_measure,
    vsr_deflicker_pairs and vsr_deflicker_apply on the current stream, the sums in small device arrays between them"""
    import torch

    from ..._lib import check, lib

    n, h, W, _ = frames.shape
    la, lb = max(s.c0 - y0, 0), min(s.c1 - y0, h)
    if n < 2 or not radius or lb <= la:
        return frames
    H = s.map.shape[0]
    for t in (frames, src):
        assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (n, h, W, 3)
        assert t.stride(3) == 1 and t.stride(2) == 3 and t.stride(1) == 3 * W, "every frame must be contiguous [h,W,3]"
    assert s.map.shape[1] == W and 0 <= y0 and y0 + h <= H and s.map.device == frames.device == src.device
    fs, ss = frames.stride(0), src.stride(0)
    with torch.cuda.device(frames.device):
        stream = torch.cuda.current_stream(frames.device)
        sums = torch.empty((n, 4), dtype=torch.int64, device=frames.device)
        pairs = torch.empty((n, int(radius)), dtype=torch.int64, device=frames.device)
        for t in (s.map, s.counts):
            t.record_stream(stream)          # (cached tensors, made on whichever stream asked first)
        st = C.c_void_p(stream.cuda_stream)
        fp, sp, mp = C.c_void_p(frames.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(s.map.data_ptr())
        check(lib.vsr_regrain_measure(fp, fs, sp, ss, mp, n, H, W, int(y0), h, s.c0, s.c1, C.c_void_p(sums.data_ptr()), st))
        check(lib.vsr_deflicker_pairs(sp, ss, mp, n, H, W, int(y0), h, s.c0, s.c1, int(radius), C.c_void_p(pairs.data_ptr()), st))
        snap = frames[:, la:lb].clone(memory_format=torch.contiguous_format)       # the unsmoothed fill, the rows of C only
        check(lib.vsr_deflicker_apply(fp, fs, C.c_void_p(snap.data_ptr()), snap.stride(0), mp, C.c_void_p(s.counts.data_ptr()),
                                      C.c_void_p(sums.data_ptr()), C.c_void_p(pairs.data_ptr()), n, H, W, int(y0), h, s.c0, s.c1,
                                      int(radius), st))
    stats["calls"] += 1
    return frames
