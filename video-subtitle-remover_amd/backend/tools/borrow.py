"""--borrow B: the fill replaced by the real picture of a neighbouring frame (not in the reference; opt-in; the numpy
statement is tests/_borrow_statement.py).

For one plugin call on frames [n,h,W,3]:   src   the frames as they came in
                                           fill  the frames as they stand when the pass runs
                                           C     the plugin's composite mask, uint8 [H,W]: plugin.composite_mask(input_mask)
                                           E     the ring of --regrain around C (tools/regrain.py) in the plugin's sample rows, m = 3 |E|
    N(t)        the pixels within 7 of a seed of --glyph-key T on frame t: where the key would show fill
    per pair    b in 0..16, --deflicker's weight of the pair of frames from the ring's sums, without its rule for frames the call did not
                inpaint: such a frame has no glyph anywhere and lends everywhere
    per pixel   of C with N(t): the first frame s of t-1, t+1, t-2, t+2, .. t-B, t+B inside the call with N(s) clear there and
                max_c |src_s - fill_t| < (24 b) >> 4 gives its source pixel; none: the fill stays
B is the radius of the window in frames, 0 <= B <= 8.  The window is the call: nothing is carried from one call to the next, and context
and look-ahead frames take no part.  The key behind the pass then judges real picture, not fill.

B = 0 (the default) is OFF: no launch, no byte written that was not before.  The option is read here and nowhere else (borrow_option:
--borrow sets VSR_BORROW).  B > 0 needs --glyph-key T > 0 (its T says what a glyph is): refuse_ranks raises otherwise, as it does for
several ranks.  The call sits inside tools/seam_feather.plugin_call / device_call, behind --regrain and in front of --glyph-key, and uses
the source clone those make, the sample sets regrain caches and the mask the key caches:

    1. vsr_regrain_measure (the ring's noise sums) and vsr_deflicker_pairs with R = B,
    2. vsr_borrow_apply with a workspace of vsr_borrow_workspace_bytes,

all on the caller's stream; the sums, the weights and the bitmaps never visit the host.

--borrow-pan P (the statement is tests/_borrow_pan_statement.py; pan_option: --borrow-pan sets VSR_BORROW_PAN) lets the
pass follow a camera that pans by whole pixels: per pair of frames a rigid shift within P pixels per frame step, found by a search over
the ring, is used where it opens the pair's gate further than standing still does, and the lender is read at the shifted pixel.
P = 0 (the default) is OFF: the calls above.  P > 0 needs B > 0 (refuse_ranks) and replaces 1. and 2. by

    1. vsr_regrain_measure and vsr_borrow_pan_search,
    2. vsr_borrow_pan_apply, both on a workspace of vsr_borrow_pan_workspace_bytes.
"""
import ctypes as C
import os

from . import glyph_key

MAX_BORROW = 8
ENV = "VSR_BORROW"
MAX_PAN = 8
PAN_ENV = "VSR_BORROW_PAN"


def borrow_option(value=None, env=None):
    """B of this run: `value`, None = the environment (VSR_BORROW, unset or empty = 0 = off).  The one reading of the option.
    ValueError for anything that is no integer in [0, 8]."""
    env = os.environ if env is None else env
    if value is None:
        value = env.get(ENV, "0") or "0"
    try:
        b = int(value)
        if isinstance(value, float) and b != value:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"borrow: {value!r} is not an integer") from None
    if b < 0 or b > MAX_BORROW:
        raise ValueError(f"borrow: B = {b} asked for, 0 <= B <= {MAX_BORROW} are possible (0 = off)")
    return b


def pan_option(value=None, env=None):
    """P of this run: `value`, None = the environment (VSR_BORROW_PAN, unset or empty = 0 = off).  The one reading of the option.
    ValueError for anything that is no integer in [0, 8]."""
    env = os.environ if env is None else env
    if value is None:
        value = env.get(PAN_ENV, "0") or "0"
    try:
        p = int(value)
        if isinstance(value, float) and p != value:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"borrow-pan: {value!r} is not an integer") from None
    if p < 0 or p > MAX_PAN:
        raise ValueError(f"borrow-pan: P = {p} asked for, 0 <= P <= {MAX_PAN} are possible (0 = off)")
    return p


def refuse_ranks(dist, borrow=None, key=None, pan=None):
    """-> B.  With B > 0, --glyph-key off (no T to say what a glyph is) raises ValueError, and more than one rank raises RuntimeError,
    before any work: the frames of a call and its source clone live on the rank that runs the call (the precedent of --regrain)."""
    b = borrow_option(borrow)
    p = pan_option(pan)
    if p and not b:
        raise ValueError(f"--borrow-pan / {PAN_ENV} = {p} says how far --borrow / {ENV} follows a pan, and that is off: "
                         "give both or neither")
    if b and not glyph_key.key_option(key):
        raise ValueError(f"--borrow / {ENV} = {b} borrows where --glyph-key / {glyph_key.ENV} would show fill, and that is off: "
                         "give both or neither")
    if b and dist is not None and dist.get_world_size() > 1:
        raise RuntimeError(f"--borrow / {ENV} = {b}" + (f" with --borrow-pan / {PAN_ENV} = {p}" if p else "") +
                           f" runs in one process (world size {dist.get_world_size()}): run without it or on one GPU")
    return b


stats = {"calls": 0, "pan_calls": 0}


def apply(frames, src, s, m, T, B, y0=0):
    """in place on `frames` (uint8 [n,h,W,3] on the GPU, every frame contiguous; it holds the fill: the rows [y0, y0 + h) of the
    picture) with the source frames `src` (same shape, its own frame stride) under the regrain.Sets `s` and the glyph_key.Mask `m`:
    vsr_regrain_measure, vsr_deflicker_pairs and vsr_borrow_apply on the current stream, the sums in small device arrays and the
    bitmaps in a workspace that live for the call; with --borrow-pan P > 0 vsr_regrain_measure, vsr_borrow_pan_search and
    vsr_borrow_pan_apply"""
    import torch

    from ..._lib import check, lib

    n, h, W, _ = frames.shape
    if n < 2 or not B or not T or min(m.c1 - y0, h) <= max(m.c0 - y0, 0):
        return frames
    H = m.c.shape[0]
    pan = pan_option()
    for t in (frames, src):
        assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (n, h, W, 3)
        assert t.stride(3) == 1 and t.stride(2) == 3 and t.stride(1) == 3 * W, "every frame must be contiguous [h,W,3]"
    assert tuple(s.map.shape) == tuple(m.c.shape) and m.c.shape[1] == W and 0 <= y0 and y0 + h <= H
    assert s.map.device == m.c.device == frames.device == src.device and (s.c0, s.c1) == (m.c0, m.c1)
    fs, ss = frames.stride(0), src.stride(0)
    with torch.cuda.device(frames.device):
        stream = torch.cuda.current_stream(frames.device)
        sums = torch.empty((n, 4), dtype=torch.int64, device=frames.device)
        nbytes = int(lib.vsr_borrow_pan_workspace_bytes(H, W, n, int(B), pan) if pan else lib.vsr_borrow_workspace_bytes(H, W, n))
        if nbytes < 0:
            check(nbytes)
        work = torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.int64, device=frames.device)
        for t in (s.map, s.counts, m.c):
            t.record_stream(stream)          # (cached tensors, made on whichever stream asked first)
        st = C.c_void_p(stream.cuda_stream)
        fp, sp, mp = C.c_void_p(frames.data_ptr()), C.c_void_p(src.data_ptr()), C.c_void_p(s.map.data_ptr())
        check(lib.vsr_regrain_measure(fp, fs, sp, ss, mp, n, H, W, int(y0), h, s.c0, s.c1, C.c_void_p(sums.data_ptr()), st))
        if pan:
            wp, cp = C.c_void_p(work.data_ptr()), C.c_void_p(s.counts.data_ptr())
            check(lib.vsr_borrow_pan_search(sp, ss, mp, cp, n, H, W, int(y0), h, s.c0, s.c1, int(B), pan, wp, st))
            check(lib.vsr_borrow_pan_apply(fp, fs, sp, ss, C.c_void_p(m.c.data_ptr()), cp, C.c_void_p(sums.data_ptr()), n, H, W, int(y0), h,
                                           m.c0, m.c1, int(T), int(B), pan, wp, st))
            stats["calls"] += 1
            stats["pan_calls"] += 1
            return frames
        pairs = torch.empty((n, int(B)), dtype=torch.int64, device=frames.device)
        check(lib.vsr_deflicker_pairs(sp, ss, mp, n, H, W, int(y0), h, s.c0, s.c1, int(B), C.c_void_p(pairs.data_ptr()), st))
        check(lib.vsr_borrow_apply(fp, fs, sp, ss, C.c_void_p(m.c.data_ptr()), C.c_void_p(s.counts.data_ptr()),
                                   C.c_void_p(sums.data_ptr()), C.c_void_p(pairs.data_ptr()), n, H, W, int(y0), h, m.c0, m.c1, int(T),
                                   int(B), C.c_void_p(work.data_ptr()), st))
    stats["calls"] += 1
    return frames
