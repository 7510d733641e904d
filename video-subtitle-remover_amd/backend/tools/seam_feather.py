"""--seam-feather F: the mask-exact, feathered composite every inpaint mode can end its plugin call with (not in the reference; opt-in,
DESIGN 4.11; the numpy statement is tests/_feather_statement.py).

For one plugin call on frames [n,H,W,3]:   src   the frames as they came in
                                           fill  what the call returns with the option off
                                           C     the plugin's composite mask, uint8 [H,W]: plugin.composite_mask(input_mask)
                                           d(p)  min(F, Chebyshev distance from p to the nearest q inside the frame with C[q] == 0)
    out[p] = (d(p) * fill[p] + (F - d(p)) * src[p] + F // 2) // F           per channel, integers
d = 0 gives the source bit for bit, d = F the fill; F = 1 is the hard composite at full resolution, F >= 2 ramps the fill in over F
pixels.  The frame border is no zero of C: a band that touches the bottom edge is not feathered there.

F = 0 (the default) is OFF: the plugin's body runs as it always has -- no clone, no launch, no byte written that was not before.
The option is read here and nowhere else (feather_option: --seam-feather sets VSR_SEAM_FEATHER).  The helper sits inside the plugin
call, so every loop that ends in one (host frames, the HBM-resident clip, resident windows, batch lanes, the single picture,
propainter's single-frame LaMa) gets it without knowing.  With F > 0, a non-empty C and n > 0 a call

    1. takes d from the cache (vsr_feather_alpha once per (mask bytes, F); the last few are kept, as TeleaEngine keeps its plans),
    2. clones the frames on the caller's stream,
    3. runs the body unchanged,
    4. launches vsr_feather_composite on the same stream, which the body's result is ordered on.

The list form uploads once, runs the device form and downloads once.  Several ranks are refused (refuse_ranks) before any work.

--regrain P (tools/regrain.py) lives in the same two calls and shares the clone: with P > 0 the fill is regrained between
steps 3 and 4, out = composite(regrain(fill), src, d, F); with F = 0 and P > 0 steps 1 and 4 fall away.  Both off: the body alone.

--deflicker R (tools/deflicker.py) is a third pass on the same clone, in front of the regrain: body -> deflicker -> regrain
-> feather, so that regrain measures the smoothed fill's deficit and its fresh per-frame grain is not averaged away.  All off: the body
alone.

--tone-match S (tools/tone_match.py) is the fourth pass on the same clone and the first to run: body -> tone-match ->
deflicker -> regrain -> feather.  A levelled fill passes deflicker's gate more often, and regrain's deficit and the feather's ramp see
the final tone.  All off: the body alone.

--glyph-key T (tools/glyph_key.py) is the fifth pass on the same clone and the last before the feather: body -> tone-match
-> deflicker -> regrain -> glyph-key -> feather.  It keeps the source wherever the levelled, steadied, regrained fill -- the fill the
viewer would have seen -- only repeats it, and the feather's ramp at C's edge then works on the keyed frames.  options() and
refuse_ranks_all() keep naming the first four; T is read through glyph_key.key_option(), and refuse_ranks_all() makes its refusal too.
All off: the body alone.  --glyph-hold K lives inside that pass: glyph_key.apply reads it, and is called here as before.

--borrow B (tools/borrow.py) is the sixth pass on the same clone, between the regrain and the key: body -> tone-match ->
deflicker -> regrain -> borrow -> glyph-key -> feather.  A borrowed pixel is real picture, so the three passes that level, mix and
regrain the model's fill run before it and do not touch it; the key then judges the frames as the borrow left them.  It needs T > 0 and
the plugin's sample rows (the ring of --regrain gates it); B is read through borrow.borrow_option(), and refuse_ranks_all() makes its
refusals too.  B = 0: the calls above and nothing else.

--logo-unblend (tools/unblend.py) is the seventh pass and the last: body -> tone-match -> deflicker -> regrain -> borrow ->
glyph-key -> feather -> unblend.  Inside the areas of --logo-scan whose translucent overlay it can un-mix it writes the un-mixed source
over whatever stands there; that is real picture, so no cosmetic pass may touch it.  It reads no option here: the plans of the run are
in unblend's registry (SubtitleRemover.run() sets it), and with plans registered a call clones its source even when every other option
is off.  No plans (the option off): the calls above and nothing else.
"""
import collections
import ctypes as C
import os
import threading

import numpy as np

from . import borrow as borrow_pass
from . import deflicker, glyph_key, regrain, tone_match
from . import unblend as unblend_pass

MAX_FEATHER = 64
ENV = "VSR_SEAM_FEATHER"
MAX_ALPHAS = 4              # alphas kept per process: an interval's batches and the lanes present the same mask again and again


def feather_option(value=None, env=None):
    """F of this run: `value`, None = the environment (VSR_SEAM_FEATHER, unset or empty = 0 = off).  The one reading of the option.
    ValueError for anything that is no integer in [0, 64]."""
    env = os.environ if env is None else env
    if value is None:
        value = env.get(ENV, "0") or "0"
    try:
        f = int(value)
        if isinstance(value, float) and f != value:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"seam feather: {value!r} is not an integer") from None
    if f < 0 or f > MAX_FEATHER:
        raise ValueError(f"seam feather: F = {f} asked for, 0 <= F <= {MAX_FEATHER} are possible (0 = off)")
    return f


def refuse_ranks(dist, feather=None):
    """-> F.  With F > 0, more than one rank raises before any work: the frames of a call and its source clone live on the rank that
    runs the call, and the ranks' writers have not been taught the option (the precedent of --sttn-context)."""
    f = feather_option(feather)
    if f and dist is not None and dist.get_world_size() > 1:
        raise RuntimeError(f"--seam-feather / {ENV} = {f} runs in one process (world size {dist.get_world_size()}): "
                           "run without it or on one GPU")
    return f


def options():
    """-> (F, P, R, S) of this run: --seam-feather, --regrain, --deflicker and --tone-match as the environment has them (the four passes
    of one plugin call)"""
    return feather_option(), regrain.regrain_option(), deflicker.deflicker_option(), tone_match.tone_option()


def refuse_ranks_all(dist):
    """-> (F, P, R, S).  The refusals every entry point makes before any work, in this order: the first bad option wins.  The fifth,
    --glyph-key's (tools/glyph_key.py), is made here too; its T is not part of the tuple (glyph_key.key_option() reads it), and
    --borrow's (tools/borrow.py) after it"""
    four = refuse_ranks(dist), regrain.refuse_ranks(dist), deflicker.refuse_ranks(dist), tone_match.refuse_ranks(dist)
    glyph_key.refuse_ranks(dist)
    borrow_pass.refuse_ranks(dist)
    return four


_alphas = collections.OrderedDict()         # (device index, H, W, F, mask bytes) -> uint8 [H,W] device tensor; least recently used first
_lock = threading.Lock()
stats = {"alpha_builds": 0, "alpha_hits": 0, "composites": 0}


def alpha(cmask, feather, device):
    """d of the composite mask `cmask` (host uint8 [H,W], non-zero = inside) on `device`: cached, or computed now by
    vsr_feather_alpha.  The computing stream is waited for once, so that any stream (another lane's) may read the cached tensor."""
    import torch

    from ..._lib import check, lib

    cmask = np.ascontiguousarray(cmask, dtype=np.uint8)
    assert cmask.ndim == 2, "composite mask must be [H, W]"
    device = torch.device(device)
    H, W = cmask.shape
    key = (device.index or 0, H, W, int(feather), cmask.tobytes())
    with _lock:
        d = _alphas.pop(key, None)
        if d is None:
            with torch.cuda.device(device):
                c_dev = torch.from_numpy(cmask).to(device)
                d = torch.empty((H, W), dtype=torch.uint8, device=device)
                stream = torch.cuda.current_stream(device)
                check(lib.vsr_feather_alpha(C.c_void_p(c_dev.data_ptr()), H, W, int(feather), C.c_void_p(d.data_ptr()),
                                            C.c_void_p(stream.cuda_stream)))
                stream.synchronize()
            stats["alpha_builds"] += 1
            while len(_alphas) >= MAX_ALPHAS:
                _alphas.popitem(last=False)
        else:
            stats["alpha_hits"] += 1
        _alphas[key] = d
    return d


def composite(frames, src, d, feather):
    """in place on `frames` (uint8 [n,H,W,3] on the GPU, every frame contiguous; it holds the fill) with the source frames `src` (same
    shape, its own frame stride) under d (uint8 [H,W] device): vsr_feather_composite on the current stream"""
    import torch

    from ..._lib import check, lib

    n, H, W, _ = frames.shape
    if n == 0:
        return frames
    for t in (frames, src):
        assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (n, H, W, 3)
        assert t.stride(3) == 1 and t.stride(2) == 3 and t.stride(1) == 3 * W, "every frame must be contiguous [H,W,3]"
    assert d.dtype == torch.uint8 and d.is_contiguous() and tuple(d.shape) == (H, W) and d.device == frames.device == src.device
    fs = frames.stride(0) if n > 1 else H * W * 3
    ss = src.stride(0) if n > 1 else H * W * 3
    with torch.cuda.device(frames.device):
        stream = torch.cuda.current_stream(frames.device)
        d.record_stream(stream)              # (a cached tensor, made on whichever stream asked first)
        check(lib.vsr_feather_composite(C.c_void_p(frames.data_ptr()), fs, C.c_void_p(src.data_ptr()), ss, C.c_void_p(d.data_ptr()),
                                        n, H, W, int(feather), C.c_void_p(stream.cuda_stream)))
    stats["composites"] += 1
    return frames


def device_call(frames, cmask, body, feather, rows=None, grain=0, sample_rows=None, flicker=0, tone=0, key=0, borrow=0, unmix=None):
    """body(frames) inpaints the device tensor `frames` in place (today's call); with F > 0 and a non-empty composite mask the frames
    come back as the definition's.  cmask: the FULL-frame composite mask (host uint8) or a callable that makes it; rows = (y_lo, y_hi):
    `frames` holds these rows of the frame only (sttn-auto's strip rows) -- d is computed on the full frame and sliced, so a mask that
    touches the first or last of the rows ramps as it does in the whole frame.
    grain = P of --regrain (tools/regrain.py), sample_rows = the plugin's (None: the whole frame): with P > 0 the fill is regrained
    against the same source clone before the composite, out = composite(regrain(fill), src, d, F); with F = 0 regrain alone.
    flicker = R of --deflicker (tools/deflicker.py): with R > 0 and more than one frame the fill is steadied over time, against the same
    clone and in the same sample rows, before the regrain.
    tone = S of --tone-match (tools/tone_match.py): with S > 0 the fill's tone is levelled to the source across the seam, against the
    same clone and in the same sample rows, before everything else.
    key = T of --glyph-key (tools/glyph_key.py): with T > 0 the source is kept, against the same clone, wherever the fill as the other
    three passes left it only repeats it; the composite follows.
    borrow = B of --borrow (tools/borrow.py): with B > 0, T > 0 and more than one frame, a pixel the key would show fill at takes the
    source pixel of a frame of the call within B frames that shows the real picture there, in front of the key.
    unmix = the plans of --logo-unblend (tools/unblend.py), None: the run's (unblend.active()): with plans, every area of theirs gets
    its un-mixed source from the same clone behind the composite."""
    unmix = unblend_pass.active() if unmix is None else unmix
    if frames.shape[0] < 2:
        flicker = 0                          # one frame has no neighbour
    if frames.shape[0] < 2 or not key:
        borrow = 0
    if not (feather or grain or flicker or tone or key or unmix) or frames.shape[0] == 0:
        return body(frames)
    cm = cmask() if callable(cmask) else cmask
    if not cm.any():
        return body(frames)
    import torch

    d = None
    if feather:
        d = alpha(cm, feather, frames.device)
        if rows is not None:
            d = d[rows[0]:rows[1]]
    sample_rows = (0, cm.shape[0]) if sample_rows is None else sample_rows
    sets = regrain.sets(cm, sample_rows, frames.device) if (grain or flicker or borrow) else None
    bands = tone_match.sets(cm, sample_rows, frames.device) if tone else None
    keyed = glyph_key.mask(cm, frames.device) if key else None
    src = frames.clone(memory_format=torch.contiguous_format)
    out = body(frames)
    if tone:
        tone_match.apply(frames, src, bands, tone, y0=0 if rows is None else rows[0])
    if flicker:
        deflicker.apply(frames, src, sets, flicker, y0=0 if rows is None else rows[0])
    if grain:
        regrain.apply(frames, src, sets, grain, y0=0 if rows is None else rows[0])
    if borrow:
        borrow_pass.apply(frames, src, sets, keyed, key, borrow, y0=0 if rows is None else rows[0])
    if key:
        glyph_key.apply(frames, src, keyed, key, y0=0 if rows is None else rows[0])
    if feather:
        composite(frames, src, d, feather)
    if unmix:
        unblend_pass.apply(frames, src, unmix, y0=0 if rows is None else rows[0], H=cm.shape[0])
    return frames if out is None else out


def plugin_call(plugin, body, input_frames, input_mask, device, context=None, lookahead=None, unmix=None):
    """The __call__ of a plugin under the option: body(input_frames, input_mask[, context=][, lookahead=]) is the plugin's call as it
    has always been (a list of HxWx3 arrays -> fresh arrays; a uint8 [n,H,W,3] device tensor -> inpainted in place and returned).
    plugin.composite_mask(input_mask) names the pixels it blends under; device: where the list form uploads to.  Context frames
    of either kind (in front of the batch, behind it) are handed through and take no part in the composite.  unmix: the plans of
    --logo-unblend, None: the run's."""
    u = unblend_pass.active() if unmix is None else unmix
    kw = {} if context is None else {"context": context}
    if lookahead is not None:
        kw["lookahead"] = lookahead
    f, g, r, s = options()
    t = glyph_key.key_option()
    b = borrow_pass.borrow_option() if t else 0
    if len(input_frames) < 2:
        r = b = 0                            # one frame has no neighbour
    if not (f or g or r or s or t or u):
        return body(input_frames, input_mask, **kw)
    import torch

    sample_rows = plugin.sample_rows(input_mask) if (g or r or s or b) else None
    if isinstance(input_frames, torch.Tensor):
        return device_call(input_frames, lambda: plugin.composite_mask(input_mask), lambda d: body(d, input_mask, **kw), f,
                           grain=g, sample_rows=sample_rows, flicker=r, tone=s, key=t, borrow=b, unmix=u)
    if len(input_frames) == 0:
        return body(input_frames, input_mask, **kw)
    cm = plugin.composite_mask(input_mask)
    if not cm.any():
        return body(input_frames, input_mask, **kw)
    if not getattr(plugin, "accepts_device_frames", False):
        # a body that works on host arrays (opencv through cv2): its fill and the source go up for the seven passes
        fill = body(input_frames, input_mask, **kw)
        frames = torch.from_numpy(np.ascontiguousarray(np.stack(fill))).to(device)
        src = torch.from_numpy(np.ascontiguousarray(np.stack(input_frames))).to(device)
        if s:
            tone_match.apply(frames, src, tone_match.sets(cm, sample_rows, frames.device), s)
        if r:
            deflicker.apply(frames, src, regrain.sets(cm, sample_rows, frames.device), r)
        if g:
            regrain.apply(frames, src, regrain.sets(cm, sample_rows, frames.device), g)
        if b:
            borrow_pass.apply(frames, src, regrain.sets(cm, sample_rows, frames.device), glyph_key.mask(cm, frames.device), t, b)
        if t:
            glyph_key.apply(frames, src, glyph_key.mask(cm, frames.device), t)
        if f:
            composite(frames, src, alpha(cm, f, frames.device), f)
        if u:
            unblend_pass.apply(frames, src, u, H=cm.shape[0])
    else:
        frames = torch.from_numpy(np.ascontiguousarray(np.stack(input_frames))).to(device)
        kw = {name: torch.from_numpy(np.ascontiguousarray(np.stack(c))).to(device)
              for name, c in (("context", context), ("lookahead", lookahead)) if c is not None and len(c)}
        device_call(frames, cm, lambda d: body(d, input_mask, **kw), f, grain=g, sample_rows=sample_rows, flicker=r, tone=s, key=t,
                    borrow=b, unmix=u)
    out = frames.cpu().numpy()
    return [out[i] for i in range(out.shape[0])]
