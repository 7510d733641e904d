"""--tone-match S: the fill's tone levelled to the picture across the seam of the composite mask (not in the reference; opt-in,
DESIGN 4.14; the numpy statement is tests/_tone_statement.py).

For one plugin call on frames [n,H,W,3]:   src   the frames as they came in
                                           fill  what the call's body returns
                                           C     the plugin's composite mask, uint8 [H,W]: plugin.composite_mask(input_mask)
                                           R     the plugin's sample rows [r0, r1): plugin.sample_rows(input_mask)
    E = the two pixels just outside C, M = the two pixels just inside it, both in R
    per frame   the means of src over E and of fill over M, pulled up a pyramid of cells (8 x 8 pixels at the finest level) and pushed
                back down: where a cell holds samples its own mean counts, elsewhere the smooth field from above -> the step h3 per cell
    per pixel   out = clamp(fill + (S * h + d / 2) / d) on C, h the bilinear interpolation of h3, d = 100 * 64 * 256
S is a percentage of the measured step, 0 <= S <= 100.  A frame the call did not inpaint (fill == src on C) comes back untouched.

S = 0 (the default) is OFF: no clone, no launch, no byte written that was not before.  The option is read here and nowhere else
(tone_option: --tone-match sets VSR_TONE_MATCH).  The call sits inside tools/seam_feather.plugin_call / device_call, right behind the
plugin's body and in front of --deflicker, --regrain and the feathered composite, and uses the source clone those make: every loop
that ends in a plugin call gets it without knowing.

    1. the seam bands come from the cache (vsr_tone_sets once per (mask bytes, R); the last few are kept),
    2. vsr_tone_apply is launched on the caller's stream with a workspace of vsr_tone_workspace_bytes; no sum visits the host.

Several ranks are refused (refuse_ranks) before any work, as --regrain refuses them.
"""
import collections
import ctypes as C
import os
import threading

import numpy as np

MAX_TONE = 100
ENV = "VSR_TONE_MATCH"
MAX_SETS = 4                # seam bands kept per process: an interval's batches and the lanes present the same mask again and again


def tone_option(value=None, env=None):
    """S of this run: `value`, None = the environment (VSR_TONE_MATCH, unset or empty = 0 = off).  The one reading of the option.
    ValueError for anything that is no integer in [0, 100]."""
    env = os.environ if env is None else env
    if value is None:
        value = env.get(ENV, "0") or "0"
    try:
        s = int(value)
        if isinstance(value, float) and s != value:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"tone match: {value!r} is not an integer") from None
    if s < 0 or s > MAX_TONE:
        raise ValueError(f"tone match: S = {s} asked for, 0 <= S <= {MAX_TONE} are possible (0 = off)")
    return s


def refuse_ranks(dist, tone=None):
    """-> S.  With S > 0, more than one rank raises before any work: the frames of a call and its source clone live on the rank that
    runs the call, and the ranks' writers have not been taught the option (the precedent of --regrain)."""
    s = tone_option(tone)
    if s and dist is not None and dist.get_world_size() > 1:
        raise RuntimeError(f"--tone-match / {ENV} = {s} runs in one process (world size {dist.get_world_size()}): "
                           "run without it or on one GPU")
    return s


class Sets:
    """the seam bands of one (composite mask, sample rows) on one device: the byte map (bit 0 = E, bit 1 = M, bit 2 = C != 0), the
    list of the 8 x 8 cells that hold a non-zero byte of it (the first `ncells` words of `cells`) and the rows [c0, c1) of the frame
    that hold a pixel of C"""
    __slots__ = ("map", "cells", "ncells", "c0", "c1")

    def __init__(self, map_, cells, ncells, c0, c1):
        self.map, self.cells, self.ncells, self.c0, self.c1 = map_, cells, ncells, c0, c1


_sets = collections.OrderedDict()           # (device index, H, W, r0, r1, mask bytes) -> Sets; least recently used first
_lock = threading.Lock()
stats = {"set_builds": 0, "set_hits": 0, "calls": 0}


def sets(cmask, sample_rows, device):
    """the Sets of the composite mask `cmask` (host uint8 [H,W], non-zero = inside, not empty) and the sample rows on `device`: cached,
    or computed now by vsr_tone_sets.  The computing stream is waited for once (the number of listed cells comes back with it), so that
    any stream (another lane's) may read them."""
    import torch

    from ..._lib import check, lib

    cmask = np.ascontiguousarray(cmask, dtype=np.uint8)
    assert cmask.ndim == 2, "composite mask must be [H, W]"
    device = torch.device(device)
    H, W = cmask.shape
    r0, r1 = int(sample_rows[0]), int(sample_rows[1])
    key = (device.index or 0, H, W, r0, r1, cmask.tobytes())
    with _lock:
        s = _sets.pop(key, None)
        if s is None:
            held = np.flatnonzero(cmask.any(axis=1))
            with torch.cuda.device(device):
                c_dev = torch.from_numpy(cmask).to(device)
                map_ = torch.empty((H, W), dtype=torch.uint8, device=device)
                counts = torch.empty(3, dtype=torch.int64, device=device)
                cells = torch.empty(-(-H // 8) * -(-W // 8), dtype=torch.int32, device=device)
                stream = torch.cuda.current_stream(device)
                check(lib.vsr_tone_sets(C.c_void_p(c_dev.data_ptr()), H, W, r0, r1, C.c_void_p(map_.data_ptr()),
                                        C.c_void_p(counts.data_ptr()), C.c_void_p(cells.data_ptr()), C.c_void_p(stream.cuda_stream)))
                ncells = int(counts.cpu()[2])                # (waits for the stream)
            s = Sets(map_, cells, ncells, int(held[0]), int(held[-1]) + 1)
            stats["set_builds"] += 1
            while len(_sets) >= MAX_SETS:
                _sets.popitem(last=False)
        else:
            stats["set_hits"] += 1
        _sets[key] = s
    return s


def apply(frames, src, s, percent, y0=0):
    """in place on `frames` (uint8 [n,h,W,3] on the GPU, every frame contiguous; it holds the fill: the rows [y0, y0 + h) of the
    picture) with the source frames `src` (same shape, its own frame stride) under the Sets `s`: vsr_tone_apply on the current stream,
    its sums and fields in a workspace that lives for the call"""
    import torch

    from ..._lib import check, lib

    n, h, W, _ = frames.shape
    if n == 0 or not percent:
        return frames
    H = s.map.shape[0]
    for t in (frames, src):
        assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (n, h, W, 3)
        assert t.stride(3) == 1 and t.stride(2) == 3 and t.stride(1) == 3 * W, "every frame must be contiguous [h,W,3]"
    assert s.map.shape[1] == W and 0 <= y0 and y0 + h <= H and s.map.device == frames.device == src.device
    fs = frames.stride(0) if n > 1 else h * W * 3
    ss = src.stride(0) if n > 1 else h * W * 3
    with torch.cuda.device(frames.device):
        stream = torch.cuda.current_stream(frames.device)
        nbytes = int(lib.vsr_tone_workspace_bytes(H, W, n))
        if nbytes < 0:
            check(nbytes)
        work = torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.int64, device=frames.device)
        for t in (s.map, s.cells):
            t.record_stream(stream)          # (cached tensors, made on whichever stream asked first)
        check(lib.vsr_tone_apply(C.c_void_p(frames.data_ptr()), fs, C.c_void_p(src.data_ptr()), ss, C.c_void_p(s.map.data_ptr()),
                                 C.c_void_p(s.cells.data_ptr()), s.ncells, n, H, W, int(y0), h, s.c0, s.c1, int(percent),
                                 C.c_void_p(work.data_ptr()), C.c_void_p(stream.cuda_stream)))
    stats["calls"] += 1
    return frames
