"""--regrain P: the source's grain, measured in a ring around the composite mask, put back inside the inpainted pixels (not in the
reference; opt-in; the numpy statement is tests/_regrain_statement.py).

For one plugin call on frames [n,H,W,3]:   src   the frames as they came in
                                           fill  what the call's body returns
                                           C     the plugin's composite mask, uint8 [H,W]: plugin.composite_mask(input_mask)
                                           R     the plugin's sample rows [r0, r1): plugin.sample_rows(input_mask)
    E = the pixels just outside C (3x3 neighbourhood outside it, within 16 pixels of it), I = the pixels well inside it, both in R
    per frame   the mean of Immerkaer's noise operator over E on src and over I on fill -> the deficit r, in quadrature
    per pixel   out = clamp(fill + ((r * P * 60701 * z + 2^39) >> 40)) on C, z a hash of the pixel's place and the frame's content
P is a percentage of the measured deficit, 0 <= P <= 200.  A frame the call did not inpaint (fill == src on C) comes back untouched.

P = 0 (the default) is OFF: no clone, no launch, no byte written that was not before.  The option is read here and nowhere else
(regrain_option: --regrain sets VSR_REGRAIN).  The call sits inside tools/seam_feather.plugin_call / device_call, between the plugin's
body and the feathered composite, and uses the source clone those make: every loop that ends in a plugin call gets it without knowing.

    1. the sample sets come from the cache (vsr_regrain_sets once per (mask bytes, R); the last few are kept),
    2. vsr_regrain_measure and vsr_regrain_apply are launched on the caller's stream; the deficit never visits the host.

Several ranks are refused (refuse_ranks) before any work, as --seam-feather refuses them.
"""
import collections
import ctypes as C
import os
import threading

import numpy as np

MAX_REGRAIN = 200
ENV = "VSR_REGRAIN"
MAX_SETS = 4                # sample sets kept per process: an interval's batches and the lanes present the same mask again and again


def regrain_option(value=None, env=None):
    """P of this run: `value`, None = the environment (VSR_REGRAIN, unset or empty = 0 = off).  The one reading of the option.
    ValueError for anything that is no integer in [0, 200]."""
    env = os.environ if env is None else env
    if value is None:
        value = env.get(ENV, "0") or "0"
    try:
        p = int(value)
        if isinstance(value, float) and p != value:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"regrain: {value!r} is not an integer") from None
    if p < 0 or p > MAX_REGRAIN:
        raise ValueError(f"regrain: P = {p} asked for, 0 <= P <= {MAX_REGRAIN} are possible (0 = off)")
    return p


def refuse_ranks(dist, regrain=None):
    """-> P.  With P > 0, more than one rank raises before any work: the frames of a call and its source clone live on the rank that
    runs the call, and the ranks' writers have not been taught the option (the precedent of --seam-feather)."""
    p = regrain_option(regrain)
    if p and dist is not None and dist.get_world_size() > 1:
        raise RuntimeError(f"--regrain / {ENV} = {p} runs in one process (world size {dist.get_world_size()}): "
                           "run without it or on one GPU")
    return p


class Sets:
    """the sample sets of one (composite mask, sample rows) on one device: the byte map (bit 0 = E, bit 1 = I, bit 2 = C != 0), the
    device words |E|, |I| and the rows [c0, c1) of the frame that hold a pixel of C"""
    __slots__ = ("map", "counts", "c0", "c1")

    def __init__(self, map_, counts, c0, c1):
        self.map, self.counts, self.c0, self.c1 = map_, counts, c0, c1


_sets = collections.OrderedDict()           # (device index, H, W, r0, r1, mask bytes) -> Sets; least recently used first
_lock = threading.Lock()
stats = {"set_builds": 0, "set_hits": 0, "calls": 0}


def sets(cmask, sample_rows, device):
    """the Sets of the composite mask `cmask` (host uint8 [H,W], non-zero = inside, not empty) and the sample rows on `device`: cached,
    or computed now by vsr_regrain_sets.  The computing stream is waited for once, so that any stream (another lane's) may read them."""
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
                counts = torch.empty(2, dtype=torch.int64, device=device)
                stream = torch.cuda.current_stream(device)
                check(lib.vsr_regrain_sets(C.c_void_p(c_dev.data_ptr()), H, W, r0, r1, C.c_void_p(map_.data_ptr()),
                                           C.c_void_p(counts.data_ptr()), C.c_void_p(stream.cuda_stream)))
                stream.synchronize()
            s = Sets(map_, counts, int(held[0]), int(held[-1]) + 1)
            stats["set_builds"] += 1
            while len(_sets) >= MAX_SETS:
                _sets.popitem(last=False)
        else:
            stats["set_hits"] += 1
        _sets[key] = s
    return s


def apply(frames, src, s, percent, y0=0):
    """in place on `frames` (uint8 [n,h,W,3] on the GPU, every frame contiguous; it holds the fill: the rows [y0, y0 + h) of the
    picture) with the source frames `src` (same shape, its own frame stride) under the Sets `s`: vsr_regrain_measure and
    vsr_regrain_apply on the current stream, the per-frame sums in a small device array between them"""
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
        sums = torch.empty((n, 4), dtype=torch.int64, device=frames.device)
        for t in (s.map, s.counts):
            t.record_stream(stream)          # (cached tensors, made on whichever stream asked first)
        st = C.c_void_p(stream.cuda_stream)
        check(lib.vsr_regrain_measure(C.c_void_p(frames.data_ptr()), fs, C.c_void_p(src.data_ptr()), ss, C.c_void_p(s.map.data_ptr()),
                                      n, H, W, int(y0), h, s.c0, s.c1, C.c_void_p(sums.data_ptr()), st))
        check(lib.vsr_regrain_apply(C.c_void_p(frames.data_ptr()), fs, C.c_void_p(s.map.data_ptr()), C.c_void_p(s.counts.data_ptr()),
                                    C.c_void_p(sums.data_ptr()), n, H, W, int(y0), h, s.c0, s.c1, int(percent), st))
    stats["calls"] += 1
    return frames
