"""--glyph-key T: the source kept wherever the fill only repeats it (not in the reference; opt-in; the numpy statement is
tests/_key_statement.py).

For one plugin call on frames [n,h,W,3]:   src   the frames as they came in
                                           fill  the frames as they stand when the pass runs
                                           C     the plugin's composite mask, uint8 [H,W]: plugin.composite_mask(input_mask)
    D = max over the channels of |src - fill| on C, a seed where the 3 x 3 sum of D reaches 9 T
    e = the Chebyshev distance to the frame's nearest seed, a = clamp(G + R - e, 0, R) with G = R = 4
    out = (a * fill + (R - a) * src + R / 2) / R on C: the fill within G pixels of a seed, the source bit for bit from G + R pixels on
A frame the call did not inpaint, and a frame on which the fill says what the source said, comes back as its source.  Nothing is carried
from one frame to the next.

T = 0 (the default) is OFF: no clone, no launch, no byte written that was not before.  The option is read here and nowhere else
(key_option: --glyph-key sets VSR_GLYPH_KEY).  The call sits inside tools/seam_feather.plugin_call / device_call, behind --tone-match,
--deflicker and --regrain and in front of the feathered composite, and uses the source clone those make: it judges the fill the
viewer would have seen, and the feather ramps the keyed frames.

    1. the composite mask on the device comes from the cache (the last few are kept, by the mask's bytes),
    2. vsr_key_apply is launched on the caller's stream with a workspace of vsr_key_workspace_bytes; no word visits the host.

Several ranks are refused (refuse_ranks) before any work, as --tone-match refuses them.

--glyph-hold K (the statement is tests/_hold_statement.py) holds a seed in time: a pixel whose 3 x 3 sum of D reaches
9 * ((T + 1) // 2) stays a seed while one of the K frames before or after it in the same call has a seed of the plain key within one
pixel of it.  K = 0 (the default) is the plain key: the same call, launches and bytes.  The option is read here and nowhere else
(hold_option: --glyph-hold sets VSR_GLYPH_HOLD); K > 0 makes apply() call vsr_key_apply_hold with a workspace of
vsr_key_hold_workspace_bytes.  K > 0 needs T > 0: refuse_ranks raises otherwise.
"""
import collections
import ctypes as C
import os
import threading

import numpy as np

MAX_KEY = 128
ENV = "VSR_GLYPH_KEY"
MAX_HOLD = 8
HOLD_ENV = "VSR_GLYPH_HOLD"
MAX_MASKS = 4               # masks kept per process: an interval's batches and the lanes present the same mask again and again


def key_option(value=None, env=None):
    """T of this run: `value`, None = the environment (VSR_GLYPH_KEY, unset or empty = 0 = off).  The one reading of the option.
    ValueError for anything that is no integer in [0, 128]."""
    env = os.environ if env is None else env
    if value is None:
        value = env.get(ENV, "0") or "0"
    try:
        t = int(value)
        if isinstance(value, float) and t != value:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"glyph key: {value!r} is not an integer") from None
    if t < 0 or t > MAX_KEY:
        raise ValueError(f"glyph key: T = {t} asked for, 0 <= T <= {MAX_KEY} are possible (0 = off)")
    return t


def hold_option(value=None, env=None):
    """K of this run: `value`, None = the environment (VSR_GLYPH_HOLD, unset or empty = 0 = off).  The one reading of the option.
    ValueError for anything that is no integer in [0, 8]."""
    env = os.environ if env is None else env
    if value is None:
        value = env.get(HOLD_ENV, "0") or "0"
    try:
        k = int(value)
        if isinstance(value, float) and k != value:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"glyph hold: {value!r} is not an integer") from None
    if k < 0 or k > MAX_HOLD:
        raise ValueError(f"glyph hold: K = {k} asked for, 0 <= K <= {MAX_HOLD} are possible (0 = off)")
    return k


def refuse_ranks(dist, key=None, hold=None):
    """-> T.  With T > 0, more than one rank raises before any work: the frames of a call and its source clone live on the rank that
    runs the call, and the ranks' writers have not been taught the option (the precedent of --regrain).  A bad K, and K > 0 with
    T = 0 (a hold with no key to hold), raise ValueError here too."""
    t = key_option(key)
    k = hold_option(hold)
    if k and not t:
        raise ValueError(f"--glyph-hold / {HOLD_ENV} = {k} holds the seeds of --glyph-key / {ENV}, which is off: give both or neither")
    if t and dist is not None and dist.get_world_size() > 1:
        raise RuntimeError(f"--glyph-key / {ENV} = {t} runs in one process (world size {dist.get_world_size()}): "
                           "run without it or on one GPU")
    return t


class Mask:
    """one composite mask on one device: its bytes (uint8 [H,W]) and the rows [c0, c1) of the picture that hold a pixel of it"""
    __slots__ = ("c", "c0", "c1")

    def __init__(self, c, c0, c1):
        self.c, self.c0, self.c1 = c, c0, c1


_masks = collections.OrderedDict()          # (device index, H, W, mask bytes) -> Mask; least recently used first
_lock = threading.Lock()
stats = {"mask_builds": 0, "mask_hits": 0, "calls": 0, "hold_calls": 0}


def mask(cmask, device):
    """the Mask of the composite mask `cmask` (host uint8 [H,W], non-zero = inside, not empty) on `device`: cached, or uploaded now.
    The uploading stream is waited for once, so that any stream (another lane's) may read it."""
    import torch

    cmask = np.ascontiguousarray(cmask, dtype=np.uint8)
    assert cmask.ndim == 2, "composite mask must be [H, W]"
    device = torch.device(device)
    H, W = cmask.shape
    key = (device.index or 0, H, W, cmask.tobytes())
    with _lock:
        m = _masks.pop(key, None)
        if m is None:
            held = np.flatnonzero(cmask.any(axis=1))
            with torch.cuda.device(device):
                c_dev = torch.from_numpy(cmask).to(device)
                torch.cuda.current_stream(device).synchronize()
            m = Mask(c_dev, int(held[0]), int(held[-1]) + 1)
            stats["mask_builds"] += 1
            while len(_masks) >= MAX_MASKS:
                _masks.popitem(last=False)
        else:
            stats["mask_hits"] += 1
        _masks[key] = m
    return m


def apply(frames, src, m, T, y0=0, hold=None):
    """in place on `frames` (uint8 [n,h,W,3] on the GPU, every frame contiguous; it holds the fill: the rows [y0, y0 + h) of the
    picture) with the source frames `src` (same shape, its own frame stride) under the Mask `m`: vsr_key_apply on the current stream,
    its seed bitmap in a workspace that lives for the call.  hold = K of --glyph-hold, None = hold_option(): with K > 0
    vsr_key_apply_hold and its three bitmaps instead"""
    import torch

    from ..._lib import check, lib

    n, h, W, _ = frames.shape
    if n == 0 or not T:
        return frames
    K = hold_option() if hold is None else int(hold)
    H = m.c.shape[0]
    for t in (frames, src):
        assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (n, h, W, 3)
        assert t.stride(3) == 1 and t.stride(2) == 3 and t.stride(1) == 3 * W, "every frame must be contiguous [h,W,3]"
    assert m.c.shape[1] == W and 0 <= y0 and y0 + h <= H and m.c.device == frames.device == src.device
    fs = frames.stride(0) if n > 1 else h * W * 3
    ss = src.stride(0) if n > 1 else h * W * 3
    with torch.cuda.device(frames.device):
        stream = torch.cuda.current_stream(frames.device)
        nbytes = int(lib.vsr_key_hold_workspace_bytes(H, W, n) if K else lib.vsr_key_workspace_bytes(H, W, n))
        if nbytes < 0:
            check(nbytes)
        work = torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.int64, device=frames.device)
        m.c.record_stream(stream)            # (a cached tensor, made on whichever stream asked first)
        if K:
            check(lib.vsr_key_apply_hold(C.c_void_p(frames.data_ptr()), fs, C.c_void_p(src.data_ptr()), ss, C.c_void_p(m.c.data_ptr()),
                                         n, H, W, int(y0), h, m.c0, m.c1, int(T), K, C.c_void_p(work.data_ptr()),
                                         C.c_void_p(stream.cuda_stream)))
            stats["hold_calls"] += 1
        else:
            check(lib.vsr_key_apply(C.c_void_p(frames.data_ptr()), fs, C.c_void_p(src.data_ptr()), ss, C.c_void_p(m.c.data_ptr()),
                                    n, H, W, int(y0), h, m.c0, m.c1, int(T), C.c_void_p(work.data_ptr()), C.c_void_p(stream.cuda_stream)))
    stats["calls"] += 1
    return frames
