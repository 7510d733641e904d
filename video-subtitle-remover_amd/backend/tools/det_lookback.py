"""sttn-det with scene-bounded intervals and look-back context across batch seams (not in the reference; opt-in).

SubtitleRemover.video_inpaint cuts every subtitle interval into batch_generator batches and inpaints each alone: the first frames of
every batch but the first have no past, and an interval that straddles a scene cut feeds frames of the other scene to the attention.
With the two options of sttn-auto (tools/chunk_parallel.lookback_options: VSR_SCENE_SPLIT=1, VSR_STTN_CONTEXT=N):

  pieces   every interval is cut by SubtitleDetect.split_range_by_scene at the scene starts; a piece keeps its interval's mask
  batches  batch_generator runs per piece: no batch holds a cut in its interior
  context  a batch [a, b) of a piece that starts at c also sees the SOURCE frames [max(a - N, c), a): as decoded, never an inpainted
           result, never in front of the piece.  The frames written for [a, b) are the last b - a frames of what the plugin gives on
           the list context ++ batch (STTNDetInpaint.__call__(frames, mask, context=...), vsr_sttn_det_batch_ctx).

This file holds the definition as one pure function (piece_jobs / det_jobs: both loops of video_inpaint and the tests share it) and the
HBM-resident loop's copies: there the batches are slices of the clip that are inpainted IN PLACE, so the source rows a later batch looks
back at are copied aside on the device before the batch that owns them is inpainted (ResidentLookback).
"""
import threading

from .inpaint_tools import batch_generator
from .subtitle_detect import SubtitleDetect

MAX_CONTEXT = 127           # what the plan cache's key holds (vsr_sttn_det_batch_ctx)


def lookback_options(max_load, context=None, scene_split=None, env=None):
    """(n_context, scene_split) of an sttn-det run: the one reading of VSR_STTN_CONTEXT / VSR_SCENE_SPLIT (chunk_parallel.lookback_options),
    with sttn-det's bound: 0 <= N <= config.getSttnMaxLoadNum(), the longest batch.  Off by default.  ValueError for anything else."""
    from .chunk_parallel import lookback_options as parse

    n, split = parse(context, scene_split, max_load, env=env, what="sttn-det", bound="getSttnMaxLoadNum()")
    if n > MAX_CONTEXT:
        raise ValueError(f"sttn-det context: {n} frames asked for, the engine takes at most {MAX_CONTEXT}")
    return n, split


def piece_jobs(first, end, cuts, n_context, max_load):
    """The batches of ONE interval, frames [first, end) 0-based -> [(lo, hi, ctx_lo)]: the interval is cut at the scene starts `cuts`
    (0-based indices of frames that start a scene; SubtitleDetect.split_range_by_scene on the 1-based inclusive numbers), every piece
    goes through batch_generator(.., max_load), and the batch [lo, hi) looks back at the source frames [ctx_lo, lo), ctx_lo =
    max(lo - n_context, start of its piece).  No cuts, n_context = 0: the batches video_inpaint has always made, ctx_lo = lo."""
    if not 0 <= int(n_context) <= int(max_load):
        raise ValueError(f"sttn-det context: {n_context} frames asked for, 0 <= N <= getSttnMaxLoadNum() = {int(max_load)} are possible")
    if end <= first:
        return []
    out = []
    for s, e in SubtitleDetect.split_range_by_scene([(first + 1, end)], [int(c) + 1 for c in cuts]):
        c = s - 1                                                   # the piece is [c, e) 0-based
        for batch in batch_generator(list(range(c, e)), max_load):
            if len(batch) >= 1:
                out.append((batch[0], batch[-1] + 1, max(batch[0] - int(n_context), c)))
    return out


def det_jobs(start_end, n, mask_of, cuts=(), n_context=0, max_load=50):
    """The walk of video_inpaint over the frame numbers of a clip of n frames -> [(lo, hi, ctx_lo, mask)], 0-based.  start_end: {first:
    last} 1-based inclusive interval numbers (already clamped to the frame count); mask_of(first, last): the mask of an interval,
    computed once per interval whatever the cuts; cuts: 0-based scene starts."""
    idx, jobs = 0, []
    while idx < n:
        idx += 1
        if idx not in start_end:
            continue
        first, last = idx, start_end[idx]
        idx = min(last, n)                                         # frames first .. idx are read (main.py:300-305)
        mask = mask_of(first, last)
        jobs += [(lo, hi, ctx_lo, mask) for lo, hi, ctx_lo in piece_jobs(first - 1, idx, cuts, n_context, max_load)]
    return jobs


class ResidentLookback:
    """The context copies of the HBM-resident loop.  jobs: [(lo, hi, ctx_lo, mask)] in frame order over `frames` (uint8 [n,H,W,3] on
    the device), each batch inpainted in place by plugin(frames[lo:hi], mask, context=...).

    call(plugin, j) runs batch j.  FIRST it copies aside, on the calling thread's current stream, every row of its own batch that a
    later batch looks back at (a context of N <= getSttnMaxLoadNum() frames can span more than one batch, since batch_generator shrinks
    the batch size: every owner copies its own part into the reader's buffer) -- in front of its own plugin call on the same stream,
    so the rows are still the source's -- and records an event.  THEN it waits, on the host and on its stream, for the owners of its
    own context, and makes the plugin call.  Batches are taken in order (the plain loop; the FIFO queue of tools/batch_lanes.run_map),
    so the owners of batch j, all in front of it, have been taken by some thread, whose first act -- without waiting for anything --
    is the copy: no lane waits for a batch nobody runs, and two plugin instances side by side (VSR_BATCH_LANES=2) give the frames of
    one.  A buffer (at most N frames of H x W x 3 bytes) is allocated by its first owner and dropped when its reader returns: with
    one lane at most three are alive (the batch's own, and those of the next two), with L lanes at most L + 2."""

    def __init__(self, frames, jobs):
        self.frames, self.jobs = frames, jobs
        self.lock = threading.Lock()
        self.bufs = {}                                              # reader j -> (its context tensor, the event of its allocation)
        self.done = [threading.Event() for _ in jobs]               # owner i has enqueued its copies ...
        self.events = [None] * len(jobs)                            # ... behind this event of its stream
        self.failed = [False] * len(jobs)
        # owner i -> [(reader j, lo, hi)]: the rows [lo, hi) of batch i that batch j looks back at; reader j -> its owners
        self.readers = [[] for _ in jobs]
        self.owners = [[] for _ in jobs]
        for j, (a, _, ctx_lo, _) in enumerate(jobs):
            for i in range(j - 1, -1, -1):
                lo, hi = max(ctx_lo, jobs[i][0]), min(a, jobs[i][1])
                if jobs[i][1] <= ctx_lo:
                    break
                if lo < hi:
                    self.readers[i].append((j, lo, hi))
                    self.owners[j].append(i)

    def _buffer(self, j, stream):
        """reader j's context tensor, made by whoever asks first, on that thread's stream; every later asker's stream is put behind
        the allocation: the caching allocator orders a block it hands out again only on the stream that allocates it, so a second
        owner copying from another lane's stream could otherwise land in a block whose previous life (an earlier batch's context) the
        allocating stream is still reading"""
        import torch

        with self.lock:
            if j not in self.bufs:
                a, _, ctx_lo, _ = self.jobs[j]
                buf = self.frames.new_empty((a - ctx_lo,) + tuple(self.frames.shape[1:]))
                ev = None
                if stream is not None:
                    ev = torch.cuda.Event()
                    ev.record(stream)
                self.bufs[j] = (buf, ev)
            buf, ev = self.bufs[j]
        if stream is not None:
            stream.wait_event(ev)                                   # (its own stream's event: nothing to wait for)
            buf.record_stream(stream)
        return buf

    def call(self, plugin, j):
        import torch

        a, b, ctx_lo, mask = self.jobs[j]
        # (a host tensor -- the logic's test -- has no streams: the host-side order below is then all there is)
        stream = torch.cuda.current_stream(self.frames.device) if self.frames.is_cuda else None
        try:
            for r, lo, hi in self.readers[j]:
                base = self.jobs[r][2]
                self._buffer(r, stream)[lo - base:hi - base].copy_(self.frames[lo:hi])
            if self.readers[j] and stream is not None:
                ev = torch.cuda.Event()
                ev.record(stream)
                self.events[j] = ev
        except BaseException:
            self.failed[j] = True
            raise
        finally:
            self.done[j].set()
        context = None
        if a > ctx_lo:
            for i in self.owners[j]:
                self.done[i].wait()
                if self.failed[i]:
                    raise RuntimeError(f"sttn-det look-back: the source rows of batch {i} could not be copied aside")
                if stream is not None:
                    stream.wait_event(self.events[i])
            context = self._buffer(j, stream)
        try:
            plugin(self.frames[a:b], mask, context=context)
        finally:
            with self.lock:
                self.bufs.pop(j, None)
