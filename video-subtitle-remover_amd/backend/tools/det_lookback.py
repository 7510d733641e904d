"""sttn-det with scene-bounded intervals and look-back context across batch seams (not in the reference; opt-in).

SubtitleRemover.video_inpaint cuts every subtitle interval into batch_generator batches and inpaints each alone: the first frames of
every batch but the first have no past, and an interval that straddles a scene cut feeds frames of the other scene to the attention.
With the two options of sttn-auto (tools/chunk_parallel.lookback_options: VSR_SCENE_SPLIT=1, VSR_STTN_CONTEXT=N):

  pieces   every interval is cut by SubtitleDetect.split_range_by_scene at the scene starts; a piece keeps its interval's mask
  batches  batch_generator runs per piece: no batch holds a cut in its interior
  context  a batch [a, b) of a piece that starts at c also sees the SOURCE frames [max(a - N, c), a): as decoded, never an inpainted
           result, never in front of the piece.  The frames written for [a, b) are the last b - a frames of what the plugin gives on
           the list context ++ batch (STTNDetInpaint.__call__(frames, mask, context=...), vsr_sttn_det_batch_ctx).
  ahead    (VSR_STTN_LOOKAHEAD=M) a batch [a, b) of a piece [c, e) also sees the SOURCE frames [b, min(b + M, e)): never behind its
           piece, so never across a cut or outside its interval, and every frame it sees shares the interval's one mask.  The frames
           written for [a, b) are those at the batch's positions of what the plugin gives on context ++ batch ++ ahead
           (STTNDetInpaint.__call__(frames, mask, context=..., lookahead=...), vsr_sttn_det_batch_ctx2).

This file holds the definition as one pure function (piece_jobs / det_jobs: both loops of video_inpaint and the tests share it) and the
HBM-resident loop's copies: there the batches are slices of the clip that are inpainted IN PLACE, so the source rows a later batch looks
back at are copied aside on the device before the batch that owns them is inpainted, and the rows a batch looks ahead at are copied
aside by that batch itself before their owners, behind it, may be inpainted (ResidentLookback).
"""
import threading

from .inpaint_tools import batch_generator
from .subtitle_detect import SubtitleDetect

MAX_CONTEXT = 127           # what the plan cache's key holds (vsr_sttn_det_batch_ctx)


_NO_LOOKAHEAD = object()


def lookback_options(max_load, context=None, scene_split=None, env=None, lookahead=_NO_LOOKAHEAD):
    """(n_context, scene_split) of an sttn-det run: the one reading of VSR_STTN_CONTEXT / VSR_SCENE_SPLIT (chunk_parallel.lookback_options),
    with sttn-det's bound: 0 <= N <= config.getSttnMaxLoadNum(), the longest batch.  Off by default.  ValueError for anything else.
    lookahead= (a value, or None = VSR_STTN_LOOKAHEAD): the look-ahead count M is read by the same function under the same bounds and
    the result is (n_context, scene_split, n_lookahead)."""
    from .chunk_parallel import lookback_options as parse

    if lookahead is _NO_LOOKAHEAD:
        n, split = parse(context, scene_split, max_load, env=env, what="sttn-det", bound="getSttnMaxLoadNum()")
        m = None
    else:
        n, split, m = parse(context, scene_split, max_load, env=env, what="sttn-det", bound="getSttnMaxLoadNum()", lookahead=lookahead)
    if n > MAX_CONTEXT:
        raise ValueError(f"sttn-det context: {n} frames asked for, the engine takes at most {MAX_CONTEXT}")
    if m is None:
        return n, split
    if m > MAX_CONTEXT:
        raise ValueError(f"sttn-det look-ahead context: {m} frames asked for, the engine takes at most {MAX_CONTEXT}")
    return n, split, m


def piece_jobs(first, end, cuts, n_context, max_load, n_lookahead=None):
    """The batches of ONE interval, frames [first, end) 0-based -> [(lo, hi, ctx_lo)]: the interval is cut at the scene starts `cuts`
    (0-based indices of frames that start a scene; SubtitleDetect.split_range_by_scene on the 1-based inclusive numbers), every piece
    goes through batch_generator(.., max_load), and the batch [lo, hi) looks back at the source frames [ctx_lo, lo), ctx_lo =
    max(lo - n_context, start of its piece).  No cuts, n_context = 0: the batches video_inpaint has always made, ctx_lo = lo.
    n_lookahead = M (an integer; None: the list above): -> [(lo, hi, ctx_lo, ahead_hi)], the same batches, each of which also looks
    ahead at the source frames [hi, ahead_hi), ahead_hi = min(hi + M, end of its piece)."""
    if not 0 <= int(n_context) <= int(max_load):
        raise ValueError(f"sttn-det context: {n_context} frames asked for, 0 <= N <= getSttnMaxLoadNum() = {int(max_load)} are possible")
    if n_lookahead is not None and not 0 <= int(n_lookahead) <= int(max_load):
        raise ValueError(f"sttn-det look-ahead context: {n_lookahead} frames asked for, 0 <= M <= getSttnMaxLoadNum() = {int(max_load)} are possible")
    if end <= first:
        return []
    out = []
    for s, e in SubtitleDetect.split_range_by_scene([(first + 1, end)], [int(c) + 1 for c in cuts]):
        c = s - 1                                                   # the piece is [c, e) 0-based
        for batch in batch_generator(list(range(c, e)), max_load):
            if len(batch) >= 1:
                job = (batch[0], batch[-1] + 1, max(batch[0] - int(n_context), c))
                out.append(job if n_lookahead is None else job + (min(batch[-1] + 1 + int(n_lookahead), e),))
    return out


def det_jobs(start_end, n, mask_of, cuts=(), n_context=0, max_load=50, n_lookahead=None):
    """The walk of video_inpaint over the frame numbers of a clip of n frames -> [(lo, hi, ctx_lo, mask)], 0-based.  start_end: {first:
    last} 1-based inclusive interval numbers (already clamped to the frame count); mask_of(first, last): the mask of an interval,
    computed once per interval whatever the cuts; cuts: 0-based scene starts.
    n_lookahead = M (None: the list above): -> [(lo, hi, ctx_lo, mask, ahead_hi)] (piece_jobs)."""
    idx, jobs = 0, []
    while idx < n:
        idx += 1
        if idx not in start_end:
            continue
        first, last = idx, start_end[idx]
        idx = min(last, n)                                         # frames first .. idx are read (main.py:300-305)
        mask = mask_of(first, last)
        jobs += [job[:3] + (mask,) + job[3:] for job in piece_jobs(first - 1, idx, cuts, n_context, max_load, n_lookahead)]
    return jobs


class ResidentLookback:
    """The context copies of the HBM-resident loop.  jobs: [(lo, hi, ctx_lo, mask)] or [(lo, hi, ctx_lo, mask, ahead_hi)] (det_jobs)
    in frame order over `frames` (uint8 [n,H,W,3] on the device), each batch inpainted in place by
    plugin(frames[lo:hi], mask, context=...[, lookahead=...]).

    call(plugin, j) runs batch j.  FIRST it copies aside, on the calling thread's current stream, every row of its own batch that a
    later batch looks back at (a context of N <= getSttnMaxLoadNum() frames can span more than one batch, since batch_generator shrinks
    the batch size: every owner copies its own part into the reader's buffer) -- in front of its own plugin call on the same stream,
    so the rows are still the source's -- and records an event.  THEN it waits, on the host and on its stream, for the owners of its
    own context, and makes the plugin call.  Batches are taken in order (the plain loop; the FIFO queue of tools/batch_lanes.run_map),
    so the owners of batch j, all in front of it, have been taken by some thread, whose first act -- without waiting for anything --
    is the copy: no lane waits for a batch nobody runs, and two plugin instances side by side (VSR_BATCH_LANES=2) give the frames of
    one.  A buffer (at most N frames of H x W x 3 bytes) is allocated by its first owner and dropped when its reader returns: with
    one lane at most three are alive (the batch's own, and those of the next two), with L lanes at most L + 2.

    Look-ahead (jobs with ahead_hi) is the mirror image, with the roles turned round: the rows [hi, ahead_hi) batch j looks ahead at
    belong to the batches BEHIND it, which are taken later.  So batch j copies them itself, into a buffer of its own, as part of the
    same first act -- every copy that concerns it, then ONE event -- and a batch k, before its plugin call, also waits (host and
    stream) for every EARLIER batch that reads look-ahead rows out of it.  Every wait, of either kind, is then on a batch taken
    earlier in FIFO order, whose first act waits for nothing: one to three lanes cannot deadlock and give the bytes of one lane.
    The look-ahead buffer (at most M frames) is allocated, filled, read and dropped by batch j on its own stream: one per batch in
    flight, so with L lanes at most L + 2 look-back buffers and L look-ahead buffers are alive, whatever the clip's length."""

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
        # reader j -> the LATER batches its look-ahead rows belong to; owner k -> the EARLIER batches that read look-ahead rows out of it
        self.ahead_hi = [job[4] if len(job) > 4 else job[1] for job in jobs]
        self.ahead_readers = [[] for _ in jobs]
        for j, job in enumerate(jobs):
            for k in range(j + 1, len(jobs)):
                if jobs[k][0] >= self.ahead_hi[j]:
                    break
                self.ahead_readers[k].append(j)
        for j, (a, _, ctx_lo, *_) in enumerate(jobs):
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
                a, _, ctx_lo = self.jobs[j][:3]
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

        a, b, ctx_lo, mask = self.jobs[j][:4]
        ahead = None
        # (a host tensor -- the logic's test -- has no streams: the host-side order below is then all there is)
        stream = torch.cuda.current_stream(self.frames.device) if self.frames.is_cuda else None
        try:
            for r, lo, hi in self.readers[j]:
                base = self.jobs[r][2]
                self._buffer(r, stream)[lo - base:hi - base].copy_(self.frames[lo:hi])
            if self.ahead_hi[j] > b:
                ahead = self.frames[b:self.ahead_hi[j]].clone()    # (this batch's stream allocates, fills, reads and frees it)
            if (self.readers[j] or ahead is not None) and stream is not None:
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
        for i in self.ahead_readers[j]:                             # earlier batches that look ahead into this one have their copy
            self.done[i].wait()
            if self.failed[i]:
                raise RuntimeError(f"sttn-det look-ahead: batch {i} could not copy the source rows of batch {j} aside")
            if stream is not None:
                stream.wait_event(self.events[i])
        try:
            if ahead is not None:
                plugin(self.frames[a:b], mask, context=context, lookahead=ahead)
            else:
                plugin(self.frames[a:b], mask, context=context)
        finally:
            with self.lock:
                self.bufs.pop(j, None)
