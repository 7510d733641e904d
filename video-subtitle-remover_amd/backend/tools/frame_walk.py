"""The frame walk of SubtitleRemover.propainter_mode (reference backend/main.py:159-245), stated once over a source of frames.

A source is a read() -> (ok, item).  The reader's read() gives host frames; counted(n) gives the 0-based frame numbers of a clip of n
frames and fails at n.  The walk is the same over both, so the host-frame loop (host_items, lazy: tools/batch_parallel._Prefetch runs
it in a thread) and the loops that index a clip in HBM (clip_jobs: the resident clip, resident windows) cannot disagree about which
frames make a batch.  Pure: no torch, no HIP library.  (video_inpaint's walk over frame numbers is tools/det_lookback.det_jobs.)
"""
from .inpaint_tools import batch_generator


def counted(n):
    """read() over the frame numbers 0 .. n - 1 of a clip of n frames"""
    numbers = iter(range(n))

    def read():
        at = next(numbers, None)
        return at is not None, at

    return read


def is_current_frame_no_start(frame_no, continuous_frame_no_list):                 # main.py:90-97
    return any(start_no == frame_no for start_no, _ in continuous_frame_no_list)


def find_frame_no_end(frame_no, continuous_frame_no_list):                          # main.py:100-107
    for start_no, end_no in continuous_frame_no_list:
        if start_no <= frame_no <= end_no:
            return end_no
    return -1


def propainter_walk(read, sub_list, ranges, mask_of, max_load):
    """-> ("pass", x) | ("single", x, mask) | ("work", [x...], mask), lazily, in frame order.  sub_list: {1-based frame number: boxes};
    ranges: [(start, end)] 1-based inclusive, same mask, already cut at the scene changes; mask_of(start): the mask of the interval
    that starts there.  An interval is read whole (a short read ends it with the frames read) and cut by batch_generator(.., max_load);
    a batch of one frame is a `single`.  A listed frame that starts no range is dropped, as is one whose range cannot be found."""
    index = 0
    while True:
        ok, x = read()
        if not ok:
            break
        index += 1
        if index not in sub_list:
            yield ("pass", x)
            continue
        if not is_current_frame_no_start(index, ranges):
            continue
        end = find_frame_no_end(index, ranges)
        if end == -1:
            continue
        start, xs = index, [x]
        while index < end:
            ok, x = read()
            if not ok:
                break
            index += 1
            xs.append(x)
        mask = mask_of(start)
        for batch in ([xs] if len(xs) == 1 else batch_generator(xs, max_load)):
            yield ("single", batch[0], mask) if len(batch) == 1 else ("work", batch, mask)


def host_items(walk, single, passed_through):
    """the walk over host frames as tools/batch_parallel items, lazily: a `single` becomes ("pass", single(frame, mask)), or, with no
    single-frame plugin (None), the frame as it is after passed_through()"""
    for item in walk:
        if item[0] != "single":
            yield item
            continue
        _, frame, mask = item
        if single is None:
            passed_through()
        yield ("pass", single(frame, mask) if single is not None else frame)


def clip_jobs(walk, single, passed_through):
    """the walk over frame numbers -> [(lo, hi, mask)], 0-based, the batches of two frames and more; a `single` is handed to
    single(frame number, mask) on the way, or, with none, counted by passed_through()"""
    jobs = []
    for kind, x, *mask in walk:
        if kind == "work":
            jobs.append((x[0], x[-1] + 1, mask[0]))
        elif kind == "single":
            single(x, mask[0]) if single is not None else passed_through()
    return jobs
