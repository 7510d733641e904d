"""tools/frame_walk.py without a GPU: the one walk of SubtitleRemover.propainter_mode, over the reader's frames and over frame numbers,
against the two loops it replaced; and the host-frame consumer stays lazy."""
import numpy as np

from vsr_amd.backend.tools import frame_walk
from vsr_amd.backend.tools.inpaint_tools import batch_generator

WARNING = "warning: no LaMa weights configured (LAMA_MODEL_PATH): isolated subtitle frames pass through"


class _ParentLoops:
    """propainter_mode's index_jobs and items as they stood before tools/frame_walk.py, restated (the mask of an interval is
    mask_of(start), the batch limit max_load): the sequences the one walk must give"""

    def __init__(self, sub_list, ranges, single_frame_inpaint, max_load):
        self.sub_list, self.ranges, self.single_frame_inpaint, self.max_load = sub_list, ranges, single_frame_inpaint, max_load
        self.passed_through_single_frames, self.said = 0, []

    is_current_frame_no_start = staticmethod(lambda frame_no, ranges: any(start_no == frame_no for start_no, _ in ranges))

    @staticmethod
    def find_frame_no_end(frame_no, ranges):
        for start_no, end_no in ranges:
            if start_no <= frame_no <= end_no:
                return end_no
        return -1

    def append_output(self, *args):
        self.said.append(args)

    @staticmethod
    def mask_of(start):
        return ("mask", start)

    def index_jobs(self, n, single):
        sub_list, ranges, single_frame_inpaint = self.sub_list, self.ranges, self.single_frame_inpaint
        index, jobs = 0, []
        while index < n:
            index += 1
            if index not in sub_list or not self.is_current_frame_no_start(index, ranges):
                continue
            start_frame_no = index
            end_frame_no = self.find_frame_no_end(index, ranges)
            if end_frame_no == -1:
                continue
            index = min(end_frame_no, n)
            nos = list(range(start_frame_no - 1, index))
            mask = self.mask_of(start_frame_no)
            for batch in ([nos] if len(nos) == 1 else batch_generator(nos, self.max_load)):
                if len(batch) == 1:
                    if single_frame_inpaint is None:
                        self.passed_through_single_frames += 1
                        if self.passed_through_single_frames == 1:
                            self.append_output(WARNING)
                    else:
                        single(batch[0], mask)
                else:
                    jobs.append((batch[0], batch[-1] + 1, mask))
        return jobs

    def items(self, reader):
        sub_list, ranges, single_frame_inpaint = self.sub_list, self.ranges, self.single_frame_inpaint
        index = 0
        while True:
            ok, frame = reader.read()
            if not ok:
                break
            index += 1
            if index not in sub_list:
                yield ("pass", frame)
                continue
            if not self.is_current_frame_no_start(index, ranges):
                continue
            start_frame_no = index
            end_frame_no = self.find_frame_no_end(index, ranges)
            if end_frame_no == -1:
                continue
            temp_frames = [frame]
            while index < end_frame_no:
                ok, frame = reader.read()
                if not ok:
                    break
                index += 1
                temp_frames.append(frame)
            mask = self.mask_of(start_frame_no)
            for batch in ([temp_frames] if len(temp_frames) == 1 else batch_generator(temp_frames, self.max_load)):
                if len(batch) == 1:
                    if single_frame_inpaint is None:
                        self.passed_through_single_frames += 1
                        if self.passed_through_single_frames == 1:
                            self.append_output(WARNING)
                    yield ("pass", single_frame_inpaint(batch[0], mask) if single_frame_inpaint is not None else batch[0])
                else:
                    yield ("work", batch, mask)


class _Reader:
    """n frames ("frame", 0) .. ("frame", n - 1); counts its read() calls"""

    def __init__(self, n):
        self.n, self.reads = n, 0

    def read(self):
        self.reads += 1
        return (True, ("frame", self.reads - 1)) if self.reads <= self.n else (False, None)


class _Counter:
    """SubtitleRemover._single_passes_through: the counter and the one warning"""

    def __init__(self):
        self.passed_through_single_frames, self.said = 0, []

    def __call__(self):
        self.passed_through_single_frames += 1
        if self.passed_through_single_frames == 1:
            self.said.append((WARNING,))


def _case(rng, trial):
    """total frames, the frames of the file (fewer: a short file), disjoint 1-based inclusive ranges with gaps, the detector's list
    (every frame of every range; in one case of five also a frame of a gap, which starts no range), the batch limit"""
    total = int(rng.integers(1, 261))
    n = int(rng.integers(0, total)) if rng.random() < 0.4 else total
    max_load = int(rng.integers(2, 81))
    ranges, at = [], 1 + int(rng.integers(0, 6))
    while at <= total:
        end = min(total, at + int(rng.choice([1, 2, 3, 31, 91, 201])) - 1)
        ranges.append((at, end))
        at = end + 1 + int(rng.integers(0, 8))        # (0: the next range follows at once, as after a scene cut)
    sub_list = {no: [(no % 3, 10, 0, 5)] for s, e in ranges for no in range(s, e + 1)}
    orphan = None
    if trial % 5 == 0:
        free = [no for no in range(1, total + 1) if no not in sub_list]
        if free:
            orphan = int(rng.choice(free))
            sub_list[orphan] = [(9, 10, 0, 5)]
    return total, n, ranges, sub_list, orphan, max_load


def test_propainter_walk_is_both_parent_loops():
    rng = np.random.default_rng(2024)
    seen = {"short": 0, "single": 0, "orphan": 0, "work": 0}
    for trial in range(1500):
        total, n, ranges, sub_list, orphan, max_load = _case(rng, trial)
        inpaint = (lambda frame, mask: ("inpainted", frame, mask)) if trial % 2 else None
        walk = lambda read: frame_walk.propainter_walk(read, sub_list, ranges, _ParentLoops.mask_of, max_load)
        # host frames
        parent, count = _ParentLoops(sub_list, ranges, inpaint, max_load), _Counter()
        want = list(parent.items(_Reader(n)))
        got = list(frame_walk.host_items(walk(_Reader(n).read), inpaint, count))
        assert got == want
        assert (count.passed_through_single_frames, count.said) == (parent.passed_through_single_frames, parent.said)
        # frame numbers
        parent_i, count_i, singles_want, singles_got = _ParentLoops(sub_list, ranges, inpaint, max_load), _Counter(), [], []
        jobs_want = parent_i.index_jobs(n, lambda at, mask: singles_want.append((at, mask)))
        jobs_got = frame_walk.clip_jobs(walk(frame_walk.counted(n)), (lambda at, mask: singles_got.append((at, mask))) if inpaint else None,
                                        count_i)
        assert jobs_got == jobs_want and singles_got == singles_want
        assert (count_i.passed_through_single_frames, count_i.said) == (parent_i.passed_through_single_frames, parent_i.said)
        # ... and the two kinds of source agree with each other: the batches of the host loop are the jobs, frame for frame
        assert [(item[1], item[2]) for item in want if item[0] == "work"] == [([("frame", i) for i in range(lo, hi)], m) for lo, hi, m in jobs_want]
        assert count_i.passed_through_single_frames == count.passed_through_single_frames
        n_single = len(singles_want) + parent_i.passed_through_single_frames
        assert n_single == sum(1 for item in want if item[0] == "pass" and item[1][0] == "inpainted") + parent.passed_through_single_frames
        seen["short"] += n < total
        seen["single"] += n_single
        seen["orphan"] += orphan is not None and orphan <= n
        seen["work"] += len(jobs_want)
        if orphan is not None and orphan <= n:
            assert ("pass", ("frame", orphan - 1)) not in want, "a listed frame that starts no range is dropped by the host loop"
    assert min(seen.values()) >= 1 and seen["single"] > 1000, seen


def test_find_frame_no_end_without_a_range_skips():
    """a frame that starts a range no range holds (end < start): neither loop makes anything of it"""
    sub_list, ranges = {3: [(0, 1, 0, 1)]}, [(3, 2)]
    walk = lambda read: frame_walk.propainter_walk(read, sub_list, ranges, _ParentLoops.mask_of, 8)
    assert list(walk(_Reader(5).read)) == list(_ParentLoops(sub_list, ranges, None, 8).items(_Reader(5))) \
        == [("pass", ("frame", i)) for i in (0, 1, 3, 4)]
    assert frame_walk.clip_jobs(walk(frame_walk.counted(5)), None, None) == []


def test_host_items_stay_lazy():
    """tools/batch_parallel._Prefetch runs the generator in a thread and the run must not buffer the video: when the first batch comes
    out, the reader has given the frames in front of the interval and the interval, not one more"""
    n, ranges = 400, [(21, 60), (100, 300)]
    sub_list = {no: [(0, 1, 0, 1)] for s, e in ranges for no in range(s, e + 1)}
    reader = _Reader(n)
    items = frame_walk.host_items(frame_walk.propainter_walk(reader.read, sub_list, ranges, _ParentLoops.mask_of, 16), None, _Counter())
    assert reader.reads == 0
    for k in range(20):
        assert next(items) == ("pass", ("frame", k)) and reader.reads == k + 1
    kind, batch, _ = next(items)
    assert kind == "work" and batch[0] == ("frame", 20) and reader.reads == 60
    while next(items)[0] == "work":
        assert reader.reads <= 61
    assert reader.reads == 61
