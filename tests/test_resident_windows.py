"""The window planner of the windowed HBM-resident path (backend/tools/resident_windows.py) and its command-line switch: no GPU."""
import random

import pytest

from vsr_amd.backend.tools.resident_windows import live_bytes, plan_windows

FRAME, KEEP = 240 * 432 * 3, 240 * 432 * 3            # bytes of a BGR frame / of a kept 10-bit 4:2:0 record of the same size


def random_jobs(rng, n):
    """disjoint batches of 1-70 frames in increasing order with gaps of 0-300 between them, inside [0, n)"""
    jobs, at = [], rng.randint(0, 300)
    while True:
        size = rng.randint(1, 70)
        if at + size > n:
            return jobs
        jobs.append((at, at + size))
        at += size + rng.randint(0, 300)


def check_plan(windows, n, jobs, budget, keep):
    assert windows is not None
    assert [lo for lo, _ in windows] == [0] + [hi for _, hi in windows[:-1]] and windows[-1][1] == n      # consecutive, cover [0, n)
    assert all(hi > lo for lo, hi in windows)
    cuts = {hi for _, hi in windows[:-1]}
    for lo, hi in jobs:
        assert not any(lo < c < hi for c in cuts), f"job {(lo, hi)} straddles a boundary"
    assert live_bytes(windows, FRAME, keep) <= budget
    for (a, b), (c, d) in zip(windows, windows[1:]):
        assert ((b - a) + (d - c)) * (FRAME + keep) <= budget


@pytest.mark.parametrize("seed", range(40))
def test_planner_properties(seed):
    rng = random.Random(seed)
    n = rng.randint(1, 5000)
    jobs = random_jobs(rng, n)
    largest = max([hi - lo for lo, hi in jobs], default=1)
    for keep in (0, KEEP):
        per = FRAME + keep
        two_largest, everything = 2 * largest * per, n * per
        budgets = [two_largest, everything] + [rng.randint(two_largest, max(two_largest, everything)) for _ in range(6)]
        for budget in budgets:
            windows = plan_windows(n, jobs, FRAME, budget, keep)
            check_plan(windows, n, jobs, budget, keep)
            if budget >= everything:
                assert windows == [(0, n)]
        assert plan_windows(n, jobs, FRAME, everything + 12345, keep) == [(0, n)]
        if jobs and everything > two_largest - 1:      # a job larger than half the budget: the documented answer, not an exception
            assert plan_windows(n, jobs, FRAME, two_largest - 1, keep) is None


def test_a_job_over_half_the_budget_does_not_fit():
    assert plan_windows(100, [(10, 31)], FRAME, 40 * FRAME) is None            # 21 frames, half the budget holds 20
    assert plan_windows(100, [(10, 30)], FRAME, 40 * FRAME) is not None
    assert plan_windows(100, [(10, 30)], FRAME, 40 * FRAME, KEEP) is None      # ... and 10 with the records kept
    assert plan_windows(100, [], FRAME, FRAME) is None                         # not one frame per window


def test_boundary_cases():
    assert plan_windows(0, [], FRAME, 10 * FRAME) == []
    # no jobs: all pass-through, windows of half the budget
    windows = plan_windows(95, [], FRAME, 20 * FRAME)
    assert windows == [(s, min(s + 10, 95)) for s in range(0, 95, 10)]
    # one job spanning the clip: fits only as one window
    assert plan_windows(50, [(0, 50)], FRAME, 50 * FRAME) == [(0, 50)]
    assert plan_windows(50, [(0, 50)], FRAME, 50 * FRAME - 1) is None
    # a last window of one frame
    windows = plan_windows(21, [(0, 10), (10, 20)], FRAME, 20 * FRAME)
    assert windows == [(0, 10), (10, 20), (20, 21)]
    # a boundary moves in front of the job it would cut
    windows = plan_windows(40, [(7, 15), (15, 23)], FRAME, 20 * FRAME)
    check_plan(windows, 40, [(7, 15), (15, 23)], 20 * FRAME, 0)
    assert windows == [(0, 7), (7, 15), (15, 25), (25, 35), (35, 40)]
    # max_frames bounds the windows beyond the budget (pass A)
    assert plan_windows(30, [], FRAME, 1000 * FRAME, max_frames=16) == [(0, 16), (16, 30)]


def test_parser_and_main_set_the_switch(monkeypatch):
    import os

    from vsr_amd.backend import main as cli
    from vsr_amd.backend.tools.args_handler import parse_args

    assert parse_args(["-i", "x"]).resident_windows is False
    assert parse_args(["-i", "x", "--resident-windows"]).resident_windows is True
    seen = {}

    class FakeRemover:
        def __init__(self, path):
            self.video_out_path = None

        def run(self):
            seen["VSR_IO_RESIDENT"] = os.environ.get("VSR_IO_RESIDENT")

        def append_output(self, *a):
            pass

    monkeypatch.setattr(cli, "SubtitleRemover", FakeRemover)
    monkeypatch.setattr(cli.config.inpaintMode, "value", cli.config.inpaintMode.value)      # (main() sets the mode: put back afterwards)
    monkeypatch.setenv("VSR_IO_RESIDENT", "1")
    cli.main(["-i", "x.y4m"])
    assert seen["VSR_IO_RESIDENT"] == "1"
    cli.main(["-i", "x.y4m", "--resident-windows"])
    assert seen["VSR_IO_RESIDENT"] == "windows"
