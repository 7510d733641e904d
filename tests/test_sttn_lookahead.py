"""Look-ahead context frames (--sttn-lookahead M) without a GPU: the plan of a list whose first n_ctx AND last n_after
frames are read-only context (vsr_plan_create_ctx2, replayed on the CPU by tests/_replay.py as it stands), the job definitions of both
STTN modes, the in-place loop's copies and waits (tools/det_lookback.ResidentLookback), the chunk loop's read-only view of the next
chunk (tools/chunk_parallel.run_chunk_parallel(lookahead=M)), and the option's parsing and refusals."""
import ctypes as C
import threading

import numpy as np
import pytest

from vsr_amd.synth import make_state_dict


@pytest.fixture(scope="module")
def host_engine(built_lib):
    from vsr_amd.engine import SttnEngine

    sd = make_state_dict(0, "auto")
    eng = SttnEngine(sd, "auto", device=None, neighbor_stride=2, ref_length=3)
    yield sd, eng
    eng.close()


def _ctx2_view(_lib, eng, L, n_ctx, n_after, rows=None, cols=None):
    from _replay import PlanView

    p = C.c_void_p()
    r, c = rows or (0, 0), cols or (0, 0)
    _lib.check(_lib.lib.vsr_plan_create_ctx2(eng.handle, L, n_ctx, n_after, int(r[0]), int(r[1]), int(c[0]), int(c[1]), C.byref(p)))
    return PlanView(_lib, eng, L, plan_ptr=p)


_nwin = lambda v: sum(1 for i, _ in v.ops if i.kind == 4)      # OP_DECODE_OUT: one per window


@pytest.mark.parametrize("rows", [None, (76, 118)], ids=["whole", "rows76-118"])
@pytest.mark.parametrize("shape", [(3, 4, 4), (0, 4, 3)], ids=["3+4+4", "0+4+3"])
def test_lookahead_plan_replay(built_lib, host_engine, shape, rows):
    """(n_ctx, Ls, n_after) against the plain plan of the same list (stride 2, refs every 3).  3 + 4 + 4 = 11 frames: the plain plan has
    windows at f = 0, 2, .., 10; f = 0 has neighbours 0..2, all prefix, f = 10 has neighbours 8..10, all suffix: both disappear.  The
    replay executes exactly the ops the plan holds and starts from zeroed buffers, so context comps that stay zero were never written.
    Bound on the written frames: that of tests/test_sttn_context.py::test_context_plan_replay (torch-CPU matmuls round by the number of
    rows they are given: a handful of u8 truncation flips; on the GPU the frames are equal bit for bit,
    tests/test_gpu_sttn_lookahead.py)."""
    from vsr_amd import _lib
    from _replay import PlanView, replay

    sd, eng = host_engine
    n_ctx, Ls, n_after = shape
    L = n_ctx + Ls + n_after
    w0, w1 = n_ctx, n_ctx + Ls
    frames = np.random.default_rng(31).integers(0, 256, size=(L, 120, 640, 3), dtype=np.uint8)
    w = eng.packed_weights()
    plain = PlanView(_lib, eng, L, rows=rows)
    short = PlanView(_lib, eng, Ls, rows=rows)
    new = _ctx2_view(_lib, eng, L, n_ctx, n_after, rows)
    try:
        want, counts, _ = replay(plain, w, frames)
        got, counts2, _ = replay(new, w, frames)
        lo, hi = (0, 120) if rows is None else (rows[0] // 2 * 2, (rows[1] + 1) // 2 * 2)
        d = np.abs(got[w0:w1, lo:hi] - want[w0:w1, lo:hi])
        print(f"{shape} rows {rows}: max |d| {d.max()}, differing {float((d > 0).mean()):.2e}; flops new {new.flops:.4e} plain {plain.flops:.4e} "
              f"short {short.flops:.4e}; windows plain {_nwin(plain)} new {_nwin(new)}")
        assert d.max() <= 1.0 and (d > 0).mean() < 1e-3, (d.max(), (d > 0).mean())
        assert list(counts2[w0:w1]) == list(counts[w0:w1])
        assert list(counts2[:w0]) == [0] * n_ctx and list(counts2[w1:]) == [0] * n_after
        assert not got[:w0].any() and not got[w1:].any()          # never written
        assert want[w1:, lo:hi].any()                              # (the plain plan does write them)
        assert short.flops < new.flops < plain.flops
        if shape == (3, 4, 4):
            assert _nwin(plain) == 6 and _nwin(new) == 4
        # decode ops address written frames only
        seen = set()
        for info, _ in new.ops:
            if info.kind == 4:
                idx = new.tables[info.t_frame_idx][: info.n]
                assert (idx >= w0).all() and (idx < w1).all()
                seen |= set(int(i) for i in idx)
        assert seen == set(range(w0, w1))
    finally:
        plain.close()
        short.close()
        new.close()


def _same_plan(a, b):
    assert a.flops == b.flops and list(a.counts) == list(b.counts) and a.buf_elems == b.buf_elems
    assert len(a.tables) == len(b.tables) and all(np.array_equal(x, y) for x, y in zip(a.tables, b.tables))
    assert len(a.ops) == len(b.ops)
    for (ia, ta), (ib, tb) in zip(a.ops, b.ops):
        assert bytes(ia) == bytes(ib) and [bytes(x) for x in ta] == [bytes(x) for x in tb]


def test_plan_without_lookahead_is_the_plan_of_today(built_lib, host_engine):
    """n_after = 0: op for op and table for table vsr_plan_create_ctx; both counts 0: the plain plan"""
    from vsr_amd import _lib
    from _replay import PlanView

    sd, eng = host_engine
    for L, n in ((7, 3), (7, 0), (11, 5)):
        p = C.c_void_p()
        _lib.check(_lib.lib.vsr_plan_create_ctx(eng.handle, L, n, 76, 118, 0, 0, C.byref(p)))
        a, b = PlanView(_lib, eng, L, plan_ptr=p), _ctx2_view(_lib, eng, L, n, 0, (76, 118))
        try:
            _same_plan(a, b)
        finally:
            a.close()
            b.close()
    a, b = PlanView(_lib, eng, 7, rows=(76, 118)), _ctx2_view(_lib, eng, 7, 0, 0, (76, 118))
    try:
        _same_plan(a, b)
    finally:
        a.close()
        b.close()
    p = C.c_void_p()
    for L, n, m in ((7, 3, 4), (7, 0, 7), (7, 5, 3), (7, 0, -1)):
        assert _lib.lib.vsr_plan_create_ctx2(eng.handle, L, n, m, 0, 0, 0, 0, C.byref(p)) != 0      # nothing left to write
        assert "context" in _lib.last_error()
    assert eng.context_flops(7, 0) == eng.flops(7) and eng.context_flops(7, 3, n_after=0) == eng.context_flops(7, 3)
    assert eng.context_flops(7, 2, n_after=2) < eng.context_flops(7, 2) < eng.flops(7)


@pytest.mark.parametrize("variant", ["auto", "det"])
def test_lookahead_plan_tables_stay_inside_buffers(built_lib, variant):
    """Every gathered address of every GEMM of the new plans (padded rows included) lies inside its buffer, and the decode ops name
    list frames n_ctx .. n_ctx + Ls - 1 of buffers sized for the whole list: the check of
    tests/test_sttn_det_context.py::test_det_context_plan_tables_stay_inside_buffers on both handles, both window schedules the GPU
    tests use, lanes 1 and 2, the whole image and a decoder box, the lists of tests/test_gpu_sttn_lookahead.py and 10 + 47 + 10."""
    from vsr_amd import _lib
    from vsr_amd.engine import SttnEngine
    from _replay import PlanView

    mh, mw = (120, 640) if variant == "auto" else (240, 432)
    box = ((76, 118), (20, 600)) if variant == "auto" else ((100, 232), (20, 400))
    checked = 0
    for ns, rl in ((5, 10), (2, 3)):
        eng = SttnEngine(make_state_dict(0 if variant == "auto" else 1, variant), variant, device=None, neighbor_stride=ns, ref_length=rl)
        try:
            for lanes in (1, 2):
                eng.set_lanes(lanes)
                for L, nc, na in ((16, 0, 4), (23, 5, 6), (24, 3, 9), (28, 7, 9), (14, 5, 5), (11, 3, 4), (67, 10, 10)):
                    for rows, cols in (((0, 0), (0, 0)), box):
                        view = _ctx2_view(_lib, eng, L, nc, na, rows, cols)
                        try:
                            for info, items in view.ops:
                                if info.kind == 4:                  # OP_DECODE_OUT
                                    idx = view.tables[info.t_frame_idx][: info.n]
                                    assert idx.min() >= nc and idx.max() < L - na
                                    assert view.buf_elems[info.buf_dst] >= L * mh * mw * 3
                                    if variant == "det":
                                        assert view.buf_elems[info.buf_mask] >= L * mh * mw
                                    assert view.buf_elems[info.buf_src] >= info.n * (info.pix // 8) * info.ldy
                                if info.kind != 1:
                                    continue
                                bm, bn = _lib.TILE_DIMS[info.tile_cfg]
                                for it in items:
                                    rowA, colA = view.tables[it.tRowA], view.tables[it.tColA]
                                    assert len(rowA) >= it.tilesM * bm and len(colA) >= it.K // 32
                                    lo = it.offA + rowA.min() + colA[: it.K // 32].min()
                                    hi = it.offA + rowA.max() + colA[: it.K // 32].max() + 31
                                    assert 0 <= lo and hi < view.buf_elems[it.bufA], info.tag
                                    rowB, colB = view.tables[it.tRowB], view.tables[it.tColB]
                                    nb = it.K // 32 if info.bmode == 0 else it.tilesN * bn // 32
                                    lo = it.offB + rowB.min() + colB[:nb].min()
                                    hi = it.offB + rowB.max() + colB[:nb].max() + 31
                                    assert 0 <= lo and hi < view.buf_elems[it.bufB], info.tag
                                    rowC, colC = view.tables[it.tRowC], view.tables[it.tColC]
                                    ncc = (it.N + 31) // 32
                                    hi = it.offC + (it.splitK - 1) * it.splitStride + rowC[: it.M].max() + colC[:ncc].max() + 31
                                    assert rowC[: it.M].min() >= 0 and hi < view.buf_elems[it.bufC] + 32, info.tag
                                    checked += 1
                        finally:
                            view.close()
        finally:
            eng.close()
    assert checked > 1000


def test_det_job_function_properties():
    from vsr_amd.backend.tools.det_lookback import det_jobs, piece_jobs
    from vsr_amd.backend.tools.subtitle_detect import SubtitleDetect

    rng = np.random.default_rng(13)
    for trial in range(300):
        n = int(rng.integers(1, 300))
        max_load = int(rng.integers(1, 60))
        N, M = int(rng.integers(0, max_load + 1)), int(rng.integers(0, max_load + 1))
        start_end, at = {}, 1
        while at <= n:
            at += int(rng.integers(0, 40))
            if at > n:
                break
            last = min(n, at + int(rng.integers(0, 130)))
            start_end[at] = last
            at = last + 1
        ncut = int(rng.integers(0, 6)) if trial % 4 else 0
        cuts = sorted({int(c) for c in rng.integers(1, max(2, n), size=ncut) if c < n})
        jobs = det_jobs(start_end, n, lambda a, b: ("mask", a, b), cuts, N, max_load, M)
        today = det_jobs(start_end, n, lambda a, b: ("mask", a, b), cuts, N, max_load)
        assert [j[:4] for j in jobs] == today                              # the same batches, the same look-back
        assert [j[:4] for j in det_jobs(start_end, n, lambda a, b: ("mask", a, b), cuts, N, max_load, 0)] == today
        assert all(j[4] == j[1] for j in det_jobs(start_end, n, lambda a, b: ("mask", a, b), cuts, N, max_load, 0))
        covered = []
        for lo, hi, ctx_lo, mask, ahead_hi in jobs:
            _, first, last = mask
            pieces = [(s - 1, e) for s, e in SubtitleDetect.split_range_by_scene([(first, last)], [c + 1 for c in cuts])]
            c, e = next(p for p in pieces if p[0] <= lo < p[1])            # its piece
            assert c <= lo < hi <= e, "batches partition the piece"
            assert ahead_hi - hi == min(M, e - hi) and hi <= ahead_hi <= e <= last, "look-ahead leaves its piece / exceeds M"
            assert not any(hi < x < ahead_hi or x == hi < ahead_hi for x in cuts), "look-ahead across a cut"
            covered += list(range(lo, hi))
        assert covered == sorted(i for f, l in start_end.items() for i in range(f - 1, l))
    assert piece_jobs(0, 30, [], 5, 12, 4) == [(0, 12, 0, 16), (12, 24, 7, 28), (24, 30, 19, 30)]
    assert piece_jobs(0, 33, [17], 5, 12, 5) == [(0, 11, 0, 16), (11, 17, 6, 17), (17, 27, 17, 32), (27, 33, 22, 33)]
    assert piece_jobs(0, 30, [], 5, 12) == [(0, 12, 0), (12, 24, 7), (24, 30, 19)]
    for bad in (13, -1):
        with pytest.raises(ValueError, match="look-ahead"):
            piece_jobs(0, 30, [], 0, 12, bad)


def test_auto_lookahead_spans_over_scene_chunk_ranges():
    from vsr_amd.backend.tools.chunk_parallel import lookahead_span, scene_chunk_ranges

    rng = np.random.default_rng(17)
    for trial in range(300):
        total = int(rng.integers(1, 400))
        gap = int(rng.integers(1, 60))
        ncut = int(rng.integers(0, 6)) if trial % 5 else 0
        cuts = sorted({int(c) for c in rng.integers(1, max(2, total), size=ncut) if c < total})
        pieces = scene_chunk_ranges(total, gap, cuts)
        ends = cuts + [total]
        for k, (a, b) in enumerate(pieces):
            c1 = min(x for x in ends if x >= b)                            # the end of its scene
            for M in (0, 1, gap // 2, gap):
                lo, hi = lookahead_span(b, c1, M)
                assert lo == b and hi - lo == min(M, c1 - b) and hi <= c1 <= total
                assert not any(b <= x < hi for x in cuts), "never across a cut"
                # what the plugin does with the chunk loop's view: the first rows of the NEXT piece, none when it starts a scene
                if k + 1 < len(pieces):
                    na, nb = pieces[k + 1]
                    assert na == b
                    mine = 0 if na in cuts else min(M, nb - na)
                    assert mine == hi - lo, "M <= clip_gap: the look-ahead never reaches past the next piece of the scene"
                else:
                    assert hi == lo
    assert lookahead_span(12, 30, 0) == (12, 12)


def test_resident_lookahead_readers():
    """who waits for whom: a look-ahead longer than the batch behind it reaches into two batches"""
    from vsr_amd.backend.tools.det_lookback import ResidentLookback, piece_jobs

    jobs = [j[:3] + (None,) + j[3:] for j in piece_jobs(0, 27, [], 0, 12, 12)]
    assert [(j[0], j[1], j[4]) for j in jobs] == [(0, 10, 22), (10, 20, 27), (20, 27, 27)]
    look = ResidentLookback(None, jobs)
    assert look.ahead_readers == [[], [0], [0, 1]] and look.owners == [[], [], []]
    jobs = [j[:3] + (None,) + j[3:] for j in piece_jobs(0, 33, [17], 5, 12, 5)]
    look = ResidentLookback(None, jobs)
    assert look.ahead_readers == [[], [0], [], [2]]                      # nothing is read across the cut
    assert look.owners == [[], [0], [], [2]]


@pytest.mark.parametrize("lanes", [1, 2, 3])
def test_resident_loop_hands_over_source_rows(lanes):
    """the in-place loop on a host tensor with a stand-in plugin: every batch is overwritten in place exactly once, yet every context
    handed over, in front and behind, is the SOURCE rows of the definition -- with one lane, and with two or three threads pulling the
    batches from one queue (tools/batch_lanes.run_map) in whatever interleaving; the run ends (join timeout: a deadlock fails)"""
    import torch

    from vsr_amd.backend.tools import batch_lanes
    from vsr_amd.backend.tools.det_lookback import ResidentLookback, det_jobs

    n, N, M, max_load = 400, 50, 50, 50
    start_end = {3: 105, 120: 131, 140: 400}
    jobs = det_jobs(start_end, n, lambda a, b: (a, b), [200, 310], N, max_load, M)
    assert len(jobs) > 8 and any(j[4] > j[1] for j in jobs) and any(j[0] > j[2] for j in jobs)
    assert any(sum(1 for k in jobs if j[1] <= k[0] < j[4]) > 1 for j in jobs), "a look-ahead that reaches into two batches"
    src = torch.arange(n * 6, dtype=torch.int32).reshape(n, 2, 3)
    for trial in range(5):
        frames = src.clone()
        look = ResidentLookback(frames, jobs)
        seen, writes, lock = {}, [], threading.Lock()

        class Plugin:
            def __call__(self, batch, mask, context=None, lookahead=None):
                with lock:
                    lo = int(batch[0, 0, 0]) // 6
                    seen[lo] = (None if context is None else context.clone(), None if lookahead is None else lookahead.clone())
                    writes.append(lo)
                assert torch.equal(batch, src[lo:lo + batch.shape[0]]), "a batch is still the source's when its turn comes"
                batch.fill_(-1)                                                      # "inpainted": the source rows are gone

        failure = []

        def run():
            try:
                batch_lanes.run_map(list(range(len(jobs))), [Plugin() for _ in range(lanes)], look.call, None)
            except BaseException as e:          # noqa: BLE001
                failure.append(e)

        t = threading.Thread(target=run, daemon=True)
        t.start()
        t.join(60)
        assert not t.is_alive(), "the in-place loop did not end"
        assert not failure, failure
        assert sorted(writes) == [j[0] for j in jobs], "every batch is overwritten exactly once"
        for lo, hi, c, _, ahead_hi in jobs:
            before, after = seen[lo]
            assert (before is None) if lo == c else torch.equal(before, src[c:lo]), (lo, c)
            assert (after is None) if ahead_hi == hi else torch.equal(after, src[hi:ahead_hi]), (hi, ahead_hi)
        assert not look.bufs
        written = torch.zeros(n, dtype=torch.bool)
        for j in jobs:
            written[j[0]:j[1]] = True
        assert (frames[written] == -1).all() and torch.equal(frames[~written], src[~written])


def test_chunk_loop_hands_over_the_next_chunk():
    """run_chunk_parallel(lookahead=M) on device="cpu": process sees the next chunk's first rows as load left them -- a short last chunk
    gives what it has -- and None behind the last chunk; without the argument the calls are those of today"""
    import torch

    from vsr_amd.backend.tools.chunk_parallel import chunk_ranges, run_chunk_parallel

    total, gap, M = 23, 5, 4
    ranges = chunk_ranges(total, gap)
    assert ranges[-1] == (20, 23)
    src = np.random.default_rng(5).integers(0, 256, size=(total, 2, 3, 3), dtype=np.uint8)

    def load(i, out):
        s, e = ranges[i]
        out[: e - s] = src[s:e]

    stored, calls = {}, []

    def store(i, arr):
        stored[i] = np.array(arr)

    def process(i, t, nxt):
        s, e = ranges[i]
        assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), src[s:e])
        calls.append((i, None if nxt is None else nxt.numpy().copy()))
        t.fill_(i)                                   # in place: the next chunk must not have been touched yet

    run_chunk_parallel(ranges, (2, 3, 3), load, process, store, device="cpu", lookahead=M)
    assert [i for i, _ in calls] == list(range(len(ranges)))
    for i, nxt in calls:
        if i + 1 == len(ranges):
            assert nxt is None
        else:
            s, e = ranges[i + 1]
            assert np.array_equal(nxt, src[s:min(s + M, e)]) and len(nxt) == min(M, e - s)
    assert len(calls[-2][1]) == 3                    # the short last chunk: 3 < M rows
    assert all((stored[i] == i).all() and len(stored[i]) == e - s for i, (s, e) in enumerate(ranges))

    old = []
    run_chunk_parallel(ranges, (2, 3, 3), load, lambda *a: old.append(len(a)), store, device="cpu")
    assert old == [2] * len(ranges)
    old.clear()
    run_chunk_parallel(ranges, (2, 3, 3), load, lambda *a: old.append(len(a)), store, device="cpu", lookahead=0)
    assert old == [2] * len(ranges)

    class TwoRanks:
        get_world_size = staticmethod(lambda: 2)
        get_rank = staticmethod(lambda: 0)

    with pytest.raises(RuntimeError, match="one process"):
        run_chunk_parallel(ranges, (2, 3, 3), load, process, store, dist=TwoRanks, device="cpu", lookahead=M)


def test_flags_and_options(built_lib):
    from vsr_amd.backend.tools import det_lookback
    from vsr_amd.backend.tools.args_handler import parse_args
    from vsr_amd.backend.tools.chunk_parallel import lookback_options

    assert parse_args(["-i", "x.y4m"]).sttn_lookahead is None
    a = parse_args(["-i", "x.y4m", "--sttn-lookahead", "6", "--sttn-context", "5"])
    assert a.sttn_lookahead == 6 and a.sttn_context == 5
    assert lookback_options(None, None, 50, env={}, lookahead=None) == (0, False, 0)                   # defaults: off
    assert lookback_options(None, None, 50, env={}) == (0, False)                                      # the call of today
    env = {"VSR_STTN_CONTEXT": "7", "VSR_SCENE_SPLIT": "1", "VSR_STTN_LOOKAHEAD": "9"}
    assert lookback_options(None, None, 50, env=env, lookahead=None) == (7, True, 9)
    assert lookback_options(5, False, 50, env=env, lookahead=3) == (5, False, 3)
    assert lookback_options(0, None, 50, env={}, lookahead=50) == (0, False, 50)                       # independent of N
    for bad in (51, -1, "x", 2.5):
        with pytest.raises(ValueError, match="look-ahead"):
            lookback_options(None, None, 50, env={}, lookahead=bad)
    with pytest.raises(ValueError, match="look-ahead"):
        lookback_options(None, None, 50, env={"VSR_STTN_LOOKAHEAD": "-3"}, lookahead=None)
    # sttn-det: the same reading, its own bound, the engine's limit
    assert det_lookback.lookback_options(50, env={}, lookahead=None) == (0, False, 0)
    assert det_lookback.lookback_options(12, env={"VSR_STTN_LOOKAHEAD": "12"}, lookahead=None) == (0, False, 12)
    for bad in ("13", "-1", "x", "2.5"):
        with pytest.raises(ValueError, match="sttn-det look-ahead"):
            det_lookback.lookback_options(12, env={"VSR_STTN_LOOKAHEAD": bad}, lookahead=None)
    with pytest.raises(ValueError, match="at most 127"):
        det_lookback.lookback_options(300, env={"VSR_STTN_LOOKAHEAD": "128"}, lookahead=None)


def test_main_hands_the_flag_to_the_run(built_lib, monkeypatch):
    """main() turns the flag into the environment the plugins read; a bad value fails in run(), before a frame is read"""
    from vsr_amd.backend import main as m

    seen = {}

    class FakeRemover:
        def __init__(self, path):
            self.sub_areas, self.video_out_path = [], None

        def run(self):
            from vsr_amd.backend.tools.chunk_parallel import lookback_options

            seen["opts"] = lookback_options(None, None, 50, lookahead=None)

        def append_output(self, *a):
            pass

    monkeypatch.setattr(m, "SubtitleRemover", FakeRemover)
    for var in ("VSR_STTN_CONTEXT", "VSR_SCENE_SPLIT", "VSR_STTN_LOOKAHEAD"):     # (main() writes os.environ itself: monkeypatch restores it)
        monkeypatch.setenv(var, "0")
    monkeypatch.setenv("VSR_Y4M_OUT", "444")
    m.main(["-i", "x.y4m", "--sttn-lookahead", "9"])
    assert seen["opts"] == (0, False, 9)
    m.main(["-i", "x.y4m", "--sttn-lookahead", "4", "--sttn-context", "3", "--scene-split"])
    assert seen["opts"] == (3, True, 4)
    with pytest.raises(ValueError, match="look-ahead"):
        m.main(["-i", "x.y4m", "--sttn-lookahead", "51"])


class _TwoRanks:
    get_world_size = staticmethod(lambda: 2)
    get_rank = staticmethod(lambda: 0)


class _NoSource:
    reads = 0

    def info(self):
        _NoSource.reads += 1
        raise AssertionError("the source was opened")

    read = info


def test_sttn_auto_refuses_ranks_and_bad_values_before_a_frame_is_read(built_lib, monkeypatch):
    """the chunk loop's head needs no engine: several ranks with M > 0 are refused by name, a bad M is a ValueError, the reader stays shut"""
    from vsr_amd.backend.inpaint.sttn_auto_inpaint import STTNAutoInpaint

    monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
    plugin = STTNAutoInpaint.__new__(STTNAutoInpaint)
    plugin.video_path, plugin.mask_path, plugin.clip_gap = _NoSource(), None, 12
    plugin.context, plugin.scene_split, plugin.lookahead = 0, False, 5
    with pytest.raises(RuntimeError, match="one process") as e:
        plugin._run(_TwoRanks, None, None, None)
    assert "--sttn-lookahead" in str(e.value)
    plugin.lookahead = None
    monkeypatch.setenv("VSR_STTN_LOOKAHEAD", "5")
    with pytest.raises(RuntimeError, match="--sttn-lookahead"):
        plugin._run(_TwoRanks, None, None, None)
    for bad in (13, -1, "x"):
        plugin.lookahead = bad
        with pytest.raises(ValueError, match="look-ahead"):
            plugin._run(None, None, None, None)
    assert _NoSource.reads == 0


def test_sttn_det_refuses_ranks_and_bad_values_before_a_frame_is_read(built_lib, monkeypatch):
    """video_inpaint's head: several ranks with M > 0 are refused by name and a bad M is a ValueError before the source is opened (the
    refusal of resident windows needs a device plugin: tests/test_gpu_sttn_lookahead.py)"""
    from vsr_amd.backend import main as m

    class Plugin:
        accepts_context = True

    reads = []

    def no_read(*a, **kw):
        reads.append(1)
        raise AssertionError("a frame was read")

    monkeypatch.delenv("VSR_SEAM_FEATHER", raising=False)
    monkeypatch.setattr(m, "open_video", no_read)
    monkeypatch.setattr(m, "SubtitleDetect", no_read)
    sr = m.SubtitleRemover.__new__(m.SubtitleRemover)
    monkeypatch.setenv("VSR_STTN_CONTEXT", "0")
    monkeypatch.setenv("VSR_SCENE_SPLIT", "0")
    monkeypatch.setenv("VSR_STTN_LOOKAHEAD", "5")
    sr._distributed = lambda: _TwoRanks
    with pytest.raises(RuntimeError, match="one process") as e:
        sr.video_inpaint(None, Plugin())
    assert "--sttn-lookahead" in str(e.value)
    sr._distributed = lambda: None
    monkeypatch.setenv("VSR_STTN_LOOKAHEAD", "100000")
    with pytest.raises(ValueError, match="sttn-det look-ahead"):
        sr.video_inpaint(None, Plugin())
    assert not reads


def test_entry_points_have_no_cpu_path(built_lib, host_engine):
    lib = built_lib.lib
    if lib.vsr_device_count() > 0:
        pytest.skip("GPU present")
    from vsr_amd.engine import SttnEngine

    _, eng = host_engine
    buf = np.zeros(8 * 16 * 3, dtype=np.uint8)
    ar, rc = np.array([[0, 8, 0, 16]], np.int32), np.array([[0, 8]], np.int32)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.vsr_sttn_auto_chunk_ctx2(eng.handle, P(buf), 1, 8, 16, P(buf), 1, P(ar), P(rc), None, None, 0, P(buf), 1, P(buf), 1,
                                        None) == built_lib.VSR_ERR_NOGPU
    assert "no CPU fallback" in built_lib.last_error()
    det = SttnEngine(make_state_dict(1, "det"), "det", device=None)
    try:
        assert lib.vsr_sttn_det_batch_ctx2(det.handle, P(buf), 1, 8, 16, P(buf), 1, P(ar), P(rc), None, P(buf), 1, P(buf), 1,
                                           None) == built_lib.VSR_ERR_NOGPU
        assert "no CPU fallback" in built_lib.last_error()
    finally:
        det.close()
