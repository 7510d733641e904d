"""sttn-det with look-back context across batch seams and scene-bounded intervals, without a GPU: the plan of a det list whose first
frames are read-only context (vsr_plan_create_ctx on a det handle, replayed on the CPU by tests/_replay.py as it stands), the new entry
point's refusal without a device, and the one pure function both loops of SubtitleRemover.video_inpaint share (tools/det_lookback.py)."""
import ctypes as C

import numpy as np
import pytest

from vsr_amd.synth import make_state_dict

MH, MW = 240, 432


@pytest.fixture(scope="module")
def host_engine(built_lib):
    from vsr_amd.engine import SttnEngine

    sd = make_state_dict(1, "det")
    eng = SttnEngine(sd, "det", device=None, neighbor_stride=2, ref_length=3)
    yield sd, eng
    eng.close()


def _ctx_view(_lib, eng, L, n_ctx, rows=None):
    from _replay import PlanView

    p = C.c_void_p()
    r = rows or (0, 0)
    _lib.check(_lib.lib.vsr_plan_create_ctx(eng.handle, L, n_ctx, int(r[0]), int(r[1]), 0, 0, C.byref(p)))
    return PlanView(_lib, eng, L, plan_ptr=p)


def _masks(L):
    """the resized mask strip of tests/_replay_check.run_det, the same for every frame of the list (context included)"""
    from oracle import cv2_restate as cv2r

    big = np.zeros((533, 1920, 1), np.uint8)
    big[150:330, 300:1500] = 255
    small = cv2r.resize_linear(big, (MW, MH))[:, :, 0]
    return small, np.stack([small] * L)


def test_det_context_plan_replay(built_lib, host_engine):
    """n_ctx = 3 context frames + 4 written ones against the plain det plan of the same 7 frames (stride 2, refs every 3: windows at
    f = 0, 2, 4, 6; the one at 0 has neighbours 0..2 only and disappears, the one at 2 has neighbours 0..4 of which 3, 4 are written).
    The replay executes exactly the ops the plan holds and starts from zeroed buffers, so context comps that stay zero were never
    written -- although det's dec.out writes EVERY row of the frames it names (the model-resolution blend with the input frame).

    Tolerance: no number of this file's.  The replay's contractions are torch-CPU matmuls, which round by the number of rows they are
    given, so two plans of different extent differ by u8 truncation flips in the decoded image (halved wherever a frame is averaged).
    That figure is measured here on two PLAIN det plans -- the whole image against the decoder rows of the mask -- and is the bound,
    with the margin tests/test_sttn_context.py::test_context_plan_replay applies for the same reason: one flip (max |d| <= 1.0) on
    fewer than 1e-3 of the values, should the two plain plans happen to agree better than that."""
    from vsr_amd import _lib
    from _replay import PlanView, replay

    sd, eng = host_engine
    n_ctx, Ls = 3, 4
    L = n_ctx + Ls
    frames = np.random.default_rng(41).integers(0, 256, size=(L, MH, MW, 3), dtype=np.uint8)
    small, masks = _masks(L)
    ys = np.flatnonzero(small.any(axis=1))
    rows = (int(ys[0]), int(ys[-1]) + 1)
    w = eng.packed_weights()
    plain, ranged, short, ctx = PlanView(_lib, eng, L), PlanView(_lib, eng, L, rows=rows), PlanView(_lib, eng, Ls), _ctx_view(_lib, eng, L, n_ctx)
    try:
        want, counts, _ = replay(plain, w, frames, masks)
        other, counts1, _ = replay(ranged, w, frames, masks)
        assert list(counts1) == list(counts)
        d0 = np.abs(other - want)
        bound_max, bound_frac = max(float(d0.max()), 1.0), max(float((d0 > 0).mean()), 1e-3)
        print(f"two plain det plans (whole image / rows {rows}): max |d| {d0.max()}, differing {float((d0 > 0).mean()):.2e} "
              f"-> bound max |d| <= {bound_max}, differing <= {bound_frac:.2e}")
        got, counts2, _ = replay(ctx, w, frames, masks)
        d = np.abs(got[n_ctx:] - want[n_ctx:])
        print(f"context plan, written frames: max |d| {d.max()}, differing {float((d > 0).mean()):.2e}; "
              f"flops ctx {ctx.flops:.4e} plain {plain.flops:.4e} short {short.flops:.4e}")
        assert d.max() <= bound_max and (d > 0).mean() <= bound_frac, (d.max(), (d > 0).mean(), bound_max, bound_frac)
        assert list(counts2[n_ctx:]) == list(counts[n_ctx:])
        assert list(counts2[:n_ctx]) == [0] * n_ctx
        assert not got[:n_ctx].any()                     # never written
        assert want[:n_ctx].any()                        # (the plain plan does write them)
        # outside the mask the written frames are the RGB input, exactly
        outside = np.broadcast_to((small == 0)[None, :, :, None], got[n_ctx:].shape)
        assert np.array_equal(got[n_ctx:][outside], frames[n_ctx:, ..., ::-1].astype(np.float32)[outside])
        assert short.flops < ctx.flops < plain.flops
        nwin = lambda v: sum(1 for i, _ in v.ops if i.kind == 4)      # OP_DECODE_OUT: one per window
        assert nwin(plain) == 4 and nwin(ctx) == 3       # the window whose neighbours are all context is gone
        for info, _ in ctx.ops:                          # decode ops address written frames only, and blend with the mask
            if info.kind == 4:
                assert (ctx.tables[info.t_frame_idx][: info.n] >= n_ctx).all() and info.buf_mask >= 0
        # the pre-masking and the mask buffer cover the whole list
        im2col = [i for i, _ in ctx.ops if i.tag == b"enc.im2col"]
        assert len(im2col) == 1 and im2col[0].n == L and im2col[0].premask == 1
        assert ctx.buf_elems[im2col[0].buf_mask] >= L * MH * MW
    finally:
        for v in (plain, ranged, short, ctx):
            v.close()


def test_det_plan_without_context_is_the_plain_plan(built_lib, host_engine):
    """n_ctx = 0 on a det handle: op for op and table for table the plan of old; n_ctx = L is refused"""
    from vsr_amd import _lib
    from _replay import PlanView

    sd, eng = host_engine
    a, b = PlanView(_lib, eng, 7, rows=(68, 152)), _ctx_view(_lib, eng, 7, 0, (68, 152))
    try:
        assert a.flops == b.flops and list(a.counts) == list(b.counts) and a.buf_elems == b.buf_elems
        assert len(a.tables) == len(b.tables) and all(np.array_equal(x, y) for x, y in zip(a.tables, b.tables))
        assert len(a.ops) == len(b.ops)
        for (ia, ta), (ib, tb) in zip(a.ops, b.ops):
            assert bytes(ia) == bytes(ib) and [bytes(x) for x in ta] == [bytes(x) for x in tb]
    finally:
        a.close()
        b.close()
    p = C.c_void_p()
    assert _lib.lib.vsr_plan_create_ctx(eng.handle, 4, 4, 0, 0, 0, 0, C.byref(p)) != 0      # nothing left to write
    assert "context" in _lib.last_error()
    assert eng.context_flops(7, 0) == eng.flops(7) and eng.context_flops(7, 3) < eng.flops(7)


def test_det_context_plan_tables_stay_inside_buffers(built_lib):
    """Every gathered address of every GEMM of the det context plans (padded rows included) lies inside its buffer, and the decode
    ops name list frames n_ctx .. L - 1 of buffers sized for the whole list: both window schedules the GPU tests use, lanes 1 and 2,
    the whole image, decoder rows and a decoder box, the list lengths of tests/test_gpu_sttn_det_context.py and config 3's 47 + 10."""
    from vsr_amd import _lib
    from vsr_amd.engine import SttnEngine
    from _replay import PlanView

    checked = 0
    for ns, rl in ((5, 10), (2, 3)):
        eng = SttnEngine(make_state_dict(1, "det"), "det", device=None, neighbor_stride=ns, ref_length=rl)
        try:
            for lanes in (1, 2):
                eng.set_lanes(lanes)
                for L, nc in ((15, 3), (19, 7), (17, 5), (7, 3), (27, 12), (57, 10)):
                    for rows, cols in (((0, 0), (0, 0)), ((68, 152), (0, 0)), ((100, 232), (20, 400))):
                        p = C.c_void_p()
                        _lib.check(_lib.lib.vsr_plan_create_ctx(eng.handle, L, nc, rows[0], rows[1], cols[0], cols[1], C.byref(p)))
                        view = PlanView(_lib, eng, L, plan_ptr=p)
                        try:
                            for info, items in view.ops:
                                if info.kind == 4:                  # OP_DECODE_OUT
                                    idx = view.tables[info.t_frame_idx][: info.n]
                                    assert idx.min() >= nc and idx.max() < L
                                    assert view.buf_elems[info.buf_dst] >= L * MH * MW * 3 and view.buf_elems[info.buf_mask] >= L * MH * MW
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


def test_det_context_entry_point_has_no_cpu_path(built_lib, host_engine):
    lib = built_lib.lib
    if lib.vsr_device_count() > 0:
        pytest.skip("GPU present")
    _, eng = host_engine
    buf = np.zeros(8 * 16 * 3, dtype=np.uint8)
    ar, rc = np.array([[0, 8, 0, 16]], np.int32), np.array([[0, 8]], np.int32)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.vsr_sttn_det_batch_ctx(eng.handle, P(buf), 1, 8, 16, P(buf), 1, P(ar), P(rc), None, P(buf), 1, None) == built_lib.VSR_ERR_NOGPU
    assert "no CPU fallback" in built_lib.last_error()


def _index_jobs_of_today(start_end, n, mask_of, max_load):
    """the walk over frame numbers SubtitleRemover.video_inpaint had of its own before det_jobs became the only one, restated: the job
    list the options being off must give"""
    from vsr_amd.backend.tools.inpaint_tools import batch_generator

    idx, jobs = 0, []
    while idx < n:
        idx += 1
        if idx not in start_end:
            continue
        first, last = idx, start_end[idx]
        idx = min(last, n)
        mask = mask_of(first, last)
        for batch in batch_generator(list(range(first - 1, idx)), max_load):
            if len(batch) >= 1:
                jobs.append((batch[0], batch[-1] + 1, mask))
    return jobs


def test_job_function_properties():
    from vsr_amd.backend.tools.det_lookback import det_jobs, piece_jobs
    from vsr_amd.backend.tools.subtitle_detect import SubtitleDetect

    rng = np.random.default_rng(11)
    for trial in range(300):
        n = int(rng.integers(1, 300))
        max_load = int(rng.integers(1, 60))
        N = int(rng.integers(0, max_load + 1))
        # disjoint 1-based inclusive intervals, some reaching the end of the clip
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
        calls = []

        def mask_of(first, last):
            calls.append((first, last))
            return ("mask", first, last)

        jobs = det_jobs(start_end, n, mask_of, cuts, N, max_load)
        assert calls == sorted(start_end.items())                      # one mask per interval, whatever the cuts
        covered = []
        for lo, hi, ctx_lo, mask in jobs:
            _, first, last = mask
            assert first - 1 <= lo < hi <= last and hi - lo <= max_load
            assert not any(lo < c < hi for c in cuts), "a batch straddles a cut"
            c = max([first - 1] + [x for x in cuts if x <= lo])        # the start of its piece
            assert lo - ctx_lo == min(N, lo - c)
            assert ctx_lo >= c >= first - 1, "context in front of the piece / the interval"
            assert not any(ctx_lo < x <= lo for x in cuts), "context across a cut"
            covered += list(range(lo, hi))
        assert covered == sorted(i for f, l in start_end.items() for i in range(f - 1, l)), "every interval frame is written once, in order"
        # the pieces are the reference's split_range_by_scene, batched one by one
        for f, l in start_end.items():
            pieces = SubtitleDetect.split_range_by_scene([(f, l)], [c + 1 for c in cuts])
            mine = [(lo, hi) for lo, hi, _, m in jobs if m[1] == f]
            assert {s - 1 for s, _ in pieces} <= {lo for lo, _ in mine} and not any(lo < e < hi for lo, hi in mine for _, e in pieces)
            assert piece_jobs(f - 1, l, cuts, N, max_load) == [(lo, hi, c) for lo, hi, c, m in jobs if m[1] == f]
        if not cuts:
            plain = det_jobs(start_end, n, lambda a, b: ("mask", a, b), (), 0, max_load)
            assert [(lo, hi, m) for lo, hi, _, m in plain] == _index_jobs_of_today(start_end, n, lambda a, b: ("mask", a, b), max_load)
            assert all(lo == c for lo, _, c, _ in plain)
    assert piece_jobs(0, 30, [], 5, 12) == [(0, 12, 0), (12, 24, 7), (24, 30, 19)]
    assert piece_jobs(0, 33, [17], 5, 12) == [(0, 11, 0), (11, 17, 6), (17, 27, 17), (27, 33, 22)]


def test_options_and_their_bound():
    from vsr_amd.backend.tools.det_lookback import lookback_options, piece_jobs

    assert lookback_options(50, env={}) == (0, False)                                    # defaults: off
    assert lookback_options(50, env={"VSR_STTN_CONTEXT": "7", "VSR_SCENE_SPLIT": "1"}) == (7, True)
    assert lookback_options(12, env={"VSR_STTN_CONTEXT": "12"}) == (12, False)
    for bad in ("13", "-1", "x", "2.5"):
        with pytest.raises(ValueError, match="sttn-det context"):
            lookback_options(12, env={"VSR_STTN_CONTEXT": bad})
    with pytest.raises(ValueError, match="at most 127"):
        lookback_options(300, env={"VSR_STTN_CONTEXT": "128"})                           # what the engine's plan key holds
    with pytest.raises(ValueError, match="context"):
        piece_jobs(0, 30, [], 13, 12)
    with pytest.raises(ValueError, match="context"):
        piece_jobs(0, 30, [], -1, 12)


def test_resident_lookback_owners():
    """who copies what aside: a context longer than the batch in front of it (batch_generator shrinks the batch size) has two owners"""
    from vsr_amd.backend.tools.det_lookback import ResidentLookback, piece_jobs

    jobs = [j + (None,) for j in piece_jobs(0, 103, [], 50, 50)]
    assert [(lo, hi, c) for lo, hi, c, _ in jobs] == [(0, 41, 0), (41, 82, 0), (82, 103, 32)]
    look = ResidentLookback(None, jobs)
    assert look.owners == [[], [0], [1, 0]]
    assert look.readers == [[(1, 0, 41), (2, 32, 41)], [(2, 41, 82)], []]
    jobs = [j + (None,) for j in piece_jobs(0, 33, [17], 5, 12)]
    look = ResidentLookback(None, jobs)
    assert look.owners == [[], [0], [], [2]] and look.readers[1] == []                   # nothing is kept across the cut


@pytest.mark.parametrize("lanes", [1, 2, 3])
def test_resident_lookback_hands_over_source_rows(lanes):
    """the in-place loop on a host tensor with a stand-in plugin: every batch is overwritten in place, yet every context handed over
    is the SOURCE rows of the definition -- with one lane, and with two or three threads pulling the batches from one queue
    (tools/batch_lanes.run_map) in whatever interleaving; no buffer is left behind"""
    import torch

    from vsr_amd.backend.tools import batch_lanes
    from vsr_amd.backend.tools.det_lookback import ResidentLookback, det_jobs

    n, N, max_load = 400, 50, 50
    start_end = {3: 105, 120: 131, 140: 400}                                         # 103 frames: a context with two owners
    jobs = det_jobs(start_end, n, lambda a, b: (a, b), [200, 310], N, max_load)
    assert len(jobs) > 8 and any(lo - c > 0 for lo, _, c, _ in jobs)
    src = torch.arange(n * 6, dtype=torch.int32).reshape(n, 2, 3)
    for trial in range(5):
        frames = src.clone()
        look = ResidentLookback(frames, jobs)
        seen, lock = {}, __import__("threading").Lock()

        class Plugin:
            def __call__(self, batch, mask, context=None):
                with lock:
                    seen[int(batch[0, 0, 0]) // 6] = None if context is None else context.clone()
                batch.fill_(-1)                                                      # "inpainted": the source rows are gone

        batch_lanes.run_map(list(range(len(jobs))), [Plugin() for _ in range(lanes)], look.call, None)
        assert sorted(seen) == [lo for lo, _, _, _ in jobs]
        for lo, hi, c, _ in jobs:
            if lo == c:
                assert seen[lo] is None
            else:
                assert torch.equal(seen[lo], src[c:lo]), (lo, c)
        assert not look.bufs
        written = torch.zeros(n, dtype=torch.bool)
        for lo, hi, _, _ in jobs:
            written[lo:hi] = True
        assert (frames[written] == -1).all() and torch.equal(frames[~written], src[~written])
