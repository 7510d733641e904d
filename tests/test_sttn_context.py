"""sttn-auto with scene-bounded chunks and look-back context frames, without a GPU: the chunk grid (scene_chunk_ranges), the plan of a
list whose first frames are read-only context (vsr_plan_create_ctx, replayed on the CPU by tests/_replay.py as it stands) and the
options' parsing."""
import ctypes as C

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


def test_scene_chunk_ranges_properties():
    from vsr_amd.backend.tools.chunk_parallel import chunk_ranges, context_span, scene_chunk_ranges

    rng = np.random.default_rng(7)
    for trial in range(300):
        total = int(rng.integers(1, 400))
        gap = int(rng.integers(1, 60))
        ncut = int(rng.integers(0, 6)) if trial % 5 else 0
        cuts = sorted({int(c) for c in rng.integers(1, max(2, total), size=ncut) if c < total})
        pieces = scene_chunk_ranges(total, gap, cuts)
        # an ordered partition of [0, total)
        assert pieces[0][0] == 0 and pieces[-1][1] == total
        assert all(a < b for a, b in pieces) and all(p[1] == q[0] for p, q in zip(pieces, pieces[1:]))
        assert max(b - a for a, b in pieces) <= gap
        assert not any(a < c < b for a, b in pieces for c in cuts)            # no cut in an interior
        assert set(cuts) <= {a for a, _ in pieces}                            # every cut starts a piece
        if not cuts:
            assert pieces == chunk_ranges(total, gap)
        # the grid restarts at every cut: inside a scene every piece but the last is a whole clip_gap
        starts = [0] + cuts
        for a, b in pieces:
            c = max(x for x in starts if x <= a)
            nxt = min([x for x in starts if x > a] + [total])
            assert (a - c) % gap == 0 and b == min(a + gap, nxt)
            for N in (0, 1, gap // 2, gap):
                lo, hi = context_span(a, c, N)
                assert hi == a and hi - lo == min(N, a - c) and lo >= c >= 0
                assert not any(lo < x < a for x in cuts)                  # never across a cut
    # unsorted, repeated and out-of-range cuts are tolerated the way the detector could hand them over
    assert scene_chunk_ranges(10, 4, [7, 7, 0, 10, 12]) == [(0, 4), (4, 7), (7, 10)]


def _ctx_view(_lib, eng, L, n_ctx, rows=None):
    from _replay import PlanView

    p = C.c_void_p()
    r = rows or (0, 0)
    _lib.check(_lib.lib.vsr_plan_create_ctx(eng.handle, L, n_ctx, int(r[0]), int(r[1]), 0, 0, C.byref(p)))
    return PlanView(_lib, eng, L, plan_ptr=p)


@pytest.mark.parametrize("rows", [None, (76, 118)], ids=["whole", "rows76-118"])
def test_context_plan_replay(built_lib, host_engine, rows):
    """n_ctx = 3 context frames + 4 written ones against the plain plan of the same 7 frames (stride 2, refs every 3: windows at
    f = 0, 2, 4, 6; the window at 0 has neighbours 0..2 only and disappears, the one at 2 has neighbours 0..4 of which 3, 4 are
    written).  The replay executes exactly the ops the plan holds and starts from zeroed buffers, so context comps that stay zero
    were never written.  Bound on the written frames: the one test_plan_replay_decoder_rows uses for two plans of different extent
    (torch-CPU matmuls round by the number of rows they are given: a handful of u8 truncation flips; on the GPU the frames are equal bit
    for bit, tests/test_gpu_sttn_context.py)."""
    from vsr_amd import _lib
    from _replay import PlanView, replay

    sd, eng = host_engine
    n_ctx, Ls = 3, 4
    L = n_ctx + Ls
    frames = np.random.default_rng(31).integers(0, 256, size=(L, 120, 640, 3), dtype=np.uint8)
    w = eng.packed_weights()
    plain = PlanView(_lib, eng, L, rows=rows)
    short = PlanView(_lib, eng, Ls, rows=rows)
    ctx = _ctx_view(_lib, eng, L, n_ctx, rows)
    try:
        want, counts, _ = replay(plain, w, frames)
        got, counts2, _ = replay(ctx, w, frames)
        lo, hi = (0, 120) if rows is None else (rows[0] // 2 * 2, (rows[1] + 1) // 2 * 2)
        d = np.abs(got[n_ctx:, lo:hi] - want[n_ctx:, lo:hi])
        print(f"rows {rows}: max |d| {d.max()}, differing {float((d > 0).mean()):.2e}; flops ctx {ctx.flops:.4e} plain {plain.flops:.4e} short {short.flops:.4e}")
        assert d.max() <= 1.0 and (d > 0).mean() < 1e-3, (d.max(), (d > 0).mean())
        assert list(counts2[n_ctx:]) == list(counts[n_ctx:])
        assert list(counts2[:n_ctx]) == [0] * n_ctx
        assert not got[:n_ctx].any()                     # never written
        assert want[:n_ctx, lo:hi].any()                 # (the plain plan does write them)
        assert short.flops < ctx.flops < plain.flops
        # the same encoder: everything before the first window op is the plain plan's
        nwin = lambda v: sum(1 for i, _ in v.ops if i.kind == 4)      # OP_DECODE_OUT: one per window
        assert nwin(plain) == 4 and nwin(ctx) == 3
        # decode ops address written frames only
        for info, _ in ctx.ops:
            if info.kind == 4:
                assert (ctx.tables[info.t_frame_idx][: info.n] >= n_ctx).all()
    finally:
        plain.close()
        short.close()
        ctx.close()


def test_context_plan_without_context_is_the_plain_plan(built_lib, host_engine):
    """n_ctx = 0: op for op and table for table the plan of old (the engine's entry point then gives the bits of _box)"""
    from vsr_amd import _lib
    from _replay import PlanView

    sd, eng = host_engine
    a, b = PlanView(_lib, eng, 7, rows=(76, 118)), _ctx_view(_lib, eng, 7, 0, (76, 118))
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


def test_context_entry_point_has_no_cpu_path(built_lib, host_engine):
    lib = built_lib.lib
    if lib.vsr_device_count() > 0:
        pytest.skip("GPU present")
    _, eng = host_engine
    buf = np.zeros(8 * 16 * 3, dtype=np.uint8)
    ar, rc = np.array([[0, 8, 0, 16]], np.int32), np.array([[0, 8]], np.int32)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.vsr_sttn_auto_chunk_ctx(eng.handle, P(buf), 1, 8, 16, P(buf), 1, P(ar), P(rc), None, None, 0, P(buf), 1, None) == built_lib.VSR_ERR_NOGPU
    assert "no CPU fallback" in built_lib.last_error()


def test_flags_and_options(built_lib):
    from vsr_amd.backend.tools.args_handler import parse_args
    from vsr_amd.backend.tools.chunk_parallel import lookback_options

    a = parse_args(["-i", "x.y4m"])
    assert a.scene_split is False and a.sttn_context is None
    a = parse_args(["-i", "x.y4m", "--scene-split", "--sttn-context", "5"])
    assert a.scene_split is True and a.sttn_context == 5
    assert parse_args(["-i", "x.y4m", "--sttn-context", "-2"]).sttn_context == -2      # parsed; refused by the run (below)
    assert lookback_options(None, None, 50, env={}) == (0, False)                       # defaults: off
    assert lookback_options(None, None, 50, env={"VSR_STTN_CONTEXT": "7", "VSR_SCENE_SPLIT": "1"}) == (7, True)
    assert lookback_options(5, False, 50, env={"VSR_STTN_CONTEXT": "7", "VSR_SCENE_SPLIT": "1"}) == (5, False)
    assert lookback_options(50, True, 50, env={}) == (50, True)
    for bad in (51, -1, "x", 2.5):
        with pytest.raises(ValueError, match="context"):
            lookback_options(bad, None, 50, env={})
    with pytest.raises(ValueError, match="context"):
        lookback_options(None, None, 50, env={"VSR_STTN_CONTEXT": "-3"})


def test_main_hands_the_flags_to_the_run(built_lib, monkeypatch):
    """main() turns the flags into the environment the plugin reads; a bad value fails in run(), before a frame is read"""
    from vsr_amd.backend import main as m

    seen = {}

    class FakeRemover:
        def __init__(self, path):
            self.sub_areas, self.video_out_path = [], None

        def run(self):
            from vsr_amd.backend.tools.chunk_parallel import lookback_options

            seen["opts"] = lookback_options(None, None, 50)

        def append_output(self, *a):
            pass

    monkeypatch.setattr(m, "SubtitleRemover", FakeRemover)
    monkeypatch.setenv("VSR_STTN_CONTEXT", "0")      # (main() writes os.environ itself: these two lines make monkeypatch restore it)
    monkeypatch.setenv("VSR_SCENE_SPLIT", "0")
    monkeypatch.setenv("VSR_Y4M_OUT", "444")
    m.main(["-i", "x.y4m", "--sttn-context", "9", "--scene-split"])
    assert seen["opts"] == (9, True)
    with pytest.raises(ValueError, match="context"):
        m.main(["-i", "x.y4m", "--sttn-context", "51"])
