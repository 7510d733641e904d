"""--inpaint-mode opencv without a GPU: the command line accepts it, the statement of OpenCV's Telea fill
(tests/_telea_statement.py) behaves as its formulas say, the C++ plan (csrc/telea_plan.cpp) is the statement's schedule bit for
bit, a level replay of that plan is the serial result bit for bit, and the plugin's host logic."""
import ctypes as C

import numpy as np
import pytest

from tests import _telea_statement as S

CASES = None


def _cases():
    global CASES
    if CASES is None:
        CASES = S.mask_cases()
    return CASES


CASE_NAMES = ["rect", "two_overlapping", "edge_and_corner", "hole", "line", "non255", "whole_frame", "empty", "portrait_odd"]
_serial = S.serial_case


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def test_case_names_cover_the_set():
    assert sorted(CASE_NAMES) == sorted(_cases())


def test_command_line_accepts_opencv():
    from vsr_amd.backend.tools.args_handler import parse_args
    from vsr_amd.backend.tools.constant import InpaintMode

    assert parse_args(["-i", "x", "--inpaint-mode", "opencv"]).inpaint_mode == InpaintMode.OPENCV


# ---- statement sanity: each derivable from the formulas alone ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_overlapping", "edge_and_corner", "whole_frame", "empty"])
def test_statement_leaves_unmasked_pixels(name):
    img, mask, out, sched = _serial(name, "random")
    assert np.array_equal(out[mask == 0], img[mask == 0])
    if name in ("whole_frame", "empty"):
        assert len(sched["yx"]) == 0 and np.array_equal(out, img)           # no band / nothing to fill: the input comes back
    else:
        assert len(sched["yx"]) == int((mask != 0).sum())                    # every masked pixel is reached exactly once
        assert len(np.unique(sched["yx"], axis=0)) == len(sched["yx"])


@pytest.mark.parametrize("name", ["hole", "edge_and_corner", "line"])
def test_statement_keeps_a_constant_image(name):
    """Every gradI is 0, so J = 0 and the value is rint(Ia / s + 0.5).  For c = 0 or a power of two the products w * c are exact
    scalings, every partial sum of Ia is c times the partial sum of s, and Ia / s == c exactly in any float format; c + 0.5 is a
    tie and goes to the even neighbour, c.  So such an image stays as it is.  (For any other c the float32 quotient may land an ulp
    above c, OpenCV's + 0.5 bias then gives c + 1, and from there on the image is no longer constant: nothing is claimed.)"""
    mask = _cases()[name]
    img = np.empty(mask.shape + (3,), np.uint8)
    img[:] = (0, 64, 128)
    out, _ = S.serial(img, mask)
    assert np.array_equal(out, img)


def test_statement_permuting_channels_permutes_the_output():
    img, mask, out, _ = _serial("non255", "random")
    perm = [2, 0, 1]
    out_p, _ = S.serial(np.ascontiguousarray(img[:, :, perm]), mask)
    assert np.array_equal(out_p, out[:, :, perm])


def test_statement_commutes_with_a_shift_away_from_the_edge():
    rng = np.random.default_rng(5)
    H, W = 44, 60
    base = rng.integers(0, 256, (H + 10, W + 10, 3), dtype=np.uint8)
    m0 = np.zeros((H, W), np.uint8)
    m0[12:22, 10:38] = 255
    m0[18:30, 30:44] = 255
    dy, dx = 5, 7
    m1 = np.roll(m0, (dy, dx), (0, 1))
    assert m1[:dy].sum() == 0 and m1[:, :dx].sum() == 0
    img0 = base[dy:dy + H, dx:dx + W]                       # the same scene seen through a window moved by (dy, dx)
    img1 = base[0:H, 0:W]
    out0, s0 = S.serial(np.ascontiguousarray(img0), m0)
    out1, s1 = S.serial(np.ascontiguousarray(img1), m1)
    assert np.array_equal(s1["yx"], s0["yx"] + (dy, dx)) and np.array_equal(s1["level"], s0["level"])
    assert np.array_equal(out1[m1 != 0], out0[m0 != 0])


# ---- the C++ plan ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_engine(built_lib):
    from vsr_amd.engine import TeleaEngine

    eng = TeleaEngine(device=None, max_plans=16)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_plan_equals_the_statement_schedule(built_lib, host_engine, name):
    img, mask, out, sched = _serial(name, "random")
    h = host_engine.plan(mask)
    plan = S.plan_schedule(built_lib.lib, h, mask)
    assert len(plan["yx"]) == len(sched["yx"])
    assert np.array_equal(plan["yx"], sched["yx"]), "same pixels in the same step order"
    assert np.array_equal(_bits(plan["T"]), _bits(sched["T"])), "T bit for bit"
    assert np.array_equal(plan["level"], sched["level"])
    assert np.array_equal(_bits(plan["tmap"]), _bits(sched["tmap"])), "T of the whole padded frame (outer ring included)"
    assert plan["levels"] == (int(sched["level"].max()) if len(sched["level"]) else 0)
    if name in ("whole_frame", "empty"):
        assert len(plan["yx"]) == 0


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("kind", ["random", "smooth"])
def test_level_replay_of_the_plan_equals_serial(built_lib, host_engine, name, kind):
    """the CPU proof that the level schedule is a valid reordering (float32, bit for bit)"""
    img, mask, out, _ = _serial(name, kind)
    plan = S.plan_schedule(built_lib.lib, host_engine.plan(mask), mask)
    assert np.array_equal(S.replay(img, plan, np.float32), out)


@pytest.mark.parametrize("name", ["two_overlapping", "edge_and_corner", "portrait_odd"])
def test_plan_weights_equal_the_statement_weights(built_lib, host_engine, name):
    """the plan stores every tap weight (the kernel only sums): they are the float32 statement's, bit for bit"""
    img, mask, out, _ = _serial(name, "random")
    h = host_engine.plan(mask)
    plan = S.plan_schedule(built_lib.lib, h, mask)
    _, w = S.replay(img, plan, np.float32, return_weights=True)
    P, NT = len(plan["yx"]), built_lib.lib.vsr_telea_plan_taps(h)
    assert NT == 28 and w.shape == (NT, P)
    cw, step = np.zeros((NT, P), np.float32), np.zeros(P, np.int32)
    assert built_lib.lib.vsr_telea_plan_weights(h, cw.ctypes.data_as(C.c_void_p), None) == 0
    assert built_lib.lib.vsr_telea_plan_read(h, None, step.ctypes.data_as(C.c_void_p), None, None) == 0
    assert np.array_equal(_bits(cw), _bits(np.ascontiguousarray(w[:, step])))


def test_float64_statement_replays_too():
    img, mask, out64, sched = _serial("two_overlapping", "smooth", np.float64)
    assert np.array_equal(S.replay(img, sched, np.float64), out64)


def test_no_cpu_fallback_for_telea(built_lib, host_engine):
    if built_lib.lib.vsr_device_count() > 0:
        pytest.skip("GPU present")
    from vsr_amd.engine import TeleaEngine

    with pytest.raises(built_lib.VsrError):
        TeleaEngine(device=0)
    h = host_engine.plan(_cases()["rect"])
    buf = np.zeros(48 * 72 * 3, np.uint8)
    assert built_lib.lib.vsr_telea_inpaint(h, buf.ctypes.data_as(C.c_void_p), buf.size, 1, None) == built_lib.VSR_ERR_NOGPU
    assert "no CPU fallback" in built_lib.last_error()


def test_plan_rejects_bad_arguments(built_lib):
    h = C.c_void_p()
    assert built_lib.lib.vsr_telea_create(C.byref(h), -1, 0) == built_lib.VSR_ERR_ARG
    assert built_lib.lib.vsr_telea_create(C.byref(h), -1, 3) == 0
    m = np.zeros((2, 9), np.uint8)
    assert built_lib.lib.vsr_telea_set_mask(h, m.ctypes.data_as(C.c_void_p), 2, 9) == built_lib.VSR_ERR_ARG
    assert built_lib.lib.vsr_telea_plan_pixels(h) == -1
    built_lib.lib.vsr_telea_destroy(h)


def test_engine_plan_cache(built_lib):
    from vsr_amd.engine import TeleaEngine

    eng = TeleaEngine(device=None, max_plans=2)
    a, b, c = _cases()["rect"], _cases()["line"], _cases()["hole"]
    eng.plan(a); eng.plan(a.copy()); eng.plan(b); eng.plan(a)
    assert (eng.plan_builds, eng.plan_hits) == (2, 2)
    eng.plan(c)                                             # evicts b, the least recently used
    eng.plan(a)
    assert (eng.plan_builds, eng.plan_hits) == (3, 3)
    eng.plan(b)
    assert eng.plan_builds == 4
    eng.close()


# ---- the plugin's host logic, engine faked -----------------------------------------------------------------------------------
class _FakeEngine:
    """stands for TeleaEngine: fills through the numpy replay of the real C++ plan, on CPU tensors"""
    device = "cpu"

    def __init__(self, lib):
        from vsr_amd.engine import TeleaEngine

        self.real = TeleaEngine(device=None)
        self.lib = lib
        self.calls = []

    def inpaint(self, frames, mask, out=None):
        self.calls.append((tuple(frames.shape), mask.shape))
        plan = S.plan_schedule(self.lib, self.real.plan(mask), mask)
        arr = frames.numpy()
        for i in range(arr.shape[0]):
            arr[i] = S.replay(arr[i], plan)
        return frames

    def close(self):
        self.real.close()


def test_plugin_host_logic(built_lib, monkeypatch):
    from vsr_amd.backend.inpaint.opencv_inpaint import OpenCVInpaint

    monkeypatch.delenv("VSR_OPENCV_BACKEND", raising=False)
    fake = _FakeEngine(built_lib.lib)
    plugin = OpenCVInpaint("cuda:0", engine=fake)
    assert plugin.accepts_device_frames and hasattr(plugin, "clone")
    mask = _cases()["rect"]
    frames = [S.random_image(*mask.shape, seed=s) for s in (1, 2, 3)]
    keep = [f.copy() for f in frames]
    mkeep = mask.copy()
    out = plugin(frames, mask)
    assert isinstance(out, list) and len(out) == 3
    assert all(np.array_equal(a, b) for a, b in zip(frames, keep)) and np.array_equal(mask, mkeep), "inputs are not mutated"
    for f, o in zip(frames, out):
        assert o.dtype == np.uint8 and o.shape == f.shape and o is not f
        assert np.array_equal(o, S.serial(f, mask)[0])
    assert plugin([], mask) == []
    one = plugin.inpaint(frames[0], mask[:, :, None])       # a 3-dim [H,W,1] mask, as the other plugins' callers pass
    assert np.array_equal(one, out[0])
    assert fake.real.plan_builds == 1 and fake.real.plan_hits >= 1, "the repeated mask hits the plan cache"
    untouched = plugin(frames[:2], np.zeros_like(mask))
    assert all(np.array_equal(a, b) and a is not b for a, b in zip(untouched, frames))
    plugin.close()
