"""--opencv-fill exemplar without a GPU: the statement's own properties (tests/_exemplar_statement.py), its quality against the Telea
statement on the fixed test texture, the host plan of csrc/exemplar_plan.cpp against the statement byte for byte (a handle with
device < 0), and the host logic: the option, the parser, the cv2 clash, and that nothing of it is touched while the option is off."""
import numpy as np
import pytest

from tests import _exemplar_statement as es
from tests import _telea_statement as ts

THREE = ("48x64", "37x53", "96x160")
_filled = {}


def filled(name):
    """the statement's fill of a case, computed once"""
    if name not in _filled:
        clean, img, mask = es.case(name)
        out = es.fill(img, mask)
        out.setflags(write=False)
        _filled[name] = (clean, img, mask, out)
    return _filled[name]


# ---- the statement ------------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_the_issues():
    assert es.CASES["48x64"] == (48, 64, [(18, 30, 12, 52)])                 # a 12 x 40 hole, interior
    assert es.CASES["37x53"] == (37, 53, [(25, 37, 8, 53)])                  # touches the bottom and the right edge, odd sizes
    assert es.CASES["96x160"] == (96, 160, [(36, 60, 20, 140)])              # 24 x 120
    clean, img, mask = es.case("48x64")
    assert (img[mask != 0] == 255).all() and np.array_equal(img[mask == 0], clean[mask == 0])
    y, x = 7, 9
    base = 110 + 60 * (((x + y // 2) // 4) % 2) + 30 * ((y // 6) % 2)
    noise = int(es.hash32(0, y, x) % np.uint64(17)) - 8
    assert clean[y, x].tolist() == [base + noise, base // 2 + 60 + noise, 255 - base + noise]


@pytest.mark.parametrize("name", THREE)
def test_outside_the_mask_nothing_changes_and_two_runs_agree(name):
    clean, img, mask, out = filled(name)
    assert np.array_equal(out[mask == 0], img[mask == 0])
    assert (out[mask != 0] != 255).any()
    assert np.array_equal(es.fill(img, mask), out), "two runs give the same bytes"


@pytest.mark.parametrize("name", THREE)
def test_the_fill_does_not_depend_on_the_frame_index(name):
    clean, img, mask, out = filled(name)
    other = es.case(name, seed=5)[1]
    a = es.exemplar(np.stack([img, other, img]), mask)
    b = es.exemplar(np.stack([other, img]), mask)
    assert np.array_equal(a[0], out) and np.array_equal(a[2], out) and np.array_equal(b[1], out)
    assert np.array_equal(a[1], b[0]) and not np.array_equal(a[1], out)


def test_an_empty_mask_changes_nothing_and_hopeless_masks_are_refused():
    clean, img, mask = es.case("48x64")
    assert np.array_equal(es.fill(img, np.zeros_like(mask)), img)
    assert es.plan(np.zeros_like(mask)) == ([], None)
    with pytest.raises(ValueError, match="no 7x7 patch"):
        es.fill(img, np.full_like(mask, 255))
    with pytest.raises(ValueError, match="no 7x7 patch"):
        es.fill(img[:6, :6], es.box_mask(6, 6, (2, 3, 2, 3)))


@pytest.mark.parametrize("name", THREE)
def test_quality_at_most_half_of_teleas_error(name):
    clean, img, mask, out = filled(name)
    telea = ts.serial(img, mask, 3, np.float32)
    telea = telea[0] if isinstance(telea, tuple) else telea
    hole = mask != 0
    mae = lambda a: float(np.abs(a[hole].astype(np.int64) - clean[hole].astype(np.int64)).mean())
    print(f"{name}: exemplar MAE {mae(out):.2f}, Telea MAE {mae(telea):.2f}, ratio {mae(out) / mae(telea):.3f}")
    assert mae(out) <= 0.5 * mae(telea)


def test_level_counts():
    assert len(es.plan(es.case("thin")[2])[0]) == 1, "a hole 3 rows tall: one level"
    assert es.CASES["thin"][2][0][1] - es.CASES["thin"][2][0][0] == 3
    assert len(es.plan(es.case("96x160")[2])[0]) >= 3
    lv = es.plan(es.case("37x53")[2])[0]
    assert [(l["H"], l["W"]) for l in lv] == [(37, 53), (19, 27)]


def test_hash_is_a_fixed_32_bit_mix():
    assert int(es.hash32(1, 2, 3)) == int(es.hash32(np.array([1]), 2, 3)[0]) < 2 ** 32
    h = es.hash32(0, 0, 0, 0, np.arange(64)[:, None], np.arange(64)[None])
    assert len(np.unique(h)) == 64 * 64 and abs(float((h % np.uint64(17)).mean()) - 8.0) < 0.5


# ---- the host plan against the statement --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_engine(built_lib):
    from vsr_amd.engine import ExemplarEngine

    eng = ExemplarEngine(device=None)
    yield eng
    eng.close()


@pytest.mark.parametrize("name", THREE + ("64x96_two", "thin"))
def test_host_plan_equals_the_statement(host_engine, name):
    mask = es.case(name)[2]
    want, table = es.plan(mask)
    got = host_engine.plan_levels(mask)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g["H"], g["W"]) == (w["H"], w["W"])
        assert np.array_equal(g["S"], w["S"]) and g["S"].dtype == np.int16
        assert np.array_equal(g["D"], w["D"])
        assert np.array_equal(g["tiles"], w["tiles"])
        assert g["box"] == w["box"] and g["holes"] == int(w["hole"].sum())
        assert np.array_equal(g["cls"], w["hole"] * 1 + w["valid"] * 2 + w["target"] * 4)
    assert np.array_equal(host_engine.plan_init(mask), table)
    if name == "thin":
        assert len(got) == 1
    if name == "96x160":
        assert len(got) >= 3


def test_host_plan_refusals_and_cache(host_engine, built_lib):
    with pytest.raises(built_lib.VsrError, match="no 7x7 patch"):
        host_engine.plan(np.full((48, 64), 255, np.uint8))
    with pytest.raises(built_lib.VsrError, match="no 7x7 patch"):
        host_engine.plan(es.box_mask(6, 6, (2, 3, 2, 3)))
    assert host_engine.plan_levels(np.zeros((48, 64), np.uint8)) == []
    mask = es.case("48x64")[2]
    host_engine.plan(mask)
    hits = host_engine.plan_hits
    host_engine.plan(mask.copy())
    assert host_engine.plan_hits == hits + 1
    # a host-only handle computes nothing
    import ctypes as C

    frames = np.zeros((1, 48, 64, 3), np.uint8)
    rc = built_lib.lib.vsr_exemplar_inpaint(host_engine.plan(mask), frames.ctypes.data_as(C.c_void_p), 48 * 64 * 3, 1, None, 0, None)
    assert rc == built_lib.VSR_ERR_NOGPU and "no CPU fallback" in built_lib.last_error()


# ---- options --------------------------------------------------------------------------------------------------------------------------------
def test_fill_option(monkeypatch, built_lib):
    from vsr_amd.backend.inpaint.opencv_inpaint import fill_option

    monkeypatch.delenv("VSR_OPENCV_FILL", raising=False)
    assert fill_option() == "telea" and fill_option("") == "telea" and fill_option("telea") == "telea"
    assert fill_option("exemplar") == "exemplar" and fill_option(" Exemplar ") == "exemplar"
    monkeypatch.setenv("VSR_OPENCV_FILL", "exemplar")
    assert fill_option() == "exemplar" and fill_option("telea") == "telea", "an argument wins over the environment"
    monkeypatch.setenv("VSR_OPENCV_FILL", "")
    assert fill_option() == "telea"
    for bad in ("patchmatch", "1", "ns"):
        with pytest.raises(ValueError, match="opencv fill"):
            fill_option(bad)
        monkeypatch.setenv("VSR_OPENCV_FILL", bad)
        with pytest.raises(ValueError, match="opencv fill"):
            fill_option()


def test_parser(built_lib):
    from vsr_amd.backend import main as m
    from vsr_amd.backend.tools.args_handler import parse_args

    assert parse_args(["-i", "x.y4m"]).opencv_fill is None
    assert parse_args(["-i", "x.y4m", "--inpaint-mode", "opencv", "--opencv-fill", "exemplar"]).opencv_fill == "exemplar"
    assert parse_args(["-i", "x.y4m", "--inpaint-mode", "opencv", "--opencv-fill", "telea"]).opencv_fill == "telea"
    assert parse_args(["-i", "x.y4m", "--opencv-fill", "telea"]).opencv_fill == "telea"
    for bad in (["--opencv-fill", "exemplar"], ["--inpaint-mode", "lama", "--opencv-fill", "exemplar"],
                ["--inpaint-mode", "sttn-det", "--opencv-fill", "exemplar"], ["--inpaint-mode", "opencv", "--opencv-fill", "fancy"]):
        with pytest.raises(SystemExit):
            parse_args(["-i", "x.y4m"] + bad)
    assert ("opencv_fill", "VSR_OPENCV_FILL", str) in m.FLAG_ENV


def test_flag_sets_the_environment_variable(monkeypatch, built_lib):
    import os

    from vsr_amd.backend import main as m
    from vsr_amd.backend.config import config

    seen = {}

    class Stop(Exception):
        pass

    def fake_remover(path):
        seen["env"] = os.environ.get("VSR_OPENCV_FILL")
        raise Stop

    monkeypatch.setenv("VSR_OPENCV_FILL", "")
    monkeypatch.setattr(m, "SubtitleRemover", fake_remover)
    old = config.inpaintMode.value
    try:
        with pytest.raises(Stop):
            m.main(["-i", "x.y4m", "--inpaint-mode", "opencv", "--opencv-fill", "exemplar"])
    finally:
        config.inpaintMode.value = old
    assert seen["env"] == "exemplar"


class _Spy:
    """the library, remembering every symbol that is looked up"""

    def __init__(self, lib):
        self._lib, self.seen = lib, []

    def __getattr__(self, name):
        self.seen.append(name)
        return getattr(self._lib, name)


def test_option_off_builds_a_telea_engine_and_touches_no_exemplar_symbol(monkeypatch, built_lib):
    from vsr_amd import engine
    from vsr_amd.backend.inpaint import opencv_inpaint as oi

    spy = _Spy(built_lib.lib)
    monkeypatch.setattr(engine, "lib", spy)
    monkeypatch.setattr(engine, "require_gpu", lambda: None)
    monkeypatch.setattr(oi, "_device_index", lambda device: -1)              # host-side handles: this test runs without a GPU
    monkeypatch.delenv("VSR_OPENCV_BACKEND", raising=False)
    for value in (None, "", "telea"):
        if value is None:
            monkeypatch.delenv("VSR_OPENCV_FILL", raising=False)
        else:
            monkeypatch.setenv("VSR_OPENCV_FILL", value)
        p = oi.OpenCVInpaint("cuda:0")
        assert type(p.engine) is engine.TeleaEngine and p.fill == "telea"
        q = p.clone()
        assert type(q.engine) is engine.TeleaEngine
        mask = es.case("48x64")[2]
        assert np.array_equal(p.composite_mask(mask), (mask != 0).astype(np.uint8)) and p.sample_rows(mask) == (0, 48)
        p.engine.plan(mask)
        p.close()
        q.close()
    assert spy.seen and not [s for s in spy.seen if "exemplar" in s], spy.seen
    # ... and on: an ExemplarEngine, which clone() keeps, and the same composite mask and sample rows
    monkeypatch.setenv("VSR_OPENCV_FILL", "exemplar")
    p = oi.OpenCVInpaint("cuda:0")
    monkeypatch.delenv("VSR_OPENCV_FILL")
    q = p.clone()
    assert type(p.engine) is engine.ExemplarEngine and type(q.engine) is engine.ExemplarEngine and q.fill == "exemplar"
    assert np.array_equal(p.composite_mask(mask), (mask != 0).astype(np.uint8)) and p.sample_rows(mask) == (0, 48)
    assert any("vsr_exemplar_create" == s for s in spy.seen)
    p.close()
    q.close()


def test_a_passed_engine_decides_the_fill(monkeypatch, built_lib):
    from vsr_amd import engine
    from vsr_amd.backend.inpaint import opencv_inpaint as oi

    monkeypatch.setattr(oi, "_device_index", lambda device: -1)
    monkeypatch.delenv("VSR_OPENCV_BACKEND", raising=False)
    monkeypatch.setenv("VSR_OPENCV_FILL", "exemplar")                        # the environment is not asked when an engine is passed
    te, ee = engine.TeleaEngine(device=None), engine.ExemplarEngine(device=None)
    try:
        p = oi.OpenCVInpaint("cuda:0", engine=te)
        assert p.engine is te and p.fill == "telea"
        q = p.clone()
        assert type(q.engine) is engine.TeleaEngine
        q.close()
        p = oi.OpenCVInpaint("cuda:0", engine=ee, fill="exemplar")
        assert p.engine is ee and p.fill == "exemplar"
        q = p.clone()
        assert type(q.engine) is engine.ExemplarEngine
        q.close()
        with pytest.raises(ValueError, match="does not match the engine"):
            oi.OpenCVInpaint("cuda:0", engine=te, fill="exemplar")
        with pytest.raises(ValueError, match="does not match the engine"):
            oi.OpenCVInpaint("cuda:0", engine=ee, fill="telea")
    finally:
        te.close()
        ee.close()


def test_cv2_backend_and_exemplar_clash(monkeypatch, built_lib):
    from vsr_amd import engine
    from vsr_amd.backend.inpaint import opencv_inpaint as oi

    monkeypatch.setattr(engine, "require_gpu", lambda: None)
    monkeypatch.setattr(oi, "_device_index", lambda device: -1)
    monkeypatch.setenv("VSR_OPENCV_BACKEND", "cv2")
    monkeypatch.setenv("VSR_OPENCV_FILL", "exemplar")
    with pytest.raises(ValueError, match="cv2"):
        oi.OpenCVInpaint("cuda:0")
    monkeypatch.setenv("VSR_OPENCV_FILL", "fancy")
    with pytest.raises(ValueError, match="opencv fill"):
        oi.OpenCVInpaint("cuda:0")
