"""Which gather-GEMM kernels the engines launch, read from their plans on host-only handles, against the lists of the kernel-level
float64 tests (tests/test_gpu_gemm_family.py): a (variant, tile, layout) an engine can launch that HANDOVER, EPI_KERNELS and GUARDED
do not hold fails here, without a GPU.

Every precision setter accepts a host-only handle, so no engine's census needs the gpu mark; vsr_plan_create gives the plan of the
handle's arithmetic (STTN's modes 1 .. 3 have no fused softmax: their P.V is a plain KN GEMM).  The plans are taken at small geometries:
the tile of an op follows its N (pickTile / wideTile of the plans) and its layout, not the picture's size.  The one rule that does
look at sizes -- STTN's modes 2 and 3 send large NK problems to the 256 x 256 kernel -- is restated below and the STTN plans are
long enough (L = 8) for it to apply.  The census is a superset of a default run's launches: ops that the device-side plan hands to
a fused kernel instead (the fused attentions, the narrow-N kernel) are counted with the GEMM kernel they take when the fusion is
switched off."""
import ctypes as C

import numpy as np
import pytest

import _replay_lama
import _replay_pp
import _replay_raft
import _replay_rfc
import test_gpu_gemm_family as fam
from vsr_amd import synth

OP_GEMM = 1
NK, KN = 0, 1
TILE_NAME = {cfg: name for name, (cfg, _, _) in fam.TILES.items()}
CUS = 256                      # compute units of an MI355X (vsr_gg_cus)


def _gemm_ops(_lib, p):
    """(tile_cfg, bmode, tag, [(M, N, K, splitK, act)]) of every GEMM op of a vsr_plan_t"""
    lib = _lib.lib
    out = []
    for i in range(lib.vsr_plan_num_ops(p)):
        info = _lib.VsrOpInfo()
        _lib.check(lib.vsr_plan_op(p, i, C.byref(info)))
        if info.kind != OP_GEMM:
            continue
        items = []
        for j in range(info.nitems):
            it = _lib.VsrGemmInfo()
            _lib.check(lib.vsr_plan_op_gemm(p, i, j, C.byref(it)))
            items.append((it.M, it.N, it.K, it.splitK, it.act))
        out.append((info.tile_cfg, info.bmode, info.tag.decode(), items))
    return out


# ---- the engines' rules, restated --------------------------------------------------------------------------------------------------
def _sttn_triples(mode, ops):
    """sttn_engine.hip gg_variant(): precision 0 -> NK problems on variant 3, KN (P.V) on variant 1; 1 -> 4; 2 -> 5; 3 -> 6.
    build_plan_dev() anchorV7: in modes 2 and 3 an NK problem (a KN one after its B operand was transposed) with N >= 192, K >= 256,
    M >= 1024 and at least half a round of 256 x 256 tiles goes to the 256 x 256 kernel of the same variant."""
    for cfg, bmode, tag, items in ops:
        variant = {0: 1 if bmode == KN else 3, 1: 4, 2: 5, 3: 6}[mode]
        for M, N, K, splitK, act in items:
            big = mode >= 2 and not (bmode == KN and (K % 32 or N % 32)) and N >= 192 and K >= 256 and M >= 1024 and \
                -(-M // 256) * -(-N // 256) * max(splitK, 1) * 2 >= CUS
            yield ((variant, "256x256", NK) if big else (variant, TILE_NAME[cfg], bmode)), tag


def _flow_triples(mode, ops):
    """flow_engine.hip run_plan(): precision 1 -> variant 4, 2 -> variant 7, 0 -> variant 3, or variant 1 where thin_variant() says so
    (a rule on K and the tile count that VSR_FLOW_THIN turns off or forces: either kernel can meet every tile)"""
    for cfg, bmode, tag, _ in ops:
        for variant in {0: (3, 1), 1: (4,), 2: (7,)}[mode]:
            yield (variant, TILE_NAME[cfg], bmode), tag


# backend/tools/ocr_det_nhwc.py emit_gemm(): N >= 128 -> 128x128, N == 32 -> 256x32, else 128x64; variant 3 or thin_variant()'s 1
DETECTOR = [((v, t, NK), "detector") for v in (1, 3) for t in ("128x128", "128x64", "256x32")]


# ---- the plans ---------------------------------------------------------------------------------------------------------------------
def _census(_lib):
    from vsr_amd.engine import LamaEngine, PpEngine, RaftEngine, RfcEngine, SttnEngine

    lib = _lib.lib
    found = {}                                                  # triple -> set of "engine mode N: tag"

    def add(engine, mode, triples):
        for triple, tag in triples:
            found.setdefault(triple, set()).add(f"{engine} mode {mode}: {tag}")

    for variant in ("auto", "det"):
        eng = SttnEngine(synth.make_state_dict(0, variant), variant, device=None)
        try:
            for mode in (0, 1, 2, 3):
                _lib.check(lib.vsr_sttn_set_precision(eng.handle, mode))
                p = C.c_void_p()
                _lib.check(lib.vsr_plan_create(eng.handle, 8, C.byref(p)))
                try:
                    add(f"sttn-{variant}", mode, _sttn_triples(mode, _gemm_ops(_lib, p)))
                finally:
                    lib.vsr_plan_destroy(p)
        finally:
            eng.close()

    def flow(name, eng, setter, view):
        try:
            for mode in (0, 1, 2):
                _lib.check(setter(eng.handle, mode))            # the generator's wideN follows (vsr_pp_set_precision)
                v = view()
                try:
                    add(name, mode, _flow_triples(mode, _gemm_ops(_lib, v.p)))
                finally:
                    v.close()
        finally:
            eng.close()

    e = RaftEngine(synth.make_raft_state_dict(0), device=-1)
    flow("raft", e, lib.vsr_raft_set_precision, lambda: _replay_raft.raft_plan_view(_lib, e, 2, 128, 128, 1))
    f = RfcEngine(synth.make_rfc_state_dict(0), device=-1)
    flow("flow completion", f, lib.vsr_rfc_set_precision, lambda: _replay_rfc.rfc_plan_view(_lib, f, 2, 64, 64))
    g = PpEngine(device=-1, state_dict=synth.make_propainter_state_dict(0))
    masks = np.zeros((2, 64, 96), np.uint8)
    masks[:, 20:40, 30:70] = 1
    flags = g.window_flags(masks)
    flow("generator", g, lib.vsr_pp_set_precision, lambda: _replay_pp.gen_plan_view(_lib, g, 3, 2, 64, 96, flags))
    la = LamaEngine(synth.make_lama_state_dict(3, 1), device=None)
    flow("lama", la, lib.vsr_lama_set_precision, lambda: _replay_lama.lama_plan_view(_lib, la, 1, 32, 48))
    add("detector", 0, DETECTOR)
    return found


@pytest.fixture(scope="module")
def census(built_lib):
    return _census(built_lib)


def _report(missing, found):
    return "\n".join(f"  v{v} {t} {'KN' if m else 'NK'}: {', '.join(sorted(found[(v, t, m)])[:6])}" for v, t, m in sorted(missing))


def test_the_census_sees_what_the_issue_names(census):
    """the census itself: the launches known from reading the plans must turn up, or the test below checks nothing"""
    for triple in ((7, "128x128", NK),         # the generator's token GEMMs in fp16 mode (wideN = 128)
                   (4, "128x128", KN), (7, "128x128", KN), (3, "128x128", KN),      # LaMa's Fourier stages
                   (4, "256x32", NK), (7, "256x32", NK), (4, "256x64", NK), (5, "256x64", NK), (6, "256x32", NK),   # narrow, first / last convs
                   (4, "128x64", KN), (6, "128x64", KN),                            # STTN's P.V in modes 1 and 3
                   (5, "256x256", NK), (6, "256x256", NK)):
        assert triple in census, f"the census no longer finds v{triple[0]} {triple[1]} {'KN' if triple[2] else 'NK'}"


def test_every_launched_kernel_has_its_handover_test(census):
    handover = set(fam.HANDOVER)
    epilogue = {(v, t, m) for v, t, m, _ in fam.EPI_KERNELS}
    missing = [k for k in census if k not in handover and not (k[0] == 1 and k in epilogue)]
    assert not missing, "launched by an engine, absent from HANDOVER (variant 1: from EPI_KERNELS):\n" + _report(missing, census)
    missing = [k for k in census if k not in epilogue]
    assert not missing, "launched by an engine, absent from EPI_KERNELS:\n" + _report(missing, census)


def test_every_reduced_precision_kernel_has_its_guard_and_epilogue_tests(census):
    reduced = [k for k in census if k[0] >= 4]
    assert reduced
    guarded = set(fam.GUARDED)
    missing = [k for k in reduced if k not in guarded]
    assert not missing, "launched by an engine, absent from GUARDED:\n" + _report(missing, census)
    epilogue = {(v, t, m) for v, t, m, _ in fam.EPI_KERNELS}
    missing = [k for k in reduced if k not in epilogue]
    assert not missing, "launched by an engine, absent from EPI_KERNELS:\n" + _report(missing, census)
    # the split-format variants write split-format output too: both rows
    both = {(v, t, m) for v, t, m, o in fam.EPI_KERNELS if o} & {(v, t, m) for v, t, m, o in fam.EPI_KERNELS if not o}
    missing = [k for k in reduced if k[0] in (5, 6) and k not in both]
    assert not missing, "split-format kernels without both output formats in EPI_KERNELS:\n" + _report(missing, census)
