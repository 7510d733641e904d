"""The kernel instantiations that only an environment switch selects (VSR_V5_STAGES, VSR_V6_STAGES, VSR_F16_KERNEL,
VSR_V7_ORDER; gather_gemm.hip launch_v5 / launch_v7 read them once per process) against the float64 reference: one child process per
setting and tile (tests/_gemm_stages_child.py), one after another, each holding an epilogue-matrix launch and a hand-over launch of
three tiles per resident workgroup to the bounds B1, B2, B3 of tests/test_gpu_gemm_family.py.  Where the code shows that a switch leaves
the k order and the MFMA sequence of every output element alone, the output bytes must be those of the default setting as well."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_gemm_stages_child.py")
SWITCHES = ("VSR_V5_STAGES", "VSR_V6_STAGES", "VSR_F16_KERNEL", "VSR_V7_ORDER")
_default = {}
_failed = []          # a child that did not end with 0: no further child is started in this session


def _child(setting, tile, variants):
    assert not _failed, f"not started: the child of {_failed[0]} failed before"
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(setting)
    r = subprocess.run([sys.executable, CHILD, tile] + [str(v) for v in variants], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        _failed.append((setting, tile))
    assert r.returncode == 0, (setting, tile, r.returncode, r.stdout[-3000:] + r.stderr[-3000:])
    for ln in r.stdout.splitlines():
        if ln.startswith("RATIO"):
            print(ln.replace("RATIO |", f"RATIO | {' '.join(f'{k}={v}' for k, v in setting.items()) or 'default'} |", 1))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("STAGES ")][-1][7:])


def _defaults(tile, variants):
    """the default setting's digests of a tile (one child per tile, shared by the tests)"""
    have = _default.setdefault(tile, {})
    want = [v for v in variants if f"v{v}" not in have]
    if want:
        have.update(_child({}, tile, want))
    return have


def _same(a, b, variant):
    return all(a[f"v{variant}"][k] == b[f"v{variant}"][k] for k in ("epilogue", "handover", "tiles"))


@pytest.mark.parametrize("tile", ["128x64", "128x128"])
@pytest.mark.parametrize("stages", [2, 3, 4])
def test_v5_stage_count(built_lib, gpu_device, stages, tile):
    """VSR_V5_STAGES: the buffer count of gather_gemm_f32_v5 on the 128-row NK tiles (default 2 on 128x64, 3 on 128x128)."""
    got = _child({"VSR_V5_STAGES": str(stages)}, tile, [5, 6])
    base = _defaults(tile, [5, 6])
    # gather_gemm_v5.h: STAGES sets the pipeline depth D = STAGES - 1 and the buffer a chunk lands in; the chunks are still consumed
    # kc = kcBeg, kcBeg + 1, ... and compute_chunk() issues the same MFMAs on the same fragments per chunk: the same bits
    assert _same(got, base, 5), "variant 5 writes other bytes with another buffer count"
    # variant 6 on an NK tile with BN >= 64 runs gather_gemm_f16_v6 (launch_v5 returns before it reads VSR_V5_STAGES): the switch
    # must not reach it
    assert _same(got, base, 6) and got["v6"]["resident"] == base["v6"]["resident"]
    if tile == "128x64":
        # the switch was read: four buffers of 24 KB leave room for one workgroup per CU, two buffers for the three of __launch_bounds__
        want = {2: base["v5"]["resident"], 4: base["v5"]["resident"] // 3}.get(stages)
        assert want is None or got["v5"]["resident"] == want, (got["v5"]["resident"], base["v5"]["resident"])


@pytest.mark.parametrize("stages,tile", [(2, "128x64"), (4, "128x64"), (2, "256x64")])
def test_v6_stage_count(built_lib, gpu_device, stages, tile):
    """VSR_V6_STAGES: the stage count of gather_gemm_f16_v6 (default 3; 4 only where (BM + BN) x 512 bytes x 4 fit, so not on 256x64)."""
    got = _child({"VSR_V6_STAGES": str(stages)}, tile, [6])
    base = _defaults(tile, [6])
    # gather_gemm_v6.h: a stage holds a pair of chunks; step() consumes the pairs in k order whatever STAGES is (the loop is unrolled
    # by STAGES so that the stage index is a constant, nothing else) and compute_step 0..3 issue the same MFMAs per pair: the same bits
    assert _same(got, base, 6), "variant 6 writes other bytes with another stage count"
    if (stages, tile) == (4, "128x64"):
        # the switch was read: four stages of 24 KB leave room for one workgroup per CU, three stages for two
        assert got["v6"]["resident"] < base["v6"]["resident"], (got["v6"]["resident"], base["v6"]["resident"])


@pytest.mark.parametrize("tile", ["128x64", "256x64"])
def test_f16_kernel_5(built_lib, gpu_device, tile):
    """VSR_F16_KERNEL=5: variant 6 on gather_gemm_f32_v5's HI_ONLY path.  Another kernel (operands the other way round in the MFMA,
    another epilogue): held to the float64 reference in the child, no bytes compared."""
    got = _child({"VSR_F16_KERNEL": "5"}, tile, [6])
    assert got["v6"]["tiles"] >= 3 * got["v6"]["resident"]


def test_v7_tile_order_0(built_lib, gpu_device):
    """VSR_V7_ORDER=0 on the 256 x 256 kernel: first round static, then one atomic counter."""
    got = _child({"VSR_V7_ORDER": "0"}, "256x256", [5, 6])
    base = _defaults("256x256", [5, 6])
    # gather_gemm_v7.h: `order` decides which workgroup takes which tile id (xcd_slot() or blockIdx / the counter) and nothing inside
    # a tile: the same bits
    for v in (5, 6):
        assert _same(got, base, v), f"variant {v} writes other bytes in the other tile order"
