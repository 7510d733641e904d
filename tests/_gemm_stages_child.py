"""Child process of tests/test_gpu_gemm_stages.py: the library reads VSR_V5_STAGES, VSR_V6_STAGES, VSR_F16_KERNEL and VSR_V7_ORDER once
per process, so every setting gets a process of its own.  argv: TILE VARIANT [VARIANT ...] (NK layout).  Per variant one epilogue-matrix
launch (split-format output) and one hand-over launch of at least three tiles per resident workgroup, both held to the float64
reference by test_gpu_gemm_family._check; prints one line `STAGES {json}` with the SHA-256 of each launch's output bytes and the grid
cap of the kernel that ran."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import vsr_amd  # noqa: E402,F401
from vsr_amd import _lib  # noqa: E402

import _gemm_f64 as g64  # noqa: E402
import test_gpu_gemm_family as fam  # noqa: E402

# workgroups per CU that the LDS of the smallest stage count leaves room for: the hand-over launch is sized from this, not from the
# grid cap of this process's setting, so that every setting runs the same problems (and the digests can be compared)
PER_CU = {"128x64": 3, "128x128": 2, "256x64": 1, "256x256": 1}


def _digest(outs):
    h = hashlib.sha256()
    for o in outs:
        h.update(np.ascontiguousarray(o).tobytes())
    return h.hexdigest()


def main():
    tile, variants = sys.argv[1], [int(v) for v in sys.argv[2:]]
    cfg, bm, bn = fam.TILES[tile]
    assert torch.cuda.is_available() and _lib.lib.vsr_device_count() > 0, "no HIP device"
    device = torch.device("cuda", 0)
    need = 3 * PER_CU[tile] * torch.cuda.get_device_properties(0).multi_processor_count
    res = {}
    for variant in variants:
        assert g64.operand_model(variant).split_tensors
        resident = _lib.lib.vsr_gg_resident_blocks(cfg, 0, variant)
        assert resident > 0, _lib.last_error()
        what = f"stages v{variant} {tile}"
        L = fam._Launch(_lib, device, fam._epilogue_cases(bm, bn, 0, True, 1), variant)
        outs = L.run(cfg, 0)
        fam._check_all(L, outs, f"{what} epilogues", key=f"v{variant} {tile} NK epilogues")
        epi = _digest(outs)
        del L, outs
        L = fam._Launch(_lib, device, fam._handover(bm, bn, 0, 0, need), variant)
        assert L.tiles() >= 3 * resident, f"{what}: {L.tiles()} tiles for {resident} resident workgroups"
        outs = L.run(cfg, 0)
        fam._check_all(L, outs, f"{what} hand-over", key=f"v{variant} {tile} NK")
        res[f"v{variant}"] = {"epilogue": epi, "handover": _digest(outs), "resident": resident, "tiles": L.tiles()}
        del L, outs
    print("STAGES " + json.dumps(res))


if __name__ == "__main__":
    main()
