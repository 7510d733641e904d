"""VSR_SKIP_PAD_TAPS on the GPU: the frames an sttn-auto chunk / an sttn-det batch writes are the same bytes whether the stride-1 3x3
convs run as one problem or as interior + border-row problems without the taps that read the zero halo (Plan::addConv).  The library
reads the switch once per process, hence two children per case (tests/_pad_taps_gpu_child.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_pad_taps_gpu_child.py")


def _digests(case):
    res = {}
    for v in ("1", "0"):
        r = subprocess.run([sys.executable, CHILD, case], env=dict(os.environ, VSR_SKIP_PAD_TAPS=v), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (case, v, r.returncode, r.stdout[-1000:] + r.stderr[-3000:])       # stop here: no second child after a failed one
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][-1].split()
        assert line[2] == v, "the child's library did not read the switch"
        res[v] = (line[1], int(line[3]), int(line[4]))
    return res


@pytest.mark.parametrize("case", ["none", "bottom", "middle"])
def test_auto_chunk_same_frames_with_and_without_the_bands(built_lib, gpu_device, case):
    """720p, L = 6 (two windows).  none: no promise about the mask rows, top and bottom band in every block; bottom: the mask reaches
    the last row of its strip, the ranged last block and the decoder end in the bottom band; middle: they are interior-only."""
    res = _digests(case)
    lo, hi = res["1"][1:]
    if case == "none":
        assert (lo, hi) == (0, 0)
    elif case == "bottom":
        assert lo > 8 and hi == 120
    else:
        assert 40 < lo < hi < 80
    assert res["1"][0] == res["0"][0]


def test_det_batch_same_frames_with_and_without_the_bands(built_lib, gpu_device):
    """sttn-det, L = 5 at 432 x 240 (60 x 108 feature maps)"""
    res = _digests("det")
    assert res["1"][0] == res["0"][0]
