"""VSR_SKIP_PAD_TAPS (Plan::addConv, csrc/sttn_plan.cpp): a stride-1 3x3 conv contracts the output rows next to the top / bottom border in
problems of their own, without the tap row that reads nothing but the zero halo.  Checked here without a GPU: the structure of the
plan's tables, the CPU replay with the switch on and off (bit-equal composites, both at the oracle), and the two FLOP counts."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

def _structure_child(what):
    """the structure checks of tests/_pad_taps_child.py in a process with the switch on (the library reads it once; this process may have it off)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_pad_taps_child.py"), "--structure", what], env=dict(os.environ, VSR_SKIP_PAD_TAPS="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("variant", ["auto", "det"])
def test_band_items_contract_everything_but_the_halo_rows(built_lib, variant):
    """L = 7 (two windows), full rows: every stride-1 3x3 conv of the transformer blocks and of the decoder is three problems --
    interior with nine taps, top and bottom band with six -- and together they contract exactly the (output pixel, tap, channel block)
    triples whose source row is inside the map, in the full problem's chunk order, A and B naming the same chunks (check_structure)."""
    res = _structure_child(variant)
    assert res["seen"] == {tag: [6, 9] for tag in ("attn.out", "ffn.1", "ffn.2", "dec.1", "dec.2", "dec.3")}, res
    assert all(taps == [9, 6, 6] for taps in res["taps"]), res["taps"]
    assert res["executed"] < res["flops"]


def test_ranged_last_block_emits_only_the_bands_it_touches(built_lib):
    """a decoder row range in the middle of the strip: the last block's convs and the decoder's are interior-only; one at the bottom or at the
    top: interior + that band, not the other.  The structure check holds for whatever has more than one problem."""
    res = _structure_child("ranged")
    assert res == {"50-70": [[9]], "84-120": [[9, 6]], "0-20": [[9, 6]]}, res


@pytest.fixture(scope="module")
def children(built_lib):
    """tests/_pad_taps_child.py with the switch on and off, a fresh process each (the library reads it once)"""
    res = {}
    for v in ("1", "0"):      # (one after the other: side by side the two oversubscribe a small host and take longer)
        r = subprocess.run([sys.executable, os.path.join(HERE, "_pad_taps_child.py")], env=dict(os.environ, VSR_SKIP_PAD_TAPS=v),
                           capture_output=True, text=True, timeout=2400)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        res[v] = json.loads(r.stdout.strip().splitlines()[-1])
        assert res[v]["switch"] == int(v)
    return res


def test_replay_is_bit_equal_with_and_without_the_bands(children):
    """three windows (L = 12), no row promise and mask rows at the bottom border: the replayed composites are the same bits with the
    switch on and off (each child has already compared them with the oracle as tests/_replay_check.py does)"""
    on, off = children["1"], children["0"]
    for name in ("full", "bottom"):
        print(name, on[name]["max_abs"], on[name]["flips"], off[name]["max_abs"], off[name]["flips"])
        assert on[name]["counts"] == off[name]["counts"]
        assert all(n == 1 for _, n in off[name]["items"]) and any(n > 1 for _, n in on[name]["items"]), (on[name]["items"], off[name]["items"])
        assert on[name]["sha"] == off[name]["sha"], name


def test_flops_algorithmic_and_executed(children):
    """vsr_plan_flops keeps the convolution count, padding taps included; vsr_plan_flops_executed is that minus the products the
    band problems leave out: 2 * (band pixels) * cout * 3 * cin per conv, from the geometry of the L = 12 plan."""
    on, off = children["1"], children["0"]
    for name in ("full", "bottom"):
        assert on[name]["flops"] == off[name]["flops"]
        assert off[name]["executed"] == off[name]["flops"]
        assert on[name]["executed"] < on[name]["flops"]
    # stride 5, references every 10 (Plan::Plan): windows of T = 7 / 11 / 8 frames with 6 / 11 / 7 neighbours; the last of the eight blocks and
    # the decoder run on the neighbours only (VSR_TRIM_LAST_BLOCK, the default)
    L, fh, fw, C = 12, 30, 160, 256
    skipped = 0.0
    for T, nn in ((7, 6), (11, 11), (8, 7)):
        for frames in [T] * 7 + [nn]:
            skipped += 2.0 * (frames * 2 * fw) * C * 3 * C         # attn.out: dilation 1, rows 0 and 29
            skipped += 2.0 * (frames * 4 * fw) * C * 3 * C         # ffn.1: dilation 2, rows 0, 1, 28, 29
            skipped += 2.0 * (frames * 2 * fw) * C * 3 * C         # ffn.2
        skipped += 2.0 * (nn * 2 * 2 * fw) * 128 * 3 * 256          # dec.1 on the 60 x 320 map
        skipped += 2.0 * (nn * 2 * 2 * fw) * 64 * 3 * 128           # dec.2
        skipped += 2.0 * (nn * 2 * 4 * fw) * 64 * 3 * 64            # dec.3 on the 120 x 640 map
    skipped += 2.0 * (L * 2 * 2 * fw) * 64 * 3 * 64                 # enc.2 (60 x 320; enc.3 has stride 2)
    skipped += 2.0 * (L * 2 * fw) * 256 * 3 * 128                   # enc.4
    got = on["full"]["flops"] - on["full"]["executed"]
    assert abs(got - skipped) <= 1e-9 * skipped, (got, skipped)
    assert 0.01 < skipped / on["full"]["flops"] < 0.03
