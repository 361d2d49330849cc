"""The shape table of tests/conv_geometry.py is what it says, without a GPU: (a) the restated host rules of
csrc/conv2d.hip and csrc/conv2d_f32.hip give exactly the geometry written beside every row, (b) the rows together reach
every configuration, split and path the kernels have, (c) the data is exact -- every y and dx a multiple of 0.5, every
dw an integer below 2^24, nothing identically zero, at most 1 % of the bf16 expected values rounded at all, the
statistics rows small enough for exact fp32 sums -- asserted on the references' own output, and (d) the C oracle and the
float64 torch reference agree bit for bit on the smallest row.

tests/test_hip_conv_geometry.py runs the rows on the device and asserts that the kernels it launched are the ones named
here; when a retuning of cv_plan, cv_wg_plan or cf_nsplit moves a row, restate the rule in conv_geometry.py and re-pick
the rows (a) and (b) then name."""
import numpy as np
import pytest

import conv_geometry as cg
from conv_geometry import BF16, F16, F32, ROWS


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_row_reaches_the_geometry_beside_it(row):
    """(a)"""
    fwd, dgrad, wg, f32 = cg.geometry(row.shape)
    assert f32 == row.f32, "%s: fp32 (quad staging, groups, nsplit, tiles per block) is %s, the row says %s" % (row.shape, f32, row.f32)
    if BF16 in row.types:
        assert fwd == row.fwd, "%s: forward (cfg, nslab, nkc, ONEK) is %s, the row says %s" % (row.shape, fwd, row.fwd)
        assert dgrad == row.dgrad, "%s: input gradient (cfg, nslab, nkc, ONEK) is %s, the row says %s" % (row.shape, dgrad, row.dgrad)
        assert wg == row.wg, "%s: weight gradient (cfg, ncislab, nz, ntiles, ksplit K3, K5) is %s, the row says %s" % (row.shape, wg, row.wg)
        assert row.shape[4] % 8 == 0, "the 16-bit entry points take W % 8 == 0"
    else:
        assert (row.fwd, row.dgrad, row.wg) == (None, None, None), "a row without 16-bit runs claims no 16-bit geometry"
    N, Cin, Cout, H, W = row.shape
    assert min(Cin, Cout) > 4, "Ct <= 4 belongs to the thin kernels (csrc/conv_thin.hip)"
    assert N * H * W < 2 ** 24 and max(Cin, Cout) * 25 < 2 ** 22      # the exactness argument of conv_geometry.py


def test_named_details_of_the_rows():
    """what the `why` texts claim beyond the tuples: tile counts, ragged ranges, idle blocks"""
    plan = lambda s, dgrad=0: cg.cv_plan(*s, 5, dgrad)
    p = plan((2, 40, 160, 5, 72))
    assert (p["th"], p["tiles_y"], p["tiles_x"]) == (2, 3, 2) and 40 % 32 == 8
    p = plan((1, 16, 264, 3, 16))
    assert p["rows"] == 256 and p["M"] - 256 == 8 and plan((1, 16, 264, 3, 16), 1)["th"] == 8 > 3
    p = plan((2, 96, 72, 9, 136))
    assert (p["th"], p["tiles_y"], p["tiles_x"]) == (4, 3, 3)
    p = plan((3, 8, 24, 10, 8))
    assert (p["th"], p["tiles_y"]) == (8, 2)
    p = plan((256, 48, 40, 9, 8))
    assert 256 * p["tiles_y"] * p["tiles_x"] == 512 and p["th"] == 8      # exactly the threshold of cfg 2
    p = plan((128, 8, 64, 12, 72))
    assert 128 * p["tiles_y"] * p["tiles_x"] == 512 and p["tiles_x"] == 2
    assert cg.cv_wg_ranges(42, 5) == [8, 8, 9, 8, 9] and 42 // 3 == 14
    assert cg.cv_wg_ranges(100, 8) == [12, 13, 12, 13, 12, 13, 12, 13] and 100 // 8 == 12
    assert cg.cv_wg_ranges(21, 2) == [10, 11]
    assert cg.cv_wg_ranges(128, 16) == [8] * 16
    p = cg.cf_plan(1, 160, 160, 22, 168, 5)
    assert (p["groups"], p["nsplit"], p["ntiles"], p["tiles_per_block"]) == (25, 10, 36, (3, 4))


def test_rows_cover_every_configuration():
    """(b)"""
    r16 = [r for r in ROWS if BF16 in r.types]
    conv = [g for r in r16 for g in (r.fwd, r.dgrad)]
    assert {(g[0], g[3]) for g in (r.fwd for r in r16)} == {(c, o) for c in range(5) for o in (False, True)}, \
        "the forward reaches every cv_plan cfg with ONEK and without"
    assert {g[0] for g in conv} == {0, 1, 2, 3, 4} and {g[3] for g in conv} == {False, True}
    assert any(g[0] == 2 for g in (r.dgrad for r in r16)), "cfg 2 as an input gradient (the up-sampler conv of the timed step)"
    assert any(g[1] == 2 for g in conv), "nslab 2"
    assert any(g[2] >= 9 for g in conv), "a long channel-chunk loop"
    wg = [r.wg for r in r16]
    assert {g[0] for g in wg} == {0, 1, 2, 3, 4, 5}
    ksplits = {k for g in wg for k in g[4:6]}
    assert ksplits & {1, 2} and ksplits & {3, 5, 6, 7} and 8 in ksplits and 16 in ksplits, ksplits
    assert any(len(set(cg.cv_wg_ranges(g[3], g[5]))) > 1 and 3 <= g[5] <= 7 for g in wg), "an uneven split in 3 .. 7"
    assert any(cg.cv_wg_plan(*r.shape, 5)["ksplit"] == 8 and min(512 // (5 * r.wg[2]), r.wg[3] // 8) > 8 for r in r16), \
        "ksplit 8 reached by the rounding"
    assert any(g[1] == 2 for g in wg) and any(g[2] >= 2 and g[1] == 1 for g in wg), "ncislab 2; nz 2 from the output channels"
    f32 = [r for r in ROWS if F32 in r.types]
    assert len(f32) == len(ROWS), "every row runs in fp32"
    assert any(r.f32[0] and r.f32[3][1] >= 3 and "wgrad" in r.passes and 5 in r.ks for r in f32), ">= 3 tiles per block on the loader-wave path"
    assert any(not r.f32[0] for r in f32) and any(r.f32[3] == (3, 4) for r in f32)
    for s in cg.STAT_ROWS:
        assert cg.BY_SHAPE[s].shape[2] % 4 == 0
    assert [cg.BY_SHAPE[s].fwd[0] for s in cg.STAT_ROWS] == [0, 1, 2], "statistics / inference epilogues at WP 1, 2 and 4"


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_data_is_exact(ora, row):
    """(c): reference() asserts the conditions (conv_geometry.check_exactness); here they are spelled out once more on
    what it returns"""
    for K in row.ks:
        ref = cg.reference(ora, row.shape, K)
        y, dx, dw = ref["y"], ref["dx"], ref["dw"]
        for t in (y, dx):
            assert np.array_equal(2 * t, np.round(2 * t)) and np.any(t)
            assert cg.bf16_inexact_fraction(t) <= 0.01
            assert np.array_equal(cg.rounded(t, F16), t)
        assert np.array_equal(dw, np.round(dw)) and float(np.abs(dw).max()) < 2 ** 24 and np.any(dw)
        if row.shape in cg.STAT_ROWS:
            assert float(np.abs(y).max()) <= cg.STAT_MAX
        assert not y.flags.writeable and cg.reference(ora, row.shape, K) is ref      # computed once, left unchanged


def test_c_oracle_and_torch_reference_agree_bit_for_bit(ora):
    """(d): on the smallest row, and on the largest the C oracle is still used for"""
    shapes = [cg.SMALLEST, max((r.shape for r in ROWS if cg.macs(r.shape, 5) <= cg.ORACLE_MACS), key=lambda s: cg.macs(s, 5))]
    assert cg.macs(cg.SMALLEST, 5) == min(cg.macs(r.shape, 5) for r in ROWS)
    for shape in shapes:
        for K in (3, 5):
            x, w, dy = cg.operands(shape, K)
            for name, a, b in zip(("y", "dx", "dw"), cg.oracle_reference(ora, x, w, dy), cg.torch_reference(x, w, dy, K)):
                assert a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes(), (shape, K, name)
