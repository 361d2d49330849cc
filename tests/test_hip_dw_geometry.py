"""The three depthwise kernels on wide and tall planes, bit for bit.  `-m gpu`.

The vector kernels (dw_vec_kernel, dw_wgrad_vec_kernel in csrc/dwconv.hip) split a plane by vec_geom(H, W, PXL): G = W / PXL
lanes per row, gpw = 64 / G row groups per wave, R = clamp(ceil(H / gpw), 4, 32) rows per group, nslabs =
ceil(H / (gpw * R)) waves per plane.  The shapes of the rest of the suite never leave nslabs = 1, G <= 16, gpw >= 4; the
shapes here reach several slabs per plane (halo rows that belong to the wave above and below, per-slab weight-gradient
partials and their reduce), one row group per wave, rows of 33 lanes with 31 idle ones, ragged and empty last groups, and
both upper edges of the vector path (W = 256 at PXL 4, W = 512 at PXL 8) with the strip kernels just past them.

Data on which the kernels have to be exact, so no tolerance is involved: x and dy are integers in [-2, 2], the taps are
from {-1, -0.5, 0, 0.5, 1}.  Every product is a multiple of 0.5 of magnitude <= 2, every partial sum of <= 49 of them is
exact in fp32 in any order, with or without FMA, and through the matrix cores (the taps are exact in bf16 / f16); every
output is a multiple of 0.5 with |y| <= 98, exact in bf16 (196 < 2^8), f16 and fp32; the weight gradient is an integer of
magnitude <= 4 * N * H * W, far below 2^24.  The test asserts these on the oracle's output before it looks at the GPU's.

The geometry guard restates vec_geom and the two matrix-core rules and asserts, per case, the geometry listed beside the
shape and the kernel family the launch table names.  It is there so that a later tuning of the dispatch cannot slide a
shape into another kernel unnoticed: when it fails, re-pick the row it names."""
import numpy as np
import pytest
import torch

from conftest import amd
from detfill import det_ints
from test_hip_kernels import DW_SHAPES, DTYPES, G, H, rounded

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------- the dispatch of csrc/dwconv.hip, restated
def vec_geom(Hh, W, pxl):
    """(G, gpw, R, nslabs) of the vector kernels at `pxl` pixels per lane, None where the vector path does not apply"""
    if W % pxl or W // pxl > 64:
        return None
    g = W // pxl
    gpw = 64 // g
    r = min(32, max(4, -(-Hh // gpw)))
    return g, gpw, r, -(-Hh // (gpw * r))


def mfma_geom_ok(Hh, W, k, dtype):
    return dtype != torch.float32 and k >= 5 and W in (32, 64) and Hh in (32, 64)


def dw_wgrad_mfma_ok(Hh, W, k, dtype):
    return dtype != torch.float32 and k in (3, 5, 7) and W in (32, 64) and Hh % 16 == 0 and 16 <= Hh <= 64


def conv_pxl(k, dtype):
    return 8 if (dtype != torch.float32 and k <= 3) else 4


def conv_family(Hh, W, k, dtype):
    """forward and input gradient (operands from the allocator: 16-byte aligned)"""
    if mfma_geom_ok(Hh, W, k, dtype):
        return "dw_mfma_kernel"
    return "dw_vec_kernel" if vec_geom(Hh, W, conv_pxl(k, dtype)) else "dw_strip_kernel"


def wgrad_family(Hh, W, k, dtype):
    if dw_wgrad_mfma_ok(Hh, W, k, dtype):
        return "dw_wgrad_mfma_kernel"
    return "dw_wgrad_vec_kernel" if vec_geom(Hh, W, 4) else "dw_wgrad_kernel"


CONV_FAMILIES = ("dw_vec_kernel", "dw_strip_kernel", "dw_mfma_kernel")
WGRAD_FAMILIES = ("dw_wgrad_vec_kernel", "dw_wgrad_kernel", "dw_wgrad_mfma_kernel")

# shape -> (G, gpw, R, nslabs) at PXL 4 (fp32, 16-bit K >= 5, every weight gradient) and at PXL 8 (16-bit K <= 3);
# None = strip kernel
GEOMETRY = {
    (1, 2, 70, 256): ((64, 1, 32, 3), (32, 2, 32, 2)),    # full-wave rows, three slabs, 6-row tail; PXL 8: one empty group
    (2, 3, 130, 128): ((32, 2, 32, 3), (16, 4, 32, 2)),   # slab tail of 2 rows, N * C planes x slabs
    (1, 2, 37, 132): ((33, 1, 32, 2), None),              # 31 idle lanes in the shuffles; 16-bit K <= 3: strip fwd, vector wgrad
    (1, 3, 9, 84): ((21, 3, 4, 1), None),                 # gpw = 3, R at its floor
    (1, 2, 20, 72): ((18, 3, 7, 1), (9, 7, 4, 1)),        # ragged last group (10 idle lanes); PXL 8: two empty groups
    (1, 2, 33, 512): (None, (64, 1, 32, 2)),              # upper edge of the PXL 8 path
    (1, 1, 40, 264): (None, (33, 1, 32, 2)),              # just past the PXL 4 edge
    (2, 2, 200, 64): ((16, 4, 32, 2), (8, 8, 25, 1)),     # training width, H beyond the matrix-core rules
    (1, 2, 72, 128): ((32, 2, 32, 2), (16, 4, 18, 1)),    # the plane of the fp32 block test (test_hip_network.py)
}
# the shapes test_dwconv_vs_oracle had before, and the 32 x 32 matrix-core plane of test_hip_placement_abi.py
EXISTING = [s for s in DW_SHAPES if s not in GEOMETRY] + [(2, 6, 32, 32)]


def test_tables_are_what_they_say():
    assert len(GEOMETRY) == 9 and all(s in DW_SHAPES for s in GEOMETRY)
    reach = [g for row in GEOMETRY.values() for g in row if g]
    assert max(g[3] for g in reach) == 3 and max(g[0] for g in reach) == 64 and min(g[1] for g in reach) == 1


def _families(table, families):
    """the families with a launch in `table` (a family name directly followed by its template arguments)"""
    return sorted(f for f in families if any((f + "<") in name for name in table))


_REF = {}


def _reference(ora, shape, k):
    """exact-arithmetic operands and the oracle's results, computed once per (shape, k) and left unchanged"""
    if (shape, k) not in _REF:
        N, C, Hh, W = shape
        x = det_ints(shape, "dwg/x%s" % (shape,), -2, 3)                  # integers in [-2, 2]
        dy = det_ints(shape, "dwg/dy%s" % (shape,), -2, 3)
        f = det_ints((C, 1, k, k), "dwg/f%d_%d" % (C, k), -2, 3) / 2      # {-1, -0.5, 0, 0.5, 1}
        for a in (x, dy, 2 * f):
            assert np.all(np.isin(a, [-2, -1, 0, 1, 2]))
        y = ora.dwconv_fwd(x, f)
        dx, df = ora.dwconv_bwd(dy, x, f)
        for t in (y, dx):   # multiples of 0.5, |.| <= 98: representable in every activation type
            assert np.array_equal(2 * t, np.round(2 * t)) and float(np.abs(t).max()) <= 98
            for dt in DTYPES:
                assert np.array_equal(rounded(t, dt), t)
        assert np.array_equal(df, np.round(df)) and float(np.abs(df).max()) < 2 ** 24
        assert x.size < 64 or (np.any(y) and np.any(dx) and np.any(df))
        for a in (x, dy, f, y, dx, df):
            a.setflags(write=False)
        _REF[(shape, k)] = (x, dy, f, y, dx, df)
    return _REF[(shape, k)]


def _check_exact(ora, shape, k, dtype):
    """forward, input gradient and weight gradient through ops.dwconv with autograd, as test_dwconv_vs_oracle calls them;
    returns the launch tables of (forward, input gradient + weight gradient)"""
    ops, C = amd("ops"), amd("_C")
    x, dy, f, y_ref, dx_ref, df_ref = _reference(ora, shape, k)
    xt = G(x, dtype).requires_grad_(True)
    ft = G(f).requires_grad_(True)
    dyt = G(dy, dtype)
    C.reset_launch_counts()
    y = ops.dwconv(xt, ft)
    fwd_table = C.launch_table()
    C.reset_launch_counts()
    y.backward(dyt)
    ops.flush_deferred()   # deferred weight gradients -> .grad (ops.py)
    torch.cuda.synchronize()
    bwd_table = C.launch_table()
    assert y.dtype == dtype and xt.grad.dtype == dtype and ft.grad.dtype == torch.float32
    for what, got, ref in (("y", y, y_ref), ("dx", xt.grad, dx_ref), ("df", ft.grad, df_ref)):
        got = H(got)
        if not np.array_equal(got, ref):
            bad = np.argwhere(got != ref)
            i = tuple(bad[0])
            raise AssertionError("%s differs from the oracle at %d of %d elements, first at %s: got %r expected %r; rows %s"
                                 % (what, len(bad), ref.size, i, got[i], ref[i], sorted(set(bad[:, 2].tolist()))[:16]))
    return fwd_table, bwd_table


def _check_families(shape, k, dtype, fwd_table, bwd_table):
    _, _, Hh, W = shape
    want = [conv_family(Hh, W, k, dtype)]
    assert _families(fwd_table, CONV_FAMILIES) == want, (shape, k, dtype, "forward", fwd_table)
    assert _families(bwd_table, CONV_FAMILIES) == want, (shape, k, dtype, "input gradient", bwd_table)
    assert _families(bwd_table, WGRAD_FAMILIES) == [wgrad_family(Hh, W, k, dtype)], (shape, k, dtype, bwd_table)


@pytest.mark.parametrize("shape", list(GEOMETRY), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", [1, 3, 5, 7])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "f16"])
def test_dwconv_exact_at_vector_geometries(ora, shape, k, dtype):
    _, _, Hh, W = shape
    row4, row8 = GEOMETRY[shape]
    # the geometry guard: the restated rules give the row, and no matrix-core rule takes the shape away
    assert vec_geom(Hh, W, 4) == row4 and vec_geom(Hh, W, 8) == row8, (shape, vec_geom(Hh, W, 4), vec_geom(Hh, W, 8))
    assert not mfma_geom_ok(Hh, W, k, dtype) and not dw_wgrad_mfma_ok(Hh, W, k, dtype)
    conv_row = row8 if conv_pxl(k, dtype) == 8 else row4
    print("geometry %s k%d %s: conv (G, gpw, R, nslabs) = %s, wgrad = %s" % (shape, k, dtype, conv_row, row4))
    fwd_table, bwd_table = _check_exact(ora, shape, k, dtype)
    # ... and it is reached: the family that owns the row served the call
    assert _families(fwd_table, CONV_FAMILIES) == ["dw_vec_kernel" if conv_row else "dw_strip_kernel"], fwd_table
    assert _families(bwd_table, CONV_FAMILIES) == ["dw_vec_kernel" if conv_row else "dw_strip_kernel"], bwd_table
    assert _families(bwd_table, WGRAD_FAMILIES) == ["dw_wgrad_vec_kernel" if row4 else "dw_wgrad_kernel"], bwd_table


@pytest.mark.parametrize("shape", EXISTING, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", [1, 3, 5, 7])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "f16"])
def test_dwconv_exact_at_existing_shapes(ora, shape, k, dtype):
    """the strip kernels with several strips and row chunks, the matrix-core forward, input gradient and weight gradient at
    64 x 64 and 32 x 32, and the degenerate shapes, on the same exact data"""
    fwd_table, bwd_table = _check_exact(ora, shape, k, dtype)
    _check_families(shape, k, dtype, fwd_table, bwd_table)
