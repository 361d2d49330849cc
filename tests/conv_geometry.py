"""Launch geometries of the dense static convolutions (csrc/conv2d.hip, csrc/conv2d_f32.hip): the host rules restated,
the shape table with what every row reaches, data on which the kernels have to be exact, and the references.  A plain
helper for tests/test_conv_geometry.py (CPU: the table is what it says, the data is exact) and
tests/test_hip_conv_geometry.py (`-m gpu`: every row bit for bit, and the device did launch what the row names).

Data.  Activations and incoming gradients are integers in {-1, 0, 1}, weights are from {-1, -0.5, 0, 0.5, 1} (exact in
bf16 and f16).  Every product is a multiple of 0.5 of magnitude <= 1; a forward or input-gradient sum has at most
Kdim * K^2 <= 264 * 25 terms and a weight-gradient sum N * H * W <= 2^18 integer terms, so every partial sum is a
multiple of 0.5 far below 2^24 halves: fp32 accumulation is exact in any order, with or without FMA, on either matrix
instruction, across any split of the reduction.  So
    fp32 y, dx      = the exact result,
    16-bit y, dx    = the exact result rounded once to the type (torch's cast: round to nearest even),
    dw (always fp32) = the exact integer,
and the tests compare with np.array_equal.  reference() asserts all of this on its own output before anyone looks at a
GPU result.

References.  ora.conv2d_fwd / ora.conv2d_bwd (the C oracle, double accumulation) up to ORACLE_MACS multiply-adds per
pass; above that torch.nn.functional.conv2d and torch.nn.grad in float64 on the CPU stand in (the C oracle's plain loops
would take minutes on the largest rows).  test_conv_geometry.py shows the two bit-equal on the smallest row; on this data
both are exact, so they cannot differ anywhere else either."""
import os

import numpy as np
import torch

from detfill import det_ints

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------ csrc/conv2d.hip, host rules restated
CV_CFGS = [(2, 4, 1), (2, 2, 2), (2, 1, 4), (1, 1, 4), (1, 2, 2)]          # CvPlan::cfg -> (RB, WM, WP)
CV_WG_CFGS = [(2, 2, 2, 1), (2, 1, 2, 2), (1, 1, 2, 2), (2, 2, 1, 2), (2, 1, 1, 4), (1, 1, 1, 4)]   # -> (RBW, WCO, WCI, WK)


def cv_plan(N, Cin, Cout, H, W, K, dgrad):
    """cv_plan + launch_conv_run: forward has (M, Kdim) = (Cout, Cin), the input gradient swaps them"""
    M, Kdim = (Cin, Cout) if dgrad else (Cout, Cin)
    cfg = 0 if M > 128 else (1 if M > 64 else (2 if M > 32 else 3))
    if cfg == 2 and N * cdiv(H, 8) * cdiv(W, 64) < 512:
        cfg = 4
    rows = {0: 256, 1: 128, 3: 32}.get(cfg, 64)
    th = 2 if cfg == 0 else (4 if cfg in (1, 4) else 8)
    nslab = cdiv(M, rows)
    nrb = nslab * (rows // 32)
    nkc = cdiv(Kdim, 32)
    return dict(cfg=cfg, rows=rows, th=th, nslab=nslab, nrb=nrb, nkc=nkc, onek=Kdim <= 16, M=M, Kdim=Kdim,
                tiles_y=cdiv(H, th), tiles_x=cdiv(W, 64), img_bytes=nkc * K * 2 * K * nrb * 1024,
                units=N * cdiv(W, 64) * cdiv(H, th) * (th // 2))


def cv_geom(N, Cin, Cout, H, W, K, dgrad):
    """what the table writes beside a row: (cfg, nslab, nkc, ONEK)"""
    p = cv_plan(N, Cin, Cout, H, W, K, dgrad)
    return p["cfg"], p["nslab"], p["nkc"], p["onek"]


def cv_wg_plan(N, Cin, Cout, H, W, K):
    wide = Cin > 32
    rcls = 0 if Cout > 64 else (1 if Cout > 32 else 2)
    cfg = (0 if wide else 3) + rcls
    rows = (128, 64, 32)[rcls]
    rbw = 1 if rcls == 2 else 2
    cib = 64 if wide else 32
    ntiles = N * cdiv(W, 64) * cdiv(H, 2)
    ncislab = cdiv(Cin, cib)
    nz = cdiv(Cout, rows) * ncislab
    ks = min(512 // (K * nz), ntiles // 8)
    if ks > 8:
        ks -= ks % 8
    ksplit = max(ks, 1)
    nwq = ((4 if rcls == 0 else 2) if wide else (2 if rcls == 0 else 1))
    return dict(cfg=cfg, rows=rows, rbw=rbw, cib=cib, ntiles=ntiles, ncislab=ncislab, nz=nz, ksplit=ksplit, nwq=nwq,
                part_bytes=ksplit * K * nz * nwq * rbw * K * 16 * 64 * 4)


def cv_wg_geom(N, Cin, Cout, H, W):
    """(cfg, ncislab, nz, ntiles, ksplit at K = 3, ksplit at K = 5)"""
    p3, p5 = cv_wg_plan(N, Cin, Cout, H, W, 3), cv_wg_plan(N, Cin, Cout, H, W, 5)
    return p5["cfg"], p5["ncislab"], p5["nz"], p5["ntiles"], p3["ksplit"], p5["ksplit"]


def cv_wg_ranges(ntiles, ksplit):
    """tiles per split: t0 = split * ntiles / ksplit"""
    return [(s + 1) * ntiles // ksplit - s * ntiles // ksplit for s in range(ksplit)]


# -------------------------------------------------------------------------- csrc/conv2d_f32.hip, host rules restated
def cf_blocks():
    """cf_nsplit's block budget: 256 unless the library's switch says otherwise (tests/test_hip_switches.py sets it in
    child processes only; the tables below are written for the default)"""
    v = os.environ.get("OFASR_CONV_F32_WG_BLOCKS", "")
    return int(v) if v.isdigit() and int(v) > 0 else 256


def cf_plan(N, Cin, Cout, H, W, K, blocks=256):
    ntiles = N * cdiv(H, 4) * cdiv(W, 32)
    groups = cdiv(Cout, 32) * cdiv(Cin, 32)
    nsplit = max(1, min(blocks // groups, ntiles))
    per = [(s + 1) * ntiles // nsplit - s * ntiles // nsplit for s in range(nsplit)]
    return dict(ntiles=ntiles, groups=groups, nsplit=nsplit, tiles_per_block=(min(per), max(per)),
                part_bytes=nsplit * 2 * Cout * Cin * K * K * 4)


def cf_fast(K, W):
    """the quad staging of conv_f32_kernel and the loader waves of conv_f32_wgrad_kernel (operands 16-byte aligned, and
    max(Cin, Cout) * H * W < 2^31, which every row here meets)"""
    return K == 5 and W % 4 == 0


def cf_geom(N, Cin, Cout, H, W):
    """(quad staging at K = 5, groups, nsplit, (fewest, most) tiles of a block)"""
    p = cf_plan(N, Cin, Cout, H, W, 5)
    return cf_fast(5, W), p["groups"], p["nsplit"], p["tiles_per_block"]


# ------------------------------------------------------------------------------------------------------- the table
class Row(object):
    def __init__(self, shape, fwd, dgrad, wg, f32, ks=(3, 5), types=(BF16, F16, F32), passes=("fwd", "dgrad", "wgrad"), why=""):
        self.shape, self.fwd, self.dgrad, self.wg, self.f32 = shape, fwd, dgrad, wg, f32
        self.ks, self.types, self.passes, self.why = ks, types, passes, why

    @property
    def id(self):
        return "x".join(map(str, self.shape))


T, F_ = True, False
# shape = (N, Cin, Cout, H, W); every row runs K = 3 and K = 5, forward, input gradient and weight gradient, in bf16, f16
# and fp32 unless it says otherwise.
#   fwd, dgrad  conv_igemm_kernel: (cfg, nslab, nkc, ONEK); cfg -> (RB, WM, WP) = CV_CFGS[cfg], tile = 2 WP rows x 64 columns
#   wg          conv_wgrad_kernel: (cfg, ncislab, nz, ntiles, ksplit at K = 3, ksplit at K = 5); tile = 2 rows x 64 columns
#   f32         conv_f32_kernel / conv_f32_wgrad_kernel: (quad staging and loader waves at K = 5, (co, ci) groups, nsplit,
#               (fewest, most) 4 x 32 pixel tiles of a block)
ROWS = [
    # ---- forward and input gradient
    Row((2, 40, 160, 5, 72), (0, 1, 2, F_), (4, 1, 5, F_), (0, 1, 2, 12, 1, 1), (T, 10, 12, (1, 1)),
        why="fwd cfg 0: 160 of a 256-row slab, nkc 2 ragged (32 + 8), row tiles 2 + 2 + 1, columns 64 + 8; "
            "dgrad cfg 4 (M = 40, 4 tiles), nkc 5"),
    Row((1, 16, 264, 3, 16), (0, 2, 1, T), (3, 1, 9, F_), (3, 1, 3, 2, 1, 1), (T, 9, 1, (1, 1)),
        why="fwd cfg 0 with nslab 2 (a second slab of 8 rows), ONEK; dgrad cfg 3 with H < its 8-row tile, nkc 9 ragged "
            "(8 x 32 + 8); wg cfg 3 with nz 3"),
    Row((2, 96, 72, 9, 136), (1, 1, 3, F_), (1, 1, 3, F_), (0, 2, 2, 30, 3, 3), (T, 9, 28, (1, 2)),
        why="fwd cfg 1: column tiles 64 + 64 + 8, row tiles 4 + 4 + 1, nkc 3; dgrad cfg 1, nkc 3 ragged (64 + 8); "
            "wg cfg 0 with ncislab 2 (64 + 32) and 72 of 128 rows"),
    Row((3, 8, 24, 10, 8), (3, 1, 1, T), (3, 1, 1, F_), (5, 1, 1, 15, 1, 1), (T, 1, 9, (1, 1)),
        why="fwd cfg 3, ONEK, row tiles 8 + 2, 8 of 64 columns; dgrad cfg 3, not ONEK (Kdim 24)"),
    Row((256, 48, 40, 9, 8), (2, 1, 2, F_), (2, 1, 2, F_), (1, 1, 1, 1280, 160, 96), (T, 4, 64, (12, 12)),
        why="fwd cfg 2: 256 * 2 * 1 = 512 tiles, the threshold; nkc 2 ragged (32 + 16), row tiles 8 + 1; dgrad cfg 2 "
            "(M = 48); wg ksplit 160 / 96: twenty / twelve rounds of 8; fp32 wg 12 tiles per block"),
    Row((128, 8, 64, 12, 72), (2, 1, 1, T), (3, 1, 2, F_), (4, 1, 1, 1536, 168, 96), (T, 2, 128, (9, 9)),
        why="fwd cfg 2 with ONEK, two column tiles, row tiles 8 + 4, a full 64-row slab; fp32 wg 9 tiles per block"),
    Row((2, 16, 72, 6, 16), (1, 1, 1, T), (3, 1, 3, F_), (3, 1, 1, 6, 1, 1), (T, 3, 4, (1, 1)),
        why="fwd cfg 1 with ONEK"),
    Row((2, 8, 40, 5, 24), (4, 1, 1, T), (3, 1, 2, F_), (4, 1, 1, 6, 1, 1), (T, 2, 4, (1, 1)),
        why="fwd cfg 4 with ONEK"),
    Row((1, 40, 264, 4, 8), (0, 2, 2, F_), (4, 1, 9, F_), (0, 1, 3, 2, 1, 1), (T, 18, 1, (1, 1)),
        why="fwd cfg 0 with nslab 2 and a chunk loop (nkc 2 ragged): the second slab's weight fragments beyond chunk 0; "
            "dgrad cfg 4 with nkc 9; wg cfg 0 with nz 3 (128 + 128 + 8 rows)"),
    Row((1, 264, 16, 3, 16), (3, 1, 9, F_), (0, 2, 1, T), (2, 5, 5, 2, 1, 1), (T, 9, 1, (1, 1)),
        why="dgrad cfg 0 with nslab 2 (the mirrored, transposed weight image in two slabs), ONEK; wg cfg 2 with ncislab 5 "
            "(4 x 64 + 8)"),
    # ---- 16-bit weight gradient
    Row((3, 64, 160, 14, 72), (0, 1, 2, F_), (4, 1, 5, F_), (0, 1, 2, 42, 5, 5), (T, 10, 25, (1, 2)),
        why="wg cfg 0, nz 2 (128 + 32 rows), 42 tiles in 5 uneven ranges 8, 8, 9, 8, 9 that cross the images' 14-tile "
            "boundaries; 3 idle blocks per group in the round of 8"),
    Row((5, 96, 48, 20, 72), (4, 1, 3, F_), (1, 1, 2, F_), (1, 2, 2, 100, 8, 8), (T, 6, 42, (1, 2)),
        why="wg cfg 1, ncislab 2 (64 + 32), 100 tiles: ksplit 12 rounded down to 8, ranges of 12 and 13"),
    Row((8, 40, 24, 16, 72), (3, 1, 2, F_), (4, 1, 1, F_), (2, 1, 1, 128, 16, 16), (T, 2, 96, (1, 1)),
        why="wg cfg 2, ksplit 16: two rounds of 8"),
    Row((2, 32, 136, 9, 136), (0, 1, 1, F_), (3, 1, 5, F_), (3, 1, 2, 30, 3, 3), (T, 5, 30, (1, 1)),
        why="wg cfg 3, Cout = 128 + 8, ksplit 3, odd H (the last tile row has one live row), column tiles 64 + 64 + 8"),
    Row((4, 24, 64, 7, 64), (4, 1, 1, F_), (3, 1, 2, F_), (4, 1, 1, 16, 2, 2), (T, 2, 16, (1, 1)),
        why="wg cfg 4, ksplit 2"),
    Row((3, 8, 8, 13, 8), (3, 1, 1, T), (3, 1, 1, T), (5, 1, 1, 21, 2, 2), (T, 1, 12, (1, 1)),
        why="wg cfg 5, ksplit 2 (10 and 11 tiles); the smallest row: C oracle and torch compared on it"),
    # ---- fp32 only
    Row((1, 40, 70, 6, 33), None, None, None, (F_, 6, 4, (1, 1)), types=(F32,),
        why="W % 4 != 0: the element-wise staging of all three kernels at K = 5 (16-bit needs W % 8 == 0)"),
    Row((1, 160, 160, 22, 168), None, None, None, (T, 25, 10, (3, 4)), ks=(5,), types=(F32,), passes=("wgrad",),
        why="fp32 wg: 25 groups, nsplit 10, 36 tiles: 3 or 4 tiles per block on the loader-wave path, the third is the "
            "first to reuse an LDS buffer; last column tile 8 wide, last row tile 2 high"),
]
BY_SHAPE = {r.shape: r for r in ROWS}
SMALLEST = (3, 8, 8, 13, 8)
# ofasr_conv2d_fwd_stat and ofasr_conv2d_infer_run: cfg 0 (WP 1), cfg 1 (WP 2), cfg 2 (WP 4); Cout % 4 == 0 for PixelShuffle
STAT_ROWS = [(2, 40, 160, 5, 72), (2, 96, 72, 9, 136), (256, 48, 40, 9, 8)]
STAT_MAX = 180.0     # 128 squares of it, in quarters, still sum exactly in fp32: 128 * 180^2 * 4 < 2^24
assert 128 * STAT_MAX ** 2 * 4 < 2 ** 24


def cases(types=None):
    """(row, K, dtype) of every run the table asks for"""
    return [(r, k, d) for r in ROWS for k in r.ks for d in r.types if types is None or d in types]


def geometry(shape):
    """the restated rules in the table's form: (fwd, dgrad, wg, f32)"""
    return cv_geom(*shape, 5, 0), cv_geom(*shape, 5, 1), cv_wg_geom(*shape), cf_geom(*shape)


# ---------------------------------------------------------------------------------------------- data and references
ORACLE_MACS = 40e6    # multiply-adds per pass up to which the C oracle computes the reference (well under a second)


def macs(shape, K):
    N, Cin, Cout, H, W = shape
    return N * Cin * Cout * H * W * K * K


def rounded(a, dtype):
    """`a` rounded once to `dtype` with torch's cast, back as float32"""
    return torch.tensor(np.asarray(a)).to(dtype).float().numpy()


def operands(shape, K):
    """x, dy in {-1, 0, 1}; w in {-1, -0.5, 0, 0.5, 1}"""
    N, Cin, Cout, H, W = shape
    x = det_ints((N, Cin, H, W), "cvg/x%s" % (shape,), -1, 2)
    dy = det_ints((N, Cout, H, W), "cvg/dy%s" % (shape,), -1, 2)
    w = det_ints((Cout, Cin, K, K), "cvg/w%s/%d" % (shape, K), -2, 3) / np.float32(2)
    assert np.all(np.isin(x, [-1, 0, 1])) and np.all(np.isin(dy, [-1, 0, 1])) and np.all(np.isin(2 * w, [-2, -1, 0, 1, 2]))
    return x, w, dy


def torch_reference(x, w, dy, K):
    """y, dx, dw by torch in float64 on the CPU"""
    xt, wt, dyt = (torch.from_numpy(a).double() for a in (x, w, dy))
    y = torch.nn.functional.conv2d(xt, wt, padding=K // 2)
    dx = torch.nn.grad.conv2d_input(xt.shape, wt, dyt, padding=K // 2)
    dw = torch.nn.grad.conv2d_weight(xt, wt.shape, dyt, padding=K // 2)
    return tuple(t.numpy().astype(np.float32) for t in (y, dx, dw))


def oracle_reference(ora, x, w, dy):
    y = ora.conv2d_fwd(x, w)
    dx, dw = ora.conv2d_bwd(dy, x, w)
    return y, dx, dw


def bf16_inexact_fraction(a):
    return float(np.mean(rounded(a, BF16) != a))


def check_exactness(shape, K, y, dx, dw):
    """the conditions under which `expected` below is what a correct kernel must give bit for bit"""
    N, Cin, Cout, H, W = shape
    for name, t, terms in (("y", y, Cin * K * K), ("dx", dx, Cout * K * K)):
        assert t.dtype == np.float32 and np.array_equal(2 * t, np.round(2 * t)), "%s is not a multiple of 0.5" % name
        assert float(np.abs(t).max()) <= terms < 2 ** 22, (name, terms)
        assert np.any(t), "%s is identically zero" % name
        assert np.array_equal(rounded(t, F16), t), "%s is not exact in f16" % name           # |t| < 2048 halves
        frac = bf16_inexact_fraction(t)
        assert frac <= 0.01, "%s: %.2f %% of the bf16 expected values are rounded; rounding could hide an error" % (name, 100 * frac)
    assert dw.dtype == np.float32 and np.array_equal(dw, np.round(dw)) and float(np.abs(dw).max()) <= N * H * W < 2 ** 24
    assert np.any(dw), "dw is identically zero"
    if shape in STAT_ROWS:
        assert float(np.abs(y).max()) <= STAT_MAX, "max|y| = %g: the statistics sums are not exact" % float(np.abs(y).max())


_REF = {}


def reference(ora, shape, K):
    """{x, w, dy, y, dx, dw}: exact-arithmetic operands and results, float32, computed once per (shape, K), checked for
    the exactness conditions and left unchanged (read-only arrays)"""
    key = (tuple(shape), K)
    if key not in _REF:
        x, w, dy = operands(shape, K)
        if macs(shape, K) <= ORACLE_MACS:
            y, dx, dw = oracle_reference(ora, x, w, dy)
        else:
            y, dx, dw = torch_reference(x, w, dy, K)
        check_exactness(tuple(shape), K, y, dx, dw)
        ref = dict(x=x, w=w, dy=dy, y=y, dx=dx, dw=dw)
        for a in ref.values():
            a.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def expected(ref, what, dtype):
    """what a correct kernel stores: dw and fp32 results are the exact values, 16-bit y / dx the exact value rounded once"""
    a = ref[what]
    return a if (what == "dw" or dtype == F32) else rounded(a, dtype)
