"""The dense static convolutions (csrc/conv2d.hip: conv_igemm_kernel, conv_wgrad_kernel + its reduce; csrc/conv2d_f32.hip:
conv_f32_kernel, conv_f32_wgrad_kernel + its reduce) bit for bit at every launch geometry they have.  `-m gpu`.

The rows, what each reaches, the exact data and the references are tests/conv_geometry.py; tests/test_conv_geometry.py
checks them without a GPU.  Here every row runs through the C ABI (include/ofasr.h) in bf16, f16 and fp32: forward, input
gradient, weight gradient, compared with np.array_equal -- no tolerance: on this data every fp32 accumulation is exact, so
a correct kernel gives the exact result (fp32, dw) or the exact result rounded once (16-bit y, dx).  A tile that drops one
tap, a split that counts one pixel tile twice or a slab the reduce forgets changes a value by at least 0.5.

Operands are placed with tests/placed.py at P0 between NaN guard bands, inputs must stay unchanged, outputs start as NaN
canaries, workspaces have exactly the queried size.

The guard: after each call the launch table holds exactly the template instance the row names (and the operand
preparation / reduce kernel that belongs to it), and the workspace queries equal ksplit * K * nz * nwq * rbw * K * 16 * 64 * 4
and nsplit * 2 * Cout * Cin * K^2 * 4 bytes for the ksplit / nsplit the row names: a later retuning cannot slide a row into
another geometry unnoticed.  When the guard fails, restate the rule in conv_geometry.py and re-pick the row.

What it is sensitive to, tried once with a deliberately wrong library: a reduce that leaves out the last of five split
slabs, fp32 compute waves that skip a block's third pixel tile, and 0.5 added to one accumulator register of cfg 2 each
failed exactly the rows that name that geometry, while test_hip_conv2d.py, test_hip_placement_abi.py and
test_hip_conv_thin.py passed on that library.

Also on the rows at cfg 0, 1, 2 (WP = 1, 2, 4 waves along the tile's rows):
    ofasr_conv2d_fwd_stat    every partial[c][u] written; sum_u of both components, folded in float64, equals the sum and
                             the sum of squares of the stored output exactly (|y| <= 180: 128 squares sum exactly in fp32)
    ofasr_conv2d_infer_run   without BN, act 0 / 1 / 2: the exact result, clipped to [0, 6] / pixel-shuffled, rounded once
    ... with BN (first row)  within one unit in the last place of the 16-bit type of acc * scale + shift in double.  The
                             kernel's fp32 scale, shift and fma are off by at most d = 2^-21 (|acc * scale| + |shift|)
                             (rsqrtf 2 ulp, four more roundings); the BN parameters keep |result| >= 2, so d is below a
                             quarter of that unit (asserted on the data) and one rounding of the fp32 value lands on one
                             of the two 16-bit neighbours of the double value."""
import ctypes

import numpy as np
import pytest
import torch

import conv_geometry as cg
from conftest import amd
from conv_geometry import BF16, F16, F32
from detfill import det_uniform
from placed import check, place, workspace

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODE = {F32: 0, F16: 1, BF16: 2}
NAME = {F32: "fp32", F16: "f16", BF16: "bf16"}
TNAME = {BF16: "ofasr::bf16_t", F16: "ofasr::f16_t"}
OK = 0


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert cg.cf_blocks() == 256, "the table is written for the default OFASR_CONV_F32_WG_BLOCKS"
    return amd("_C").lib()


def G(a, dtype=F32):
    return torch.tensor(np.asarray(a)).to(dtype).to(DEV)


def E(shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device=DEV)


def Hn(t):
    return t.detach().float().cpu().numpy()


def ptr(t):
    if t is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t.ptr)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def status_ok(L, rc, what):
    assert rc == OK, "%s returned %d (%s)" % (what, rc, L.ofasr_last_error_string().decode())


def finish(*placed_things):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device error: start nothing else on this device
        pytest.exit("device error after a conv launch, ending the run: %s" % e, returncode=3)
    for p in placed_things:
        check(p)


def assert_exact(what, got, want, axes):
    """np.array_equal, and on a mismatch: how many, where first, and the index ranges the wrong elements span"""
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(~(got == want))
    i = tuple(int(v) for v in bad[0])
    spans = ", ".join("%s %d..%d (%d distinct)" % (a, bad[:, d].min(), bad[:, d].max(), len(np.unique(bad[:, d])))
                      for d, a in enumerate(axes))
    raise AssertionError("%s differs at %d of %d elements, first at %s: got %r expected %r; %s"
                         % (what, len(bad), want.size, i, got[i], want[i], spans))


ACT_AXES = ("image", "channel", "row", "column")
DW_AXES = ("co", "ci", "ty", "tx")


def launched(want, what):
    """the launch table holds exactly `want` {full kernel symbol: launches}"""
    table = amd("_C").launch_table()
    assert table == want, "%s: launched %s, the row names %s" % (what, table, want)


def igemm_name(dtype, K, geom):
    rb, wm, wp = cg.CV_CFGS[geom[0]]
    return "conv_igemm_kernel<%s, %d, %d, %d, %d, %s>" % (TNAME[dtype], K, rb, wm, wp, "true" if geom[3] else "false")


def conv_kernels(row, K, dtype, dgrad):
    if dtype == F32:
        return {"conv_f32_prep_kernel": 1, "conv_f32_kernel<%d>" % K: 1}
    return {"conv_prep_kernel<%s>" % TNAME[dtype]: 1, igemm_name(dtype, K, row.dgrad if dgrad else row.fwd): 1}


def wgrad_kernels(row, K, dtype):
    if dtype == F32:
        return {"conv_f32_wgrad_kernel<%d>" % K: 1, "conv_f32_wgrad_reduce_kernel": 1}
    rbw, wco, wci, wk = cg.CV_WG_CFGS[row.wg[0]]
    return {"conv_wgrad_kernel<%s, %d, %d, %d, %d, %d>" % (TNAME[dtype], K, rbw, wco, wci, wk): 1,
            "conv_wgrad_reduce_kernel<%d, %d, %d, %d>" % (K, rbw, wco, wci): 1}


class Conv(object):
    """the entry points of one (row, K, dtype); operands placed at P0 between guards, workspaces of the queried size"""

    def __init__(self, L, shape, K, dtype):
        self.L, self.dtype, self.K = L, dtype, K
        self.N, self.Cin, self.Cout, self.H, self.W = shape
        self.f32 = dtype == F32
        self.dims = (self.N, self.Cin, self.Cout, self.H, self.W, K)

    def _ws(self, dgrad):
        L = self.L
        n = L.ofasr_conv2d_f32_workspace(self.Cin, self.Cout, self.K, dgrad) if self.f32 else \
            L.ofasr_conv2d_workspace(self.Cin, self.Cout, self.K, dgrad)
        return workspace(n, DEV)

    def fwd(self, xg, wg, units=None):
        """-> (y, partial or None)"""
        L = self.L
        px, pw = place(xg, 0, "in", "x"), place(wg, 0, "in", "w")
        py = place(E((self.N, self.Cout, self.H, self.W), self.dtype), 0, "out", "y")
        ws = self._ws(0)
        pp = None
        amd("_C").reset_launch_counts()
        if units is not None:
            pp = place(E((self.Cout, units, 2)), 0, "out", "partial")
            rc = L.ofasr_conv2d_fwd_stat(ptr(px), ptr(pw), ptr(py), *self.dims, CODE[self.dtype], ptr(pp), units, ptr(ws),
                                         ws.nbytes, stream())
        elif self.f32:
            rc = L.ofasr_conv2d_f32_fwd(ptr(px), ptr(pw), ptr(py), *self.dims, ptr(ws), ws.nbytes, stream())
        else:
            rc = L.ofasr_conv2d_fwd(ptr(px), ptr(pw), ptr(py), *self.dims, CODE[self.dtype], ptr(ws), ws.nbytes, stream())
        status_ok(L, rc, "conv2d fwd")
        finish(*[p for p in (px, pw, py, ws, pp) if p is not None])
        return py, pp

    def dgrad(self, dyg, wg):
        L = self.L
        pdy, pw = place(dyg, 0, "in", "dy"), place(wg, 0, "in", "w")
        pdx = place(E((self.N, self.Cin, self.H, self.W), self.dtype), 0, "out", "dx")
        ws = self._ws(1)
        amd("_C").reset_launch_counts()
        if self.f32:
            rc = L.ofasr_conv2d_f32_dgrad(ptr(pdy), ptr(pw), ptr(pdx), *self.dims, ptr(ws), ws.nbytes, stream())
        else:
            rc = L.ofasr_conv2d_dgrad(ptr(pdy), ptr(pw), ptr(pdx), *self.dims, CODE[self.dtype], ptr(ws), ws.nbytes, stream())
        status_ok(L, rc, "conv2d dgrad")
        finish(pdy, pw, pdx, ws)
        return pdx

    def wgrad_bytes(self):
        L = self.L
        return int(L.ofasr_conv2d_f32_wgrad_workspace(*self.dims) if self.f32 else L.ofasr_conv2d_wgrad_workspace(*self.dims))

    def wgrad(self, dyg, xg):
        L = self.L
        pdy, px = place(dyg, 0, "in", "dy"), place(xg, 0, "in", "x")
        pdw = place(E((self.Cout, self.Cin, self.K, self.K)), 0, "out", "dw")
        ws = workspace(self.wgrad_bytes(), DEV)
        amd("_C").reset_launch_counts()
        if self.f32:
            rc = L.ofasr_conv2d_f32_wgrad(ptr(pdy), ptr(px), ptr(pdw), *self.dims, ptr(ws), ws.nbytes, stream())
        else:
            rc = L.ofasr_conv2d_wgrad(ptr(pdy), ptr(px), ptr(pdw), *self.dims, CODE[self.dtype], ptr(ws), ws.nbytes, stream())
        status_ok(L, rc, "conv2d wgrad")
        finish(pdy, px, pdw, ws)
        return pdw

    def infer(self, xg, wg, act, bn=None):
        """ofasr_conv2d_infer_prepare + _run -> (y, launch table of the prepare, of the run)"""
        L, C = self.L, amd("_C")
        pw = place(wg, 0, "in", "w")
        pbn = [place(G(a), 0, "in", n) for n, a in zip(("gamma", "beta", "mean", "var"), bn[:4])] if bn else [None] * 4
        ops = workspace(L.ofasr_conv2d_infer_operand_bytes(self.Cin, self.Cout, self.K), DEV, "operands")
        C.reset_launch_counts()
        rc = L.ofasr_conv2d_infer_prepare(ptr(pw), *[ptr(p) for p in pbn], float(bn[4]) if bn else 0.0, self.Cin, self.Cout,
                                          self.K, CODE[self.dtype], ptr(ops), ops.nbytes, stream())
        status_ok(L, rc, "conv2d infer_prepare")
        finish(pw, ops, *[p for p in pbn if p is not None])
        t_prep = C.launch_table()
        px = place(xg, 0, "in", "x")
        oshape = (self.N, self.Cout // 4, 2 * self.H, 2 * self.W) if act == 2 else (self.N, self.Cout, self.H, self.W)
        py = place(E(oshape, self.dtype), 0, "out", "y")
        C.reset_launch_counts()
        rc = L.ofasr_conv2d_infer_run(ptr(px), ptr(py), self.N, self.Cin, self.Cout, self.H, self.W, self.K, CODE[self.dtype],
                                      act, ptr(ops), ops.nbytes, stream())
        status_ok(L, rc, "conv2d infer_run")
        finish(px, py, ops)
        return py, t_prep, C.launch_table()


def _id(case):
    row, K, dtype = case
    return "%s-k%d-%s" % (row.id, K, NAME[dtype])


@pytest.mark.parametrize("case", cg.cases(), ids=_id)
def test_conv_exact_at_every_geometry(L, ora, case):
    row, K, dtype = case
    N, Cin, Cout, H, W = row.shape
    ref = cg.reference(ora, row.shape, K)
    conv = Conv(L, row.shape, K, dtype)
    what = "%s K%d %s" % (row.shape, K, NAME[dtype])
    errs = []

    def run(label, fn):
        if label not in row.passes:
            return
        try:
            fn()
        except AssertionError as e:
            errs.append("[%s %s] %s" % (what, label, e))

    def fwd():
        py, _ = conv.fwd(G(ref["x"], dtype), G(ref["w"]))
        want = conv_kernels(row, K, dtype, 0)
        print("observed %s fwd: %s" % (what, sorted(amd("_C").launch_table())))
        launched(want, "fwd")
        assert_exact("y", Hn(py), cg.expected(ref, "y", dtype), ACT_AXES)

    def dgrad():
        pdx = conv.dgrad(G(ref["dy"], dtype), G(ref["w"]))
        want = conv_kernels(row, K, dtype, 1)
        print("observed %s dgrad: %s" % (what, sorted(amd("_C").launch_table())))
        launched(want, "dgrad")
        assert_exact("dx", Hn(pdx), cg.expected(ref, "dx", dtype), ACT_AXES)

    def wgrad():
        got = conv.wgrad_bytes()
        if dtype == F32:
            p = cg.cf_plan(N, Cin, Cout, H, W, K)
            assert p["nsplit"] == row.f32[2]
            unit = 2 * Cout * Cin * K * K * 4
            print("observed %s wgrad: workspace %d B = nsplit %g" % (what, got, got / unit))
            assert got == p["part_bytes"] == row.f32[2] * unit, "fp32 wgrad workspace %d B: nsplit %g, the row says %d" % (got, got / unit, row.f32[2])
        else:
            p = cg.cv_wg_plan(N, Cin, Cout, H, W, K)
            ksplit = row.wg[4] if K == 3 else row.wg[5]
            unit = K * p["nz"] * p["nwq"] * p["rbw"] * K * 16 * 64 * 4
            print("observed %s wgrad: workspace %d B = ksplit %g" % (what, got, got / unit))
            assert p["ksplit"] == ksplit and (p["nz"], p["ncislab"]) == (row.wg[2], row.wg[1])
            assert got == p["part_bytes"] == ksplit * unit, "wgrad workspace %d B: ksplit %g, the row says %d" % (got, got / unit, ksplit)
        pdw = conv.wgrad(G(ref["dy"], dtype), G(ref["x"], dtype))
        print("observed %s wgrad: %s" % (what, sorted(amd("_C").launch_table())))
        launched(wgrad_kernels(row, K, dtype), "wgrad")
        assert not bool(pdw.placement.unwritten().any()), "dw: elements never written"
        assert_exact("dw", Hn(pdw), cg.expected(ref, "dw", dtype), DW_AXES)

    run("fwd", fwd)
    run("dgrad", dgrad)
    run("wgrad", wgrad)
    assert not errs, "%d pass(es) failed:\n%s" % (len(errs), "\n".join(errs))


EPILOGUE_CASES = [(cg.BY_SHAPE[s], K, d) for s in cg.STAT_ROWS for K in (3, 5) for d in (BF16, F16)]


@pytest.mark.parametrize("case", EPILOGUE_CASES, ids=_id)
def test_statistics_epilogue_exact(L, ora, case):
    """ofasr_conv2d_fwd_stat at WP = 1, 2, 4: one partial per (channel, wave strip of 2 x 64 pixels); strips below the
    image (row tiles 2 + 2 + 1, 4 + 4 + 1, 8 + 1) still write their zeros"""
    row, K, dtype = case
    N, Cin, Cout, H, W = row.shape
    ref = cg.reference(ora, row.shape, K)
    conv = Conv(L, row.shape, K, dtype)
    units = L.ofasr_conv2d_stat_units(N, Cin, Cout, H, W, K)
    assert units == cg.cv_plan(N, Cin, Cout, H, W, K, 0)["units"], units
    py, pp = conv.fwd(G(ref["x"], dtype), G(ref["w"]), units=units)
    launched(conv_kernels(row, K, dtype, 0), "fwd_stat")
    y = Hn(py)
    assert_exact("y", y, cg.expected(ref, "y", dtype), ACT_AXES)
    assert not bool(pp.placement.unwritten().any()), "statistics partials not all written"
    part = pp.cpu().numpy().astype(np.float64)
    assert np.isfinite(part).all()
    yd = y.astype(np.float64)
    s_ref, q_ref = yd.sum(axis=(0, 2, 3)), (yd * yd).sum(axis=(0, 2, 3))
    assert float(q_ref.max()) < 2 ** 51      # quarters: the float64 folds are exact too
    assert_exact("sum", part[:, :, 0].sum(axis=1), s_ref, ("channel",))
    assert_exact("sum of squares", part[:, :, 1].sum(axis=1), q_ref, ("channel",))


@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "relu6", "pixelshuffle"])
@pytest.mark.parametrize("case", EPILOGUE_CASES, ids=_id)
def test_inference_epilogue_exact_without_bn(L, ora, case, act):
    row, K, dtype = case
    ref = cg.reference(ora, row.shape, K)
    conv = Conv(L, row.shape, K, dtype)
    py, t_prep, t_run = conv.infer(G(ref["x"], dtype), G(ref["w"]), act)
    assert t_prep == {"conv_prep_kernel<%s>" % TNAME[dtype]: 1}, t_prep
    assert t_run == {igemm_name(dtype, K, row.fwd): 1}, t_run
    want = ref["y"]
    if act == 1:
        want = np.clip(want, 0.0, 6.0)
    elif act == 2:
        want = ora.pixel_shuffle(want, 2)
    assert_exact("y", Hn(py), cg.rounded(want, dtype), ACT_AXES)


def ulp16(e, dtype):
    """the spacing of `dtype` at |e| (0 at 0): 8 significand bits in bf16, 11 in f16"""
    a = np.abs(e)
    ex = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a > 0, 2.0 ** (ex - (7 if dtype == BF16 else 10)), 0.0)


@pytest.mark.parametrize("act", [0, 1, 2], ids=["none", "relu6", "pixelshuffle"])
@pytest.mark.parametrize("case", [c for c in EPILOGUE_CASES if c[0].shape == cg.STAT_ROWS[0]], ids=_id)
def test_inference_epilogue_with_bn_within_one_ulp(L, ora, case, act):
    row, K, dtype = case
    N, Cin, Cout, H, W = row.shape
    ref = cg.reference(ora, row.shape, K)
    tag = "cvg/bn%s" % (row.shape,)
    gamma = det_uniform((Cout,), tag + "g", 0.5, 1.5) / np.float32(16)
    var = det_uniform((Cout,), tag + "v", 0.5, 1.5)
    mean = det_uniform((Cout,), tag + "m", -0.3, 0.3)
    beta = det_uniform((Cout,), tag + "b", 12.0, 13.0) * np.where(np.arange(Cout) % 3 == 1, -1, 1).astype(np.float32)
    eps = 1e-5
    sc = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + eps)
    sh = beta.astype(np.float64) - mean.astype(np.float64) * sc
    acc = ref["y"].astype(np.float64)
    sc4, sh4 = sc.reshape(1, -1, 1, 1), sh.reshape(1, -1, 1, 1)
    e = acc * sc4 + sh4
    # the condition under which one ulp is the bound (see the docstring of this file)
    d = 2.0 ** -21 * (np.abs(acc * sc4) + np.abs(sh4))
    assert float(np.abs(e).min()) >= 2.0 and bool((d <= ulp16(e, dtype) / 4).all())
    if act == 1:
        e = np.clip(e, 0.0, 6.0)
    elif act == 2:
        e = ora.pixel_shuffle(e, 2)
    conv = Conv(L, row.shape, K, dtype)
    py, t_prep, t_run = conv.infer(G(ref["x"], dtype), G(ref["w"]), act, bn=(gamma, beta, mean, var, eps))
    assert t_prep == {"conv_prep_kernel<%s>" % TNAME[dtype]: 1}, t_prep
    assert t_run == {igemm_name(dtype, K, row.fwd): 1}, t_run
    got = Hn(py).astype(np.float64)
    assert got.shape == e.shape and np.isfinite(got).all()
    err, tol = np.abs(got - e), ulp16(e, dtype)
    print("infer with BN %s K%d %s act %d: max |error| / ulp = %.3f" % (row.shape, K, NAME[dtype], act,
                                                                      float((err / np.where(tol > 0, tol, 1.0)).max())))
    if not (err <= tol).all():
        bad = np.argwhere(err > tol)
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("y is more than one ulp from acc * scale + shift at %d of %d elements, first at %s: got %r expected %r"
                             % (len(bad), e.size, i, got[i], e[i]))
