"""The arithmetic kernels on misaligned, guard-banded operands, through the C ABI (include/ofasr.h), where the caller
places every operand and workspace (tests/placed.py).

Every compute entry point picks its kernel from the ADDRESSES it is given; the rest of the suite hands them allocator
pointers only (256-byte aligned, sizes rounded up).  Here every operand sits between guard bands at 0 (P0), one element
(P1) or 8 bytes (P8) past a 16-byte boundary: all operands together, then each pointer alone at P1.  Workspaces have
exactly the queried size.  After each call
  * the result is compared with the CPU oracle on the same rounded inputs, at the tolerance the kernel already has in
    test_hip_kernels.py / test_hip_bnact.py / test_hip_conv2d.py (restated below with its source; nothing new),
  * every operand and workspace is check()ed: guards intact (no write outside), inputs unchanged; a read outside an input
    meets NaN and fails the comparison; an output element never written keeps its NaN canary and fails it too.
A failure names the placement ("x@P1": only x one element off) and the operand, so the dispatch branch to read is known.
Where misalignment is refused by contract (the 16-bit static conv, the PixelShuffle-BN pair) the refusal is asserted.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import amd, assert_close
from detfill import det_ints, det_uniform
from placed import check, lead_of, place, workspace

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
CODE = {F32: 0, F16: 1, BF16: 2}
OK, UNSUPPORTED = 0, -2


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return amd("_C").lib()


# ------------------------------------------------------------------------------------------------ tolerances (restated)
def tol(dtype, scale=1.0):
    """test_hip_kernels.py tol(): activations of the pointwise / depthwise kernels"""
    if dtype == F32:
        return dict(rtol=2e-5, atol=2e-6 * scale)
    if dtype == BF16:
        return dict(rtol=1e-2, atol=1e-2 * scale)
    return dict(rtol=2e-3, atol=2e-3 * scale)


def wgrad_tol(n_terms):
    """test_hip_kernels.py test_pwconv_vs_oracle / test_dwconv_vs_oracle: weight gradients, all dtypes"""
    return dict(rtol=1e-4, atol=2e-6 * max(1.0, float(np.sqrt(n_terms))))


def bn_tol(dtype):
    """test_hip_bnact.py _tol()"""
    return {F32: (5e-5, 5e-6), BF16: (1.5e-2, 1.5e-2), F16: (3e-3, 3e-3)}[dtype]


def conv16_rt(dtype):
    """test_hip_conv2d.py test_conv2d_vs_oracle"""
    return 1e-2 if dtype == BF16 else 2e-3


# ------------------------------------------------------------------------------------------------------------- plumbing
def rounded(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


def G(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def E(shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device=DEV)


def Hn(t):
    return t.detach().float().cpu().numpy()


def plans(names, alone=None):
    """[(label, {operand: placement})]: all P0, all P1, all P8, then each pointer the dispatcher looks at alone at P1"""
    out = [("all@" + p, dict((n, p) for n in names)) for p in ("P0", "P1", "P8")]
    for n in (names if alone is None else alone):
        d = dict((m, "P0") for m in names)
        d[n] = "P1"
        out.append((n + "@P1", d))
    return out


def put(t, plan, name, role):
    return place(t, lead_of(plan.get(name, "P0"), t.element_size()), role, name)


def ptr(t):
    """address of a placed tensor (or a slice of one), of a workspace() placement, or NULL"""
    if t is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t.ptr)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def status_ok(L, rc, what):
    assert rc == OK, "%s returned %d (%s)" % (what, rc, L.ofasr_last_error_string().decode())


class Report(object):
    """runs every placement of a case and reports all that fail, each under its label"""

    def __init__(self, what):
        self.what, self.errs, self.n = what, [], 0

    def run(self, label, fn):
        self.n += 1
        try:
            fn()
            torch.cuda.synchronize()
        except AssertionError as e:
            self.errs.append("[%s %s] %s" % (self.what, label, e))

    def done(self):
        assert not self.errs, "%d of %d placements failed:\n%s" % (len(self.errs), self.n, "\n".join(self.errs))


def finish(*placed_things):
    torch.cuda.synchronize()
    for p in placed_things:
        if p is not None:
            check(p)


_REF = {}


def cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------ pointwise
PW_CASES = [
    # Cin, Cout, ldw (Cin_max), Cout_max, HW
    (64, 256, 64, 384, 256),    # slab walk, two tiles per image
    (64, 192, 64, 384, 136),    # generic fan-out, whole tile plus an 8-pixel tail
    (256, 64, 384, 64, 256),    # pipelined fan-in
    (100, 70, 128, 96, 136),    # generic fan-in
    (64, 256, 64, 384, 135),    # odd, more than one tile: the unaligned kernels' multi-tile walk
    (256, 64, 384, 64, 135),
    (64, 256, 64, 384, 289),
    (256, 64, 384, 64, 289),
]


def _pw_ref(ora, case, dtype):
    Cin, Cout, ldw, Cout_max, HW = case
    N = 2

    def make():
        x = rounded(det_uniform((N, Cin, 1, HW), "pab/x%s" % (case,)), dtype)
        a = float(np.sqrt(3.0 / Cin))
        w = det_uniform((Cout_max, ldw, 1, 1), "pab/w%s" % (case,), -a, a)
        dy = rounded(det_uniform((N, Cout, 1, HW), "pab/dy%s" % (case,)), dtype)
        w_eff = w if dtype == F32 else rounded(w, dtype)      # 16-bit paths round the master weights in the kernel
        y = ora.pwconv_fwd(x, w_eff, Cout)
        dx, _ = ora.pwconv_bwd(dy, x, w_eff)
        _, dw = ora.pwconv_bwd(dy, x, w)
        return x, w, dy, y, dx, dw
    return cached(("pw", case, dtype), make)


@pytest.mark.parametrize("case", PW_CASES, ids=lambda c: "%dto%d_hw%d" % (c[0], c[1], c[4]))
@pytest.mark.parametrize("dtype", DTYPES)
def test_pwconv_placed(L, ora, case, dtype):
    Cin, Cout, ldw, Cout_max, HW = case
    N = 2
    x, w, dy, y_ref, dx_ref, dw_ref = _pw_ref(ora, case, dtype)
    xg, wg, dyg = G(x, dtype).view(N, Cin, HW), G(w).view(Cout_max, ldw), G(dy, dtype).view(N, Cout, HW)
    rep = Report("pwconv %s %s" % (case, dtype))

    def fwd(plan):
        px, pw, py = put(xg, plan, "x", "in"), put(wg, plan, "w", "in"), put(E((N, Cout, HW), dtype), plan, "y", "out")
        status_ok(L, L.ofasr_pwconv_fwd(ptr(px), ptr(pw), ldw, ptr(py), N, Cin, Cout, HW, CODE[dtype], stream()), "pwconv_fwd")
        finish(px, pw, py)
        assert_close(Hn(py), y_ref.reshape(N, Cout, HW), what="y", **tol(dtype))

    def dgrad(plan):
        pdy, pw = put(dyg, plan, "dy", "in"), put(wg, plan, "w", "in")
        pdx = put(E((N, Cin, HW), dtype), plan, "dx", "out")
        status_ok(L, L.ofasr_pwconv_dgrad(ptr(pdy), ptr(pw), ldw, ptr(pdx), N, Cin, Cout, HW, CODE[dtype], stream()),
                  "pwconv_dgrad")
        finish(pdy, pw, pdx)
        assert_close(Hn(pdx), dx_ref.reshape(N, Cin, HW), what="dx",
                     **tol(dtype, np.sqrt(Cout / Cin) if Cout > Cin else 1.0))

    def wgrad(plan):
        pdy, px = put(dyg, plan, "dy", "in"), put(xg, plan, "x", "in")
        pdw = put(E((Cout_max, ldw)), plan, "dw", "out")
        ws = workspace(L.ofasr_pwconv_wgrad_workspace(N, Cin, Cout, HW), DEV)
        status_ok(L, L.ofasr_pwconv_wgrad(ptr(pdy), ptr(px), ptr(pdw), ldw, N, Cin, Cout, HW, CODE[dtype], ptr(ws),
                                          ws.nbytes, stream()), "pwconv_wgrad")
        finish(pdy, px, pdw, ws)
        inside = torch.zeros((Cout_max, ldw), dtype=torch.bool, device=DEV)
        inside[:Cout, :Cin] = True
        assert torch.equal(pdw.placement.unwritten(), ~inside), "dw: only the [:Cout, :Cin] slice may be written, and all of it"
        assert_close(Hn(pdw)[:Cout, :Cin], dw_ref.reshape(Cout_max, ldw)[:Cout, :Cin], what="dw", **wgrad_tol(N * HW))

    for label, plan in plans(["y", "x", "w"]):
        rep.run("fwd " + label, lambda: fwd(plan))
    for label, plan in plans(["dx", "dy", "w"]):
        rep.run("dgrad " + label, lambda: dgrad(plan))
    for label, plan in plans(["dw", "dy", "x"]):
        rep.run("wgrad " + label, lambda: wgrad(plan))
    rep.done()


# ------------------------------------------------------------------------------------------------------------ depthwise
DW_SHAPES = [
    (2, 6, 32, 32),     # matrix-core geometry when aligned, strip kernel when not
    (1, 4, 64, 64),
    (2, 6, 12, 8),
    (1, 3, 70, 65),
    (1, 6, 40, 150),
    (1, 2, 37, 132),    # vector kernels, two slabs per plane, rows of 33 lanes: clamped halo-row loads of both slabs
    (1, 2, 70, 256),    # three slabs (two at 8 pixels per lane): the weight gradient's workspace holds a partial per slab
]


@pytest.mark.parametrize("shape", DW_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", [1, 3, 5, 7])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dwconv_placed(L, ora, shape, k, dtype):
    N, C, Hh, W = shape

    def make():
        x = rounded(det_uniform(shape, "dab/x%s" % (shape,)), dtype)
        f = det_uniform((C, 1, k, k), "dab/f%d_%d" % (C, k), -0.4, 0.4)
        dy = rounded(det_uniform(shape, "dab/dy%s" % (shape,)), dtype)
        dx, df = ora.dwconv_bwd(dy, x, f)
        return x, f, dy, ora.dwconv_fwd(x, f), dx, df
    x, f, dy, y_ref, dx_ref, df_ref = cached(("dw", shape, k, dtype), make)
    xg, fg, dyg = G(x, dtype), G(f).view(C, k, k), G(dy, dtype)
    rep = Report("dwconv %s k%d %s" % (shape, k, dtype))

    def fwd(plan):
        px, pf, py = put(xg, plan, "x", "in"), put(fg, plan, "f", "in"), put(E(shape, dtype), plan, "y", "out")
        status_ok(L, L.ofasr_dwconv_fwd(ptr(px), ptr(pf), ptr(py), N, C, Hh, W, k, CODE[dtype], stream()), "dwconv_fwd")
        finish(px, pf, py)
        assert_close(Hn(py), y_ref, what="y", **tol(dtype, k))

    def dgrad(plan):
        pdy, pf, pdx = put(dyg, plan, "dy", "in"), put(fg, plan, "f", "in"), put(E(shape, dtype), plan, "dx", "out")
        status_ok(L, L.ofasr_dwconv_dgrad(ptr(pdy), ptr(pf), ptr(pdx), N, C, Hh, W, k, CODE[dtype], stream()), "dwconv_dgrad")
        finish(pdy, pf, pdx)
        assert_close(Hn(pdx), dx_ref, what="dx", **tol(dtype, k))

    def wgrad(plan):
        pdy, px, pdf = put(dyg, plan, "dy", "in"), put(xg, plan, "x", "in"), put(E((C, k, k)), plan, "df", "out")
        ws = workspace(L.ofasr_dwconv_wgrad_workspace(N, C, Hh, W, k), DEV)
        status_ok(L, L.ofasr_dwconv_wgrad(ptr(pdy), ptr(px), ptr(pdf), N, C, Hh, W, k, CODE[dtype], ptr(ws), ws.nbytes,
                                          stream()), "dwconv_wgrad")
        finish(pdy, px, pdf, ws)
        assert_close(Hn(pdf), df_ref.reshape(C, k, k), what="df", **wgrad_tol(N * Hh * W))

    for label, plan in plans(["y", "x", "f"]):
        rep.run("fwd " + label, lambda: fwd(plan))
    for label, plan in plans(["dx", "dy", "f"]):
        rep.run("dgrad " + label, lambda: dgrad(plan))
    for label, plan in plans(["df", "dy", "x"]):
        rep.run("wgrad " + label, lambda: wgrad(plan))
    rep.done()


# ------------------------------------------------------------------------------------------------------------ BatchNorm
BN_SHAPES = [(3, 6, 64), (3, 7, 135)]     # N, C, HW
CMAX = 8
EPS, MOM = 1e-5, 0.1


def _bn_params():
    return (det_uniform((CMAX,), "bab/gamma", 0.5, 1.5), det_uniform((CMAX,), "bab/beta", -0.3, 0.3),
            det_uniform((CMAX,), "bab/rm", -0.2, 0.2), det_uniform((CMAX,), "bab/rv", 0.5, 1.5))


def _bn_ref(ora, shape, dtype, training, act, res):
    N, C, HW = shape

    def make():
        gamma, beta, rm, rv = _bn_params()
        x = rounded(det_uniform((N, C, 1, HW), "bab/x%s" % (shape,), -2.0, 2.0), dtype)
        r = rounded(det_uniform((N, C, 1, HW), "bab/r%s" % (shape,), -1.0, 1.0), dtype) if res else None
        rm2, rv2 = rm.copy(), rv.copy()
        yb, mean, invstd = ora.bn_fwd(x, gamma, beta, rm2, rv2, training, MOM, EPS)
        pre = yb + (r if res else 0.0)
        y = np.clip(pre, 0.0, 6.0) if act else pre
        return x, r, pre, y, rm2, rv2
    return cached(("bnf", shape, dtype, training, act, res), make)


@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_forward_placed(L, ora, shape, res, act, training, dtype):
    """ofasr_bn_fwd (one call), and the same result in pieces: ofasr_bn_stats -> ofasr_bn_finalize -> ofasr_bn_act_fwd"""
    N, C, HW = shape
    gamma, beta, rm, rv = _bn_params()
    x, r, pre, y_ref, rm_ref, rv_ref = _bn_ref(ora, shape, dtype, training, act, res)
    xg = G(x, dtype).view(N, C, HW)
    rg = G(r, dtype).view(N, C, HW) if res else None
    rt, at = bn_tol(dtype)
    rep = Report("bn_fwd %s %s training=%d act=%d res=%d" % (shape, dtype, training, act, res))
    names = ["y", "x"] + (["residual"] if res else [])

    def vectors(plan):
        return (put(G(gamma), plan, "gamma", "in"), put(G(beta), plan, "beta", "in"), put(G(rm), plan, "running_mean", "in"),
                put(G(rv), plan, "running_var", "in"))

    def verify(py, prm, prv):
        assert_close(Hn(py), y_ref.reshape(N, C, HW), rt, at, "y")
        if training:
            assert_close(Hn(prm), rm_ref, 1e-5, 1e-6, "running_mean")     # test_hip_bnact.py test_bn_act_vs_oracle
            assert_close(Hn(prv), rv_ref, 1e-5, 1e-6, "running_var")
        assert np.array_equal(Hn(prm)[C:], rm[C:]) and np.array_equal(Hn(prv)[C:], rv[C:]), "running stats beyond C moved"

    def one_call(plan):
        px, py = put(xg, plan, "x", "in"), put(E((N, C, HW), dtype), plan, "y", "out")
        pr = put(rg, plan, "residual", "in") if res else None
        pg, pb, prm, prv = vectors(plan)
        pst = put(E((4 * C,)), plan, "stats", "out")
        ws = workspace(L.ofasr_bn_workspace(N, C) if training else 0, DEV)
        status_ok(L, L.ofasr_bn_fwd(ptr(px), ptr(pr), ptr(py), ptr(pg), ptr(pb), ptr(prm), ptr(prv), MOM, EPS, int(training),
                                    ptr(pst), N, C, HW, act, CODE[dtype], ptr(ws), ws.nbytes, stream()), "bn_fwd")
        finish(px, py, pr, pg, pb, pst, ws)
        check(prm, payload=not training)
        check(prv, payload=not training)
        assert not bool(pst.placement.unwritten().any()), "stats: mean | invstd | scale | shift not all written"
        verify(py, prm, prv)

    def pieces(plan):
        px, py = put(xg, plan, "x", "in"), put(E((N, C, HW), dtype), plan, "y", "out")
        pr = put(rg, plan, "residual", "in") if res else None
        pg, pb, prm, prv = vectors(plan)
        pst = put(E((4, C)), plan, "stats", "out")
        ws = workspace(L.ofasr_bn_workspace(N, C), DEV)
        if training:
            status_ok(L, L.ofasr_bn_stats(ptr(px), N, C, HW, CODE[dtype], ptr(ws), ws.nbytes, stream()), "bn_stats")
        status_ok(L, L.ofasr_bn_finalize(ptr(ws), L.ofasr_bn_partials(N, C), C, float(N * HW), ptr(pg), ptr(pb), ptr(prm),
                                         ptr(prv), MOM, EPS, int(training), ptr(pst[0]), ptr(pst[1]), ptr(pst[2]),
                                         ptr(pst[3]), stream()), "bn_finalize")
        status_ok(L, L.ofasr_bn_act_fwd(ptr(px), ptr(pr), ptr(py), ptr(pst[2]), ptr(pst[3]), ptr(pst[0]), N, C, HW, act,
                                        CODE[dtype], stream()), "bn_act_fwd")
        finish(px, py, pr, pg, pb, pst, ws)
        check(prm, payload=not training)
        check(prv, payload=not training)
        verify(py, prm, prv)

    for label, plan in plans(names):
        rep.run("bn_fwd " + label, lambda: one_call(plan))
        rep.run("stats+finalize+act_fwd " + label, lambda: pieces(plan))
    rep.done()


@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_act_bwd_placed(L, ora, shape, res, act, training, dtype):
    """ofasr_bn_act_bwd on statistics computed here in double (mean | invstd | scale | shift as the forward leaves them);
    assertions and tolerances as test_hip_bnact.py test_bn_act_vs_oracle"""
    N, C, HW = shape
    gamma, beta, rm, rv = _bn_params()
    x, r, pre, _, _, _ = _bn_ref(ora, shape, dtype, training, act, res)
    dy = cached(("bnb/dy", shape, dtype), lambda: rounded(det_uniform((N, C, 1, HW), "bab/dy%s" % (shape,)), dtype))
    xd = x.astype(np.float64)
    if training:
        mu = xd.mean(axis=(0, 2, 3))
        istd = 1.0 / np.sqrt(xd.var(axis=(0, 2, 3)) + EPS)
    else:
        mu, istd = rm[:C].astype(np.float64), 1.0 / np.sqrt(rv[:C].astype(np.float64) + EPS)
    scale = gamma[:C] * istd
    shift = beta[:C] - mu * scale
    stats = np.stack([mu, istd, scale, shift]).astype(np.float32)
    dz = dy * ((pre > 0) & (pre < 6)) if act else dy
    v4 = lambda a: a.reshape(1, C, 1, 1)
    if training:
        dx_ref, dg_ref, db_ref = ora.bn_bwd_train(dz, x, gamma, EPS)
    else:
        dx_ref = (dz * v4(gamma[:C]) * v4(istd)).astype(np.float32)
        dg_ref = (dz * (xd - v4(mu)) * v4(istd)).sum(axis=(0, 2, 3)).astype(np.float32)
        db_ref = dz.sum(axis=(0, 2, 3)).astype(np.float32)
    safe = np.ones_like(pre, bool)
    if act and dtype != F32:      # a 16-bit rounding of `pre` may flip the mask at the window's edges
        safe = (np.abs(pre) > 0.05) & (np.abs(pre - 6) > 0.05)
    safe3 = safe.reshape(N, C, HW)
    xg, dyg = G(x, dtype).view(N, C, HW), G(dy, dtype).view(N, C, HW)
    rg = G(r, dtype).view(N, C, HW) if res else None
    rt, at = bn_tol(dtype)
    rep = Report("bn_act_bwd %s %s training=%d act=%d res=%d" % (shape, dtype, training, act, res))
    names = ["dx", "dy", "x"] + (["residual", "dresidual"] if res else [])

    def run(plan):
        pdy, px, pdx = put(dyg, plan, "dy", "in"), put(xg, plan, "x", "in"), put(E((N, C, HW), dtype), plan, "dx", "out")
        pr = put(rg, plan, "residual", "in") if res else None
        pdr = put(E((N, C, HW), dtype), plan, "dresidual", "out") if res else None
        pst = put(G(stats), plan, "stats", "in")
        pdg, pdb = put(E((CMAX,)), plan, "dgamma", "out"), put(E((CMAX,)), plan, "dbeta", "out")
        ws = workspace(L.ofasr_bn_act_bwd_workspace(N, C), DEV)
        status_ok(L, L.ofasr_bn_act_bwd(ptr(pdy), ptr(px), ptr(pr), ptr(pdx), ptr(pdr), ptr(pst[2]), ptr(pst[3]), ptr(pst[0]),
                                        ptr(pst[1]), ptr(pdg), ptr(pdb), N, C, HW, act, int(training), CODE[dtype], ptr(ws),
                                        ws.nbytes, stream()), "bn_act_bwd")
        finish(pdy, px, pdx, pr, pdr, pst, pdg, pdb, ws)
        for p in (pdg, pdb):
            u = p.placement.unwritten()
            assert bool(u[C:].all()) and not bool(u[:C].any()), "%r: channels [0, C) written, the rest left alone" % p.placement
        if dtype == F32 or not training:
            assert_close(np.where(safe3, Hn(pdx), 0), np.where(safe3, dx_ref.reshape(N, C, HW), 0), 5 * rt, 5 * at, "dx")
        else:
            assert not bool(torch.isnan(pdx.float()).any()), "dx: element not written or NaN read"
        assert_close(Hn(pdg)[:C], dg_ref, 5 * rt, 20 * at, "dgamma")
        assert_close(Hn(pdb)[:C], db_ref, 5 * rt, 20 * at, "dbeta")
        if res:
            assert_close(np.where(safe3, Hn(pdr), 0), np.where(safe3, dz.reshape(N, C, HW), 0), 1e-6, 1e-6, "dresidual")

    for label, plan in plans(names):
        rep.run(label, lambda: run(plan))
    rep.done()


# ------------------------------------------------------------------------------------------------- dense conv, fp32
CF_CASES = [
    # Cin, Cout, H, W, K
    (64, 64, 6, 8, 5),     # fast window staging on / off with x's alignment
    (3, 64, 8, 8, 5),      # thin input
    (64, 3, 8, 8, 5),      # thin output
    (64, 64, 6, 8, 3),
]


@pytest.mark.parametrize("case", CF_CASES, ids=lambda c: "%dto%d_%dx%d_k%d" % c)
def test_conv2d_f32_placed(L, ora, case):
    """tolerances: test_hip_conv2d.py test_conv2d_fp32_vs_oracle; the workspace is 16-byte aligned as the header demands"""
    Cin, Cout, Hh, W, K = case
    N = 2

    def make():
        x = det_uniform((N, Cin, Hh, W), "cfab/x%s" % (case,))
        a = float(np.sqrt(3.0 / (Cin * K * K)))
        w = det_uniform((Cout, Cin, K, K), "cfab/w%s" % (case,), -a, a)
        dy = det_uniform((N, Cout, Hh, W), "cfab/dy%s" % (case,))
        dx, dw = ora.conv2d_bwd(dy, x, w)
        return x, w, dy, ora.conv2d_fwd(x, w), dx, dw
    x, w, dy, y_ref, dx_ref, dw_ref = cached(("cf", case), make)
    xg, wg, dyg = G(x), G(w), G(dy)
    scale = float(np.sqrt(Cout * K * K / max(Cin * K * K, 1)))
    rep = Report("conv2d_f32 %s" % (case,))

    def fwd(plan):
        px, pw, py = put(xg, plan, "x", "in"), put(wg, plan, "w", "in"), put(E((N, Cout, Hh, W)), plan, "y", "out")
        ws = workspace(L.ofasr_conv2d_f32_workspace(Cin, Cout, K, 0), DEV)
        status_ok(L, L.ofasr_conv2d_f32_fwd(ptr(px), ptr(pw), ptr(py), N, Cin, Cout, Hh, W, K, ptr(ws), ws.nbytes, stream()),
                  "conv2d_f32_fwd")
        finish(px, pw, py, ws)
        assert_close(Hn(py), y_ref, 5e-5, 5e-6, "y")

    def dgrad(plan):
        pdy, pw, pdx = put(dyg, plan, "dy", "in"), put(wg, plan, "w", "in"), put(E((N, Cin, Hh, W)), plan, "dx", "out")
        ws = workspace(L.ofasr_conv2d_f32_workspace(Cin, Cout, K, 1), DEV)
        status_ok(L, L.ofasr_conv2d_f32_dgrad(ptr(pdy), ptr(pw), ptr(pdx), N, Cin, Cout, Hh, W, K, ptr(ws), ws.nbytes,
                                              stream()), "conv2d_f32_dgrad")
        finish(pdy, pw, pdx, ws)
        assert_close(Hn(pdx), dx_ref, 5e-5, 5e-6 * max(1.0, scale), "dx")

    def wgrad(plan):
        pdy, px, pdw = put(dyg, plan, "dy", "in"), put(xg, plan, "x", "in"), put(E((Cout, Cin, K, K)), plan, "dw", "out")
        ws = workspace(L.ofasr_conv2d_f32_wgrad_workspace(N, Cin, Cout, Hh, W, K), DEV)
        status_ok(L, L.ofasr_conv2d_f32_wgrad(ptr(pdy), ptr(px), ptr(pdw), N, Cin, Cout, Hh, W, K, ptr(ws), ws.nbytes,
                                              stream()), "conv2d_f32_wgrad")
        finish(pdy, px, pdw, ws)
        assert_close(Hn(pdw), dw_ref, 1e-4, 2e-6 * float(np.abs(dw_ref).max()) * np.sqrt(N * Hh * W), "dw")

    for label, plan in plans(["y", "x", "w"]):
        rep.run("fwd " + label, lambda: fwd(plan))
    for label, plan in plans(["dx", "dy", "w"]):
        rep.run("dgrad " + label, lambda: dgrad(plan))
    for label, plan in plans(["dw", "dy", "x"]):
        rep.run("wgrad " + label, lambda: wgrad(plan))
    rep.done()


# ------------------------------------------------------------------------------------------------ dense conv, 16-bit
def refused(L, rc, out, what):
    """the documented refusal: OFASR_ERR_UNSUPPORTED, a message that names alignment, nothing written"""
    msg = L.ofasr_last_error_string().decode()
    assert rc == UNSUPPORTED, "%s: expected the refusal (-2), got %d (%s)" % (what, rc, msg)
    assert "aligned" in msg, "%s: the refusal does not name alignment: %r" % (what, msg)
    torch.cuda.synchronize()
    check(out)
    assert bool(out.placement.unwritten().all()), "%s: refused, yet %r was written" % (what, out.placement)


@pytest.mark.parametrize("chan", [(64, 64), (3, 64), (64, 3)], ids=lambda c: "%dto%d" % c)
@pytest.mark.parametrize("hw", [(8, 8), (6, 16)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_conv2d_16bit_placed(L, ora, chan, hw, K, dtype):
    """P0 between guards: result and bounds.  P1 / P8 (x, the output, or both): the refusal, output untouched.
    Tolerances: test_hip_conv2d.py test_conv2d_vs_oracle; the statistics partials of ofasr_conv2d_fwd_stat are folded in
    double and compared at the running-statistics tolerance of test_conv_layer_training_epilogue_statistics_vs_oracle."""
    (Cin, Cout), (Hh, W) = chan, hw
    N = 2
    case = (Cin, Cout, Hh, W, K)

    def make():
        x = rounded(det_uniform((N, Cin, Hh, W), "c16ab/x%s" % (case,)), dtype)
        a = float(np.sqrt(3.0 / (Cin * K * K)))
        w = det_uniform((Cout, Cin, K, K), "c16ab/w%s" % (case,), -a, a)
        dy = rounded(det_uniform((N, Cout, Hh, W), "c16ab/dy%s" % (case,)), dtype)
        dx, dw = ora.conv2d_bwd(dy, x, rounded(w, dtype))
        return x, w, dy, ora.conv2d_fwd(x, rounded(w, dtype)), dx, dw
    x, w, dy, y_ref, dx_ref, dw_ref = cached(("c16", case, dtype), make)
    xg, wg, dyg = G(x, dtype), G(w), G(dy, dtype)
    rt = conv16_rt(dtype)
    scale = float(np.sqrt(Cout * K * K / max(Cin * K * K, 1)))
    code = CODE[dtype]
    rep = Report("conv2d %s %s" % (case, dtype))

    def fwd(plan, stat):
        px, pw, py = put(xg, plan, "x", "in"), put(wg, plan, "w", "in"), put(E((N, Cout, Hh, W), dtype), plan, "y", "out")
        ws = workspace(L.ofasr_conv2d_workspace(Cin, Cout, K, 0), DEV)
        if stat:
            units = L.ofasr_conv2d_stat_units(N, Cin, Cout, Hh, W, K)
            pp = put(E((Cout, units, 2)), plan, "partial", "out")
            rc = L.ofasr_conv2d_fwd_stat(ptr(px), ptr(pw), ptr(py), N, Cin, Cout, Hh, W, K, code, ptr(pp), units, ptr(ws),
                                         ws.nbytes, stream())
        else:
            pp = None
            rc = L.ofasr_conv2d_fwd(ptr(px), ptr(pw), ptr(py), N, Cin, Cout, Hh, W, K, code, ptr(ws), ws.nbytes, stream())
        if plan["x"] != "P0" or plan["y"] != "P0":
            refused(L, rc, py, "conv2d_fwd" + ("_stat" if stat else ""))
            finish(px, pw, pp)
            return
        status_ok(L, rc, "conv2d_fwd")
        finish(px, pw, py, ws, pp)
        assert_close(Hn(py), y_ref, rt, rt, "y")
        if stat:
            assert not bool(pp.placement.unwritten().any()), "statistics partials not all written"
            s = Hn(pp).astype(np.float64).sum(axis=1)
            M = float(N * Hh * W)
            yd = Hn(py).astype(np.float64)          # the partials are statistics of what the kernel stored
            mean, var = s[:, 0] / M, s[:, 1] / M - (s[:, 0] / M) ** 2
            # as the running statistics a fresh BatchNorm (0, 1; momentum 0.1) would hold after this batch
            assert_close(0.1 * mean, 0.1 * yd.mean(axis=(0, 2, 3)), 1e-3, 1e-4, "running_mean from the partials")
            assert_close(0.9 + 0.1 * var * M / (M - 1), 0.9 + 0.1 * yd.var(axis=(0, 2, 3), ddof=1), 2e-3, 1e-4,
                         "running_var from the partials")

    def dgrad(plan):
        pdy, pw, pdx = put(dyg, plan, "dy", "in"), put(wg, plan, "w", "in"), put(E((N, Cin, Hh, W), dtype), plan, "dx", "out")
        ws = workspace(L.ofasr_conv2d_workspace(Cin, Cout, K, 1), DEV)
        rc = L.ofasr_conv2d_dgrad(ptr(pdy), ptr(pw), ptr(pdx), N, Cin, Cout, Hh, W, K, code, ptr(ws), ws.nbytes, stream())
        if plan["dy"] != "P0" or plan["dx"] != "P0":
            refused(L, rc, pdx, "conv2d_dgrad")
            finish(pdy, pw)
            return
        status_ok(L, rc, "conv2d_dgrad")
        finish(pdy, pw, pdx, ws)
        assert_close(Hn(pdx), dx_ref, rt, rt * max(1.0, scale), "dx")

    def wgrad(plan):
        pdy, px, pdw = put(dyg, plan, "dy", "in"), put(xg, plan, "x", "in"), put(E((Cout, Cin, K, K)), plan, "dw", "out")
        ws = workspace(L.ofasr_conv2d_wgrad_workspace(N, Cin, Cout, Hh, W, K), DEV)
        rc = L.ofasr_conv2d_wgrad(ptr(pdy), ptr(px), ptr(pdw), N, Cin, Cout, Hh, W, K, code, ptr(ws), ws.nbytes, stream())
        if plan["dy"] != "P0" or plan["x"] != "P0":
            refused(L, rc, pdw, "conv2d_wgrad")
            finish(pdy, px, ws)
            return
        status_ok(L, rc, "conv2d_wgrad")
        finish(pdy, px, pdw, ws)
        assert_close(Hn(pdw), dw_ref, 1e-3, 1e-3 * float(np.abs(dw_ref).max()), "dw")

    # the weights and dw are fp32 operands the entry points do not test: w@P1 / dw@P1 must give a result, not a refusal
    for label, plan in plans(["y", "x", "w"]):
        rep.run("fwd " + label, lambda: fwd(plan, False))
        rep.run("fwd_stat " + label, lambda: fwd(plan, True))
    for label, plan in plans(["dx", "dy", "w"]):
        rep.run("dgrad " + label, lambda: dgrad(plan))
    for label, plan in plans(["dw", "dy", "x"]):
        rep.run("wgrad " + label, lambda: wgrad(plan))
    rep.done()


# ----------------------------------------------------------------------------------------------------- pixel shuffle
PS_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


@pytest.mark.parametrize("case", [(2, 3, 5, 7, 2), (1, 4, 6, 8, 2), (2, 2, 4, 5, 3)], ids=lambda c: "%dx%dx%dx%d_r%d" % c)
@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_pixel_shuffle_placed(L, ora, case, es):
    """bit-exact (test_hip_kernels.py test_pixel_shuffle_bit_exact), shuffle and unshuffle"""
    N, C, Hh, W, r = case
    dt = PS_INT[es]
    npdt = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[es]

    def ints(shape, tag):      # byte j of an element holds value + j: a half-moved element shows
        v = det_ints(shape, tag, 0, 200).astype(np.uint8)
        return np.ascontiguousarray(np.stack([v + j for j in range(es)], axis=-1)).view(npdt).reshape(shape)
    x, z = ints((N, C * r * r, Hh, W), "psab/x%s" % (case,)), ints((N, C, Hh * r, W * r), "psab/z%s" % (case,))
    y_ref, u_ref = ora.pixel_shuffle(x, r), ora.pixel_unshuffle(z, r)
    xg, zg = torch.from_numpy(x).to(DEV), torch.from_numpy(z).to(DEV)
    rep = Report("pixel_shuffle %s es=%d" % (case, es))

    def run(plan, inverse):
        src, ref = (zg, u_ref) if inverse else (xg, y_ref)
        px = put(src, plan, "x", "in")
        py = put(torch.empty(ref.shape, dtype=dt, device=DEV), plan, "y", "out")
        fn = L.ofasr_pixel_unshuffle if inverse else L.ofasr_pixel_shuffle
        status_ok(L, fn(ptr(px), ptr(py), N, C, Hh, W, r, es, stream()), "pixel_%sshuffle" % ("un" if inverse else ""))
        finish(px, py)
        assert py.cpu().numpy().tobytes() == ref.tobytes(), "y differs from the oracle (bit-exact contract)"

    for label, plan in plans(["y", "x"]):
        rep.run("shuffle " + label, lambda: run(plan, False))
        rep.run("unshuffle " + label, lambda: run(plan, True))
    rep.done()


# --------------------------------------------------------------------------- PixelShuffle(2) + BatchNorm, conv-partials BN
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_pixel_shuffle2_bn_and_backward_placed(L, ora, dtype):
    """ofasr_pixel_shuffle2_bn, ofasr_bn_bwd_ps2 at (2, 4, 4, 8) -- x [2, 16, 4, 8] <-> y [2, 4, 8, 16]: P0 between guards
    (BatchNorm tolerances of test_hip_bnact.py, the shuffle itself exact), and the refusal at P1."""
    N, Co, Hh, W = 2, 4, 4, 8
    C = 4 * Co
    x = rounded(det_uniform((N, C, Hh, W), "ps2ab/x", -2.0, 2.0), dtype)
    dout = rounded(det_uniform((N, Co, 2 * Hh, 2 * W), "ps2ab/dout"), dtype)
    gamma, beta = det_uniform((C,), "ps2ab/g", 0.5, 1.5), det_uniform((C,), "ps2ab/b", -0.3, 0.3)
    xd = x.astype(np.float64)
    mu, istd = xd.mean(axis=(0, 2, 3)), 1.0 / np.sqrt(xd.var(axis=(0, 2, 3)) + EPS)
    scale = gamma * istd
    shift = beta - mu * scale
    stats = np.stack([mu, istd, scale, shift]).astype(np.float32)
    v4 = lambda a: a.reshape(1, C, 1, 1)
    y_ref = ora.pixel_shuffle(((xd - v4(mu)) * v4(scale) + v4(beta)).astype(np.float32), 2)
    dy = ora.pixel_unshuffle(dout, 2)
    dx_ref, dg_ref, db_ref = ora.bn_bwd_train(dy, x, gamma, EPS)
    xg, dg = G(x, dtype), G(dout, dtype)
    rt, at = bn_tol(dtype)
    rep = Report("pixel_shuffle2_bn / bn_bwd_ps2 %s" % dtype)

    def fwd(plan):
        px, pst = put(xg, plan, "x", "in"), put(G(stats), plan, "stats", "in")
        py = put(E((N, Co, 2 * Hh, 2 * W), dtype), plan, "y", "out")
        rc = L.ofasr_pixel_shuffle2_bn(ptr(px), ptr(py), ptr(pst), N, Co, Hh, W, CODE[dtype], stream())
        if plan["x"] != "P0" or plan["y"] != "P0":
            refused(L, rc, py, "pixel_shuffle2_bn")
            finish(px, pst)
            return
        status_ok(L, rc, "pixel_shuffle2_bn")
        finish(px, pst, py)
        assert_close(Hn(py), y_ref, rt, at, "y")

    def bwd(plan):
        pd, px, pst = put(dg, plan, "dout", "in"), put(xg, plan, "x", "in"), put(G(stats), plan, "stats", "in")
        pdx = put(E((N, C, Hh, W), dtype), plan, "dx", "out")
        pdg, pdb = put(E((C,)), plan, "dgamma", "out"), put(E((C,)), plan, "dbeta", "out")
        ws = workspace(L.ofasr_bn_bwd_ps2_workspace(N, C), DEV)
        rc = L.ofasr_bn_bwd_ps2(ptr(pd), ptr(px), ptr(pdx), ptr(pst[2]), ptr(pst[0]), ptr(pst[1]), ptr(pdg), ptr(pdb), N, C, Hh,
                                W, 1, CODE[dtype], ptr(ws), ws.nbytes, stream())
        if plan["dout"] != "P0" or plan["x"] != "P0" or plan["dx"] != "P0":
            refused(L, rc, pdx, "bn_bwd_ps2")
            finish(pd, px, pst, pdg, pdb, ws)
            assert bool(pdg.placement.unwritten().all()) and bool(pdb.placement.unwritten().all())
            return
        status_ok(L, rc, "bn_bwd_ps2")
        finish(pd, px, pst, pdx, pdg, pdb, ws)
        assert not bool(torch.isnan(pdx.float()).any()), "dx: element not written or NaN read"
        assert_close(Hn(pdg), dg_ref, 5 * rt, 20 * at, "dgamma")       # test_hip_bnact.py test_bn_act_vs_oracle
        assert_close(Hn(pdb), db_ref, 5 * rt, 20 * at, "dbeta")

    for label, plan in plans(["y", "x"]):
        rep.run("pixel_shuffle2_bn " + label, lambda: fwd(plan))
    for label, plan in plans(["dx", "dout", "x"]):
        rep.run("bn_bwd_ps2 " + label, lambda: bwd(plan))
    rep.done()


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bn_fwd_cp_placed(L, ora, act, dtype):
    """ofasr_bn_fwd_cp at (2, 4, 4, 8) on float (sum, sum of squares) partials made here, two units per channel"""
    N, C, Hh, W = 2, 4, 4, 8
    HW = Hh * W
    gamma, beta, rm, rv = [a[:C].copy() for a in _bn_params()]
    x = rounded(det_uniform((N, C, 1, HW), "cpab/x", -2.0, 2.0), dtype)
    rm_ref, rv_ref = rm.copy(), rv.copy()
    yb, _, _ = ora.bn_fwd(x, gamma, beta, rm_ref, rv_ref, True, MOM, EPS)
    y_ref = np.clip(yb, 0.0, 6.0) if act else yb
    xd = x.astype(np.float64).reshape(N, C, HW)
    partial = np.stack([np.stack([xd[n].sum(axis=1), (xd[n] ** 2).sum(axis=1)], axis=-1) for n in range(N)], axis=1)
    partial = partial.astype(np.float32)      # [C][units = N][2]
    rt, at = bn_tol(dtype)
    rep = Report("bn_fwd_cp %s act=%d" % (dtype, act))

    def run(plan):
        px, py = put(G(x, dtype).view(N, C, HW), plan, "x", "in"), put(E((N, C, HW), dtype), plan, "y", "out")
        pp = put(G(partial), plan, "partial", "in")
        pg, pb = put(G(gamma), plan, "gamma", "in"), put(G(beta), plan, "beta", "in")
        prm, prv = put(G(rm), plan, "running_mean", "in"), put(G(rv), plan, "running_var", "in")
        pst = put(E((4 * C,)), plan, "stats", "out")
        status_ok(L, L.ofasr_bn_fwd_cp(ptr(px), None, ptr(py), ptr(pp), N, ptr(pg), ptr(pb), ptr(prm), ptr(prv), MOM, EPS, 1,
                                       ptr(pst), N, C, HW, act, CODE[dtype], stream()), "bn_fwd_cp")
        finish(px, py, pp, pg, pb, pst)
        check(prm, payload=False)
        check(prv, payload=False)
        assert not bool(pst.placement.unwritten().any())
        assert_close(Hn(py), y_ref.reshape(N, C, HW), rt, at, "y")
        # float partials: the running-statistics tolerance of test_conv_layer_training_epilogue_statistics_vs_oracle
        assert_close(Hn(prm), rm_ref, 1e-3, 1e-4, "running_mean")
        assert_close(Hn(prv), rv_ref, 2e-3, 1e-4, "running_var")

    for label, plan in plans(["y", "x"]):
        rep.run(label, lambda: run(plan))
    rep.done()


# --------------------------------------------------------------------------------------------------------------- add
@pytest.mark.parametrize("n", [1, 7, 1024, 1031])
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_placed(L, n, dtype):
    """ofasr_add: the same bits as ATen's add (ops.skip_add's contract, test_hip_self_ensemble.py)"""
    a = torch.from_numpy(det_uniform((n,), "addab/a%d" % n)).to(dtype)
    b = torch.from_numpy(det_uniform((n,), "addab/b%d" % n)).to(dtype)
    ref = a + b
    rep = Report("add n=%d %s" % (n, dtype))

    def run(plan):
        pa, pb, py = put(a.to(DEV), plan, "a", "in"), put(b.to(DEV), plan, "b", "in"), put(E((n,), dtype), plan, "y", "out")
        status_ok(L, L.ofasr_add(ptr(pa), ptr(pb), ptr(py), n, CODE[dtype], stream()), "ofasr_add")
        finish(pa, pb, py)
        assert torch.equal(py.cpu().view(torch.int16 if dtype != F32 else torch.int32),
                           ref.view(torch.int16 if dtype != F32 else torch.int32)), "y differs from ATen's add"

    for label, plan in plans(["y", "a", "b"]):
        rep.run(label, lambda: run(plan))
    rep.done()


# --------------------------------------------------------------------------------------------------- kernel transform
@pytest.mark.parametrize("K", [7, 5, 3])
@pytest.mark.parametrize("transform", [0, 1])
def test_ktransform_placed(L, ora, K, transform):
    """C = 5 rows of a Cmax = 8 parameter, chain 7 -> 5 -> 3.  Tolerances: test_hip_kernels.py test_ktransform_golden.
    dw_max rows >= C are the caller's: they must keep the canary."""
    C, Cm = 5, 8
    chain = [s for s in (7, 5, 3) if s >= K]
    n = len(chain) - 1
    w7 = det_uniform((Cm, 1, 7, 7), "ktab/w7", -0.3, 0.3)
    mats = {"7to5": (np.eye(25, dtype=np.float32) + det_uniform((25, 25), "ktab/m75", -0.2, 0.2)),
            "5to3": (np.eye(9, dtype=np.float32) + det_uniform((9, 9), "ktab/m53", -0.2, 0.2))}
    names = ["%dto%d" % (chain[s], chain[s + 1]) for s in range(n)] if transform else []
    f_ref = ora.ktransform_fwd(w7, C, K, [3, 5, 7], mats if transform else None)
    df = det_uniform(f_ref.shape, "ktab/df%d" % K)
    dw_ref, dm_ref = ora.ktransform_bwd(df, w7, C, K, [3, 5, 7], mats if transform else None)
    ks = (ctypes.c_int * len(chain))(*chain)
    rep = Report("ktransform K=%d transform=%d" % (K, transform))
    operands = ["w_max"] + names

    def parr(ts):
        return (ctypes.c_void_p * max(n, 1))(*([t.data_ptr() for t in ts] if ts else [None] * max(n, 1)))

    def fwd(plan):
        pw = put(G(w7).view(Cm, 7, 7), plan, "w_max", "in")
        pm = [put(G(mats[m]), plan, m, "in") for m in names]
        pf = put(E((C, K, K)), plan, "f", "out")
        status_ok(L, L.ofasr_ktransform_fwd(ptr(pw), ks, n, parr(pm), transform, ptr(pf), C, stream()), "ktransform_fwd")
        finish(pw, pf, *pm)
        assert_close(Hn(pf), f_ref.reshape(C, K, K), 2e-5, 2e-6, "f")

    def bwd(plan):
        pw = put(G(w7).view(Cm, 7, 7), plan, "w_max", "in")
        pm = [put(G(mats[m]), plan, m, "in") for m in names]
        pdf = put(G(df).view(C, K, K), plan, "df", "in")
        pdw = put(E((Cm, 7, 7)), plan, "dw_max", "out")
        pdm = [put(E(mats[m].shape), plan, "d" + m, "out") for m in names]
        ws = workspace(L.ofasr_ktransform_bwd_workspace(ks, n, C) if names else 0, DEV)
        status_ok(L, L.ofasr_ktransform_bwd(ptr(pw), ks, n, parr(pm), transform, ptr(pdf), ptr(pdw), parr(pdm), C, ptr(ws),
                                            ws.nbytes, stream()), "ktransform_bwd")
        finish(pw, pdf, pdw, ws, *(pm + pdm))
        u = pdw.placement.unwritten()
        assert bool(u[C:].all()), "dw_max rows >= C were written"
        assert not bool(u[:C].any()), "dw_max rows < C not fully written"
        assert_close(Hn(pdw)[:C], dw_ref.reshape(Cm, 7, 7)[:C], 2e-5, 2e-5, "dw_max")
        for m, p in zip(names, pdm):
            assert_close(Hn(p), dm_ref[m], 2e-5, 2e-5, "d" + m)

    for label, plan in plans(["f"] + operands):
        rep.run("fwd " + label, lambda: fwd(plan))
    for label, plan in plans(["dw_max", "df"] + operands + ["d" + m for m in names]):
        rep.run("bwd " + label, lambda: bwd(plan))
    rep.done()
