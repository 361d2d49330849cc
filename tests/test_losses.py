"""The training losses on the host: losses.py, the single statement of what csrc/loss.hip computes, against torch autograd
in fp64; the C ABI of the fused loss (ofasr_sr_loss_*): argument validation and the workspace query, without a GPU.

Bounds.  The statement rounds every step to fp32; the reference is exact up to fp64.  Per element the gradient may be off
by k * 2^-24 * (|ga rho'(d)| + |gb rho'(e)|) plus half an ulp of the output dtype, k counted from the statement:
    mse          5: d, ca, ga, the product, the final add (x + x is exact)
    l1           4: ca, ga, the product, the final add (the sign is exact)
    charbonnier  8: with u = x^2 / (x^2 + eps^2): d reaches rho' with weight 1 - u, x * x with u / 2, the cast of eps^2
                 with (1 - u) / 2, their sum with 1 / 2 (all three sit under the square root), then the sqrt, the
                 division, ca, ga, the product and the final add: 8 - u
The value: the fp64 sum of the statement's own fp32 terms may differ from torch's fp64 sum of the same terms by the
summation order alone, M * 2^-52 relative; against the all-fp64 loss it carries the terms' roundings on top, 3 * 2^-24
relative for every kind (mse: twice d's and the product's; l1: d's; charbonnier: at most d's, half of each of the three
under the root, and the root's)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import amd

KINDS = ("mse", "l1", "charbonnier")
K_GRAD = {"mse": 5, "l1": 4, "charbonnier": 8}
EPS = 1e-3
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
PREC = {"f32": (24, -126), "f16": (11, -14), "bf16": (8, -126)}     # significand bits, smallest normal exponent


def half_ulp(v, dtype):
    """half an ulp of `dtype` at the fp64 values v"""
    p, emin = PREC[dtype]
    _, e = np.frexp(np.abs(v))                   # |v| = m * 2^e, 0.5 <= m < 1
    return np.ldexp(1.0, np.maximum(e - 1, emin) - p)


def operands(shape, dtype, seed):
    """(o, t, s) as fp32 numpy arrays; o holds values of `dtype`.  A few elements of t and s equal o's."""
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(shape, generator=g).mul_(1.2).sub_(0.1).to(TDT[dtype]).float()
    t = torch.rand(shape, generator=g)
    s = (o + 0.05 * torch.randn(shape, generator=g)).float()
    t.view(-1)[::7] = o.view(-1)[::7]
    s.view(-1)[::11] = o.view(-1)[::11]
    return o.numpy(), t.numpy(), s.numpy()


def rho64(x, kind):
    if kind == "mse":
        return x * x
    if kind == "l1":
        return x.abs()
    return torch.sqrt(x * x + EPS * EPS)


def reference64(o, t, s, kind, w_main, w_kd, g):
    """(loss, gradient, |ga rho'(d)| + |gb rho'(e)|) by torch autograd in fp64"""
    od = torch.from_numpy(o).double().requires_grad_(True)
    main = rho64(od - torch.from_numpy(t).double(), kind).mean()
    ga, = torch.autograd.grad(w_main * main * g, od, retain_graph=True)
    mag = ga.abs()
    loss = w_main * main
    if s is not None:
        kd = rho64(od - torch.from_numpy(s).double(), kind).mean()
        gb, = torch.autograd.grad(w_kd * kd * g, od, retain_graph=True)
        mag = mag + gb.abs()
        loss = loss + w_kd * kd
    grad, = torch.autograd.grad(loss * g, od)
    return float(loss.detach()), grad.numpy(), mag.numpy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_s", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_statement_against_fp64_autograd(kind, with_s, dtype):
    losses = amd("losses")
    shape = (2, 3, 5, 7)
    o, t, s = operands(shape, dtype, 3)
    s = s if with_s else None
    w_main, w_kd = (0.75, 0.5) if with_s else (1.0, 0.0)
    M = o.size
    for g in (1.0, 3.0):
        want_l, want_g, mag = reference64(o, t, s, kind, w_main, w_kd, g)
        got = losses.sr_loss_grad_np(o, t, s, kind, EPS, w_main, w_kd, g=g, dtype=dtype)
        assert got.dtype == np.float32 and got.shape == shape
        assert np.array_equal(got, losses.round_to(got, dtype))          # values of the output dtype
        bound = K_GRAD[kind] * 2.0 ** -24 * mag + half_ulp(want_g, dtype)
        err = np.abs(got.astype(np.float64) - want_g)
        assert (err <= bound).all(), (kind, with_s, dtype, g, float((err / bound).max()))
    r = losses.sr_loss_np(o, t, s, kind, EPS, w_main, w_kd)
    # the statement's fp32 terms, summed by torch in fp64: the summation order alone
    sm = float(torch.from_numpy(losses.rho(o - t, kind, EPS)).double().sum())
    sk = float(torch.from_numpy(losses.rho(o - s, kind, EPS)).double().sum()) if with_s else 0.0
    assert abs(r["sum_main"] - sm) <= M * 2.0 ** -52 * sm and abs(r["sum_kd"] - sk) <= M * 2.0 ** -52 * sk
    same_terms = w_main * sm / M + w_kd * sk / M
    assert abs(r["loss"] - same_terms) <= M * 2.0 ** -52 * same_terms
    assert abs(r["loss"] - want_l) <= (3 * 2.0 ** -24 + M * 2.0 ** -52) * want_l
    assert r["loss_f32"] == np.float32(r["loss"]) and isinstance(r["loss_f32"], np.float32)


def test_sign_of_zero_and_equal_operands():
    losses = amd("losses")
    z = np.array([0.0, -0.0, 2.0, -3.0, np.nan], dtype=np.float32)
    assert losses.drho(z, "l1").tolist() == [0.0, 0.0, 1.0, -1.0, 0.0]
    o, _, _ = operands((1, 3, 4, 6), "f32", 5)
    for dtype in ("f32", "bf16", "f16"):
        g = losses.sr_loss_grad_np(o, o.copy(), o.copy(), "l1", w_main=1.0, w_kd=0.5, g=3.0, dtype=dtype)
        assert not g.any()
    r = losses.sr_loss_np(o, o.copy(), kind="charbonnier", eps=EPS)
    rho0 = losses.rho(np.zeros(1, np.float32), "charbonnier", EPS)[0]
    assert abs(float(rho0) - EPS) <= EPS * 2.0 ** -23              # sqrt(fp32(eps^2)): eps to an fp32 ulp
    assert abs(r["sum_main"] - o.size * float(rho0)) <= o.size * 2.0 ** -52 * r["sum_main"]
    assert abs(r["loss"] - EPS) <= EPS * 2.0 ** -22 and r["y_sse"] == 0 and r["psnr"] == float("inf")
    assert not losses.sr_loss_grad_np(o, o.copy(), kind="charbonnier").any()
    assert not losses.sr_loss_grad_np(o, o.copy(), kind="mse").any()


def test_y_sse_is_the_exact_luma_error_of_the_quantised_images():
    losses, utils = amd("losses"), amd("utils")
    rng = np.random.RandomState(11)
    o = rng.uniform(-0.2, 1.2, (3, 3, 9, 13)).astype(np.float32)           # values the quantiser clamps
    t = (rng.randint(0, 256, o.shape) / 255.0).astype(np.float32)
    o[0, :, 0, :4] = np.float32(0.5 / 255.0)                                # a rounding tie of the quantiser

    def luma(x):
        q = np.rint(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
        return utils.y_exact(np.transpose(q, (0, 2, 3, 1))).astype(np.int64)
    want = int(((luma(o) - luma(t)) ** 2).sum())
    assert want > 0
    r = losses.sr_loss_np(o, t, kind="l1", psnr_count=losses.mosaic_count(3, 9, 13))
    assert r["y_sse"] == want == losses.y_sse(o, t)
    assert r["psnr"] == utils.psnr_from_sse(want, losses.mosaic_count(3, 9, 13))
    assert losses.sr_loss_np(o, t, kind="l1")["psnr"] == utils.psnr_from_sse(want, 3 * 9 * 13)
    # the count is the one utils.psnr_y_device divides by: the same PSNR wherever no luma is a rounding tie
    dev = float(utils.psnr_y_device(torch.from_numpy(o), torch.from_numpy(t)))
    assert abs(dev - r["psnr"]) < 0.05
    assert losses.mosaic_count(1, 9, 13) == 9 * 13 and losses.mosaic_count(16, 256, 256) == (258 * 4 + 2) ** 2


@pytest.mark.parametrize("kd", [0.5, 1.0, 3.0])
def test_weight_pairs_are_the_two_kd_formulas(kd):
    losses = amd("losses")
    F = torch.nn.functional
    o, t, s = operands((2, 3, 6, 5), "f32", 9)
    od, td, sd = (torch.from_numpy(x).double() for x in (o, t, s))
    teacher = float(kd * F.mse_loss(od, sd) + F.mse_loss(od, td))                      # SRRunManager.train_one_epoch
    shrinking = float((kd * F.mse_loss(od, sd) + F.mse_loss(od, td)) * (2 / (kd + 1)))   # progressive_shrinking
    assert losses.kd_weights(kd, False) == (1.0, kd)
    assert losses.kd_weights(kd, True) == (2.0 / (kd + 1.0), 2.0 * kd / (kd + 1.0))
    for want, shr in ((teacher, False), (shrinking, True)):
        w_main, w_kd = losses.kd_weights(kd, shr)
        got = losses.sr_loss_np(o, t, s, "mse", w_main=w_main, w_kd=w_kd)["loss"]
        assert abs(got - want) <= 4 * 2.0 ** -24 * want                    # the fp32 terms (3) and the weights' product


# ---------------------------------------------------------------------------------------------- C ABI, ops
def test_workspace_query_is_host_only():
    L = amd("_C").lib()
    assert L.ofasr_sr_loss_workspace(0) == 0 and L.ofasr_sr_loss_workspace(-5) == 0
    one = L.ofasr_sr_loss_workspace(1)
    assert 0 < one <= 64 and L.ofasr_sr_loss_workspace(3 * 8 * 8) == one       # fewer elements than one workgroup
    assert L.ofasr_sr_loss_workspace(3 * 3 * 64 * 64) == 6 * one               # 36864 elements: 6 workgroups
    big = L.ofasr_sr_loss_workspace(1 << 40)
    assert one < big <= (1 << 20) and L.ofasr_sr_loss_workspace(1 << 50) == big


def test_argument_validation_without_gpu():
    C = amd("_C")
    L = C.lib()
    err = L.ofasr_last_error_string
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    n = 4096

    def fwd(o=p, fo=0, t=p, ft=0, s=None, fs=0, N=1, H=8, W=8, kind=1, eps=1e-3, count=64.0, res=p, ws=p, wsn=n):
        return L.ofasr_sr_loss_fwd(o, fo, t, ft, s, fs, N, H, W, kind, eps, 1.0, 0.0, count, res, ws, wsn, None)

    def bwd(o=p, fo=0, t=p, ft=0, s=None, fs=0, g=p, N=1, H=8, W=8, kind=1, eps=1e-3, grad=p):
        return L.ofasr_sr_loss_bwd(o, fo, t, ft, s, fs, g, N, H, W, kind, eps, 1.0, 0.0, grad, None)

    assert fwd(o=None) == -1 and b"null" in err()
    assert fwd(t=None) == -1 and b"null" in err()
    assert fwd(res=None) == -1 and b"null" in err()
    assert fwd(kind=3) == -1 and b"kind" in err()
    assert fwd(kind=-1) == -1 and b"kind" in err()
    assert fwd(fo=C.U8_HWC) == -1 and b"f32" in err()
    assert fwd(s=p, fs=5) == -1 and b"f32" in err()
    assert fwd(N=0) == -1 and fwd(H=-1) == -1
    assert fwd(kind=2, eps=0.0) == -1 and b"eps" in err()
    assert fwd(kind=2, eps=float("nan")) == -1 and b"eps" in err()
    assert fwd(count=0.0) == -1 and b"psnr_count" in err()
    assert fwd(N=1 << 30, H=1 << 10, W=1 << 10) == -2
    assert fwd(ws=None, wsn=0) == -3 and b"workspace" in err()
    assert fwd(N=3, H=64, W=64, wsn=32) == -3
    assert bwd(o=None) == -1 and b"null" in err()
    assert bwd(g=None) == -1 and b"null" in err()
    assert bwd(grad=None) == -1 and b"null" in err()
    assert bwd(kind=7) == -1 and b"kind" in err()
    assert bwd(ft=4) == -1 and b"f32" in err()
    assert bwd(kind=2, eps=-1e-3) == -1 and b"eps" in err()
    assert bwd(W=0) == -1


def test_ops_sr_loss_refusals():
    ops, C = amd("ops"), amd("_C")
    a = torch.zeros(1, 3, 8, 8)
    with pytest.raises(C.OfasrError, match="no CPU fallback"):
        ops.sr_loss(a, a)
    with pytest.raises(C.OfasrError, match="unknown kind"):
        ops.sr_loss(a, a, kind="huber")
    with pytest.raises(C.OfasrError, match="target is"):
        ops.sr_loss(a, torch.zeros(1, 3, 8, 9))
    with pytest.raises(C.OfasrError, match="soft is"):
        ops.sr_loss(a, a, torch.zeros(2, 3, 8, 8))
    with pytest.raises(C.OfasrError, match=r"\[N, 3, H, W\]"):
        ops.sr_loss(torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8))
