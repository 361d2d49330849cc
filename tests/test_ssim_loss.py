"""The SSIM term of the training loss on the host: losses.ssim_np / sr_loss_ssim_np / sr_loss_ssim_grad_np, the statement of
what the SSIM kernels of csrc/loss.hip compute, against torch fp64 (a grouped conv2d with the 11 x 11 window, autograd);
the C ABI of ofasr_sr_loss_ssim_* and ops.sr_loss(ssim=): argument validation and the workspace query, without a GPU.

Bounds.  Statement and reference are both fp64 and differ by the order of their sums: |dS| <= 1e-12, and the gradient
within 1e-9 * max|grad| (the margin tests/test_quality.py gives the SSIM metric) plus one fp32 ulp of the element, since
the statement hands out fp32 values."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import amd

SHAPE = (2, 3, 13, 45)
KINDS = ("mse", "l1", "charbonnier")


def operands(shape=SHAPE, seed=5):
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(shape, generator=g).mul_(1.2).sub_(0.1)
    t = torch.rand(shape, generator=g)
    s = o + 0.05 * torch.randn(shape, generator=g)
    return o.numpy(), t.numpy(), s.numpy()


def ssim64(o, t):
    """mean SSIM per colour plane of fp64 torch tensors: the 11 x 11 window as one grouped conv2d"""
    losses = amd("losses")
    g = torch.from_numpy(losses.ssim_window())
    w = (g[:, None] * g[None, :])[None, None].repeat(3, 1, 1, 1)
    conv = lambda x: torch.nn.functional.conv2d(x, w, groups=3)
    m1, m2 = conv(o), conv(t)
    s1, s2, s12 = conv(o * o) - m1 * m1, conv(t * t) - m2 * m2, conv(o * t) - m1 * m2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * m1 * m2 + c1) * (2 * s12 + c2)) / ((m1 * m1 + m2 * m2 + c1) * (s1 + s2 + c2))).mean()


def ulp32(v):
    _, e = np.frexp(np.abs(v).astype(np.float64))
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 23)


def test_ssim_np_against_fp64_conv2d():
    losses = amd("losses")
    o, t, _ = operands()
    S, K = losses.ssim_np(o, t)
    want = float(ssim64(torch.from_numpy(o).double(), torch.from_numpy(t).double()))
    print("S", S, "torch", want, "diff", abs(S - want))
    assert K == 2 * 3 * 3 * 35 and -1.0 < S < 1.0
    assert abs(S - want) <= 1e-12


def test_gradient_against_fp64_autograd():
    losses = amd("losses")
    o, t, _ = operands()
    od = torch.from_numpy(o).double().requires_grad_(True)
    (1.0 - ssim64(od, torch.from_numpy(t).double())).backward()
    want = od.grad.numpy()
    for kind in KINDS:          # alpha = 1: the pixel term has weight 0 whatever its kind
        got = losses.sr_loss_ssim_grad_np(o, t, None, kind, w_main=1.0, alpha=1.0, g=1.0, dtype="f32")
        assert got.dtype == np.float32 and got.shape == SHAPE
        err = np.abs(got.astype(np.float64) - want)
        bound = 1e-9 * np.abs(want).max() + ulp32(want)
        print(kind, "max err", err.max(), "max |grad|", np.abs(want).max())
        assert (err <= bound).all(), float((err / bound).max())
    raw = losses.ssim_grad_np(o, t)
    assert np.abs(-raw - want).max() <= 1e-9 * np.abs(want).max()


def test_equal_operands_score_exactly_one():
    losses = amd("losses")
    o, _, _ = operands((1, 3, 11, 17))
    assert losses.ssim_np(o, o.copy()) == (1.0, 3 * 7)
    r = losses.sr_loss_ssim_np(o, o.copy(), kind="l1", alpha=1.0)
    assert r["ssim"] == 1.0 and r["loss"] == 0.0 and r["ssim_sum"] == 21.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alpha", [0.25, 1.0])
def test_the_two_weights_scale_as_stated(kind, alpha):
    losses = amd("losses")
    o, t, s = operands()
    w_main, w_kd = 0.75, 0.5
    plain = losses.sr_loss_np(o, t, s, kind, w_main=w_main, w_kd=w_kd)
    S, K = losses.ssim_np(o, t)
    r = losses.sr_loss_ssim_np(o, t, s, kind, w_main=w_main, w_kd=w_kd, alpha=alpha)
    assert r["ssim"] == S and r["loss_pix"] == plain["loss"] and abs(r["ssim_sum"] - S * K) <= 1e-12 * K
    assert r["loss"] == (1.0 - alpha) * plain["loss"] + alpha * (1.0 - S)
    assert r["loss_f32"] == np.float32(r["loss"]) and isinstance(r["loss_f32"], np.float32)
    for key in ("sum_main", "sum_kd", "y_sse", "psnr"):
        assert r[key] == plain[key]
    # the gradient: the pixel addend is today's element for the weights scaled by (1 - alpha), the SSIM addend is
    # -alpha * g * dS/do, and the two meet in one fp32 addition
    for g in (1.0, 3.0):
        pix, add = losses.sr_loss_ssim_parts_np(o, t, s, kind, w_main=w_main, w_kd=w_kd, g=g, alpha=alpha)
        want_pix = losses.sr_loss_grad_np(o, t, s, kind, w_main=(1.0 - alpha) * w_main, w_kd=(1.0 - alpha) * w_kd, g=g)
        assert np.array_equal(pix, want_pix)
        if alpha == 1.0:
            assert not pix.any()
        assert np.array_equal(add, (g * -alpha * losses.ssim_grad_np(o, t)).astype(np.float32))
        for dtype in ("f32", "bf16", "f16"):
            got = losses.sr_loss_ssim_grad_np(o, t, s, kind, w_main=w_main, w_kd=w_kd, g=g, dtype=dtype, alpha=alpha)
            assert np.array_equal(got, losses.round_to(pix + add, dtype))


def test_statement_refusals():
    losses = amd("losses")
    o, t, _ = operands((1, 3, 10, 12))
    with pytest.raises(ValueError, match="10x12"):
        losses.ssim_np(o, t)
    o, t, _ = operands((1, 3, 11, 11))
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="SSIM weight"):
            losses.sr_loss_ssim_np(o, t, alpha=bad)


# ---------------------------------------------------------------------------------------------- C ABI, ops
def test_workspace_query_is_host_only():
    L = amd("_C").lib()
    q = L.ofasr_sr_loss_ssim_workspace
    for bad in ((0, 16, 16), (-1, 16, 16), (1, 10, 16), (1, 16, 10), (1, 0, 0), (1 << 30, 1 << 10, 1 << 10)):
        assert q(*bad) == 0, bad
    plain = L.ofasr_sr_loss_workspace
    one = q(1, 11, 11) - plain(3 * 11 * 11)
    assert one == 3 * 8                                    # one window per plane: one fp64 partial per plane
    # monotone in the number of 16 x 16 tiles of positions
    assert q(1, 26, 26) - plain(3 * 26 * 26) == one
    assert q(1, 27, 26) - plain(3 * 27 * 26) == 2 * one
    assert q(1, 27, 27) - plain(3 * 27 * 27) == 4 * one
    assert q(2, 27, 27) - plain(2 * 3 * 27 * 27) == 8 * one
    last = 0
    for side in (11, 27, 43, 64, 256):       # 1, 2, 3, 4, 16 tiles per side
        n = q(3, side, side)
        assert n > last and n % 8 == 0
        last = n


def test_argument_validation_without_gpu():
    C = amd("_C")
    L = C.lib()
    err = L.ofasr_last_error_string
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.cast(buf, ctypes.c_void_p)
    base = (p.value + 15) // 16 * 16
    p = ctypes.c_void_p(base)
    n = 4096

    def fwd(o=p, fo=0, t=p, ft=0, s=None, fs=0, N=1, H=16, W=16, kind=1, eps=1e-3, count=64.0, alpha=0.2, res=p, ws=p,
            wsn=n):
        return L.ofasr_sr_loss_ssim_fwd(o, fo, t, ft, s, fs, N, H, W, kind, eps, 1.0, 0.0, count, alpha, res, ws, wsn, None)

    def bwd(o=p, fo=0, t=p, ft=0, s=None, fs=0, g=p, N=1, H=16, W=16, kind=1, eps=1e-3, alpha=0.2, grad=p):
        return L.ofasr_sr_loss_ssim_bwd(o, fo, t, ft, s, fs, g, N, H, W, kind, eps, 1.0, 0.0, alpha, grad, None)

    for call in (fwd, bwd):
        assert call(o=None) == -1 and b"null" in err()
        assert call(t=None) == -1 and b"null" in err()
        assert call(fo=C.U8_HWC) == -1 and b"f32" in err()
        assert call(ft=4) == -1 and b"f32" in err()
        assert call(s=p, fs=5) == -1 and b"f32" in err()
        assert call(kind=3) == -1 and b"kind" in err()
        assert call(kind=2, eps=0.0) == -1 and b"eps" in err()
        assert call(N=0) == -1 and call(H=-1) == -1
        for alpha in (0.0, -0.2, 1.0001, float("nan"), float("inf")):
            assert call(alpha=alpha) == -1 and b"alpha" in err(), alpha
        assert call(H=10) == -1 and b"10x16" in err() and b"11-pixel" in err()
        assert call(W=10) == -1 and b"16x10" in err()
        assert call(N=1 << 30, H=1 << 10, W=1 << 10) == -2
    assert fwd(res=None) == -1 and b"null" in err()
    assert fwd(count=0.0) == -1 and b"psnr_count" in err()
    assert fwd(res=ctypes.c_void_p(base + 4)) == -1 and b"8-byte" in err()
    assert fwd(ws=None, wsn=0) == -3 and b"workspace" in err()
    assert fwd(ws=ctypes.c_void_p(base + 8)) == -3 and b"16-byte" in err()
    need = L.ofasr_sr_loss_ssim_workspace(3, 64, 64)
    assert fwd(N=3, H=64, W=64, wsn=need - 1) == -3 and str(need).encode() in err()
    assert bwd(g=None) == -1 and b"null" in err()
    assert bwd(grad=None) == -1 and b"null" in err()
    assert bwd(g=ctypes.c_void_p(base + 2)) == -1 and b"4-byte" in err()


def test_ops_sr_loss_refusals():
    ops, C = amd("ops"), amd("_C")
    a = torch.zeros(1, 3, 16, 16)
    with pytest.raises(C.OfasrError, match="10x16"):
        ops.sr_loss(torch.zeros(1, 3, 10, 16), torch.zeros(1, 3, 10, 16), ssim=0.2)
    with pytest.raises(C.OfasrError, match=r"\[0, 1\]"):
        ops.sr_loss(a, a, ssim=-0.1)
    with pytest.raises(C.OfasrError, match=r"\[0, 1\]"):
        ops.sr_loss(a, a, ssim=1.5)
    with pytest.raises(C.OfasrError, match=r"fp64 \[8\]"):
        ops.sr_loss(a, a, ssim=0.2, out=torch.zeros(6, dtype=torch.float64))
    with pytest.raises(C.OfasrError, match="no CPU fallback"):
        ops.sr_loss(a, a, ssim=0.2)
    assert (ops.SR_LOSS_SSIM_SUM, ops.SR_LOSS_SSIM) == (6, 7)


def test_run_manager_and_cli_rules_need_no_gpu():
    losses = amd("losses")

    class Ap(object):
        def error(self, msg):
            raise SystemExit(msg)
    assert losses.check_cli(Ap(), "l1", None) == losses.DEFAULT_EPS               # the callers of before
    assert losses.check_cli(Ap(), "l1", None, 0.2) == losses.DEFAULT_EPS
    assert losses.check_cli(Ap(), "charbonnier", 1e-2, 1.0) == 1e-2
    assert losses.check_cli(Ap(), "reference", None, 0.0) == losses.DEFAULT_EPS
    for loss, a in (("reference", 0.2), ("l1", 1.5), ("l1", -0.1), ("mse", float("nan"))):
        with pytest.raises(SystemExit, match="--loss-ssim"):
            losses.check_cli(Ap(), loss, None, a)
