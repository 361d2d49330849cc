"""The training losses of the SR path: the single host statement (numpy) of what csrc/loss.hip computes on the GPU
(ops.sr_loss; C ABI ofasr_sr_loss_fwd / ofasr_sr_loss_bwd).

Operands: o (network output), t (HR batch), s (teacher output, optional), all [N, 3, H, W] and read as fp32; M is the
element count, d = o - t and e = o - s in fp32.

    kind          rho(x)                rho'(x)
    mse           x * x                 x + x
    l1            |x|                   1, -1 or 0 by the sign of x (0 at 0: torch's rule; 0 at NaN)
    charbonnier   sqrt(x * x + eps2)    x / sqrt(x * x + eps2)

eps2 = fp32(eps * eps), the product formed in fp64.  Every step above is ONE fp32 operation -- sqrt and the division
correctly rounded, nothing contracted into a fused multiply-add.

    L = w_main * sum rho(d) / M + w_kd * sum rho(e) / M        the terms fp32, the sums and this line fp64

and the value autograd sees is fp32(L).  Gradient with respect to o alone: ca = fp32(w_main / M), cb = fp32(w_kd / M)
(the quotients in fp64), ga = ca * g and gb = cb * g in fp32 for the incoming gradient g, and per element

    fl(ga * rho'(d))                              without s
    fl(fl(ga * rho'(d)) + fl(gb * rho'(e)))       with s

rounded to nearest even into o's dtype.  The logged metric is the exact integer squared error of the two luma images
(utils.y_exact on the images quantised as utils.tensor2img_np does) and utils.psnr_from_sse of it over a pixel count
the caller passes; the training loops pass mosaic_count, the count utils.psnr_y_device divides by.
"""
import math

import numpy as np

from . import utils

KINDS = ("mse", "l1", "charbonnier")     # index = the OFASR_LOSS_* code of include/ofasr.h
DEFAULT_EPS = 1e-3
_F32 = np.float32


def eps2_f32(eps):
    return _F32(float(eps) * float(eps))


def _f32(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, "operands are handed over as the fp32 values they are read as, got %s" % x.dtype
    return x


def rho(x, kind, eps=DEFAULT_EPS):
    """fp32 rho of an fp32 array"""
    x = _f32(x)
    if kind == "mse":
        return x * x
    if kind == "l1":
        return np.abs(x)
    if kind == "charbonnier":
        return np.sqrt(x * x + eps2_f32(eps))
    raise ValueError("unknown loss kind %r (one of %s)" % (kind, ", ".join(KINDS)))


def drho(x, kind, eps=DEFAULT_EPS):
    """fp32 rho' of an fp32 array"""
    x = _f32(x)
    if kind == "mse":
        return x + x
    if kind == "l1":
        return np.where(x > 0, _F32(1), np.where(x < 0, _F32(-1), _F32(0))).astype(np.float32)
    if kind == "charbonnier":
        return x / np.sqrt(x * x + eps2_f32(eps))
    raise ValueError("unknown loss kind %r (one of %s)" % (kind, ", ".join(KINDS)))


def mosaic_count(n, h, w):
    """pixels of the make_grid mosaic the reference's logged PSNR is taken over (utils.psnr_y_device: n images, 2-pixel
    zero padding that adds no error but is counted)"""
    if n == 1:
        return h * w
    xmaps = min(int(math.sqrt(n)), n)
    ymaps = int(math.ceil(float(n) / xmaps))
    return ((h + 2) * ymaps + 2) * ((w + 2) * xmaps + 2)


def y_sse(o, t):
    """exact integer squared error of the luma images of two fp32 NCHW batches"""
    ya = utils.y_exact(utils._quantise_u8(_f32(o))).astype(np.int64)
    yb = utils.y_exact(utils._quantise_u8(_f32(t))).astype(np.int64)
    return int(((ya - yb) ** 2).sum())


def sr_loss_np(o, t, s=None, kind="l1", eps=DEFAULT_EPS, w_main=1.0, w_kd=0.0, psnr_count=None):
    """{"sum_main", "sum_kd", "loss" (fp64), "loss_f32", "y_sse" (int), "psnr"} of fp32 arrays o, t and s"""
    o, t = _f32(o), _f32(t)
    M = float(o.size)
    sum_main = float(rho(o - t, kind, eps).astype(np.float64).sum())
    sum_kd = float(rho(o - _f32(s), kind, eps).astype(np.float64).sum()) if s is not None else 0.0
    loss = float(w_main) * sum_main / M + float(w_kd) * sum_kd / M
    sse = y_sse(o, t)
    if psnr_count is None:
        psnr_count = o.shape[0] * o.shape[2] * o.shape[3]
    return {"sum_main": sum_main, "sum_kd": sum_kd, "loss": loss, "loss_f32": _F32(loss), "y_sse": sse,
            "psnr": utils.psnr_from_sse(sse, psnr_count)}


def round_to(x, dtype):
    """fp32 array -> the fp32 values of its round-to-nearest-even into "f32", "f16" or "bf16" """
    x = _f32(x)
    if dtype == "f32":
        return x
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    if dtype == "bf16":
        b = np.ascontiguousarray(x).view(np.uint32)
        r = ((b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).view(np.float32)
        return np.where(np.isnan(x), x, r).astype(np.float32)
    raise ValueError("unknown dtype %r" % (dtype,))


def sr_loss_grad_np(o, t, s=None, kind="l1", eps=DEFAULT_EPS, w_main=1.0, w_kd=0.0, g=1.0, dtype="f32"):
    """dL/do for the incoming gradient g, as the fp32 values of the result in o's dtype ("f32", "f16", "bf16")"""
    o, t = _f32(o), _f32(t)
    M = float(o.size)
    ga = _F32(float(w_main) / M) * _F32(g)
    out = ga * drho(o - t, kind, eps)
    if s is not None:
        gb = _F32(float(w_kd) / M) * _F32(g)
        out = out + gb * drho(o - _f32(s), kind, eps)
    assert out.dtype == np.float32
    return round_to(out, dtype)


def kd_weights(kd_ratio, shrinking):
    """(w_main, w_kd) of the two training loops: the teacher loop adds kd_ratio times the teacher term, the
    progressive-shrinking loop scales that sum by 2 / (kd_ratio + 1)"""
    kd = float(kd_ratio)
    return (2.0 / (kd + 1.0), 2.0 * kd / (kd + 1.0)) if shrinking else (1.0, kd)


def check_cli(ap, loss, loss_eps):
    """the --loss / --loss-eps rules of the training scripts; `ap` is the argparse parser that reports the refusal.
    Returns the eps to use."""
    if loss_eps is not None:
        if loss != "charbonnier":
            ap.error("--loss-eps belongs to --loss charbonnier (got --loss %s)" % loss)
        if not (loss_eps > 0 and math.isfinite(loss_eps)):
            ap.error("--loss-eps must be positive, got %r" % (loss_eps,))
        return float(loss_eps)
    return DEFAULT_EPS
