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

With an SSIM weight alpha (ops.sr_loss(ssim=alpha), --loss-ssim) the loss is (1 - alpha) * L + alpha * (1 - S); S, its
gradient and how the two addends of an element meet are stated further down (ssim_np, sr_loss_ssim_np,
sr_loss_ssim_grad_np).
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


# ------------------------------------------------------------------------------------------------ the SSIM term
# L = (1 - alpha) * L_pix + alpha * (1 - S), alpha in (0, 1] (ops.sr_loss(ssim=alpha); ofasr_sr_loss_ssim_*; DESIGN.md
# section 3.1s).  S is the mean SSIM of o against t over the three colour planes of every image: the fp32 values
# promoted to fp64, no clamp and no quantisation, the metric's window (utils.SSIM_WINDOW taps, utils.SSIM_SIGMA,
# utils._gauss_valid: along W, then along H) at the (H - 10) x (W - 10) positions where it lies inside the plane,
# C1 = 0.01^2 and C2 = 0.03^2 (data range 1).  The teacher term stays pixel-wise.
SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2


def ssim_window():
    g = np.exp(-((np.arange(utils.SSIM_WINDOW) - utils.SSIM_WINDOW // 2) ** 2) / (2.0 * utils.SSIM_SIGMA ** 2))
    return g / g.sum()


def check_ssim(alpha, h, w):
    if not (0.0 < alpha <= 1.0):
        raise ValueError("the SSIM weight must lie in (0, 1], got %r" % (alpha,))
    if h < utils.SSIM_WINDOW or w < utils.SSIM_WINDOW:
        raise ValueError("a %dx%d plane has a side below the %d-pixel SSIM window" % (h, w, utils.SSIM_WINDOW))


def _ssim_terms(o, t):
    """(m1, m2, A1, A2, B1, B2) of fp32 NCHW batches, each [N * C, H - 10, W - 10] fp64"""
    o, t = _f32(o), _f32(t)
    check_ssim(1.0, o.shape[2], o.shape[3])
    a = o.astype(np.float64).reshape((-1,) + o.shape[2:])
    b = t.astype(np.float64).reshape((-1,) + t.shape[2:])
    g = ssim_window()
    m1, m2 = utils._gauss_valid(a, g), utils._gauss_valid(b, g)
    s1 = utils._gauss_valid(a * a, g) - m1 * m1
    s2 = utils._gauss_valid(b * b, g) - m2 * m2
    s12 = utils._gauss_valid(a * b, g) - m1 * m2
    return m1, m2, 2.0 * m1 * m2 + SSIM_C1, 2.0 * s12 + SSIM_C2, m1 * m1 + m2 * m2 + SSIM_C1, s1 + s2 + SSIM_C2


def ssim_np(o, t):
    """(S, K): the mean SSIM of fp32 arrays o and t over all planes and valid positions, and their number"""
    _, _, A1, A2, B1, B2 = _ssim_terms(o, t)
    ssim = (A1 * A2) / (B1 * B2)
    return float(ssim.sum()) / float(ssim.size), int(ssim.size)


def _gauss_full_t(d, g):
    """the transpose of utils._gauss_valid: [P, h, w] maps at the valid positions -> [P, h + 10, w + 10], the full
    correlation with the same taps (the map is zero outside the valid positions), along H and then along W"""
    k = len(g)
    P, h, w = d.shape
    u = np.zeros((P, h + k - 1, w), np.float64)
    for i in range(k):
        u[:, i:i + h, :] += g[i] * d
    v = np.zeros((P, h + k - 1, w + k - 1), np.float64)
    for i in range(k):
        v[:, :, i:i + w] += g[i] * u
    return v


def ssim_grad_np(o, t):
    """dS/do of fp32 arrays o and t, fp64, shaped like o"""
    m1, m2, A1, A2, B1, B2 = _ssim_terms(o, t)
    K = float(m1.size)
    dr = 2.0 * A1 / (B1 * B2)
    dp = -A1 * A2 / (B1 * B2 * B2)
    dm = 2.0 * m2 * (A2 - A1) / (B1 * B2) - 2.0 * m1 * A1 * A2 * (B2 - B1) / ((B1 * B2) * (B1 * B2))
    g = ssim_window()
    od = _f32(o).astype(np.float64).reshape((-1,) + o.shape[2:])
    td = _f32(t).astype(np.float64).reshape((-1,) + t.shape[2:])
    return ((_gauss_full_t(dm, g) + 2.0 * od * _gauss_full_t(dp, g) + td * _gauss_full_t(dr, g)) / K).reshape(o.shape)


def sr_loss_ssim_np(o, t, s=None, kind="l1", eps=DEFAULT_EPS, w_main=1.0, w_kd=0.0, psnr_count=None, alpha=0.2):
    """sr_loss_np's dict with "loss" = (1 - alpha) * L_pix + alpha * (1 - S) in fp64, its "loss_f32", "loss_pix" (what
    sr_loss_np calls "loss"), "ssim" (S) and "ssim_sum" (S * K as summed)"""
    check_ssim(alpha, o.shape[2], o.shape[3])
    r = sr_loss_np(o, t, s, kind, eps, w_main, w_kd, psnr_count)
    _, _, A1, A2, B1, B2 = _ssim_terms(o, t)
    ssim = (A1 * A2) / (B1 * B2)
    r["ssim_sum"] = float(ssim.sum())
    r["ssim"] = r["ssim_sum"] / float(ssim.size)
    r["loss_pix"] = r["loss"]
    r["loss"] = (1.0 - float(alpha)) * r["loss_pix"] + float(alpha) * (1.0 - r["ssim"])
    r["loss_f32"] = _F32(r["loss"])
    return r


def sr_loss_ssim_parts_np(o, t, s=None, kind="l1", eps=DEFAULT_EPS, w_main=1.0, w_kd=0.0, g=1.0, alpha=0.2):
    """(pix, add): the two fp32 addends of the gradient -- sr_loss_grad_np's fp32 element for the weights scaled by
    (1 - alpha) (the products formed in fp64) and fp32(fp64(g) * -alpha * dS/do)"""
    check_ssim(alpha, o.shape[2], o.shape[3])
    a = float(alpha)
    pix = sr_loss_grad_np(o, t, s, kind, eps, (1.0 - a) * float(w_main), (1.0 - a) * float(w_kd), g=g, dtype="f32")
    add = (float(_F32(g)) * -a * ssim_grad_np(o, t)).astype(np.float32)
    return pix, add


def sr_loss_ssim_grad_np(o, t, s=None, kind="l1", eps=DEFAULT_EPS, w_main=1.0, w_kd=0.0, g=1.0, dtype="f32", alpha=0.2):
    """dL/do with the SSIM term for the incoming gradient g: fl32(pix + fl32(fp64(g) * -alpha * dS/do)) per element, as
    the fp32 values of its round-to-nearest-even into o's dtype ("f32", "f16", "bf16")"""
    pix, add = sr_loss_ssim_parts_np(o, t, s, kind, eps, w_main, w_kd, g, alpha)
    out = pix + add
    assert out.dtype == np.float32
    return round_to(out, dtype)


def kd_weights(kd_ratio, shrinking):
    """(w_main, w_kd) of the two training loops: the teacher loop adds kd_ratio times the teacher term, the
    progressive-shrinking loop scales that sum by 2 / (kd_ratio + 1)"""
    kd = float(kd_ratio)
    return (2.0 / (kd + 1.0), 2.0 * kd / (kd + 1.0)) if shrinking else (1.0, kd)


def check_cli(ap, loss, loss_eps, loss_ssim=0.0):
    """the --loss / --loss-eps / --loss-ssim rules of the training scripts; `ap` is the argparse parser that reports the
    refusal.  Returns the eps to use."""
    if not (0.0 <= loss_ssim <= 1.0):
        ap.error("--loss-ssim must lie in [0, 1], got %r" % (loss_ssim,))
    if loss_ssim > 0 and loss == "reference":
        ap.error("--loss-ssim belongs to the fused losses (--loss mse|l1|charbonnier), got --loss reference")
    if loss_eps is not None:
        if loss != "charbonnier":
            ap.error("--loss-eps belongs to --loss charbonnier (got --loss %s)" % loss)
        if not (loss_eps > 0 and math.isfinite(loss_eps)):
            ap.error("--loss-eps must be positive, got %r" % (loss_eps,))
        return float(loss_eps)
    return DEFAULT_EPS
