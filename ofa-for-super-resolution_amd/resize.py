"""Host definition of target-size output: Pillow's fixed-point resize, restated for 8-bit and 10-bit samples.

The result of TiledUpscaler.upscale(img, out_size=(TH, TW), resample=F) is DEFINED as Pillow's
Image.resize((TW, TH), F) of the quantised full-size output; for video it is video.rgb_to_yuv420_host of the resized
quantised RGB of the full-size output.  This module states that resize (Pillow src/libImaging/Resample.c:
precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc -> clip -> ImagingResampleVertical_8bpc -> clip)
in numpy; the fused HIP sink (csrc/resize_scatter.hip, ofasr_tile_resize_scatter_*) is tested against it bit for bit,
and it is pinned to the installed Pillow and, for bicubic, to oracle/pil_bicubic.py (tests/test_resize.py).

Per output index xx of an axis resized from in_size to out_size, with the filter's support sup (bicubic 2, lanczos 3):
    scale = in_size / out_size; filterscale = max(scale, 1); support = sup * filterscale; ksize = 2 * ceil(support) + 1
    center = (xx + 0.5) * scale; xmin = max(int(center - support + 0.5), 0); xmax = min(int(center + support + 0.5), in_size)
    w[x] = filter((x + xmin - center + 0.5) / filterscale), x < xmax - xmin, normalised to sum 1 in double
    k[x] = int(w[x] * 2**bits +- 0.5)     (round half away from zero by a truncating cast), bits = 32 - depth - 2
    out = clip((sum_x pixel[xmin + x] * k[x] + 2**(bits - 1)) >> bits, 0, 2**depth - 1)
horizontal pass first, its clipped result the input of the vertical pass; an axis whose size does not change is not
resampled.  Depth 8 is Pillow (22 coefficient bits).  Depth 10 is not something Pillow has: the same arithmetic with
1023 in place of 255 and 20 coefficient bits.  Pillow accumulates in int32 and so does the kernel; the host code
accumulates in int64 and asserts that no accumulator leaves int32.

The weights are always computed here (double, libm's sin) and uploaded: a device sin need not equal libm's.
"""
import math

import numpy as np

FILTERS = ("bicubic", "lanczos")
SUPPORT = {"bicubic": 2.0, "lanczos": 3.0}
MAX_TAPS = 25            # 2 * ceil(3 * 4) + 1: lanczos at a 4 : 1 reduction, the most the fused sink takes per axis


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


_KERNELS = {"bicubic": _bicubic, "lanczos": _lanczos}


def check_filter(filter):
    if filter not in FILTERS:
        raise ValueError("resample must be one of %s, got %r" % (list(FILTERS), filter))
    return filter


def precision_bits(depth):
    if isinstance(depth, bool) or depth not in (8, 10):
        raise ValueError("depth must be 8 or 10, got %r" % (depth,))
    return 32 - depth - 2


def ksize(in_size, out_size, filter):
    scale = float(in_size) / float(out_size)
    return int(math.ceil(SUPPORT[check_filter(filter)] * max(scale, 1.0))) * 2 + 1


def coeff_table(in_size, out_size, filter, depth=8):
    """int32 [out_size, 2 + ksize] rows (xmin, count, k[0 .. ksize)): precompute_coeffs + normalize_coeffs_8bpc (the
    layout of rs_coeff_kernel, csrc/resample.hip); coefficients past `count` are 0"""
    fn = _KERNELS[check_filter(filter)]
    bits = precision_bits(depth)
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("empty axis %d -> %d" % (in_size, out_size))
    scale = float(in_size) / float(out_size)
    filterscale = scale if scale >= 1.0 else 1.0
    support = SUPPORT[filter] * filterscale
    ks = int(math.ceil(support)) * 2 + 1
    table = np.zeros((out_size, 2 + ks), np.int32)
    ss = 1.0 / filterscale
    one = float(1 << bits)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        row = table[xx]
        row[0], row[1] = xmin, xmax
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            row[2 + x] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
    return table


def identity_table(size, depth=8):
    """the table of an axis that is not resampled: one tap of weight 1 at the pixel itself (the pass is then exact:
    (p * 2**bits + 2**(bits - 1)) >> bits == p)"""
    table = np.zeros((int(size), 3), np.int32)
    table[:, 0] = np.arange(int(size))
    table[:, 1] = 1
    table[:, 2] = 1 << precision_bits(depth)
    return table


def axis_table(in_size, out_size, filter, depth=8):
    """coeff_table, or identity_table where the axis keeps its size (Pillow skips that pass)"""
    check_filter(filter)
    return identity_table(in_size, depth) if int(in_size) == int(out_size) else coeff_table(in_size, out_size, filter, depth)


def apply_table(img, table, depth=8, axis=-1):
    """one pass along `axis` of integer samples img with a table of coeff_table's layout -> the clipped samples, in
    img's dtype (uint8 for depth 8, uint16 for depth 10).  int64 accumulators, asserted to stay inside int32."""
    bits = precision_bits(depth)
    peak = (1 << depth) - 1
    src = np.moveaxis(np.asarray(img), axis, -1).astype(np.int64)
    out = np.empty(src.shape[:-1] + (table.shape[0],), np.asarray(img).dtype)
    for xx in range(table.shape[0]):
        x0, n = int(table[xx, 0]), int(table[xx, 1])
        prod = src[..., x0:x0 + n] * table[xx, 2:2 + n].astype(np.int64)
        acc = prod.sum(axis=-1) + (1 << (bits - 1))
        # every partial sum, in the order the kernel adds them, stays inside int32 as well
        part = np.cumsum(prod, axis=-1) + (1 << (bits - 1))
        if part.size:
            assert int(part.max()) < 2 ** 31 and int(part.min()) >= -2 ** 31, "an accumulator left int32"
        out[..., xx] = np.clip(acc >> bits, 0, peak)
    return np.moveaxis(out, -1, axis)


def _dtype(depth):
    precision_bits(depth)
    return np.uint8 if depth == 8 else np.uint16


def resize_host(img, out_h, out_w, filter="lanczos", depth=8, hwc=False):
    """img: integer samples [..., H, W] (planes), or [H, W, C] with hwc=True -> [..., out_h, out_w] / [out_h, out_w, C]:
    Pillow's Image.resize((out_w, out_h), filter) per plane for depth 8 (uint8), the same arithmetic at 10 bits for
    depth 10 (uint16 samples <= 1023)"""
    check_filter(filter)
    img = np.ascontiguousarray(img, dtype=_dtype(depth))
    if hwc:
        if img.ndim != 3:
            raise ValueError("an HWC image has three axes, got %s" % (img.shape,))
        return np.ascontiguousarray(np.moveaxis(resize_host(np.moveaxis(img, 2, 0), out_h, out_w, filter, depth), 0, 2))
    if img.ndim < 2:
        raise ValueError("resize_host needs [..., H, W], got %s" % (img.shape,))
    if depth == 10 and img.size and int(img.max()) > 1023:
        raise ValueError("a 10-bit sample above 1023")
    if int(out_w) != img.shape[-1]:
        img = apply_table(img, coeff_table(img.shape[-1], out_w, filter, depth), depth, -1)
    if int(out_h) != img.shape[-2]:
        img = apply_table(img, coeff_table(img.shape[-2], out_h, filter, depth), depth, -2)
    return np.ascontiguousarray(img)


def quantise(x, depth=8):
    """the scatter kernels' quantisation of network output (float32 array): round_half_even(clamp(v, 0, 1) * peak), the
    product rounded to fp32 first"""
    peak = np.float32((1 << depth) - 1)
    v = np.clip(np.asarray(x, np.float32), np.float32(0), np.float32(1)) * peak
    return np.rint(v).astype(_dtype(depth))


# ---------------------------------------------------------------------------------------------- target partition
def target_edge(p, S, T, even=False):
    """t(p) = ceil(p * T / S), rounded up to even for YUV planes, capped at T: the first target pixel that the core
    starting at source pixel p owns"""
    t = -(-p * T // S)
    if even:
        t += t & 1
    return min(t, T)


def needed_range(table, t0, t1):
    """[lo, hi): the source pixels that the target pixels [t0, t1) read, from a table of coeff_table's layout"""
    if t1 <= t0:
        return None
    rows = table[t0:t1]
    return int(rows[:, 0].min()), int((rows[:, 0] + rows[:, 1]).max())


def parse_size(text):
    """'WxH' -> (W, H); raises ValueError"""
    try:
        w, h = str(text).lower().split("x")
        w, h = int(w), int(h)
    except ValueError:
        raise ValueError("expected WxH, got %r" % (text,))
    if w < 1 or h < 1:
        raise ValueError("expected a positive WxH, got %r" % (text,))
    return w, h
