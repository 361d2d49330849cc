"""Content-aware routing of tile windows between two exported networks: the host statement (numpy only, no GPU).

A window of the tile plan is *easy* when its luma is flat and goes to the cheaper network, *hard* otherwise
(upscale.TiledUpscaler(net, easy_net=..., easy_threshold=T)).  Everything here is an exact integer function of the
window's own input bytes, which is what the HIP kernels (csrc/route.hip) are tested against:

  luma sample L    YUV input: the Y plane as stored (uint8, or uint16 at depth 10);
                   RGB input: L = (77 R + 150 G + 29 B + 128) >> 8
  activity A       with the origin clamped as the gather kernels clamp it, y0 = clamp(oy, 0, H - h), x0 alike, over the
                   window rectangle rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1:
                     A = sum_{r < h, c < w - 1} |L[r, c + 1] - L[r, c]| + sum_{r < h - 1, c < w} |L[r + 1, c] - L[r, c]|
                   only differences with both samples inside the rectangle count
  terms D          D = h (w - 1) + (h - 1) w, the same for every window of a plan
  class            easy iff A <= limit, limit = floor(T * D * (4 if depth 10 else 1)) from the decimal the user wrote:
                   T is the mean absolute luma difference in 8-bit levels.  T < 0: limit = -1 (every window hard),
                   T = inf: limit = INT64_MAX (every window easy), NaN is refused.
"""
import math
from fractions import Fraction

import numpy as np

INT64_MAX = 2 ** 63 - 1


def luma_rgb(img):
    """L of an HWC uint8 RGB image, as int64 [H, W]"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("luma_rgb takes an HWC uint8 RGB image, got %s %s" % (img.shape, img.dtype))
    p = img.astype(np.int64)
    return (77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8


def luma_plane(src):
    """the luma samples of an input as int64 [H, W]: an HWC uint8 RGB image, or one 2-D uint8 / uint16 plane"""
    src = np.asarray(src)
    if src.ndim == 3:
        return luma_rgb(src)
    if src.ndim != 2 or src.dtype not in (np.uint8, np.uint16):
        raise ValueError("a luma plane is 2-D uint8 or uint16, got %s %s" % (src.shape, src.dtype))
    return src.astype(np.int64)


def activity_terms(h, w):
    """D: the number of differences in the activity of an h x w window"""
    return h * (w - 1) + (h - 1) * w


def depth_factor(depth):
    if isinstance(depth, bool) or depth not in (8, 10):
        raise ValueError("depth must be 8 or 10, got %r" % (depth,))
    return 4 if depth == 10 else 1


def window_activity_host(src, origins, h, w):
    """A per window, int64 [n]: src an RGB image or a luma plane (luma_plane), origins [(oy, ox)] of h x w windows"""
    L = luma_plane(src)
    H, W = L.shape
    if not (0 < h <= H and 0 < w <= W):
        raise ValueError("window %dx%d does not fit the %dx%d frame" % (w, h, W, H))
    dh = np.abs(np.diff(L, axis=1))      # [H, W - 1]: |L[r, c + 1] - L[r, c]|
    dv = np.abs(np.diff(L, axis=0))      # [H - 1, W]
    out = np.zeros(len(origins), dtype=np.int64)
    for i, (oy, ox) in enumerate(origins):
        y0, x0 = min(max(int(oy), 0), H - h), min(max(int(ox), 0), W - w)
        out[i] = int(dh[y0:y0 + h, x0:x0 + w - 1].sum()) + int(dv[y0:y0 + h - 1, x0:x0 + w].sum())
    return out


def activity_limit(T, h, w, depth=8):
    """the integer `limit` of a threshold T (a number, or the decimal string the user wrote) for h x w windows"""
    f = depth_factor(depth)
    if isinstance(T, bool):
        raise ValueError("the threshold must be a number, got %r" % (T,))
    if isinstance(T, str):
        text = T.strip()
        try:
            v = float(text)
        except ValueError:
            raise ValueError("the threshold must be a number, got %r" % (T,))
    else:
        v, text = float(T), str(T)
    if math.isnan(v):
        raise ValueError("the threshold must not be NaN")
    if v < 0:
        return -1
    if math.isinf(v):
        return INT64_MAX
    try:
        exact = Fraction(text)
    except (ValueError, ZeroDivisionError):
        exact = Fraction(str(v))
    return min(INT64_MAX, int(math.floor(exact * activity_terms(h, w) * f)))


def classify_host(src, origins, h, w, T, depth=None):
    """bool [n]: True where the window is easy.  depth: None takes it from the sample type (uint16: 10)"""
    arr = np.asarray(src)
    if depth is None:
        depth = 10 if arr.dtype == np.uint16 else 8
    return window_activity_host(arr, origins, h, w) <= activity_limit(T, h, w, depth)


def mean_activity(A, h, w, depth=8):
    """A / (D * depth factor) as float64: the per-difference mean in 8-bit levels, what a user compares with T"""
    d = activity_terms(h, w) * depth_factor(depth)
    A = np.asarray(A, dtype=np.float64)
    return A / d if d else np.zeros_like(A)


def shared_plan_params(a, b):
    """a, b: (receptive radius, alignment, activation elements per pixel) of two networks -> the (radius, align, halo,
    px_elems) of the one tile plan both can run: the larger radius, the lcm of the alignments, the halo rounded up to
    it, the larger activation.  A halo larger than a network needs changes no core: every core pixel is still at least
    that network's radius from every outer window edge that is not an image edge."""
    radius = max(int(a[0]), int(b[0]))
    align = int(a[1]) * int(b[1]) // math.gcd(int(a[1]), int(b[1]))
    halo = -(-radius // align) * align
    return radius, align, halo, max(int(a[2]), int(b[2]))
