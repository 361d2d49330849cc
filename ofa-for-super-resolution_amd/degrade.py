"""The blind-SR degradation of the training inputs, LR = (HR * k) downsampled + n, as exact integer functions: the host
statement (numpy, no GPU) of csrc/degrade.hip (ofasr_degrade_blur_u8, ofasr_degrade_noise_u8).  Everything the kernels
compute is defined here, and they are tested against it bit for bit.

Blur.  A separable, axis-aligned Gaussian on a uint8 batch [N, 3, H, W], each sample with its own (sigma_x, sigma_y) in
HR pixels.  blur_taps(sigma) is formed on the host in float64: radius r = min(10, max(1, ceil(3 sigma))) (r = 0 for
sigma = 0), t[d] = floor(g[d] * 2^14 + 0.5) of the normalised Gaussian, the centre tap then corrected so that the taps
sum to exactly 2^14.  The horizontal pass is h = (sum_d t_x[d] * p[y][clamp(x + d)] + 2^13) >> 14 -- a uint8 without a
clip, because the taps are non-negative and sum to 2^14 -- and the vertical pass the same sum on h with t_y.  The border
rule is clamp to the edge of the [H, W] plane.  r_x = r_y = 0 is a copy.

Noise.  Additive, laid on the uint8 LR image after the bicubic.  One Philox4x32-10 call per element, counter
(y * W + x, channel, stream, scale), key (seed & 0xffffffff, seed >> 32): `stream` a per-sample 31-bit word, `scale` 2
or 4, the down-scale of the image the noise is laid on.  With s the sum of the 16 output bytes, c = s - 2040 has mean 0
and standard deviation sqrt(16 * 65535 / 12) = 295.601 and is near-Gaussian (a sum of 16 uniform bytes); the
per-sample amplitude is a = round(sigma_n * 2^16 / 295.601), the noise (a * c + 2^15) >> 16 (arithmetic shift) and the
output clip(v + noise, 0, 255).  With the sample's `gray` flag all three channels use channel 0's value.  a = 0 is a
copy.  sigma_n <= 50 8-bit levels, so |a * c| < 2^25.

Table.  One int32 [N, 48] table serves both kernels:
    0, 1    r_x, r_y            2   a           3   gray        4   stream      5   0
    6..26   t_x, the tap for offset d at 16 + d, zero outside the radius        27..47  t_y likewise (at 37 + d)

Drawing.  draw_degrade(spec) uses the torch global RNG: per sample one torch.rand(5) (on / sigma_x / sigma_y / sigma_n /
gray) and one torch.randint(0, 2**31, (1,)) (stream), both always made, so the RNG stream does not depend on the
outcomes.  sigma = lo + (hi - lo) * u in float64; sigma_y = sigma_x unless `aniso`; a sample whose u_on >= prob gets the
identity row.  A loader draws a batch's rows after all crop draws of that batch, in batch order.
"""
import math

import numpy as np

TAP_BITS = 14
MAX_RADIUS = 10
MAX_SIGMA = MAX_RADIUS / 3.0
TABLE_COLS = 48
COL_RX, COL_RY, COL_A, COL_GRAY, COL_STREAM = 0, 1, 2, 3, 4
COL_TX, COL_TY = 16, 37            # the column of the centre tap (offset d stands at COL + d)
NOISE_STD = 295.601                # sqrt(16 * 65535 / 12), as the amplitude is defined with it
MAX_NOISE = 50.0

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------- blur
def blur_radius(sigma):
    sigma = float(sigma)
    if not 0.0 <= sigma <= MAX_SIGMA:
        raise ValueError("blur sigma %r outside 0 .. 10/3 HR pixels (the radius is at most %d)" % (sigma, MAX_RADIUS))
    return 0 if sigma == 0.0 else min(MAX_RADIUS, max(1, int(math.ceil(3.0 * sigma))))


def blur_taps(sigma):
    """the 2r + 1 integer taps of one axis (int64), summing to 2^14"""
    r = blur_radius(sigma)
    one = 1 << TAP_BITS
    if r == 0:
        return np.array([one], np.int64)
    d = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-(d * d) / (2.0 * float(sigma) * float(sigma)))
    g /= g.sum()
    t = np.floor(g * one + 0.5).astype(np.int64)
    t[r] += one - int(t.sum())
    return t


def _blur_axis(img, taps, axis):
    r = (len(taps) - 1) // 2
    if r == 0:
        return img
    size = img.shape[axis]
    src = img.astype(np.int64)
    acc = np.full(img.shape, 1 << (TAP_BITS - 1), np.int64)
    pos = np.arange(size)
    for d in range(-r, r + 1):
        acc += int(taps[d + r]) * np.take(src, np.clip(pos + d, 0, size - 1), axis=axis)
    return (acc >> TAP_BITS).astype(np.uint8)


def blur_plane_np(img, taps_x, taps_y):
    """uint8 [..., H, W] blurred with one pair of tap vectors: the horizontal pass, then the vertical pass on its uint8"""
    return _blur_axis(_blur_axis(np.asarray(img, np.uint8), taps_x, -1), taps_y, -2)


def _row_taps(row, col):
    r = int(row[COL_RX if col == COL_TX else COL_RY])
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError("degrade table: radius %d outside 0 .. %d" % (r, MAX_RADIUS))
    return np.asarray(row[col - r:col + r + 1], np.int64)


def blur_np(hr_u8, table):
    """the blurred batch: uint8 [N, 3, H, W] under rows 0 .. N - 1 of the table"""
    hr_u8 = np.asarray(hr_u8, np.uint8)
    out = np.empty_like(hr_u8)
    for n in range(hr_u8.shape[0]):
        out[n] = blur_plane_np(hr_u8[n], _row_taps(table[n], COL_TX), _row_taps(table[n], COL_TY))
    return out


# ---------------------------------------------------------------------------------------------- noise
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays that hold 32-bit words: counter [..., 4], key [..., 2]
    (broadcast against each other) -> [..., 4]"""
    c = np.asarray(counter, np.uint64) & _M32
    k = np.asarray(key, np.uint64) & _M32
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0          # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & _M32, p0 & _M32
        k0 = (k0 + np.uint64(PHILOX_W0)) & _M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def noise_amplitude(sigma_n):
    sigma_n = float(sigma_n)
    if not 0.0 <= sigma_n <= MAX_NOISE:
        raise ValueError("noise sigma %r outside 0 .. %g 8-bit levels" % (sigma_n, MAX_NOISE))
    return int(round(sigma_n * 65536.0 / NOISE_STD))


def noise_field_np(H, W, channels, stream, scale, seed):
    """c = s - 2040 per element: int64 [len(channels), H, W]"""
    if H * W >= 1 << 32:
        raise ValueError("noise: H * W = %d does not fit the 32-bit counter word" % (H * W))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    cnt = np.zeros((len(channels), H * W, 4), np.uint64)
    cnt[..., 0] = np.arange(H * W, dtype=np.uint64)
    cnt[..., 1] = np.asarray(channels, np.uint64)[:, None]
    cnt[..., 2] = np.uint64(int(stream) & 0xFFFFFFFF)
    cnt[..., 3] = np.uint64(int(scale))
    out = philox4x32_10(cnt, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
    s = np.zeros(out.shape[:-1], np.int64)
    for b in range(4):
        s += ((out >> np.uint64(8 * b)) & np.uint64(0xFF)).sum(axis=-1).astype(np.int64)
    return (s - 2040).reshape(len(channels), H, W)


def noise_np(lr_u8, table, seed, scale):
    """the noisy batch: uint8 [N, 3, H, W] under rows 0 .. N - 1 of the table"""
    if scale not in (2, 4):
        raise ValueError("noise: scale %r (2 or 4)" % (scale,))
    lr_u8 = np.asarray(lr_u8, np.uint8)
    out = np.empty_like(lr_u8)
    N, C, H, W = lr_u8.shape
    for n in range(N):
        a, gray, stream = int(table[n][COL_A]), int(table[n][COL_GRAY]), int(table[n][COL_STREAM])
        if a == 0:
            out[n] = lr_u8[n]
            continue
        c = noise_field_np(H, W, [0] * C if gray else list(range(C)), stream, scale, seed)
        out[n] = np.clip(lr_u8[n].astype(np.int64) + ((a * c + (1 << 15)) >> 16), 0, 255).astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------- table
def identity_row(stream=0):
    return (0.0, 0.0, 0.0, False, int(stream))


def degrade_table(rows, out=None):
    """int32 [N, 48] from rows (sigma_x, sigma_y, sigma_n, gray, stream); `out`: a numpy int32 array or torch int32 tensor
    of at least N rows to fill instead (the filled rows are returned)"""
    t = np.zeros((len(rows), TABLE_COLS), np.int32)
    for n, (sx, sy, sn, gray, stream) in enumerate(rows):
        tx, ty = blur_taps(sx), blur_taps(sy)
        rx, ry = (len(tx) - 1) // 2, (len(ty) - 1) // 2
        if not 0 <= int(stream) < 1 << 31:
            raise ValueError("degrade table: stream %r is no 31-bit word" % (stream,))
        t[n, :6] = (rx, ry, noise_amplitude(sn), 1 if gray else 0, int(stream), 0)
        t[n, COL_TX - rx:COL_TX + rx + 1] = tx
        t[n, COL_TY - ry:COL_TY + ry + 1] = ty
    if out is None:
        return t
    dst = out[:len(rows)]
    if isinstance(dst, np.ndarray):
        dst[...] = t
    else:
        import torch
        dst.copy_(torch.from_numpy(t))
    return dst


def degrade_np(hr_u8, table, seed):
    """{2: uint8 [N, 3, H/2, W/2], 4: uint8 [N, 3, H/4, W/4]}: the blur, Pillow's 8-bit bicubic (oracle/pil_bicubic.py's
    statement where it can be imported, Pillow itself otherwise), then the noise"""
    blurred = blur_np(hr_u8, table)
    return {f: noise_np(_scale_down(blurred, f), table, seed, f) for f in (2, 4)}


def _scale_down(img, f):
    h, w = int(img.shape[-2] * (1.0 / f)), int(img.shape[-1] * (1.0 / f))
    try:
        from oracle import pil_bicubic
    except ImportError:
        from PIL import Image
        flat = img.reshape((-1,) + img.shape[-2:])
        out = np.stack([np.asarray(Image.fromarray(p).resize((w, h), Image.BICUBIC)) for p in flat])
        return out.reshape(img.shape[:-2] + (h, w))
    return pil_bicubic.resize_u8(img, h, w)


def batch_np(hr_u8, table, seed):
    """the whole degraded batch under the loader's keys, float32 = u8 / 255 correctly rounded: 'image' stays clean"""
    lr = degrade_np(hr_u8, table, seed)
    unit = lambda a: a.astype(np.float32) / np.float32(255.0)
    return {"image": unit(np.asarray(hr_u8, np.uint8)), "2x_down_image": unit(lr[2]), "4x_down_image": unit(lr[4])}


# ---------------------------------------------------------------------------------------------- the spec and its draws
def _range(v, what, top):
    try:
        lo, hi = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError("%s: a range LO:HI of two numbers, got %r" % (what, v))
    if not (math.isfinite(lo) and math.isfinite(hi)) or not 0.0 <= lo <= hi:
        raise ValueError("%s: a range needs 0 <= LO <= HI, got %r:%r" % (what, lo, hi))
    if hi > top:
        raise ValueError("%s: HI %r above the limit %.6g" % (what, hi, top))
    return (lo, hi)


def _prob(v, what):
    p = float(v)
    if not 0.0 <= p <= 1.0:
        raise ValueError("%s: a probability in 0 .. 1, got %r" % (what, v))
    return p


def check_spec(spec, names=None):
    """the normalised spec {'blur': (lo, hi), 'aniso': bool, 'noise': (lo, hi), 'gray_prob': p, 'prob': p} (plain Python
    values: a checkpoint and a JSON config hold it as it is); None stays None.  `names`: what each key is called in the
    messages (the command line's option names)"""
    if spec is None:
        return None
    names = names or {}
    unknown = set(spec) - {"blur", "aniso", "noise", "gray_prob", "prob"}
    if unknown:
        raise ValueError("degrade: unknown key(s) %s" % sorted(unknown))
    blur = spec.get("blur") or (0.0, 0.0)
    noise = spec.get("noise") or (0.0, 0.0)
    return {"blur": _range(blur, names.get("blur", "degrade blur"), MAX_SIGMA),
            "aniso": bool(spec.get("aniso", False)),
            "noise": _range(noise, names.get("noise", "degrade noise"), MAX_NOISE),
            "gray_prob": _prob(spec.get("gray_prob", 0.0), names.get("gray_prob", "degrade gray_prob")),
            "prob": _prob(spec.get("prob", 1.0), names.get("prob", "degrade prob"))}


def describe(spec):
    return "blur %g:%g%s noise %g:%g gray-prob %g prob %g" % (
        spec["blur"][0], spec["blur"][1], " aniso" if spec["aniso"] else "", spec["noise"][0], spec["noise"][1],
        spec["gray_prob"], spec["prob"])


def draw_degrade(spec):
    """one sample's row (sigma_x, sigma_y, sigma_n, gray, stream) from the torch global RNG: always one rand(5) and one
    randint, whatever they give"""
    import torch
    u_on, u_x, u_y, u_n, u_g = (float(v) for v in torch.rand(5).double().tolist())
    stream = int(torch.randint(0, 2 ** 31, (1,)).item())
    if u_on >= spec["prob"]:
        return identity_row(stream)
    (blo, bhi), (nlo, nhi) = spec["blur"], spec["noise"]
    sx = blo + (bhi - blo) * u_x
    sy = blo + (bhi - blo) * u_y if spec["aniso"] else sx
    return (sx, sy, nlo + (nhi - nlo) * u_n, u_g < spec["gray_prob"], stream)


def fixed_rows(count, blur, noise, first=0):
    """the evaluation's fixed degradation: sigma_x = sigma_y = blur, sigma_n = noise, stream = the image's running index"""
    return [(float(blur), float(blur), float(noise), False, first + k) for k in range(count)]
