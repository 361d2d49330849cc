"""Host definition of keeping an image's mode through upscaling: L, LA, RGB and RGBA in, the same mode out.

The network takes and returns RGB.  With F = TiledUpscaler.upscale (tiled or whole, any mix_prec, self_ensemble, routing,
out_size / resample) and (TH, TW) the size F returns, TiledUpscaler.upscale_image(img) is DEFINED, for an HWC uint8 image
of C channels, as

    rgb_in    = L, L, L for L / LA (Pillow's convert("RGB") of L); the first three channels of RGBA, untouched (straight
                alpha: the colour under transparent pixels is fed as it is)
    rgb_out   = F(rgb_in)                                             exactly today's result
    alpha_out = PIL.Image.fromarray(alpha_in, "L").resize((TW, TH), A)   = resize.resize_host(alpha_in, TH, TW, A)
                a resize of the SOURCE alpha straight to the output's size, never a resize of a resize; A is "bicubic"
                (the default) or "lanczos"; the ratio is between 1 and the network's factor on each axis, and an axis
                whose size does not change is not resampled
    grey_out  = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 of rgb_out   Pillow's convert("L")
    result    = grey_out | grey_out, alpha_out | rgb_out | rgb_out, alpha_out      for C = 1 | 2 | 3 | 4

All integers.  The HIP kernels (csrc/mode_io.hip: ofasr_mode_unpack_u8, ofasr_mode_pack_u8) are tested against this module
bit for bit, and this module is pinned to the installed Pillow (tests/test_modes.py).  numpy only: no GPU is needed to
import it.
"""
import numpy as np

from . import resize

MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}      # channels of an HWC uint8 image -> Pillow's mode
ALPHA_FILTER = "bicubic"
MAX_TAPS = 7             # per axis of the pack kernel: lanczos enlarging (2 * ceil(3) + 1); bicubic 5, identity 1
TILE_ROWS = 16           # target rows of one workgroup of the pack kernel ...
MAX_SOURCE_ROWS = 24     # ... and the most alpha rows they may read (the kernel's LDS intermediate)


def channels(img):
    """C of an HWC uint8 image with C in MODES; refuses everything else"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in MODES:
        raise ValueError("an image is HWC uint8 with 1 (L), 2 (LA), 3 (RGB) or 4 (RGBA) channels, got %s %s"
                         % (img.shape, img.dtype))
    return int(img.shape[2])


def split_host(img):
    """HWC uint8 [H, W, C] -> (rgb [H, W, 3], alpha [H, W] or None)"""
    C = channels(img)
    img = np.asarray(img)
    rgb = img[:, :, :3] if C >= 3 else np.repeat(img[:, :, :1], 3, axis=2)
    alpha = img[:, :, C - 1] if C in (2, 4) else None
    return np.ascontiguousarray(rgb), None if alpha is None else np.ascontiguousarray(alpha)


def alpha_host(alpha, TH, TW, filter=ALPHA_FILTER):
    """the source alpha plane [H, W] resized straight to [TH, TW]: Pillow's Image.resize((TW, TH), filter)"""
    alpha = np.asarray(alpha)
    if alpha.dtype != np.uint8 or alpha.ndim != 2:
        raise ValueError("an alpha plane is [H, W] uint8, got %s %s" % (alpha.shape, alpha.dtype))
    return resize.resize_host(alpha, TH, TW, filter)


def luma_host(rgb):
    """HWC uint8 RGB -> [H, W] uint8: Pillow's convert("L")"""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("luma_host takes an HWC uint8 RGB image, got %s %s" % (rgb.shape, rgb.dtype))
    v = rgb.astype(np.uint32)
    return ((19595 * v[:, :, 0] + 38470 * v[:, :, 1] + 7471 * v[:, :, 2] + 0x8000) >> 16).astype(np.uint8)


def join_host(rgb_out, channels, alpha_out=None):
    """the RGB output [TH, TW, 3] and the resized alpha [TH, TW] (LA / RGBA only) -> HWC uint8 [TH, TW, channels]"""
    rgb_out = np.asarray(rgb_out)
    if channels not in MODES:
        raise ValueError("channels must be one of %s, got %r" % (sorted(MODES), channels))
    if rgb_out.dtype != np.uint8 or rgb_out.ndim != 3 or rgb_out.shape[2] != 3:
        raise ValueError("join_host takes an HWC uint8 RGB image, got %s %s" % (rgb_out.shape, rgb_out.dtype))
    if (alpha_out is not None) != (channels in (2, 4)):
        raise ValueError("%s %s an alpha plane" % (MODES[channels], "needs" if alpha_out is None else "has no room for"))
    if alpha_out is not None:
        alpha_out = np.asarray(alpha_out)
        if alpha_out.dtype != np.uint8 or alpha_out.shape != rgb_out.shape[:2]:
            raise ValueError("the alpha plane must be uint8 %s, got %s %s" % (rgb_out.shape[:2], alpha_out.shape, alpha_out.dtype))
    colour = rgb_out if channels >= 3 else luma_host(rgb_out)[:, :, None]
    parts = [colour] + ([alpha_out[:, :, None]] if alpha_out is not None else [])
    return np.ascontiguousarray(np.concatenate(parts, axis=2))


def alpha_tables(H, W, TH, TW, filter=ALPHA_FILTER):
    """(vertical [TH, 2 + kh], horizontal [TW, 2 + kw]) int32 coefficient tables of the alpha resize H x W -> TH x TW
    (resize.axis_table, depth 8), after checking what the pack kernel relies on: the resize enlarges, an axis has at
    most MAX_TAPS taps, and any TILE_ROWS consecutive target rows read at most MAX_SOURCE_ROWS source rows"""
    H, W, TH, TW = int(H), int(W), int(TH), int(TW)
    if H < 1 or W < 1 or TH < H or TW < W:
        raise ValueError("the alpha plane is only enlarged: %dx%d -> %dx%d" % (W, H, TW, TH))
    vt, ht = resize.axis_table(H, TH, filter), resize.axis_table(W, TW, filter)
    for t in (vt, ht):
        assert 1 <= t.shape[1] - 2 <= MAX_TAPS and int(t[:, 1].max()) <= MAX_TAPS, "more than %d taps" % MAX_TAPS
    for t0 in range(max(TH - TILE_ROWS, 0) + 1):
        lo, hi = resize.needed_range(vt, t0, min(t0 + TILE_ROWS, TH))
        assert hi - lo <= MAX_SOURCE_ROWS, "target rows %d .. read %d source rows, more than %d" % (t0, hi - lo, MAX_SOURCE_ROWS)
    return vt, ht
