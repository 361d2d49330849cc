"""Tiled any-size image upscaling with an exported static SR network (SRNetS4 / SRNetX4, sr_static.py).

A whole large image is not run through the network in one call: at 4x for a 1920x1080 input the 64 -> 256 conv before
the last PixelShuffle alone would be 2.1e9 elements, past the 32-bit extents some kernels guard (mg_supported refuses an
MB block above 2^31 bytes and the block drops to the slower composite path).  Instead the input is cut into core tiles,
each core is given a halo of `receptive_radius(config)` input pixels, and the equally shaped windows run as one batch:

  * a window is the core plus `halo` on every side, CLAMPED INTO THE IMAGE BY SHIFTING, never by padding:
    start = clamp(x0 - halo, 0, W - win).  An outer window edge is then either a true image edge, where every conv
    zero-pads exactly as in the whole-image forward, or at least halo >= radius away from every core pixel.  Zero-filling
    outside the image would be wrong: from the second layer on the whole-image forward sees zero padding there, while a
    zero-filled window would see conv(0) + BN shift != 0.
  * the core pixels of a window's output therefore equal the whole-image forward's (up to summation order).

The 8-bit image <-> tile batch moves are the HIP kernels ofasr_tile_gather_u8 / ofasr_tile_scatter_u8 (csrc/tile_io.hip:
ToTensor's / 255 and tensor2img_np's clamp * 255 round, one launch per batch); the network runs on its own HIP kernels,
replayed from one captured graph per window shape (graphed.GraphedEval).

Geometric self-ensemble (`self_ensemble=k`, the "+" of EDSR+ / RCAN+): every batch of windows is run under the first k of
the 8 flips / transposes T_t and the outputs, mapped back, are averaged in fp32 (ops.self_ensemble: csrc/d4.hip).  Tiling
stays exact: T_t of a window that was shifted into the image is the window of T_t(image) at the transformed place, so every
outer window edge is still an image edge or at least `halo` from the core, and the tiled ensemble equals the ensemble of
the whole image.  d4_transform / d4_inverse below are the host definition of T_t.

Video frames (`upscale_yuv420`): a planar 8-bit YUV 4:2:0 frame goes through the same plan with the colour conversion of
video.py inside the two tile moves (ofasr_tile_gather_yuv420 / ofasr_tile_scatter_yuv420, csrc/yuv.hip), so no RGB frame
exists on either side of the network.  The gather decodes at frame coordinates (a window edge never replicates chroma) and
takes the odd origins that a shift by the halo makes; the scatter needs even output rectangles, which an even frame and an
even upscale factor give.  Planes of uint16 are 10-bit frames (video.py, depth 10) and go through the 16-bit twins of
the two kernels (ofasr_tile_gather_yuv420p16 / ofasr_tile_scatter_yuv420p16); the output depth is independent of the
input's (`out_depth`), and 8 -> 10 keeps the precision that the network computed and an 8-bit output rounds away.

Video streams (`yuv420_stream`): consecutive frames often repeat bytes exactly (screen recordings, animation, letterbox
bars, duplicated frames, a codec's skip blocks).  The core of a window's output depends only on the input bytes of that
window, so a window whose support (video.window_support) is unchanged keeps the previous frame's output bytes.
YUV420Stream keeps the previous input planes and the output planes on the GPU, finds the changed windows with
ofasr_window_diff_yuv420, compacts their table rows with ofasr_window_compact (csrc/reuse.hip) and runs only those,
in batches of the full plan's batch size, so that every forward has the shape of the non-reuse path and replays the
same captured graph: the output equals upscale_yuv420's bit for bit.  The comparison is exact, so it does nothing for
camera noise.

Target-size output (`out_size=(TH, TW)`, `resample`): the result is DEFINED as Pillow's Image.resize of the quantised
full-size output (resize.py), and the resize is fused into the scatter (ofasr_tile_resize_scatter_*,
csrc/resize_scatter.hip), so the full-size frame never exists.  With S = scale * L full-size pixels and T target pixels on
an axis, L <= T <= S.  A core covering the full-size pixels [a, b) owns the target pixels [t(a), t(b)), t(p) =
ceil(p T / S) (rounded up to even for YUV planes, capped at T): the cores' rectangles tile the target exactly once.  Those
target pixels read full-size pixels a little outside the core, by at most `extra` input pixels, which plan_resize
computes from the coefficient tables themselves (the largest overhang of [xmin, xmin + count) over the owning core); the
halo becomes radius + extra, so every pixel a window's rectangle reads lies at least `radius` input pixels inside the
window's non-image edges, where the window's output equals the whole-image forward's.  plan_resize checks that for every
window.  Hence tiled = whole, as before.  T = S on both axes is today's plan, halo and kernels, bit for bit.

Content-aware routing (`easy_net`, `easy_threshold`): two networks exported from one supernet share one tile plan (the
larger receptive radius, the lcm of the alignments, the larger activation: routing.shared_plan_params); a window whose
luma activity (routing.py: the sum of absolute differences of neighbouring luma samples inside the window, an exact
integer) is at most the threshold's integer limit runs `easy_net`, every other window `net`.  ofasr_window_activity_* and
ofasr_window_route (csrc/route.hip) classify on the GPU and compact the plan's tables into one list per class; the host
reads the two counts (the one synchronisation routing adds) and runs the batch loop once per class, in batches of the
plan's size, so each network replays the graph of its full-batch shape.  The class is a function of the window's own
bytes, so it composes with window reuse: an unchanged window keeps its class and its output.  There is no blending:
neighbouring cores from different networks can differ at the seam.

Image modes (`upscale_image`, `split_image`, `join_image`): an L, LA or RGBA image keeps its mode (modes.py is the
definition).  ofasr_mode_unpack_u8 makes the RGB image (R = G = B = L; RGBA's colour untouched) that everything above reads,
upscale() runs on it unchanged, and ofasr_mode_pack_u8 (csrc/mode_io.hip) joins its output -- as it is, or as Pillow's
convert("L") of it -- with the SOURCE alpha plane resized straight to the output's size, Pillow's Image.resize bit for
bit.  The alpha does not go through the network.  Three channels take no new kernel: upscale_image is upscale.
"""
import math
from fractions import Fraction

import torch

from . import _C, modes, ops, resize, routing
from .graphed import GraphedEval

LIMIT = 2 ** 31          # no activation of one window reaches 2^31 bytes (fp32); no batched tensor 2^31 elements
MAX_WINDOWS = 65535      # per launch of the tile kernels (grid.y)

_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
_CODES = {torch.float32: _C.F32, torch.bfloat16: _C.BF16, torch.float16: _C.F16}


# ---------------------------------------------------------------------------------------------- network geometry
def _layers(config):
    """the static network as ("conv", kernel extent, out channels) / ("mb", kernel, mid, out) / ("shuffle",) /
    ("unshuffle",) steps, in the order of SRNetS4.forward / SRNetX4.forward (long skips and residual adds do not widen
    the support and are left out)"""
    def conv(c):
        k = c["kernel_size"]
        d = c.get("dilation", 1)
        steps = [("conv", d * (k - 1) + 1, c["out_channels"])]
        if c.get("act_func") == "pixelshuffle":
            steps.append(("shuffle",))
        elif c.get("act_func") == "pixelunshuffle":
            steps.append(("unshuffle",))
        return steps

    def block(c):
        if c["name"] == "MobileInvertedResidualBlock":
            m = c["mobile_inverted_conv"]
            return [("mb", m["kernel_size"], m["mid_channels"], m["out_channels"])]
        return conv(c)

    out = []
    blocks = config["blocks"]
    if config["name"] == "SRNetS4":
        out += conv(config["dec_first_conv_block"])
        for c in blocks[:config["n_mb"]]:
            out += block(c)
        for c in config["dec_final_conv_blocks"]:
            out += conv(c)
        for c in blocks[config["n_mb"]:]:
            out += block(c)
    elif config["name"] == "SRNetX4":
        u, e, d = config["n_unshuffle"], config["n_enc"], config["n_dec"]
        for c in blocks[:u + e]:
            out += block(c)
        for c in config["enc_final_conv_blocks"]:
            out += conv(c)
        out += conv(config["dec_first_conv_block"])
        for c in blocks[u + e:u + e + d]:
            out += block(c)
        for c in config["dec_final_conv_blocks"]:
            out += conv(c)
        for c in blocks[u + e + d:]:
            out += block(c)
    else:
        raise ValueError("not a static SR network config: %r" % config.get("name"))
    out += conv(config["dec_final_output_conv_block"])
    return out


def receptive_radius(config):
    """the largest distance, in input pixels, at which an input pixel can affect an output pixel.  At resolution f
    (layer pixels per input pixel) a k x k conv adds (k - 1) / 2 / f; PixelShuffle(2) doubles f; PixelUnshuffle(2)
    halves it after its 2 x 2 grouping has added up to one pixel of the finer resolution, 1 / f."""
    r, f = Fraction(0), Fraction(1)
    for step in _layers(config):
        if step[0] in ("conv", "mb"):
            r += Fraction(step[1] - 1, 2) / f
        elif step[0] == "shuffle":
            f *= 2
        else:
            r += 1 / f
            f /= 2
    return int(math.ceil(r))


def activation_elems_per_pixel(config):
    """elements of the largest activation per input pixel of a window (the MB blocks' mid tensor counted, as the composite
    path materialises it); for the max S4 sub-network it is the 64 -> 256 conv output before the last PixelShuffle"""
    f, best = Fraction(1), Fraction(3)
    for step in _layers(config):
        if step[0] == "conv":
            best = max(best, step[2] * f * f)
        elif step[0] == "mb":
            best = max(best, max(step[2], step[3]) * f * f)
        elif step[0] == "shuffle":
            f *= 2
        else:
            f /= 2
    return int(math.ceil(best))


def alignment(config):
    """the side multiple an input needs: 2 ** (PixelUnshuffle blocks) for X4, 1 for S4"""
    return 2 ** config.get("n_unshuffle", 0) if config["name"] == "SRNetX4" else 1


def shared_geometry(config_a, config_b):
    """(radius, align, halo, px_elems) of the one tile plan that two static networks can both run
    (routing.shared_plan_params of their receptive radii, alignments and activation sizes); symmetric in its arguments"""
    return routing.shared_plan_params(*((receptive_radius(c), alignment(c), activation_elems_per_pixel(c))
                                        for c in (config_a, config_b)))


# ---------------------------------------------------------------------------------------------- tile plan
def _up(v, m):
    return -(-v // m) * m


def _px(px_elems, scale):
    """activation elements per input pixel of a window: px_elems, or a bound for the networks of this project"""
    return px_elems if px_elems is not None else max(384, 64 * scale * scale, 3 * scale * scale)


class TilePlan(object):
    """windows of one image: all win_h x win_w; windows[i] = (wy, wx, cy, cx, ch, cw): window origin and core rectangle,
    in input pixels.  `batch` is the most windows one batch may hold (no batched tensor reaches 2^31 elements)."""

    def __init__(self, H, W, win_h, win_w, windows, scale, batch):
        self.H, self.W, self.win_h, self.win_w = H, W, win_h, win_w
        self.windows = windows
        self.scale = scale
        self.batch = batch

    def __len__(self):
        return len(self.windows)

    def overhead(self):
        """window pixels / core pixels"""
        return len(self.windows) * self.win_h * self.win_w / float(self.H * self.W)


def _axis(L, core, halo, align, mult):
    """(window side, [(window start, core start, core length)]) along one axis"""
    n = -(-L // core)
    c = _up(-(-L // n), align)         # cores of at most `core`, split evenly
    win = _up(c + 2 * halo, mult)
    if win >= L:                       # the image is no wider than one window: the window is the whole axis
        return L, [(0, 0, L)]
    out = []
    x0 = 0
    while x0 < L:
        out.append((min(max(x0 - halo, 0), L - win), x0, min(c, L - x0)))
        x0 += c
    return win, out


def plan_windows(H, W, core, halo, align=1, scale=4, px_elems=None, height8=False):
    """the tile plan of an H x W input: cores of at most core x core input pixels that tile the image exactly once, each in
    a window of the core plus `halo` on every side, shifted into the image (never padded).  Window sides are multiples
    of `align` (input sides must be, too) and, where the image is wide enough, widths are multiples of 8.  `px_elems` is
    activation_elems_per_pixel(config): it bounds the batch.  `height8`: heights are multiples of 8 too, where the image is
    tall enough (the 8-fold self-ensemble runs the transposed windows as well)."""
    H, W, core, halo, align = int(H), int(W), int(core), int(halo), int(align)
    if H <= 0 or W <= 0:
        raise ValueError("empty image %dx%d" % (H, W))
    if H % align or W % align:
        raise ValueError("this network needs input sides that are multiples of %d (2 ** PixelUnshuffle blocks); got %dx%d"
                         % (align, H, W))
    if core < align:
        raise ValueError("core %d is smaller than the alignment %d" % (core, align))
    core = core // align * align
    halo = _up(max(halo, 0), align)
    m8 = align * 8 // math.gcd(align, 8)
    win_h, rows = _axis(H, core, halo, align, m8 if height8 else align)
    win_w, cols = _axis(W, core, halo, align, m8)
    windows = [(wy, wx, cy, cx, ch, cw) for (wy, cy, ch) in rows for (wx, cx, cw) in cols]
    batch = max(1, min(MAX_WINDOWS, (LIMIT - 1) // (_px(px_elems, scale) * win_h * win_w)))
    return TilePlan(H, W, win_h, win_w, windows, scale, batch)


class ResizePlan(TilePlan):
    """a TilePlan for a target size: out_h x out_w, the filter, targets[i] = (dy, dx, eh, ew), the target rectangle that
    window i owns (possibly empty), `extra` (input pixels added to the halo), `halo`, and `core`, the core side the
    windows were planned with (plan_resize may have shrunk the one it was given)"""

    def __init__(self, plan, out_h, out_w, resample, even, targets, extra, halo, radius, core=None):
        TilePlan.__init__(self, plan.H, plan.W, plan.win_h, plan.win_w, plan.windows, plan.scale, plan.batch)
        self.out_h, self.out_w, self.resample, self.even = out_h, out_w, resample, even
        self.targets, self.extra, self.halo, self.radius, self.core = targets, extra, halo, radius, core
        self._device_tables = {}

    def tables(self, depth=8):
        """(vertical, horizontal) coefficient tables of a sample depth (numpy int32, resize.axis_table)"""
        return (resize.axis_table(self.H * self.scale, self.out_h, self.resample, depth),
                resize.axis_table(self.W * self.scale, self.out_w, self.resample, depth))

    def device_tables(self, depth, device):
        """tables(depth) as int32 tensors on `device`, uploaded once per depth and device and kept with the plan"""
        key = (depth, str(device))
        if key not in self._device_tables:
            self._device_tables[key] = tuple(torch.from_numpy(t).to(device) for t in self.tables(depth))
        return self._device_tables[key]


def check_out_size(H, W, scale, out_size, even=False):
    """(TH, TW) of an `out_size` for an H x W input, or a ValueError that names the allowed range"""
    try:
        TH, TW = (int(v) for v in out_size)
    except (TypeError, ValueError):
        raise ValueError("out_size must be (height, width), got %r" % (out_size,))
    if not (H <= TH <= H * scale and W <= TW <= W * scale):
        raise ValueError("out_size %dx%d is outside what a %dx%d input allows: width %d .. %d, height %d .. %d (never "
                         "smaller than the input, never larger than the network's x%d output)"
                         % (TW, TH, W, H, W, W * scale, H, H * scale, scale))
    if even and (TH % 2 or TW % 2):
        raise ValueError("a YUV 4:2:0 output needs even sides, got out_size %dx%d" % (TW, TH))
    if scale > 4 and (TH, TW) != (H * scale, W * scale):
        raise ValueError("out_size needs an upscale factor of at most 4 (the resampling scatter holds the source rows of "
                         "a 4 : 1 reduction), this network's is %d" % scale)
    return TH, TW


def _axis_targets(cores, s, T, L, even):
    """[(t0, t1)] per core (core start, core length) of an axis of L input pixels"""
    S = s * L
    return [(resize.target_edge(c0 * s, S, T, even), resize.target_edge((c0 + cl) * s, S, T, even)) for (c0, cl) in cores]


def _axis_extra(cores, s, T, L, even, table):
    """the largest overhang, in input pixels rounded up, of the source range a core's target pixels read over the core"""
    over = 0
    for (c0, cl), (t0, t1) in zip(cores, _axis_targets(cores, s, T, L, even)):
        need = resize.needed_range(table, t0, t1)
        if need is not None:
            over = max(over, c0 * s - need[0], need[1] - (c0 + cl) * s)
    return -(-over // s)


def attach_targets(plan, out_h, out_w, resample, even, radius, extra=0, halo=0, core=None):
    """the ResizePlan of a TilePlan: each window's target rectangle, after checking that the full-size pixels it reads lie
    inside the window's exact region (the window minus radius * scale on every side that is not an image edge)"""
    s = plan.scale
    vt = resize.axis_table(plan.H * s, out_h, resample)
    ht = resize.axis_table(plan.W * s, out_w, resample)
    targets = []
    for (wy, wx, cy, cx, ch, cw) in plan.windows:
        (ty0, ty1), = _axis_targets([(cy, ch)], s, out_h, plan.H, even)
        (tx0, tx1), = _axis_targets([(cx, cw)], s, out_w, plan.W, even)
        for tab, t0, t1, w0, wl, L, what in ((vt, ty0, ty1, wy, plan.win_h, plan.H, "rows"),
                                             (ht, tx0, tx1, wx, plan.win_w, plan.W, "columns")):
            need = resize.needed_range(tab, t0, t1)
            if need is None:
                continue
            lo = (w0 + (radius if w0 > 0 else 0)) * s
            hi = (w0 + wl - (radius if w0 + wl < L else 0)) * s
            if need[0] < lo or need[1] > hi:
                raise ValueError("the %s [%d, %d) that the target of window (%d, %d) reads leave its exact region [%d, %d)"
                                 % (what, need[0], need[1], wy, wx, lo, hi))
        targets.append((ty0, tx0, ty1 - ty0, tx1 - tx0))
    return ResizePlan(plan, out_h, out_w, resample, even, targets, extra, halo, radius, core)


def plan_resize(H, W, out_size, resample, core, radius, align=1, scale=4, px_elems=None, height8=False, even=False):
    """the tile plan of an H x W input for the target size out_size = (TH, TW): plan_windows with the halo widened by
    what the filter reads outside a core (see the module docstring).  TH x TW equal to the network's own output size:
    plan_windows(H, W, core, radius rounded up to align, ...) itself, today's plan.  The wider halo must not push a window
    over the 2^31-byte limit that `core` was sized for (default_core knows the plain halo only): where the plain plan's
    window keeps an fp32 activation below LIMIT and the widened one does not, the core shrinks, by the side multiple at
    a time, until it does again; a core that cannot shrink further is a ValueError."""
    resize.check_filter(resample)
    H, W, s, core, align = int(H), int(W), int(scale), int(core), int(align)
    TH, TW = check_out_size(H, W, s, out_size, even)
    halo0 = _up(max(int(radius), 0), align)
    base = plan_windows(H, W, core, halo0, align, s, px_elems, height8)
    if (TH, TW) == (H * s, W * s):
        return base
    px4 = 4 * _px(px_elems, s)
    fits = px4 * base.win_h * base.win_w < LIMIT
    step = align * 8 // math.gcd(align, 8)
    tabs = (resize.axis_table(H * s, TH, resample), resize.axis_table(W * s, TW, resample))
    while True:
        extra = 0
        for L, T, tab, cores in ((H, TH, tabs[0], sorted(set((w[2], w[4]) for w in base.windows))),
                                 (W, TW, tabs[1], sorted(set((w[3], w[5]) for w in base.windows)))):
            if len(cores) > 1:          # one core is the whole axis: nothing lies outside it
                extra = max(extra, _axis_extra(cores, s, T, L, even, tab))
        halo = _up(int(radius) + extra, align)
        plan = plan_windows(H, W, core, halo, align, s, px_elems, height8)
        if not fits or px4 * plan.win_h * plan.win_w < LIMIT:
            return attach_targets(plan, TH, TW, resample, even, int(radius), extra, halo, core)
        if core - step < max(align, 1):
            raise ValueError("with the halo of %d that out_size %dx%d (%s) needs, a window of core %d is %dx%d and an fp32 "
                             "activation of it would reach 2^31 bytes, and the core cannot shrink further: there is no "
                             "core (--core) for this network at this target size"
                             % (halo, TW, TH, resample, core, plan.win_w, plan.win_h))
        core -= step
        base = plan_windows(H, W, core, halo0, align, s, px_elems, height8)


def default_core(halo, align, px_elems):
    """the largest core (a multiple of 8 and of align) whose window keeps every fp32 activation below 2^31 bytes"""
    m = align * 8 // math.gcd(align, 8)
    side = int(math.isqrt((LIMIT - 1) // (4 * px_elems)))
    core = (side - 2 * _up(halo, align)) // m * m
    while core > m and 4 * px_elems * _up(core + 2 * halo, m) ** 2 >= LIMIT:
        core -= m
    if core < m:
        raise ValueError("the network's receptive radius (%d) leaves no room for a core under the 2^31-byte limit" % halo)
    return core


# ---------------------------------------------------------------------------------------------- kernels
def _origin_table(origins, name, shaped=True):
    """the window count of an int64 origin table on the GPU; `shaped`: its [n, 2] shape is part of the caller's contract"""
    bad = origins.dtype != torch.int64 or not origins.is_cuda or not origins.is_contiguous()
    if shaped:
        bad = bad or origins.dim() != 2 or origins.size(1) != 2
    if bad:
        raise ValueError("%s needs a contiguous int64 origin table%s on the GPU" % (name, " [n, 2]" if shaped else ""))
    return origins.size(0)


def _scatter_table(table, src, name, shaped=False):
    """the checks of a scatter table against its source batch; `shaped`: [n, 6] with n >= 1 is part of the contract"""
    bad = table.dtype != torch.int64 or not table.is_cuda or not table.is_contiguous() or table.size(0) > src.size(0)
    if shaped:
        bad = bad or table.dim() != 2 or table.size(1) != 6 or table.size(0) < 1
    if bad:
        raise ValueError("%s needs a contiguous int64 table%s on the GPU, one row per source window at most"
                         % (name, " [n, 6]" if shaped else ""))


def _call_depth(base, depth, head, tail):
    """the 8-bit entry point `base` as it is, or its 16-bit twin `base`p16 with `depth` between head and tail"""
    name = base if depth == 8 else base + "p16"
    _C.check(getattr(_C.lib(), name)(*(head + (() if depth == 8 else (depth,)) + tail)), name)


def tile_gather(img, origins, h, w, dtype, out=None):
    """img: HWC uint8 [H, W, 3] on the GPU; origins: int64 [n, 2] (y0, x0) on the GPU -> [n, 3, h, w] of dtype,
    u8 / 255 (fp32) then cast (ofasr_tile_gather_u8)"""
    ops._gpu(img)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.size(2) != 3 or not img.is_contiguous():
        raise ValueError("tile_gather needs a contiguous HWC uint8 RGB image")
    n = _origin_table(origins, "tile_gather", shaped=False)
    if out is None:
        out = torch.empty(n, 3, h, w, dtype=dtype, device=img.device)
    _C.check(_C.lib().ofasr_tile_gather_u8(img.data_ptr(), img.size(0), img.size(1), origins.data_ptr(), n, h, w,
                                           out.data_ptr(), _CODES[out.dtype], ops._stream()), "ofasr_tile_gather_u8")
    return out


def tile_scatter(src, table, img, max_eh, max_ew):
    """src: network output [n, 3, sh, sw] (contiguous, fp32 / bf16 / f16); table: int64 [n, 6] (sy, sx, dy, dx, eh, ew)
    on the GPU; writes round_half_even(clamp(v, 0, 1) * 255) into the HWC uint8 image img (ofasr_tile_scatter_u8)"""
    ops._gpu(src)
    if not src.is_contiguous() or src.dim() != 4 or src.size(1) != 3:
        raise ValueError("tile_scatter needs a contiguous [n, 3, h, w] source")
    if img.dtype != torch.uint8 or img.dim() != 3 or img.size(2) != 3 or not img.is_contiguous():
        raise ValueError("tile_scatter needs a contiguous HWC uint8 RGB destination")
    _scatter_table(table, src, "tile_scatter")
    _C.check(_C.lib().ofasr_tile_scatter_u8(src.data_ptr(), table.size(0), src.size(2), src.size(3), _CODES[src.dtype],
                                            table.data_ptr(), img.data_ptr(), img.size(0), img.size(1), max_eh, max_ew,
                                            ops._stream()), "ofasr_tile_scatter_u8")
    return img


def tile_gather_yuv420(y, u, v, origins, h, w, dtype, matrix="bt601", full_range=False, out=None):
    """planar YUV 4:2:0 frame (uint8 GPU planes y [H, W], u, v [H/2, W/2]) -> [n, 3, h, w] of dtype: the RGB of the
    windows at `origins` (int64 [n, 2] on the GPU; odd origins are fine), decoded at frame coordinates, / 255 (fp32), cast
    -- tile_gather(ops.yuv420_to_rgb_u8(y, u, v)) bit for bit without the RGB frame (ofasr_tile_gather_yuv420).  uint16
    planes are a 10-bit frame: the decode of depth 10, / 1023 (ofasr_tile_gather_yuv420p16)."""
    H, W = ops.yuv420_planes(y, u, v, "tile_gather_yuv420")
    n = _origin_table(origins, "tile_gather_yuv420", shaped=False)
    if out is None:
        out = torch.empty(n, 3, h, w, dtype=dtype, device=y.device)
    depth = ops.YUV_DEPTHS[y.dtype]
    coeffs = ops.yuv_table(matrix, full_range, False, depth)
    _call_depth("ofasr_tile_gather_yuv420", depth, (y.data_ptr(), u.data_ptr(), v.data_ptr(), H, W),
                (coeffs, origins.data_ptr(), n, h, w, out.data_ptr(), _CODES[out.dtype], ops._stream()))
    return out


def tile_scatter_yuv420(src, table, y, u, v, max_eh, max_ew, matrix="bt601", full_range=False):
    """src: network output [n, 3, sh, sw]; table: int64 [n, 6] (sy, sx, dy, dx, eh, ew) on the GPU, dy / dx / eh / ew even
    (the kernel clears their low bit); quantises as tile_scatter does and encodes every 2x2 block of the extents into the
    planes y [OH, OW], u, v [OH/2, OW/2] (ofasr_tile_scatter_yuv420).  uint16 planes are a 10-bit frame: quantised to
    round_half_even(clamp(v, 0, 1) * 1023) and encoded at depth 10 (ofasr_tile_scatter_yuv420p16)."""
    ops._gpu(src)
    if not src.is_contiguous() or src.dim() != 4 or src.size(1) != 3:
        raise ValueError("tile_scatter_yuv420 needs a contiguous [n, 3, h, w] source")
    OH, OW = ops.yuv420_planes(y, u, v, "tile_scatter_yuv420")
    _scatter_table(table, src, "tile_scatter_yuv420")
    depth = ops.YUV_DEPTHS[y.dtype]
    coeffs = ops.yuv_table(matrix, full_range, True, depth)
    _call_depth("ofasr_tile_scatter_yuv420", depth,
                (src.data_ptr(), table.size(0), src.size(2), src.size(3), _CODES[src.dtype], table.data_ptr()),
                (coeffs, y.data_ptr(), u.data_ptr(), v.data_ptr(), OH, OW, max_eh, max_ew, ops._stream()))
    return y, u, v


def _resize_args(name, src, table, vtab, htab, TH, TW):
    ops._gpu(src)
    if not src.is_contiguous() or src.dim() != 4 or src.size(1) != 3:
        raise ValueError("%s needs a contiguous [n, 3, h, w] source" % name)
    _scatter_table(table, src, name, shaped=True)
    for t, rows, what in ((vtab, TH, "vertical"), (htab, TW, "horizontal")):
        if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or t.size(0) != rows or \
                not 3 <= t.size(1) <= 2 + resize.MAX_TAPS:
            raise ValueError("%s needs a contiguous int32 %s coefficient table [%d, 2 + taps] on the GPU, taps <= %d"
                             % (name, what, rows, resize.MAX_TAPS))


def tile_resize_scatter(src, table, vtab, htab, img, max_eh, max_ew):
    """src: network output [n, 3, sh, sw]; table: int64 [n, 6] (oy, ox, dy, dx, eh, ew) on the GPU: each window's origin in
    the full-size output and its target rectangle; vtab / htab: int32 coefficient tables [TH, 2 + kh] / [TW, 2 + kw] on the
    GPU (resize.axis_table, depth 8); writes Pillow's resize of the quantised full-size output into the rectangles of the
    HWC uint8 image img [TH, TW, 3] (ofasr_tile_resize_scatter_u8)"""
    if img.dtype != torch.uint8 or img.dim() != 3 or img.size(2) != 3 or not img.is_contiguous():
        raise ValueError("tile_resize_scatter needs a contiguous HWC uint8 RGB destination")
    _resize_args("tile_resize_scatter", src, table, vtab, htab, img.size(0), img.size(1))
    _C.check(_C.lib().ofasr_tile_resize_scatter_u8(src.data_ptr(), table.size(0), src.size(2), src.size(3), _CODES[src.dtype],
                                                   table.data_ptr(), vtab.data_ptr(), vtab.size(1) - 2, htab.data_ptr(),
                                                   htab.size(1) - 2, img.data_ptr(), img.size(0), img.size(1), max_eh, max_ew,
                                                   ops._stream()), "ofasr_tile_resize_scatter_u8")
    return img


def tile_resize_scatter_yuv420(src, table, vtab, htab, y, u, v, max_eh, max_ew, matrix="bt601", full_range=False):
    """the same into the planes y [TH, TW], u, v [TH/2, TW/2] through the 2x2 encode of tile_scatter_yuv420: dy, dx, eh,
    ew even (the kernel clears their low bit).  uint16 planes are a 10-bit frame: quantised to 1023 levels, resampled
    with the tables of depth 10 (20 coefficient bits) and encoded at depth 10 (ofasr_tile_resize_scatter_yuv420 /
    _yuv420p16)"""
    TH, TW = ops.yuv420_planes(y, u, v, "tile_resize_scatter_yuv420")
    _resize_args("tile_resize_scatter_yuv420", src, table, vtab, htab, TH, TW)
    depth = ops.YUV_DEPTHS[y.dtype]
    coeffs = ops.yuv_table(matrix, full_range, True, depth)
    head = (src.data_ptr(), table.size(0), src.size(2), src.size(3), _CODES[src.dtype], table.data_ptr(), vtab.data_ptr(),
            vtab.size(1) - 2, htab.data_ptr(), htab.size(1) - 2)
    tail = (coeffs, y.data_ptr(), u.data_ptr(), v.data_ptr(), TH, TW, max_eh, max_ew, ops._stream())
    _call_depth("ofasr_tile_resize_scatter_yuv420", depth, head, tail)
    return y, u, v


def window_diff_slabs(h, w):
    """row slabs per window of window_diff_yuv420's flag table (ofasr_window_diff_slabs; host only)"""
    return int(_C.lib().ofasr_window_diff_slabs(h, w))


def window_diff_yuv420(y, u, v, py, pu, pv, origins, h, w, flags=None):
    """two planar YUV 4:2:0 frames of one size (current y, u, v and previous py, pu, pv: uint8 GPU planes) and the
    int64 origin table [n, 2] of h x w windows on the GPU -> int32 flags [n, window_diff_slabs(h, w)]: a window's row is
    non-zero iff any byte of its support (video.window_support) differs between the frames (ofasr_window_diff_yuv420;
    host definition: video.changed_windows_host).  Two frames of uint16 planes alike (ofasr_window_diff_yuv420p16)."""
    H, W = ops.yuv420_planes(y, u, v, "window_diff_yuv420")
    if ops.yuv420_planes(py, pu, pv, "window_diff_yuv420") != (H, W) or py.dtype != y.dtype:
        raise ValueError("window_diff_yuv420 needs two frames of one size and dtype")
    n = _origin_table(origins, "window_diff_yuv420")
    S = window_diff_slabs(h, w)
    if flags is None:
        flags = torch.empty(n, max(S, 1), dtype=torch.int32, device=y.device)
    elif flags.dtype != torch.int32 or not flags.is_cuda or not flags.is_contiguous() or flags.numel() != n * S:
        raise ValueError("window_diff_yuv420 needs contiguous int32 flags [n, %d] on the GPU" % S)
    _call_depth("ofasr_window_diff_yuv420", ops.YUV_DEPTHS[y.dtype],
                (y.data_ptr(), u.data_ptr(), v.data_ptr(), py.data_ptr(), pu.data_ptr(), pv.data_ptr(), H, W),
                (origins.data_ptr(), n, h, w, flags.data_ptr(), ops._stream()))
    return flags


def window_compact(flags, origins, table, batch, out=None):
    """flags: int32 [n, S] from window_diff_yuv420; origins [n, 2] and table [n, 6]: the plan's int64 tables on the GPU ->
    (origins of the changed windows in plan order, filled up to a multiple of `batch` by repeating the last one
    [ceil(n / batch) * batch, 2]; their table rows [n, 6]; their plan indices [n]; their number, int64 [1]), all on the
    GPU; rows past the count (past the filled count for the origins) are not written.  One workgroup, no
    synchronisation (ofasr_window_compact)."""
    ops._gpu(flags)
    n = origins.size(0)
    batch = int(batch)
    for t, cols in ((origins, 2), (table, 6)):
        if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2 or tuple(t.shape) != (n, cols):
            raise ValueError("window_compact needs contiguous int64 tables [n, 2] and [n, 6] on the GPU")
    if flags.dtype != torch.int32 or not flags.is_contiguous() or flags.dim() != 2 or flags.size(0) != n:
        raise ValueError("window_compact needs contiguous int32 flags [n, S]")
    if batch < 1:
        raise ValueError("window_compact needs a positive batch size")
    rows = -(-n // batch) * batch
    if out is None:
        out = (torch.zeros(rows, 2, dtype=torch.int64, device=flags.device),
               torch.zeros(n, 6, dtype=torch.int64, device=flags.device),
               torch.zeros(n, dtype=torch.int64, device=flags.device),
               torch.zeros(1, dtype=torch.int64, device=flags.device))
    o, t, idx, count = out
    if (tuple(o.shape), tuple(t.shape), tuple(idx.shape), tuple(count.shape)) != ((rows, 2), (n, 6), (n,), (1,)) or \
            any(b.dtype != torch.int64 or not b.is_cuda or not b.is_contiguous() for b in out):
        raise ValueError("window_compact needs contiguous int64 outputs [%d, 2], [%d, 6], [%d], [1] on the GPU" % (rows, n, n))
    _C.check(_C.lib().ofasr_window_compact(flags.data_ptr(), flags.size(1), origins.data_ptr(), table.data_ptr(), n, batch,
                                           o.data_ptr(), t.data_ptr(), idx.data_ptr(), count.data_ptr(), ops._stream()),
             "ofasr_window_compact")
    return out


def window_activity_slabs(h, w):
    """row slabs per window of window_activity's partial table (ofasr_window_activity_slabs; host only)"""
    return int(_C.lib().ofasr_window_activity_slabs(h, w))


def window_activity(src, origins, h, w, partial=None):
    """src: an HWC uint8 RGB image [H, W, 3] or one 2-D luma plane (uint8, or uint16: depth 10) on the GPU; origins: int64
    [n, 2] of h x w windows on the GPU -> int64 partial [n, window_activity_slabs(h, w)]: a window's row sums to its
    luma activity A (routing.window_activity_host; ofasr_window_activity_rgb8 / ofasr_window_activity_plane)"""
    ops._gpu(src)
    if not src.is_contiguous() or not ((src.dim() == 3 and src.size(2) == 3 and src.dtype == torch.uint8) or
                                       (src.dim() == 2 and src.dtype in ops.YUV_DEPTHS)):
        raise ValueError("window_activity needs a contiguous HWC uint8 RGB image or a 2-D uint8 / uint16 plane, got %s %s"
                         % (tuple(src.shape), src.dtype))
    n = _origin_table(origins, "window_activity")
    S = window_activity_slabs(h, w)
    if partial is None:
        partial = torch.empty(n, max(S, 1), dtype=torch.int64, device=src.device)
    elif partial.dtype != torch.int64 or not partial.is_cuda or not partial.is_contiguous() or partial.numel() != n * S:
        raise ValueError("window_activity needs contiguous int64 partials [n, %d] on the GPU" % S)
    if src.dim() == 3:
        _C.check(_C.lib().ofasr_window_activity_rgb8(src.data_ptr(), src.size(0), src.size(1), origins.data_ptr(), n, h, w,
                                                     partial.data_ptr(), ops._stream()), "ofasr_window_activity_rgb8")
    else:
        _C.check(_C.lib().ofasr_window_activity_plane(src.data_ptr(), src.size(0), src.size(1), ops.YUV_DEPTHS[src.dtype],
                                                      origins.data_ptr(), n, h, w, partial.data_ptr(), ops._stream()),
                 "ofasr_window_activity_plane")
    return partial


def window_route(partial, limit, origins, table, batch, changed=None, out=None):
    """partial: int64 [n, S] from window_activity; limit: the integer of routing.activity_limit; origins [n, 2] and table
    [n, 6]: the plan's int64 tables on the GPU; changed: None, or the int32 flags [n, S'] of window_diff_yuv420 (a window
    whose flags are all zero goes into neither list) -> (origins [2, ceil(n / batch) * batch, 2], table rows [2, n, 6],
    plan indices [2, n], counts [2]), index 0 the hard windows (A > limit), index 1 the easy ones, each in plan order and
    its origins filled up to a multiple of `batch` by repeating the class's last window; rows past those are not
    written.  One workgroup, no synchronisation (ofasr_window_route)."""
    ops._gpu(partial)
    n = _origin_table(origins, "window_route")
    batch, limit = int(batch), int(limit)
    if table.dtype != torch.int64 or not table.is_cuda or not table.is_contiguous() or tuple(table.shape) != (n, 6):
        raise ValueError("window_route needs a contiguous int64 table [n, 6] on the GPU")
    if partial.dtype != torch.int64 or not partial.is_contiguous() or partial.dim() != 2 or partial.size(0) != n:
        raise ValueError("window_route needs contiguous int64 partials [n, S]")
    if changed is not None and (changed.dtype != torch.int32 or not changed.is_cuda or not changed.is_contiguous() or
                                changed.dim() != 2 or changed.size(0) != n):
        raise ValueError("window_route needs contiguous int32 changed flags [n, S] on the GPU")
    if batch < 1:
        raise ValueError("window_route needs a positive batch size")
    if not -1 <= limit <= routing.INT64_MAX:
        raise ValueError("window_route needs a limit in -1 .. 2^63 - 1")
    rows = -(-n // batch) * batch
    if out is None:
        out = (torch.zeros(2, rows, 2, dtype=torch.int64, device=partial.device),
               torch.zeros(2, n, 6, dtype=torch.int64, device=partial.device),
               torch.zeros(2, n, dtype=torch.int64, device=partial.device),
               torch.zeros(2, dtype=torch.int64, device=partial.device))
    o, t, idx, count = out
    if (tuple(o.shape), tuple(t.shape), tuple(idx.shape), tuple(count.shape)) != ((2, rows, 2), (2, n, 6), (2, n), (2,)) or \
            any(b.dtype != torch.int64 or not b.is_cuda or not b.is_contiguous() for b in out):
        raise ValueError("window_route needs contiguous int64 outputs [2, %d, 2], [2, %d, 6], [2, %d], [2] on the GPU"
                         % (rows, n, n))
    _C.check(_C.lib().ofasr_window_route(partial.data_ptr(), partial.size(1), limit,
                                         None if changed is None else changed.data_ptr(),
                                         0 if changed is None else changed.size(1), origins.data_ptr(), table.data_ptr(), n,
                                         batch, o.data_ptr(), t.data_ptr(), idx.data_ptr(), count.data_ptr(), ops._stream()),
             "ofasr_window_route")
    return out


# ---------------------------------------------------------------------------------------------- self-ensemble
def _d4_index(t):
    if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < 8:
        raise ValueError("the transform index must be an integer in 0..7, got %r" % (t,))
    return t


def d4_transform(x, t):
    """T_t(x) on the last two axes: bit 0 of t flips W, bit 1 flips H, bit 2 transposes, applied in that order.  Pure torch:
    the definition the HIP kernels (ops.d4_apply / ops.d4_accumulate) are tested against."""
    t = _d4_index(t)
    if t & 1:
        x = x.flip(-1)
    if t & 2:
        x = x.flip(-2)
    if t & 4:
        x = x.transpose(-1, -2)
    return x.contiguous()


def d4_inverse(x, t):
    """T_t^{-1}(x): the steps of d4_transform undone in reverse order"""
    t = _d4_index(t)
    if t & 4:
        x = x.transpose(-1, -2)
    if t & 2:
        x = x.flip(-2)
    if t & 1:
        x = x.flip(-1)
    return x.contiguous()


# ---------------------------------------------------------------------------------------------- upscaler
class TiledUpscaler(object):
    """Tiled inference of a static SR network (SRNetS4 / SRNetX4 on the GPU; put into eval mode here).

    upscale(img) takes an HWC uint8 RGB image (CPU or GPU tensor, or numpy array) and returns the HWC uint8 output on the
    GPU.  Per batch of windows: gather (HIP), the network (replayed from one captured graph per window shape when
    `graphed`; the last batch is padded by repeating a window), scatter of the cores (HIP).  `core` = None: the largest
    core that keeps every fp32 activation of a window below 2^31 bytes; `batch` = None: as many windows per batch as
    keep every batched tensor below 2^31 elements, spread evenly over the batches.  `self_ensemble` = k in {1, 2, 4, 8}:
    every batch runs under the first k flips / transposes and the fp32 mean of the mapped-back outputs is what is
    scattered (ops.self_ensemble); k = 8 plans window heights as multiples of 8 as well and replays two graphs, one per
    window orientation.

    `easy_net` and `easy_threshold` (both or neither) switch content-aware routing on: a window whose mean absolute luma
    difference (routing.py, in 8-bit levels) is at most `easy_threshold` runs `easy_net`, a cheaper export with the same
    upscale factor, every other window `net`.  The threshold is a number or the decimal string the user wrote (the limit
    is computed from the decimal exactly); window_activity() shows the measure per window and route_stats the counts of
    the last call.  Both networks share one plan (the larger radius, the lcm of the alignments)."""

    def __init__(self, net, core=None, batch=None, mix_prec="f32", graphed=True, self_ensemble=1, easy_net=None,
                 easy_threshold=None):
        if mix_prec not in _DTYPES:
            raise ValueError("mix_prec must be one of %s" % sorted(_DTYPES))
        if isinstance(self_ensemble, bool) or self_ensemble not in ops.ENSEMBLE_SIZES:
            raise ValueError("self_ensemble must be one of %s, got %r" % (ops.ENSEMBLE_SIZES, self_ensemble))
        self.self_ensemble = int(self_ensemble)
        self.net = net.eval()
        self.config = net.config
        self.scale = int(self.config["upscale"])
        if self.scale != self.config["upscale"] or self.scale < 1:
            raise ValueError("tiled upscaling needs an integer upscale factor, got %r" % self.config["upscale"])
        self.align = alignment(self.config)
        self.radius = receptive_radius(self.config)
        self.halo = _up(self.radius, self.align)
        self.px_elems = activation_elems_per_pixel(self.config)
        if (easy_net is None) != (easy_threshold is None):
            raise ValueError("routing needs both easy_net and easy_threshold (or neither)")
        self.easy_net = self.easy_threshold = None
        self.route_stats = None
        self._limits = {}
        if easy_net is not None:
            routing.activity_limit(easy_threshold, 1, 2)        # refuses NaN and what is not a number now
            if easy_net.config["upscale"] != self.config["upscale"]:
                raise ValueError("the two networks of a routed upscaler need the same upscale factor, got x%s and x%s"
                                 % (self.config["upscale"], easy_net.config["upscale"]))
            devs = [next(m.parameters()).device for m in (net, easy_net)]
            if devs[0] != devs[1]:
                raise ValueError("the two networks of a routed upscaler must be on the same device, got %s and %s"
                                 % (devs[0], devs[1]))
            self.easy_net, self.easy_threshold = easy_net.eval(), easy_threshold
            self.radius, self.align, self.halo, self.px_elems = shared_geometry(self.config, easy_net.config)
        self.core = int(core) if core else default_core(self.halo, self.align, self.px_elems)
        self.batch = batch
        self.dtype = _DTYPES[mix_prec]
        self.autocast_dtype = None if mix_prec == "f32" else self.dtype
        self.graphed = GraphedEval(net, autocast_dtype=self.autocast_dtype, copy_output=False) if graphed else None
        self.graphed_easy = GraphedEval(easy_net, autocast_dtype=self.autocast_dtype, copy_output=False) \
            if graphed and easy_net is not None else None
        self._plans = {}
        self._alpha_tables = {}

    def plan(self, H, W, out_size=None, resample="lanczos", even=False):
        """the tile plan of an H x W input; with `out_size` = (TH, TW) the ResizePlan of that target (kept: its tables
        take a pass over every target row and column), which for TH x TW = the network's own size is the plain plan.
        Up to 8 plans are kept and all are dropped when a ninth comes, with their device tables: a directory of images
        of more than 8 sizes recomputes and uploads its tables again each time round, a video never does."""
        if out_size is None:
            return plan_windows(H, W, self.core, self.halo, self.align, self.scale, self.px_elems,
                                height8=self.self_ensemble == 8)
        key = (int(H), int(W), tuple(int(v) for v in out_size), resample, bool(even))
        if key not in self._plans:
            if len(self._plans) >= 8:
                self._plans.clear()
            self._plans[key] = plan_resize(H, W, out_size, resample, self.core, self.radius, self.align, self.scale,
                                           self.px_elems, self.self_ensemble == 8, even)
        return self._plans[key]

    def _whole_resize_plan(self, H, W, out_size, resample, even):
        resize.check_filter(resample)
        TH, TW = check_out_size(H, W, self.scale, out_size, even)
        plan = self._whole_plan(H, W)
        if (TH, TW) == (H * self.scale, W * self.scale):
            return plan
        return attach_targets(plan, TH, TW, resample, even, self.radius)

    def _whole_plan(self, H, W):
        if H % self.align or W % self.align:
            raise ValueError("this network needs input sides that are multiples of %d; got %dx%d" % (self.align, H, W))
        if 4 * self.px_elems * H * W >= LIMIT:
            raise ValueError("a %dx%d image is too large for one forward (an fp32 activation would reach 2^31 bytes): "
                             "use the tiled path" % (H, W))
        return TilePlan(H, W, H, W, [(0, 0, 0, 0, H, W)], self.scale, 1)

    def _forward(self, x, easy=False):
        # A window's output must not depend on the shape of the batch it was computed in: that is what makes tiling, and
        # reuse between frames, exact.  The fused 16-bit MB kernel breaks it on small inputs: a launch of fewer tiles than
        # CUs spreads each tile's mid-channel chunks over several workgroups (csrc/mbfused.hip, mf_plan) and then sums
        # them in another order, and how many tiles a launch has depends on the batch.  So the upscaler's forwards (and
        # the graphs captured from them) run with that split off; it never applied to launches of more than 128 tiles,
        # which is every batch of real video windows.
        split = _C.lib().ofasr_debug_mbfused_split(0) if self.autocast_dtype is not None else None
        try:
            if self.graphed is not None:
                return (self.graphed_easy if easy else self.graphed)(x)
            with torch.autocast("cuda", dtype=self.autocast_dtype or torch.bfloat16,
                                enabled=self.autocast_dtype is not None):
                return (self.easy_net if easy else self.net)(x)
        finally:
            if split is not None:
                _C.lib().ofasr_debug_mbfused_split(split)

    def _image(self, img):
        if not torch.is_tensor(img):
            img = torch.from_numpy(img)
        if img.dtype != torch.uint8 or img.dim() != 3 or img.size(2) != 3:
            raise ValueError("upscale takes an HWC uint8 RGB image, got %s %s" % (tuple(img.shape), img.dtype))
        dev = next(self.net.parameters()).device
        if dev.type != "cuda":
            raise _C.OfasrError("TiledUpscaler needs the network on the GPU")
        return img.to(dev).contiguous()

    def _run(self, img, whole, sink, plan=None):
        """run every batch of the plan; sink(y, real, tables, plan) consumes the network output of a batch"""
        img = self._image(img)
        return self._run_windows(img.size(0), img.size(1), img.device, whole, sink,
                                 lambda origins, h, w: tile_gather(img, origins, h, w, self.dtype), plan, luma=img)

    def _batching(self, plan):
        """(batches, windows per batch) of a plan: as many windows per batch as the plan and `batch` allow, spread evenly"""
        n = len(plan)
        cap = min(plan.batch, int(self.batch)) if self.batch else plan.batch
        nb = -(-n // cap)
        return nb, -(-n // nb)

    def _tables(self, plan, device):
        """the plan's device tables: window origins [nb * B, 2], the last batch padded by repeating a window, and the
        scatter rows [n, 6] = (sy, sx, dy, dx, eh, ew) in output pixels; for a ResizePlan the rows of the resampling
        scatter, (oy, ox, dy, dx, eh, ew): the window's origin in full-size pixels and its target rectangle"""
        s = self.scale
        nb, B = self._batching(plan)
        wins = plan.windows + [plan.windows[-1]] * (nb * B - len(plan))
        origins = torch.tensor([[wy, wx] for (wy, wx, _, _, _, _) in wins], dtype=torch.int64).to(device)
        if isinstance(plan, ResizePlan):
            rows = [[w[0] * s, w[1] * s] + list(t) for w, t in zip(plan.windows, plan.targets)]
        else:
            rows = [[(cy - wy) * s, (cx - wx) * s, cy * s, cx * s, ch * s, cw * s] for (wy, wx, cy, cx, ch, cw) in plan.windows]
        return origins, torch.tensor(rows, dtype=torch.int64).to(device)

    def _run_batches(self, plan, origins, table, n, B, sink, gather, wins=None, easy=False):
        """the batch loop: the first n rows of `origins` (padded to a multiple of B) / `table` in batches of B windows.
        `wins`: the plan windows behind the rows, where the host knows them (sink gets the batch's slice, or None).
        `easy`: the batches run the easy network of a routed upscaler"""
        forward = (lambda x: self._forward(x, True)) if easy else self._forward
        with torch.no_grad():
            for b in range(-(-n // B)):
                x = gather(origins[b * B:(b + 1) * B], plan.win_h, plan.win_w)
                if self.self_ensemble == 1:
                    y = forward(x)
                else:
                    y = ops.self_ensemble(forward, x, self.self_ensemble)
                real = min(B, n - b * B)
                sink(y, real, table[b * B:b * B + real], wins[b * B:b * B + real] if wins is not None else None, plan)

    def _refuse_whole(self, whole):
        if whole and self.easy_net is not None:
            raise ValueError("whole=True runs one window: there is nothing to route (use an upscaler without easy_net)")

    def set_easy_threshold(self, threshold):
        """another `easy_threshold` for the calls that follow (a routed upscaler only); plans and graphs are kept.  A
        YUV420Stream on this upscaler must be reset(): its kept windows were classified with the old threshold"""
        if self.easy_net is None:
            raise ValueError("this upscaler has no easy_net: there is no threshold to set")
        routing.activity_limit(threshold, 1, 2)
        self.easy_threshold = threshold
        self._limits = {}

    def _limit(self, plan, depth):
        """the integer activity limit of the threshold for the plan's windows at a sample depth"""
        key = (plan.win_h, plan.win_w, depth)
        if key not in self._limits:
            self._limits[key] = routing.activity_limit(self.easy_threshold, plan.win_h, plan.win_w, depth)
        return self._limits[key]

    def _route(self, luma, plan, origins, table, B, changed=None, partial=None, out=None):
        """classify the plan's windows on the GPU by the luma activity of `luma` (an HWC RGB image or a Y plane) and run
        nothing yet: (routed origins [2, rows, 2], routed table [2, n, 6], indices [2, n], hard count, easy count).
        Reading the two counts back is the one synchronisation that routing adds."""
        n = len(plan)
        depth = 8 if luma.dim() == 3 else ops.YUV_DEPTHS[luma.dtype]
        partial = window_activity(luma, origins[:n], plan.win_h, plan.win_w, partial)
        o, t, idx, count = window_route(partial, self._limit(plan, depth), origins[:n], table, B, changed, out)
        hard, easy = count.tolist()
        self.route_stats = {"windows": n, "easy": easy, "hard": hard}
        return o, t, idx, hard, easy

    def _run_windows(self, H, W, device, whole, sink, gather, plan=None, luma=None):
        """the same for any source of windows: gather(origins, h, w) -> the [n, 3, h, w] batch of self.dtype.  `luma`:
        what a routed upscaler classifies the windows by (the RGB image or the Y plane)"""
        self._refuse_whole(whole)
        if plan is None:
            plan = self._whole_plan(H, W) if whole else self.plan(H, W)
        _, B = self._batching(plan)
        origins, table = self._tables(plan, device)
        if self.easy_net is None:
            self._run_batches(plan, origins, table, len(plan), B, sink, gather, plan.windows)
            return plan
        if len(plan) > MAX_WINDOWS:
            raise ValueError("a %dx%d image makes %d windows with core %d; routing takes at most %d: use a larger core"
                             % (W, H, len(plan), self.core, MAX_WINDOWS))
        o, t, _, hard, easy = self._route(luma, plan, origins, table, B)
        self._run_batches(plan, o[0], t[0], hard, B, sink, gather)
        self._run_batches(plan, o[1], t[1], easy, B, sink, gather, easy=True)
        return plan

    def window_activity(self, img, out_size=None, resample="lanczos"):
        """the mean absolute luma difference, in 8-bit levels, of every window of the plan of an image (HWC uint8 RGB) or
        of a YUV 4:2:0 frame (a tuple (y, u, v); only y is read): A / (D * depth factor) of routing.py as a CPU float64
        tensor [windows], in plan order -- what `easy_threshold` is compared with.  A read-back, for choosing the
        threshold; not on the hot path."""
        if isinstance(img, (tuple, list)):
            _, (luma, _, _), H, W = self._yuv420_frame(*img)
            depth, even = ops.YUV_DEPTHS[luma.dtype], True
        else:
            luma = self._image(img)
            H, W, depth, even = luma.size(0), luma.size(1), 8, False
        plan = self.plan(H, W) if out_size is None else self.plan(H, W, out_size, resample, even)
        origins, _ = self._tables(plan, luma.device)
        A = window_activity(luma, origins[:len(plan)], plan.win_h, plan.win_w).sum(dim=1).cpu()
        d = routing.activity_terms(plan.win_h, plan.win_w) * routing.depth_factor(depth)
        return A.to(torch.float64) / d if d else torch.zeros(len(plan), dtype=torch.float64)

    def _target_plan(self, H, W, whole, out_size, resample, even):
        """None without `out_size` or for the network's own size (today's path), else the ResizePlan"""
        if out_size is None:
            return None
        plan = self._whole_resize_plan(H, W, out_size, resample, even) if whole else self.plan(H, W, out_size, resample, even)
        return plan if isinstance(plan, ResizePlan) else None

    def upscale(self, img, whole=False, out_size=None, resample="lanczos"):
        """HWC uint8 RGB -> HWC uint8 RGB (scale x) on the GPU.  whole=True: one forward of the whole image (parity;
        refuses images whose activations would reach 2^31 bytes).  out_size = (TH, TW), between the input's size and the
        network's own on each axis: the output has that size and equals PIL's Image.fromarray(upscale(img)).resize((TW,
        TH), resample) bit for bit ("lanczos" or "bicubic"), resampled inside the scatter (tile_resize_scatter)"""
        self._refuse_whole(whole)
        H, W = int(img.shape[0]), int(img.shape[1])
        out = None
        rplan = self._target_plan(H, W, whole, out_size, resample, False)
        if rplan is not None:
            max_eh, max_ew = max(t[2] for t in rplan.targets), max(t[3] for t in rplan.targets)

            def rsink(y, real, table, wins, plan):
                nonlocal out
                if out is None:
                    out = torch.empty(plan.out_h, plan.out_w, 3, dtype=torch.uint8, device=y.device)
                vtab, htab = plan.device_tables(8, y.device)
                tile_resize_scatter(y.contiguous(), table, vtab, htab, out, max_eh, max_ew)

            self._run(img, whole, rsink, rplan)
            return out

        def sink(y, real, table, wins, plan):
            nonlocal out
            if out is None:
                out = torch.empty(H * self.scale, W * self.scale, 3, dtype=torch.uint8, device=y.device)
            wins = plan.windows if wins is None else wins         # routed batches: the plan's largest core bounds them
            tile_scatter(y.contiguous(), table, out, max(w[4] for w in wins) * self.scale,
                         max(w[5] for w in wins) * self.scale)

        self._run(img, whole, sink)
        return out

    # ------------------------------------------------------------------------------------------ image modes
    def split_image(self, img):
        """an HWC uint8 image of 1 (L), 2 (LA), 3 (RGB) or 4 (RGBA) channels (CPU or GPU tensor, or numpy array) ->
        (rgb [H, W, 3], channels, alpha [H, W] or None), on the GPU: modes.split_host (ops.mode_unpack_u8).  The RGB
        image is what upscale(), window_activity() and the metric take; three channels pass through untouched."""
        if not torch.is_tensor(img):
            img = torch.from_numpy(img)
        if img.dtype != torch.uint8 or img.dim() != 3 or img.size(2) not in modes.MODES:
            raise ValueError("upscale_image takes an HWC uint8 image of 1 (L), 2 (LA), 3 (RGB) or 4 (RGBA) channels, got %s %s"
                             % (tuple(img.shape), img.dtype))
        C = int(img.size(2))
        if C == 3:
            return self._image(img), 3, None
        dev = next(self.net.parameters()).device
        if dev.type != "cuda":
            raise _C.OfasrError("TiledUpscaler needs the network on the GPU")
        rgb, alpha = ops.mode_unpack_u8(img.to(dev).contiguous())
        return rgb, C, alpha

    def _alpha_device_tables(self, H, W, TH, TW, filter, device):
        """modes.alpha_tables as int32 tensors on `device`; up to 8 are kept and all are dropped when a ninth comes, as
        plan() does"""
        key = (int(H), int(W), int(TH), int(TW), filter, str(device))
        if key not in self._alpha_tables:
            if len(self._alpha_tables) >= 8:
                self._alpha_tables.clear()
            self._alpha_tables[key] = tuple(torch.from_numpy(t).to(device) for t in modes.alpha_tables(H, W, TH, TW, filter))
        return self._alpha_tables[key]

    def join_image(self, rgb_out, channels, alpha=None, in_hw=None, alpha_resample=modes.ALPHA_FILTER):
        """the RGB output [TH, TW, 3] on the GPU, the channel count and the SOURCE alpha plane of split_image -> the HWC
        uint8 output of that channel count: modes.join_host(rgb_out, channels, modes.alpha_host(alpha, TH, TW,
        alpha_resample)) (ops.mode_pack_u8).  `in_hw`: the input's (H, W), checked against the alpha plane.  Three
        channels: rgb_out itself."""
        resize.check_filter(alpha_resample)
        if isinstance(channels, bool) or channels not in modes.MODES:
            raise ValueError("channels must be one of %s, got %r" % (sorted(modes.MODES), channels))
        if (alpha is not None) != (channels in (2, 4)):
            raise ValueError("%s %s an alpha plane" % (modes.MODES[channels], "needs" if alpha is None else "takes no"))
        if channels == 3:
            return rgb_out
        if channels == 1:
            return ops.mode_pack_u8(rgb_out, 1)
        if alpha.dim() != 2 or (in_hw is not None and tuple(int(v) for v in in_hw) != tuple(alpha.shape)):
            raise ValueError("the alpha plane must be the input's [H, W], got %s" % (tuple(alpha.shape),))
        vtab, htab = self._alpha_device_tables(alpha.size(0), alpha.size(1), rgb_out.size(0), rgb_out.size(1), alpha_resample,
                                               rgb_out.device)
        return ops.mode_pack_u8(rgb_out, channels, alpha, vtab, htab)

    def upscale_image(self, img, whole=False, out_size=None, resample="lanczos", alpha_resample=modes.ALPHA_FILTER):
        """upscale() for an HWC uint8 image of 1 (L), 2 (LA), 3 (RGB) or 4 (RGBA) channels: the output, on the GPU, has
        the input's channel count (modes.py is the definition).  The network sees L as R = G = B and RGBA's colour
        untouched; the colour of the result is upscale() of that, bit for bit (for L / LA its Pillow luma); the alpha is
        the SOURCE alpha resized straight to the output's size with `alpha_resample` ("bicubic" or "lanczos"), Pillow's
        Image.resize bit for bit; it does not go through the network.  Three channels: upscale() itself."""
        resize.check_filter(alpha_resample)
        rgb, C, alpha = self.split_image(img)
        out = self.upscale(rgb, whole=whole, out_size=out_size, resample=resample)
        return self.join_image(out, C, alpha, rgb.shape[:2], alpha_resample)

    def _yuv420_frame(self, y, u, v):
        """(device, the three planes on it, H, W) of one frame for the YUV paths; refuses what they cannot take"""
        dev = next(self.net.parameters()).device
        if dev.type != "cuda":
            raise _C.OfasrError("TiledUpscaler needs the network on the GPU")
        planes = []
        for p in (y, u, v):
            if not torch.is_tensor(p):
                p = torch.from_numpy(p)
            if p.dtype not in ops.YUV_DEPTHS or p.dim() != 2:
                raise ValueError("upscale_yuv420 takes three 2-D uint8 (or, 10-bit, uint16) planes, got %s %s"
                                 % (tuple(p.shape), p.dtype))
            planes.append(p.to(dev).contiguous())
        y, u, v = planes
        H, W = int(y.shape[0]), int(y.shape[1])
        if H < 2 or W < 2 or H % 2 or W % 2:
            raise ValueError("a YUV 4:2:0 frame needs even sides, got %dx%d" % (W, H))
        if self.scale % 2:
            raise ValueError("YUV 4:2:0 upscaling needs an even upscale factor (window cores must land on whole chroma "
                             "samples of the output), this network's is %d" % self.scale)
        ops.yuv420_planes(y, u, v, "upscale_yuv420")
        return dev, (y, u, v), H, W

    @staticmethod
    def _yuv420_out(H, W, s, depth, dev):
        """fresh output planes of a depth (8 or 10) for an H x W input at scale s"""
        if isinstance(depth, bool) or depth not in ops.YUV_DTYPES:
            raise ValueError("out_depth must be 8 or 10, got %r" % (depth,))
        dt = ops.YUV_DTYPES[depth]
        return (torch.empty(H * s, W * s, dtype=dt, device=dev), torch.empty(H * s // 2, W * s // 2, dtype=dt, device=dev),
                torch.empty(H * s // 2, W * s // 2, dtype=dt, device=dev))

    def upscale_yuv420(self, y, u, v, matrix="bt601", full_range=False, whole=False, out_depth=None, out_size=None,
                       resample="lanczos"):
        """one planar YUV 4:2:0 frame (uint8 planes y [H, W], u, v [H/2, W/2]; CPU or GPU tensors, or numpy arrays) ->
        the upscaled planes (Y [H*s, W*s], U, V [H*s/2, W*s/2]) on the GPU.  The same plan, graph replay and self-ensemble
        as upscale(); the colour conversion is fused into the two tile moves (tile_gather_yuv420 / tile_scatter_yuv420),
        so no RGB frame exists on either side: the result equals
        ops.rgb_to_yuv420_u8(upscale(ops.yuv420_to_rgb_u8(y, u, v))) bit for bit.  uint16 planes are a 10-bit frame.
        `out_depth` (8 or 10; None: the input's) is the depth of the output planes, whatever the input's: 8 -> 10 writes
        the network's output at 1024 levels instead of rounding it to 256.  out_size = (TH, TW), even, between the
        input's size and the network's own: planes of that size, equal to the encode (ops.rgb_to_yuv420_u8, at the
        output depth) of resize.resize_host of the quantised full-size RGB, resampled inside the scatter."""
        self._refuse_whole(whole)
        dev, (y, u, v), H, W = self._yuv420_frame(y, u, v)
        s = self.scale
        depth = ops.YUV_DEPTHS[y.dtype] if out_depth is None else out_depth
        rplan = self._target_plan(H, W, whole, out_size, resample, True)
        if rplan is not None:
            out = self._yuv420_out(rplan.out_h, rplan.out_w, 1, depth, dev)
            vtab, htab = rplan.device_tables(depth, dev)
            max_eh, max_ew = max(t[2] for t in rplan.targets), max(t[3] for t in rplan.targets)

            def rsink(t, real, table, wins, plan):
                tile_resize_scatter_yuv420(t.contiguous(), table, vtab, htab, out[0], out[1], out[2], max_eh, max_ew, matrix,
                                           full_range)

            self._run_windows(H, W, dev, whole, rsink,
                              lambda origins, h, w: tile_gather_yuv420(y, u, v, origins, h, w, self.dtype, matrix, full_range),
                              rplan, luma=y)
            return out
        out = self._yuv420_out(H, W, s, depth, dev)

        def sink(t, real, table, wins, plan):
            wins = plan.windows if wins is None else wins         # routed batches: the plan's largest core bounds them
            tile_scatter_yuv420(t.contiguous(), table, out[0], out[1], out[2], max(w[4] for w in wins) * s,
                                max(w[5] for w in wins) * s, matrix, full_range)

        self._run_windows(H, W, dev, whole, sink,
                          lambda origins, h, w: tile_gather_yuv420(y, u, v, origins, h, w, self.dtype, matrix, full_range),
                          luma=y)
        return out

    def yuv420_stream(self, matrix="bt601", full_range=False, out_depth=None, out_size=None, resample="lanczos"):
        """a YUV420Stream on this upscaler: upscale_yuv420 for the consecutive frames of one video, re-running only the
        windows whose input bytes changed since the previous frame; the same output bit for bit"""
        return YUV420Stream(self, matrix, full_range, out_depth, out_size, resample)

    def upscale_float(self, img, whole=False):
        """the network's fp32 output [3, H*scale, W*scale] before quantisation, assembled from the same window cores
        as upscale() (torch copies; for parity checks)"""
        if self.easy_net is not None:
            raise ValueError("upscale_float is the parity path of one network: use an upscaler without easy_net")
        H, W = int(img.shape[0]), int(img.shape[1])
        s = self.scale
        out = None

        def sink(y, real, table, wins, plan):
            nonlocal out
            if out is None:
                out = torch.empty(3, H * s, W * s, dtype=torch.float32, device=y.device)
            for i, (wy, wx, cy, cx, ch, cw) in enumerate(wins):
                out[:, cy * s:(cy + ch) * s, cx * s:(cx + cw) * s] = \
                    y[i, :, (cy - wy) * s:(cy - wy + ch) * s, (cx - wx) * s:(cx - wx + cw) * s].float()

        self._run(img, whole, sink)
        return out


# ---------------------------------------------------------------------------------------------- video stream
class StreamStats(object):
    """windows / run / batches: the plan's windows, the windows that went through the network and the forward batches of
    the last frame; frames, frames_unchanged (no window run), total_windows, total_run, total_batches: since the stream
    was made.  run_easy / run_hard (total_run_easy / total_run_hard): the windows of `run` that a routed upscaler gave to
    its easy / hard network; without routing every window is hard."""

    def __init__(self):
        self.windows = self.run = self.batches = self.run_easy = self.run_hard = 0
        self.frames = self.frames_unchanged = self.total_windows = self.total_run = self.total_batches = 0
        self.total_run_easy = self.total_run_hard = 0

    def _frame(self, windows, run, batches, run_easy=0):
        self.windows, self.run, self.batches = windows, run, batches
        self.run_easy, self.run_hard = run_easy, run - run_easy
        self.frames += 1
        self.frames_unchanged += run == 0
        self.total_windows += windows
        self.total_run += run
        self.total_batches += batches
        self.total_run_easy += run_easy
        self.total_run_hard += run - run_easy


class YUV420Stream(object):
    """TiledUpscaler.upscale_yuv420 for the consecutive frames of one video, with exact reuse of unchanged windows.

    upscale(y, u, v) takes a frame as upscale_yuv420 does and returns the upscaled planes (Y, U, V) on the GPU, equal to
    upscale_yuv420's bit for bit.  THE RETURNED PLANES ARE THE STREAM'S OWN BUFFERS: they are valid until the next call
    of upscale() and are overwritten by it; copy them if they must outlive it.

    The stream keeps the previous input planes, the output planes and the plan's tables on the GPU.  Per frame:
    ofasr_window_diff_yuv420 flags the windows whose support (video.window_support) differs from the previous frame's,
    ofasr_window_compact gathers their table rows, the host reads their number m (one 8-byte read-back, the only
    synchronisation the stream adds), and ceil(m / B) batches run gather -> network (or self-ensemble) -> scatter into the
    persistent output planes, where the cores of unchanged windows keep their bytes.  B is the batch size of the full
    plan, whatever m is: every forward has the shape of the non-reuse path and replays the same captured graph, which
    is what makes the result bit-equal (a batch of fewer windows would be another graph, free to pick other kernels).
    Skipping is therefore per batch of B windows of changed content; a smaller `batch` or `core` of the upscaler skips
    more finely and pays for it with more launches or a larger plan.overhead() (window pixels per core pixel).

    The first frame, a frame of another size or dtype (uint8 / uint16: 8-bit / 10-bit) and the frame after reset() run
    every window.  The previous-frame planes have the input's dtype, the output planes that of `out_depth` (None: the
    input's).  The comparison is exact: it pays off on content that repeats bit for bit and does nothing for camera
    noise.

    On a routed upscaler (easy_net) a frame runs diff, then ofasr_window_activity_plane on the Y plane, then
    ofasr_window_route with the diff's flags: a changed window goes to the list of its class, an unchanged one to neither,
    and the two counts replace the one read-back.  A window's class depends on its own bytes alone, so an unchanged
    window would have been given the same network again: the output still equals the routed upscale_yuv420's."""

    def __init__(self, upscaler, matrix="bt601", full_range=False, out_depth=None, out_size=None, resample="lanczos"):
        ops.yuv_table(matrix, full_range, False)       # refuses an unknown matrix now rather than at the first frame
        if out_depth is not None and (isinstance(out_depth, bool) or out_depth not in ops.YUV_DTYPES):
            raise ValueError("out_depth must be 8 or 10, got %r" % (out_depth,))
        resize.check_filter(resample)
        self.up = upscaler
        self.matrix, self.full_range, self.out_depth = matrix, full_range, out_depth
        self.out_size, self.resample = out_size, resample
        self.stats = StreamStats()
        self._size = None
        self._fresh = self._all = True
        self._plan = None

    def reset(self):
        """forget the previous frame: the next one runs every window"""
        self._fresh = True

    def _setup(self, H, W, dev, dtype):
        up = self.up
        s = up.scale
        plan = up.plan(H, W) if self.out_size is None else up.plan(H, W, self.out_size, self.resample, True)
        if len(plan) > MAX_WINDOWS:
            raise ValueError("a %dx%d frame makes %d windows with core %d; a stream takes at most %d: use a larger core"
                             % (W, H, len(plan), up.core, MAX_WINDOWS))
        self._plan = plan
        _, self._B = up._batching(plan)
        self._origins, self._table = up._tables(plan, dev)
        depth = ops.YUV_DEPTHS[dtype] if self.out_depth is None else self.out_depth
        self._coeffs = None
        if isinstance(plan, ResizePlan):               # a window's target rectangle depends on that window's bytes alone
            self._max_eh, self._max_ew = max(t[2] for t in plan.targets), max(t[3] for t in plan.targets)
            self._coeffs = plan.device_tables(depth, dev)
        else:
            self._max_eh = max(w[4] for w in plan.windows) * s
            self._max_ew = max(w[5] for w in plan.windows) * s
        self._prev = (torch.empty(H, W, dtype=dtype, device=dev), torch.empty(H // 2, W // 2, dtype=dtype, device=dev),
                      torch.empty(H // 2, W // 2, dtype=dtype, device=dev))
        self._out = up._yuv420_out(plan.out_h, plan.out_w, 1, depth, dev) if self._coeffs is not None else \
            up._yuv420_out(H, W, s, depth, dev)
        n = len(plan)
        self._flags = torch.zeros(n, window_diff_slabs(plan.win_h, plan.win_w), dtype=torch.int32, device=dev)
        self._compact = (torch.zeros(self._origins.size(0), 2, dtype=torch.int64, device=dev),
                         torch.zeros(n, 6, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
                         torch.zeros(1, dtype=torch.int64, device=dev))
        self._routed = None
        if up.easy_net is not None:
            self._partial = torch.zeros(n, window_activity_slabs(plan.win_h, plan.win_w), dtype=torch.int64, device=dev)
            self._routed = (torch.zeros(2, -(-n // self._B) * self._B, 2, dtype=torch.int64, device=dev),
                            torch.zeros(2, n, 6, dtype=torch.int64, device=dev),
                            torch.zeros(2, n, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
        self._size = (H, W, dev, dtype)
        self._fresh = True

    def changed_windows(self):
        """plan indices of the windows the last frame ran, in plan order (a read-back; for tests and diagnostics)"""
        if self._plan is None:
            return []
        if self._all:
            return list(range(len(self._plan)))
        if self._routed is not None:
            idx = self._routed[2]
            return sorted(idx[0, :self.stats.run_hard].tolist() + idx[1, :self.stats.run_easy].tolist())
        return self._compact[2][:self.stats.run].tolist()

    def upscale(self, y, u, v):
        """one frame -> the upscaled planes (Y, U, V): the stream's own buffers, valid until the next call"""
        up = self.up
        dev, (y, u, v), H, W = up._yuv420_frame(y, u, v)
        if self._size != (H, W, dev, y.dtype):
            self._setup(H, W, dev, y.dtype)
        plan, B, n = self._plan, self._B, len(self._plan)
        out = self._out

        def sink(t, real, table, wins, plan):
            if self._coeffs is not None:
                tile_resize_scatter_yuv420(t.contiguous(), table, self._coeffs[0], self._coeffs[1], out[0], out[1], out[2],
                                           self._max_eh, self._max_ew, self.matrix, self.full_range)
            else:
                tile_scatter_yuv420(t.contiguous(), table, out[0], out[1], out[2], self._max_eh, self._max_ew, self.matrix,
                                    self.full_range)

        def gather(origins, h, w):
            return tile_gather_yuv420(y, u, v, origins, h, w, up.dtype, self.matrix, self.full_range)

        self._all = self._fresh
        self._fresh = True                             # until this frame is complete: a failed frame leaves nothing to reuse
        if self._routed is not None:
            flags = None
            if not self._all:
                flags = window_diff_yuv420(y, u, v, self._prev[0], self._prev[1], self._prev[2], self._origins[:n],
                                           plan.win_h, plan.win_w, self._flags)
            o, t, _, hard, easy = up._route(y, plan, self._origins, self._table, B, flags, self._partial, self._routed)
            up._run_batches(plan, o[0], t[0], hard, B, sink, gather)
            up._run_batches(plan, o[1], t[1], easy, B, sink, gather, easy=True)
            for dst, src in zip(self._prev, (y, u, v)):
                dst.copy_(src)
            self._fresh = False
            self.stats._frame(n, hard + easy, -(-hard // B) + -(-easy // B), easy)
            return out
        if self._all:
            m = n
            up._run_batches(plan, self._origins, self._table, n, B, sink, gather)
        else:
            window_diff_yuv420(y, u, v, self._prev[0], self._prev[1], self._prev[2], self._origins[:n], plan.win_h,
                               plan.win_w, self._flags)
            c_origins, c_table, _, count = window_compact(self._flags, self._origins[:n], self._table, B, self._compact)
            m = int(count.item())                      # the stream's one synchronisation per frame
            up._run_batches(plan, c_origins, c_table, m, B, sink, gather)
        for dst, src in zip(self._prev, (y, u, v)):
            dst.copy_(src)                             # stream-ordered behind the kernels that read both
        self._fresh = False
        self.stats._frame(n, m, -(-m // B))
        return out
