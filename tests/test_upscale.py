"""Tiled upscaling, host side (CPU): the tile plan's properties (upscale.plan_windows), the receptive radius of static
networks against a test-local mask propagation (upscale.receptive_radius), the refusal of unaligned X4 inputs, and the
argument validation of the two tile kernels' entry points.  The kernels and the tiled = whole parity run on the GPU:
test_hip_upscale.py."""
import ctypes
import math
import random

import numpy as np
import pytest

from conftest import amd

KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])


def _config(kind, setting):
    nets = amd("elastic_nn.networks")
    net = nets.OFAMobileNetS4(**KW) if kind == "s4" else nets.OFAMobileNetX4(**KW)
    if isinstance(setting, dict):
        net.set_active_subnet(**setting)
    else:
        random.seed(setting)
        net.sample_active_subnet()
    return net.get_active_net_config()


# ---------------------------------------------------------------------------------------------- plan
def _check_plan(plan, H, W, core, halo, align, px):
    assert plan.H == H and plan.W == W
    wh, ww = plan.win_h, plan.win_w
    assert 0 < wh <= H and 0 < ww <= W
    assert wh % align == 0 and ww % align == 0
    if ww < W:
        assert ww % 8 == 0
    cover = np.zeros((H, W), np.int32)
    for (wy, wx, cy, cx, ch, cw) in plan.windows:
        # inside the image
        assert 0 <= wy and wy + wh <= H and 0 <= wx and wx + ww <= W
        assert wy % align == 0 and wx % align == 0
        assert ch > 0 and cw > 0 and ch <= max(core, H if wh == H else 0) and cw <= max(core, W if ww == W else 0)
        # the core is inside its window, >= halo from every window edge that is not an image edge
        assert wy <= cy and cy + ch <= wy + wh and wx <= cx and cx + cw <= wx + ww
        if wy > 0:
            assert cy - wy >= halo
        if wy + wh < H:
            assert wy + wh - (cy + ch) >= halo
        if wx > 0:
            assert cx - wx >= halo
        if wx + ww < W:
            assert wx + ww - (cx + cw) >= halo
        cover[cy:cy + ch, cx:cx + cw] += 1
    assert (cover == 1).all(), "the cores must tile the image exactly once"
    # the batch cap: no batched tensor reaches 2^31 elements
    assert plan.batch >= 1
    assert plan.batch * px * wh * ww < 2 ** 31 or plan.batch == 1


def test_plan_properties_random():
    up = amd("upscale")
    rng = random.Random(0)
    for trial in range(600):
        align = rng.choice([1, 1, 2, 4])
        H = align * rng.randint(1, 700 // align)
        W = align * rng.randint(1, 900 // align)
        core = align * rng.randint(1, 300 // align)
        halo = rng.randint(0, 80)
        px = rng.choice([64, 384, 1024, 4096])
        plan = up.plan_windows(H, W, core, halo, align, 4, px)
        _check_plan(plan, H, W, core, up._up(halo, align), align, px)


@pytest.mark.parametrize("H,W", [(1, 1), (7, 5), (30, 301), (187, 301), (1080, 1920), (4320, 7680)])
def test_plan_small_and_large_images(H, W):
    up = amd("upscale")
    plan = up.plan_windows(H, W, 48, 20, 1, 4, 1024)
    _check_plan(plan, H, W, 48, 20, 1, 1024)
    if H <= 48 + 40:
        assert plan.win_h == H          # smaller than one window: the window is the whole axis
    if W <= 48 + 40:
        assert plan.win_w == W


def test_plan_default_core_keeps_activations_below_2g():
    up = amd("upscale")
    cfg = _config("s4", dict(ks=7, e=6, d=4, pixel_d=2))
    r = up.receptive_radius(cfg)
    px = up.activation_elems_per_pixel(cfg)
    assert px == 256 * 4     # the 64 -> 256 conv before the last PixelShuffle, at twice the input resolution
    core = up.default_core(r, 1, px)
    assert core % 8 == 0 and core > 2 * r
    plan = up.plan_windows(1080, 1920, core, r, 1, 4, px)
    _check_plan(plan, 1080, 1920, core, r, 1, px)
    assert 4 * px * plan.win_h * plan.win_w < 2 ** 31
    assert len(plan) > 1     # the whole image would not fit


def test_x4_unaligned_inputs_refused():
    up = amd("upscale")
    with pytest.raises(ValueError, match="multiples of 4"):
        up.plan_windows(301, 188, 64, 8, 4, 1)
    with pytest.raises(ValueError, match="multiples of 2"):
        up.plan_windows(300, 187, 64, 8, 2, 1)
    up.plan_windows(300, 188, 64, 8, 4, 1)


# ---------------------------------------------------------------------------------------------- radius
def _support(config, parity):
    """test-local restatement: a one-pixel 1-D mask through the layer list (square kernels: the 2-D support is the 1-D
    one per axis).  Returns the largest distance, in output pixels, of an affected output pixel from the input pixel's
    output block."""
    steps = []

    def conv(c):
        steps.append(("conv", c["kernel_size"]))
        if c.get("act_func") == "pixelshuffle":
            steps.append(("ps",))
        elif c.get("act_func") == "pixelunshuffle":
            steps.append(("pu",))

    def block(c):
        if c["name"] == "MobileInvertedResidualBlock":
            steps.append(("conv", c["mobile_inverted_conv"]["kernel_size"]))
        else:
            conv(c)

    b = config["blocks"]
    if config["name"] == "SRNetS4":
        order = [config["dec_first_conv_block"]] + b[:config["n_mb"]] + config["dec_final_conv_blocks"] + b[config["n_mb"]:]
    else:
        u, e, d = config["n_unshuffle"], config["n_enc"], config["n_dec"]
        order = (b[:u + e] + config["enc_final_conv_blocks"] + [config["dec_first_conv_block"]] + b[u + e:u + e + d]
                 + config["dec_final_conv_blocks"] + b[u + e + d:])
    for c in order + [config["dec_final_output_conv_block"]]:
        block(c)

    L = 4096
    p = L // 2 + parity
    m = np.zeros(L, bool)
    m[p] = True
    for s in steps:
        if s[0] == "conv":
            h = (s[1] - 1) // 2
            idx = np.nonzero(m)[0]
            m = np.zeros(len(m), bool)
            m[max(idx.min() - h, 0):idx.max() + h + 1] = True
        elif s[0] == "ps":
            m = np.repeat(m, 2)
        else:
            m = m.reshape(-1, 2).any(1)
    scale = len(m) // L
    idx = np.nonzero(m)[0]
    lo, hi = p * scale, (p + 1) * scale - 1
    return max(lo - idx.min(), idx.max() - hi, 0), scale


CASES = [("s4", dict(ks=7, e=6, d=4, pixel_d=2)), ("s4", dict(ks=3, e=3, d=2, pixel_d=1)), ("s4", 0), ("s4", 3), ("s4", 11),
         ("x4", dict(ks=5, e=4, d=2, pixel_d=2)), ("x4", dict(ks=3, e=3, d=2, pixel_d=1))]


@pytest.mark.parametrize("kind,setting", CASES, ids=lambda v: str(v))
def test_receptive_radius_matches_mask_propagation(kind, setting):
    up = amd("upscale")
    cfg = _config(kind, setting)
    r = up.receptive_radius(cfg)
    for parity in (0, 1, 2, 3):
        support, scale = _support(cfg, parity)
        assert scale == cfg["upscale"]
        assert math.ceil(support / scale) <= r, (support, scale, r)
        if parity == 0:
            worst = support
        worst = max(worst, support)
    assert r <= math.ceil(worst / scale) + 1, (worst, scale, r)


def test_max_s4_radius():
    up = amd("upscale")
    cfg = _config("s4", dict(ks=7, e=6, d=4, pixel_d=2))
    # stem k5 (2) + 14 MB k7 (42) + 2 convs k5 (4) + shuffle conv k5 at 1x (2) + at 2x (1) + head k5 at 4x (0.5)
    assert up.receptive_radius(cfg) == 52


# ---------------------------------------------------------------------------------------------- ABI
def test_tile_entry_points_validate_without_gpu():
    C = amd("_C")
    L = C.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.ofasr_tile_gather_u8(None, 4, 4, p, 1, 2, 2, p, 0, None) == -1
    assert b"null" in L.ofasr_last_error_string()
    assert L.ofasr_tile_gather_u8(p, 4, 4, p, 0, 2, 2, p, 0, None) == -1        # no window
    assert L.ofasr_tile_gather_u8(p, 4, 4, p, 1, 5, 2, p, 0, None) == -1        # window taller than the image
    assert L.ofasr_tile_gather_u8(p, 4, 4, p, 1, 2, 2, p, 7, None) == -1        # bad dtype
    assert L.ofasr_tile_gather_u8(p, 4, 4, p, 70000, 2, 2, p, 0, None) == -2    # too many windows for one launch
    assert L.ofasr_tile_scatter_u8(p, 1, 8, 8, 0, None, p, 8, 8, 8, 8, None) == -1
    assert L.ofasr_tile_scatter_u8(p, 1, 8, 8, 3, p, p, 8, 8, 8, 8, None) == -1  # bad dtype
    assert L.ofasr_tile_scatter_u8(p, 1, 8, 8, 0, p, p, 8, 8, 9, 8, None) == -1  # extent bound past the source window
    assert L.ofasr_tile_scatter_u8(p, 1, 8, 8, 0, p, p, 0, 8, 8, 8, None) == -1  # empty destination
    assert L.ofasr_version() >= 303
