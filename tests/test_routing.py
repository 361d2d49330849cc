"""Content-aware routing, host side (CPU): the activity statement (routing.window_activity_host) against a plain double
loop, the threshold -> integer limit conversion, the shared tile plan of two networks (upscale.shared_geometry) and the
refusals of TiledUpscaler(easy_net=...) that need no GPU.  The kernels and the routed upscaler run on the GPU:
test_hip_routing.py."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import amd
from test_upscale import _config

WILD = [(-5, 1000), (10 ** 12, -3), (-2 ** 62, 2 ** 62), (7, 10 ** 6)]


def _luma_loop(src):
    src = np.asarray(src)
    if src.ndim == 2:
        return [[int(v) for v in row] for row in src]
    return [[(77 * int(p[0]) + 150 * int(p[1]) + 29 * int(p[2]) + 128) >> 8 for p in row] for row in src]


def _activity_loop(src, origins, h, w):
    L = _luma_loop(src)
    H, W = len(L), len(L[0])
    out = []
    for (oy, ox) in origins:
        y0, x0 = min(max(oy, 0), H - h), min(max(ox, 0), W - w)
        A = 0
        for r in range(h):
            for c in range(w):
                if c + 1 < w:
                    A += abs(L[y0 + r][x0 + c + 1] - L[y0 + r][x0 + c])
                if r + 1 < h:
                    A += abs(L[y0 + r + 1][x0 + c] - L[y0 + r][x0 + c])
        out.append(A)
    return out


def _sources(H, W, seed):
    rng = np.random.RandomState(seed)
    return {"rgb": rng.randint(0, 256, (H, W, 3)).astype(np.uint8), "u8": rng.randint(0, 256, (H, W)).astype(np.uint8),
            "u16": rng.randint(0, 1024, (H, W)).astype(np.uint16)}


@pytest.mark.parametrize("kind", ["rgb", "u8", "u16"])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (5, 1), (5, 7), (9, 11)])
def test_activity_matches_a_double_loop(kind, h, w):
    routing = amd("routing")
    H, W = 9, 11
    src = _sources(H, W, h * 16 + w)[kind]
    origins = [(0, 0), (H - h, W - w), (1, 2), (3, 0), (0, 4)] + WILD
    got = routing.window_activity_host(src, origins, h, w)
    assert got.dtype == np.int64 and got.tolist() == _activity_loop(src, origins, h, w)
    assert routing.activity_terms(h, w) == h * (w - 1) + (h - 1) * w
    if (h, w) == (1, 1):
        assert routing.activity_terms(1, 1) == 0 and not got.any()
    # a wild origin is the clamped one
    clamped = [(min(max(oy, 0), H - h), min(max(ox, 0), W - w)) for (oy, ox) in WILD]
    assert got[-4:].tolist() == routing.window_activity_host(src, clamped, h, w).tolist()


def test_activity_extremes_and_refusals():
    routing = amd("routing")
    board = ((np.add.outer(np.arange(6), np.arange(8)) & 1) * 255).astype(np.uint8)
    assert routing.window_activity_host(board, [(0, 0)], 6, 8)[0] == 255 * routing.activity_terms(6, 8)
    board10 = ((np.add.outer(np.arange(6), np.arange(8)) & 1) * 1023).astype(np.uint16)
    assert routing.window_activity_host(board10, [(0, 0)], 6, 8)[0] == 1023 * routing.activity_terms(6, 8)
    assert routing.window_activity_host(np.full((6, 8, 3), 200, np.uint8), [(0, 0), (2, 2)], 4, 4).tolist() == [0, 0]
    white = np.full((1, 1, 3), 255, np.uint8)
    assert routing.luma_rgb(white)[0, 0] == 255 and routing.luma_rgb(white * 0)[0, 0] == 0
    with pytest.raises(ValueError):
        routing.window_activity_host(board, [(0, 0)], 7, 8)
    with pytest.raises(ValueError):
        routing.window_activity_host(board.astype(np.float32), [(0, 0)], 2, 2)
    with pytest.raises(ValueError):
        routing.luma_rgb(board)
    assert routing.mean_activity([0, 255 * 82], 6, 8).tolist() == [0.0, 255.0]
    assert routing.mean_activity([1023 * 82], 6, 8, 10).tolist() == [1023 / 4.0]
    assert routing.mean_activity([0], 1, 1).tolist() == [0.0]


def test_limit_is_exact():
    routing = amd("routing")
    h, w = 49, 56
    D = routing.activity_terms(h, w)
    assert D == 49 * 55 + 48 * 56
    for T in (0.1, "0.1", 0.3, "0.7", 1.1, "2.675", 1e-3, "1e-3", 0, 5, "12.5"):
        exp = math.floor(Fraction(str(T)) * D)
        assert routing.activity_limit(T, h, w) == exp, T
        assert routing.activity_limit(T, h, w, 10) == math.floor(Fraction(str(T)) * D * 4), T
    # float multiplication is off by one where the decimal is not: 0.1 * 30 = 3.0000000000000004, 0.7 * 10 = 7.000000000000001 ...
    # and in the other direction 0.29 * 100 = 28.999999999999996
    assert routing.activity_terms(1, 101) == 100 and routing.activity_limit(0.29, 1, 101) == 29
    assert math.floor(0.29 * 100) == 28
    assert routing.activity_terms(4, 4) == 24 and routing.activity_limit("1.15", 4, 4, 10) == 110
    assert routing.activity_limit(-0.001, h, w) == -1 and routing.activity_limit(float("-inf"), h, w) == -1
    assert routing.activity_limit("-3", h, w, 10) == -1
    assert routing.activity_limit(float("inf"), h, w) == routing.INT64_MAX == 2 ** 63 - 1
    assert routing.activity_limit("inf", h, w, 10) == 2 ** 63 - 1
    assert routing.activity_limit(1e300, h, w) == 2 ** 63 - 1                    # capped: the kernel compares int64
    assert routing.activity_limit(3, 1, 1) == 0                                  # D = 0: every 1 x 1 window is easy for T >= 0
    for bad in (float("nan"), "nan", "flat", True, None):
        with pytest.raises((ValueError, TypeError)):
            routing.activity_limit(bad, h, w)
    with pytest.raises(ValueError):
        routing.activity_limit(1, h, w, 12)


def test_classify_host():
    routing = amd("routing")
    img = np.zeros((8, 16), np.uint8)
    img[:, 8:] = np.random.RandomState(0).randint(0, 256, (8, 8))
    origins = [(0, 0), (0, 8), (0, 4)]
    A = routing.window_activity_host(img, origins, 8, 8)
    assert A[0] == 0 and A[1] > A[2] > 0
    T = float(A[2]) / routing.activity_terms(8, 8)                               # the limit is A[2] exactly or just below
    assert routing.classify_host(img, origins, 8, 8, -1).tolist() == [False, False, False]
    assert routing.classify_host(img, origins, 8, 8, float("inf")).tolist() == [True, True, True]
    assert routing.classify_host(img, origins, 8, 8, 0).tolist() == [True, False, False]
    assert routing.classify_host(img, origins, 8, 8, Fraction(int(A[2]), routing.activity_terms(8, 8)).limit_denominator(10 ** 9)
                                 + Fraction(1, 10 ** 6)).tolist() == [True, False, True]
    assert T > 0
    # depth 10: the same picture at four times the levels has the same classes
    assert routing.classify_host(img.astype(np.uint16) * 4, origins, 8, 8, "0.5").tolist() == \
        routing.classify_host(img, origins, 8, 8, "0.5").tolist()


def test_shared_plan_parameters_of_two_configs():
    up, routing = amd("upscale"), amd("routing")
    big = _config("s4", dict(ks=7, e=6, d=4, pixel_d=2))
    small = _config("s4", dict(ks=3, e=3, d=2, pixel_d=1))
    x4 = _config("x4", 0)
    for a, b in ((big, small), (big, x4), (small, x4)):
        ra, rb = up.receptive_radius(a), up.receptive_radius(b)
        al = up.alignment(a) * up.alignment(b) // math.gcd(up.alignment(a), up.alignment(b))
        exp = (max(ra, rb), al, -(-max(ra, rb) // al) * al,
               max(up.activation_elems_per_pixel(a), up.activation_elems_per_pixel(b)))
        assert up.shared_geometry(a, b) == exp == up.shared_geometry(b, a)       # the roles in both orders
        assert exp[2] % up.alignment(a) == 0 and exp[2] % up.alignment(b) == 0 and exp[2] >= exp[0]
    assert up.receptive_radius(big) > up.receptive_radius(small)
    assert up.shared_geometry(big, big) == (up.receptive_radius(big), 1, up.receptive_radius(big),
                                            up.activation_elems_per_pixel(big))
    assert up.alignment(x4) > 1
    assert routing.shared_plan_params((17, 1, 64), (5, 4, 384)) == (17, 4, 20, 384)
    assert routing.shared_plan_params((5, 4, 384), (17, 6, 64)) == (17, 12, 24, 384)


def test_constructor_refusals():
    up = amd("upscale")
    st = amd("imagenet_codebase.networks.sr_static")
    small = st.build_static_net(_config("s4", dict(ks=3, e=3, d=2, pixel_d=1)))
    big = st.build_static_net(_config("s4", dict(ks=5, e=4, d=3, pixel_d=1)))
    with pytest.raises(ValueError, match="both easy_net and easy_threshold"):
        up.TiledUpscaler(big, core=16, graphed=False, easy_net=small)
    with pytest.raises(ValueError, match="both easy_net and easy_threshold"):
        up.TiledUpscaler(big, core=16, graphed=False, easy_threshold=0.5)
    with pytest.raises(ValueError, match="NaN"):
        up.TiledUpscaler(big, core=16, graphed=False, easy_net=small, easy_threshold=float("nan"))
    with pytest.raises(ValueError, match="number"):
        up.TiledUpscaler(big, core=16, graphed=False, easy_net=small, easy_threshold="flat")
    class Other(torch.nn.Module):                        # stands for an export of another upscale factor
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.weight = torch.nn.Parameter(torch.zeros(1))
            self.config = dict(small.config, upscale=2)

    other = Other()
    with pytest.raises(ValueError, match="same upscale factor"):
        up.TiledUpscaler(big, core=16, graphed=False, easy_net=other, easy_threshold=0.5)
    tu = up.TiledUpscaler(big, core=16, graphed=False, easy_net=small, easy_threshold="0.5")
    assert (tu.radius, tu.align, tu.halo, tu.px_elems) == up.shared_geometry(big.config, small.config)
    assert tu.radius == up.receptive_radius(big.config) > up.receptive_radius(small.config)
    swapped = up.TiledUpscaler(small, core=16, graphed=False, easy_net=big, easy_threshold="0.5")
    assert (swapped.radius, swapped.halo) == (tu.radius, tu.halo)
    assert tu.plan(72, 104).windows == swapped.plan(72, 104).windows
    plain = up.TiledUpscaler(small, core=16, graphed=False)
    assert plain.easy_net is None and plain.route_stats is None and plain.radius == up.receptive_radius(small.config)
    img = np.zeros((40, 56, 3), np.uint8)
    with pytest.raises(ValueError, match="nothing to route"):
        tu.upscale(img, whole=True)
    with pytest.raises(ValueError, match="without easy_net"):
        tu.upscale_float(img)
