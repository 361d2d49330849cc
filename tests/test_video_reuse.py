"""Host definition of window reuse between video frames (video.window_support / changed_windows_host), no GPU: a window
that is not flagged decodes to the same RGB, the flagged windows are the ones whose support rectangle holds the changed
sample, the 9-3-3-1 filter's neighbour tap is part of the support, and the plan of the GPU tests is what they say it is.
Everything is bit-exact."""
import numpy as np
import pytest

from conftest import amd

H, W = 14, 18
# (y0, x0, h, w): even / odd origins, odd sizes, a 1x1 window, the whole frame, windows at the far edges
WINDOWS = [(0, 0, 5, 7), (1, 3, 6, 4), (3, 5, 7, 9), (4, 2, 1, 1), (0, 0, 14, 18), (9, 11, 5, 7), (7, 1, 2, 16), (13, 17, 1, 1)]


def _frame(seed, h=H, w=W):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 256, (h, w)).astype(np.uint8), rng.randint(0, 256, (h // 2, w // 2)).astype(np.uint8),
            rng.randint(0, 256, (h // 2, w // 2)).astype(np.uint8))


def _in_support(plane, r, c, y0, x0, h, w, HH, WW):
    """the issue's formula, written out on its own"""
    if plane == 0:
        return y0 <= r <= y0 + h - 1 and x0 <= c <= x0 + w - 1
    return max(0, (y0 - 1) >> 1) <= r <= min(HH // 2 - 1, (y0 + h) >> 1) and \
        max(0, (x0 - 1) >> 1) <= c <= min(WW // 2 - 1, (x0 + w) >> 1)


def test_window_support_rectangles():
    video = amd("video")
    assert video.window_support(0, 0, 5, 7, H, W) == ((0, 4, 0, 6), (0, 2, 0, 3))
    assert video.window_support(1, 3, 6, 4, H, W) == ((1, 6, 3, 6), (0, 3, 1, 3))
    assert video.window_support(4, 2, 1, 1, H, W) == ((4, 4, 2, 2), (1, 2, 0, 1))
    assert video.window_support(0, 0, 14, 18, H, W) == ((0, 13, 0, 17), (0, 6, 0, 8))
    # origins are clamped as the gather clamps them
    assert video.window_support(-5, 1000, 5, 7, H, W) == video.window_support(0, 11, 5, 7, H, W)
    assert video.window_support(10 ** 12, -3, 5, 7, H, W) == video.window_support(9, 0, 5, 7, H, W)


def test_unflagged_windows_decode_identically_and_flags_follow_the_formula():
    video = amd("video")
    base = _frame(0)
    rgb0 = video.yuv420_to_rgb_host(*base)
    cases = 0
    tight = 0
    for plane in range(3):
        for r in range(base[plane].shape[0]):
            for c in range(base[plane].shape[1]):
                cur = [p.copy() for p in base]
                cur[plane][r, c] ^= 0x80
                rgb1 = video.yuv420_to_rgb_host(*cur)
                for (y0, x0, h, w) in WINDOWS:
                    flag = bool(video.changed_windows_host(base, cur, [(y0, x0)], h, w)[0])
                    assert flag == _in_support(plane, r, c, y0, x0, h, w, H, W), (plane, r, c, y0, x0, h, w)
                    same = np.array_equal(rgb0[y0:y0 + h, x0:x0 + w], rgb1[y0:y0 + h, x0:x0 + w])
                    if not flag:
                        assert same, (plane, r, c, y0, x0, h, w)
                    else:
                        tight += not same
                cases += 1
    assert cases == 14 * 18 + 2 * 7 * 9
    assert tight > 0          # flagged windows do change (clamping may hide a single flip, never all of them)


def test_changed_windows_host_takes_a_table_and_refuses_misfits():
    video = amd("video")
    a, b = _frame(1), _frame(1)
    origins = [(0, 0), (1, 3), (9, 11), (99, 10 ** 12)]      # the last one is clamped to (9, 11)
    assert not video.changed_windows_host(a, b, origins, 5, 7).any()
    b[2][6, 8] ^= 1                                      # the last chroma sample: only the windows at the far corner
    assert video.changed_windows_host(a, b, origins, 5, 7).tolist() == [False, False, True, True]
    assert video.changed_windows_host(a, _frame(2), origins, 5, 7).all()
    with pytest.raises(ValueError):
        video.changed_windows_host(a, _frame(1, 16, 18), origins, 5, 7)
    with pytest.raises(ValueError):
        video.changed_windows_host(a, b, origins, 15, 7)


def test_neighbour_tap_is_part_of_the_support():
    """72x104, 49-row windows: chroma row 31 belongs to pixel rows 62 / 63, outside a window over rows 13 .. 61, but pixel
    row 61 (odd) takes row 31 as its neighbour tap"""
    video = amd("video")
    HH, WW, h, w = 72, 104, 49, 56
    base = _frame(3, HH, WW)
    base[1][:] = 128                                     # mid chroma: the flip below moves the decode well inside 0 .. 255
    base[0][:] = 128
    cur = [p.copy() for p in base]
    cur[1][31, 20] = 255
    origins = [(wy, wx) for wy in (0, 13, 23) for wx in (0, 13, 48)]
    flags = video.changed_windows_host(base, cur, origins, h, w).tolist()
    # chroma column 20 = pixels 40, 41: inside the windows at x 0 and 13, outside the one at x 48 (support from column 23)
    assert flags == [False, False, False, True, True, False, True, True, False]
    assert not 13 <= 2 * 31 <= 13 + h - 1                # the sample's own 2x2 block lies below the window
    rgb0, rgb1 = video.yuv420_to_rgb_host(*base), video.yuv420_to_rgb_host(*cur)
    assert not np.array_equal(rgb0[61, 13:13 + w], rgb1[61, 13:13 + w])      # and the window's last row does change
    assert np.array_equal(rgb0[:61], rgb1[:61])


def test_plan_of_the_gpu_tests():
    """core 16, halo 17 (the small test network's radius) on 72x104: 35 windows of 49x56 at the origins the GPU tests use"""
    up = amd("upscale")
    plan = up.plan_windows(72, 104, 16, 17, 1, 4, 64)
    assert (len(plan), plan.win_h, plan.win_w) == (35, 49, 56)
    assert [w[1] for w in plan.windows[:7]] == [0, 0, 13, 28, 43, 48, 48]
    assert [w[0] for w in plan.windows[::7]] == [0, 0, 13, 23, 23]
