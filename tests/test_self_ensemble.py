"""Geometric self-ensemble, host side: the 8 transforms T_t of upscale.d4_transform / d4_inverse form the dihedral group
D4 (inverse, distinctness, closure), the tile plan's opt-in height rule, and the argument checks of the ops (no GPU)."""
import pytest
import torch

from conftest import amd


def _asym(h, w):
    return torch.arange(h * w, dtype=torch.int64).view(1, 1, h, w) ** 2 + 3


def test_inverse_undoes_transform():
    up = amd("upscale")
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.int32).view(2, 3, 5, 7)
    for t in range(8):
        y = up.d4_transform(x, t)
        assert y.shape == ((2, 3, 7, 5) if t & 4 else (2, 3, 5, 7)) and y.is_contiguous()
        assert torch.equal(up.d4_inverse(y, t), x), t
    # the pinned order: flip W, then flip H, then transpose
    assert torch.equal(up.d4_transform(x, 1), x.flip(-1))
    assert torch.equal(up.d4_transform(x, 2), x.flip(-2))
    assert torch.equal(up.d4_transform(x, 7), x.flip(-1).flip(-2).transpose(-1, -2))


def test_transforms_are_pairwise_distinct():
    up = amd("upscale")
    x = _asym(3, 5)
    outs = [up.d4_transform(x, t) for t in range(8)]
    for s in range(8):
        for t in range(s + 1, 8):
            assert outs[s].shape != outs[t].shape or not torch.equal(outs[s], outs[t]), (s, t)


def test_closure():
    up = amd("upscale")
    x = _asym(3, 5)
    outs = [up.d4_transform(x, t) for t in range(8)]
    for s in range(8):
        hit = set()
        for t in range(8):
            y = up.d4_transform(outs[s], t)            # T_t o T_s
            us = [u for u in range(8) if outs[u].shape == y.shape and torch.equal(outs[u], y)]
            assert len(us) == 1, (s, t, us)
            hit.add(us[0])
        assert hit == set(range(8)), s                 # t -> u is a bijection for every s


def test_bad_transform_index():
    up = amd("upscale")
    x = _asym(3, 5)
    for t in (-1, 8, 1.0, True, None):
        with pytest.raises(ValueError):
            up.d4_transform(x, t)
        with pytest.raises(ValueError):
            up.d4_inverse(x, t)


def test_plan_height_rule():
    up = amd("upscale")
    args = (187, 301, 48, 18, 1, 4, 384)
    plan = up.plan_windows(*args, height8=True)
    assert plan.win_h % 8 == 0 and plan.win_w % 8 == 0 and plan.win_h < 187
    # cores still tile the image once, every window lies inside it and holds its core with the halo (or an image edge)
    seen = torch.zeros(187, 301, dtype=torch.int32)
    for (wy, wx, cy, cx, ch, cw) in plan.windows:
        seen[cy:cy + ch, cx:cx + cw] += 1
        assert 0 <= wy and wy + plan.win_h <= 187 and 0 <= wx and wx + plan.win_w <= 301
        assert (wy == 0 or cy - wy >= 18) and (wy + plan.win_h == 187 or wy + plan.win_h - cy - ch >= 18)
        assert (wx == 0 or cx - wx >= 18) and (wx + plan.win_w == 301 or wx + plan.win_w - cx - cw >= 18)
    assert int(seen.min()) == 1 and int(seen.max()) == 1
    # an image lower than one window keeps its height
    assert up.plan_windows(37, 301, 48, 18, 1, 4, 384, height8=True).win_h == 37
    # X4: multiples of lcm(align, 8)
    assert up.plan_windows(184, 304, 32, 20, 4, 4, 384, height8=True).win_h % 8 == 0


def test_plan_default_unchanged():
    """without the argument plan_windows returns what it returned before the argument existed (values recorded from the
    parent revision's rule: window height = cores of ceil(H / n) plus 2 halo, no rounding to 8)"""
    up = amd("upscale")
    for args in [(187, 301, 48, 18, 1, 4, 384), (184, 304, 32, 20, 4, 4, 384), (1080, 1920, 616, 52, 1, 4, None)]:
        a = up.plan_windows(*args)
        b = up.plan_windows(*args, height8=False)
        assert (a.win_h, a.win_w, a.windows, a.batch) == (b.win_h, b.win_w, b.windows, b.batch)
    p = up.plan_windows(187, 301, 48, 18, 1, 4, 384)
    assert (p.win_h, p.win_w, len(p), p.batch) == (83, 80, 28, 842)
    assert p.windows[0] == (0, 0, 0, 0, 47, 43) and p.windows[-1] == (104, 221, 141, 258, 46, 43)
    p = up.plan_windows(184, 304, 32, 20, 4, 4, 384)
    assert (p.win_h, p.win_w, len(p), p.batch) == (72, 72, 60, 1078)
    assert p.windows[0] == (0, 0, 0, 0, 32, 32) and p.windows[-1] == (112, 232, 160, 288, 24, 16)
    p = up.plan_windows(1080, 1920, 616, 52, 1, 4, None)
    assert (p.win_h, p.win_w, len(p), p.batch) == (644, 584, 8, 5)       # 8 windows of 644 x 584
    assert p.windows[-1] == (436, 1336, 540, 1440, 540, 480)


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    ops, C = amd("ops"), amd("_C")
    x = torch.zeros(1, 3, 4, 6)
    with pytest.raises(C.OfasrError):
        ops.d4_apply(x, 1)
    with pytest.raises(C.OfasrError):
        ops.d4_accumulate(x, 1, torch.zeros(1, 3, 4, 6), True, 1.0)
    with pytest.raises(C.OfasrError):
        ops.self_ensemble(lambda v: v, x, 2)
    for k in (3, 0, 16, -1, 2.5, True):
        with pytest.raises(ValueError):
            ops.self_ensemble(lambda v: v, x, k)
    assert ops.ENSEMBLE_SIZES == (1, 2, 4, 8)


def test_upscaler_refuses_bad_k():
    up = amd("upscale")
    for k in (3, 0, 16):
        with pytest.raises(ValueError):
            up.TiledUpscaler(torch.nn.Identity(), self_ensemble=k)


def test_entry_points_validate_arguments_without_gpu():
    import ctypes
    C = amd("_C")
    L = C.lib()
    assert L.ofasr_version() >= 306
    buf, buf2 = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    p, q = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf2, ctypes.c_void_p)
    assert L.ofasr_d4_apply(None, q, 1, 1, 2, 2, 0, 0, None) == -1
    assert L.ofasr_d4_apply(p, p, 1, 1, 2, 2, 0, 0, None) == -1          # in place
    assert L.ofasr_d4_apply(p, q, 1, 1, 2, 2, 8, 0, None) == -1          # t outside 0..7
    assert L.ofasr_d4_apply(p, q, 1, 1, 0, 2, 1, 0, None) == -1
    assert L.ofasr_d4_apply(p, q, 1, 1, 2, 2, 1, 7, None) == -1          # dtype
    assert L.ofasr_d4_apply(p, q, 1, 1, 1 << 16, 1 << 16, 1, 0, None) == -2
    assert L.ofasr_d4_accumulate(p, None, 1, 1, 2, 2, 0, 0, 1, 1.0, None) == -1
    assert L.ofasr_d4_accumulate(p, q, 1, 1, 2, 2, -1, 0, 1, 1.0, None) == -1
