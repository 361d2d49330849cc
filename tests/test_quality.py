"""The Y-PSNR / Y-SSIM definition on the host (utils.y_exact, utils.ssim_y, utils.sse_y) against an fp64 oracle kept in
this file, and the C ABI of the GPU metric (ofasr_quality_y, ofasr_quality_mse): argument validation and the workspace
queries, which run before any launch and therefore on a GPU-less host."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import amd


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_luma(u8):
    """round_half_even((65481 R + 128553 G + 24966 B) / 255000 + 16) with Python integers per distinct value"""
    c = u8.astype(np.int64)
    num = 65481 * c[..., 0] + 128553 * c[..., 1] + 24966 * c[..., 2] + 16 * 255000
    twice = 2 * num                                   # y = round_half_even(twice / 510000)
    lo = twice // 510000
    rem = twice - lo * 510000
    y = np.where(rem > 255000, lo + 1, np.where(rem < 255000, lo, lo + (lo & 1)))
    return y.astype(np.uint8)


def oracle_quant(x):
    """NCHW float -> NHWC uint8: clamp, * 255 in fp32, round half to even"""
    x = np.asarray(x, dtype=np.float32)
    return np.transpose(np.rint(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)), (0, 2, 3, 1)).astype(np.uint8)


def oracle_window():
    g = np.exp(-0.5 * ((np.arange(11, dtype=np.float64) - 5.0) / 1.5) ** 2)
    return g / g.sum()


def oracle_ssim_map(a, b):
    """SSIM map of two 2-D fp64 images: dense 11x11 window (the outer product), valid positions, direct sums"""
    g = oracle_window()
    win = np.outer(g, g)
    H, W = a.shape
    h, w = H - 10, W - 10

    def filt(x):
        out = np.zeros((h, w))
        for i in range(11):
            for j in range(11):
                out += win[i, j] * x[i:i + h, j:j + w]
        return out

    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    m1, m2 = filt(a), filt(b)
    s1, s2, s12 = filt(a * a) - m1 * m1, filt(b * b) - m2 * m2, filt(a * b) - m1 * m2
    return ((2 * m1 * m2 + c1) * (2 * s12 + c2)) / ((m1 * m1 + m2 * m2 + c1) * (s1 + s2 + c2))


def oracle_quality(ya, yb, shave=0):
    """(sse, ssim) of two uint8 Y images"""
    if shave:
        ya, yb = ya[shave:-shave, shave:-shave], yb[shave:-shave, shave:-shave]
    d = ya.astype(np.int64) - yb.astype(np.int64)
    return int((d * d).sum()), float(oracle_ssim_map(ya.astype(np.float64), yb.astype(np.float64)).mean())


def image_pair(n, h, w, seed):
    """structured content plus noise, values below 0 and above 1: (output, target) NCHW fp32"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.5 + 0.6 * np.sin(xx / (3.0 + c) + yy / 7.0 + i) * np.cos(yy / (4.0 + i)) for i in range(n)
                     for c in range(3)]).reshape(n, 3, h, w)
    tgt = base + rng.uniform(-0.15, 0.15, base.shape)
    out = tgt + rng.normal(0, 0.08, base.shape) + 0.05 * np.sin(xx / 2.0)
    return out.astype(np.float32), tgt.astype(np.float32)


# ------------------------------------------------------------------------------------------------ luma
def test_y_exact_all_colours():
    utils = amd("utils")
    v = np.arange(256, dtype=np.uint8)
    ties = 0
    for r in range(256):
        col = np.empty((256, 256, 3), dtype=np.uint8)
        col[..., 0] = r
        col[..., 1] = v[:, None]
        col[..., 2] = v[None, :]
        y = utils.y_exact(col)
        assert np.array_equal(y, oracle_luma(col)), r
        num = 65481 * int(r) + 128553 * col[..., 1].astype(np.int64) + 24966 * col[..., 2].astype(np.int64)
        tie = num % 255000 == 127500
        ties += int(tie.sum())
        diff = y != utils.rgb2y(col)
        assert not np.any(diff & ~tie), "y_exact differs from rgb2y at a colour that is not a tie (R = %d)" % r
    assert ties == 194


def test_y_exact_range_and_ties():
    utils = amd("utils")
    assert utils.y_exact(np.array([[0, 0, 0], [255, 255, 255]], dtype=np.uint8)).tolist() == [16, 235]
    # a tie colour: 65481 R + 128553 G + 24966 B = 255000 k + 127500
    found = None
    for r in range(256):
        for g in range(256):
            rest = 65481 * r + 128553 * g
            b = np.arange(256)
            hit = b[(rest + 24966 * b) % 255000 == 127500]
            if len(hit):
                found = (r, g, int(hit[0]))
                break
        if found:
            break
    num = 65481 * found[0] + 128553 * found[1] + 24966 * found[2]
    lo = num // 255000 + 16
    assert int(utils.y_exact(np.array([found], dtype=np.uint8))[0]) == (lo if lo % 2 == 0 else lo + 1)


# ------------------------------------------------------------------------------------------------ ssim_y
SIZES = [(1, 11, 11), (3, 12, 37), (1, 64, 96), (2, 45, 31)]


@pytest.mark.parametrize("n,h,w", SIZES)
def test_ssim_y_matches_oracle(n, h, w):
    utils = amd("utils")
    out, tgt = image_pair(n, h, w, h * w)
    got = utils.ssim_y(out, tgt)
    sse, count = utils.sse_y(out, tgt)
    assert count == h * w
    qa, qb = oracle_quant(out), oracle_quant(tgt)
    for i in range(n):
        e, s = oracle_quality(oracle_luma(qa[i]), oracle_luma(qb[i]))
        print("ssim_y %r oracle %r  sse %d oracle %d" % (got[i], s, sse[i], e))
        assert abs(got[i] - s) <= 1e-12
        assert sse[i] == e
        assert 0.05 < s < 0.999            # not degenerate
    # the PSNR formed from (sse, count) is utils.psnr on the same Y images, bit for bit
    for i in range(n):
        assert utils.psnr_from_sse(sse[i], count) == utils.psnr(oracle_luma(qa[i]), oracle_luma(qb[i]))


def test_oracle_agrees_with_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    out, tgt = image_pair(1, 40, 52, 5)
    a = oracle_luma(oracle_quant(out)[0]).astype(np.float64)
    b = oracle_luma(oracle_quant(tgt)[0]).astype(np.float64)
    g = oracle_window()

    def filt(x):
        y = ndi.correlate1d(ndi.correlate1d(x, g, axis=0, mode="constant"), g, axis=1, mode="constant")
        return y[5:-5, 5:-5]

    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    m1, m2 = filt(a), filt(b)
    s1, s2, s12 = filt(a * a) - m1 * m1, filt(b * b) - m2 * m2, filt(a * b) - m1 * m2
    ref = (((2 * m1 * m2 + c1) * (2 * s12 + c2)) / ((m1 * m1 + m2 * m2 + c1) * (s1 + s2 + c2))).mean()
    assert abs(ref - oracle_ssim_map(a, b).mean()) <= 1e-12


def test_ssim_y_identical_symmetric_shave():
    utils = amd("utils")
    out, tgt = image_pair(2, 37, 41, 2)
    assert utils.ssim_y(out, out) == [1.0, 1.0]
    assert utils.sse_y(out, out)[0] == [0, 0] and utils.psnr_from_sse(0, 10) == float("inf")
    assert utils.ssim_y(out, tgt) == utils.ssim_y(tgt, out)
    assert utils.ssim_y(out, tgt, shave=4) == utils.ssim_y(out[:, :, 4:-4, 4:-4], tgt[:, :, 4:-4, 4:-4])
    assert utils.sse_y(out, tgt, shave=4) == utils.sse_y(out[:, :, 4:-4, 4:-4], tgt[:, :, 4:-4, 4:-4])
    # uint8 HWC operands are taken as they are; torch tensors are accepted
    qa, qb = oracle_quant(out), oracle_quant(tgt)
    assert utils.ssim_y(qa[1], qb[1]) == utils.ssim_y(out, tgt)[1:]
    assert utils.ssim_y(torch.from_numpy(out), torch.from_numpy(tgt)) == utils.ssim_y(out, tgt)
    with pytest.raises(ValueError, match="below the 11-pixel"):
        utils.ssim_y(out, tgt, shave=14)          # 37 - 28 = 9
    with pytest.raises(ValueError, match="negative"):
        utils.ssim_y(out, tgt, shave=-1)
    with pytest.raises(ValueError, match="shape"):
        utils.ssim_y(out, tgt[:, :, :-1])


# ------------------------------------------------------------------------------------------------ C ABI
def test_quality_abi_validation_without_gpu():
    C = amd("_C")
    L = C.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    n = ctypes.c_size_t(4096)

    def err():
        return L.ofasr_last_error_string()

    assert L.ofasr_quality_y(None, 0, p, 0, 1, 16, 16, 0, p, p, p, n, None) == -1 and b"null" in err()
    assert L.ofasr_quality_y(p, 0, p, 0, 1, 16, 16, 0, None, p, p, n, None) == -1 and b"null" in err()
    assert L.ofasr_quality_y(p, 0, p, 0, 1, 16, 16, 0, p, None, p, n, None) == -1 and b"null" in err()
    assert L.ofasr_quality_y(p, 0, p, 0, 1, 10, 16, 0, p, p, p, n, None) == -1 and b"window" in err()    # side < 11
    assert L.ofasr_quality_y(p, 0, p, 0, 1, 16, 18, 3, p, p, p, n, None) == -1 and b"window" in err()    # after shave
    assert L.ofasr_quality_y(p, 0, p, 0, 1, 16, 16, -1, p, p, p, n, None) == -1 and b"negative shave" in err()
    assert L.ofasr_quality_y(p, 4, p, 0, 1, 16, 16, 0, p, p, p, n, None) == -1 and b"format" in err()
    assert L.ofasr_quality_y(p, 0, p, -1, 1, 16, 16, 0, p, p, p, n, None) == -1 and b"format" in err()
    assert L.ofasr_quality_y(p, C.U8_HWC, p, 0, 2, 16, 16, 0, p, p, p, n, None) == -1 and b"one image" in err()
    assert L.ofasr_quality_y(p, 0, p, 0, 0, 16, 16, 0, p, p, p, n, None) == -1
    assert L.ofasr_quality_y(p, 0, p, 0, 1, 16, 16, 0, p, p, None, 0, None) == -3 and b"workspace" in err()
    assert L.ofasr_quality_y(p, 0, p, 0, 1, 64, 64, 0, p, p, p, 16, None) == -3
    assert L.ofasr_quality_mse(None, 0, p, 0, 1, 16, p, p, n, None) == -1 and b"null" in err()
    assert L.ofasr_quality_mse(p, C.U8_HWC, p, 0, 1, 16, p, p, n, None) == -1 and b"f32" in err()
    assert L.ofasr_quality_mse(p, 0, p, 0, 1, 0, p, p, n, None) == -1
    assert L.ofasr_quality_mse(p, 0, p, 0, 1, 16, p, None, 0, None) == -3


def test_quality_workspace_is_host_only():
    L = amd("_C").lib()
    one = L.ofasr_quality_y_workspace(1, 11, 11, 0)
    assert one > 0
    assert L.ofasr_quality_y_workspace(3, 11, 11, 0) == 3 * one
    assert L.ofasr_quality_y_workspace(1, 11 + 32, 11 + 64, 0) == 2 * 3 * one        # tiles of 32 x 32 positions
    assert L.ofasr_quality_y_workspace(1, 19 + 32, 19 + 64, 4) == 2 * 3 * one
    assert L.ofasr_quality_y_workspace(1, 4320, 7680, 0) < (1 << 20)
    assert L.ofasr_quality_y_workspace(1, 10, 64, 0) == 0 and L.ofasr_quality_y_workspace(1, 64, 64, -1) == 0
    assert L.ofasr_quality_y_workspace(0, 64, 64, 0) == 0 and L.ofasr_quality_y_workspace(1, 16, 16, 3) == 0
    assert L.ofasr_quality_mse_workspace(4, 3 * 64 * 64) > 0 and L.ofasr_quality_mse_workspace(4, 0) == 0


def test_quality_ops_refuse_cpu_tensors():
    ops, utils, C = amd("ops"), amd("utils"), amd("_C")
    a = torch.zeros(1, 3, 16, 16)
    with pytest.raises(C.OfasrError):
        ops.quality_y(a, a)
    with pytest.raises(C.OfasrError):
        ops.quality_mse(a, a)
    with pytest.raises(C.OfasrError):
        utils.quality_y_device(a, a)
