"""Host statement of the training augmentation (data_providers/augment.py) against PIL itself: the nearest rotation bit
for bit over sizes x angles, the parameter draws against the provider's Compose under the same seed (values and number
of draws), and the refusals of the GPU entry point that need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import amd

Image = pytest.importorskip("PIL.Image")

SIZES = [(1, 1), (2, 2), (5, 7), (33, 17), (128, 96), (64, 64), (256, 256)]      # (w, h)
FIXED_ANGLES = [0.0, 90.0, -90.0, 180.0, 45.0, -45.0, 1e-9, -1e-9, 89.999999]


def _aug():
    return amd("imagenet_codebase.data_providers.augment")


def _angles(k):
    rng = np.random.RandomState(1000 + k)
    g = torch.Generator().manual_seed(2000 + k)
    draws = [float(torch.empty(1).uniform_(-90, 90, generator=g).item()) for _ in range(100)]
    return FIXED_ANGLES + rng.uniform(-360.0, 720.0, 300).tolist() + draws


def _image(w, h, seed):
    return np.random.RandomState(seed).randint(1, 256, (h, w, 3)).astype(np.uint8)    # no zeros: the fill is visible


@pytest.mark.parametrize("k", range(len(SIZES)))
def test_rotation_equals_pil(k):
    aug = _aug()
    w, h = SIZES[k]
    a = _image(w, h, k)
    pil = Image.fromarray(a)
    for angle in _angles(k):
        ref = np.asarray(pil.rotate(angle, Image.NEAREST, False, None))
        got = aug.rotate_nearest_np(a, angle)
        assert got.dtype == np.uint8 and got.shape == ref.shape
        assert np.array_equal(got, ref), "%dx%d angle %r: %d pixels differ" % (w, h, angle, int((got != ref).any(-1).sum()))


@pytest.mark.parametrize("S", [1, 2, 8, 30, 64])
def test_shortcut_angles_as_coefficients(S):
    """0 / 180 / 90 / 270 (and their aliases) as integer coefficients through the generic walk = PIL's transposes"""
    aug = _aug()
    a = _image(S, S, S)
    pil = Image.fromarray(a)
    for angle in (0.0, 90.0, -90.0, 180.0, -180.0, 270.0, 360.0, -270.0, 450.0):
        ref = np.asarray(pil.rotate(angle, Image.NEAREST, False, None))
        assert np.array_equal(aug.walk_fixed_np(a, aug.rotate_coeffs(angle, S)), ref), (S, angle)
    for angle in (45.0, -33.3, 1e-9):      # the generic angles take the same walk
        ref = np.asarray(pil.rotate(angle, Image.NEAREST, False, None))
        assert np.array_equal(aug.walk_fixed_np(a, aug.rotate_coeffs(angle, S)), ref), (S, angle)


def test_coefficients_fit_int32_at_the_largest_side():
    aug = _aug()
    S = aug.MAX_SIDE
    for angle in np.linspace(-360.0, 360.0, 2881):
        a0, a1, a2, a3, a4, a5 = aug.rotate_coeffs(float(angle), S)
        for (p, q, r) in ((a0, a1, a2), (a3, a4, a5)):
            worst = abs(r) + (S - 1) * (abs(p) + abs(q))
            assert worst < 2 ** 31, (angle, worst)


@pytest.mark.parametrize("seed", [0, 1, 7, 123, 99991])
@pytest.mark.parametrize("hw", [(41, 57), (16, 16), (16, 23)])
def test_parameter_draws_match_the_provider(seed, hw):
    aug = _aug()
    dp = amd("imagenet_codebase.data_providers.div2k_setxx")
    size = 16
    h, w = hw
    a = _image(w, h, seed)
    tf = dp.Compose([dp.RandomCrop(size), dp.RandomHorizontalFlip(), dp.RandomRotation(degrees=(-90, 90))])
    torch.manual_seed(seed)
    ref = np.asarray(tf(Image.fromarray(a)))
    ref_next = torch.rand(1)
    torch.manual_seed(seed)
    params = aug.draw_train_params(h, w, size)
    got = aug.apply_params_np(a, size, params)
    got_next = torch.rand(1)
    assert np.array_equal(got, ref)
    assert torch.equal(ref_next, got_next), "a different number of draws was consumed"
    if (h, w) == (size, size):
        assert params[:2] == (0, 0)


def test_refusals():
    aug = _aug()
    C, ops = amd("_C"), amd("ops")
    L = C.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 3 * 4097 * 4097
    assert L.ofasr_aug_gather_u8(p, big, p, 1, 4097, p, None, None) == -2 and b"4096" in L.ofasr_last_error_string()
    assert L.ofasr_aug_gather_u8(p, big, p, 65536, 8, p, None, None) == -2
    assert L.ofasr_aug_gather_u8(p, 3 * 8 * 8 - 1, p, 1, 8, p, None, None) == -2      # no H, W >= S image fits the pool
    assert L.ofasr_aug_gather_u8(None, 64, p, 1, 8, p, None, None) == -1
    with pytest.raises(ValueError):
        aug.rotate_coeffs(10.0, 4097)
    with pytest.raises(ValueError):            # H < S: refused where the table is made
        aug.make_table([(0, 7, 64, (0, 0, False, 0.0))], 8)
    with pytest.raises(ValueError):
        aug.make_table([(0, 64, 64, (57, 0, False, 0.0))], 8)
    with pytest.raises(ValueError):
        aug.draw_train_params(7, 64, 8)
    with pytest.raises(C.OfasrError):
        ops.aug_gather_u8(torch.zeros(3 * 64, dtype=torch.uint8), torch.zeros((1, 12), dtype=torch.int64), 1, 8)
    with pytest.raises(C.OfasrError):
        aug.ResidentTrainSet(["x.png"], "cpu")
