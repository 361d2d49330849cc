"""degrade.py, the host statement of the blind-SR degradation (Gaussian blur before the bicubic, Philox noise after it):
the generator's known answers, the tap rules, the blur's and the noise's properties, the table, the draw order, and the
run configs' refusals.  No GPU: the kernels are compared with this statement in tests/test_hip_degrade.py."""
import contextlib
import math

import numpy as np
import pytest
import torch

from conftest import amd

dg = amd("degrade")

KNOWN = [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    out = dg.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
    assert " ".join("%08x" % int(v) for v in out) == want


def test_philox_is_elementwise():
    rng = np.random.RandomState(0)
    c = rng.randint(0, 1 << 32, (5, 4)).astype(np.uint64)
    k = rng.randint(0, 1 << 32, (2,)).astype(np.uint64)
    whole = dg.philox4x32_10(c, k)
    for i in range(5):
        assert (whole[i] == dg.philox4x32_10(c[i], k)).all()


# ------------------------------------------------------------------------------------------------ taps
@pytest.mark.parametrize("sigma,radius", [(0.0, 0), (0.2, 1), (1.0 / 3.0, 1), (1.0, 3), (3.3, 10)])
def test_radius_rule(sigma, radius):
    assert dg.blur_radius(sigma) == radius == (0 if sigma == 0 else min(10, max(1, math.ceil(3 * sigma))))
    assert len(dg.blur_taps(sigma)) == 2 * radius + 1


@pytest.mark.parametrize("sigma", [0.0, 0.2, 1.0 / 3.0, 0.5, 1.0, 2.0, 3.3, 10.0 / 3.0])
def test_taps(sigma):
    t = dg.blur_taps(sigma)
    r = (len(t) - 1) // 2
    assert int(t.sum()) == 1 << 14
    assert (t == t[::-1]).all() and (t >= 0).all()
    assert (np.diff(t[:r + 1]) >= 0).all()                 # monotone up to the centre
    if sigma > 0:
        d = np.arange(-r, r + 1, dtype=np.float64)
        g = np.exp(-d * d / (2 * sigma * sigma))
        assert np.abs(t - g / g.sum() * (1 << 14)).max() <= r + 0.5 + 1e-9      # the centre takes the rounding residue


def test_small_sigma_is_the_identity():
    assert list(dg.blur_taps(0.2)) == [0, 16384, 0] and list(dg.blur_taps(0.0)) == [16384]


@pytest.mark.parametrize("sigma", [3.34, 10.0, -0.1, float("nan")])
def test_sigma_outside_the_range_is_refused(sigma):
    with pytest.raises(ValueError, match="sigma"):
        dg.blur_taps(sigma)


# ------------------------------------------------------------------------------------------------ blur
def _table(*rows):
    return dg.degrade_table(list(rows))


def test_blur_leaves_a_constant_image():
    for v in (0, 1, 127, 255):
        img = np.full((2, 3, 13, 9), v, np.uint8)
        assert (dg.blur_np(img, _table((3.3, 1.0, 0, False, 0), (0.5, 2.0, 0, False, 0))) == v).all()


def test_radius_zero_is_a_copy():
    img = np.random.RandomState(1).randint(0, 256, (1, 3, 11, 17)).astype(np.uint8)
    out = dg.blur_np(img, _table(dg.identity_row()))
    assert (out == img).all() and out is not img


def test_impulse_gives_the_two_pass_rounding_of_the_outer_product():
    sx, sy = 2.0, 1.0
    tx, ty = dg.blur_taps(sx), dg.blur_taps(sy)
    img = np.zeros((1, 3, 33, 33), np.uint8)
    img[:, :, 16, 16] = 255
    out = dg.blur_np(img, _table((sx, sy, 0, False, 0)))[0, 0].astype(np.int64)
    h = (255 * tx + (1 << 13)) >> 14                           # the impulse's row after the horizontal pass
    want = np.zeros((33, 33), np.int64)
    rx, ry = len(tx) // 2, len(ty) // 2
    want[16 - ry:16 + ry + 1, 16 - rx:16 + rx + 1] = (ty[:, None] * h[None, :] + (1 << 13)) >> 14
    assert (out == want).all() and out.max() > 0


def test_clamp_rule_on_a_one_row_plane():
    row = np.array([10, 200, 30, 90, 255], np.int64)
    img = np.broadcast_to(row.astype(np.uint8), (1, 3, 1, 5)).copy()
    t = dg.blur_taps(1.0)                                      # radius 3: wider than what is left of the plane
    out = dg.blur_np(img, _table((1.0, 1.0, 0, False, 0)))[0, 1, 0]
    h = [(sum(int(t[d + 3]) * int(row[min(max(x + d, 0), 4)]) for d in range(-3, 4)) + 8192) >> 14 for x in range(5)]
    assert list(out) == h                                      # the vertical pass sees one row seven times: no change


# ------------------------------------------------------------------------------------------------ noise
@pytest.fixture(scope="module")
def flat():
    return np.full((1, 3, 512, 512), 128, np.uint8)            # 2^18 pixels a channel


@pytest.mark.parametrize("sigma", [1.0, 5.0, 25.0])
def test_noise_statistics(flat, sigma):
    out = dg.noise_np(flat, _table((0, 0, sigma, False, 77)), seed=123456789012345, scale=2)
    for c in range(3):
        e = out[0, c].astype(np.float64) - 128.0
        want = math.sqrt(sigma * sigma + 1.0 / 12.0)           # the rounding to integers adds a uniform's variance
        print("sigma %g channel %d: std %.4f (want %.4f), mean %.4f" % (sigma, c, e.std(), want, e.mean()))
        assert abs(e.std() / want - 1.0) < 0.01
        assert abs(e.mean()) < 0.1 * sigma
    assert (out[0, 0] != out[0, 1]).any() and (out[0, 1] != out[0, 2]).any()


def test_gray_noise_is_equal_in_the_three_channels(flat):
    out = dg.noise_np(flat[:, :, :64, :64], _table((0, 0, 10.0, True, 5)), seed=9, scale=4)
    colour = dg.noise_np(flat[:, :, :64, :64], _table((0, 0, 10.0, False, 5)), seed=9, scale=4)
    assert (out[0, 0] == out[0, 1]).all() and (out[0, 0] == out[0, 2]).all()
    assert (out[0, 0] == colour[0, 0]).all()                   # channel 0's value


def test_amplitude_zero_is_a_copy_and_the_output_is_clipped():
    img = np.random.RandomState(2).randint(0, 256, (2, 3, 9, 7)).astype(np.uint8)
    assert (dg.noise_np(img, _table(dg.identity_row(3), dg.identity_row(4)), 1, 2) == img).all()
    for v in (0, 255):
        out = dg.noise_np(np.full((1, 3, 32, 32), v, np.uint8), _table((0, 0, 50.0, False, 1)), 1, 2)
        assert ((out == v).mean() > 0.4) and (out != v).any()  # about half the noise points outside the range


def test_stream_scale_and_seed_change_the_noise(flat):
    img = flat[:, :, :32, :32]
    base = dg.noise_np(img, _table((0, 0, 10.0, False, 5)), 9, 2)
    assert (base == dg.noise_np(img, _table((0, 0, 10.0, False, 5)), 9, 2)).all()
    assert (base != dg.noise_np(img, _table((0, 0, 10.0, False, 6)), 9, 2)).any()
    assert (base != dg.noise_np(img, _table((0, 0, 10.0, False, 5)), 9, 4)).any()
    assert (base != dg.noise_np(img, _table((0, 0, 10.0, False, 5)), 10, 2)).any()
    assert (base != dg.noise_np(img, _table((0, 0, 10.0, False, 5)), 9 + (1 << 32), 2)).any()      # the key's high word
    with pytest.raises(ValueError, match="scale"):
        dg.noise_np(img, _table(dg.identity_row()), 9, 3)


def test_amplitude():
    assert dg.noise_amplitude(0) == 0 and dg.noise_amplitude(1) == 222 == round(65536 / 295.601)
    assert dg.noise_amplitude(50) * 2040 < 1 << 25
    with pytest.raises(ValueError, match="noise sigma"):
        dg.noise_amplitude(50.5)


# ------------------------------------------------------------------------------------------------ table
def test_table_layout():
    t = _table((1.0, 0.0, 5.0, True, 1234567), (0.2, 3.3, 0.0, False, (1 << 31) - 1))
    assert t.dtype == np.int32 and t.shape == (2, 48)
    assert list(t[0, :6]) == [3, 0, dg.noise_amplitude(5.0), 1, 1234567, 0]
    assert list(t[0, 16 - 3:16 + 4]) == list(dg.blur_taps(1.0)) and t[0, 6:13].sum() == 0 and t[0, 20:27].sum() == 0
    assert t[0, 37] == 16384 and t[0, 27:37].sum() == 0 and t[0, 38:48].sum() == 0
    assert list(t[1, :6]) == [1, 10, 0, 0, (1 << 31) - 1, 0]
    assert list(t[1, 27:48]) == list(dg.blur_taps(3.3)) and list(t[1, 15:18]) == [0, 16384, 0]
    out = torch.zeros((4, 48), dtype=torch.int32)
    got = dg.degrade_table([(1.0, 0.0, 5.0, True, 1234567)], out=out)
    assert got.shape == (1, 48) and (got.numpy() == t[:1]).all() and (out[0].numpy() == t[0]).all()
    with pytest.raises(ValueError, match="stream"):
        _table((0, 0, 0, False, 1 << 31))


def test_degrade_np_is_blur_bicubic_noise():
    from oracle import pil_bicubic
    img = np.random.RandomState(3).randint(0, 256, (2, 3, 24, 40)).astype(np.uint8)
    t = _table((1.5, 0.7, 8.0, False, 11), dg.identity_row(12))
    lr = dg.degrade_np(img, t, seed=4)
    blurred = dg.blur_np(img, t)
    for f in (2, 4):
        assert lr[f].shape == (2, 3, 24 // f, 40 // f)
        assert (lr[f] == dg.noise_np(pil_bicubic.scale_down(blurred, f), t, 4, f)).all()
        assert (lr[f][1] == pil_bicubic.scale_down(img[1], f)).all()          # the identity row: Pillow's clean bicubic
    b = dg.batch_np(img, t, 4)
    assert b["image"].dtype == np.float32 and (b["image"] == img.astype(np.float32) / np.float32(255)).all()


# ------------------------------------------------------------------------------------------------ draws
SPEC = {"blur": (0.5, 3.0), "aniso": True, "noise": (1.0, 20.0), "gray_prob": 0.4, "prob": 0.7}


def _hand_drawn(spec):
    u = [float(v) for v in torch.rand(5).double().tolist()]
    stream = int(torch.randint(0, 2 ** 31, (1,)).item())
    if u[0] >= spec["prob"]:
        return (0.0, 0.0, 0.0, False, stream)
    lo, hi = spec["blur"]
    sx = lo + (hi - lo) * u[1]
    sy = lo + (hi - lo) * u[2] if spec["aniso"] else sx
    return (sx, sy, spec["noise"][0] + (spec["noise"][1] - spec["noise"][0]) * u[3], u[4] < spec["gray_prob"], stream)


def test_draws_take_a_fixed_count_per_sample():
    spec = dg.check_spec(SPEC)
    torch.manual_seed(5)
    rows = [dg.draw_degrade(spec) for _ in range(40)]
    after = torch.rand(1).item()
    torch.manual_seed(5)
    assert rows == [_hand_drawn(spec) for _ in range(40)]
    assert torch.rand(1).item() == after
    kinds = {r[:4] == (0.0, 0.0, 0.0, False) for r in rows}
    assert kinds == {True, False}                              # degraded and identity rows alike took the same draws
    assert all(0 <= r[4] < 1 << 31 for r in rows)
    assert any(r[0] != r[1] for r in rows) and any(r[3] for r in rows)
    torch.manual_seed(5)
    iso = [dg.draw_degrade(dict(spec, aniso=False)) for _ in range(40)]
    assert all(r[0] == r[1] for r in iso) and [r[0] for r in iso] == [r[0] for r in rows]


def test_prob_zero_gives_identity_rows():
    spec = dg.check_spec(dict(SPEC, prob=0.0))
    torch.manual_seed(6)
    rows = [dg.draw_degrade(spec) for _ in range(8)]
    assert all(r[:4] == (0.0, 0.0, 0.0, False) for r in rows)
    t = dg.degrade_table(rows)
    assert (t[:, :4] == 0).all() and (t[:, 16] == 16384).all() and (t[:, 37] == 16384).all()
    assert (t[:, 4] == [r[4] for r in rows]).all()


@pytest.mark.parametrize("bad,word", [
    ({"blur": (2.0, 1.0)}, "LO <= HI"), ({"blur": (0.0, 3.5)}, "above the limit"), ({"noise": (0.0, 51.0)}, "above the limit"),
    ({"noise": (-1.0, 2.0)}, "LO <= HI"), ({"prob": 1.5}, "probability"), ({"gray_prob": -0.1}, "probability"),
    ({"blurr": (0, 1)}, "unknown key"), ({"blur": 3}, "range LO:HI")])
def test_bad_specs_are_refused(bad, word):
    with pytest.raises(ValueError, match=word):
        dg.check_spec(bad)


def test_spec_defaults():
    assert dg.check_spec(None) is None
    assert dg.check_spec({"noise": [1, 2]}) == {"blur": (0.0, 0.0), "aniso": False, "noise": (1.0, 2.0), "gray_prob": 0.0,
                                                "prob": 1.0}


# the loader on a stand-in device: what a batch draws from the torch global RNG, without a GPU
class _Set(object):
    device = "cpu"

    def __init__(self, sizes):
        self.entries = [(0, h, w) for (h, w) in sizes]
        self.paths = ["img%d" % k for k in range(len(sizes))]
        self.pool = torch.zeros(1, dtype=torch.uint8)


@pytest.fixture
def host_loader(monkeypatch):
    aug, ops = amd("imagenet_codebase.data_providers.augment"), amd("ops")

    class _Event(object):
        def record(self):
            pass

        def synchronize(self):
            pass
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(ops, "aug_gather_u8", lambda pool, table, n, S, want_f32=False: torch.zeros((n, 3, S, S), dtype=torch.uint8))

    def make(**kw):
        return aug.ResidentTrainLoader(_Set([(40, 56), (33, 47), (16, 16)]), 3, [0, 1, 2], 16, **kw)
    return aug, make


def test_loader_without_degrade_draws_what_it_always_drew(host_loader):
    aug, make = host_loader
    torch.manual_seed(7)
    hand = [aug.draw_train_params(h, w, 16) for (h, w) in [(40, 56), (33, 47), (16, 16)]]
    after = torch.rand(1).item()
    for kw in ({}, {"degrade": None}):
        torch.manual_seed(7)
        loader = make(**kw)
        batch = loader.batch([0, 1, 2])
        assert torch.rand(1).item() == after
        assert loader.last_params == hand and loader.last_degrade is None
        assert sorted(batch) == ["image_u8"]


def test_loader_draws_the_degrade_rows_after_all_crop_draws(host_loader):
    aug, make = host_loader
    spec = dg.check_spec(SPEC)
    torch.manual_seed(8)
    hand = [aug.draw_train_params(h, w, 16) for (h, w) in [(40, 56), (33, 47), (16, 16)]]
    rows = [_hand_drawn(spec) for _ in range(3)]
    after = torch.rand(1).item()
    torch.manual_seed(8)
    loader = make(degrade=SPEC, degrade_seed=99)
    batch = loader.batch([0, 1, 2])
    assert torch.rand(1).item() == after
    assert loader.last_params == hand and loader.last_degrade == rows
    assert batch["degrade_seed"] == 99 and batch["degrade"].dtype == torch.int32
    assert (batch["degrade"].numpy() == dg.degrade_table(rows)).all()
    given = [dg.identity_row(1), (1.0, 2.0, 3.0, True, 2), dg.identity_row(3)]
    batch = loader.batch([2, 1, 0], degrade_rows=given)
    assert loader.last_degrade == given and (batch["degrade"].numpy() == dg.degrade_table(given)).all()
    with pytest.raises(ValueError, match="degrade rows"):
        loader.batch([0, 1], degrade_rows=given)


def test_a_paired_set_refuses_degrade(host_loader):
    _, make = host_loader
    ds = _Set([(32, 32)])
    ds.make_table = lambda *a, **k: None
    aug = amd("imagenet_codebase.data_providers.augment")
    with pytest.raises(ValueError, match="degrade= with a paired set"):
        aug.ResidentTrainLoader(ds, 1, [0], 16, degrade=SPEC)


# ------------------------------------------------------------------------------------------------ run configs
def test_run_configs_carry_the_spec_only_when_set():
    rm = amd("imagenet_codebase.run_manager")
    with pytest.raises(ValueError, match="degrade= needs resident=True"):
        rm.Div2K_SetXXRunConfig(degrade=SPEC)
    cfg = rm.Div2K_SetXXRunConfig(degrade=SPEC, degrade_seed=3, resident=True)
    assert cfg.config["degrade"] == dg.check_spec(SPEC) and cfg.config["degrade_seed"] == 3
    import json
    json.dumps(cfg.config)                                     # run.config holds it as it is
    plain = rm.Div2K_SetXXRunConfig(resident=True).config
    assert "degrade" not in plain and "degrade_seed" not in plain and "lr_on_device" not in plain
    assert "degrade" not in rm.VideoFramesRunConfig(videos=["a.y4m"]).config
    assert rm.VideoFramesRunConfig(videos=["a.y4m"], degrade=SPEC).config["degrade"]["aniso"] is True
    with pytest.raises(ValueError, match="degrade= with videos_lr"):
        rm.VideoFramesRunConfig(videos=["a.y4m"], videos_lr=["b.y4m"], degrade=SPEC)
    with pytest.raises(ValueError, match="above the limit"):
        rm.Div2K_SetXXRunConfig(degrade={"blur": (0, 4)}, resident=True)
