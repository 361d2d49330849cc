"""ofasr_degrade_blur_u8 / ofasr_degrade_noise_u8 (csrc/degrade.hip), ops.lr_images_from_u8(degrade=) and the degrading
resident loader on the GPU against the host statement (degrade.py, itself pinned by tests/test_degrade.py): bit for bit.

The blur kernel's tile is DG_TW x DG_TH = 64 x 32 output pixels with a halo of DG_HALO = 10 (csrc/degrade.hip): (16, 16)
is smaller than the halo, (75, 139) and (97, 161) span two or three tiles plus a ragged rest on each axis.  The noise
kernel takes 4 flat indices per lane: 1 x 5, 33 x 47, 75 x 139 and 97 x 161 leave a ragged rest, and their planes are
not 4-byte aligned inside the batch."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import amd
from test_video_pair import write_video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANES = [(1, 5), (16, 16), (33, 47), (97, 161), (75, 139)]
SIGMA_OF_RADIUS = {0: 0.0, 1: 0.3, 3: 1.0, 10: 3.3}
BLUR_ROWS = [(0, 10), (1, 3), (3, 0), (10, 1)]             # (r_x, r_y), mixed within one batch of 4
NOISE_ROWS = [(0, 0), (222, 0), (11086, 1), (11086, 0), (222, 1)]      # (a, gray)
SEED = 0x123456789ABCDEF

dg = amd("degrade")


def _blur_table():
    rows = [(SIGMA_OF_RADIUS[rx], SIGMA_OF_RADIUS[ry], 0.0, False, 0) for rx, ry in BLUR_ROWS]
    t = dg.degrade_table(rows)
    assert [tuple(r) for r in t[:, :2]] == BLUR_ROWS
    return t


def _noise_table():
    t = dg.degrade_table([dg.identity_row(1000 + k) for k in range(len(NOISE_ROWS))])
    for k, (a, gray) in enumerate(NOISE_ROWS):
        t[k, 2], t[k, 3] = a, gray
    return t


@pytest.fixture(scope="module")
def ref():
    """the inputs and what the host statement makes of them, computed once"""
    rng = np.random.RandomState(31)
    bt, nt = _blur_table(), _noise_table()
    out = {"blur_table": bt, "noise_table": nt, "blur": {}, "noise": {}}
    for (h, w) in PLANES:
        img = rng.randint(0, 256, (len(BLUR_ROWS), 3, h, w)).astype(np.uint8)
        out["blur"][(h, w)] = (img, dg.blur_np(img, bt))
        img = rng.randint(0, 256, (len(NOISE_ROWS), 3, h, w)).astype(np.uint8)
        img[:, :, 0, :2] = (0, 255)                        # the clip on both sides
        out["noise"][(h, w)] = (img, {f: dg.noise_np(img, nt, SEED, f) for f in (2, 4)})
    return out


def _at(host, lead):
    """`host` on the device, `lead` bytes past a 4-byte aligned address, in its own shape"""
    buf = torch.empty(host.size + lead + 3, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0
    dev = buf[lead:lead + host.size].view(host.shape)
    dev.copy_(torch.from_numpy(host))
    return dev


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("plane", PLANES)
def test_blur_equals_the_host_statement(ref, plane, lead):
    C = amd("_C")
    img, want = ref["blur"][plane]
    table = torch.from_numpy(ref["blur_table"]).to(DEV)
    src = _at(img, lead)
    dst = _at(np.zeros_like(img), lead)                    # lead = 1: byte loads AND byte stores
    n, _, h, w = img.shape
    C.check(C.lib().ofasr_degrade_blur_u8(_p(src), _p(table), n, h, w, 10, _p(dst), _stream()), "blur")
    assert np.array_equal(dst.cpu().numpy(), want)
    if lead == 0:                                          # the module-level op: a fresh, aligned output
        assert np.array_equal(amd("ops").degrade_blur_u8(_at(img, 1), table).cpu().numpy(), want)


def test_blur_of_one_256_sample():
    rng = np.random.RandomState(32)
    img = rng.randint(0, 256, (1, 3, 256, 256)).astype(np.uint8)
    t = dg.degrade_table([(3.3, 1.0, 0.0, False, 0)])
    got = amd("ops").degrade_blur_u8(torch.from_numpy(img).to(DEV), torch.from_numpy(t).to(DEV))
    assert np.array_equal(got.cpu().numpy(), dg.blur_np(img, t))


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("plane", PLANES)
def test_noise_equals_the_host_statement(ref, plane, scale, lead):
    C, ops = amd("_C"), amd("ops")
    img, want = ref["noise"][plane]
    want = want[scale]
    table = torch.from_numpy(ref["noise_table"]).to(DEV)
    n, _, h, w = img.shape
    src, dst = _at(img, lead), _at(np.zeros_like(img), lead)
    f32 = torch.zeros(img.shape, dtype=torch.float32, device=DEV)
    C.check(C.lib().ofasr_degrade_noise_u8(_p(src), _p(table), SEED & 0xFFFFFFFF, SEED >> 32, scale, n, h, w, _p(dst),
                                           _p(f32), _stream()), "noise")
    assert np.array_equal(dst.cpu().numpy(), want)                                     # out of place
    assert np.array_equal(src.cpu().numpy(), img)
    assert np.array_equal(f32.cpu().numpy(), want.astype(np.float32) / np.float32(255.0))   # the 256 quotients v / 255
    assert np.array_equal(want[0], img[0]) and (want[1] != img[1]).any()               # a = 0 is a copy
    C.check(C.lib().ofasr_degrade_noise_u8(_p(src), _p(table), SEED & 0xFFFFFFFF, SEED >> 32, scale, n, h, w, _p(src),
                                           None, _stream()), "noise in place")
    assert np.array_equal(src.cpu().numpy(), want)
    if lead == 0:
        x = torch.from_numpy(img).to(DEV)
        u8, f = ops.degrade_noise_u8(x, table, SEED, scale, want_f32=True)
        assert np.array_equal(u8.cpu().numpy(), want) and torch.equal(f, f32)
        assert ops.degrade_noise_u8(x, table, SEED, scale, out=x) is x and np.array_equal(x.cpu().numpy(), want)


def test_noise_of_one_256_sample():
    img = np.full((1, 3, 256, 256), 128, np.uint8)
    t = dg.degrade_table([(0.0, 0.0, 25.0, False, 7)])
    got = amd("ops").degrade_noise_u8(torch.from_numpy(img).to(DEV), torch.from_numpy(t).to(DEV), 5, 4)
    assert np.array_equal(got.cpu().numpy(), dg.noise_np(img, t, 5, 4))


# ---------------------------------------------------------------------------------------------- the composite
@pytest.mark.parametrize("S", [32, 48])
def test_lr_images_equal_the_host_statement(S):
    ops = amd("ops")
    rng = np.random.RandomState(33 + S)
    hr = rng.randint(0, 256, (4, 3, S, S)).astype(np.uint8)
    t = dg.degrade_table([(2.0, 0.5, 10.0, False, 1), dg.identity_row(2), (0.0, 3.3, 0.0, False, 3), (1.0, 1.0, 50.0, True, 4)])
    want = dg.batch_np(hr, t, SEED)
    x = torch.from_numpy(hr).to(DEV)
    image = ops._unit_lut(x.device)[x.long()]
    got = ops.lr_images_from_u8(x, image=image, degrade=torch.from_numpy(t).to(DEV), degrade_seed=SEED)
    assert sorted(got) == sorted(want) and got["image"] is image
    for k in want:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    clean = ops.lr_images_from_u8(x, image=image)
    assert torch.equal(got["2x_down_image"][1], clean["2x_down_image"][1])          # the identity row: the clean bicubic
    assert not torch.equal(got["2x_down_image"][0], clean["2x_down_image"][0])
    none = ops.lr_images_from_u8(x, image=image, degrade=None)
    assert all(torch.equal(none[k], clean[k]) for k in clean)
    with pytest.raises(amd("_C").OfasrError, match="given="):
        ops.lr_images_from_u8(x, image=image, given={2: clean["2x_down_image"]}, degrade=torch.from_numpy(t).to(DEV))


# ---------------------------------------------------------------------------------------------- the loader
SPEC = {"blur": (0.2, 3.3), "aniso": True, "noise": (0.0, 30.0), "gray_prob": 0.5, "prob": 0.8}


def _check_batches(loader, image_of, batches, S):
    aug, utils = amd("imagenet_codebase.data_providers.augment"), amd("utils")
    for indices in batches:
        raw = loader.batch(indices)
        assert raw["degrade"].dtype == torch.int32 and tuple(raw["degrade"].shape) == (len(indices), 48)
        got = utils.device_batch(raw, DEV)
        params = loader.last_params
        if loader.candidates > 1:
            params = [ps[c] for ps, c in zip(params, loader.last_choice.tolist())]
        hr = np.stack([aug.apply_params_np(image_of(k), S, p).transpose(2, 0, 1) for k, p in zip(indices, params)])
        assert len(loader.last_degrade) == len(indices)
        want = dg.batch_np(hr, dg.degrade_table(loader.last_degrade), loader.degrade_seed)
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(got[k].cpu().numpy(), want[k]), k


@pytest.mark.parametrize("K", [1, 2])
def test_array_set_loader(K):
    aug = amd("imagenet_codebase.data_providers.augment")
    rng = np.random.RandomState(34)
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for (h, w) in [(40, 56), (33, 47), (24, 24)]]
    rs = aug.ResidentArraySet(imgs, DEV)
    torch.manual_seed(35)
    loader = aug.ResidentTrainLoader(rs, 3, [0, 1, 2], 24, want_f32=True, degrade=SPEC, degrade_seed=SEED,
                                     **({} if K == 1 else {"candidates": K}))
    _check_batches(loader, lambda k: imgs[k], [[0, 1, 2], [2, 0, 1]], 24)


def test_loader_rng_use():
    """without the option the loader draws what it always drew; with it, the rows come after all crop draws"""
    aug = amd("imagenet_codebase.data_providers.augment")
    sizes = [(40, 56), (33, 47)]
    rs = aug.ResidentArraySet([np.zeros((h, w, 3), np.uint8) for (h, w) in sizes], DEV)
    spec = dg.check_spec(SPEC)
    torch.manual_seed(36)
    hand = [aug.draw_train_params(h, w, 24) for (h, w) in sizes]
    mark_plain = torch.get_rng_state()
    rows = [dg.draw_degrade(spec) for _ in sizes]
    mark_degrade = torch.get_rng_state()
    torch.manual_seed(36)
    plain = aug.ResidentTrainLoader(rs, 2, [0, 1], 24, degrade=None)
    assert sorted(plain.batch([0, 1])) == ["image_u8"] and plain.last_params == hand and plain.last_degrade is None
    assert torch.equal(torch.get_rng_state(), mark_plain)
    torch.manual_seed(36)
    loader = aug.ResidentTrainLoader(rs, 2, [0, 1], 24, degrade=SPEC)
    loader.batch([0, 1])
    assert loader.last_params == hand and loader.last_degrade == rows
    assert torch.equal(torch.get_rng_state(), mark_degrade)


def test_video_set_loader(tmp_path):
    aug = amd("imagenet_codebase.data_providers.augment")
    path = str(tmp_path / "v.y4m")
    write_video(path, 2, 38, 54, seed=9)
    rs = aug.ResidentVideoSet([(path, None, [0, 1])], torch.device(DEV))
    torch.manual_seed(37)
    loader = aug.ResidentTrainLoader(rs, 2, [0, 1], 24, want_f32=True, degrade=SPEC, degrade_seed=7)
    _check_batches(loader, rs.image_np, [[0, 1], [1, 0]], 24)


def test_synthetic_provider_and_evaluation(tmp_path):
    """the stand-in provider trains on degraded batches, and the fixed evaluation degradation is the host statement's"""
    rm = amd("imagenet_codebase.run_manager")
    cfg = rm.Div2K_SetXXRunConfig(degrade=SPEC, degrade_seed=11, resident=True, allow_synthetic=True, image_size=32,
                                  train_batch_size=2, n_train_batches=1, test_batch_size=1, test_sizes=[(32, 40), (24, 24)],
                                  lr_on_device=True, n_epochs=1, init_lr=1e-3, opt_type="adam")
    cfg.dataset_root = str(tmp_path / "absent")
    prov = cfg.data_provider
    batch = next(iter(prov.train))
    assert "degrade" in batch and batch["degrade_seed"] == 11 and len(prov.train.last_degrade) == 2
    assert "degrade" not in prov.build_sub_train_loader(2, 2).batches[0]       # BN re-calibration sees plain crops
    mgr = type("M", (), {"device": torch.device(DEV), "_eval_batch": rm.SRRunManager._eval_batch})()
    at = 0
    for item in prov.test:
        assert sorted(item) == ["image_u8"]
        got = mgr._eval_batch(item, (1.5, 8.0, 21), at)
        hr = item["image_u8"].numpy()
        want = dg.batch_np(hr, dg.degrade_table(dg.fixed_rows(1, 1.5, 8.0, first=at)), 21)
        for k in want:
            assert np.allclose(got[k].cpu().numpy(), want[k], rtol=0, atol=1e-7), k      # no exact `image`: ATen's / 255
            assert np.array_equal(np.rint(got[k].cpu().numpy() * 255), np.rint(want[k] * 255)), k
        at += 1
    with pytest.raises(ValueError, match="lr_on_device"):
        mgr._eval_batch({"image": torch.zeros(1, 3, 8, 8)}, (1.0, 1.0, 0), 0)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_at_the_c_boundary():
    C = amd("_C")
    L = C.lib()
    x = torch.zeros((1, 3, 8, 8), dtype=torch.uint8, device=DEV)
    y = torch.zeros_like(x)
    t = torch.from_numpy(dg.degrade_table([dg.identity_row()])).to(DEV)
    st = _stream()
    blur = lambda src=_p(x), tab=_p(t), n=1, H=8, W=8, r=10, dst=_p(y): L.ofasr_degrade_blur_u8(src, tab, n, H, W, r, dst, st)
    noise = lambda src=_p(x), tab=_p(t), scale=2, n=1, H=8, W=8, out=_p(y), f32=None: \
        L.ofasr_degrade_noise_u8(src, tab, 1, 2, scale, n, H, W, out, f32, st)
    assert blur() == 0 and noise() == 0 and noise(out=_p(x)) == 0
    assert blur(n=0) == 0 and noise(n=0) == 0
    for bad in (blur(src=None), blur(tab=None), blur(dst=None), noise(src=None), noise(tab=None), noise(out=None),
                blur(n=-1), noise(n=-1), blur(H=0), noise(W=0), blur(dst=_p(x))):
        assert bad == -1
    for bad in (blur(r=11), blur(r=-1), noise(scale=3), noise(scale=1), blur(H=1 << 16, W=1 << 16),
                noise(H=1 << 16, W=1 << 16), blur(n=21846), noise(n=21846)):
        assert bad == -2
    assert blur(r=11) == -2 and b"radius 11" in L.ofasr_last_error_string()
    assert noise(scale=3) == -2 and b"scale 3" in L.ofasr_last_error_string()
    torch.cuda.synchronize()
    assert int(y.sum()) == 0


def test_cpu_tensors_are_refused():
    ops, C = amd("ops"), amd("_C")
    x = torch.zeros((1, 3, 8, 8), dtype=torch.uint8)
    t = torch.from_numpy(dg.degrade_table([dg.identity_row()]))
    with pytest.raises(C.OfasrError, match="no CPU fallback"):
        ops.degrade_blur_u8(x, t)
    with pytest.raises(C.OfasrError, match="no CPU fallback"):
        ops.degrade_noise_u8(x, t, 0, 2)
    with pytest.raises(C.OfasrError, match="no CPU fallback"):
        ops.degrade_blur_u8(x.to(DEV), t)
    with pytest.raises(C.OfasrError, match="int32"):
        ops.degrade_blur_u8(x.to(DEV), t.to(DEV).long())
    with pytest.raises(C.OfasrError, match="uint8"):
        ops.degrade_noise_u8(x.to(DEV).float(), t.to(DEV), 0, 2)
    with pytest.raises(C.OfasrError, match="scale 3"):
        ops.degrade_noise_u8(x.to(DEV), t.to(DEV), 0, 3)
