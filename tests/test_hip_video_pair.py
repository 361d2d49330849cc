"""ofasr_aug_gather_yuv420_pair (csrc/augment.hip) and training / evaluation on paired video on the GPU
(augment.ResidentVideoPairSet, data_providers/video_frames.py, VideoFramesRunConfig with videos_lr) against the host
statements (augment.gather_yuv420_pair_np, apply_pair_params_np): equal bytes everywhere."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import amd
from test_video_pair import COMBOS, PAIRS, SIZES, make_pair_pools, pair_cases, pair_rows, write_video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_KEEP = []


def _aug():
    return amd("imagenet_codebase.data_providers.augment")


def _tail(t):
    """a copy of t that ends exactly where its own > 10 MB device allocation ends (the allocator's segment)"""
    nbytes = t.numel() * t.element_size()
    seg = max(12 << 20, (nbytes + (2 << 20) - 1) // (2 << 20) * (2 << 20) + (2 << 20))
    torch.cuda.empty_cache()
    # larger than every free block inside a segment that live tensors of earlier tests still pin: the allocator then has
    # to make a new segment of exactly `seg` bytes, whatever ran before
    free = max([b["size"] for s in torch.cuda.memory_snapshot() for b in s["blocks"] if b["state"] == "inactive"] or [0])
    seg = max(seg, (free + (2 << 20) - 1) // (2 << 20) * (2 << 20) + (2 << 20))
    buf = torch.empty(seg, dtype=torch.uint8, device=DEV)
    out = buf[seg - nbytes:].view(t.dtype).view(t.shape)
    out.copy_(t.to(DEV))
    end = out.data_ptr() + nbytes
    segs = [s for s in torch.cuda.memory_snapshot() if s["address"] <= out.data_ptr() < s["address"] + s["total_size"]]
    assert len(segs) == 1 and segs[0]["address"] + segs[0]["total_size"] == end, "tensor is not at its allocation's end"
    _KEEP.append(buf)
    return out


@pytest.fixture(scope="module")
def pools():
    """per scale the HR and the LR pool, each the tail of an allocation of its own: the last V plane of either ends on
    the last byte of its segment"""
    out = {}
    for f in PAIRS:
        p = make_pair_pools(f)
        p["hr_dev"], p["lr_dev"] = _tail(torch.from_numpy(p["hr_host"])), _tail(torch.from_numpy(p["lr_host"]))
        assert p["hr_dev"].numel() == p["hr_host"].size and p["lr_dev"].numel() == p["lr_host"].size
        out[f] = p
    yield out
    _KEEP.clear()


@pytest.fixture(scope="module")
def runs(pools):
    """one launch per (S, f) and matrix over all cases, with the fp32 outputs; shared by the tests below.  Every table
    is made by make_pair_table, which refuses what the kernel would have to clamp."""
    aug, ops = _aug(), amd("ops")
    res = {}
    for S, f in SIZES:
        cs = pair_cases(S, f, 200 + S + f)
        table = aug.make_pair_table(pair_rows(pools[f], f, cs), S, f)
        for (matrix, full) in COMBOS:
            out = ops.aug_gather_yuv420_pair(pools[f]["hr_dev"], pools[f]["lr_dev"], table.to(DEV), len(cs), S, f, matrix,
                                             full, want_f32=True)
            torch.cuda.synchronize()
            res[S, f, matrix] = dict(zip(("hr", "hr32", "lr", "lr32"), out), cases=cs, table=table)
    return res


@pytest.mark.parametrize("matrix,full", COMBOS)
@pytest.mark.parametrize("S,f", SIZES)
def test_pair_kernel_equals_host(pools, runs, S, f, matrix, full):
    aug, video = _aug(), amd("video")
    r, p, s = runs[S, f, matrix], pools[f], S // f
    hr, lr = r["hr"].cpu().numpy(), r["lr"].cpu().numpy()
    n = len(r["cases"])
    assert hr.shape == (n, 3, S, S) and lr.shape == (n, 3, s, s) and hr.dtype == lr.dtype == np.uint8
    ref_h, ref_l = aug.gather_yuv420_pair_np(p["hr_host"], p["lr_host"], r["table"].numpy(), S, f,
                                             video.yuv_coeffs(matrix, full)[0])
    assert np.array_equal(hr, ref_h) and np.array_equal(lr, ref_l)
    # the per-case PIL statement: the three transforms of the decode of each side's own whole frame
    hr_rgb = [video.yuv420_to_rgb_host(*fr, matrix=matrix, full_range=full) for fr in p["hr"]]
    lr_rgb = [video.yuv420_to_rgb_host(*fr, matrix=matrix, full_range=full) for fr in p["lr"]]
    for m, (k, prm) in enumerate(r["cases"]):
        i, j, flip, angle = prm
        assert np.array_equal(hr[m], aug.apply_params_np(hr_rgb[k], S, (f * i, f * j, flip, angle)).transpose(2, 0, 1)), \
            "HR S=%d f=%d pair %d params %r" % (S, f, k, prm)
        assert np.array_equal(lr[m], aug.apply_params_np(lr_rgb[k], s, prm).transpose(2, 0, 1)), \
            "LR S=%d f=%d pair %d params %r" % (S, f, k, prm)
    for m in range(0, n, 41):
        k, prm = r["cases"][m]
        a, b = aug.apply_pair_params_np(p["hr"][k], p["lr"][k], S, f, prm, matrix=matrix, full_range=full)
        assert np.array_equal(hr[m], a.transpose(2, 0, 1)) and np.array_equal(lr[m], b.transpose(2, 0, 1))


@pytest.mark.parametrize("S,f", SIZES)
def test_fp32_outputs_variants_and_the_sibling(pools, runs, S, f):
    ops = amd("ops")
    r, p = runs[S, f, "bt601"], pools[f]
    n, table = len(r["cases"]), r["table"].to(DEV)
    for u8, f32 in ((r["hr"], r["hr32"]), (r["lr"], r["lr32"])):
        assert f32.dtype == torch.float32 and f32.shape == u8.shape
        assert torch.equal(f32.cpu(), u8.cpu().float().div_(255.0))       # the reference division runs on the host
    hr_b, lr_b = ops.aug_gather_yuv420_pair(p["hr_dev"], p["lr_dev"], table, n, S, f)           # uint8 only: the other variant
    again = ops.aug_gather_yuv420_pair(p["hr_dev"], p["lr_dev"], table, n, S, f, want_f32=True)
    assert torch.equal(hr_b, r["hr"]) and torch.equal(lr_b, r["lr"])
    for got, key in zip(again, ("hr", "hr32", "lr", "lr32")):
        assert got.cpu().numpy().tobytes() == r[key].cpu().numpy().tobytes(), key
    # each side is the sibling kernel on its own pool and table block
    assert torch.equal(ops.aug_gather_yuv420(p["hr_dev"], table[0].contiguous(), n, S), r["hr"])
    assert torch.equal(ops.aug_gather_yuv420(p["lr_dev"], table[1].contiguous(), n, S // f), r["lr"])
    assert not torch.equal(runs[S, f, "bt709"]["hr"], r["hr"]) and not torch.equal(runs[S, f, "bt709"]["lr"], r["lr"])
    # a table with more rows than samples: block 1 is still read at its own place
    few = ops.aug_gather_yuv420_pair(p["hr_dev"], p["lr_dev"], table, 3, S, f)
    assert torch.equal(few[0], r["hr"][:3]) and torch.equal(few[1], r["lr"][:3])


def test_ops_refuses_bad_operands(pools):
    ops, C = amd("ops"), amd("_C")
    p = pools[4]
    table = torch.zeros((2, 1, 12), dtype=torch.int64, device=DEV)
    table[0, 0, 1:3] = 64
    table[1, 0, 1:3] = 16
    ops.aug_gather_yuv420_pair(p["hr_dev"], p["lr_dev"], table, 1, 32, 4)
    for bad in (dict(table=table[0]), dict(table=table.int()), dict(n=2), dict(table=table.cpu()),
                dict(lr_pool=p["lr_dev"].view(-1, 2)), dict(hr_pool=p["hr_dev"].view(torch.int8)), dict(lr_pool=p["lr_host"]),
                dict(f=3), dict(S=30), dict(S=4100, f=4)):
        kw = dict(dict(hr_pool=p["hr_dev"], lr_pool=p["lr_dev"], table=table, n=1, S=32, f=4), **bad)
        if not torch.is_tensor(kw["lr_pool"]):
            kw["lr_pool"] = torch.from_numpy(kw["lr_pool"])
        with pytest.raises(C.OfasrError):
            ops.aug_gather_yuv420_pair(**kw)


def test_abi_error_codes_without_a_launch(pools):
    """the documented codes of include/ofasr.h; none of these calls launches anything"""
    C, ops = amd("_C"), amd("ops")
    L = C.lib()
    INVALID, UNSUPPORTED = -1, -2
    p = pools[4]
    hp, lp = p["hr_dev"], p["lr_dev"]
    table = torch.zeros((2, 1, 12), dtype=torch.int64, device=DEV)
    S, f = 32, 4
    hr = torch.empty((1, 3, S, S), dtype=torch.uint8, device=DEV)
    lr = torch.empty((1, 3, S // f, S // f), dtype=torch.uint8, device=DEV)
    hr32, lr32 = hr.float(), lr.float()
    coeffs = ops.yuv_table("bt601", False, False)
    good = dict(hr_pool=hp.data_ptr(), hr_bytes=hp.numel(), lr_pool=lp.data_ptr(), lr_bytes=lp.numel(), table=table.data_ptr(),
                n=1, S=S, f=f, coeffs=coeffs, hr_u8=hr.data_ptr(), hr_f32=None, lr_u8=lr.data_ptr(), lr_f32=None)
    order = ("hr_pool", "hr_bytes", "lr_pool", "lr_bytes", "table", "n", "S", "f", "coeffs", "hr_u8", "hr_f32", "lr_u8", "lr_f32")

    def call(**kw):
        a = dict(good, **kw)
        return L.ofasr_aug_gather_yuv420_pair(*([a[k] for k in order] + [None]))

    C.reset_launch_counts()
    for k in ("hr_pool", "lr_pool", "table", "coeffs", "hr_u8", "lr_u8"):
        assert call(**{k: None}) == INVALID, k
    assert call(hr_f32=hr32.data_ptr()) == INVALID and call(lr_f32=lr32.data_ptr()) == INVALID
    assert call(n=0) == INVALID and call(S=0) == INVALID and call(hr_bytes=0) == INVALID and call(lr_bytes=0) == INVALID
    assert call(S=30) == INVALID                                   # S % f != 0
    for bad_f in (3, 1, 0, 8, -2):
        assert call(f=bad_f) == UNSUPPORTED, bad_f
    assert call(S=4100) == UNSUPPORTED and call(n=65536) == UNSUPPORTED
    assert call(hr_bytes=32 * 32 * 3 // 2 - 1) == UNSUPPORTED      # no 32 x 32 frame fits
    assert call(lr_bytes=8 * 8 * 3 // 2 - 1) == UNSUPPORTED        # no 8 x 8 frame fits
    assert call(S=28, lr_bytes=8 * 8 * 3 // 2 - 1) == UNSUPPORTED  # s = 7: an even-sided frame of at least 8 x 8
    assert b"LR pool" in L.ofasr_last_error_string()
    assert C.launch_count("aug_gather_yuv420_pair") == 0
    assert call(hr_bytes=32 * 32 * 3 // 2, lr_bytes=8 * 8 * 3 // 2, hr_f32=hr32.data_ptr(), lr_f32=lr32.data_ptr()) == 0
    torch.cuda.synchronize()
    assert C.launch_count("aug_gather_yuv420_pair") == 1


# ----------------------------------------------------------------------------------------------- end to end
CLIPS = {4: ((64, 64), (16, 16)), 2: ((64, 96), (32, 48))}


@pytest.fixture()
def clips(tmp_path):
    """per scale a 6-frame HR Y4M and its LR Y4M"""
    out = {}
    for f, ((H, W), (h, w)) in CLIPS.items():
        hr, lr = str(tmp_path / ("hr%d.y4m" % f)), str(tmp_path / ("lr%d.y4m" % f))
        out[f] = {"hr": hr, "lr": lr, "hr_frames": write_video(hr, 6, H, W, seed=20 + f),
                  "lr_frames": write_video(lr, 6, h, w, seed=30 + f)}
    return out


@pytest.mark.parametrize("f", [4, 2])
def test_pair_provider_end_to_end(clips, f):
    Image = pytest.importorskip("PIL.Image")
    aug, video, utils = _aug(), amd("video"), amd("utils")
    vf = amd("imagenet_codebase.data_providers.video_frames")
    dp = amd("imagenet_codebase.data_providers.div2k_setxx")
    torch.cuda.set_device(0)
    c = clips[f]
    (H, W), (h, w) = CLIPS[f]
    S, s, other = 32, 32 // f, 6 - f
    kw = dict(videos=[c["hr"]], videos_lr=[c["lr"]], valid_every=3, matrix="bt709", full_range=True, test_batch_size=1,
              image_size=S, train_batch_size=2)
    prov = vf.VideoFramesDataProvider(**kw)
    rs, loader = prov.resident_set, prov.train
    assert isinstance(rs, aug.ResidentVideoPairSet) and rs.scale == f and len(rs) == 6 and len(loader) == 2
    assert prov.train_indices == [1, 2, 4, 5] and prov.eval_indices == [0, 3]
    assert rs.entries[2] == (2 * H * W * 3 // 2, H, W) and rs.lr_entries[2] == (2 * h * w * 3 // 2, h, w)
    assert rs.nbytes == 6 * (H * W + h * w) * 3 // 2
    assert np.array_equal(rs.pool.cpu().numpy(), np.concatenate([p.reshape(-1) for fr in c["hr_frames"] for p in fr]))
    assert np.array_equal(rs.lr_pool.cpu().numpy(), np.concatenate([p.reshape(-1) for fr in c["lr_frames"] for p in fr]))
    assert np.array_equal(rs.lr_image_np(4), video.yuv420_to_rgb_host(*c["lr_frames"][4], matrix="bt709", full_range=True))
    assert np.array_equal(rs.image_np(4), video.yuv420_to_rgb_host(*c["hr_frames"][4], matrix="bt709", full_range=True))

    torch.manual_seed(5)
    seen = []
    for batch in loader:
        idx, params = loader.last_indices, loader.last_params
        seen += idx
        assert set(batch) == {"image_u8", "image", "lr_u8", "lr", "lr_scale"} and batch["lr_scale"] == f
        pairs = [aug.apply_pair_params_np(c["hr_frames"][k], c["lr_frames"][k], S, f, p, matrix="bt709", full_range=True)
                 for k, p in zip(idx, params)]
        hr, lr = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
        assert all(0 <= p[0] <= h - s and 0 <= p[1] <= w - s for p in params)                    # drawn on the LR grid
        assert np.array_equal(batch["image_u8"].cpu().numpy(), hr.transpose(0, 3, 1, 2))
        assert np.array_equal(batch["lr_u8"].cpu().numpy(), lr.transpose(0, 3, 1, 2))
        assert tuple(batch["lr"].shape) == (2, 3, s, s) and batch["lr"].dtype == torch.float32
        dev = utils.device_batch(batch, torch.device(DEV))
        assert set(dev) == {"image", "2x_down_image", "4x_down_image"}
        assert dev["image"] is batch["image"] and dev["%dx_down_image" % f] is batch["lr"]       # the decoded LR stream
        assert torch.equal(batch["lr"].cpu(), torch.from_numpy(lr.transpose(0, 3, 1, 2).copy()).float().div_(255.0))
        for n in range(len(idx)):                  # the other scale stays Pillow's bicubic of the HR crop
            H_img = Image.fromarray(hr[n])
            assert torch.equal(dev["image"][n].cpu(), dp.to_tensor(H_img))
            assert torch.equal(dev["%dx_down_image" % other][n].cpu(), dp.to_tensor(dp.get_transform_L(other)(H_img)))
    assert sorted(seen) == prov.train_indices

    # the same draws as the unpaired path on the LR frame with crop s: the RNG ends where that path leaves it
    torch.manual_seed(9)
    want = [aug.draw_train_params(h, w, s) for _ in range(2)]
    state = torch.get_rng_state()
    torch.manual_seed(9)
    loader.batch([1, 4])
    assert loader.last_params == want and torch.equal(torch.get_rng_state(), state)
    # rotate=False: the same corner and flip, angle 0, the same RNG use; the LR crop then covers the HR crop exactly
    flat = vf.VideoFramesDataProvider(**dict(kw, rotate=False))
    torch.manual_seed(9)
    b = flat.train.batch([1, 4])
    assert flat.train.last_params == [p[:3] + (0.0,) for p in want] and torch.equal(torch.get_rng_state(), state)
    for n, (k, p) in enumerate(zip([1, 4], flat.train.last_params)):
        a, l = aug.apply_pair_params_np(c["hr_frames"][k], c["lr_frames"][k], S, f, p, matrix="bt709", full_range=True)
        assert np.array_equal(b["image_u8"][n].cpu().numpy(), a.transpose(2, 0, 1))
        assert np.array_equal(b["lr_u8"][n].cpu().numpy(), l.transpose(2, 0, 1))

    # evaluation: whole frames, ModCrop(4), the decoded LR frame beside them
    items = list(prov.test)
    assert len(items) == 2
    for it, k in zip(items, prov.eval_indices):
        assert set(it) == {"image_u8", "lr_u8", "lr_scale"} and it["lr_scale"] == f
        assert tuple(it["image_u8"].shape) == (1, 3, H, W) and tuple(it["lr_u8"].shape) == (1, 3, H // f, W // f)
        assert np.array_equal(it["image_u8"][0].cpu().numpy(), rs.image_np(k).transpose(2, 0, 1))
        assert np.array_equal(it["lr_u8"][0].cpu().numpy(), rs.lr_image_np(k).transpose(2, 0, 1))
    dev = utils.device_batch(items[1], torch.device(DEV))
    assert set(dev) == {"image", "2x_down_image", "4x_down_image"}
    assert torch.equal(dev["%dx_down_image" % f].cpu(), items[1]["lr_u8"].cpu().float().div_(255.0))
    assert tuple(dev["%dx_down_image" % other].shape) == (1, 3, H // other, W // other)
    plain = utils.device_batch({"image_u8": items[1]["image_u8"]}, torch.device(DEV))
    assert torch.equal(dev["%dx_down_image" % other], plain["%dx_down_image" % other]) and torch.equal(dev["image"], plain["image"])
    assert not torch.equal(dev["%dx_down_image" % f], plain["%dx_down_image" % f])

    # BN re-calibration batches carry the paired LR too
    sub = prov.build_sub_train_loader(3, 2)
    assert [set(b) for b in sub] == [{"image_u8", "lr_u8", "lr_scale"}] * 2 and [b["lr_u8"].shape[0] for b in sub] == [2, 1]
    assert all(b["lr_u8"].is_cuda and b["lr_u8"].shape[1:] == (3, s, s) and b["image_u8"].shape[1:] == (3, S, S) for b in sub)

    with pytest.raises(MemoryError, match="bytes"):
        vf.VideoFramesDataProvider(**dict(kw, resident_max_bytes=6 * (H * W + h * w) * 3 // 2 - 1))
    with pytest.raises(ValueError, match="multiple of its scale"):
        aug.ResidentTrainLoader(rs, 2, [0, 1], 30 if f == 4 else 31)
    with pytest.raises(ValueError, match="matched by position"):
        vf.VideoFramesDataProvider(**dict(kw, videos_lr=[c["lr"], c["lr"]]))
    with pytest.raises(ValueError, match="exactly 2 or 4 times"):
        vf.VideoFramesDataProvider(**dict(kw, videos_lr=[c["hr"]]))
    with pytest.raises(ValueError, match="paired video"):
        vf.VideoFramesDataProvider(**dict(kw, videos_lr=None, rotate=False))


def test_validate_and_checkpoint_on_a_pair(clips, tmp_path):
    rm, nets = amd("imagenet_codebase.run_manager"), amd("elastic_nn.networks")
    eutils = amd("elastic_nn.utils")
    amd("elastic_nn.modules.dynamic_op").DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    torch.cuda.set_device(0)
    c = clips[2]
    args = argparse.Namespace(kd_ratio=0, teacher_model=None)
    nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = False          # the intended indexing, for a 2x network (pd = [1])
    try:
        torch.manual_seed(7)
        net = nets.OFAMobileNetS4(ks_list=[5], expand_ratio_list=[3], depth_list=[2], pixelshuffle_depth_list=[1])
        cfg = rm.VideoFramesRunConfig([c["hr"]], videos_lr=[c["lr"]], video_valid_every=0, n_epochs=1, init_lr=1e-3,
                                      opt_type="adam", no_decay_keys="bn#bias", label_smoothing=0.0, train_batch_size=2,
                                      test_batch_size=1, image_size=32)
        assert cfg.dataset == "video_frames: %s (lr: %s)" % (c["hr"], c["lr"])
        net.set_active_subnet(ks=5, e=3, d=2, pixel_d=1)
        mgr = rm.SRRunManager(str(tmp_path / "run"), net, cfg, init=True, num_gpus=1, args=args)
        assert len(cfg.test_loader) == 1                           # valid_every = 0: the first frame evaluates
        # what the network is fed at the pair's scale is the decoded LR frame
        fed = []
        hook = mgr.net.register_forward_pre_hook(lambda m, inp: fed.append(inp[0].detach().clone()))
        loss, psnr = mgr.validate(is_test=True, input_key="2x_down_image")
        hook.remove()
        assert np.isfinite(loss) and np.isfinite(psnr)
        lr0 = cfg.data_provider.resident_set.lr_image_np(0).transpose(2, 0, 1)[None]
        assert len(fed) == 1 and torch.equal(fed[0].float().cpu(), torch.from_numpy(lr0.copy()).float().div_(255.0))
        sub = cfg.data_provider.build_sub_train_loader(2, 2)
        assert "lr_u8" in sub[0]
        eutils.recalibrate_bn(mgr.net, sub, input_key="2x_down_image")
        mgr.save_model()
        ck = torch.load(os.path.join(str(tmp_path / "run"), "checkpoint", "checkpoint.pth.tar"), map_location="cpu",
                        weights_only=True)
        assert ck["dataset"] == cfg.dataset and c["hr"] in ck["dataset"] and c["lr"] in ck["dataset"]
    finally:
        nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = True
