"""ofasr_aug_gather_yuv420 (csrc/augment.hip) and training on raw YUV 4:2:0 video on the GPU (augment.ResidentVideoSet,
data_providers/video_frames.py, VideoFramesRunConfig) against the host statements (augment.gather_yuv420_np,
apply_params_yuv420_np, video.yuv420_to_rgb_host): equal bytes everywhere."""
import argparse

import numpy as np
import pytest
import torch

from conftest import amd
from test_video_train import COMBOS, SHAPES, _write_video, cases, make_frames

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
def pool():
    """three frames of different sizes back to back; the last V plane ends on the last byte of the pool, and the pool on
    the last byte of its own allocation"""
    frames, offs, host = make_frames()
    dev = _tail(torch.from_numpy(host))
    assert dev.is_contiguous() and dev.numel() == host.size == offs[-1] + SHAPES[-1][0] * SHAPES[-1][1] * 3 // 2
    yield {"frames": frames, "offs": offs, "host": host, "dev": dev}
    _KEEP.clear()


@pytest.fixture(scope="module")
def runs(pool):
    """one launch per S (and matrix / range) over all cases, with the fp32 output; shared by the tests below"""
    aug, ops = _aug(), amd("ops")
    res = {}
    for S in (8, 30, 32):
        cs = cases(S, 100 + S)
        table = aug.make_table([(pool["offs"][k],) + SHAPES[k] + (p,) for k, p in cs], S, yuv420=True)
        for (matrix, full) in COMBOS:
            u8, f32 = ops.aug_gather_yuv420(pool["dev"], table.to(DEV), len(cs), S, matrix, full, want_f32=True)
            torch.cuda.synchronize()
            res[S, matrix] = {"cases": cs, "table": table, "u8": u8, "f32": f32}
    return res


@pytest.mark.parametrize("matrix,full", COMBOS)
@pytest.mark.parametrize("S", [8, 30, 32])
def test_kernel_equals_host(pool, runs, S, matrix, full):
    aug, video = _aug(), amd("video")
    r = runs[S, matrix]
    got = r["u8"].cpu().numpy()
    assert got.shape == (len(r["cases"]), 3, S, S)
    rgb = [video.yuv420_to_rgb_host(*f, matrix=matrix, full_range=full) for f in pool["frames"]]
    for n, (k, p) in enumerate(r["cases"]):
        ref = aug.apply_params_np(rgb[k], S, p).transpose(2, 0, 1)     # apply_params_yuv420_np with the decode shared
        assert np.array_equal(got[n], ref), "S=%d frame %d params %r: %d bytes differ" % (S, k, p, int((got[n] != ref).sum()))
    for n in range(0, len(r["cases"]), 37):
        k, p = r["cases"][n]
        ref = aug.apply_params_yuv420_np(*pool["frames"][k], size=S, params=p, matrix=matrix, full_range=full)
        assert np.array_equal(got[n], ref.transpose(2, 0, 1))
    assert np.array_equal(aug.gather_yuv420_np(pool["host"], r["table"].numpy(), S, video.yuv_coeffs(matrix, full)[0]), got)


@pytest.mark.parametrize("S", [8, 30, 32])
def test_fp32_output_and_determinism(pool, runs, S):
    ops = amd("ops")
    r = runs[S, "bt601"]
    assert r["f32"].dtype == torch.float32
    # the reference division runs on the host (ToTensor's, correctly rounded)
    assert torch.equal(r["f32"].cpu(), r["u8"].cpu().float().div_(255.0))
    n = len(r["cases"])
    again = ops.aug_gather_yuv420(pool["dev"], r["table"].to(DEV), n, S)                  # uint8 only: the other variant
    u8b, f32b = ops.aug_gather_yuv420(pool["dev"], r["table"].to(DEV), n, S, want_f32=True)
    assert torch.equal(again, r["u8"]) and torch.equal(u8b, r["u8"])
    assert f32b.cpu().numpy().tobytes() == r["f32"].cpu().numpy().tobytes()
    assert not torch.equal(runs[S, "bt709"]["u8"], r["u8"])                               # the table is used


@pytest.mark.parametrize("S", [30, 32])
def test_out_of_range_table_entries_are_clamped(pool, S):
    """values only: whatever the table holds, the call returns OFASR_OK and gives what the clamping rules of the file
    header give (Se = S rounded up to even: H = clamp(H, Se, 2^24) & ~1, W alike; (i, j) into [0, H - S] x [0, W - S];
    offset into [0, pool bytes]; every sample's byte address into [0, pool bytes - 1])"""
    aug, ops, video = _aug(), amd("ops"), amd("video")
    nb = pool["host"].size
    o2 = pool["offs"][2]
    rows = []
    for (off, H, W, i, j) in ((o2, 40, 96, -5, 10 ** 6), (o2, 40, 96, 10 ** 9, -1), (-17, 40, 96, 3, 4),
                              (nb + 99, 40, 96, 0, 0), (nb - 1000, 40, 96, 2, 60), (o2 + 8, 40, 96, 7, 3),
                              (2 ** 50, 40, 96, -2 ** 40, 2 ** 40), (o2, 39, 95, 5, 7), (o2, 41, 97, 11, 65),
                              (0, 2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40), (0, -2 ** 40, -2 ** 40, 1, 1), (o2, 0, 1, 0, 0),
                              (0, 2 ** 24 + 1, 64, 2 ** 24, 3), (pool["offs"][1], 64, 2 ** 30, 9, 2 ** 29), (5, 31, 33, 1, 3)):
        for flip, angle in ((0, 0.0), (1, 45.0), (0, -90.0), (1, 17.25)):
            rows.append((off, H, W, i, j, flip) + tuple(aug.rotate_coeffs(angle, S)))
    rows.append((o2, 40, 96, 3, 5, 0, 2 ** 40 + 65536, -2 ** 40, 2 ** 33 + 32768, 2 ** 32, 65536 - 2 ** 32, 32768))
    rows.append((o2, 40, 96, 3, 5, 1, -2 ** 31, 2 ** 31 - 1, 12345678, 2 ** 31 + 7, -99999, -2 ** 31))
    table = torch.tensor(rows, dtype=torch.int64)
    got = ops.aug_gather_yuv420(pool["dev"], table.to(DEV), len(rows), S, "bt709", True)   # raises unless OFASR_OK
    torch.cuda.synchronize()
    ref = aug.gather_yuv420_np(pool["host"], table.numpy(), S, video.yuv_coeffs("bt709", True)[0])
    assert np.array_equal(got.cpu().numpy(), ref)


def test_entry_refuses_bad_arguments(pool):
    ops, C = amd("ops"), amd("_C")
    table = torch.zeros((1, 12), dtype=torch.int64, device=DEV)
    small = torch.zeros(32 * 32 * 3 // 2 - 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(C.OfasrError):
        ops.aug_gather_yuv420(small, table, 1, 31)            # S' = 32: the pool holds no 32 x 32 frame
    with pytest.raises(C.OfasrError):
        ops.aug_gather_yuv420(pool["dev"], table, 1, 4097)
    with pytest.raises(C.OfasrError):
        ops.aug_gather_yuv420(pool["dev"], table, 2, 8)       # fewer rows than samples
    with pytest.raises(C.OfasrError):
        ops.aug_gather_yuv420(pool["dev"].view(-1, 2), table, 1, 8)


# ----------------------------------------------------------------------------------------------- end to end
@pytest.fixture()
def clips(tmp_path):
    """a 7-frame 54 x 38 Y4M and a headerless copy of its frames"""
    frames = _write_video(tmp_path / "clip.y4m")
    video = amd("video")
    with video.RawYUV420Writer(str(tmp_path / "clip.yuv"), 54, 38) as w:
        for f in frames:
            w.write_frame(*f)
    return {"y4m": str(tmp_path / "clip.y4m"), "raw": str(tmp_path / "clip.yuv"), "frames": frames}


def test_video_provider_end_to_end(clips):
    Image = pytest.importorskip("PIL.Image")
    aug, video, utils = _aug(), amd("video"), amd("utils")
    vf = amd("imagenet_codebase.data_providers.video_frames")
    dp = amd("imagenet_codebase.data_providers.div2k_setxx")
    torch.cuda.set_device(0)
    frames = clips["frames"]
    kw = dict(videos=[clips["y4m"], clips["raw"]], video_size=(54, 38), valid_every=3, matrix="bt709", full_range=True,
              test_batch_size=1, image_size=16)
    prov = vf.VideoFramesDataProvider(train_batch_size=2, **kw)
    rs, loader = prov.resident_set, prov.train
    assert isinstance(loader, aug.ResidentTrainLoader) and loader.batch_size == 2 and len(loader) == 4
    assert prov.data_shape == (3, 16, 16) and prov.valid is prov.test and prov.name() == "video_frames"
    assert prov.train_indices == [1, 2, 4, 5, 8, 9, 11, 12] and prov.eval_indices == [0, 3, 6, 7, 10, 13]
    # the pool holds the files' frame bytes, as they are in the files
    file_bytes = np.concatenate([p.reshape(-1) for f in frames for p in f])
    assert np.array_equal(rs.pool.cpu().numpy(), np.concatenate([file_bytes, file_bytes]))
    assert rs.entries[8] == (8 * 38 * 54 * 3 // 2, 38, 54) and len(rs) == 14
    for k in (0, 6, 7, 13):
        assert all(np.array_equal(a, b) for a, b in zip(rs.frame_planes_np(k), frames[k % 7]))
    rgb = [video.yuv420_to_rgb_host(*f, matrix="bt709", full_range=True) for f in frames]
    assert np.array_equal(rs.image_np(9), rgb[2])

    torch.manual_seed(3)
    seen = []
    for batch in loader:
        idx, params = loader.last_indices, loader.last_params
        seen += idx
        assert set(batch) == {"image_u8", "image"} and batch["image_u8"].is_cuda and batch["image_u8"].dtype == torch.uint8
        hr = np.stack([aug.apply_params_yuv420_np(*frames[k % 7], size=16, params=p, matrix="bt709", full_range=True)
                       for k, p in zip(idx, params)])                                               # [N, 16, 16, 3]
        assert np.array_equal(batch["image_u8"].cpu().numpy(), hr.transpose(0, 3, 1, 2))
        dev = utils.device_batch(batch, torch.device(DEV))
        assert dev["image"] is batch["image"]
        for n in range(len(idx)):                                  # the image provider's host PIL path on the same HR crop
            H_img = Image.fromarray(hr[n])
            want = {"image": dp.to_tensor(H_img), "2x_down_image": dp.to_tensor(dp.get_transform_L(2)(H_img)),
                    "4x_down_image": dp.to_tensor(dp.get_transform_L(4)(H_img))}
            for key, t in want.items():
                assert torch.equal(dev[key][n].cpu(), t), key
    assert sorted(seen) == prov.train_indices

    # evaluation: whole frames, ModCrop(4), batch 1, file order; device_batch makes the three keys
    items = list(prov.test)
    assert len(items) == len(prov.test) == 6
    for it, k in zip(items, prov.eval_indices):
        assert set(it) == {"image_u8"} and it["image_u8"].is_cuda and tuple(it["image_u8"].shape) == (1, 3, 36, 52)
        assert np.array_equal(it["image_u8"][0].cpu().numpy(), rgb[k % 7][:36, :52].transpose(2, 0, 1))
    dev = utils.device_batch(items[1], torch.device(DEV))
    assert set(dev) == {"image", "2x_down_image", "4x_down_image"} and tuple(dev["4x_down_image"].shape) == (1, 3, 9, 13)
    assert torch.equal(dev["image"], items[1]["image_u8"].float().div_(255.0))

    sub = prov.build_sub_train_loader(3, 2)
    assert [set(b) for b in sub] == [{"image_u8"}] * 2 and [b["image_u8"].shape[0] for b in sub] == [2, 1]
    assert all(b["image_u8"].is_cuda and b["image_u8"].shape[1:] == (3, 16, 16) for b in sub)
    assert prov.build_sub_train_loader(3, 2) is sub                # cached

    # valid_every = 0: every frame trains, the first of each video evaluates
    p0 = vf.VideoFramesDataProvider(train_batch_size=2, **dict(kw, valid_every=0, frames=(2, 6)))
    assert p0.train_indices == list(range(8)) and p0.eval_indices == [0, 4]
    assert np.array_equal(p0.resident_set.frame_planes_np(5)[0], frames[3][0])
    with pytest.raises(ValueError, match="no training frame"):
        vf.VideoFramesDataProvider(train_batch_size=2, **dict(kw, valid_every=1))

    with pytest.raises(MemoryError, match="bytes"):
        vf.VideoFramesDataProvider(train_batch_size=2, resident_max_bytes=14 * 38 * 54 * 3 // 2 - 1, **kw)
    with pytest.raises(ValueError, match="larger than input image size"):
        aug.ResidentTrainLoader(rs, 2, [0, 1], 40)
    with pytest.raises(ValueError, match="needs its frame size"):
        vf.VideoFramesDataProvider(videos=[clips["raw"]], train_batch_size=2, image_size=16)


def test_video_provider_under_sharding(clips):
    vf = amd("imagenet_codebase.data_providers.video_frames")
    dp = amd("imagenet_codebase.data_providers.div2k_setxx")
    torch.cuda.set_device(0)
    prov = vf.VideoFramesDataProvider([clips["y4m"]], valid_every=3, train_batch_size=1, image_size=16, num_replicas=2,
                                      rank=1)
    loader = prov.train
    assert isinstance(loader.sampler, dp.RankShardSampler) and len(loader) == 2
    assert len(list(prov.test)) == 3                               # every rank evaluates the whole set
    ref = dp.RankShardSampler([1, 2, 4, 5], 2, 1)
    orders = []
    for e in (0, 1, 2, 0):
        ref.set_epoch(e)
        loader.sampler.set_epoch(e)
        order = []
        for _ in loader:
            order += loader.last_indices
        orders.append(order)
        assert order == list(ref)
    assert orders[0] == orders[3] and len({tuple(o) for o in orders}) > 1


def test_training_smoke_on_video(clips, tmp_path):
    rm, nets = amd("imagenet_codebase.run_manager"), amd("elastic_nn.networks")
    amd("elastic_nn.modules.dynamic_op").DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    torch.cuda.set_device(0)
    args = argparse.Namespace(kd_ratio=0, teacher_model=None)

    def run(seed, path):
        torch.manual_seed(seed)
        net = nets.OFAMobileNetS4(ks_list=[5], expand_ratio_list=[3], depth_list=[2], pixelshuffle_depth_list=[1])
        cfg = rm.VideoFramesRunConfig([clips["y4m"]], video_valid_every=3, n_epochs=1, init_lr=1e-3, opt_type="adam",
                                      no_decay_keys="bn#bias", label_smoothing=0.0, train_batch_size=2, test_batch_size=1,
                                      image_size=32)
        assert cfg.dataset == "video_frames: " + clips["y4m"]
        net.set_active_subnet(ks=5, e=3, d=2, pixel_d=1)
        mgr = rm.SRRunManager(str(path), net, cfg, init=True, num_gpus=1, args=args)
        assert isinstance(cfg.data_provider, amd("imagenet_codebase.data_providers.video_frames").VideoFramesDataProvider)
        assert len(cfg.train_loader) == 2                          # 4 training frames, batch 2: two steps
        torch.manual_seed(seed + 1)
        batches = [(b["image_u8"].clone(), b["image"].clone()) for b in cfg.train_loader]
        torch.manual_seed(seed + 1)
        train = mgr.train_one_epoch(args, 0)
        valid = mgr.validate(is_test=False)
        return batches, train, valid

    nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = False          # the intended indexing, for a 2x network (pd = [1])
    try:
        b1, t1, v1 = run(7, tmp_path / "a")
        b2, t2, v2 = run(7, tmp_path / "b")
    finally:
        nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = True
    assert all(np.isfinite(x) for x in t1 + v1 + t2 + v2)
    assert len(b1) == len(b2) == 2
    for (u1, f1), (u2, f2) in zip(b1, b2):
        assert tuple(u1.shape) == (2, 3, 32, 32) and torch.equal(u1, u2) and torch.equal(f1, f2)
