"""ofasr_aug_gather_u8 (csrc/augment.hip) and the resident training loader on the GPU, against the host statement of the
transforms (data_providers/augment.py, itself pinned to PIL by tests/test_augment.py): equal bytes everywhere."""
import numpy as np
import pytest
import torch

from conftest import amd

Image = pytest.importorskip("PIL.Image")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(37, 53), (64, 64), (40, 96)]        # (H, W) of the three pooled images
FIXED_ANGLES = [0.0, 90.0, -90.0, 180.0, 45.0, -33.3, 1e-9]
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
    """three images of different sizes packed back to back; the last one ends on the last byte of the pool, and the
    pool on the last byte of its own allocation"""
    rng = np.random.RandomState(5)
    imgs = [rng.randint(1, 256, (h, w, 3)).astype(np.uint8) for (h, w) in SHAPES]
    offs = np.cumsum([0] + [a.size for a in imgs])
    host = np.concatenate([a.reshape(-1) for a in imgs])
    dev = _tail(torch.from_numpy(host))
    assert dev.is_contiguous() and dev.numel() == offs[-1]
    yield {"imgs": imgs, "offs": [int(o) for o in offs[:-1]], "host": host, "dev": dev}
    _KEEP.clear()


def _cases(S, seed):
    """(image, (i, j, flip, angle)): four corners and an interior crop of every image, flip on and off, every angle"""
    g = torch.Generator().manual_seed(seed)
    angles = FIXED_ANGLES + [float(torch.empty(1).uniform_(-90, 90, generator=g).item()) for _ in range(10)]
    out = []
    for k, (h, w) in enumerate(SHAPES):
        corners = [(0, 0), (0, w - S), (h - S, 0), (h - S, w - S), ((h - S) // 2, (w - S) // 3)]
        for (i, j) in corners:
            for flip in (False, True):
                for a in angles:
                    out.append((k, (i, j, flip, a)))
    return out


def _gather_np(pool, table, S):
    """the kernel restated on the pool's bytes, clamping rules included (csrc/augment.hip header)"""
    nb = pool.size
    y, x = np.mgrid[0:S, 0:S].astype(np.int64)
    out = np.zeros((len(table), 3, S, S), np.uint8)
    for n, row in enumerate(np.asarray(table, dtype=np.int64)):
        off, H, W, i, j, flip, a0, a1, a2, a3, a4, a5 = (int(v) for v in row)
        H, W = min(max(H, S), 1 << 24), min(max(W, S), 1 << 24)
        i, j = min(max(i, 0), H - S), min(max(j, 0), W - S)
        off = min(max(off, 0), nb)
        xin, yin = (a2 + y * a1 + x * a0) >> 16, (a5 + y * a4 + x * a3) >> 16
        ok = (xin >= 0) & (xin < S) & (yin >= 0) & (yin < S)
        xc, yc = np.clip(xin, 0, S - 1), np.clip(yin, 0, S - 1)
        col = S - 1 - xc if flip else xc
        b = np.minimum(off + ((i + yc) * W + j + col) * 3, nb - 3)
        for c in range(3):
            out[n, c] = np.where(ok, pool[b + c], 0)
    return out


@pytest.fixture(scope="module")
def runs(pool):
    """one launch per S over all cases, with the fp32 output; shared by the tests below"""
    aug, ops = _aug(), amd("ops")
    res = {}
    for S in (8, 30, 32):
        cases = _cases(S, 100 + S)
        table = aug.make_table([(pool["offs"][k],) + SHAPES[k] + (p,) for k, p in cases], S)
        u8, f32 = ops.aug_gather_u8(pool["dev"], table.to(DEV), len(cases), S, want_f32=True)
        torch.cuda.synchronize()
        res[S] = {"cases": cases, "table": table, "u8": u8, "f32": f32}
    return res


@pytest.mark.parametrize("S", [8, 30, 32])
def test_kernel_equals_host_transforms(pool, runs, S):
    aug = _aug()
    r = runs[S]
    got = r["u8"].cpu().numpy()
    assert got.shape == (len(r["cases"]), 3, S, S)
    for n, (k, p) in enumerate(r["cases"]):
        ref = aug.apply_params_np(pool["imgs"][k], S, p).transpose(2, 0, 1)
        assert np.array_equal(got[n], ref), "S=%d image %d params %r: %d bytes differ" % (S, k, p, int((got[n] != ref).sum()))
    # the byte-level restatement used by the clamping test says the same on a valid table
    assert np.array_equal(_gather_np(pool["host"], r["table"].numpy(), S), got)


@pytest.mark.parametrize("S", [8, 30, 32])
def test_fp32_output_and_determinism(pool, runs, S):
    ops = amd("ops")
    r = runs[S]
    assert r["f32"].dtype == torch.float32
    # the reference division runs on the host (ToTensor's, correctly rounded): ATen's GPU division by a scalar multiplies
    # by the rounded reciprocal instead, up to 1 ulp away (tests/test_hip_resample.py same_u8)
    assert torch.equal(r["f32"].cpu(), r["u8"].cpu().float().div_(255.0))
    again = ops.aug_gather_u8(pool["dev"], r["table"].to(DEV), len(r["cases"]), S)       # uint8 only: the other variant
    u8b, f32b = ops.aug_gather_u8(pool["dev"], r["table"].to(DEV), len(r["cases"]), S, want_f32=True)
    assert torch.equal(again, r["u8"]) and torch.equal(u8b, r["u8"])
    assert f32b.cpu().numpy().tobytes() == r["f32"].cpu().numpy().tobytes()


@pytest.mark.parametrize("S", [30, 32])
def test_out_of_range_table_entries_are_clamped(pool, S):
    """values only: i, j and offset out of range give what the clamped table gives, and the call returns OFASR_OK"""
    aug, ops = _aug(), amd("ops")
    nb = pool["host"].size
    o2 = pool["offs"][2]
    rows = []
    for (i, j, off) in ((-5, 10 ** 6, o2), (10 ** 9, -1, o2), (3, 4, -17), (0, 0, nb + 99), (2, 60, nb - 1000),
                        (7, 3, o2 + 8), (-2 ** 40, 2 ** 40, 2 ** 50)):
        for flip, angle in ((0, 0.0), (1, 45.0), (0, -90.0), (1, 17.25)):
            rows.append((off, 40, 96, i, j, flip) + tuple(aug.rotate_coeffs(angle, S)))
    table = torch.tensor(rows, dtype=torch.int64)
    got = ops.aug_gather_u8(pool["dev"], table.to(DEV), len(rows), S)      # raises unless the status is OFASR_OK
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), _gather_np(pool["host"], table.numpy(), S))


# ----------------------------------------------------------------------------------------------- end to end
def _write_dataset(root):
    rng = np.random.RandomState(11)
    (root / "train").mkdir()
    (root / "val").mkdir()
    for k, (h, w) in enumerate([(16, 16), (23, 31), (40, 17), (33, 48), (19, 64)]):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(str(root / "train" / ("t%d.png" % k)))
    for k, (h, w) in enumerate([(21, 18), (16, 30)]):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(str(root / "val" / ("v%d.png" % k)))


def test_resident_provider_end_to_end(tmp_path):
    aug = _aug()
    dp = amd("imagenet_codebase.data_providers.div2k_setxx")
    utils = amd("utils")
    _write_dataset(tmp_path)
    kw = dict(save_path=str(tmp_path), train_batch_size=2, test_batch_size=1, n_worker=0, image_size=16)
    torch.cuda.set_device(0)
    host = dp.Div2K_SetXXDataProvider(**kw)
    prov = dp.Div2K_SetXXDataProvider(resident=True, **kw)
    loader = prov.train
    assert isinstance(loader, aug.ResidentTrainLoader) and loader.batch_size == 2
    assert len(loader) == len(host.train) == 2                     # 5 images, drop_last
    paths = prov.resident_set.paths
    assert paths == host.train.dataset.paths
    files = [np.asarray(Image.open(p).convert("RGB")) for p in paths]
    for k, a in enumerate(files):                                  # the pool holds the decoded files
        assert np.array_equal(prov.resident_set.image_np(k), a)
    assert prov.resident_set.pool.numel() == sum(a.size for a in files)

    torch.manual_seed(3)
    seen = []
    for batch in loader:
        idx, params = loader.last_indices, loader.last_params
        seen += idx
        assert set(batch) == {"image_u8", "image"} and batch["image_u8"].is_cuda and batch["image_u8"].dtype == torch.uint8
        hr = np.stack([aug.apply_params_np(files[k], 16, p) for k, p in zip(idx, params)])       # [N, 16, 16, 3]
        assert np.array_equal(batch["image_u8"].cpu().numpy(), hr.transpose(0, 3, 1, 2))
        dev = utils.device_batch(batch, torch.device(DEV))
        assert dev["image"] is batch["image"]
        for n in range(len(idx)):                                  # the dataset's host PIL path on the same HR image
            H_img = Image.fromarray(hr[n])
            want = {"image": dp.to_tensor(H_img), "2x_down_image": dp.to_tensor(dp.get_transform_L(2)(H_img)),
                    "4x_down_image": dp.to_tensor(dp.get_transform_L(4)(H_img))}
            for key, t in want.items():
                assert torch.equal(dev[key][n].cpu(), t), key
    assert len(seen) == 4 and len(set(seen)) == 4 and set(seen) <= set(range(5))

    # without the fp32 output the batch carries the uint8 image alone and device_batch forms 'image' itself
    plain = aug.ResidentTrainLoader(prov.resident_set, 2, [1, 3], 16)
    (b,) = list(plain)
    assert set(b) == {"image_u8"}
    assert torch.equal(utils.device_batch(b, torch.device(DEV))["image"], b["image_u8"].float().div_(255.0))

    sub = prov.build_sub_train_loader(3, 2)
    assert [set(b) for b in sub] == [{"image_u8"}] * 2 and [b["image_u8"].shape[0] for b in sub] == [2, 1]
    assert all(b["image_u8"].is_cuda and b["image_u8"].shape[1:] == (3, 16, 16) for b in sub)
    assert prov.build_sub_train_loader(3, 2) is sub                # cached, as on the DataLoader path
    assert [b["image"].shape[0] for b in host.build_sub_train_loader(3, 2)] == [2, 1]

    # valid / test are the DataLoader path, untouched
    assert isinstance(prov.test, torch.utils.data.DataLoader) and prov.valid is prov.test

    with pytest.raises(MemoryError, match="bytes"):
        aug.ResidentTrainSet(paths, DEV, max_bytes=1000)
    with pytest.raises(ValueError, match="larger than input image size"):
        aug.ResidentTrainLoader(prov.resident_set, 2, [0, 1], 17)


def test_resident_loader_under_sharding(tmp_path):
    aug = _aug()
    dp = amd("imagenet_codebase.data_providers.div2k_setxx")
    _write_dataset(tmp_path)
    torch.cuda.set_device(0)
    prov = dp.Div2K_SetXXDataProvider(save_path=str(tmp_path), train_batch_size=1, test_batch_size=1, n_worker=0,
                                      image_size=16, num_replicas=2, rank=0, resident=True)
    loader = prov.train
    assert isinstance(loader.sampler, dp.RankShardSampler) and len(loader) == 3

    def epoch(e):
        loader.sampler.set_epoch(e)
        order = []
        for _ in loader:
            order += loader.last_indices
        return order

    ref = dp.RankShardSampler(list(range(5)), 2, 0)
    orders = []
    for e in (0, 1, 0):
        ref.set_epoch(e)
        orders.append(epoch(e))
        assert orders[-1] == list(ref)
    assert orders[0] == orders[2] and orders[0] != orders[1]
