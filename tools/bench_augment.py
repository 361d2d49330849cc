#!/usr/bin/env python3
"""Training input path on resident images (ops.aug_gather_u8, csrc/augment.hip, data_providers/augment.py):
 * kernel time at N=16, S=256 with and without the fp32 output (library per-launch events) against the byte floor --
   bytes written plus source bytes touched (one 3-byte pixel per output pixel) at the measured 6.3 TB/s copy rate;
 * loader throughput in img/s over >= 200 batches after a warm-up: the resident loader (augmented batch + the LR images
   of utils.device_batch, GPU time included) and the DataLoader path of the same provider with n_worker=16 (batch on the
   device, LR images included), both on a directory of synthetic PNGs the tool writes itself (32 files of 2040x1356
   under 256 names).
 * the YUV leg (--yuv-frames F, default 64: a 199 MB pool against 398 MB of RGB; --only-yuv runs nothing else): ops.aug_gather_yuv420 at N=16, S=256 on F
   resident 1920x1080 YUV 4:2:0 frames against ops.aug_gather_u8 on the same crops from an RGB pool of the same frames
   made with ops.yuv420_to_rgb_u8 (equal bytes out, checked): both kernel times and their ratio.  The fused gather
   issues 9 byte loads per pixel against 3.
 * the pair leg (--only-pair runs nothing else; --yuv-frames F frame pairs): ops.aug_gather_yuv420_pair at N=16, S=256,
   f=4 on F resident 1920x1080 frames and their 480x270 LR frames against the two separate ops.aug_gather_yuv420
   launches that produce the same bytes (checked), on the same crops: the one launch's time, the two launches' times
   and their sum.
 * the best-of-K leg (--crop-candidates 1,4,8; --only-candidates runs nothing else): the resident loader's img/s per K
   (--repeats measurements each) on the PNG pool and on --yuv-frames 1920x1080 4:2:0 frames, and per K > 1 the GPU time
   of ofasr_aug_select's two launches per batch; K = 1 is the loader without candidates.
 * the degrade leg (--degrade; runs nothing else): the resident loader's img/s on the PNG pool without the option and
   with ResidentTrainLoader(degrade=...) (blur 0.2:3.3 anisotropic, noise 1:25, every sample degraded; --repeats
   measurements each, interleaved; the batch counts when its HR + LR images are on the device), and the GPU time per
   batch of the blur launch and of the two noise launches.
Prints one JSON line.
usage: python tools/bench_augment.py [--files 32] [--entries 256] [--height 1356] [--width 2040] [--batches 200]
                                     [--warmup 10] [--host-batches 200] [--workers 16] [--skip-host]
                                     [--yuv-frames 64] [--only-yuv] [--only-pair]
                                     [--crop-candidates 1,4,8] [--repeats 3] [--only-candidates] [--degrade]"""
import argparse
import importlib
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"
COPY_TBPS = 6.3


def write_pngs(root, files, entries, h, w):
    """`files` distinct PNGs and links to them up to `entries` names, so that an epoch is long enough to keep every
    DataLoader worker busy (a worker makes a whole batch) without writing hundreds of large files"""
    import numpy as np
    from PIL import Image
    os.makedirs(os.path.join(root, "train"))
    os.makedirs(os.path.join(root, "val"))
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:h, 0:w]
    # a smooth colour field with mild noise: compresses like a photograph rather than like white noise
    base = np.stack([127 + 120 * np.sin(yy / 37.0 + c) * np.cos(xx / 53.0 - c) for c in range(3)], -1)
    for k in range(files):
        a = np.clip(np.roll(base, 61 * k, axis=1) + rng.randint(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(root, "train", "img%04d.png" % k), compress_level=3)
    for k in range(files, entries):
        os.symlink("img%04d.png" % (k % files), os.path.join(root, "train", "img%04d.png" % k))
    Image.fromarray(np.zeros((64, 64, 3), np.uint8)).save(os.path.join(root, "val", "v.png"))


def loader_rate(loader, batches, warmup, step, sync):
    """img/s over `batches` batches after `warmup`, cycling through epochs; `step` consumes a batch on the GPU"""
    done, images, t0 = 0, 0, None
    while done < warmup + batches:
        for b in loader:
            n = step(b)
            done += 1
            if done == warmup:
                sync()
                t0 = time.perf_counter()
            elif done > warmup:
                images += n
            if done >= warmup + batches:
                break
    sync()
    return images / (time.perf_counter() - t0)


def kernel_us(C, L, fn, tables, name):
    """mean time of the launches of kernel `name` over fn(table) for every table (library per-launch events)"""
    import torch
    fn(tables[0])
    torch.cuda.synchronize()
    L.ofasr_profile_enable(1)
    C.profile_read()
    for t in tables:
        fn(t)
    prof = C.profile_read()
    L.ofasr_profile_enable(0)
    return sum(v["total_us"] for k, v in prof.items() if name in k) / len(tables)


def yuv_leg(C, L, ops, aug, dev, N, S, frames, reps, H=1080, W=1920):
    """the fused gather on resident YUV 4:2:0 frames against aug_gather_u8 on the decoded frames, same crops"""
    import numpy as np
    import torch
    rng = np.random.RandomState(1)
    yy, xx = np.mgrid[0:H, 0:W]
    fb = H * W * 3 // 2
    pool = torch.empty(frames * fb, dtype=torch.uint8, device=dev)
    rgb_pool = torch.empty(frames * H * W * 3, dtype=torch.uint8, device=dev)
    ybase = 126 + 100 * np.sin(yy / 41.0) * np.cos(xx / 59.0)
    cbase = [128 + 90 * np.sin(yy[::2, ::2] / (67.0 + 9 * j)) * np.cos(xx[::2, ::2] / 83.0) for j in range(2)]
    for k in range(frames):      # smooth luma and chroma fields, shifted per frame, with mild noise, in the legal ranges
        y = np.clip(np.roll(ybase, 61 * k, axis=1) + rng.randint(-5, 6, (H, W)), 16, 235)
        c = [np.clip(np.roll(cb, 29 * k, axis=1) + rng.randint(-3, 4, (H // 2, W // 2)), 16, 240) for cb in cbase]
        host = np.concatenate([p.astype(np.uint8).reshape(-1) for p in (y, c[0], c[1])])
        pool[k * fb:(k + 1) * fb].copy_(torch.from_numpy(host))
        f = pool[k * fb:(k + 1) * fb]
        planes = (f[:H * W].view(H, W), f[H * W:H * W * 5 // 4].view(H // 2, W // 2), f[H * W * 5 // 4:].view(H // 2, W // 2))
        rgb_pool[k * H * W * 3:(k + 1) * H * W * 3].copy_(ops.yuv420_to_rgb_u8(*planes).reshape(-1))
    torch.manual_seed(0)
    ty, tr = [], []
    for r in range(reps):
        idx = torch.randint(0, frames, (N,)).tolist()
        params = [aug.draw_train_params(H, W, S) for _ in idx]
        ty.append(aug.make_table([(k * fb, H, W, p) for k, p in zip(idx, params)], S, yuv420=True).to(dev))
        tr.append(aug.make_table([(k * H * W * 3, H, W, p) for k, p in zip(idx, params)], S).to(dev))
    res = {"frames": frames, "frame_hw": [H, W], "yuv_pool_bytes": pool.numel(), "rgb_pool_bytes": rgb_pool.numel(),
           "launches": reps}
    for want_f32 in (False, True):
        a = ops.aug_gather_yuv420(pool, ty[0], N, S, want_f32=want_f32)
        b = ops.aug_gather_u8(rgb_pool, tr[0], N, S, want_f32=want_f32)
        same = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) if want_f32 else torch.equal(a, b)
        if not same:
            raise SystemExit("aug_gather_yuv420 and aug_gather_u8 of the decoded frames differ")
        us_y = kernel_us(C, L, lambda t: ops.aug_gather_yuv420(pool, t, N, S, want_f32=want_f32), ty,
                         "aug_gather_yuv420_kernel")
        us_r = kernel_us(C, L, lambda t: ops.aug_gather_u8(rgb_pool, t, N, S, want_f32=want_f32), tr, "aug_gather_u8_kernel")
        res["f32" if want_f32 else "u8"] = {"yuv420_kernel_us": us_y, "rgb_kernel_us": us_r, "ratio": us_y / us_r}
    return res


def synthetic_yuv_pool(dev, frames, H, W, seed):
    """`frames` H x W 4:2:0 frames back to back on `dev`: smooth luma and chroma fields, shifted per frame, with mild
    noise, in the legal ranges"""
    import numpy as np
    import torch
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    fb = H * W * 3 // 2
    pool = torch.empty(frames * fb, dtype=torch.uint8, device=dev)
    ybase = 126 + 100 * np.sin(yy * (26.3 / H)) * np.cos(xx * (32.5 / W))
    cbase = [128 + 90 * np.sin(yy[::2, ::2] * ((16.1 - 2 * j) / H)) * np.cos(xx[::2, ::2] * (23.1 / W)) for j in range(2)]
    for k in range(frames):
        y = np.clip(np.roll(ybase, (61 * k) % W, axis=1) + rng.randint(-5, 6, (H, W)), 16, 235)
        c = [np.clip(np.roll(cb, (29 * k) % (W // 2), axis=1) + rng.randint(-3, 4, (H // 2, W // 2)), 16, 240) for cb in cbase]
        host = np.concatenate([p.astype(np.uint8).reshape(-1) for p in (y, c[0], c[1])])
        pool[k * fb:(k + 1) * fb].copy_(torch.from_numpy(host))
    return pool, fb


def pair_leg(C, L, ops, aug, dev, N, S, frames, reps, f=4, h=270, w=480):
    """one ofasr_aug_gather_yuv420_pair launch against the two ofasr_aug_gather_yuv420 launches that write the same two
    batches, on the same crops"""
    import torch
    H, W, s = f * h, f * w, S // f
    hr_pool, hfb = synthetic_yuv_pool(dev, frames, H, W, 1)
    lr_pool, lfb = synthetic_yuv_pool(dev, frames, h, w, 2)
    torch.manual_seed(0)
    tables = []
    for r in range(reps):
        idx = torch.randint(0, frames, (N,)).tolist()
        rows = [(k * hfb, H, W, k * lfb, h, w, aug.draw_pair_params(h, w, S, f)) for k in idx]
        t = aug.make_pair_table(rows, S, f).to(dev)
        tables.append((t, t[0].contiguous(), t[1].contiguous()))
    res = {"frames": frames, "hr_hw": [H, W], "lr_hw": [h, w], "f": f, "hr_pool_bytes": hr_pool.numel(),
           "lr_pool_bytes": lr_pool.numel(), "launches": reps}
    for want_f32 in (False, True):
        t = tables[0]
        pair = ops.aug_gather_yuv420_pair(hr_pool, lr_pool, t[0], N, S, f, want_f32=want_f32)
        a = ops.aug_gather_yuv420(hr_pool, t[1], N, S, want_f32=want_f32)
        b = ops.aug_gather_yuv420(lr_pool, t[2], N, s, want_f32=want_f32)
        two = (a + b) if want_f32 else (a, b)
        if len(pair) != len(two) or not all(torch.equal(x, y) for x, y in zip(pair, two)):
            raise SystemExit("aug_gather_yuv420_pair and the two aug_gather_yuv420 launches differ")
        us_p = kernel_us(C, L, lambda t: ops.aug_gather_yuv420_pair(hr_pool, lr_pool, t[0], N, S, f, want_f32=want_f32),
                         tables, "aug_gather_yuv420_pair_kernel")
        us_h = kernel_us(C, L, lambda t: ops.aug_gather_yuv420(hr_pool, t[1], N, S, want_f32=want_f32), tables,
                         "aug_gather_yuv420_kernel")
        us_l = kernel_us(C, L, lambda t: ops.aug_gather_yuv420(lr_pool, t[2], N, s, want_f32=want_f32), tables,
                         "aug_gather_yuv420_kernel")
        res["f32" if want_f32 else "u8"] = {"pair_kernel_us": us_p, "hr_kernel_us": us_h, "lr_kernel_us": us_l,
                                            "two_launches_us": us_h + us_l, "ratio": us_p / (us_h + us_l)}
    return res


class _FramePool(object):
    """what ResidentTrainLoader needs of a ResidentVideoSet, over a pool that is on the device already"""
    yuv420 = True

    def __init__(self, pool, fb, frames, H, W):
        self.pool, self.device = pool, pool.device
        self.entries = [(k * fb, H, W) for k in range(frames)]
        self.paths = ["frame#%d" % k for k in range(frames)]

    def __len__(self):
        return len(self.entries)

    def gather(self, table, n, S, want_f32=False):
        ops = importlib.import_module(PKG + ".ops")
        return ops.aug_gather_yuv420(self.pool, table, n, S, want_f32=want_f32)


def candidates_leg(C, L, aug, utils, dev, N, S, Ks, sets, batches, warmup, repeats, reps):
    """best of K candidate crops (--crop-candidates K1,K2,...): per pool and K the resident loader's img/s (`repeats`
    measurements each; the batch counts when its HR + LR images are on the device, as resident_img_per_s) and, for K > 1,
    the GPU time of the two launches of ofasr_aug_select per batch.  K = 1 is the loader without candidates."""
    import torch
    sync = torch.cuda.synchronize

    def step(b):
        return utils.device_batch(b, dev)["image"].size(0)

    res = {}
    for name, ds in sets:
        r = {"images": len(ds), "pool_bytes": int(ds.pool.numel())}
        sampler = torch.utils.data.RandomSampler(range(len(ds)))
        for K in Ks:
            loader = aug.ResidentTrainLoader(ds, N, sampler, S, want_f32=True, **({} if K == 1 else dict(candidates=K)))
            entry = {"img_per_s": [loader_rate(loader, batches, warmup, step, sync) for _ in range(repeats)]}
            if K > 1:
                idx = [torch.randint(0, len(ds), (N,)).tolist() for _ in range(reps)]
                run = lambda ix: loader.batch(ix)
                entry["activity_kernel_us"] = kernel_us(C, L, run, idx, "aug_select_activity_kernel")
                entry["choose_kernel_us"] = kernel_us(C, L, run, idx, "aug_select_choose_kernel")
                chosen, first, count = loader.selection_stats()
                entry["activity_chosen_over_first"] = chosen / max(first, 1)
            r["K=%d" % K] = entry
        res[name] = r
    return res


DEGRADE_SPEC = {"blur": (0.2, 3.3), "aniso": True, "noise": (1.0, 25.0), "gray_prob": 0.4, "prob": 1.0}


def degrade_leg(C, L, aug, utils, dev, N, S, ds, batches, warmup, repeats, reps):
    """blurred, noisy LR inputs (--degrade): the resident loader's img/s with the option off and on, measured in turns, and
    the GPU time of the option's three launches per batch"""
    import torch
    sync = torch.cuda.synchronize

    def step(b):
        return utils.device_batch(b, dev)["image"].size(0)

    sampler = torch.utils.data.RandomSampler(range(len(ds)))
    off = aug.ResidentTrainLoader(ds, N, sampler, S, want_f32=True)
    on = aug.ResidentTrainLoader(ds, N, sampler, S, want_f32=True, degrade=DEGRADE_SPEC, degrade_seed=1)
    res = {"images": len(ds), "spec": DEGRADE_SPEC, "off_img_per_s": [], "on_img_per_s": []}
    for _ in range(repeats):
        res["off_img_per_s"].append(loader_rate(off, batches, warmup, step, sync))
        res["on_img_per_s"].append(loader_rate(on, batches, warmup, step, sync))
    idx = [torch.randint(0, len(ds), (N,)).tolist() for _ in range(reps)]
    run = lambda ix: step(on.batch(ix))
    res["blur_kernel_us"] = kernel_us(C, L, run, idx, "degrade_blur_kernel")
    res["noise_kernels_us"] = kernel_us(C, L, run, idx, "degrade_noise_kernel")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--entries", type=int, default=256, help="names in train/ (links to the files beyond --files)")
    ap.add_argument("--height", type=int, default=1356)
    ap.add_argument("--width", type=int, default=2040)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--host-batches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--yuv-frames", type=int, default=64, help="1920x1080 frames of the YUV leg (0: skip it)")
    ap.add_argument("--only-yuv", action="store_true", help="run the YUV leg alone")
    ap.add_argument("--only-pair", action="store_true", help="run the pair leg alone (--yuv-frames frame pairs)")
    ap.add_argument("--crop-candidates", default=None, metavar="K1,K2,...",
                    help="the best-of-K leg: the resident loader's img/s per K on the PNG pool and on --yuv-frames "
                         "1920x1080 4:2:0 frames (1 = the loader without candidates)")
    ap.add_argument("--repeats", type=int, default=3, help="measurements per K of the best-of-K leg")
    ap.add_argument("--only-candidates", action="store_true", help="run the best-of-K leg alone")
    ap.add_argument("--degrade", action="store_true", help="run the degrade leg alone: the resident loader with and "
                                                           "without blurred, noisy LR inputs")
    a = ap.parse_args()
    import torch
    C = importlib.import_module(PKG + "._C")
    ops = importlib.import_module(PKG + ".ops")
    utils = importlib.import_module(PKG + ".utils")
    aug = importlib.import_module(PKG + ".imagenet_codebase.data_providers.augment")
    dp = importlib.import_module(PKG + ".imagenet_codebase.data_providers.div2k_setxx")
    L = C.lib()
    sync = torch.cuda.synchronize
    dev = torch.device("cuda", 0)
    N, S = 16, 256
    out = {"N": N, "S": S, "copy_TBps": COPY_TBPS, "files": a.files, "entries": max(a.entries, a.files),
           "file_hw": [a.height, a.width]}
    if a.only_pair:
        out["yuv420_pair"] = pair_leg(C, L, ops, aug, dev, N, S, max(a.yuv_frames, 1), a.reps)
        print(json.dumps(out), flush=True)
        return
    if a.only_candidates and not a.crop_candidates:
        raise SystemExit("--only-candidates needs --crop-candidates K1,K2,...")
    if a.yuv_frames > 0 and not a.only_candidates and not a.degrade:
        out["yuv420"] = yuv_leg(C, L, ops, aug, dev, N, S, a.yuv_frames, a.reps)
    if a.only_yuv:
        print(json.dumps(out), flush=True)
        return
    root = tempfile.mkdtemp(prefix="bench_augment_")
    try:
        t0 = time.perf_counter()
        write_pngs(root, a.files, max(a.entries, a.files), a.height, a.width)
        out["write_pngs_s"] = time.perf_counter() - t0
        kw = dict(save_path=root, train_batch_size=N, test_batch_size=1, image_size=S)
        t0 = time.perf_counter()
        prov = dp.Div2K_SetXXDataProvider(n_worker=0, resident=True, **kw)
        sync()
        out["resident_decode_upload_s"] = time.perf_counter() - t0
        out["resident_bytes"] = prov.resident_set.nbytes
        loader = prov.train
        if a.degrade:
            out["degrade"] = degrade_leg(C, L, aug, utils, dev, N, S, prov.resident_set, a.batches, a.warmup, a.repeats,
                                         a.reps)
            print(json.dumps(out), flush=True)
            return
        if a.crop_candidates:
            frames = max(a.yuv_frames, 1)
            ypool, fb = synthetic_yuv_pool(dev, frames, 1080, 1920, 1)
            sets = [("rgb", prov.resident_set), ("yuv420_1080p", _FramePool(ypool, fb, frames, 1080, 1920))]
            out["crop_candidates"] = candidates_leg(C, L, aug, utils, dev, N, S, [int(k) for k in a.crop_candidates.split(",")],
                                                    sets, a.batches, a.warmup, a.repeats, a.reps)
            del ypool, sets
            if a.only_candidates:
                print(json.dumps(out), flush=True)
                return

        # ---- the kernel: library per-launch events over `reps` launches with freshly drawn tables
        torch.manual_seed(0)
        ds = prov.resident_set
        tables = []
        for r in range(a.reps):
            idx = torch.randint(0, len(ds), (N,)).tolist()
            rows = [ds.entries[k] + (aug.draw_train_params(ds.entries[k][1], ds.entries[k][2], S),) for k in idx]
            tables.append(aug.make_table(rows, S).to(dev))
        for want_f32 in (False, True):
            ops.aug_gather_u8(ds.pool, tables[0], N, S, want_f32=want_f32)
            sync()
            L.ofasr_profile_enable(1)
            C.profile_read()
            for t in tables:
                ops.aug_gather_u8(ds.pool, t, N, S, want_f32=want_f32)
            prof = C.profile_read()
            L.ofasr_profile_enable(0)
            us = sum(v["total_us"] for k, v in prof.items() if "aug_gather_u8_kernel" in k) / a.reps
            floor_bytes = N * 3 * S * S * (2 + (4 if want_f32 else 0))
            floor_us = floor_bytes / (COPY_TBPS * 1e12) * 1e6
            out["kernel_f32" if want_f32 else "kernel_u8"] = {
                "kernel_us": us, "floor_bytes": floor_bytes, "floor_us": floor_us, "fraction_of_floor": floor_us / us,
                "launches": a.reps}

        # ---- the loaders: a batch counts when its HR + LR images are on the device
        def step(b):
            d = utils.device_batch(b, dev)
            return d["image"].size(0)

        out["resident_img_per_s"] = loader_rate(loader, a.batches, a.warmup, step, sync)
        plain = aug.ResidentTrainLoader(ds, N, loader.sampler, S, want_f32=False)
        out["resident_u8_only_img_per_s"] = loader_rate(plain, a.batches, a.warmup, lambda b: b["image_u8"].size(0), sync)
        if not a.skip_host:
            for name, lr_on_device in (("dataloader_img_per_s", False), ("dataloader_lr_on_device_img_per_s", True)):
                host = dp.Div2K_SetXXDataProvider(n_worker=a.workers, lr_on_device=lr_on_device, **kw)
                out[name] = loader_rate(host.train, a.host_batches, min(a.warmup, 2), step, sync)
                del host
            out["dataloader_workers"] = a.workers
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
