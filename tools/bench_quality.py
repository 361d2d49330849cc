#!/usr/bin/env python3
"""Y-PSNR / Y-SSIM scoring cost (ops.quality_y, csrc/quality.hip): kernel time (tile + finishing kernel, from the library's
per-launch events) and its fraction of the byte floor N*H*W*3*(sizeof(out) + sizeof(target)) at the measured 6.3 TB/s copy
rate, for a 16x3x256x256 batch and one 3x4320x7680 image (fp32 and bf16 output against an fp32 target), beside the wall
time of the host metric it replaces (utils.psnr_y_per_image: the .cpu() round trip + numpy) and of the ATen fp64 device
metric (utils.psnr_y_device, called per image) on the same tensors.  Prints one JSON line.
usage: python tools/bench_quality.py [--reps 10] [--skip-8k]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"
COPY_TBPS = 6.3


def wall(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_ms": 1e3 * ts[len(ts) // 2], "min_ms": 1e3 * ts[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-8k", action="store_true")
    a = ap.parse_args()
    import torch
    C = importlib.import_module(PKG + "._C")
    ops = importlib.import_module(PKG + ".ops")
    utils = importlib.import_module(PKG + ".utils")
    L = C.lib()
    sync = torch.cuda.synchronize
    shapes = [(16, 256, 256)] + ([] if a.skip_8k else [(1, 4320, 7680)])
    out = {"reps": a.reps, "copy_TBps": COPY_TBPS, "runs": []}
    for (N, H, W) in shapes:
        g = torch.Generator(device="cuda").manual_seed(0)
        tgt = torch.rand(N, 3, H, W, device="cuda", generator=g)
        base = (tgt + 0.05 * torch.randn(N, 3, H, W, device="cuda", generator=g))
        for dt in (torch.float32, torch.bfloat16):
            o = base.to(dt)
            floor_bytes = N * H * W * 3 * (o.element_size() + tgt.element_size())
            floor_us = floor_bytes / (COPY_TBPS * 1e12) * 1e6
            ops.quality_y(o, tgt)
            sync()
            L.ofasr_profile_enable(1)
            C.profile_read()
            for _ in range(a.reps):
                ops.quality_y(o, tgt)
            prof = C.profile_read()
            L.ofasr_profile_enable(0)
            tile = sum(v["total_us"] for k, v in prof.items() if "quality_y_tile_kernel" in k) / a.reps
            fin = sum(v["total_us"] for k, v in prof.items() if "quality_y_finish_kernel" in k) / a.reps
            rec = {"shape": [N, 3, H, W], "output": str(dt).replace("torch.", ""), "floor_bytes": floor_bytes,
                   "floor_us": floor_us, "tile_kernel_us": tile, "finish_kernel_us": fin,
                   "fraction_of_floor": floor_us / (tile + fin),
                   "quality_y_wall": wall(lambda: utils.quality_y_device(o, tgt).psnr(), a.reps, sync)}
            of = o.float()
            reps_h = max(1, a.reps // 5) if H * W > 1 << 22 else a.reps
            rec["psnr_y_per_image_wall"] = wall(lambda: utils.psnr_y_per_image(of, tgt), reps_h, sync)
            rec["psnr_y_device_wall"] = wall(
                lambda: [float(utils.psnr_y_device(of[i:i + 1], tgt[i:i + 1])) for i in range(N)], reps_h, sync)
            out["runs"].append(rec)
            del o, of
        del tgt, base
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
