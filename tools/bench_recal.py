#!/usr/bin/env python3
"""BatchNorm re-calibration of one search candidate: set_running_statistics (deep copy, ATen batch_norm, vendor / per-op
fp32 path) against recalibrate_bn (csrc/mbrecal_f32.hip + the fp32 conv kernels) on --calib-images LR images of 64x64
in batches of 16, wall time per candidate after one warm-up; the S1 / S2 / S3 passes of ofasr_mbconv_recal_f32 per
(mid, K) at N=16, 64x64 from the library's per-launch events; and the latency table's prediction error on --subnets
random S4 sub-networks against the measured static nets.  Prints one JSON line.
usage: python tools/bench_recal.py [--calib-images 256] [--reps 10] [--subnets 10]"""
import argparse
import copy
import importlib
import json
import os
import random
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calib-images", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--subnets", type=int, default=10)
    ap.add_argument("--lat-size", type=int, default=64)
    a = ap.parse_args()
    import torch
    C = importlib.import_module(PKG + "._C")
    ops = importlib.import_module(PKG + ".ops")
    nets = importlib.import_module(PKG + ".elastic_nn.networks")
    eutils = importlib.import_module(PKG + ".elastic_nn.utils")
    search = importlib.import_module(PKG + ".elastic_nn.search")
    dop = importlib.import_module(PKG + ".elastic_nn.modules.dynamic_op")
    dop.DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    dev = "cuda:0"
    L = C.lib()
    res = {}
    torch.manual_seed(0)
    net = nets.OFAMobileNetS4(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4],
                              pixelshuffle_depth_list=[1, 2]).to(dev).eval()
    net.init_model("he_fout")
    net.set_active_subnet(ks=7, e=6, d=4, pixel_d=2)      # the c3-shaped candidate (the largest of the space)
    g = torch.Generator().manual_seed(1)
    loader = [{"image": torch.rand((a.batch, 3, 64, 64), generator=g).to(dev)}
              for _ in range(a.calib_images // a.batch)]

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    res["candidate"] = "S4 ks7 e6 d4 pd2, %d images of 64x64 LR" % a.calib_images
    res["set_running_statistics_s"] = wall(lambda: eutils.set_running_statistics(net, loader))
    res["recalibrate_bn_s"] = wall(lambda: eutils.recalibrate_bn(net, loader))
    res["speedup"] = res["set_running_statistics_s"] / res["recalibrate_bn_s"]

    # pass times per (mid, K) at N = 16, 64 x 64
    st = importlib.import_module(PKG + ".imagenet_codebase.networks.sr_static")
    blk = importlib.import_module(PKG + ".imagenet_codebase.networks.proxyless_nets")
    x = torch.randn(16, 64, 64, 64, device=dev)
    passes = {}
    for mid in (192, 256, 384):
        for K in (3, 5, 7):
            mb = blk.MobileInvertedResidualBlock.build_from_config(
                st.mb_block_config(64, 64, K, mid // 64, mid)).mobile_inverted_conv.to(dev).train()
            cfg, ps = mb.composite_args(64, True)
            acc = tuple(torch.zeros((2, c), dtype=torch.float64, device=dev) for c in (mid, mid, 64))
            with torch.no_grad():
                ops.mbconv_recal_f32(x, cfg, *ps, acc=acc)
                torch.cuda.synchronize()
                L.ofasr_profile_enable(1)
                C.profile_read()
                for _ in range(a.reps):
                    ops.mbconv_recal_f32(x, cfg, *ps, acc=acc)
                torch.cuda.synchronize()
                prof = C.profile_read()
                L.ofasr_profile_enable(0)
            row = {"other_us": 0.0}
            for name, v in prof.items():
                m = re.search(r"mb_recal_f32_kernel<(\d), (\d)>", name)
                us = v["total_us"] / a.reps
                if m:
                    row["S%s_us" % m.group(2)] = us
                else:
                    row["other_us"] += us
            row["total_us"] = sum(v for k, v in row.items() if k.endswith("_us") and k != "total_us")
            passes["mid%d_k%d" % (mid, K)] = row
    res["passes_N16_64x64"] = passes

    # latency table against measured static nets
    space = search.ArchSpace(net, 4)
    table = search.LatencyTable(space, 1, a.lat_size, a.lat_size).build(reps=a.reps)
    rng = random.Random(3)
    errs = []
    for _ in range(a.subnets):
        arch = space.random_sample(rng)
        pred = table.predict(arch)
        space.apply(net, arch)
        meas = search.measure(net.get_active_subnet().eval(), 1, a.lat_size, a.lat_size, reps=a.reps)
        errs.append({"predicted_ms": pred, "measured_ms": meas, "rel_err": pred / meas - 1.0})
    res["latency_table"] = errs
    res["latency_table_mean_abs_rel_err"] = sum(abs(e["rel_err"]) for e in errs) / len(errs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
