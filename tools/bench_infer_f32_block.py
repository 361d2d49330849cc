#!/usr/bin/env python3
"""fp32 eval-mode MB block (+ shortcut): the one-kernel fp32 block (ofasr_mbconv_infer_f32, csrc/mbfused_f32.hip) against
the composite fp32 eval path (ofasr_mbconv_fwd: the un-fused kernels with the BN apply passes between them), per (mid, K)
at N=16, 64x64.  Device time per block from the library's per-launch events (include/ofasr.h Diagnostics; the composite
path is several launches per block), the HBM bytes each path moves by construction, and the matrix FLOP/s of the useful
1x1 work.  usage: python tools/bench_infer_f32_block.py [--reps 30] [--mids 192,384] [--ks 3,7]"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--N", type=int, default=16)
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--mids", default="192,384")
    ap.add_argument("--ks", default="3,7")
    a = ap.parse_args()
    import torch
    ops = importlib.import_module(PKG + ".ops")
    C = importlib.import_module(PKG + "._C")
    st = importlib.import_module(PKG + ".imagenet_codebase.networks.sr_static")
    blk = importlib.import_module(PKG + ".imagenet_codebase.networks.proxyless_nets")
    dev = "cuda:0"
    N, S = a.N, a.S
    px = N * S * S
    x = torch.randn(N, 64, S, S, device=dev)
    print("%-10s %10s %10s %8s %10s %10s %9s" % ("mid,K", "fused us", "comp. us", "speedup", "fused MB", "comp. MB",
                                                  "fused TF"))
    for mid in (int(v) for v in a.mids.split(",")):
        for K in (int(v) for v in a.ks.split(",")):
            block = blk.MobileInvertedResidualBlock.build_from_config(st.mb_block_config(64, 64, K, mid // 64, mid))
            mb = block.mobile_inverted_conv.to(dev).eval()
            cfg, ps = mb.composite_args(64, True)
            paths = {"fused": lambda: ops.mbconv_infer_f32(x, cfg, *ps), "comp": lambda: ops.FusedMBConvFn.apply(x, cfg, *ps)}
            us = {}
            for name, fn in paths.items():
                with torch.no_grad():
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    C.lib().ofasr_profile_enable(1)
                    C.profile_read()
                    for _ in range(a.reps):
                        fn()
                    torch.cuda.synchronize()
                    prof = C.profile_read()
                    C.lib().ofasr_profile_enable(0)
                us[name] = sum(v["total_us"] for v in prof.values()) / a.reps
                if name == "comp":
                    comp_kernels = {k: round(v["total_us"] / a.reps, 1) for k, v in prof.items()}
            # HBM bytes by construction: fused reads x (+ the shortcut re-read) and writes out; the composite path writes
            # y1 / y2 / y3 (mid, mid, 64 channels), reads each back for its BN apply, and reads / writes the activations
            fused_b = 4 * px * 64 * 3
            comp_b = 4 * px * (64 + 2 * mid + 2 * mid + 2 * mid + 2 * mid + 2 * 64 + 64 + 64)
            tf = 2.0 * px * (2 * 64 * mid) / (us["fused"] * 1e-6) / 1e12
            print("%-10s %10.1f %10.1f %7.2fx %10.1f %10.1f %9.1f" % ("%d,%d" % (mid, K), us["fused"], us["comp"],
                                                                      us["comp"] / us["fused"], fused_b / 1e6,
                                                                      comp_b / 1e6, tf))
            print("    composite kernels (us/block):", comp_kernels)


if __name__ == "__main__":
    main()
