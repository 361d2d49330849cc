#!/usr/bin/env python3
"""YUV 4:2:0 frame upscaling (upscale.TiledUpscaler.upscale_yuv420): milliseconds per 1920x1080 frame at 4x for the max
S4 sub-network in fp32 and bf16, random he_fout weights, graphed, default core and batch:
  (a) fused     upscale_yuv420: the colour conversion inside the two tile moves, planar YUV only
  (b) unfused   ops.rgb_to_yuv420_u8(upscale(ops.yuv420_to_rgb_u8(frame))): this commit's whole-frame kernels around the
                RGB tile kernels, with both RGB frames in memory
  (c) network   the forwards of the same batches alone (graph replays on a gathered batch, no tile move)
Each is timed with a pair of events around --reps runs after one warm-up run.  Prints one JSON line (ms per frame, frames/s
of (a) and (b), and the peak memory each of (a) and (b) adds over the resident network).
usage: python tools/bench_video.py [--size 1080 1920] [--reps 3] [--precs f32 bf16]"""
import argparse
import importlib
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"
KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])
MAX = dict(ks=7, e=6, d=4, pixel_d=2)


def event_ms(fn, reps):
    """ms per call: one warm-up call, then two events around `reps` calls"""
    import torch
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def peak_extra_mb(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 2 ** 20, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[1080, 1920], metavar=("H", "W"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precs", nargs="+", default=["f32", "bf16"])
    a = ap.parse_args()
    import torch
    nets = importlib.import_module(PKG + ".elastic_nn.networks")
    st = importlib.import_module(PKG + ".imagenet_codebase.networks.sr_static")
    up = importlib.import_module(PKG + ".upscale")
    ops = importlib.import_module(PKG + ".ops")
    H, W = a.size
    g = torch.Generator().manual_seed(0)
    y = torch.randint(16, 236, (H, W), generator=g, dtype=torch.uint8).cuda()
    u, v = (torch.randint(16, 241, (H // 2, W // 2), generator=g, dtype=torch.uint8).cuda() for _ in range(2))
    sup = nets.OFAMobileNetS4(**KW)
    random.seed(0)
    sup.set_active_subnet(**MAX)
    net = st.build_static_net(sup.get_active_net_config())
    net.init_model("he_fout")
    net = net.cuda().eval()
    out = {"size": [H, W], "reps": a.reps, "runs": {}}
    for prec in a.precs:
        tu = up.TiledUpscaler(net, mix_prec=prec)
        plan = tu.plan(H, W)

        def fused():
            return tu.upscale_yuv420(y, u, v)

        def unfused():
            return ops.rgb_to_yuv420_u8(tu.upscale(ops.yuv420_to_rgb_u8(y, u, v)))

        batches = []

        def record(origins, h, w):
            x = up.tile_gather_yuv420(y, u, v, origins, h, w, tu.dtype)
            batches.append(x)
            return x

        tu._run_windows(H, W, y.device, False, lambda *args: None, record)      # the batches the plan makes, kept

        def network():
            with torch.no_grad():
                for x in batches:
                    tu._forward(x)

        ms = {"fused": event_ms(fused, a.reps), "unfused": event_ms(unfused, a.reps), "network": event_ms(network, a.reps)}
        del batches[:]
        rec = {"windows": len(plan), "window": [plan.win_h, plan.win_w], "ms": {k: round(t, 2) for k, t in ms.items()},
               "frames_per_s": {k: round(1e3 / ms[k], 3) for k in ("fused", "unfused")},
               "out_MP_per_s_fused": round(H * W * tu.scale ** 2 / 1e6 / (ms["fused"] / 1e3), 2),
               "peak_extra_MiB": {"fused": peak_extra_mb(fused), "unfused": peak_extra_mb(unfused)}}
        out["runs"]["max_" + prec] = rec
        print(prec, rec, file=sys.stderr, flush=True)
        del tu
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
