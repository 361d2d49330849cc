#!/usr/bin/env python3
"""Tiled upscaling throughput (upscale.TiledUpscaler): output megapixels/s for a 1920x1080 input at 4x, for the max S4
sub-network and a small one, in fp32 and bf16 (graphed, default core and batch, after one warm-up upscale; wall time of
--reps upscales ending in a device sync); the halo overhead (window pixels / core pixels); and the share of the gather /
scatter kernels in the GPU time of one eager upscale, from the library's per-launch events (every kernel of the path is a
library kernel; ATen's pads / casts are not counted).  Random he_fout weights.  Prints one JSON line.
--self-ensemble K adds, per run, the same measurement with TiledUpscaler(self_ensemble=K): MP/s beside the plain MP/s of
the same run, its ratio to the ideal plain / K, and each D4 kernel's (csrc/d4.hip) time from the per-launch events of one
eager upscale against its byte floor (the bytes the launches annotate -- apply: 2 B per element, accumulate: B + 8, B + 4
on the first call -- at the measured 6.3 TB/s copy rate) and their share of the kernel time.
usage: python tools/bench_upscale.py [--size 1080 1920] [--reps 5] [--self-ensemble 8]"""
import argparse
import importlib
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"
KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])
COPY_RATE = 6.3e12   # bytes / s, the measured device copy rate
NETS = {"max": dict(ks=7, e=6, d=4, pixel_d=2), "small": dict(ks=3, e=3, d=2, pixel_d=2)}


def timed(tu, img, reps):
    """(seconds per upscale, output) after one warm-up upscale"""
    import torch
    tu.upscale(img)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        y = tu.upscale(img)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, y


def profiled(C, tu, img):
    """the library's per-launch events of one eager upscale (after a warm-up one)"""
    import torch
    tu.upscale(img)
    torch.cuda.synchronize()
    C.profile_read()
    C.lib().ofasr_profile_enable(1)
    tu.upscale(img)
    torch.cuda.synchronize()
    prof = C.profile_read()
    C.lib().ofasr_profile_enable(0)
    return prof


def ensemble_run(C, up, net, prec, k, img, reps, plain_mp_s):
    import torch
    tu = up.TiledUpscaler(net, mix_prec=prec, self_ensemble=k)
    plan = tu.plan(img.shape[0], img.shape[1])
    dt, y = timed(tu, img, reps)
    mp = y.shape[0] * y.shape[1] / 1e6
    del tu, y
    torch.cuda.empty_cache()
    prof = profiled(C, up.TiledUpscaler(net, mix_prec=prec, graphed=False, self_ensemble=k), img)
    total = sum(v["total_us"] for v in prof.values())
    rec = {"k": k, "windows": len(plan), "window": [plan.win_h, plan.win_w], "ms_per_image": round(dt * 1e3, 2),
           "out_MP_per_s": round(mp / dt, 2), "ratio_to_plain_over_k": round(mp / dt / (plain_mp_s / k), 4),
           "gpu_ms_eager": round(total / 1e3, 2)}
    d4 = 0.0
    for tag, what in (("apply", "false"), ("accumulate", "true")):
        # d4_flip_kernel<T, ACC, VEC> / d4_tr_kernel<T, ACC>: the second template argument tells the two calls apart
        sel = [v for name, v in prof.items()
               if "d4_" in name and "<" in name and name.split("<", 1)[1].split(",")[1].strip(" >") == what]
        us, by, n = sum(v["total_us"] for v in sel), sum(v["bytes"] for v in sel), sum(v["launches"] for v in sel)
        d4 += us
        rec["d4_" + tag] = {"launches": int(n), "us": round(us, 1), "floor_us": round(by / COPY_RATE * 1e6, 1),
                            "fraction_of_floor": round(by / COPY_RATE * 1e6 / us, 3) if us else None}
    rec["d4_share"] = round(d4 / total, 5) if total else None
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[1080, 1920], metavar=("H", "W"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nets", nargs="+", default=list(NETS))
    ap.add_argument("--precs", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--self-ensemble", type=int, default=1, choices=[1, 2, 4, 8], metavar="K")
    a = ap.parse_args()
    import torch
    C = importlib.import_module(PKG + "._C")
    nets = importlib.import_module(PKG + ".elastic_nn.networks")
    st = importlib.import_module(PKG + ".imagenet_codebase.networks.sr_static")
    up = importlib.import_module(PKG + ".upscale")
    H, W = a.size
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
    out = {"size": [H, W], "reps": a.reps, "runs": {}}
    for name in a.nets:
        sup = nets.OFAMobileNetS4(**KW)
        random.seed(0)
        sup.set_active_subnet(**NETS[name])
        net = st.build_static_net(sup.get_active_net_config())
        net.init_model("he_fout")
        net = net.cuda().eval()
        for prec in a.precs:
            tu = up.TiledUpscaler(net, mix_prec=prec)
            plan = tu.plan(H, W)
            tu.upscale(img)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                y = tu.upscale(img)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.reps
            mp = y.shape[0] * y.shape[1] / 1e6
            # gather / scatter share of one eager upscale's library kernel time
            eager = up.TiledUpscaler(net, mix_prec=prec, graphed=False)
            eager.upscale(img)
            torch.cuda.synchronize()
            C.profile_read()
            C.lib().ofasr_profile_enable(1)
            eager.upscale(img)
            torch.cuda.synchronize()
            prof = C.profile_read()
            C.lib().ofasr_profile_enable(0)
            total = sum(v["total_us"] for v in prof.values())
            tio = sum(v["total_us"] for k, v in prof.items() if "tile_gather" in k or "tile_scatter" in k)
            out["runs"]["%s_%s" % (name, prec)] = {
                "radius": tu.radius, "core": tu.core, "windows": len(plan), "window": [plan.win_h, plan.win_w],
                "halo_overhead": round(plan.overhead(), 3), "ms_per_image": round(dt * 1e3, 2),
                "out_MP_per_s": round(mp / dt, 2), "gpu_ms_eager": round(total / 1e3, 2),
                "gather_scatter_us": round(tio, 1), "gather_scatter_share": round(tio / total, 5) if total else None}
            del tu, eager
            torch.cuda.empty_cache()
            if a.self_ensemble != 1:
                out["runs"]["%s_%s" % (name, prec)]["self_ensemble"] = ensemble_run(C, up, net, prec, a.self_ensemble, img,
                                                                                    a.reps, mp / dt)
            print(name, prec, out["runs"]["%s_%s" % (name, prec)], file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
