#!/usr/bin/env python3
"""The loss section of one progressive-shrinking sub-step: the reference lines -- output.float(),
nn.MSELoss, optionally F.mse_loss against the teacher, utils.psnr_y_device, and the backward of all of them down to the
network output -- against ops.sr_loss with psnr_count set and its backward, on a 16x3x256x256 bf16 output, an fp32 HR
batch and an fp32 teacher output (the teacher runs outside autocast).  Per variant (without / with the teacher term,
the fused path with kind mse, l1 and charbonnier):
  * GPU kernels launched per section, counted by torch.profiler (null where the profiler gives no device events);
  * the section's time: device events around each of `--reps` runs (median), the two paths alternating in one process,
    and the wall time per section of `--reps` back-to-back runs ended by one synchronise (what a host-bound step pays);
  * the three new kernels alone, from the library's per-launch events, against the bytes they move at the 8.0 TB/s HBM
    peak and the 6.3 TB/s measured copy rate.
The SSIM section (key "ssim"): on the same tensors, ops.sr_loss(ssim=A) for each kind, without /
with the teacher term, against an ATen statement of the same loss -- fp32, the five moments as one grouped F.conv2d with
the 11 x 11 window each, autograd -- with launches, device time and wall time of forward plus backward for both, the two
alternating in one process, and the SSIM kernels alone from the library's per-launch events.
Prints one JSON line.  usage: python tools/bench_loss.py [--reps 200] [--warmup 20] [--ssim 0.2]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"
HBM_TBPS, COPY_TBPS = 8.0, 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shape", default="16x256x256")
    ap.add_argument("--no-launch-count", action="store_true", help="leave torch.profiler out")
    ap.add_argument("--ssim", type=float, default=0.2, metavar="A", help="the SSIM weight of the SSIM section (0: skip it)")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    C = importlib.import_module(PKG + "._C")
    ops = importlib.import_module(PKG + ".ops")
    utils = importlib.import_module(PKG + ".utils")
    losses = importlib.import_module(PKG + ".losses")
    L = C.lib()
    sync = torch.cuda.synchronize
    N, H, W = (int(v) for v in a.shape.split("x"))
    g = torch.Generator(device="cuda").manual_seed(0)
    images = torch.rand(N, 3, H, W, device="cuda", generator=g)
    out16 = (images + 0.05 * torch.randn(N, 3, H, W, device="cuda", generator=g)).to(torch.bfloat16).requires_grad_(True)
    soft = images + 0.02 * torch.randn(N, 3, H, W, device="cuda", generator=g)   # the teacher runs outside autocast: fp32
    kd = 1.0
    crit = torch.nn.MSELoss()
    count = losses.mosaic_count(N, H, W)

    def reference(teacher):
        out16.grad = None
        output = out16.float()
        loss = crit(output, images)
        if teacher:
            loss = (kd * F.mse_loss(output, soft) + loss) * (2 / (kd + 1))
        psnr = utils.psnr_y_device(output, images)
        loss.backward()
        return loss, psnr

    def fused(kind, teacher):
        out16.grad = None
        w_main, w_kd = losses.kd_weights(kd, True) if teacher else (1.0, 0.0)
        loss, res = ops.sr_loss(out16, images, soft if teacher else None, kind=kind, w_main=w_main, w_kd=w_kd,
                                psnr_count=count)
        loss.backward()
        return loss, res[ops.SR_LOSS_PSNR]

    def fused_ssim(kind, teacher):
        out16.grad = None
        w_main, w_kd = losses.kd_weights(kd, True) if teacher else (1.0, 0.0)
        loss, res = ops.sr_loss(out16, images, soft if teacher else None, kind=kind, w_main=w_main, w_kd=w_kd,
                                psnr_count=count, ssim=a.ssim)
        loss.backward()
        return loss, res[ops.SR_LOSS_SSIM]

    gw = torch.from_numpy(losses.ssim_window()).float().cuda()
    win = (gw[:, None] * gw[None, :])[None, None].repeat(3, 1, 1, 1).contiguous()
    eps2 = float(losses.eps2_f32(losses.DEFAULT_EPS))

    def rho(x, kind):
        if kind == "mse":
            return (x * x).mean()
        if kind == "l1":
            return x.abs().mean()
        return torch.sqrt(x * x + eps2).mean()

    def aten_ssim(kind, teacher):
        """the same loss through ATen in fp32 (no PSNR: the loss alone)"""
        out16.grad = None
        w_main, w_kd = losses.kd_weights(kd, True) if teacher else (1.0, 0.0)
        o = out16.float()
        pix = w_main * rho(o - images, kind)
        if teacher:
            pix = pix + w_kd * rho(o - soft, kind)
        conv = lambda x: F.conv2d(x, win, groups=3)
        m1, m2 = conv(o), conv(images)
        s1, s2, s12 = conv(o * o) - m1 * m1, conv(images * images) - m2 * m2, conv(o * images) - m1 * m2
        S = (((2 * m1 * m2 + 1e-4) * (2 * s12 + 9e-4)) / ((m1 * m1 + m2 * m2 + 1e-4) * (s1 + s2 + 9e-4))).mean()
        loss = (1.0 - a.ssim) * pix + a.ssim * (1.0 - S)
        loss.backward()
        return loss, S

    def launches(fn):
        if a.no_launch_count:
            return None
        try:
            from torch.profiler import ProfilerActivity, profile
            fn()
            sync()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                sync()
            n = sum(1 for e in prof.events() if "cuda" in str(e.device_type).lower() and "memcpy" not in e.name.lower()
                    and "memset" not in e.name.lower())
            return n or None
        except Exception as exc:        # a profiler without device tracing: the count stays unmeasured
            return "unmeasured: %s" % type(exc).__name__

    def device_us(fns):
        """median device-event time of each section, the sections alternating"""
        for _ in range(a.warmup):
            for fn in fns:
                fn()
        sync()
        ts = [[] for _ in fns]
        evs = []
        for _ in range(a.reps):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                evs.append((i, e0, e1))
        sync()
        for i, e0, e1 in evs:
            ts[i].append(1e3 * e0.elapsed_time(e1))
        return [sorted(t)[len(t) // 2] for t in ts]

    def wall_us(fn):
        for _ in range(a.warmup):
            fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        sync()
        return 1e6 * (time.perf_counter() - t0) / a.reps

    out = {"shape": [N, 3, H, W], "output": "bfloat16", "reps": a.reps, "sections": [], "kernels": []}
    for teacher in (False, True):
        ref = lambda: reference(teacher)
        variants = [("reference", ref)] + [(k, (lambda k=k: fused(k, teacher))) for k in losses.KINDS]
        dev = device_us([fn for _, fn in variants])
        for (name, fn), d in zip(variants, dev):
            out["sections"].append({"loss": name, "teacher": teacher, "gpu_launches": launches(fn), "device_us": d,
                                    "wall_us": wall_us(fn)})
        l_ref, p_ref = reference(teacher)
        l_new, p_new = fused("mse", teacher)
        out["sections"][-3]["loss_vs_reference"] = [float(l_new.detach()), float(l_ref.detach())]
        out["sections"][-3]["psnr_vs_reference"] = [float(p_new), float(p_ref)]
        # the three kernels alone
        for kind in losses.KINDS:
            fused(kind, teacher)
            sync()
            L.ofasr_profile_enable(1)
            C.profile_read()
            for _ in range(a.reps):
                fused(kind, teacher)
            prof = C.profile_read()
            L.ofasr_profile_enable(0)
            for sym, v in sorted(prof.items()):
                if "sr_loss" not in sym:
                    continue
                us = v["total_us"] / v["launches"]
                by = v["bytes"] / v["launches"]
                out["kernels"].append({"kernel": sym, "kind": kind, "teacher": teacher, "us": us, "bytes": by,
                                       "TBps": by / us * 1e-6 if us else None,
                                       "fraction_of_hbm_peak": by / us * 1e-6 / HBM_TBPS if us else None,
                                       "fraction_of_copy_rate": by / us * 1e-6 / COPY_TBPS if us else None})
    if a.ssim > 0:
        out["ssim"] = {"alpha": a.ssim, "sections": [], "kernels": []}
        for teacher in (False, True):
            variants = [("fused", k, (lambda k=k: fused_ssim(k, teacher))) for k in losses.KINDS]
            variants += [("aten", k, (lambda k=k: aten_ssim(k, teacher))) for k in losses.KINDS]
            dev = device_us([fn for _, _, fn in variants])
            for (path, kind, fn), d in zip(variants, dev):
                loss, S = fn()
                out["ssim"]["sections"].append({"path": path, "loss": kind, "teacher": teacher, "gpu_launches": launches(fn),
                                                "device_us": d, "wall_us": wall_us(fn), "value": float(loss.detach()),
                                                "S": float(S.detach())})
            for kind in losses.KINDS:
                fused_ssim(kind, teacher)
                sync()
                L.ofasr_profile_enable(1)
                C.profile_read()
                for _ in range(a.reps):
                    fused_ssim(kind, teacher)
                prof = C.profile_read()
                L.ofasr_profile_enable(0)
                for sym, v in sorted(prof.items()):
                    if "sr_loss" in sym or "sr_ssim" in sym:
                        out["ssim"]["kernels"].append({"kernel": sym, "kind": kind, "teacher": teacher,
                                                       "us": v["total_us"] / v["launches"]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
