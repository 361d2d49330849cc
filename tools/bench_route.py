#!/usr/bin/env python3
"""Content-aware routing (upscale.TiledUpscaler(easy_net=..., easy_threshold=T)): what it costs and what it gains on a
1920x1080 8-bit YUV 4:2:0 clip of which about half the area is flat, at 4x, graphed, default core and batch.  hard = the max
S4 sub-network, easy = the min one (ks 3, e 3, d 2, pixel_d 1), random he_fout weights.  The flat area is the constant left
part of the luma plane, cut where a window column of the plan ends, so that a window is either all flat or not; the rest is
smooth content plus noise.  Per precision, ms per frame (wall clock around --reps frames after one warm-up frame, --rounds
times, the modes interleaved within a round; median and range reported) of
  plain      TiledUpscaler(hard).upscale_yuv420                      (the path without routing)
  all_hard   the routed upscaler at T = -1: plain + the two kernels and the read-back of the two counts
  routed     the routed upscaler at --threshold
  all_easy   the routed upscaler at T = inf
and, from the library's per-dispatch events of three profiled routed frames, the time and GB/s of the activity and routing
kernels, and "route_alone_ms": activity + routing + the read-back of the two counts run alone, back to back (wall clock
over 200 calls), which is what a frame pays for routing when nothing else is in the way.  Prints one JSON line.
--plain-only measures `plain` alone and needs nothing of the routing feature, so the same file can time another checkout
of the project: --tree DIR imports the package from DIR instead of this checkout.
usage: python tools/bench_route.py [--size 1080 1920] [--reps 5] [--rounds 3] [--precs f32 bf16] [--threshold 1.0]
       [--core N] [--batch N] [--plain-only] [--tree DIR]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

PKG = "ofa-for-super-resolution_amd"
KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])
MAX = dict(ks=7, e=6, d=4, pixel_d=2)
MIN = dict(ks=3, e=3, d=2, pixel_d=1)


def wall_ms(fn, frames, reps):
    import torch
    fn(frames[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(frames[i % len(frames)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def summary(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def make_clip(n, H, W, flat_cols, seed):
    """n frames: luma constant left of flat_cols, smooth content plus noise right of it; chroma smooth"""
    import torch
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        base = torch.rand(1, 1, H // 16 + 2, W // 16 + 2, generator=g)
        y = torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear", align_corners=False)[0, 0] * 160 + 30
        y = (y + torch.rand(H, W, generator=g) * 40).clamp(16, 235).to(torch.uint8)
        y[:, :flat_cols] = 96
        u, v = (torch.randint(112, 144, (H // 2, W // 2), generator=g, dtype=torch.uint8) for _ in range(2))
        out.append((y.cuda(), u.cuda(), v.cuda()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[1080, 1920], metavar=("H", "W"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precs", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--threshold", default="1.0", help="easy_threshold of the routed mode")
    ap.add_argument("--core", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    import torch
    C = importlib.import_module(PKG + "._C")
    nets = importlib.import_module(PKG + ".elastic_nn.networks")
    st = importlib.import_module(PKG + ".imagenet_codebase.networks.sr_static")
    up = importlib.import_module(PKG + ".upscale")
    H, W = a.size

    def static(setting, seed):
        sup = nets.OFAMobileNetS4(**KW)
        sup.set_active_subnet(**setting)
        net = st.build_static_net(sup.get_active_net_config())
        torch.manual_seed(seed)
        net.init_model("he_fout")
        return net.cuda().eval()

    hard, easy = static(MAX, 0), static(MIN, 1)
    out = {"size": [H, W], "reps": a.reps, "rounds": a.rounds, "threshold": a.threshold, "tree": a.tree, "runs": {}}
    for prec in a.precs:
        plain = up.TiledUpscaler(hard, core=a.core, batch=a.batch, mix_prec=prec)
        plan = plain.plan(H, W)
        # the flat part ends where the window column whose core ends nearest the middle ends
        ends = sorted(set(cx + cw for (_, _, _, cx, _, cw) in plan.windows))
        mid = min(ends, key=lambda e: abs(e - W // 2))
        flat_cols = max(wx + plan.win_w for (_, wx, _, cx, _, cw) in plan.windows if cx + cw <= mid)
        clip = make_clip(4, H, W, flat_cols, 7)
        modes = {"plain": lambda fr: plain.upscale_yuv420(*fr)}
        rec = {"windows": len(plan), "window": [plan.win_h, plan.win_w], "batch": plain._batching(plan)[1],
               "core": plain.core, "flat_area": round(flat_cols / float(W), 4)}
        if not a.plain_only:
            routed = {}
            for name, T in (("all_hard", -1), ("routed", a.threshold), ("all_easy", float("inf"))):
                routed[name] = up.TiledUpscaler(hard, core=a.core, batch=a.batch, mix_prec=prec, easy_net=easy, easy_threshold=T)
                modes[name] = (lambda tu: lambda fr: tu.upscale_yuv420(*fr))(routed[name])
            rplan = routed["routed"].plan(H, W)
            assert rplan.windows == plan.windows, "the shared plan differs from the hard network's"
            routed["routed"].upscale_yuv420(*clip[0])
            rec["route_stats"] = routed["routed"].route_stats
            rec["easy_share"] = round(rec["route_stats"]["easy"] / float(len(plan)), 4)
            act = routed["routed"].window_activity(clip[0])
            rec["activity"] = {"min": round(float(act.min()), 4), "median": round(float(act.median()), 4),
                               "max": round(float(act.max()), 4)}
        times = {k: [] for k in modes}
        for _ in range(a.rounds):
            for k, fn in modes.items():
                times[k].append(wall_ms(fn, clip, a.reps))
        rec["ms"] = {k: summary(v) for k, v in times.items()}
        rec["ms_rounds"] = {k: [round(t, 3) for t in v] for k, v in times.items()}
        if not a.plain_only:
            C.profile_read()
            C.lib().ofasr_profile_enable(1)
            for _ in range(3):
                routed["routed"].upscale_yuv420(*clip[1])
            torch.cuda.synchronize()
            prof = C.profile_read()
            C.lib().ofasr_profile_enable(0)
            rec["kernels"] = {}
            for key in ("window_activity_kernel", "window_route_kernel"):
                hit = [v for k, v in prof.items() if key in k]
                us = sum(v["total_us"] for v in hit) / max(sum(v["launches"] for v in hit), 1)
                by = sum(v["bytes"] for v in hit) / max(sum(v["launches"] for v in hit), 1)
                rec["kernels"][key] = {"us": round(us, 2), "bytes": int(by), "GB_per_s": round(by / max(us, 1e-9) / 1e3, 2)}
            tu = routed["routed"]
            origins, table = tu._tables(plan, clip[0][0].device)
            B = tu._batching(plan)[1]
            rec["route_alone_ms"] = round(wall_ms(lambda fr: tu._route(fr[0], plan, origins, table, B), clip, 200), 4)
            m = rec["ms"]
            share = rec["easy_share"]
            rec["overhead_ms"] = round(m["all_hard"]["median"] - m["plain"]["median"], 3)
            rec["gain_ms"] = round(m["plain"]["median"] - m["routed"]["median"], 3)
            # linear expectation: the easy share of the hard time is replaced by the easy share of the all-easy time
            rec["expected_routed_ms"] = round((1 - share) * m["all_hard"]["median"] + share * m["all_easy"]["median"], 3)
        out["runs"][prec] = rec
        print(prec, rec, file=sys.stderr, flush=True)
        del plain, modes
        if not a.plain_only:
            del routed
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
