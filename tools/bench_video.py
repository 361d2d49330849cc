#!/usr/bin/env python3
"""YUV 4:2:0 frame upscaling (upscale.TiledUpscaler.upscale_yuv420): milliseconds per 1920x1080 frame at 4x for the max
S4 sub-network in fp32 and bf16, random he_fout weights, graphed, default core and batch:
  (a) fused     upscale_yuv420: the colour conversion inside the two tile moves, planar YUV only
  (b) unfused   ops.rgb_to_yuv420_u8(upscale(ops.yuv420_to_rgb_u8(frame))): this commit's whole-frame kernels around the
                RGB tile kernels, with both RGB frames in memory
  (c) network   the forwards of the same batches alone (graph replays on a gathered batch, no tile move)
Each is timed with a pair of events around --reps runs after one warm-up run.  Prints one JSON line (ms per frame, frames/s
of (a) and (b), and the peak memory each of (a) and (b) adds over the resident network).

--reuse FRACTION [FRACTION ...] measures window reuse between frames (upscale.YUV420Stream) instead: a synthetic clip of
two alternating frames that differ in one luma sample at the core centre of every window that is to change, the rest of
the windows static (about FRACTION of the plan; with small cores a centre can lie in a neighbour's halo too, so the
fraction of windows that really ran is reported beside the one asked for).  Per fraction: wall-clock frames/s over --reps
frames of per-frame upscale_yuv420 and of the stream on the same clip in the same process, and once per precision the
cost of what the stream adds to a frame where nothing is skipped: diff + compaction + the count's read-back, timed alone.

--depth 10 runs the same on a 10-bit frame (uint16 planes, the 16-bit tile moves and window diff), --out-depth 8|10 sets
the output's depth independently (default: the input's; 8 -> 10 is the 8-bit gather with the 16-bit scatter).  There is no
whole-frame 10-bit kernel, so (b) is left out whenever either depth is 10.

--out-size WxH measures target-size output (upscale_yuv420(out_size=...), the resampling scatter) beside the full-size
frame: "fused" and "target" are timed alternately, twice each, in the same process ("ms_rounds"); the record adds the
plan overhead (window pixels per input pixel) with and without the target, the scatter's own time per frame from the
library's launch events of one profiled frame ("scatter_ms": the full-size and the resampling scatter), and the bytes a
frame copies to the host at either size.  --resample bicubic|lanczos picks the filter.
usage: python tools/bench_video.py [--size 1080 1920] [--reps 3] [--precs f32 bf16] [--reuse 0 0.5 0.9 1.0] [--core N]
       [--batch N] [--depth 8|10] [--out-depth 8|10] [--out-size WxH] [--resample lanczos]"""
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


def wall_ms(fn, reps):
    """ms per call by the host's clock: one warm-up call, then `reps` calls and a synchronisation"""
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def bench_reuse(up, tu, planes, fractions, reps, out_depth=None):
    """frames/s with and without reuse on two alternating frames, per fraction of static windows"""
    import torch
    y, u, v = planes
    H, W = y.shape
    plan = tu.plan(H, W)
    n = len(plan)
    _, B = tu._batching(plan)
    rec = {"windows": n, "window": [plan.win_h, plan.win_w], "batch": B, "overhead": round(plan.overhead(), 3), "fractions": {}}
    stream = tu.yuv420_stream(out_depth=out_depth)
    for frac in fractions:
        moving = plan.windows[:n - int(round(frac * n))]
        other = y.cpu().numpy().copy()                    # on the host: torch has no arithmetic on uint16
        for (_, _, cy, cx, ch, cw) in moving:
            other[cy + ch // 2, cx + cw // 2] ^= 0x40
        other = torch.from_numpy(other).to(y.device)
        clip = [(y, u, v), (other, u, v)]
        state = {"i": 0, "run": 0, "frames": 0}

        def plain():
            state["i"] ^= 1
            return tu.upscale_yuv420(*clip[state["i"]], out_depth=out_depth)

        def reuse():
            state["i"] ^= 1
            out = stream.upscale(*clip[state["i"]])
            state["run"] += stream.stats.run
            state["frames"] += 1
            return out

        stream.reset()
        ms_plain = wall_ms(plain, reps)
        reuse()                                            # the stream's first frame runs every window: not part of the clip
        state.update(run=0, frames=0)
        ms_reuse = wall_ms(reuse, reps)
        rec["fractions"]["%g" % frac] = {
            "static_asked": frac, "windows_run_per_frame": round(state["run"] / state["frames"], 2),
            "static_measured": round(1.0 - state["run"] / float(state["frames"] * n), 4),
            "ms": {"plain": round(ms_plain, 3), "reuse": round(ms_reuse, 3)},
            "frames_per_s": {"plain": round(1e3 / ms_plain, 3), "reuse": round(1e3 / ms_reuse, 3)}}
    # what a frame pays when nothing is skipped: the two kernels and the read-back of the count, alone
    origins, table = tu._tables(plan, y.device)
    flags = up.window_diff_yuv420(y, u, v, y, u, v, origins[:n], plan.win_h, plan.win_w)
    bufs = up.window_compact(flags, origins[:n], table, B)

    def price():
        up.window_diff_yuv420(y, u, v, other, u, v, origins[:n], plan.win_h, plan.win_w, flags)
        return int(up.window_compact(flags, origins[:n], table, B, bufs)[3].item())

    rec["diff_compact_readback_ms"] = round(wall_ms(price, max(reps, 20)), 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[1080, 1920], metavar=("H", "W"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precs", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--reuse", type=float, nargs="+", default=None, metavar="FRACTION",
                    help="measure window reuse with this fraction of static windows instead (several: one run each)")
    ap.add_argument("--core", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--depth", type=int, default=8, choices=[8, 10], help="bits per input sample")
    ap.add_argument("--out-depth", type=int, default=None, choices=[8, 10], help="bits per output sample (default: --depth)")
    ap.add_argument("--out-size", default=None, metavar="WxH", help="also measure this target size (even sides)")
    ap.add_argument("--resample", default="lanczos", choices=["bicubic", "lanczos"])
    a = ap.parse_args()
    import torch
    C = importlib.import_module(PKG + "._C")
    target = None
    if a.out_size is not None:
        try:
            tw, th = importlib.import_module(PKG + ".resize").parse_size(a.out_size)
        except ValueError as e:
            raise SystemExit("--out-size: %s" % e)
        target = (th, tw)
    nets = importlib.import_module(PKG + ".elastic_nn.networks")
    st = importlib.import_module(PKG + ".imagenet_codebase.networks.sr_static")
    up = importlib.import_module(PKG + ".upscale")
    ops = importlib.import_module(PKG + ".ops")
    H, W = a.size
    g = torch.Generator().manual_seed(0)
    out_depth = a.depth if a.out_depth is None else a.out_depth
    if a.depth == 8:
        y = torch.randint(16, 236, (H, W), generator=g, dtype=torch.uint8).cuda()
        u, v = (torch.randint(16, 241, (H // 2, W // 2), generator=g, dtype=torch.uint8).cuda() for _ in range(2))
    else:                                                  # legal 10-bit values, made as int16 (torch.randint has no uint16)
        y = torch.randint(64, 941, (H, W), generator=g, dtype=torch.int16).view(torch.uint16).cuda()
        u, v = (torch.randint(64, 961, (H // 2, W // 2), generator=g, dtype=torch.int16).view(torch.uint16).cuda()
                for _ in range(2))
    sup = nets.OFAMobileNetS4(**KW)
    random.seed(0)
    sup.set_active_subnet(**MAX)
    net = st.build_static_net(sup.get_active_net_config())
    net.init_model("he_fout")
    net = net.cuda().eval()
    out = {"size": [H, W], "reps": a.reps, "depth": a.depth, "out_depth": out_depth, "runs": {}}
    for prec in a.precs:
        tu = up.TiledUpscaler(net, core=a.core, batch=a.batch, mix_prec=prec)
        plan = tu.plan(H, W)
        if a.reuse is not None:
            if any(not 0.0 <= f <= 1.0 for f in a.reuse):
                raise SystemExit("--reuse takes fractions in 0 .. 1")
            rec = bench_reuse(up, tu, (y, u, v), a.reuse, a.reps, out_depth)
            out["runs"]["max_" + prec] = rec
            print(prec, rec, file=sys.stderr, flush=True)
            del tu
            torch.cuda.empty_cache()
            continue

        def fused():
            return tu.upscale_yuv420(y, u, v, out_depth=out_depth)

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

        paths = {"fused": fused, "unfused": unfused} if a.depth == out_depth == 8 else {"fused": fused}
        extra = {}
        if target is not None:
            def resized():
                return tu.upscale_yuv420(y, u, v, out_depth=out_depth, out_size=target, resample=a.resample)

            tplan = tu.plan(H, W, target, a.resample, True)
            rounds = {"fused": [], "target": []}
            for _ in range(2):                             # alternating, same process
                rounds["fused"].append(round(event_ms(fused, a.reps), 2))
                rounds["target"].append(round(event_ms(resized, a.reps), 2))
            scatter = {}
            for name, fn in (("fused", fused), ("target", resized)):
                C.profile_read()
                C.lib().ofasr_profile_enable(1)
                fn()
                torch.cuda.synchronize()
                prof = C.profile_read()
                C.lib().ofasr_profile_enable(0)
                scatter[name] = round(sum(v["total_us"] for k, v in prof.items() if "scatter" in k) / 1e3, 3)
            bps = 1 if out_depth == 8 else 2
            extra = {"out_size": [target[1], target[0]], "resample": a.resample, "ms_rounds": rounds, "scatter_ms": scatter,
                     "overhead": {"full": round(plan.overhead(), 3), "target": round(tplan.overhead(), 3)},
                     "windows_target": len(tplan), "window_target": [tplan.win_h, tplan.win_w],
                     "halo": {"full": tu.halo, "target": getattr(tplan, "halo", tu.halo)},
                     "host_bytes_per_frame": {"full": H * W * tu.scale ** 2 * 3 // 2 * bps,
                                              "target": target[0] * target[1] * 3 // 2 * bps},
                     "peak_extra_MiB_target": peak_extra_mb(resized)}
        ms = {k: event_ms(fn, a.reps) for k, fn in paths.items()}
        ms["network"] = event_ms(network, a.reps)
        del batches[:]
        rec = {"windows": len(plan), "window": [plan.win_h, plan.win_w], "ms": {k: round(t, 2) for k, t in ms.items()},
               "frames_per_s": {k: round(1e3 / ms[k], 3) for k in paths},
               "out_MP_per_s_fused": round(H * W * tu.scale ** 2 / 1e6 / (ms["fused"] / 1e3), 2),
               "peak_extra_MiB": {k: peak_extra_mb(fn) for k, fn in paths.items()}}
        rec.update(extra)
        out["runs"]["max_" + prec] = rec
        print(prec, rec, file=sys.stderr, flush=True)
        del tu
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
