#!/usr/bin/env python3
"""Scene cuts (csrc/scene.hip, scenes.py, scenes_ofa_net_sr.py, upscale_video_ofa_net_sr.py --scene-map): the three
measurements of DESIGN.md 3.1o on 1920x1080 8-bit frames.
  kernels   ofasr_rgb_hist_yuv420 + ofasr_hist_fold_distance against what the project offered before for the same
            histograms, ops.yuv420_to_rgb_u8 + three torch.bincount, on a random and on a flat frame (results checked
            equal): us per frame from device events around a loop of both (--rounds times, alternating), and each library
            kernel's own begin -> end time from the per-dispatch events, with the GB/s of the bytes it notes.
  tool      scenes_ofa_net_sr.py on a --frames long yuv420p file against the same tool with --no-kernel (frames read and
            uploaded, nothing launched), each a fresh process, alternating.
  upscale   upscale_video_ofa_net_sr.py (bf16) on --upscale-frames N and 2 N frames of the file: one export a, one export
            b, and --scene-map switching between them every --scene-length frames; the steady state is
            N / (t(2 N) - t(N)), which leaves out start-up and the first capture of each export.  a / b: the S4
            sub-networks (ks 3, e 3, d 2, pixel_d 1 / 0), random he_fout weights.
usage: python tools/bench_scenes.py [--rounds 3] [--frames 240] [--upscale-frames 64] [--scene-length 8] [--skip-upscale]"""
import argparse
import importlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"
KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])
H, W = 1080, 1920
DEV = "cuda:0"


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


def planes(kind, seed=0):
    rng = np.random.RandomState(seed)
    if kind == "random":
        p = (rng.randint(0, 256, (H, W)), rng.randint(0, 256, (H // 2, W // 2)), rng.randint(0, 256, (H // 2, W // 2)))
    else:
        p = (np.full((H, W), 16), np.full((H // 2, W // 2), 128), np.full((H // 2, W // 2), 128))
    return tuple(torch.from_numpy(x.astype(np.uint8)).to(DEV) for x in p)


def timed(fn, n):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n           # us per call


def bench_kernels(rounds):
    ops = importlib.import_module(PKG + ".ops")
    C = importlib.import_module(PKG + "._C")
    S = ops.rgb_hist_slabs(H, W)
    say("device", torch.cuda.get_device_name(0), "slabs(1080p) =", S)
    partial = torch.empty(S, 3, 256, dtype=torch.int32, device=DEV)
    ring = torch.zeros(2, 3, 256, dtype=torch.int32, device=DEV)
    dist = torch.zeros(1, dtype=torch.int64, device=DEV)
    for kind in ("random", "flat"):
        y, u, v = planes(kind)

        def new():
            ops.rgb_hist_yuv420(y, u, v, out=partial)
            ops.hist_fold_distance(partial, ring[0], ring[1], dist)

        def old():
            rgb = ops.yuv420_to_rgb_u8(y, u, v).view(-1, 3)
            return [torch.bincount(rgb[:, c], minlength=256) for c in range(3)]

        new()
        assert torch.equal(ring[0].to(torch.int64), torch.stack(old())), kind
        for rnd in range(rounds):
            say("%s round %d: hist + fold (2 launches) %.2f us/frame   decode + 3 bincount %.2f us/frame"
                % (kind, rnd, timed(new, 400), timed(old, 100)))
        torch.cuda.synchronize()
        C.lib().ofasr_profile_enable(1)
        for _ in range(100):
            new()
        for _ in range(20):
            ops.yuv420_to_rgb_u8(y, u, v)
        torch.cuda.synchronize()
        C.lib().ofasr_profile_enable(0)
        for name, r in sorted(C.profile_read().items()):
            us, nbytes = r["total_us"] / r["launches"], r["bytes"] / r["launches"]
            say("%s kernel %s: %.2f us, %.0f bytes noted -> %.1f GB/s (%.1f %% of the 8 TB/s HBM peak)"
                % (kind, name.split("(")[0][-60:], us, nbytes, nbytes / us / 1e3, 100 * nbytes / us / 1e6 / 8.0))


def write_clip(path, n, seed=1):
    """n frames: 6 random ones and a flat one, each held for 5 frames"""
    rng = np.random.RandomState(seed)
    pool = [rng.randint(16, 236, H * W * 3 // 2).astype(np.uint8).tobytes() for _ in range(6)]
    pool.append(np.full(H * W * 3 // 2, 128, np.uint8).tobytes())
    with open(path, "wb") as f:
        for i in range(n):
            f.write(pool[(i // 5) % len(pool)])
    say("file: %d frames of 1920x1080 yuv420p, %.0f MB" % (n, os.path.getsize(path) / 1e6))


def run_tool(cmd):
    r = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return [ln for ln in r.stdout.splitlines() if "frames/s" in ln][0]


def bench_tool(path, rounds):
    tool = [os.path.join(ROOT, "scenes_ofa_net_sr.py"), "--size", "1920x1080", "--top", "0"]
    for rnd in range(rounds):
        for label, extra in (("reader alone", ["--no-kernel"]), ("detector", [])):
            say("tool round %d %-12s: %s" % (rnd, label, run_tool(tool + extra + [path])))


def export(setting, seed, d):
    nets = importlib.import_module(PKG + ".elastic_nn.networks")
    st = importlib.import_module(PKG + ".imagenet_codebase.networks.sr_static")
    torch.manual_seed(seed)
    net = nets.OFAMobileNetS4(**KW)
    net.set_active_subnet(**setting)
    net = st.build_static_net(net.get_active_net_config())
    net.init_model("he_fout")
    os.makedirs(d)
    with open(os.path.join(d, "net_config.json"), "w") as f:
        json.dump(net.config, f)
    torch.save({"state_dict": {k: t.cpu() for k, t in net.state_dict().items()}}, os.path.join(d, "static_state_dict.pth"))
    return d


def bench_upscale(path, tmp, N, length):
    scenes = importlib.import_module(PKG + ".scenes")
    a = export(dict(ks=3, e=3, d=2, pixel_d=1), 4, os.path.join(tmp, "a"))
    b = export(dict(ks=3, e=3, d=2, pixel_d=0), 5, os.path.join(tmp, "b"))
    tool = [os.path.join(ROOT, "upscale_video_ofa_net_sr.py"), "--size", "1920x1080", "--mix-prec", "bf16", "--out",
            os.path.join(tmp, "out.yuv")]
    times = {}
    for frames in (N, 2 * N, N, 2 * N):
        m = scenes.SceneMap(video=path, frames=frames, first=0, width=W, height=H, depth=8, matrix="bt601", range="tv",
                            threshold=None, min_scene=1, distance=[0] * frames,
                            scenes=[dict(first=i, stop=min(i + length, frames), **({"static": b} if (i // length) % 2 else {}))
                                    for i in range(0, frames, length)])
        mp = os.path.join(tmp, "map%d.json" % frames)
        m.save(mp)
        for label, extra in (("one export a", ["--static", a]), ("one export b", ["--static", b]),
                             ("scene map a/b", ["--static", a, "--scene-map", mp])):
            line = run_tool(tool + extra + ["--frames", "0:%d" % frames, path])
            times[label, frames] = min(times.get((label, frames), 1e9), float(re.search(r"in ([0-9.]+) s", line).group(1)))
            say("%-14s %3d frames: %s" % (label, frames, line))
    for label in ("one export a", "one export b", "scene map a/b"):
        dt = times[label, 2 * N] - times[label, N]
        say("%-14s steady state (best of 2 runs each): %.2f frames/s (%d frames in %.3f s)" % (label, N / dt, N, dt))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--upscale-frames", type=int, default=64)
    ap.add_argument("--scene-length", type=int, default=8)
    ap.add_argument("--skip-upscale", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("the measurements run on the GPU")
    bench_kernels(a.rounds)
    tmp = tempfile.mkdtemp()
    try:
        path = os.path.join(tmp, "clip_1920x1080.yuv")
        write_clip(path, max(a.frames, 2 * a.upscale_frames))
        bench_tool(path, a.rounds)
        if not a.skip_upscale:
            bench_upscale(path, tmp, a.upscale_frames, a.scene_length)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
