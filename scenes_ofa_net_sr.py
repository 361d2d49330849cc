#!/usr/bin/env python3
"""Find the scene cuts of a raw 8-bit or 10-bit YUV 4:2:0 video (Y4M, or headerless yuv420p with --size) on the GPU.

The measure is the squared difference of the per-channel colour histograms of consecutive frames (scenes.py: an exact
integer function of the frames' bytes).  Every frame is read into a pinned host buffer on a worker thread, uploaded, and
its histogram is counted by a HIP kernel that decodes the planar frame as it reads it (csrc/scene.hip): no RGB frame
exists on the host or on the GPU, and nothing is copied back until the end.
Printed: the min / median / max of the normalised distance d / (6 P^2), P the pixels of a frame, and the --top K largest
with their frame numbers -- what to look at when choosing --threshold T.  With --threshold, frame i starts a new scene
iff its normalised distance exceeds T and the current scene has at least --min-scene frames; each scene is printed as
first:stop, which is what --video-frames of the training scripts and --frames of the upscaler take, and --out FILE holds
the scene map that `upscale_video_ofa_net_sr.py --scene-map` and `--video-scene FILE:K` read.  Without --threshold the
file holds the distances only: no default threshold is built in.  Frame numbers are absolute in the file, whatever
--frames selects.  An untagged file means bt601 / limited range; --matrix / --range must be the ones the video is later
decoded with.  --no-kernel reads and uploads the frames and launches nothing: the reader's own frames/s, to compare with.
There is no handling of fades, dissolves or flashes and no motion estimate: one fixed threshold and a minimum scene
length."""
import argparse
import concurrent.futures
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"
SLOTS = 2   # pinned frame buffers


def parse_size(text):
    try:
        w, h = text.lower().split("x")
        return int(w), int(h)
    except ValueError:
        raise argparse.ArgumentTypeError("expected WxH, got %r" % text)


def parse_frames(text):
    try:
        a, b = text.split(":")
        a, b = (int(a) if a else 0), (int(b) if b else None)
    except ValueError:
        raise argparse.ArgumentTypeError("expected A:B, got %r" % text)
    if a < 0 or (b is not None and b < a):
        raise argparse.ArgumentTypeError("empty or negative frame range %r" % text)
    return a, b


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0], epilog=__doc__.split("\n\n", 1)[1],
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=parse_size, default=None, metavar="WxH", help="frame size of a headerless input")
    ap.add_argument("--depth", type=int, default=None, choices=[8, 10],
                    help="bits per sample of a headerless input (default 8); a Y4M input says it itself")
    ap.add_argument("--matrix", default="bt601", choices=["bt601", "bt709"])
    ap.add_argument("--range", default="tv", choices=["tv", "pc"], help="tv: limited (16..235), pc: full range")
    ap.add_argument("--frames", type=parse_frames, default=(0, None), metavar="A:B", help="frames A .. B-1 only")
    ap.add_argument("--threshold", default=None, metavar="T",
                    help="a frame whose normalised distance to its predecessor exceeds T (0 .. 1) starts a scene")
    ap.add_argument("--min-scene", type=int, default=1, metavar="N", help="a scene has at least N frames (default 1)")
    ap.add_argument("--out", default=None, metavar="FILE", help="write the scene map (JSON) here")
    ap.add_argument("--top", type=int, default=10, metavar="K", help="print the K largest distances (default 10)")
    ap.add_argument("--no-kernel", action="store_true",
                    help="read and upload the frames only (the reader's own frames/s, for comparison)")
    ap.add_argument("input", metavar="INPUT", help="*.y4m, or a headerless yuv420p file (then --size is required)")
    a = ap.parse_args(argv)
    if a.min_scene < 1:
        ap.error("--min-scene must be >= 1")
    if a.top < 0:
        ap.error("--top must be >= 0")
    if a.threshold is not None:
        try:
            importlib.import_module(PKG + ".scenes").distance_limit(a.threshold, 4)
        except ValueError as e:
            ap.error("--threshold: %s" % e)
    return a


def main(argv=None):
    a = parse_args(argv)
    import numpy as np
    import torch
    video = importlib.import_module(PKG + ".video")
    scenes = importlib.import_module(PKG + ".scenes")
    if not torch.cuda.is_available():
        raise SystemExit("the histograms are counted on the GPU")
    try:
        reader = video.open_reader(a.input, a.size, a.depth)
    except ValueError as e:
        raise SystemExit(str(e))
    W, H, depth = reader.width, reader.height, reader.depth
    try:
        det = scenes.SceneDetector(H, W, depth, a.matrix, a.range == "pc", "cuda:0")
    except ValueError as e:
        raise SystemExit(str(e))
    P = det.P
    first, stop = a.frames
    for _ in range(first):
        if not reader.skip_frame():
            raise SystemExit("%s has fewer than %d frames" % (a.input, first))
    n_in = video.frame_bytes(W, H, depth)
    pin_in = [torch.empty(n_in, dtype=torch.uint8).pin_memory() for _ in range(SLOTS)]
    dev_in = [torch.empty(n_in, dtype=torch.uint8, device="cuda:0") for _ in range(SLOTS)]

    def read(slot):
        return reader.read_frame(pin_in[slot].numpy()) is not None

    done = 0
    want = None if stop is None else stop - first
    with concurrent.futures.ThreadPoolExecutor(1) as rd:
        t0 = time.perf_counter()
        nxt = rd.submit(read, 0) if want != 0 else None
        while nxt is not None:
            if not nxt.result():
                break
            slot = done % SLOTS
            # the kernels of the frame before last have read dev_in[slot] once this frame's copy, queued behind them on
            # the one stream, runs; the synchronisation frees the pinned slot, as in the upscaler
            dev_in[slot].copy_(pin_in[slot], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            nxt = rd.submit(read, (done + 1) % SLOTS) if want is None or done + 1 < want else None
            if not a.no_kernel:
                det.push(*video.split_frame(dev_in[slot], W, H, depth))
            done += 1
        d = det.distances()
        dt = time.perf_counter() - t0
    reader.close()
    if want is not None and done < want:
        raise SystemExit("%s ended after %d of the %d frames asked for" % (a.input, done, want))
    if done == 0:
        raise SystemExit("no frames")
    print("%s: %dx%d, %d bits, %s %s, frames %d:%d" % (a.input, W, H, depth, a.matrix, a.range, first, first + done))
    print("%d frames in %.3f s: %.2f frames/s, %.2f input MP/s" % (done, dt, done / dt, done * P / 1e6 / dt))
    if a.no_kernel:
        return
    norm = scenes.normalised(d, P)
    pairs = norm[1:]
    if len(pairs):
        print("normalised distance of %d frame pairs: min %.6g median %.6g max %.6g"
              % (len(pairs), pairs.min(), float(np.median(pairs)), pairs.max()))
        order = sorted(range(1, done), key=lambda i: (-d[i], i))[:a.top]
        for i in order:
            print("frame %d: %.6g" % (first + i, norm[i]))
    found = []
    if a.threshold is not None:
        limit = scenes.distance_limit(a.threshold, P)
        found = [(first + s0, first + s1) for s0, s1 in scenes.cuts(d, limit, a.min_scene)]
        print("%d scene%s at threshold %s, at least %d frame%s each:" % (
            len(found), "" if len(found) == 1 else "s", a.threshold, a.min_scene, "" if a.min_scene == 1 else "s"))
        for s0, s1 in found:
            print("%d:%d" % (s0, s1))
    if a.out is not None:
        m = scenes.SceneMap(video=a.input, frames=done, first=first, width=W, height=H, depth=depth, matrix=a.matrix,
                            range=a.range, threshold=a.threshold, min_scene=a.min_scene, distance=d,
                            scenes=[{"first": s0, "stop": s1} for s0, s1 in found])
        m.save(a.out)
        print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
