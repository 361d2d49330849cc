#!/usr/bin/env python3
"""Upscale your own images with an exported static SR network, tiled so that any image size works.

The network is a static SRNetS4 / SRNetX4 exported with `search_ofa_net_sr.py --export DIR` or
`eval_ofa_net_sr.py --export DIR` (DIR/net_config.json + DIR/static_state_dict.pth); a supernet checkpoint is not loaded
here: export its sub-network first.  Inputs are image files or directories of them; grayscale and RGBA images become RGB
(unless --keep-mode, below), and every output is written as OUTDIR/<name>.png.  The next image is decoded (and the
previous one encoded) on a small host thread pool while the GPU upscales the current one.  Prints output megapixels per
second at the end.
--reference DIR scores every output against the equally named ground-truth image in DIR on the GPU (Y-PSNR and Y-SSIM by
the HIP metric kernel, --shave border pixels left out), prints the numbers and writes them to OUTDIR/quality.json.
--out-size WxH writes every output at that size instead of the network's own: any size from the input's up to the
network's, each axis on its own.  The result equals Pillow's Image.resize (--resample lanczos, the default, or bicubic) of
the full-size output bit for bit and is computed inside the scatter kernel; the full-size image never exists.  It applies to
every input: an input that the size does not fit is refused by name.  --reference then compares at the target size.
--easy-static DIR --easy-threshold T route every window by its content: a window whose mean absolute difference of
neighbouring luma samples (L = (77 R + 150 G + 29 B + 128) >> 8, in 8-bit levels) is at most T runs the cheaper export in
DIR, every other window the --static network; both need the same upscale factor and share one tile plan.  There is no
blending: neighbouring cores from different networks can differ at the seam.  --route-report prints per image the easy and
hard window counts and the min / median / max of the per-window measure (what to look at when choosing T) and, with
--reference, writes the counts into quality.json.  Routing needs the tiled path: it is refused with --whole.
--keep-mode writes every output in its input's mode instead of RGB: RGB, RGBA, L (greyscale) and LA files keep theirs, 1-bit
files become L, paletted files with transparency and every file with a tRNS chunk become RGBA, paletted files without
become RGB, and everything else (CMYK, 16-bit, float, YCbCr ...) becomes RGB as without the flag.  The network still sees
RGB (R = G = B for greyscale; the colour under transparent pixels as it is, neither premultiplied nor bled), the RGB it
returns is what the other options and --reference see, and a greyscale output is Pillow's convert("L") of it.  The alpha
channel does not go through the network: it is the file's alpha resized straight to the output's size as Pillow's
Image.resize does it, bit for bit (--alpha-resample bicubic, the default, or lanczos).  8 bits per channel."""
import argparse
import collections
import concurrent.futures
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"

EXTS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp", ".ppm", ".pgm")
WORKERS = 4   # host decode / encode threads


def parse_out_size(text):
    try:
        return importlib.import_module(PKG + ".resize").parse_size(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0], epilog=__doc__.split("\n\n", 1)[1],
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--static", required=True, metavar="DIR",
                    help="exported static network (search_ofa_net_sr.py / eval_ofa_net_sr.py --export DIR)")
    ap.add_argument("--out", required=True, metavar="OUTDIR", help="output directory (PNG files)")
    ap.add_argument("--mix-prec", default="f32", choices=["f32", "bf16", "f16"], help="activation precision")
    ap.add_argument("--core", type=int, default=None,
                    help="core tile side in input pixels (default: the largest that keeps every activation < 2 GiB)")
    ap.add_argument("--batch", type=int, default=None, help="windows per forward call (default: as many as fit)")
    ap.add_argument("--whole", action="store_true", help="run each image as one forward call (small images only)")
    ap.add_argument("--self-ensemble", type=int, default=1, choices=[1, 2, 4, 8], metavar="K",
                    help="geometric self-ensemble: average the outputs under the first K of the 8 flips / transposes "
                         "(K times the network time; 2: + horizontal flip, 4: + vertical flips, 8: + transposes)")
    ap.add_argument("--out-size", type=parse_out_size, default=None, metavar="WxH",
                    help="output size of every image (default: the network's own): from the input's size up to the network's")
    ap.add_argument("--resample", default="lanczos", choices=["bicubic", "lanczos"], help="the filter of --out-size")
    ap.add_argument("--easy-static", default=None, metavar="DIR",
                    help="a cheaper exported network of the same upscale factor for flat windows (needs --easy-threshold)")
    ap.add_argument("--easy-threshold", default=None, metavar="T",
                    help="a window is easy when its mean absolute luma difference, in 8-bit levels, is at most T")
    ap.add_argument("--route-report", action="store_true", help="per image: easy / hard windows and the activity")
    ap.add_argument("--keep-mode", action="store_true",
                    help="write RGBA, L and LA inputs (and paletted ones with transparency, as RGBA) in their own mode")
    ap.add_argument("--alpha-resample", default=None, choices=["bicubic", "lanczos"],
                    help="with --keep-mode: the filter that brings the alpha channel to the output's size (default: bicubic)")
    ap.add_argument("--reference", default=None, metavar="PATH",
                    help="directory of ground-truth HR images named as the inputs: report Y-PSNR / Y-SSIM per image")
    ap.add_argument("--shave", type=int, default=0, help="with --reference: border pixels left out of the metric")
    ap.add_argument("inputs", nargs="+", metavar="INPUT", help="image files or directories")
    a = ap.parse_args(argv)
    if (a.easy_static is None) != (a.easy_threshold is None):
        ap.error("--easy-static and --easy-threshold need each other")
    if a.route_report and a.easy_static is None:
        ap.error("--route-report needs --easy-static and --easy-threshold")
    if a.easy_static is not None and a.whole:
        ap.error("--whole runs one window per image: there is nothing to route")
    if a.alpha_resample is not None and not a.keep_mode:
        ap.error("--alpha-resample needs --keep-mode")
    if a.easy_threshold is not None:
        try:
            importlib.import_module(PKG + ".routing").activity_limit(a.easy_threshold, 1, 2)
        except ValueError as e:
            ap.error("--easy-threshold: %s" % e)
    return a


def list_inputs(inputs):
    files = []
    for p in inputs:
        if os.path.isdir(p):
            files += sorted(os.path.join(p, f) for f in os.listdir(p) if f.lower().endswith(EXTS))
        elif os.path.isfile(p):
            files.append(p)
        else:
            raise SystemExit("no such input: %s" % p)
    return files


def decode(path):
    """HWC uint8 RGB numpy array"""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))


def decode_keep(path):
    """HWC uint8 numpy array in the mode --keep-mode keeps for the file: [H, W, 1] L, [H, W, 2] LA, [H, W, 3] RGB or
    [H, W, 4] RGBA"""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        if "transparency" in im.info or im.mode == "PA":
            im = im.convert("RGBA")
        elif im.mode == "1":
            im = im.convert("L")
        elif im.mode not in ("RGB", "RGBA", "L", "LA"):
            im = im.convert("RGB")
        arr = np.array(im, dtype=np.uint8)
    return np.ascontiguousarray(arr if arr.ndim == 3 else arr[:, :, None])


def encode(arr, path):
    from PIL import Image
    Image.fromarray(arr, "RGB").save(path, format="PNG")
    return path


def encode_keep(arr, path):
    """[H, W, C] uint8 -> a PNG of mode L, LA, RGB or RGBA by C"""
    from PIL import Image
    mode = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[arr.shape[2]]
    Image.fromarray(arr[:, :, 0] if mode == "L" else arr, mode).save(path, format="PNG")
    return path


def out_path(out_dir, path, taken):
    name = os.path.splitext(os.path.basename(path))[0]
    p = os.path.join(out_dir, name + ".png")
    i = 1
    while p in taken:
        p = os.path.join(out_dir, "%s_%d.png" % (name, i))
        i += 1
    taken.add(p)
    return p


def reference_path(ref_dir, path):
    """the ground-truth image of input `path`: the file of the same stem in ref_dir"""
    stem = os.path.splitext(os.path.basename(path))[0]
    for ext in (os.path.splitext(path)[1],) + EXTS:
        p = os.path.join(ref_dir, stem + ext)
        if os.path.isfile(p):
            return p
    raise SystemExit("no reference image for %s in %s" % (path, ref_dir))


def main(argv=None):
    a = parse_args(argv)
    files = list_inputs(a.inputs)
    if not files:
        raise SystemExit("no input images")
    import torch
    evals = importlib.import_module("eval_ofa_net_sr")
    upscale = importlib.import_module(PKG + ".upscale")
    if not torch.cuda.is_available():
        raise SystemExit("upscaling runs on the GPU")
    net = evals.load_static(a.static).cuda()
    easy = None if a.easy_static is None else evals.load_static(a.easy_static).cuda()
    try:
        up = upscale.TiledUpscaler(net, core=a.core, batch=a.batch, mix_prec=a.mix_prec, self_ensemble=a.self_ensemble,
                                   easy_net=easy, easy_threshold=a.easy_threshold)
    except ValueError as e:
        if easy is None:
            raise
        raise SystemExit("--easy-static: %s" % e)
    os.makedirs(a.out, exist_ok=True)
    print("%s x%d: receptive radius %d px, halo %d, core %d, %s%s" % (
        net.name(), up.scale, up.radius, up.halo, up.core, a.mix_prec,
        "" if a.self_ensemble == 1 else ", self-ensemble x%d" % a.self_ensemble))
    if easy is not None:
        print("routing: windows of mean luma activity <= %s run %s (receptive radius %d px)"
              % (a.easy_threshold, easy.name(), upscale.receptive_radius(easy.config)))
    routes = []
    taken = set()
    mpix = 0.0
    saves = []
    scores = []
    if a.reference is not None:
        utils = importlib.import_module(PKG + ".utils")
        if not os.path.isdir(a.reference):
            raise SystemExit("--reference %s is not a directory" % a.reference)
        refs = [reference_path(a.reference, f) for f in files]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(WORKERS, len(files) + 1)) as pool:
        dec = decode_keep if a.keep_mode else decode
        pending = collections.deque(pool.submit(dec, f) for f in files[:2])
        t0 = time.perf_counter()
        for i, f in enumerate(files):
            img = pending.popleft().result()
            if i + 2 < len(files):
                pending.append(pool.submit(dec, files[i + 2]))
            out_size = None if a.out_size is None else (a.out_size[1], a.out_size[0])
            src = torch.from_numpy(img)
            if a.keep_mode:                 # everything up to the join below sees the RGB image, as without the flag
                src, channels, alpha = up.split_image(src)
            try:
                plan = None if a.whole else up.plan(img.shape[0], img.shape[1], out_size, a.resample)
                out_gpu = up.upscale(src, whole=a.whole, out_size=out_size, resample=a.resample)
            except ValueError as e:
                if a.out_size is None:
                    raise
                raise SystemExit("%s: %s" % (f, e))
            if easy is not None:
                routes.append({k: up.route_stats[k] for k in ("windows", "easy", "hard")})
                if a.route_report:
                    act = up.window_activity(src, out_size, a.resample)
                    print("%s: easy %d hard %d of %d windows; activity min %.3f median %.3f max %.3f" % (
                        f, routes[-1]["easy"], routes[-1]["hard"], routes[-1]["windows"], float(act.min()),
                        float(act.median()), float(act.max())))
            if a.reference is not None:
                ref = decode(refs[i])
                if ref.shape != tuple(out_gpu.shape):
                    raise SystemExit("%s is %dx%d, the upscaled %s is %dx%d: the reference must have the output's size"
                                     % (refs[i], ref.shape[1], ref.shape[0], f, out_gpu.shape[1], out_gpu.shape[0]))
                if min(ref.shape[:2]) - 2 * a.shave < 11 or a.shave < 0:
                    raise SystemExit("%s: a %dx%d image shaved by %d has a side below the 11-pixel SSIM window"
                                     % (refs[i], ref.shape[1], ref.shape[0], a.shave))
                scores.append((f, refs[i], utils.quality_y_device(out_gpu, torch.from_numpy(ref).to(out_gpu.device),
                                                                  a.shave)))
            if a.keep_mode:
                out_gpu = up.join_image(out_gpu, channels, alpha, img.shape[:2], a.alpha_resample or "bicubic")
            out = out_gpu.cpu().numpy()
            dst = out_path(a.out, f, taken)
            saves.append(pool.submit(encode_keep if a.keep_mode else encode, out, dst))
            mpix += out.shape[0] * out.shape[1] / 1e6
            print("%s: %dx%d -> %dx%d%s" % (f, img.shape[1], img.shape[0], out.shape[1], out.shape[0],
                                           "" if plan is None else "  (%d windows of %dx%d, %.2fx halo overhead)"
                                           % (len(plan), plan.win_w, plan.win_h, plan.overhead())))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        for s in saves:
            s.result()
    dt_all = time.perf_counter() - t0
    if a.reference is not None:
        import json
        recs = []
        for i, (f, r, q) in enumerate(scores):
            recs.append({"input": f, "reference": r, "psnr": q.psnr()[0], "ssim": q.ssim_list()[0], "sse": q.sse_list()[0],
                         "count": q.count})
            if a.route_report:
                recs[-1]["route"] = routes[i]
            print("%s: Y-PSNR %.3f dB  Y-SSIM %.4f" % (f, recs[-1]["psnr"], recs[-1]["ssim"]))
        mean = {"psnr": sum(x["psnr"] for x in recs) / len(recs), "ssim": sum(x["ssim"] for x in recs) / len(recs)}
        print("mean of %d images: Y-PSNR %.3f dB  Y-SSIM %.4f  (shave %d)" % (len(recs), mean["psnr"], mean["ssim"], a.shave))
        with open(os.path.join(a.out, "quality.json"), "w") as fh:
            json.dump({"shave": a.shave, "self_ensemble": a.self_ensemble, "images": recs, "mean": mean}, fh, indent=1)
    print("%d images, %.2f output MP in %.3f s: %.2f MP/s (%.2f MP/s with PNG encoding)" % (
        len(files), mpix, dt, mpix / dt, mpix / dt_all))


if __name__ == "__main__":
    main()
