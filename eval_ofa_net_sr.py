#!/usr/bin/env python3
"""Sampled sub-network evaluation -- counterpart of the reference's eval_ofa_net_sr.py (:187-220,247-251): build
OFAMobileNetS4(k7,e6,d4,pd2), load a checkpoint, fix a sub-network and report (loss, Y-PSNR) on the test loader
(BASELINE config 5; full-resolution images, sides multiples of 4).  Images of equal size are batched together
(--batched, the default: SRRunManager.validate_batched; per-image loss / PSNR, identical to the batch-1 pass) and the
pass is timed: images/s of the evaluation, after one untimed warm-up pass.  --degrade-blur S / --degrade-noise V score
on LR inputs under one fixed degradation (degrade.py; stream = the image's running index), made on the GPU."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"


STATIC_WEIGHTS = "static_state_dict.pth"


def input_key(upscale):
    """the data provider's LR image for an upscale factor (ask the net, not pixel_d)"""
    return "%dx_down_image" % upscale


def load_checkpoint_weights(fname, ema=False):
    """the state dict a checkpoint reader loads: checkpoint["state_dict"], or with `ema` (--ema) the averaged parameters
    of a run with --ema-decay laid over it (ema.averaged_state_dict: a checkpoint without them is refused)"""
    import torch
    checkpoint = torch.load(fname, map_location="cpu", weights_only=True)
    if not ema:
        return checkpoint["state_dict"]
    return importlib.import_module(PKG + ".ema").averaged_state_dict(checkpoint, fname)


def export_static(supernet, out_dir, ema=False):
    """the supernet's active sub-network as a static network: out_dir/net_config.json + its state dict.  `ema`: the
    supernet holds averaged weights (--ema); net_config.json then records "ema": true"""
    import json
    import torch
    os.makedirs(out_dir, exist_ok=True)
    sub = supernet.get_active_subnet(preserve_weight=True)
    with open(os.path.join(out_dir, "net_config.json"), "w") as f:
        json.dump(dict(sub.config, ema=True) if ema else sub.config, f, indent=1)
    torch.save({"state_dict": sub.state_dict()}, os.path.join(out_dir, STATIC_WEIGHTS))
    return sub


def load_static(in_dir):
    """the static network export_static() wrote (on the CPU; the run manager moves it)"""
    import json
    import torch
    st = importlib.import_module(PKG + ".imagenet_codebase.networks.sr_static")
    with open(os.path.join(in_dir, "net_config.json")) as f:
        net = st.build_static_net(json.load(f))
    net.load_state_dict(torch.load(os.path.join(in_dir, STATIC_WEIGHTS), map_location="cpu", weights_only=True)["state_dict"])
    return net


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--ema", action="store_true", help="with --checkpoint: load the averaged weights of a run with "
                                                       "--ema-decay (the checkpoint's \"ema\" entry) instead of the raw ones")
    ap.add_argument("--path", default="exp/sr/eval")
    ap.add_argument("--ks", type=int, default=7)
    ap.add_argument("--expand", type=int, default=6)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--pixelshuffle-depth", type=int, default=2)
    ap.add_argument("--mix-prec", default="f32", choices=["f32", "bf16", "f16"])
    ap.add_argument("--synthetic", action="store_true", help="evaluate on synthetic Set14-sized images when the "
                                                             "dataset directory is absent")
    ap.add_argument("--batch1", action="store_true", help="the reference's batch-1 pass instead of size buckets")
    ap.add_argument("--export", default=None, metavar="DIR",
                    help="also write the selected sub-network as a static network: DIR/net_config.json + DIR/%s" % STATIC_WEIGHTS)
    ap.add_argument("--static", default=None, metavar="DIR", help="evaluate the static network exported to DIR "
                                                                  "(instead of a supernet sub-network)")
    ap.add_argument("--test-sizes", default=None, help="synthetic test HR sizes instead of the Set14-like ones, e.g. 64x64,48x80")
    ap.add_argument("--ssim", action="store_true", help="also report Y-SSIM (and the exact-luma Y-PSNR), scored on the GPU "
                                                        "by the HIP metric kernel (SRRunManager.validate_quality)")
    ap.add_argument("--shave", type=int, default=0, help="with --ssim / --self-ensemble: border pixels left out of the metric")
    ap.add_argument("--self-ensemble", type=int, default=1, choices=[1, 2, 4, 8], metavar="K",
                    help="with --static: also score the geometric self-ensemble, the fp32 mean of the outputs under the "
                         "first K of the 8 flips / transposes (2: + horizontal flip, 4: + vertical flips, 8: + transposes)")
    ap.add_argument("--degrade-blur", type=float, default=None, metavar="S",
                    help="score on degraded LR inputs (degrade.py): every test image blurred with sigma_x = sigma_y = S HR "
                         "pixels before the down-sampling")
    ap.add_argument("--degrade-noise", type=float, default=None, metavar="V",
                    help="score on degraded LR inputs: noise of sigma V 8-bit levels after the down-sampling, a stream per "
                         "image (its running index)")
    ap.add_argument("--degrade-seed", type=int, default=0, metavar="N", help="the seed of the noise generator (default 0)")
    vf = importlib.import_module(PKG + ".imagenet_codebase.data_providers.video_frames")
    vf.add_video_args(ap)
    a = ap.parse_args(argv)
    if a.ema and not a.checkpoint:
        ap.error("--ema needs --checkpoint FILE (the averaged weights live in a training checkpoint's \"ema\" entry)")
    if a.ema and a.static:
        ap.error("--ema with --static: an exported network holds one set of weights (its net_config.json says which)")
    video_kw = vf.take_video_args(a)        # --video: evaluate on the evaluation frames of raw YUV 4:2:0 video
    weights = None
    if a.ema:                               # refused here, before anything is set up, when the file has no average
        try:
            weights = load_checkpoint_weights(a.checkpoint, ema=True)
        except ValueError as e:
            ap.error("--ema: %s" % e)
    degrade = None
    if a.degrade_blur is not None or a.degrade_noise is not None:
        dg = importlib.import_module(PKG + ".degrade")
        try:
            dg.blur_radius(a.degrade_blur or 0.0)
        except ValueError as e:
            ap.error("--degrade-blur: %s" % e)
        try:
            dg.noise_amplitude(a.degrade_noise or 0.0)
        except ValueError as e:
            ap.error("--degrade-noise: %s" % e)
        if video_kw and video_kw.get("videos_lr"):
            ap.error("--degrade-blur / --degrade-noise with --video-lr: the LR inputs of paired video are the decoded LR "
                     "stream's, there is no bicubic to degrade")
        degrade = (a.degrade_blur or 0.0, a.degrade_noise or 0.0, a.degrade_seed)
    elif a.degrade_seed != 0:
        ap.error("--degrade-seed needs --degrade-blur S or --degrade-noise V")
    dkw = {} if degrade is None else {"degrade": degrade}      # without the options every call is what it was
    if a.self_ensemble != 1 and not a.static:
        ap.error("--self-ensemble needs an exported static network (--static DIR)")
    import torch
    rm = importlib.import_module(PKG + ".imagenet_codebase.run_manager")
    nets = importlib.import_module(PKG + ".elastic_nn.networks")
    dop = importlib.import_module(PKG + ".elastic_nn.modules.dynamic_op")
    dop.DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    if a.static:
        net = load_static(a.static)
    else:
        net = nets.OFAMobileNetS4(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4],
                                  pixelshuffle_depth_list=[1, 2])
    # Set14-like sizes (HR sides multiples of 4)
    sizes = [(480, 500), (576, 720), (512, 512), (288, 352), (360, 248), (276, 276), (360, 500), (288, 352),
             (512, 512), (512, 512), (512, 768), (512, 512), (656, 528), (388, 584)]
    if a.test_sizes:
        sizes = [tuple(int(v) for v in s.split("x")) for s in a.test_sizes.split(",")]
    kw = dict(n_epochs=1, init_lr=1e-3, opt_type="adam", no_decay_keys="bn#bias", label_smoothing=0.0,
              train_batch_size=1, test_batch_size=1)
    if video_kw:
        cfg = rm.VideoFramesRunConfig(image_size=32, **dict(kw, **video_kw))
    else:
        cfg = rm.Div2K_SetXXRunConfig(image_size=256, test_sizes=sizes, n_train_batches=1,
                                      allow_synthetic=True if a.synthetic else None,
                                      **({} if degrade is None else {"lr_on_device": True}), **kw)
    mgr = rm.SRRunManager(a.path, net, cfg, init=a.checkpoint is None and not a.static, mix_prec=a.mix_prec, num_gpus=1)
    if a.static:
        key = input_key(net.upscale)
    else:
        if a.checkpoint:
            net.load_weights_from_net(load_checkpoint_weights(a.checkpoint) if weights is None else weights)
        net.set_active_subnet(ks=a.ks, e=a.expand, d=a.depth, pixel_d=a.pixelshuffle_depth)
        key = "4x_down_image" if a.pixelshuffle_depth == 2 or net.COMPAT_REFERENCE_INDEXING else "2x_down_image"
        if a.export:
            export_static(net, a.export, ema=a.ema)
    import time
    if degrade is not None:
        print("degraded LR inputs: blur sigma %g, noise sigma %g, seed %d" % degrade)
    n_img = len(cfg.test_loader) if video_kw else sum(b["image" if degrade is None else "image_u8"].shape[0]
                                                       for b in cfg.test_loader)

    def run():
        if a.batch1:
            return mgr.validate(is_test=True, input_key=key, **dkw) + (n_img,)
        return mgr.validate_batched(is_test=True, input_key=key, **dkw)

    run()                                   # warm-up (allocator, MIOpen find for the vendor-path convs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, psnr, calls = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("loss %.5f  Y-PSNR %.3f dB  (%d images in %d forward calls, %.1f images/s)" % (loss, psnr, n_img, calls,
                                                                                       n_img / dt))
    q = None
    if a.ssim:
        q = mgr.validate_quality(is_test=True, input_key=key, shave=a.shave, **dkw)
        print("Y-SSIM %.4f  Y-PSNR %.3f dB  (exact luma, shave %d, scored on the GPU)" % (q["ssim"], q["psnr"], a.shave))
    if a.self_ensemble != 1:
        q = mgr.validate_quality(is_test=True, input_key=key, shave=a.shave, self_ensemble=a.self_ensemble, **dkw)
        print("self-ensemble x%d: Y-SSIM %.4f  Y-PSNR %.3f dB  loss %.5f  (exact luma, shave %d, %d forward calls)"
              % (a.self_ensemble, q["ssim"], q["psnr"], q["loss"], a.shave, q["calls"]))
    return q


if __name__ == "__main__":
    main()
