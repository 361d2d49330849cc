#!/usr/bin/env python3
"""Sub-network search (Once-for-All's second step): evolutionary search of an OFA-SR supernet for the arch with the best
fp32 Y-PSNR under a budget of GMACs or of milliseconds on this GPU.  Every candidate is re-calibrated on --calib-images
training images (elastic_nn.utils.recalibrate_bn, the HIP re-calibration kernels) and validated on the test loader.
--export DIR re-calibrates the winner and writes it as a static network (eval_ofa_net_sr.py's export_static) plus
DIR/search.json: the history, the final arch, its PSNR, MACs, predicted and measured ms.  `eval_ofa_net_sr.py --static
DIR` reports the same PSNR for the export."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "ofa-for-super-resolution_amd"

TEST_SIZES = [(480, 500), (576, 720), (512, 512), (288, 352), (360, 248), (276, 276), (360, 500), (288, 352),
              (512, 512), (512, 512), (512, 768), (512, 512), (656, 528), (388, 584)]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--net", default="s4", choices=["s4", "x4"])
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--ema", action="store_true", help="with --checkpoint: search and export the averaged weights of a run "
                                                       "with --ema-decay (the checkpoint's \"ema\" entry)")
    ap.add_argument("--path", default="exp/sr/search")
    ap.add_argument("--upscale", type=int, default=4, help="LR -> HR factor of every candidate (s4)")
    budget = ap.add_mutually_exclusive_group(required=True)
    budget.add_argument("--budget-gmacs", type=float, default=None, help="GMACs per LR image of --lr-size")
    budget.add_argument("--budget-ms", type=float, default=None, help="predicted ms per batch (--lat-table)")
    ap.add_argument("--lat-table", default=None, metavar="PATH", help="latency table JSON (built there when absent)")
    ap.add_argument("--lr-size", type=int, nargs=2, default=[64, 64], metavar=("H", "W"),
                    help="input size the MACs and the latency table are taken at")
    ap.add_argument("--lat-batch", type=int, default=1)
    ap.add_argument("--calib-images", type=int, default=256)
    ap.add_argument("--calib-batch", type=int, default=16)
    ap.add_argument("--population", type=int, default=100)
    ap.add_argument("--generations", type=int, default=500)
    ap.add_argument("--parent-ratio", type=float, default=0.25)
    ap.add_argument("--mutation-ratio", type=float, default=0.5)
    ap.add_argument("--mutate-prob", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--synthetic", action="store_true", help="synthetic images when the dataset directory is absent")
    ap.add_argument("--image-size", type=int, default=256, help="HR training patch size of the calibration images")
    ap.add_argument("--test-sizes", default=None, help="synthetic validation HR sizes, e.g. 64x64,48x80")
    ap.add_argument("--export", default=None, metavar="DIR")
    ap.add_argument("--fitness", default="psnr", choices=["psnr", "ssim", "psnr-gpu"],
                    help="what a candidate is scored by: psnr = the host Y-PSNR (the default), psnr-gpu / ssim = Y-PSNR / "
                         "Y-SSIM by the HIP metric kernel (search.quality_fitness)")
    ap.add_argument("--shave", type=int, default=0, help="border pixels the GPU metric leaves out")
    vf = importlib.import_module(PKG + ".imagenet_codebase.data_providers.video_frames")
    vf.add_video_args(ap)
    a = ap.parse_args(argv)
    if a.ema and not a.checkpoint:
        ap.error("--ema needs --checkpoint FILE (the averaged weights live in a training checkpoint's \"ema\" entry)")
    a.video_kw = vf.take_video_args(a)      # --video: calibrate and validate on the frames of raw YUV 4:2:0 video
    a.weights = None
    if a.ema:                               # refused here, before anything is set up, when the file has no average
        import eval_ofa_net_sr as ev
        try:
            a.weights = ev.load_checkpoint_weights(a.checkpoint, ema=True)
        except ValueError as e:
            ap.error("--ema: %s" % e)
    vf.refuse_pair_for_hr_input(a.video_kw, "image" if a.net == "x4" else None, "--net x4")
    if a.test_sizes:
        a.test_sizes = [tuple(int(v) for v in s.split("x")) for s in a.test_sizes.split(",")]
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    rm = importlib.import_module(PKG + ".imagenet_codebase.run_manager")
    nets = importlib.import_module(PKG + ".elastic_nn.networks")
    dop = importlib.import_module(PKG + ".elastic_nn.modules.dynamic_op")
    search = importlib.import_module(PKG + ".elastic_nn.search")
    eutils = importlib.import_module(PKG + ".elastic_nn.utils")
    import eval_ofa_net_sr as ev
    dop.DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    kw = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])
    net = nets.OFAMobileNetS4(**kw) if a.net == "s4" else nets.OFAMobileNetX4(**kw)
    n_batches = max(1, (a.calib_images + a.calib_batch - 1) // a.calib_batch)
    kw = dict(n_epochs=1, init_lr=1e-3, opt_type="adam", no_decay_keys="bn#bias", label_smoothing=0.0,
              train_batch_size=a.calib_batch, test_batch_size=1, image_size=a.image_size)
    if a.video_kw:
        cfg = rm.VideoFramesRunConfig(**dict(kw, **a.video_kw))
    else:
        cfg = rm.Div2K_SetXXRunConfig(test_sizes=a.test_sizes or TEST_SIZES, n_train_batches=n_batches,
                                      allow_synthetic=True if a.synthetic else None, **kw)
    mgr = rm.SRRunManager(a.path, net, cfg, init=a.checkpoint is None, mix_prec="f32", num_gpus=1)
    if a.checkpoint:
        net.load_weights_from_net(ev.load_checkpoint_weights(a.checkpoint) if a.weights is None else a.weights)
    net = mgr.net
    bn_before = search.bn_buffers(net)
    calib = cfg.data_provider.build_sub_train_loader(a.calib_images, a.calib_batch)
    space = search.ArchSpace(net, a.upscale)
    lr_hw = tuple(a.lr_size)
    table = None
    if a.budget_ms is not None or a.lat_table:
        if a.lat_table and os.path.exists(a.lat_table):
            table = search.LatencyTable.load(a.lat_table, space)
        else:
            table = search.LatencyTable(space, a.lat_batch, lr_hw[0], lr_hw[1]).build()
            if a.lat_table:
                table.save(a.lat_table)
    if a.budget_ms is not None:
        efficiency, budget = table.predict, a.budget_ms
    else:
        efficiency, budget = (lambda arch: space.macs(net, arch, lr_hw) / 1e9), a.budget_gmacs
    if a.fitness == "psnr":
        fitness = search.psnr_fitness(net, calib, cfg.test_loader, mgr, space, max_calib_batches=n_batches)
    else:
        fitness = search.quality_fitness(net, calib, cfg.test_loader, mgr, space, max_calib_batches=n_batches,
                                         metric="ssim" if a.fitness == "ssim" else "psnr", shave=a.shave)
    es = search.EvolutionSearch(space, fitness, efficiency, budget, a.population, a.generations, a.parent_ratio,
                                a.mutation_ratio, a.mutate_prob, seed=a.seed)
    best, history = es.run()
    score = es.cache[space.key(best)]
    gmacs = space.macs(net, best, lr_hw) / 1e9
    if a.fitness == "ssim":
        psnr = None
        print("best arch: %s\nY-SSIM %.4f  %.3f GMACs  (%d archs evaluated)" % (json.dumps(best), score, gmacs,
                                                                              len(es.evaluated)))
    else:
        psnr = score
        print("best arch: %s\nY-PSNR %.3f dB  %.3f GMACs  (%d archs evaluated)" % (json.dumps(best), psnr, gmacs,
                                                                                  len(es.evaluated)))
    if a.export:
        snap = search.bn_buffers(net)
        space.apply(net, best)
        eutils.recalibrate_bn(net, calib, input_key=search.lr_key(net), max_batches=n_batches)
        static = ev.export_static(net, a.export, ema=a.ema)
        quality = None
        if a.fitness != "psnr":      # the winner's numbers by the GPU metric, on the re-calibrated supernet path
            quality = mgr.validate_quality(net=net, data_loader=cfg.test_loader, input_key=search.lr_key(net), graphs=False,
                                           shave=a.shave)
            psnr = quality["psnr"]
        search.restore_bn_buffers(net, snap)
        result = {"arch": best, "psnr": psnr, "gmacs": gmacs, "lr_size": list(lr_hw),
                  "predicted_ms": table.predict(best) if table is not None else None,
                  "measured_ms": search.measure(static, a.lat_batch, lr_hw[0], lr_hw[1]) if table is not None else None,
                  "history": history, "evaluated": len(es.evaluated), "seed": a.seed, "budget": budget,
                  "budget_kind": "ms" if a.budget_ms is not None else "gmacs"}
        if quality is not None:
            result.update({"ssim": quality["ssim"], "fitness": a.fitness, "shave": a.shave})
        if a.ema:
            result["ema"] = True
        with open(os.path.join(a.export, "search.json"), "w") as f:
            json.dump(result, f, indent=1)
        print("exported to %s" % a.export)
    return {"best": best, "history": history, "psnr": psnr, "gmacs": gmacs, "net": net, "bn_before": bn_before,
            "manager": mgr, "search": es}


if __name__ == "__main__":
    main()
