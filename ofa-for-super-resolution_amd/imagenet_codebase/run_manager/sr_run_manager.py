"""RunConfig + SRRunManager: the trainer API of the SR path (mirror of reference
ofa/imagenet_codebase/run_manager/sr_run_manager.py:25-549), re-hosted for one process per GPU.

Differences that are deliberate (MI355X-first) and do not change results on one GPU:
  * multi-GPU is process-per-GPU data parallelism with ONE flat RCCL all-reduce per optimizer step
    (distributed.FlatGradReducer) instead of single-process nn.DataParallel (:197-198); `num_gpus` is
    accepted for signature compatibility, the world size comes from torch.distributed;
  * the PSNR logged during training is computed on the device with the reference's exact formula
    (utils.psnr_y_device) so there is no per-sub-step host sync (:496 -> .cpu() every step);
  * apex / tensorboardX hooks are not carried over (both absent; dead code in the reference).
Checkpoint files, dict keys, log files and the optimizer grouping are the reference's.
"""
import contextlib
import json
import math
import os
import time

import numpy as np
import torch
import torch.nn as nn

from ... import distributed as dd
from ... import ops
from ...graphed import GraphedEval
from ... import degrade as sr_degrade
from ... import ema as sr_ema
from ... import losses as sr_losses
from ...utils import (AverageMeter, bucket_by_size, device_batch, psnr_from_sse, psnr_y, psnr_y_device,
                      psnr_y_per_image)
from ..utils import get_net_info


class RunConfig(object):
    """reference :25-133"""

    def __init__(self, n_epochs, init_lr, lr_schedule_type, lr_schedule_param, dataset, train_batch_size,
                 test_batch_size, valid_size, opt_type, opt_param, weight_decay, label_smoothing, no_decay_keys,
                 mixup_alpha, model_init, validation_frequency, print_frequency, resident=False):
        self.n_epochs = n_epochs
        self.init_lr = init_lr
        self.lr_schedule_type = lr_schedule_type
        self.lr_schedule_param = lr_schedule_param
        self.dataset = dataset
        self.train_batch_size = train_batch_size
        self.test_batch_size = test_batch_size
        self.valid_size = valid_size
        self.opt_type = opt_type
        self.opt_param = opt_param
        self.weight_decay = weight_decay
        self.label_smoothing = label_smoothing
        self.no_decay_keys = no_decay_keys
        self.mixup_alpha = mixup_alpha
        self.model_init = model_init
        self.validation_frequency = validation_frequency
        self.print_frequency = print_frequency
        self.resident = bool(resident)   # DIV2K provider: training set resident on the GPU (data_providers/augment.py)

    @property
    def config(self):
        return {k: v for k, v in self.__dict__.items() if not k.startswith("_")}

    def copy(self):
        return RunConfig(**self.config)

    # -- learning rate (cosine over all iterations, linear warm-up) -- reference :62-90
    def calc_learning_rate(self, epoch, batch=0, nBatch=None):
        if self.lr_schedule_type == "cosine":
            total, cur = self.n_epochs * nBatch, epoch * nBatch + batch
            return 0.5 * self.init_lr * (1 + math.cos(math.pi * cur / total))
        if self.lr_schedule_type is None:
            return self.init_lr
        raise ValueError("do not support: %s" % self.lr_schedule_type)

    def adjust_learning_rate(self, optimizer, epoch, batch=0, nBatch=None):
        new_lr = self.calc_learning_rate(epoch, batch, nBatch)
        for group in optimizer.param_groups:
            group["lr"] = new_lr
        return new_lr

    def warmup_adjust_learning_rate(self, optimizer, T_total, nBatch, epoch, batch=0, warmup_lr=0):
        cur = epoch * nBatch + batch + 1
        new_lr = cur / T_total * (self.init_lr - warmup_lr) + warmup_lr
        for group in optimizer.param_groups:
            group["lr"] = new_lr
        return new_lr

    # -- data provider
    @property
    def data_provider(self):
        raise NotImplementedError

    @property
    def train_loader(self):
        return self.data_provider.train

    @property
    def valid_loader(self):
        return self.data_provider.valid

    @property
    def test_loader(self):
        return self.data_provider.test

    def random_sub_train_loader(self, n_images, batch_size, num_worker=None, num_replicas=None, rank=None):
        return self.data_provider.build_sub_train_loader(n_images, batch_size, num_worker, num_replicas, rank)

    # -- optimizer (reference :115-133; Adam ignores momentum / nesterov there too)
    def build_optimizer(self, net_params):
        if self.no_decay_keys is not None:
            assert isinstance(net_params, list) and len(net_params) == 2
            groups = [{"params": net_params[0], "weight_decay": self.weight_decay},
                      {"params": net_params[1], "weight_decay": 0}]
        else:
            groups = [{"params": net_params, "weight_decay": self.weight_decay}]
        if self.opt_type == "sgd":
            opt_param = self.opt_param or {}
            return torch.optim.SGD(groups, self.init_lr, momentum=opt_param.get("momentum", 0.9),
                                   nesterov=opt_param.get("nesterov", True))
        if self.opt_type == "adam":
            # same update rule as the reference's torch.optim.Adam(groups, lr); on the GPU torch's fused multi-tensor
            # implementation does it in 2 launches instead of ~20 (parameters without a gradient are skipped either way)
            groups = [dict(g, params=list(g["params"])) for g in groups]   # the reference passes generators
            plist = [p for g in groups for p in g["params"]]
            fused = bool(plist) and all(p.is_cuda for p in plist) and os.environ.get("OFASR_FUSED_ADAM", "1") != "0"
            return torch.optim.Adam(groups, self.init_lr, fused=True if fused else None)
        raise NotImplementedError


class SRRunManager(object):
    """reference :136-549.  attrs: net, network, optimizer, run_config, device, best_acc, start_epoch, path,
    train_criterion, test_criterion; plus `reducer` (None on one GPU) and `ema` (None without ema_decay)."""

    def __init__(self, path, net, run_config, init=True, measure_latency=None, no_gpu=False, mix_prec=None,
                 num_gpus=None, args=None, loss="reference", loss_eps=sr_losses.DEFAULT_EPS, loss_ssim=0.0,
                 ema_decay=0.0):
        if loss != "reference" and loss not in sr_losses.KINDS:
            raise ValueError("loss must be 'reference' or one of %s, got %r" % (", ".join(sr_losses.KINDS), loss))
        if not (loss_eps > 0 and math.isfinite(loss_eps)):
            raise ValueError("loss_eps must be positive, got %r" % (loss_eps,))
        self.loss = loss           # 'reference': nn.MSELoss through ATen, as ever; else the fused HIP loss (train_loss)
        self.loss_eps = float(loss_eps)
        if not (0.0 <= loss_ssim <= 1.0):
            raise ValueError("loss_ssim must lie in [0, 1], got %r" % (loss_ssim,))
        if loss_ssim > 0 and loss == "reference":
            raise ValueError("loss_ssim belongs to the fused losses (%s), got loss='reference'" % ", ".join(sr_losses.KINDS))
        self.loss_ssim = float(loss_ssim)   # alpha of (1 - alpha) * loss + alpha * (1 - SSIM); 0: no SSIM term
        self._ssim_sum, self._ssim_steps, self.last_train_ssim = None, 0, None
        self.ema_decay = sr_ema.check_decay(ema_decay)   # 0: no weight average; else ema.ParamEMA after every step()
        self.ema = None
        self.path = path
        self.net = net
        self.run_config = run_config
        self.mix_prec = mix_prec   # None | 'bf16' | 'f16': activation dtype via torch.autocast (apex in the reference)
        self.best_acc = 0
        self.start_epoch = 0
        os.makedirs(self.path, exist_ok=True)
        ops.single_thread_backward(True)   # one process drives one GPU: backward() on the calling thread (ops.py)

        if no_gpu or not torch.cuda.is_available():
            raise RuntimeError("SRRunManager drives the MI355X HIP hot path: a GPU is required (no CPU fallback)")
        self.device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(self.device)
        self.net = self.net.to(self.device)
        torch.backends.cudnn.benchmark = True

        if init:
            self.network.init_model(run_config.model_init)
        dd.broadcast_module(self.network)

        if self.is_root:
            net_info = get_net_info(self.net, self.run_config.data_provider.data_shape, measure_latency, True, args)
            with open("%s/net_info.txt" % self.path, "w") as fout:
                fout.write(json.dumps(net_info, indent=4) + "\n")
                try:
                    fout.write(self.network.module_str)
                except Exception:
                    pass

        self.train_criterion = nn.MSELoss()
        self.test_criterion = nn.MSELoss()
        spec = getattr(run_config, "degrade", None)
        if spec is not None:
            if type(self.network).__name__ == "OFAMobileNetX4":      # its input key is 'image' (search.lr_key)
                raise ValueError("degrade=: %s takes the HR image as its input ('image'), it has no LR input to degrade"
                                 % type(self.network).__name__)
            self.write_log("Degraded LR inputs: %s seed %d (degrade.py: Gaussian blur before, noise after the bicubic)" % (
                sr_degrade.describe(spec), run_config.degrade_seed), prefix="train")
        if self.loss != "reference":
            self.write_log("Training loss: %s%s%s (fused HIP loss, ops.sr_loss)" % (
                self.loss, " eps %g" % self.loss_eps if self.loss == "charbonnier" else "",
                " + %g (1 - SSIM), the pixel term weighted %g" % (self.loss_ssim, 1.0 - self.loss_ssim)
                if self.loss_ssim > 0 else ""), prefix="train")

        if self.run_config.no_decay_keys:
            keys = self.run_config.no_decay_keys.split("#")
            net_params = [list(self.network.get_parameters(keys, mode="exclude")),   # with weight decay
                          list(self.network.get_parameters(keys, mode="include"))]   # without
        else:
            net_params = list(self.network.weight_parameters())
        self.optimizer = self.run_config.build_optimizer(net_params)
        # OFASR_DP_OVERLAP=1: two buckets, the decoder tail's exchanged while the MB stack's backward still runs
        # (distributed.FlatGradReducer(early_params=...)); default: the single flat bucket
        early = None
        if os.environ.get("OFASR_DP_OVERLAP", "0") != "0" and hasattr(self.network, "early_gradient_parameters"):
            early = self.network.early_gradient_parameters()
        self.reducer = dd.FlatGradReducer(self.network.parameters(), gather=True, early_params=early) \
            if dd.is_distributed() else None
        if self.ema_decay > 0:
            self.ema = sr_ema.ParamEMA(self.network.named_parameters(), self.ema_decay)
            self.write_log("Weight EMA: decay %g (warm-up (1+t)/(10+t)); validation, best_acc and model_best use the "
                           "averaged weights" % self.ema_decay, prefix="train")

    # ------------------------------------------------------------------ distributed helpers
    @property
    def is_root(self):
        return dd.rank() == 0

    def zero_grad(self):
        """optimizer.zero_grad() on one GPU; re-arm the flat gradient bucket under data parallelism."""
        if self.reducer is not None:
            self.reducer.prepare()
        else:
            self.optimizer.zero_grad(set_to_none=True)

    def last_backward_next(self):
        """the next backward pass is the last one before step(): the overlapped gradient exchange may start in it"""
        if self.reducer is not None:
            self.reducer.arm()

    def step(self):
        """gradient exchange (one flat all-reduce) + optimizer step + (with ema_decay) the weight average's update, one
        launch.  Under data parallelism every rank updates its own shadow from parameters that are identical on all
        ranks after the all-reduce and the same optimizer step, so the shadows stay equal and nothing is exchanged."""
        if self.reducer is not None:
            self.reducer.reduce()
        self.optimizer.step()
        if self.ema is not None:
            self.ema.update()

    @contextlib.contextmanager
    def ema_weights(self):
        """inside: the network holds the averaged parameters (and its own current buffers); on exit, also by an
        exception, the trained ones again -- one swap launch each way, at the same addresses (ema.ParamEMA.swap, which
        clears the inference operand cache both times).  A no-op without ema_decay."""
        if self.ema is None:
            yield
            return
        self.ema.swap()
        try:
            yield
        finally:
            self.ema.swap()

    def reset_ema(self, why=None):
        """re-initialise the shadow from the parameters as they are now (updates = 0): after anything that rewrites
        the parameters other than an optimizer step -- a warm start, a re-organisation of the channels"""
        if self.ema is None:
            return
        self.ema.reset()
        if why:
            self.write_log("Weight EMA: re-initialised from the current parameters, updates = 0 (%s)" % why, prefix="train")

    def autocast(self):
        if self.mix_prec in (None, "f32"):
            return torch.autocast("cuda", enabled=False)
        return torch.autocast("cuda", dtype={"bf16": torch.bfloat16, "f16": torch.float16}[self.mix_prec])

    # --------------------------------------------------------------------------- paths / logs
    @property
    def save_path(self):
        p = os.path.join(self.path, "checkpoint")
        os.makedirs(p, exist_ok=True)
        return p

    @property
    def logs_path(self):
        p = os.path.join(self.path, "logs")
        os.makedirs(p, exist_ok=True)
        return p

    @property
    def network(self):
        return self.net

    @network.setter
    def network(self, new_val):
        self.net = new_val

    def write_log(self, log_str, prefix="valid", should_print=True):
        """prefix: valid, train, test (reference :232-249)"""
        if not self.is_root:
            return
        if prefix in ("valid", "test"):
            with open(os.path.join(self.logs_path, "valid_console.txt"), "a") as fout:
                fout.write(log_str + "\n")
        if prefix in ("valid", "test", "train"):
            with open(os.path.join(self.logs_path, "train_console.txt"), "a") as fout:
                if prefix in ("valid", "test"):
                    fout.write("=" * 10)
                fout.write(log_str + "\n")
        else:
            with open(os.path.join(self.logs_path, "%s.txt" % prefix), "a") as fout:
                fout.write(log_str + "\n")
        if should_print:
            print(log_str)

    # ------------------------------------------------------------------------- checkpoints
    def save_model(self, checkpoint=None, is_best=False, model_name=None, best_state_dict=None):
        """checkpoint/{<model_name>,model_best}.pth.tar + latest.txt (reference :253-273).  `best_state_dict`: what
        model_best holds when it is not the checkpoint's own state dict (the averaged weights, taken inside
        ema_weights()).  With ema_decay every checkpoint written here gains "ema" and "ema_decay"."""
        if not self.is_root:
            return
        if checkpoint is None:
            checkpoint = {"state_dict": self.network.state_dict()}
        if model_name is None:
            model_name = "checkpoint.pth.tar"
        checkpoint["dataset"] = self.run_config.dataset
        if getattr(self.run_config, "crop_candidates", 1) != 1:      # best-of-K training crops (data_providers/augment.py)
            checkpoint["crop_candidates"] = int(self.run_config.crop_candidates)
        if getattr(self.run_config, "degrade", None) is not None:    # blurred, noisy LR inputs (degrade.py)
            checkpoint["degrade"] = dict(self.run_config.degrade, blur=list(self.run_config.degrade["blur"]),
                                         noise=list(self.run_config.degrade["noise"]))
            checkpoint["degrade_seed"] = int(self.run_config.degrade_seed)
        if self.loss != "reference":
            checkpoint["loss"] = self.loss
            if self.loss == "charbonnier":
                checkpoint["loss_eps"] = self.loss_eps
            if self.loss_ssim > 0:
                checkpoint["loss_ssim"] = self.loss_ssim
        if self.ema is not None:
            checkpoint["ema_decay"] = self.ema_decay
            if "ema" not in checkpoint:
                checkpoint["ema"] = self.ema.state_dict()
        model_path = os.path.join(self.save_path, model_name)
        with open(os.path.join(self.save_path, "latest.txt"), "w") as fout:
            fout.write(model_path + "\n")
        torch.save(checkpoint, model_path)
        if is_best:
            torch.save({"state_dict": checkpoint["state_dict"] if best_state_dict is None else best_state_dict},
                       os.path.join(self.save_path, "model_best.pth.tar"))

    def best_state_dict(self):
        """a copy of the network's state dict as it is now, for save_model(best_state_dict=): called inside
        ema_weights(), where it holds the averaged parameters.  None without ema_decay (model_best is then written from
        the checkpoint itself, as ever)."""
        if self.ema is None:
            return None
        return {k: v.detach().clone() for k, v in self.network.state_dict().items()}

    def load_model(self, model_fname=None):
        """reference :275-308 -- but failures are raised, not swallowed."""
        latest = os.path.join(self.save_path, "latest.txt")
        if model_fname is None and os.path.exists(latest):
            with open(latest) as fin:
                model_fname = fin.readline().rstrip("\n")
        if model_fname is None or not os.path.exists(model_fname):
            model_fname = "%s/checkpoint.pth.tar" % self.save_path
        checkpoint = torch.load(model_fname, map_location="cpu", weights_only=True)
        self.network.load_state_dict(checkpoint["state_dict"])
        if "epoch" in checkpoint:
            self.start_epoch = checkpoint["epoch"] + 1
        if "best_acc" in checkpoint:
            self.best_acc = checkpoint["best_acc"]
        if "optimizer" in checkpoint:
            self.optimizer.load_state_dict(checkpoint["optimizer"])
        if self.ema is not None:
            if "ema" in checkpoint:
                self.ema.load_state_dict(checkpoint["ema"])
            else:
                self.reset_ema("%s has no \"ema\" entry" % model_fname)
        return model_fname

    def save_config(self):
        if not self.is_root:
            return
        run_save_path = os.path.join(self.path, "run.config")
        config = self.run_config.config
        if self.loss_ssim > 0:      # the one setting of the run that lives on the manager and has no other record here
            config = dict(config, loss_ssim=self.loss_ssim)
        if self.ema_decay > 0:
            config = dict(config, ema_decay=self.ema_decay)
        with open(run_save_path, "w") as f:
            json.dump(config, f, indent=4)
        print("Run configs dump to %s" % run_save_path)

    # --------------------------------------------------------------------- validate / train
    def _eval_batch(self, mini_batch, degrade, at):
        """device_batch of an evaluation item.  `degrade` = (blur sigma, noise sigma, seed): its LR images carry that fixed
        degradation (degrade.fixed_rows: sigma_x = sigma_y, stream = the image's running index, `at` for the item's
        first), which needs items that carry the uint8 HR image (a provider built with lr_on_device=True, or video)."""
        if degrade is None:
            return device_batch(mini_batch, self.device)
        if "image_u8" not in mini_batch or "lr_u8" in mini_batch:
            raise ValueError("degrade= evaluates items that carry 'image_u8' alone (a provider built with lr_on_device=True, "
                             "or unpaired video): got keys %s" % sorted(mini_batch))
        blur, noise, seed = degrade
        rows = sr_degrade.fixed_rows(mini_batch["image_u8"].shape[0], blur, noise, first=at)
        table = torch.from_numpy(sr_degrade.degrade_table(rows)).to(self.device)
        return device_batch(dict(mini_batch, degrade=table, degrade_seed=int(seed)), self.device)

    def validate(self, epoch=0, is_test=True, run_str="", net=None, data_loader=None, no_logs=False,
                 tensorboard_logging=False, input_key="2x_down_image", degrade=None):
        """eval-mode pass over the test (or valid) loader: (mean MSE loss, mean Y-PSNR).  The reference
        always feeds '2x_down_image' (:352-361, quirk Q4); `input_key` lifts that for 4x nets.  `degrade`: _eval_batch."""
        if net is None:
            net = self.net
        if data_loader is None:
            data_loader = self.run_config.test_loader if is_test else self.run_config.valid_loader
        net.eval()
        losses, psnrs = AverageMeter(), AverageMeter()
        with torch.no_grad():
            at = 0
            for mini_batch in data_loader:
                mini_batch = self._eval_batch(mini_batch, degrade, at)
                at += mini_batch["image"].shape[0]
                images, lr = mini_batch["image"], mini_batch[input_key]
                with self.autocast():
                    output = net(lr)
                output = output.float()
                loss = self.test_criterion(output, images)
                losses.update(loss.item(), images.size(0))
                psnrs.update(psnr_y(output, images), images.size(0))
        return losses.avg, psnrs.avg

    def graphed(self, net):
        """the hipGraph-replayed forward of `net` in this manager's precision (graphed.GraphedEval), one per network"""
        cache = self.__dict__.setdefault("_graphed", {})
        g = cache.get(id(net))
        if g is None or g.net is not net:
            dt = None if self.mix_prec in (None, "f32") else {"bf16": torch.bfloat16, "f16": torch.float16}[self.mix_prec]
            g = cache[id(net)] = GraphedEval(net, autocast_dtype=dt)
        return g

    def validate_batched(self, net=None, data_loader=None, is_test=True, input_key="2x_down_image", max_batch=None,
                         graphs=None, degrade=None):
        """`validate` with the loader's batch-1 items of EQUAL size run as one batch (BASELINE config 5: Set14 at
        full resolution, reference eval_ofa_net_sr.py:187-220,247-251 / sr_run_manager.py:323-393).  Loss and PSNR are
        taken per image, so the result equals `validate` on the batch-1 loader (tests/test_hip_configs.py).
        `graphs` (default: on for 16-bit GPU inference unless OFASR_EVAL_GRAPHS=0): the forwards of all size buckets are
        captured once as ONE hipGraph and replayed -- the per-launch host cost otherwise bounds this loop (graphed.py).
        `degrade`: _eval_batch.  Returns (mean loss, mean PSNR, number of forward calls)."""
        if net is None:
            net = self.net
        if graphs is None:
            # 16-bit inference (the one-kernel blocks / ConvLayers) by default; the fp32 path is eager unless asked
            graphs = (os.environ.get("OFASR_EVAL_GRAPHS", "1") != "0" and str(self.device).startswith("cuda")
                      and self.mix_prec in ("bf16", "f16"))
        fwd = self.graphed(net) if graphs else None
        if data_loader is None:
            data_loader = self.run_config.test_loader if is_test else self.run_config.valid_loader
        net.eval()
        items = []
        for mini_batch in data_loader:
            mini_batch = self._eval_batch(mini_batch, degrade, len(items))
            for i in range(mini_batch["image"].shape[0]):
                items.append({k: v[i:i + 1] for k, v in mini_batch.items() if torch.is_tensor(v)})
        losses, psnrs, calls = AverageMeter(), AverageMeter(), 0
        with torch.no_grad():
            groups = list(bucket_by_size(items, key=lambda it: it[input_key], max_batch=max_batch))
            lrs = [torch.cat([it[input_key] for it in group]).to(self.device) for group in groups]
            # all size buckets of the pass in ONE captured graph / one replay (the validation set is the same every epoch)
            outs = fwd.call_many(lrs) if (fwd is not None and lrs) else None
            for gi, group in enumerate(groups):
                images = torch.cat([it["image"] for it in group]).to(self.device)
                if outs is not None:
                    output = outs[gi].float()
                else:
                    with self.autocast():
                        output = net(lrs[gi]).float()
                calls += 1
                per_img = ((output - images) ** 2).mean(dim=(1, 2, 3))
                for v in per_img.tolist():
                    losses.update(v, 1)
                for v in psnr_y_per_image(output, images):
                    psnrs.update(v, 1)
        return losses.avg, psnrs.avg, calls

    def validate_quality(self, net=None, data_loader=None, is_test=True, input_key="2x_down_image", max_batch=None,
                         graphs=None, shave=0, self_ensemble=1, degrade=None):
        """`validate_batched` (same size buckets, same forwards) scored on the GPU: Y-PSNR and Y-SSIM by the HIP metric
        kernel (ops.quality_y: exact integer luma, `shave` border pixels dropped) and the per-image MSE loss by
        ops.quality_mse, straight from the network's output.  No image goes to the host and no ATen kernel runs between
        the forwards and the ONE read-back of the per-image numbers at the end.  PSNR equals validate_batched's unless an
        image holds one of the 194 colours whose exact luma is a rounding tie (utils.y_exact).
        `self_ensemble` = k in {2, 4, 8}: every bucket is scored on the fp32 mean of the network's outputs under the first
        k flips / transposes (ops.self_ensemble); with graphs, the transformed inputs of all buckets run as one replay.
        "calls" then counts k forwards per bucket.  `degrade`: _eval_batch.
        Returns {"loss", "psnr", "ssim", "calls"} (means over the images; "psnr_per_image" / "ssim_per_image" beside)."""
        if net is None:
            net = self.net
        k = self_ensemble
        if isinstance(k, bool) or k not in ops.ENSEMBLE_SIZES:
            raise ValueError("self_ensemble must be one of %s, got %r" % (ops.ENSEMBLE_SIZES, k))
        if graphs is None:
            graphs = (os.environ.get("OFASR_EVAL_GRAPHS", "1") != "0" and str(self.device).startswith("cuda")
                      and self.mix_prec in ("bf16", "f16"))
        fwd = self.graphed(net) if graphs else None
        if data_loader is None:
            data_loader = self.run_config.test_loader if is_test else self.run_config.valid_loader
        net.eval()
        items = []
        for mini_batch in data_loader:
            mini_batch = self._eval_batch(mini_batch, degrade, len(items))
            for i in range(mini_batch["image"].shape[0]):
                items.append({k_: v[i:i + 1] for k_, v in mini_batch.items() if torch.is_tensor(v)})
        calls = 0

        def eager(x):
            with self.autocast():
                return net(x)
        with torch.no_grad():
            groups = list(bucket_by_size(items, key=lambda it: it[input_key], max_batch=max_batch))
            lrs = [torch.cat([it[input_key] for it in group]).to(self.device) for group in groups]
            hrs = [torch.cat([it["image"] for it in group]).to(self.device) for group in groups]
            # rows: sse (int64), the bits of ssim (fp64), the bits of the mse (fp64); one column per image
            res = torch.empty((3, len(items)), dtype=torch.int64, device=self.device)
            counts, at = [], 0
            if k > 1:
                lrs = [x.contiguous() for x in lrs]
            if fwd is not None and lrs:
                # with the ensemble: T_t of every bucket, t = 0 .. k-1, in the one captured graph
                outs = fwd.call_many([x if t == 0 else ops.d4_apply(x, t) for x in lrs for t in range(k)])
            else:
                outs = None
            for gi, group in enumerate(groups):
                if k > 1 and outs is not None:
                    output = None
                    for t in range(k):
                        y = outs[gi * k + t].contiguous()
                        if output is None:
                            output = torch.empty(y.shape, dtype=torch.float32, device=y.device)
                        ops.d4_accumulate(y, t, output, t == 0, 1.0 / k if t == k - 1 else 1.0)
                elif k > 1:
                    output = ops.self_ensemble(eager, lrs[gi], k)
                elif outs is not None:
                    output = outs[gi]
                else:
                    output = eager(lrs[gi])
                calls += k
                n = len(group)
                _, _, count = ops.quality_y(output, hrs[gi], shave, out=res[:2, at:at + n])
                ops.quality_mse(output, hrs[gi], out=res[2, at:at + n].view(torch.float64))
                counts += [count] * n
                at += n
            host = res.cpu()
        sse, ssim, mse = host[0].tolist(), host[1].view(torch.float64).tolist(), host[2].view(torch.float64).tolist()
        psnr = [psnr_from_sse(s, c) for s, c in zip(sse, counts)]
        mean = lambda v: sum(v) / len(v) if v else 0.0
        return {"loss": mean(mse), "psnr": mean(psnr), "ssim": mean(ssim), "calls": calls, "psnr_per_image": psnr,
                "ssim_per_image": ssim}

    def train_loss(self, output, images, soft=None, kd_ratio=0, shrinking=False):
        """The loss section of one training (sub-)step, for both loops: (loss, psnr, output).  `output` is the network's
        output as the autocast region left it, `soft` the teacher's or None; `shrinking` tells the progressive-shrinking
        loop, which scales the sum by 2 / (kd_ratio + 1) and takes its PSNR on the device, from the teacher loop.
        loss='reference': the lines the two loops always ran -- output.float(), nn.MSELoss, F.mse_loss against the
        teacher, utils.psnr_y_device (psnr is None in the teacher loop, which scores `output` on the host after its
        step).  Otherwise ops.sr_loss on the output as it is: loss, gradient and PSNR from the HIP kernels, psnr a 0-dim
        fp64 view of the result buffer.  With loss_ssim > 0 the loss carries the SSIM term and the step's mean SSIM is
        added, on the GPU, to the epoch's sum (log_train_ssim)."""
        if self.loss == "reference":
            output = output.float()
            loss = self.train_criterion(output, images)
            if soft is not None:
                loss = kd_ratio * torch.nn.functional.mse_loss(output, soft) + loss
                if shrinking:
                    loss = loss * (2 / (kd_ratio + 1))
            return loss, (psnr_y_device(output, images) if shrinking else None), output
        w_main, w_kd = sr_losses.kd_weights(kd_ratio, shrinking) if soft is not None else (1.0, 0.0)
        n, _, h, w = output.shape
        loss, res = ops.sr_loss(output, images, soft, kind=self.loss, eps=self.loss_eps, w_main=w_main, w_kd=w_kd,
                                psnr_count=sr_losses.mosaic_count(n, h, w), ssim=self.loss_ssim)
        if self.loss_ssim > 0:
            if self._ssim_sum is None:
                self._ssim_sum = torch.zeros((), device=res.device, dtype=torch.float64)
            self._ssim_sum += res[ops.SR_LOSS_SSIM]
            self._ssim_steps += 1
        return loss, res[ops.SR_LOSS_PSNR], output

    def train_one_epoch(self, args, epoch, warmup_epochs=0, warmup_lr=0, input_key="2x_down_image"):
        """fixed-architecture ("teacher") epoch: BatchNorm layers run in eval mode (frozen statistics,
        reference :417-420), MSE loss, one optimizer step per batch.  Returns (mean loss, mean PSNR)."""
        self.net.train()
        for m in self.net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()
        loader = self.run_config.train_loader
        sampler = getattr(loader, "sampler", None)
        if hasattr(sampler, "set_epoch"):      # a rank-sharding sampler replays the same permutation otherwise
            sampler.set_epoch(epoch)
        nBatch = len(loader)
        losses, psnrs, data_time = AverageMeter(), AverageMeter(), AverageMeter()
        end = time.time()
        for i, mini_batch in enumerate(loader):
            data_time.update(time.time() - end)
            if epoch < warmup_epochs:
                new_lr = self.run_config.warmup_adjust_learning_rate(self.optimizer, warmup_epochs * nBatch, nBatch,
                                                                     epoch, i, warmup_lr)
            else:
                new_lr = self.run_config.adjust_learning_rate(self.optimizer, epoch - warmup_epochs, i, nBatch)
            mini_batch = device_batch(mini_batch, self.device)
            images, lr_img = mini_batch["image"], mini_batch[input_key]
            with self.autocast():
                output = self.net(lr_img)
            teacher = getattr(args, "teacher_model", None)
            soft = None
            if teacher is not None:
                teacher.train()
                with torch.no_grad():
                    soft = teacher(images).detach()
            loss, psnr, output = self.train_loss(output, images, soft, args.kd_ratio)
            self.zero_grad()
            loss.backward()
            ops.flush_deferred()   # the MB blocks' weight gradients: joined once per backward pass (ops.py)
            self.step()
            losses.update(loss.item(), images.size(0))
            psnrs.update(psnr_y(output, images) if psnr is None else float(psnr), images.size(0))
            end = time.time()
        self._last_lr = new_lr
        self.log_crop_selection(epoch)
        self.log_train_ssim(epoch)
        return losses.avg, psnrs.avg

    def log_train_ssim(self, epoch):
        """with loss_ssim > 0: one line per epoch, the mean over the epoch's loss calls of S, the mean SSIM of the output
        against the HR batch (slot SR_LOSS_SSIM of each call's result buffer, summed on the GPU).  Both loops call it
        after their own host reads, so the one read here waits for nothing; last_train_ssim keeps the value for the
        epoch's Valid line."""
        self.last_train_ssim = None
        if self.loss_ssim <= 0 or self._ssim_steps == 0:
            return
        self.last_train_ssim = float(self._ssim_sum) / self._ssim_steps
        self.write_log("Train SSIM [%d]\tmean S %.6f\tloss calls %d" % (epoch + 1, self.last_train_ssim, self._ssim_steps),
                       prefix="train")
        self._ssim_sum.zero_()
        self._ssim_steps = 0

    def log_crop_selection(self, epoch):
        """with best-of-K training crops (ResidentTrainLoader(candidates=K > 1)): one line per epoch, the mean luma
        activity per difference in 8-bit levels (routing.mean_activity) of the chosen crops and of the first candidates
        -- what a loader without candidates would have served.  The epoch's one read of the selection counters."""
        loader = self.run_config.train_loader
        if getattr(loader, "candidates", 1) <= 1:
            return
        from ... import routing
        chosen, first, count = loader.selection_stats()
        S, c = loader.size, max(count, 1)
        self.write_log("Crop selection [%d]\tK=%d\tcrops %d\tmean activity chosen %.3f\tfirst candidate %.3f" % (
            epoch + 1, loader.candidates, count, float(routing.mean_activity(chosen, S, S)) / c,
            float(routing.mean_activity(first, S, S)) / c), prefix="train")

    def train(self, args, warmup_epoch=0, warmup_lr=0):
        """reference :516-541"""
        for epoch in range(self.start_epoch, self.run_config.n_epochs + warmup_epoch):
            train_loss, train_psnr = self.train_one_epoch(args, epoch, warmup_epoch, warmup_lr)
            is_best, best_sd = False, None
            if (epoch + 1) % self.run_config.validation_frequency == 0:
                with self.ema_weights():       # with ema_decay: the averaged weights are what is validated and kept
                    val_loss, val_psnr = self.validate(epoch=epoch, is_test=False)
                    is_best = np.mean(val_psnr) > self.best_acc
                    if is_best:
                        best_sd = self.best_state_dict()
                self.best_acc = max(self.best_acc, np.mean(val_psnr))
                self.write_log("Valid [%d/%d]\tloss %.3f\ttop-1 acc %.3f (%.3f)\tTrain top-1 %.3f\tloss %.3f\t%s" % (
                    epoch + 1 - warmup_epoch, self.run_config.n_epochs, np.mean(val_loss), np.mean(val_psnr),
                    self.best_acc, train_psnr, train_loss,
                    "" if self.last_train_ssim is None else "SSIM %.4f\t" % self.last_train_ssim),
                    prefix="valid", should_print=False)
            self.save_model({"epoch": epoch, "best_acc": self.best_acc, "optimizer": self.optimizer.state_dict(),
                             "state_dict": self.network.state_dict()}, is_best=is_best, best_state_dict=best_sd)

    def reset_running_statistics(self, net=None):
        from ...elastic_nn.utils import set_running_statistics
        set_running_statistics(self.network if net is None else net, self.run_config.train_loader)
