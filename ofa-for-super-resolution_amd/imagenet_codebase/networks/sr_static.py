"""Specialized static SR networks: what OFAMobileNetS4 / OFAMobileNetX4.get_active_subnet() extract.

A static network holds exactly the active sub-network of a supernet -- fixed kernel size and mid width per MB block, the
active depth per stage, the active number of (un)shuffle blocks -- as plain layers (layers.py ConvLayer,
MBInvertedConvLayer, IdentityLayer), with a real forward, a JSON config (`config` / `build_from_config`) and state-dict
keys in the static spelling (`blocks.N.mobile_inverted_conv.inverted_bottleneck.conv.weight`, `....bn.weight`, ...;
blocks numbered consecutively, MB blocks first, then the conv + PixelShuffle blocks, as in the supernet).

The MB blocks (each with its identity shortcut) run on the HIP block kernels, never on ATen:
  * eval-mode BN, no gradients, 16-bit activations: the one-kernel block (ops.mbconv_infer)
  * eval-mode BN, no gradients, fp32: the fp32 one-kernel block (ops.mbconv_infer_f32) when ops.F32_INFER is on and the
    kernel supports the shape, else the composite block (ops.FusedMBConvFn)
  * gradients or train-mode BN (fine-tuning): the whole MB stack as one node (ops.mbstack)
"""
import torch
import torch.nn as nn

from ... import ops
from ...layers import IdentityLayer, MBInvertedConvLayer, set_layer_from_config
from ...utils import MyNetwork
from .proxyless_nets import MobileInvertedResidualBlock


def _block_from_config(cfg):
    if cfg["name"] == MobileInvertedResidualBlock.__name__:
        return MobileInvertedResidualBlock.build_from_config(cfg)
    return set_layer_from_config(cfg)


def mb_block_config(in_channels, out_channels, kernel_size, expand_ratio, mid_channels, act_func="relu6"):
    """config of MobileInvertedResidualBlock(MBInvertedConvLayer, IdentityLayer) -- what the extraction builds"""
    return {
        "name": MobileInvertedResidualBlock.__name__,
        "mobile_inverted_conv": {
            "name": MBInvertedConvLayer.__name__, "in_channels": in_channels, "out_channels": out_channels,
            "kernel_size": kernel_size, "stride": 1, "expand_ratio": expand_ratio, "mid_channels": mid_channels,
            "act_func": act_func, "use_se": False,
        },
        "shortcut": {"name": IdentityLayer.__name__, "in_channels": in_channels, "out_channels": in_channels,
                     "use_bn": False, "act_func": None, "dropout_rate": 0, "ops_order": "weight_bn_act"},
    }


def run_mb_blocks(x, blocks):
    """the MB blocks (MobileInvertedResidualBlock of MBInvertedConvLayer + identity shortcut) in turn, on the HIP block
    kernels (module docstring)"""
    if not blocks:
        return x
    ops._gpu(x)
    if torch.is_autocast_enabled() and x.dtype == torch.float32:
        x = x.to(torch.get_autocast_dtype("cuda"))
    items = []
    ch = x.size(1)
    for b in blocks:
        mb = b.mobile_inverted_conv
        if not (isinstance(mb, MBInvertedConvLayer) and mb.composite_eligible()):
            raise NotImplementedError("static MB block outside the HIP block kernels: %s" % mb.module_str)
        add_x = isinstance(b.shortcut, IdentityLayer) and not b.shortcut._modules
        if b.shortcut is not None and not add_x:
            raise NotImplementedError("static MB block with a non-identity shortcut")
        items.append(mb.composite_args(ch, add_x))
        ch = mb.out_channels
    if ops.RECAL is not None:   # BatchNorm re-calibration (elastic_nn.utils.recalibrate_bn)
        for cfg, ps in items:
            x = ops.RECAL.mb_block(x, cfg, ps, x if cfg["residual"] else None)
        return x
    infer = not torch.is_grad_enabled() and not any(bn.training for cfg, _ in items for bn in cfg["bns"])
    if infer:
        for cfg, ps in items:
            y = None
            if ops.FUSED_INFER:
                if x.dtype == torch.float32:
                    y = ops.mbconv_infer_f32(x, cfg, *ps) if ops.F32_INFER else None
                else:
                    y = ops.mbconv_infer(x, cfg, *ps)
            x = y if y is not None else ops.FusedMBConvFn.apply(x, cfg, *ps)
        return x
    if ops.FUSED_STACK:
        return ops.mbstack(x, [cfg for cfg, _ in items], [p for _, ps in items for p in ps])
    for cfg, ps in items:
        x = ops.FusedMBConvFn.apply(x, cfg, *ps)
    return x


class _StaticSRNet(MyNetwork):

    def _common_config(self):
        return {"name": type(self).__name__, "bn": self.get_bn_param(), "upscale": self.upscale}

    @property
    def module_str(self):
        return "\n".join(b.module_str for b in self.blocks) + "\n"

    def mb_blocks(self):
        return [b for b in self.blocks if isinstance(b, MobileInvertedResidualBlock)]

    def zero_last_gamma(self):
        ops.clear_infer_cache()
        for b in self.mb_blocks():
            b.mobile_inverted_conv.point_linear.bn.weight.data.zero_()


class SRNetS4(_StaticSRNet):
    """stem -> long skip -> MB blocks -> 2 residual convs (skip added after the first) -> conv + PixelShuffle blocks ->
    head (OFAMobileNetS4.forward with the active path fixed).  `upscale` is the factor the LR input must have: the
    supernet's active_upscale() at extraction time."""

    def __init__(self, dec_first_conv_block, mb_blocks, dec_final_conv_blocks, shuffle_blocks,
                 dec_final_output_conv_block, upscale):
        super().__init__()
        self.dec_first_conv_block = dec_first_conv_block
        self.blocks = nn.ModuleList(list(mb_blocks) + list(shuffle_blocks))
        self.dec_final_conv_blocks = nn.ModuleList(dec_final_conv_blocks)
        self.dec_final_output_conv_block = dec_final_output_conv_block
        self.n_mb = len(mb_blocks)
        self.upscale = int(upscale)

    @staticmethod
    def name():
        return "SRNetS4"

    def forward(self, x):
        with ops.batched_counters():
            x = self.dec_first_conv_block(x)
            skip = x
            x = run_mb_blocks(x, list(self.blocks[:self.n_mb]))
            for i, conv in enumerate(self.dec_final_conv_blocks):
                x = conv(x)
                if i == 0:
                    x = ops.skip_add(x, skip)
            for blk in self.blocks[self.n_mb:]:
                x = blk(x)
            return self.dec_final_output_conv_block(x)

    @property
    def config(self):
        return {
            **self._common_config(),
            "dec_first_conv_block": self.dec_first_conv_block.config,
            "blocks": [b.config for b in self.blocks],
            "n_mb": self.n_mb,
            "dec_final_conv_blocks": [c.config for c in self.dec_final_conv_blocks],
            "dec_final_output_conv_block": self.dec_final_output_conv_block.config,
        }

    @staticmethod
    def build_from_config(config):
        blocks = [_block_from_config(c) for c in config["blocks"]]
        n_mb = config["n_mb"]
        net = SRNetS4(set_layer_from_config(config["dec_first_conv_block"]), blocks[:n_mb],
                      [set_layer_from_config(c) for c in config["dec_final_conv_blocks"]], blocks[n_mb:],
                      set_layer_from_config(config["dec_final_output_conv_block"]), config["upscale"])
        if config.get("bn") is not None:
            net.set_bn_param(**config["bn"])
        return net


class SRNetX4(_StaticSRNet):
    """conv + PixelUnshuffle blocks -> encoder MB blocks -> 3 encoder convs (skip after the first) -> decoder first conv ->
    decoder MB blocks -> 2 convs (skip after the first) -> conv + PixelShuffle blocks -> head (OFAMobileNetX4.forward with
    the active path fixed).  `upscale` = 2 ** (shuffle blocks - unshuffle blocks): the output / input size ratio."""

    def __init__(self, unshuffle_blocks, enc_blocks, enc_final_conv_blocks, dec_first_conv_block, dec_blocks,
                 dec_final_conv_blocks, shuffle_blocks, dec_final_output_conv_block, upscale):
        super().__init__()
        self.blocks = nn.ModuleList(list(unshuffle_blocks) + list(enc_blocks) + list(dec_blocks) + list(shuffle_blocks))
        self.enc_final_conv_blocks = nn.ModuleList(enc_final_conv_blocks)
        self.dec_first_conv_block = dec_first_conv_block
        self.dec_final_conv_blocks = nn.ModuleList(dec_final_conv_blocks)
        self.dec_final_output_conv_block = dec_final_output_conv_block
        self.n_unshuffle, self.n_enc, self.n_dec = len(unshuffle_blocks), len(enc_blocks), len(dec_blocks)
        self.upscale = upscale

    @staticmethod
    def name():
        return "SRNetX4"

    def forward(self, x):
        u, e, d = self.n_unshuffle, self.n_enc, self.n_dec
        with ops.batched_counters():
            for blk in self.blocks[:u]:
                x = blk(x)
            skip = x
            x = run_mb_blocks(x, list(self.blocks[u:u + e]))
            for i, c in enumerate(self.enc_final_conv_blocks):
                x = c(x)
                if i == 0:
                    x = ops.skip_add(x, skip)
            x = self.dec_first_conv_block(x)
            skip = x
            x = run_mb_blocks(x, list(self.blocks[u + e:u + e + d]))
            for i, c in enumerate(self.dec_final_conv_blocks):
                x = c(x)
                if i == 0:
                    x = ops.skip_add(x, skip)
            for blk in self.blocks[u + e + d:]:
                x = blk(x)
            return self.dec_final_output_conv_block(x)

    @property
    def config(self):
        return {
            **self._common_config(),
            "blocks": [b.config for b in self.blocks],
            "n_unshuffle": self.n_unshuffle, "n_enc": self.n_enc, "n_dec": self.n_dec,
            "enc_final_conv_blocks": [c.config for c in self.enc_final_conv_blocks],
            "dec_first_conv_block": self.dec_first_conv_block.config,
            "dec_final_conv_blocks": [c.config for c in self.dec_final_conv_blocks],
            "dec_final_output_conv_block": self.dec_final_output_conv_block.config,
        }

    @staticmethod
    def build_from_config(config):
        blocks = [_block_from_config(c) for c in config["blocks"]]
        u, e, d = config["n_unshuffle"], config["n_enc"], config["n_dec"]
        net = SRNetX4(blocks[:u], blocks[u:u + e], [set_layer_from_config(c) for c in config["enc_final_conv_blocks"]],
                      set_layer_from_config(config["dec_first_conv_block"]), blocks[u + e:u + e + d],
                      [set_layer_from_config(c) for c in config["dec_final_conv_blocks"]], blocks[u + e + d:],
                      set_layer_from_config(config["dec_final_output_conv_block"]), config["upscale"])
        if config.get("bn") is not None:
            net.set_bn_param(**config["bn"])
        return net


def build_static_net(config):
    """SRNetS4 / SRNetX4 from its config (config["name"])"""
    table = {SRNetS4.__name__: SRNetS4, SRNetX4.__name__: SRNetX4}
    return table[config["name"]].build_from_config(config)
