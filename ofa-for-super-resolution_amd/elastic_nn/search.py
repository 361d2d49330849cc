"""Sub-network search of the SR supernets: the architecture space, efficiency models and an evolutionary search.

Once-for-All's second step: find the per-block kernel sizes, expand ratios and stage depths that give the best Y-PSNR
under a budget of MACs or of milliseconds on this GPU.  A candidate's fitness is measured directly (psnr_fitness): fix the
sub-network, re-estimate its BatchNorm statistics on calibration images (recalibrate_bn, the HIP re-calibration
kernels), then take the fp32 Y-PSNR on validation images.  No accuracy predictor and no downloaded latency table:
LatencyTable times the layers of the space on this machine.

An arch is a dict {"ks": [per MB block], "e": [per MB block], "d": [per stage], "pixel_d": int}: what
set_active_subnet takes, drawn from the net's own candidate lists.
"""
import copy
import json
import math

import torch
import torch.nn as nn

from .. import _C, ops
from ..imagenet_codebase.utils.pytorch_utils import count_net_flops
from ..layers import ConvLayer
from ..utils import make_divisible
from .modules.dynamic_layers import DynamicMBConvLayer
from .utils import recalibrate_bn


def _is_x4(net):
    return type(net).__name__ == "OFAMobileNetX4"


class ArchSpace(object):
    """the architectures of `net` (OFAMobileNetS4 / OFAMobileNetX4).  `upscale` (S4): the LR -> HR factor every arch of
    the space must have; under COMPAT_REFERENCE_INDEXING the shuffle stage follows the first MB stage's depth (quirk
    Q1), so that depth is restricted instead of pixel_d.  X4 is an autoencoder: its archs are unconstrained, and the net's
    own _depth_of decides which entries of `d` a forward reads."""

    def __init__(self, net, upscale=None):
        self.net = net
        self.x4 = _is_x4(net)
        if self.x4:
            self.n_mb = len(net._mb_blocks())
            self.n_stages = len(net.block_group_info) - 2
        else:
            self.n_stages = len(net.block_group_info) - 1
            self.n_mb = len(net.blocks) - len(net.block_group_info[-1])
        self.ks_list = list(net.ks_list)
        self.e_list = list(net.expand_ratio_list)
        self.d_list = list(net.depth_list)
        self.pd_list = list(net.pixelshuffle_depth_list)
        self.d0_list = list(self.d_list)
        self.upscale = None if self.x4 else upscale
        if self.upscale is not None:
            n_shuffle = len(net.block_group_info[-1])
            steps = int(round(math.log2(self.upscale)))
            if 2 ** steps != self.upscale:
                raise ValueError("upscale must be a power of two, got %r" % upscale)
            if type(net).COMPAT_REFERENCE_INDEXING:
                self.d0_list = [d for d in self.d_list if min(d, n_shuffle) == steps]
            else:
                self.pd_list = [p for p in self.pd_list if min(p, n_shuffle) == steps]
            if not self.d0_list or not self.pd_list:
                raise ValueError("no arch of this space has upscale %d" % self.upscale)

    # -------------------------------------------------------------------------------------------- archs
    def _choices(self):
        """(field, index, candidates) for every entry of an arch"""
        out = [("ks", i, self.ks_list) for i in range(self.n_mb)]
        out += [("e", i, self.e_list) for i in range(self.n_mb)]
        out += [("d", i, self.d0_list if i == 0 else self.d_list) for i in range(self.n_stages)]
        return out + [("pixel_d", None, self.pd_list)]

    @staticmethod
    def _set(arch, field, idx, v):
        if idx is None:
            arch[field] = v
        else:
            arch[field][idx] = v

    @staticmethod
    def _get(arch, field, idx):
        return arch[field] if idx is None else arch[field][idx]

    def random_sample(self, rng):
        arch = {"ks": [None] * self.n_mb, "e": [None] * self.n_mb, "d": [None] * self.n_stages, "pixel_d": None}
        for field, idx, cands in self._choices():
            self._set(arch, field, idx, rng.choice(cands))
        return arch

    def mutate(self, arch, prob, rng):
        out = copy.deepcopy(arch)
        for field, idx, cands in self._choices():
            if rng.random() < prob:
                self._set(out, field, idx, rng.choice(cands))
        return out

    def crossover(self, a, b, rng):
        out = copy.deepcopy(a)
        for field, idx, _ in self._choices():
            self._set(out, field, idx, self._get(a if rng.random() < 0.5 else b, field, idx))
        return out

    def valid(self, arch):
        return all(self._get(arch, f, i) in c for f, i, c in self._choices())

    def apply(self, net, arch):
        # set_active_subnet inserts into its depth list: hand it copies
        net.set_active_subnet(ks=list(arch["ks"]), e=list(arch["e"]), d=list(arch["d"]), pixel_d=arch["pixel_d"])
        return net

    def key(self, arch):
        """canonical key of the active path (get_active_net_config without BN parameters): archs that differ only in
        blocks beyond the active depth share it"""
        self.apply(self.net, arch)
        cfg = self.net.get_active_net_config()
        cfg.pop("bn", None)
        return json.dumps(cfg, sort_keys=True)

    def macs(self, net, arch, lr_hw):
        """MACs of the convolutions on the arch's active path for one input of lr_hw (count_net_flops)"""
        self.apply(net, arch)
        return count_net_flops(net, (1, 3) + tuple(lr_hw))

    def upscale_of(self, arch):
        self.apply(self.net, arch)
        if self.x4:
            return 1
        return self.net.active_upscale()


def macs(net, arch, lr_hw, space=None):
    return (space or ArchSpace(net)).macs(net, arch, lr_hw)


# ------------------------------------------------------------------------------------------------ latency
def _layer_signatures(seq, H, W):
    """(signature, resolution) of every layer of an active_block_sequence() for an input of H x W, in order"""
    out = []
    for kind, m in seq:
        if isinstance(m, ConvLayer):
            sig = ("conv", m.in_channels, m.out_channels, m.kernel_size, m.act_func, H, W)
            out.append((sig, m))
            if m.act_func is not None and "pixelunshuffle" in m.act_func:
                H, W = H // 2, W // 2
            elif m.act_func is not None and "pixelshuffle" in m.act_func:
                H, W = H * 2, W * 2
        elif isinstance(m, DynamicMBConvLayer):
            cin = max(m.in_channel_list)
            out.append((("mb", m.active_kernel_size, m.active_middle_channel(cin), H, W), m))
        else:
            raise ValueError("unknown layer on the active path: %r" % (m,))
    return out


def _sig_str(sig):
    return "|".join(str(v) for v in sig)


def _time_us(fn, reps):
    """microseconds per call of fn() from the library's per-launch events (every launch of fn must be a library
    kernel); one untimed call first (operand preparation)"""
    L = _C.lib()
    with torch.no_grad():
        fn()
        torch.cuda.synchronize()
        L.ofasr_profile_enable(1)
        try:
            _C.profile_read()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            prof = _C.profile_read()
        finally:
            L.ofasr_profile_enable(0)
    return sum(v["total_us"] for v in prof.values()) / reps


class LatencyTable(object):
    """per-layer latency of the inference path a static net of the space takes (one-kernel fp32 / 16-bit MB blocks per
    (K, mid), the static conv layers), measured at batch N for an input of H x W with the library's per-launch events;
    predict(arch) sums the table over the arch's active path"""

    def __init__(self, space, N=1, H=64, W=64, dtype="f32", table=None):
        self.space = space
        self.N, self.H, self.W, self.dtype = int(N), int(H), int(W), dtype
        self.table = dict(table or {})

    def _archs_for_coverage(self):
        """archs whose active paths hold every conv-layer signature and every MB resolution of the space"""
        sp = self.space
        out = []
        for pd in sp.pd_list:
            for d0 in sp.d0_list:
                a = {"ks": [sp.ks_list[0]] * sp.n_mb, "e": [sp.e_list[0]] * sp.n_mb,
                     "d": [d0] + [max(sp.d_list)] * (sp.n_stages - 1), "pixel_d": pd}
                out.append(a)
        return out

    def signatures(self, arch):
        self.space.apply(self.space.net, arch)
        return [s for s, _ in _layer_signatures(self.space.net.active_block_sequence(), self.H, self.W)]

    def build(self, reps=10, verbose=False):
        sp, net = self.space, self.space.net
        st = __import__(__name__.rsplit(".", 2)[0] + ".imagenet_codebase.networks.sr_static", fromlist=["x"])
        blk = __import__(__name__.rsplit(".", 2)[0] + ".imagenet_codebase.networks.proxyless_nets", fromlist=["x"])
        dev = next(net.parameters()).device
        dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[self.dtype]
        convs, mb_res = {}, set()
        for a in self._archs_for_coverage():
            sp.apply(net, a)
            for sig, m in _layer_signatures(net.active_block_sequence(), self.H, self.W):
                if sig[0] == "conv":
                    convs.setdefault(sig, m)
                else:
                    mb_res.add(sig[3:])
        mids = sorted({make_divisible(round(64 * e), 8) for e in sp.e_list})
        was = net.training
        try:
            for sig, m in convs.items():
                if _sig_str(sig) in self.table:
                    continue
                layer = copy.deepcopy(m).eval()
                x = torch.rand((self.N, sig[1], sig[5], sig[6]), device=dev)

                def run(layer=layer, x=x):
                    if dt == torch.float32:
                        return layer(x)
                    with torch.autocast("cuda", dtype=dt):
                        return layer(x)
                self.table[_sig_str(sig)] = _time_us(run, reps) / 1000.0
            for (h, w) in sorted(mb_res):
                x = torch.rand((self.N, 64, h, w), device=dev, dtype=dt)
                for K in sp.ks_list:
                    for mid in mids:
                        sig = ("mb", K, mid, h, w)
                        if _sig_str(sig) in self.table:
                            continue
                        b = blk.MobileInvertedResidualBlock.build_from_config(
                            st.mb_block_config(64, 64, K, mid // 64, mid)).to(dev).eval()
                        self.table[_sig_str(sig)] = _time_us(lambda b=b, x=x: st.run_mb_blocks(x, [b]), reps) / 1000.0
                        if verbose:
                            print("latency %-28s %.4f ms" % (_sig_str(sig), self.table[_sig_str(sig)]), flush=True)
        finally:
            net.train(was)
        return self

    def predict(self, arch):
        """predicted ms of the arch's static net (sum over its layers)"""
        return sum(self.table[_sig_str(s)] for s in self.signatures(arch))

    def to_json(self):
        return {"N": self.N, "H": self.H, "W": self.W, "dtype": self.dtype, "table": self.table}

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.to_json(), f, indent=1, sort_keys=True)

    @staticmethod
    def load(path, space):
        with open(path) as f:
            d = json.load(f)
        return LatencyTable(space, d["N"], d["H"], d["W"], d["dtype"], d["table"])


def measure(static_net, N=1, H=64, W=64, dtype="f32", reps=10):
    """ms per eval forward of a whole static net at (N, 3, H, W) from the library's per-launch events"""
    dev = next(static_net.parameters()).device
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    was = static_net.training
    static_net.eval()
    x = torch.rand((N, 3, H, W), device=dev)

    def run():
        if dt == torch.float32:
            return static_net(x)
        with torch.autocast("cuda", dtype=dt):
            return static_net(x)
    try:
        return _time_us(run, reps) / 1000.0
    finally:
        static_net.train(was)


# ------------------------------------------------------------------------------------------------ the search
class EvolutionSearch(object):
    """evolutionary search under a budget (the shape of upstream's EvolutionFinder): the initial population comes from
    rejection sampling under the budget; every generation keeps the best `parent_ratio` of the population and fills the
    rest with budget-respecting mutants (`mutation_ratio`) and crossovers.  Fitness (higher is better) is cached by
    ArchSpace.key; `evaluated` lists the keys in the order they were first evaluated.  Deterministic for a given seed and
    a deterministic fitness."""

    def __init__(self, space, fitness, efficiency, budget, population_size=100, generations=500, parent_ratio=0.25,
                 mutation_ratio=0.5, mutate_prob=0.1, seed=None, max_tries=10000):
        self.space, self.fitness, self.efficiency, self.budget = space, fitness, efficiency, float(budget)
        self.population_size, self.generations = int(population_size), int(generations)
        self.parent_ratio, self.mutation_ratio, self.mutate_prob = parent_ratio, mutation_ratio, mutate_prob
        self.seed, self.max_tries = seed, max_tries
        self.cache, self.evaluated, self.costs = {}, [], {}

    def _cost(self, arch):
        k = self.space.key(arch)
        if k not in self.costs:
            self.costs[k] = float(self.efficiency(arch))
        return self.costs[k]

    def _draw(self, make):
        for _ in range(self.max_tries):
            a = make()
            if self._cost(a) <= self.budget:
                return a
        raise RuntimeError("no arch within the budget %g after %d draws" % (self.budget, self.max_tries))

    def _score(self, arch):
        k = self.space.key(arch)
        if k not in self.cache:
            self.cache[k] = float(self.fitness(arch))
            self.evaluated.append(k)
        return self.cache[k]

    def run(self):
        import random
        rng = random.Random(self.seed)
        P = self.population_size
        n_par = max(1, int(round(P * self.parent_ratio)))
        n_mut = int(round(P * self.mutation_ratio))
        pop = [self._draw(lambda: self.space.random_sample(rng)) for _ in range(P)]
        scored = [(self._score(a), a) for a in pop]
        history = []
        for g in range(self.generations + 1):
            scored.sort(key=lambda t: -t[0])     # stable: ties keep their order
            best_f, best_a = scored[0]
            history.append({"generation": g, "best_fitness": best_f, "best_arch": copy.deepcopy(best_a),
                            "best_cost": self._cost(best_a),
                            "mean_fitness": sum(f for f, _ in scored) / len(scored), "evaluated": len(self.evaluated)})
            if g == self.generations:
                break
            parents = scored[:n_par]
            children = []
            for _ in range(n_mut):
                p = rng.choice(parents)[1]
                children.append(self._draw(lambda: self.space.mutate(p, self.mutate_prob, rng)))
            for _ in range(P - n_par - n_mut):
                def cross():
                    a, b = rng.choice(parents)[1], rng.choice(parents)[1]
                    return self.space.crossover(a, b, rng)
                children.append(self._draw(cross))
            scored = parents + [(self._score(c), c) for c in children]
        self.history = history
        return copy.deepcopy(history[-1]["best_arch"]), history


# ------------------------------------------------------------------------------------------------ fitness
def bn_buffers(net):
    """copies of every BatchNorm buffer of `net` (running statistics, num_batches_tracked)"""
    out = {}
    for name, m in net.named_modules():
        if isinstance(m, nn.BatchNorm2d):
            for bname, b in m.named_buffers(prefix=name):
                out[bname] = b.clone()
    return out


def restore_bn_buffers(net, snap):
    with torch.no_grad():
        for name, m in net.named_modules():
            if isinstance(m, nn.BatchNorm2d):
                for bname, b in m.named_buffers(prefix=name):
                    b.copy_(snap[bname])
    ops.clear_infer_cache()


def lr_key(net):
    """the data loaders' input for the net's active path: the LR image of its upscale (S4), the HR image (X4)"""
    return "image" if _is_x4(net) else "%dx_down_image" % net.active_upscale()


def psnr_fitness(net, calib_loader, val_loader, run_manager, space, max_calib_batches=None):
    """fitness(arch) = fp32 Y-PSNR on `val_loader` (SRRunManager.validate_batched) of the arch after apply and
    recalibrate_bn on `calib_loader`.  Every BatchNorm buffer of the supernet is snapshot before and restored after each
    evaluation, so the loaded checkpoint is left as it was."""

    def fitness(arch):
        snap = bn_buffers(net)
        try:
            space.apply(net, arch)
            key = lr_key(net)
            recalibrate_bn(net, calib_loader, input_key=key, max_batches=max_calib_batches)
            _, psnr, _ = run_manager.validate_batched(net=net, data_loader=val_loader, input_key=key, graphs=False)
            return psnr
        finally:
            restore_bn_buffers(net, snap)

    return fitness


def quality_fitness(net, calib_loader, val_loader, run_manager, space, max_calib_batches=None, metric="psnr", shave=0):
    """psnr_fitness scored on the GPU: fitness(arch) = the Y-PSNR (`metric="psnr"`) or Y-SSIM (`"ssim"`) of
    SRRunManager.validate_quality -- the HIP metric kernel on the network's output, no host round trip of the images."""
    if metric not in ("psnr", "ssim"):
        raise ValueError("metric is 'psnr' or 'ssim', got %r" % (metric,))

    def fitness(arch):
        snap = bn_buffers(net)
        try:
            space.apply(net, arch)
            key = lr_key(net)
            recalibrate_bn(net, calib_loader, input_key=key, max_batches=max_calib_batches)
            return run_manager.validate_quality(net=net, data_loader=val_loader, input_key=key, graphs=False,
                                                shave=shave)[metric]
        finally:
            restore_bn_buffers(net, snap)

    return fitness
