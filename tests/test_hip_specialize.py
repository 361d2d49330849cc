"""Extracted static sub-networks on the MI355X (`-m gpu`): SRNetS4 / SRNetX4 (imagenet_codebase/networks/sr_static.py)
against the oracle and against the supernet they came from, the fp32 one-kernel eval block (ofasr_mbconv_infer_f32,
csrc/mbfused_f32.hip) against a double-precision restatement of the block, fine-tuning parity, the inference-operand cache
and the export / load round trip of eval_ofa_net_sr.py."""
import ctypes
import importlib
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import amd, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

S4_KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])

# fp32 bar of the whole network against the double oracle: every conv of the path is exact-product fp32 with fp32
# accumulation (K = 64 .. 1600 terms) and BN is folded in fp32, so the error is a few hundred fp32 ulps of the values
# that flow through ~25 layers: |err| <= 2e-4 |ref| + 2e-4 rms(ref)
NET_RTOL = 2e-4
# the bf16 bound of tests/test_hip_mbfused.py (relative L2 of a 16-bit realisation)
BF16_REL_L2 = 8e-3


@pytest.fixture(params=[True, False], ids=["compat", "intended"])
def compat(request):
    nets = amd("elastic_nn.networks")
    saved = (nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING, nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING)
    nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING = request.param
    nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING = request.param
    yield request.param
    nets.OFAMobileNetS4.COMPAT_REFERENCE_INDEXING, nets.OFAMobileNetX4.COMPAT_REFERENCE_INDEXING = saved


def _randomize(net, seed):
    """he_fout weights, perturbed transform matrices, non-trivial BN affine parameters and running statistics"""
    g = torch.Generator().manual_seed(seed)
    net.init_model("he_fout")
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("_matrix"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.6 + 0.7)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) * 0.2 - 0.1)
                m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=g) * 0.2 - 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.6 + 0.7)
    amd("ops").clear_infer_cache()
    return net


def _s4(seed=0):
    dop = amd("elastic_nn.modules.dynamic_op")
    dop.DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    return _randomize(amd("elastic_nn.networks").OFAMobileNetS4(**S4_KW), seed).to(DEV)


def _x4(seed=0):
    dop = amd("elastic_nn.modules.dynamic_op")
    dop.DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    return _randomize(amd("elastic_nn.networks").OFAMobileNetX4(**S4_KW), seed).to(DEV)


def _arch_of(net):
    from oracle import s4_port
    arch = s4_port.Arch()
    n_mb = 16
    arch.ks = [net.blocks[i].mobile_inverted_conv.active_kernel_size for i in range(n_mb)]
    arch.e = [net.blocks[i].mobile_inverted_conv.active_expand_ratio for i in range(n_mb)]
    arch.runtime_depth = list(net.runtime_depth)
    return arch


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _mb_launches():
    C = amd("_C")
    t = C.launch_table()
    return (sum(n for k, n in t.items() if k.startswith("mb_fused_f32_kernel")),
            sum(n for k, n in t.items() if k.startswith("mb_fused_kernel")), t)


ARCHS = [dict(ks=7, e=6, d=4, pixel_d=2), dict(ks=3, e=3, d=2, pixel_d=1), dict(ks=5, e=4, d=3, pixel_d=2), 11, 23]


@pytest.mark.parametrize("arch", ARCHS, ids=lambda a: "sample%d" % a if isinstance(a, int) else
                         "k%(ks)d_e%(e)d_d%(d)d_pd%(pixel_d)d" % a)
def test_static_s4_vs_oracle(arch, compat):
    from oracle import s4_port
    C = amd("_C")
    net = _s4(5)
    if isinstance(arch, int):
        random.seed(arch)
        net.sample_active_subnet()
    else:
        net.set_active_subnet(**arch)
    net.eval()
    sub = net.get_active_subnet(preserve_weight=True).eval()
    n_mb = sub.n_mb
    up = sub.upscale
    assert up == net.active_upscale()
    g = torch.Generator().manual_seed(2)
    lr = torch.rand((2, 3, 14, 18), generator=g)

    # fp32: the new one-kernel block serves every MB block, against the oracle in double on the SUPERNET's state
    C.reset_launch_counts()
    with torch.no_grad():
        y = sub(lr.to(DEV))
    torch.cuda.synchronize()
    n32, n16, table = _mb_launches()
    assert n32 == n_mb and n16 == 0, table
    assert not any(k.startswith(("pw_", "dw_")) for k in table), table
    sd = {k: v.detach().double().cpu() for k, v in net.state_dict().items()}
    ref = s4_port.s4_forward(sd, lr.double(), _arch_of(net), training=False, compat=compat)
    assert tuple(y.shape) == tuple(ref.shape) == (2, 3, 14 * up, 18 * up)
    ref = ref.numpy()
    assert_close(y.cpu().numpy(), ref, NET_RTOL, NET_RTOL * float(np.sqrt(np.mean(ref ** 2))), "static S4 fp32 vs oracle")

    # bf16: the static net against the supernet's own eval output, and both against the oracle
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ys = sub(lr.to(DEV)).float()
        yn = net(lr.to(DEV)).float()
    assert _rel_l2(ys, yn) <= BF16_REL_L2


@pytest.mark.parametrize("arch", [dict(ks=3, e=6, d=2, pixel_d=2), 4, 9], ids=str)
def test_static_x4_vs_supernet(arch, compat):
    net = _x4(8)
    if isinstance(arch, int):
        random.seed(arch)
        net.sample_active_subnet()
    else:
        net.set_active_subnet(**arch)
    net.eval()
    sub = net.get_active_subnet(preserve_weight=True).eval()
    x = torch.rand((2, 3, 32, 40), generator=torch.Generator().manual_seed(6)).to(DEV)
    amd("_C").reset_launch_counts()
    with torch.no_grad():
        y = sub(x)
        y0 = net(x)          # the supernet's fp32 eval: the composite block (its default path is unchanged)
    n32, _, table = _mb_launches()
    assert n32 == len(sub.mb_blocks()), table
    r = y0.cpu().numpy()
    assert_close(y.cpu().numpy(), r, NET_RTOL, NET_RTOL * float(np.sqrt(np.mean(r ** 2))), "static X4 fp32 vs supernet")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ys = sub(x).float()
        yn = net(x).float()
    assert _rel_l2(ys, yn) <= BF16_REL_L2


# ------------------------------------------------------------------------------------- the fp32 block alone
CASES = [
    # (N, H, W, expand, K): the shape list of tests/test_hip_mbfused.py
    (2, 64, 64, 6, 7), (2, 64, 64, 6, 5), (2, 64, 64, 6, 3), (2, 64, 64, 4, 7), (2, 64, 64, 3, 5), (2, 64, 64, 3, 3),
    (3, 32, 32, 4, 7), (1, 48, 48, 6, 3), (1, 30, 31, 6, 7), (1, 45, 62, 4, 5), (2, 17, 20, 3, 3), (1, 16, 16, 6, 7),
    (1, 5, 9, 6, 5), (1, 33, 125, 6, 7), (1, 36, 44, 6, 5), (1, 9, 3, 3, 3), (1, 9, 4, 3, 5), (1, 6, 7, 4, 7),
    (1, 12, 8, 3, 3), (1, 125, 90, 3, 7), (1, 24, 128, 4, 5), (1, 13, 70, 3, 7), (9, 64, 64, 3, 3), (5, 64, 128, 3, 5),
]
_KEEP = []


def _tail(t):
    """a copy of t that ends exactly where its own > 10 MB device allocation ends (the allocator's segment)"""
    nbytes = t.numel() * t.element_size()
    seg = max(12 << 20, (nbytes + (2 << 20) - 1) // (2 << 20) * (2 << 20) + (2 << 20))
    torch.cuda.empty_cache()
    # larger than every free block inside a segment that live tensors of earlier tests still pin: the allocator then has
    # to make a new segment of exactly `seg` bytes, whatever ran before
    free = max([b["size"] for s in torch.cuda.memory_snapshot() for b in s["blocks"] if b["state"] == "inactive"] or [0])
    seg = max(seg, (free + (2 << 20) - 1) // (2 << 20) * (2 << 20) + (2 << 20))
    buf = torch.empty(seg, dtype=torch.uint8, device=DEV)
    out = buf[seg - nbytes:].view(t.dtype).view(t.shape)
    out.copy_(t.to(DEV))
    end = out.data_ptr() + nbytes
    segs = [s for s in torch.cuda.memory_snapshot() if s["address"] <= out.data_ptr() < s["address"] + s["total_size"]]
    assert len(segs) == 1 and segs[0]["address"] + segs[0]["total_size"] == end, "tensor is not at its allocation's end"
    _KEEP.append(buf)
    return out


def _double_block(x, w1, wdw, w2, bns, K, residual):
    """eval-mode MB block in double (oracle/s4_port.py _mb_block semantics, running statistics)"""
    def bn(h, i):
        gm, bt, rm, rv = (t.double().cpu() for t in bns[i])
        return F.batch_norm(h, rm, rv, gm, bt, False, 0.0, 1e-5)
    h = F.relu6(bn(F.conv2d(x, w1), 0))
    h = F.relu6(bn(F.conv2d(h, wdw, None, 1, K // 2, 1, wdw.shape[0]), 1))
    h = bn(F.conv2d(h, w2), 2)
    return h + x if residual else h


@pytest.mark.parametrize("residual", [True, False], ids=["shortcut", "no_shortcut"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d_%dx%d_e%d_k%d" % c)
def test_f32_block_vs_double(case, residual):
    ops, C = amd("ops"), amd("_C")
    st = amd("imagenet_codebase.networks.sr_static")
    blk = amd("imagenet_codebase.networks.proxyless_nets")
    N, Hh, Ww, e, K = case
    mid = 64 * e
    block = blk.MobileInvertedResidualBlock.build_from_config(st.mb_block_config(64, 64, K, e, mid))
    mb = block.mobile_inverted_conv.to(DEV).eval()
    g = torch.Generator().manual_seed(1000 + 10 * K + e)
    cfg, params = mb.composite_args(64, residual)
    w1 = torch.randn((mid, 64, 1, 1), generator=g) * 0.125
    wdw = torch.randn((mid, 1, K, K), generator=g) * (1.0 / K)
    w2 = torch.randn((64, mid, 1, 1), generator=g) * (1.0 / mid ** 0.5)
    bns = [[torch.rand(c, generator=g) * 0.6 + 0.7, torch.rand(c, generator=g) * 0.2 - 0.1,
            torch.rand(c, generator=g) * 0.2 - 0.1, torch.rand(c, generator=g) * 0.6 + 0.7] for c in (mid, mid, 64)]
    x = torch.randn((N, 64, Hh, Ww), generator=g)
    # every input as the tail of its own allocation; the BN modules read their running statistics from those tails
    xt, w1t, wdwt, w2t = _tail(x), _tail(w1), _tail(wdw), _tail(w2)
    bt = [[_tail(t) for t in b] for b in bns]
    for i, bn in enumerate(cfg["bns"]):
        bn.running_mean, bn.running_var = bt[i][2], bt[i][3]
    C.reset_launch_counts()
    with torch.no_grad():
        y = ops.mbconv_infer_f32(xt, cfg, w1t, bt[0][0], bt[0][1], wdwt, bt[1][0], bt[1][1], w2t, bt[2][0], bt[2][1])
    torch.cuda.synchronize()
    assert y is not None and C.launch_count("mb_fused_f32_kernel") == 1
    ref = _double_block(x.double(), w1.double(), wdw.double(), w2.double(), bns, K, residual).numpy()
    # fp32 bar of one block: 64 + K*K + mid exact-product fp32 terms, BN folded in fp32
    assert_close(y.cpu().numpy(), ref, 2e-5, 2e-5 * float(np.sqrt(np.mean(ref ** 2))), "fp32 block")
    assert torch.equal(xt.cpu(), x)            # the input is not written
    _KEEP.clear()


def test_f32_block_supported_scope():
    ops, C = amd("ops"), amd("_C")
    st = amd("imagenet_codebase.networks.sr_static")
    blk = amd("imagenet_codebase.networks.proxyless_nets")
    L = C.lib()
    for (cin, mid, K, dtype, ok) in ((64, 192, 3, torch.float32, 1), (64, 384, 7, torch.float32, 1),
                                     (64, 200, 3, torch.float32, 0), (32, 192, 3, torch.float32, 0),
                                     (64, 192, 3, torch.bfloat16, 0)):
        block = blk.MobileInvertedResidualBlock.build_from_config(st.mb_block_config(cin, 64, K, 3, mid))
        mb = block.mobile_inverted_conv.to(DEV).eval()
        cfg, ps = mb.composite_args(cin, True)
        x = torch.zeros((1, cin, 8, 8), dtype=dtype, device=DEV)
        d = ops._mbconv_desc(x, cfg, *ps, [])
        assert L.ofasr_mbconv_infer_f32_supported(ctypes.byref(d)) == ok, (cin, mid, K, dtype)
    mb.train()
    cfg, ps = mb.composite_args(64, True)
    d = ops._mbconv_desc(torch.zeros((1, 64, 8, 8), device=DEV), cfg, *ps, [])
    assert L.ofasr_mbconv_infer_f32_supported(ctypes.byref(d)) == 0


def test_supernet_fp32_eval_path_unchanged_by_default():
    """the supernet keeps the composite fp32 eval block unless OFASR_MBCONV_F32_INFER_SUPERNET=1"""
    ops = amd("ops")
    assert not ops.F32_INFER_SUPERNET
    net = _s4(1)
    net.set_active_subnet(ks=5, e=4, d=2, pixel_d=2)
    net.eval()
    amd("_C").reset_launch_counts()
    with torch.no_grad():
        net(torch.rand(1, 3, 16, 16, device=DEV))
    n32, _, table = _mb_launches()
    assert n32 == 0, table


# ------------------------------------------------------------------------------------------ fine-tuning
def test_static_finetune_step_matches_supernet(compat):
    """one training step (train-mode BN, Adam) of the static net = the same step of the supernet at that sub-network:
    same loss, same gradients on the active slices, same parameters after the update (fp32 composite bar)"""
    net = _s4(3)
    net.set_active_subnet(ks=7, e=[3, 4, 6, 4] * 4, d=3, pixel_d=2)   # K = max: the static filter is the supernet's slice
    net.train()
    sub = net.get_active_subnet(preserve_weight=True).train()
    g = torch.Generator().manual_seed(4)
    lr = torch.rand((2, 3, 16, 16), generator=g).to(DEV)
    up = sub.upscale
    hr = torch.rand((2, 3, 16 * up, 16 * up), generator=g).to(DEV)
    opt_s = torch.optim.Adam(sub.parameters(), lr=1e-3)
    opt_n = torch.optim.Adam(net.parameters(), lr=1e-3)
    ls, ln = F.mse_loss(sub(lr), hr), F.mse_loss(net(lr), hr)
    ls.backward()
    ln.backward()
    amd("ops").flush_deferred()
    assert abs(ls.item() - ln.item()) <= 1e-5 * abs(ln.item())
    sup = dict(net.named_parameters())
    mb_idx = [idx for stage in range(4) for idx in net.block_group_info[stage][:net.runtime_depth[stage]]]
    assert len(mb_idx) == sub.n_mb
    pairs = []
    for name, p in sub.named_parameters():
        sk = name
        if name.startswith("blocks.") and int(name.split(".")[1]) < sub.n_mb:
            i = int(name.split(".")[1])
            src = mb_idx[i]
            sk = name.replace("blocks.%d." % i, "blocks.%d." % src, 1).replace(".bn.", ".bn.bn.")
            if sk.endswith("conv.weight"):
                sk = sk[:-len("conv.weight")] + "conv.conv.weight"
        elif name.startswith("blocks."):
            i = int(name.split(".")[1]) - sub.n_mb
            src = net.block_group_info[4][i]
            sk = name.replace("blocks.%d." % (i + sub.n_mb), "blocks.%d." % src, 1)
        q = sup[sk]
        sl = tuple(slice(0, s) for s in p.shape)
        pairs.append((name, p, q, sl))
    for name, p, q, sl in pairs:
        ref = q.grad[sl].detach().cpu().numpy()
        assert_close(p.grad.detach().cpu().numpy(), ref, 5e-3, 2e-5 * max(1.0, float(np.abs(ref).max())), name)
    opt_s.step()
    opt_n.step()
    for name, p, q, sl in pairs:
        ref = q[sl].detach().cpu().numpy()
        assert_close(p.detach().cpu().numpy(), ref, 1e-5, 1e-6, name + " after the step")


# ----------------------------------------------------------------------------------- operand cache, export
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_load_state_dict_invalidates_inference_operands(dtype):
    net = _s4(6)
    net.set_active_subnet(ks=5, e=4, d=2, pixel_d=2)
    sub = net.get_active_subnet().eval()
    x = torch.rand(1, 3, 16, 20, device=DEV)

    def run(m):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype != torch.float32):
            return m(x).float().clone()

    y0 = run(sub)
    sd = {k: v.clone() for k, v in sub.state_dict().items()}
    for i in range(sub.n_mb):
        sd["blocks.%d.mobile_inverted_conv.point_linear.bn.weight" % i].mul_(1.5)
        sd["blocks.%d.mobile_inverted_conv.depth_conv.bn.running_var" % i].mul_(2.0)
    sub.load_state_dict(sd)
    y1 = run(sub)
    assert not torch.equal(y0, y1)
    fresh = amd("imagenet_codebase.networks.sr_static").build_static_net(sub.config).to(DEV).eval()
    fresh.load_state_dict(sd)
    amd("ops").clear_infer_cache()
    assert torch.equal(y1, run(fresh))


def test_export_load_round_trip(tmp_path):
    ev = importlib.import_module("eval_ofa_net_sr")
    net = _s4(9)
    net.set_active_subnet(ks=[3, 5, 7, 5] * 4, e=[6, 3, 4, 6] * 4, d=3, pixel_d=1)
    net.eval()
    sub = ev.export_static(net, str(tmp_path)).eval()
    assert sorted(os.listdir(tmp_path)) == sorted(["net_config.json", ev.STATIC_WEIGHTS])
    back = ev.load_static(str(tmp_path)).to(DEV).eval()
    assert back.config == sub.config and back.upscale == net.active_upscale()
    x = torch.rand(2, 3, 12, 16, device=DEV)
    with torch.no_grad():
        a, b, s = sub(x), back(x), net(x)
    assert torch.equal(a, b)
    r = s.cpu().numpy()
    assert_close(b.cpu().numpy(), r, NET_RTOL, NET_RTOL * float(np.sqrt(np.mean(r ** 2))), "exported vs supernet")
    assert ev.input_key(back.upscale) in ("2x_down_image", "4x_down_image")
