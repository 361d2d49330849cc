"""BatchNorm re-calibration on the MI355X (`-m gpu`): the MB block's statistics passes (ofasr_mbconv_recal_f32,
csrc/mbrecal_f32.hip) against a float64 restatement, elastic_nn.utils.recalibrate_bn against the upstream golden and
against set_running_statistics, determinism, what later eval paths see, which kernels run, and the sub-network search
(elastic_nn/search.py) end to end."""
import copy
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import placed
from conftest import amd, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

S4_KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])


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
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.6 + 0.7)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) * 0.2 - 0.1)
                m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=g) * 0.2 - 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.6 + 0.7)
    amd("ops").clear_infer_cache()
    return net


def _net(kind, seed=0):
    amd("elastic_nn.modules.dynamic_op").DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    cls = amd("elastic_nn.networks").OFAMobileNetS4 if kind == "s4" else amd("elastic_nn.networks").OFAMobileNetX4
    return _randomize(cls(**S4_KW), seed).to(DEV)


def _loader(kind, seed, sizes=(3, 2)):
    g = torch.Generator().manual_seed(seed)
    hw = (20, 24) if kind == "s4" else (32, 40)
    return [{"image": torch.rand((n, 3) + hw, generator=g).to(DEV)} for n in sizes]


def _bn_state(net):
    return {k: v.clone() for k, v in net.state_dict().items()}


# ------------------------------------------------------------------------------------------------ 1. the block
def _placed(t, name):
    """a 16-byte aligned copy of t inside a buffer of its own, NaN guard bands on both sides (tests/placed.py, role "in"):
    a read before t[0] or past t[-1] poisons the statistics and the output, and placed.check() demands afterwards that
    guards and payload are unchanged.  Independent of the caching allocator's state."""
    return placed.place(t.to(DEV), 0, "in", name)


def _double_recal_block(x, w1, wdw, w2, bns, K, residual):
    """train-mode MB block in float64: (out, [(mean, biased var) of y1, y2, y3])"""
    stats = []

    def bn(h, i):
        gm, bt = (t.double() for t in bns[i][:2])
        m = h.mean(dim=(0, 2, 3))
        v = ((h - m.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
        stats.append((m, v))
        return F.batch_norm(h, m, v, gm, bt, False, 0.0, 1e-5)
    h = F.relu6(bn(F.conv2d(x, w1), 0))
    h = F.relu6(bn(F.conv2d(h, wdw, None, 1, K // 2, 1, wdw.shape[0]), 1))
    h = bn(F.conv2d(h, w2), 2)
    return (h + x if residual else h), stats


# (N, H, W, mid, K): every mid, K, N and size of the issue's grid appears
BLOCK_CASES = [
    (16, 64, 64, 384, 7), (16, 64, 64, 192, 3), (16, 48, 48, 256, 5), (3, 13, 21, 384, 5), (3, 64, 64, 256, 7),
    (1, 13, 21, 192, 7), (1, 48, 48, 384, 3), (3, 48, 48, 192, 5), (1, 64, 64, 256, 3), (16, 13, 21, 256, 3),
]


@pytest.mark.parametrize("residual", [True, False], ids=["shortcut", "no_shortcut"])
@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: "N%d_%dx%d_mid%d_k%d" % c)
def test_recal_block_vs_double(case, residual):
    ops, C = amd("ops"), amd("_C")
    st = amd("imagenet_codebase.networks.sr_static")
    blk = amd("imagenet_codebase.networks.proxyless_nets")
    N, Hh, Ww, mid, K = case
    block = blk.MobileInvertedResidualBlock.build_from_config(st.mb_block_config(64, 64, K, mid // 64, mid))
    mb = block.mobile_inverted_conv.to(DEV).train()
    g = torch.Generator().manual_seed(2000 + 10 * K + mid)
    cfg, _ = mb.composite_args(64, residual)
    w1 = torch.randn((mid, 64, 1, 1), generator=g) * 0.125
    wdw = torch.randn((mid, 1, K, K), generator=g) * (1.0 / K)
    w2 = torch.randn((64, mid, 1, 1), generator=g) * (1.0 / mid ** 0.5)
    bns = [[torch.rand(c, generator=g) * 0.6 + 0.7, torch.rand(c, generator=g) * 0.2 - 0.1] for c in (mid, mid, 64)]
    x = torch.randn((N, 64, Hh, Ww), generator=g) + 0.5     # an offset mean: the statistics must not cancel
    xt, w1t, wdwt, w2t = _placed(x, "x"), _placed(w1, "w1"), _placed(wdw, "wdw"), _placed(w2, "w2")
    bt = [[_placed(t, "%s%d" % (nm, i + 1)) for t, nm in zip(b, ("gamma", "beta"))] for i, b in enumerate(bns)]
    buffers = [(bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()) for bn in cfg["bns"]]
    acc = tuple(torch.zeros((2, c), dtype=torch.float64, device=DEV) for c in (mid, mid, 64))
    C.reset_launch_counts()
    with torch.no_grad():
        y = ops.mbconv_recal_f32(xt, cfg, w1t, bt[0][0], bt[0][1], wdwt, bt[1][0], bt[1][1], w2t, bt[2][0], bt[2][1],
                                 acc=acc)
    torch.cuda.synchronize()
    assert y is not None
    t = C.launch_table()
    assert sum(n for k, n in t.items() if k.startswith("mb_recal_f32_kernel")) == 3, t
    ref, stats = _double_recal_block(x.double(), w1.double(), wdw.double(), w2.double(), bns, K, residual)
    for i, (m, v) in enumerate(stats):
        got_m = (acc[i][0] / N).cpu().numpy()
        got_v = (acc[i][1] / N).cpu().numpy()
        sd = np.sqrt(v.numpy())
        assert_close(got_m, m.numpy(), 1e-5, 2e-5 * sd + 1e-7, "batch mean of y%d" % (i + 1))
        assert_close(got_v, v.numpy(), 2e-4, 1e-9, "batch variance of y%d" % (i + 1))
    ref = ref.numpy()
    assert_close(y.cpu().numpy(), ref, 1e-4, 1e-4 * float(np.sqrt(np.mean(ref ** 2))), "block output")
    assert torch.equal(xt.cpu(), x)
    for bn, (rm, rv, nb) in zip(cfg["bns"], buffers):   # running statistics are neither read nor written
        assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv)
        assert torch.equal(bn.num_batches_tracked, nb)
    views = [xt, w1t, wdwt, w2t] + [t for b in bt for t in b]
    placed.check_all(*views)   # guards and payloads byte for byte
    for v in views:   # a placed view and its bookkeeping refer to each other: part them, so that the buffers (16 MB for x)
        v.placement.t = None   # go back to the allocator when this test returns and not at some later collection


def test_recal_block_scope():
    ops, C = amd("ops"), amd("_C")
    import ctypes
    st = amd("imagenet_codebase.networks.sr_static")
    blk = amd("imagenet_codebase.networks.proxyless_nets")
    L = C.lib()
    for (cin, mid, K, dtype, ok) in ((64, 192, 3, torch.float32, 1), (64, 384, 7, torch.float32, 1),
                                     (64, 200, 3, torch.float32, 0), (32, 192, 3, torch.float32, 0),
                                     (64, 192, 3, torch.bfloat16, 0)):
        block = blk.MobileInvertedResidualBlock.build_from_config(st.mb_block_config(cin, 64, K, 3, mid))
        mb = block.mobile_inverted_conv.to(DEV).train()
        cfg, ps = mb.composite_args(cin, True)
        d = ops._mbconv_desc(torch.zeros((1, cin, 8, 8), dtype=dtype, device=DEV), cfg, *ps, [])
        assert L.ofasr_mbconv_recal_f32_supported(ctypes.byref(d)) == ok, (cin, mid, K, dtype)


# ---------------------------------------------------------------------------------------------- 2. the golden
def test_recalibrate_bn_golden(golden):
    """the same sub-network, batches and tolerance as test_hip_network.py::test_bn_recalibration_golden"""
    from detfill import fill_state_dict
    g = golden("calibration.npz")
    eutils = amd("elastic_nn.utils")
    amd("elastic_nn.modules.dynamic_op").DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    net = amd("elastic_nn.networks").OFAMobileNetS4(**S4_KW)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state_dict(shapes, "s4").items()})
    net = net.to(DEV).eval()
    net.set_active_subnet(ks=5, e=4, d=3, pixel_d=2)
    before = {k: v.clone() for k, v in net.state_dict().items() if "running_" in k}
    loader = [{"image": torch.from_numpy(g["b0"]).to(DEV)}, {"image": torch.from_numpy(g["b1"]).to(DEV)}]
    info = eutils.recalibrate_bn(net, loader)
    assert info["mb_fallback"] == 0 and info["mb_kernel"] > 0 and info["images"] == g["b0"].shape[0] + g["b1"].shape[0]
    changed = 0
    for k, v in net.state_dict().items():
        if "running_mean" in k or "running_var" in k:
            ref = g[k]
            assert_close(v.cpu().numpy(), ref, 2e-4, 2e-5 * max(1.0, float(np.abs(ref).max())), k)
            changed += int(not torch.equal(v, before[k]))
    assert changed > 40


# ------------------------------------------------------------------------- 3. against set_running_statistics
def _check_against_aten(net, loader, train_mode):
    eutils = amd("elastic_nn.utils")
    ref = copy.deepcopy(net)
    eutils.set_running_statistics(ref, loader)
    net.train(train_mode)
    before = _bn_state(net)
    params = {k: p.clone() for k, p in net.named_parameters()}
    info = eutils.recalibrate_bn(net, loader)
    assert net.training == train_mode
    assert info["mb_fallback"] == 0 and info["batches"] == len(loader)
    now, want = net.state_dict(), ref.state_dict()
    moved = 0
    for k, v in now.items():
        if k.endswith("num_batches_tracked"):
            assert torch.equal(v, before[k]), k
        elif "running_" in k:
            w = want[k]
            scale = max(1.0, float(w.abs().max()))
            assert_close(v.cpu().numpy(), w.cpu().numpy(), 2e-4, 2e-5 * scale, k)
            # channels set_running_statistics left alone (inactive) are untouched here too
            same = before[k] == w
            assert torch.equal(v[same], before[k][same]), k
            moved += int(not torch.equal(v, before[k]))
    assert moved > 10
    for k, p in net.named_parameters():
        assert torch.equal(p, params[k]), k
    return info


@pytest.mark.parametrize("kind", ["s4", "x4"])
@pytest.mark.parametrize("seed", [3, 8])
def test_recalibrate_bn_matches_set_running_statistics(kind, seed, compat):
    net = _net(kind, seed)
    random.seed(seed)
    net.sample_active_subnet()
    _check_against_aten(net, _loader(kind, seed), train_mode=bool(seed % 2))


def _mb_bns(mb):
    return [s.bn.bn if hasattr(s.bn, "bn") else s.bn for s in (mb.inverted_bottleneck, mb.depth_conv, mb.point_linear)]


def _s4_path_bns(net):
    """BatchNorms of an S4 supernet's active path / of an SRNetS4, in execution order"""
    if hasattr(net, "active_block_sequence"):
        out = []
        for kind, m in net.active_block_sequence():
            out += _mb_bns(m) if kind == "mb" else [m.bn]
        return out
    mbs = [_mb_bns(b.mobile_inverted_conv) for b in net.blocks[:net.n_mb]]
    return ([net.dec_first_conv_block.bn] + [bn for t in mbs for bn in t] + [c.bn for c in net.dec_final_conv_blocks]
            + [b.bn for b in net.blocks[net.n_mb:]] + [net.dec_final_output_conv_block.bn])


def test_recalibrate_bn_static_net(compat):
    """an extracted SRNetS4 re-calibrates to what set_running_statistics gives its supernet (set_running_statistics
    itself does not reach the static MB blocks, which run on the composite kernels)"""
    eutils = amd("elastic_nn.utils")
    net = _net("s4", 5)
    net.set_active_subnet(ks=[3, 5, 7, 5] * 4, e=[3, 4, 6, 4] * 4, d=[2, 3, 4, 3], pixel_d=2)
    static = net.get_active_subnet().eval()
    loader = _loader("s4", 5)
    eutils.set_running_statistics(net, loader)
    nbt = {k: v.clone() for k, v in static.state_dict().items() if k.endswith("num_batches_tracked")}
    info = eutils.recalibrate_bn(static, loader)
    assert info["mb_fallback"] == 0 and info["mb_kernel"] == static.n_mb * len(loader) and not static.training
    got, want = _s4_path_bns(static), _s4_path_bns(net)
    assert len(got) == len(want) > 10
    for i, (a, b) in enumerate(zip(got, want)):
        c = a.num_features
        for name in ("running_mean", "running_var"):
            w = getattr(b, name)[:c]
            assert_close(getattr(a, name).cpu().numpy(), w.cpu().numpy(), 2e-4, 2e-5 * max(1.0, float(w.abs().max())),
                         "BN %d %s" % (i, name))
    for k, v in static.state_dict().items():
        if k in nbt:
            assert torch.equal(v, nbt[k]), k


def test_recalibrate_bn_fallback_path_matches():
    """the per-op fallback (blocks outside the one-kernel scope) computes the same statistics"""
    ops, eutils = amd("ops"), amd("elastic_nn.utils")
    net = _net("s4", 4)
    net.set_active_subnet(ks=5, e=4, d=2, pixel_d=1)
    loader = _loader("s4", 4)
    a = copy.deepcopy(net)
    eutils.recalibrate_bn(net, loader)
    ops.RECAL_MB_KERNEL = False
    try:
        info = eutils.recalibrate_bn(a, loader)
    finally:
        ops.RECAL_MB_KERNEL = True
    assert info["mb_fallback"] > 0 and info["mb_kernel"] == 0
    for (k, v), (_, w) in zip(net.state_dict().items(), a.state_dict().items()):
        if "running_" in k:
            assert_close(v.cpu().numpy(), w.cpu().numpy(), 1e-4, 1e-5 * max(1.0, float(w.abs().max())), k)


# --------------------------------------------------------------------------------------------- 4. determinism
def test_recalibrate_bn_bit_identical():
    eutils = amd("elastic_nn.utils")
    net = _net("x4", 6)
    random.seed(6)
    net.sample_active_subnet()
    loader = _loader("x4", 6)
    eutils.recalibrate_bn(net, loader)
    first = _bn_state(net)
    eutils.recalibrate_bn(net, loader)
    for k, v in net.state_dict().items():
        assert torch.equal(v, first[k]), k


# -------------------------------------------------------------------------------------- 5. later eval paths
def test_eval_paths_see_new_statistics():
    eutils, graphed = amd("elastic_nn.utils"), amd("graphed")
    net = _net("s4", 7).eval()
    net.set_active_subnet(ks=5, e=4, d=3, pixel_d=2)
    x = _loader("s4", 70, sizes=(2,))[0]["image"]
    ge = graphed.GraphedEval(net, autocast_dtype=torch.bfloat16)
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y0 = net(x).float().clone()
        ge(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):   # autocast around the calibration changes nothing
            eutils.recalibrate_bn(net, _loader("s4", 7))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y1 = net(x).float().clone()
        z1 = ge(x).float().clone()
    fresh = _net("s4", 7).eval()
    fresh.set_active_subnet(ks=5, e=4, d=3, pixel_d=2)
    fresh.load_state_dict(net.state_dict())
    ge2 = graphed.GraphedEval(fresh, autocast_dtype=torch.bfloat16)
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y2 = fresh(x).float()
        z2 = ge2(x).float()
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, y2) and torch.equal(z1, z2)


# --------------------------------------------------------------------------------------- 6. which kernels run
def test_no_aten_batch_norm_or_vendor_conv():
    eutils, C = amd("elastic_nn.utils"), amd("_C")
    from torch.profiler import ProfilerActivity, profile
    net = _net("x4", 9)
    random.seed(9)
    net.sample_active_subnet()
    loader = _loader("x4", 9)
    eutils.recalibrate_bn(net, loader)     # warm-up outside the profile
    torch.cuda.synchronize()
    C.reset_launch_counts()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        eutils.recalibrate_bn(net, loader)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert any("mb_recal_f32_kernel" in n for n in names), "the profiler saw no library kernel"
    bad = [n for n in set(names) if any(s in n.lower() for s in ("batch_norm", "batchnorm", "miopen", "naive_conv",
                                                                  "igemm", "sp3asm", "cudnn"))]
    assert not bad, bad
    ops_seen = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU}
    assert not any(n in ops_seen for n in ("aten::batch_norm", "aten::convolution", "aten::conv2d")), ops_seen
    t = C.launch_table()
    assert sum(n for k, n in t.items() if k.startswith("mb_recal_f32_kernel")) > 0


# ------------------------------------------------------------------------------------------------- 7. search
def test_search_end_to_end(tmp_path):
    import search_ofa_net_sr as cli
    import eval_ofa_net_sr as ev
    search = amd("elastic_nn.search")
    rmod = amd("imagenet_codebase.run_manager")
    out = str(tmp_path / "export")
    args = ["--net", "s4", "--budget-gmacs", "12", "--synthetic", "--calib-images", "8", "--calib-batch", "4",
            "--population", "4", "--generations", "2", "--seed", "1", "--image-size", "64", "--lr-size", "64", "64",
            "--test-sizes", "64x64,48x80", "--path", str(tmp_path / "run"), "--export", out]
    res = cli.main(args)
    net, es = res["net"], res["search"]
    assert res["gmacs"] <= 12 and all(es.costs[k] <= 12 for k in es.evaluated)
    after = search.bn_buffers(net)
    assert set(after) == set(res["bn_before"])
    for k, v in after.items():
        assert torch.equal(v, res["bn_before"][k]), k
    rec = json.load(open(os.path.join(out, "search.json")))
    assert rec["arch"] == res["best"] and len(rec["history"]) == 3
    # the export, loaded fresh and validated the way eval_ofa_net_sr.py --static does, gives the recorded PSNR
    static = ev.load_static(out)
    cfg = rmod.Div2K_SetXXRunConfig(n_epochs=1, init_lr=1e-3, opt_type="adam", no_decay_keys="bn#bias",
                                    label_smoothing=0.0, train_batch_size=1, test_batch_size=1, image_size=256,
                                    test_sizes=[(64, 64), (48, 80)], n_train_batches=1, allow_synthetic=True)
    mgr = rmod.SRRunManager(str(tmp_path / "eval"), static, cfg, init=False, mix_prec="f32", num_gpus=1)
    _, psnr, _ = mgr.validate_batched(is_test=True, input_key=ev.input_key(static.upscale))
    assert abs(psnr - rec["psnr"]) <= 1e-3, (psnr, rec["psnr"])


# ------------------------------------------------------------------------------------------ 8. latency table
def test_latency_table(tmp_path):
    search = amd("elastic_nn.search")
    net = _net("s4", 12).eval()
    space = search.ArchSpace(net, 4)
    table = search.LatencyTable(space, 1, 32, 32).build(reps=3)
    path = str(tmp_path / "lat.json")
    table.save(path)
    table = search.LatencyTable.load(path, space)
    rng = random.Random(12)
    for i in range(3):
        a = space.random_sample(rng)
        for s in table.signatures(a):
            assert search._sig_str(s) in table.table, s
        pred = table.predict(a)
        space.apply(net, a)
        meas = search.measure(net.get_active_subnet().eval(), 1, 32, 32, reps=3)
        print("latency table: predicted %.4f ms, measured %.4f ms" % (pred, meas))
        assert pred > 0 and meas > 0
        assert 0.2 < pred / meas < 5.0   # loose: timings on a shared card are noisy
