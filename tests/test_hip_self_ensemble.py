"""Geometric self-ensemble on the MI355X (`-m gpu`): the D4 kernels (csrc/d4.hip: ofasr_d4_apply / ofasr_d4_accumulate)
against the torch definition (upscale.d4_transform / d4_inverse) bit for bit, ops.self_ensemble on a real static network,
its equivariance, tiled = whole-image parity of TiledUpscaler(self_ensemble=8), which ops the ensemble runs,
SRRunManager.validate_quality(self_ensemble=8) and the command line."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, amd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# single element, below a tile, the transposing kernel's 64-tile in part / exactly / ragged / several tiles
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 3, 32, 32), (3, 3, 33, 65), (1, 64, 64, 48), (1, 3, 130, 257)]
SMALL = dict(ks=3, e=3, d=2, pixel_d=1)
_KEEP = []


def _rand(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 0.5).to(dtype)


def _ensemble_ref(ys, k, inverse):
    """the definition: (1 / k) * ((((v_0 + v_1) + v_2) + ...) + v_{k-1}), v_t = float32(T_t^{-1}(y_t)), fp32 adds"""
    s = inverse(ys[0], 0).float()
    for t in range(1, k):
        s = s + inverse(ys[t], t).float()
    return s * (1.0 / k)


def _offset_view(t, pad=1):
    """a contiguous copy of t whose base pointer is `pad` elements into a larger buffer"""
    buf = torch.empty(pad + t.numel(), dtype=t.dtype, device=DEV)
    out = buf[pad:].view(t.shape)
    out.copy_(t)
    return out


def _tail(t):
    """a copy of t that ends exactly where its own > 10 MB device allocation ends (the allocator's segment): a read
    past its end leaves the allocation"""
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


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_d4_apply_equals_d4_transform(shape, dtype):
    ops, up = amd("ops"), amd("upscale")
    host = _rand(shape, dtype, sum(shape))
    x = host.to(DEV)
    for t in range(8):
        y = ops.d4_apply(x, t)
        ref = up.d4_transform(host, t)
        assert y.dtype == dtype and y.shape == ref.shape and y.is_contiguous()
        assert torch.equal(y.cpu(), ref), t
    assert torch.equal(x.cpu(), host)          # the source is left alone
    # `out`: written in place and returned
    out = torch.empty(up.d4_transform(host, 5).shape, dtype=dtype, device=DEV)
    assert ops.d4_apply(x, 5, out=out) is out and torch.equal(out.cpu(), up.d4_transform(host, 5))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("place", ["offset", "tail"])
def test_d4_apply_unaligned_base_and_end_of_allocation(place, dtype):
    """a base pointer one element off (no vector access is legal) / every input at the very end of its allocation"""
    ops, up = amd("ops"), amd("upscale")
    for shape in [(2, 3, 5, 7), (1, 3, 32, 32), (3, 3, 33, 65), (1, 3, 36, 64)]:
        host = _rand(shape, dtype, 7 + sum(shape))
        x = _offset_view(host.to(DEV)) if place == "offset" else _tail(host)
        for t in range(8):
            ref = up.d4_transform(host, t)
            if place == "offset":
                out = _offset_view(torch.zeros(ref.shape, dtype=dtype, device=DEV))
                ops.d4_apply(x, t, out=out)
            else:
                out = ops.d4_apply(x, t)
            assert torch.equal(out.cpu(), ref), (shape, t)
    torch.cuda.synchronize()
    del _KEEP[:]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_d4_accumulate_equals_definition(shape, dtype):
    ops, up = amd("ops"), amd("upscale")
    N, C, H, W = shape
    ys = [_rand((N, C, W, H) if t & 4 else shape, dtype, 100 * t + sum(shape)) for t in range(8)]
    dev = [y.to(DEV) for y in ys]
    for k in (2, 4, 8):
        ref = _ensemble_ref(ys, k, up.d4_inverse)
        runs = []
        for _ in range(2):
            acc = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)   # `first` must not read it
            for t in range(k):
                assert ops.d4_accumulate(dev[t], t, acc, t == 0, 1.0 / k if t == k - 1 else 1.0) is acc
            runs.append(acc.cpu())
        assert torch.equal(runs[0], ref), k
        assert torch.equal(runs[0], runs[1]), k


@pytest.mark.parametrize("place", ["offset", "tail"])
def test_d4_accumulate_unaligned_base_and_end_of_allocation(place):
    ops, up = amd("ops"), amd("upscale")
    for shape, dtype in [((2, 3, 5, 7), torch.bfloat16), ((3, 3, 33, 65), torch.float32), ((1, 3, 36, 64), torch.float16),
                         ((1, 3, 36, 64), torch.float32)]:
        N, C, H, W = shape
        ys = [_rand((N, C, W, H) if t & 4 else shape, dtype, 11 * t + sum(shape)) for t in range(8)]
        ref = _ensemble_ref(ys, 8, up.d4_inverse)
        if place == "offset":
            acc = _offset_view(torch.zeros(shape, dtype=torch.float32, device=DEV))
            dev = [_offset_view(y.to(DEV)) for y in ys]
        else:
            acc = _tail(torch.zeros(shape, dtype=torch.float32))
            dev = [_tail(y) for y in ys]
        for t in range(8):
            ops.d4_accumulate(dev[t], t, acc, t == 0, 0.125 if t == 7 else 1.0)
        assert torch.equal(acc.cpu(), ref), (shape, dtype)
    torch.cuda.synchronize()
    del _KEEP[:]


def test_ops_argument_checks_on_gpu():
    ops = amd("ops")
    x = torch.zeros(1, 3, 6, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.d4_apply(x[..., ::2], 1)                       # not contiguous
    with pytest.raises(ValueError):
        ops.d4_apply(x, 8)
    with pytest.raises(ValueError):
        ops.d4_apply(x, 4, out=torch.empty_like(x))        # t = 4 writes [1, 3, 8, 6]
    with pytest.raises(ValueError):
        ops.d4_apply(x, 1, out=x)
    with pytest.raises(ValueError):
        ops.d4_accumulate(x, 4, torch.zeros_like(x), True, 1.0)
    with pytest.raises(ValueError):
        ops.d4_accumulate(x, 0, torch.zeros_like(x, dtype=torch.bfloat16), True, 1.0)
    with pytest.raises(ValueError):
        ops.self_ensemble(lambda v: v, x, 3)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_skip_add_equals_aten_add(dtype):
    """the static networks' long skip at inference time (ops.skip_add -> ofasr_add): the bits of a + b"""
    ops, C = amd("ops"), amd("_C")
    for shape, pad in [((1, 1, 1, 1), 0), ((2, 3, 5, 7), 0), ((1, 64, 33, 65), 0), ((1, 5, 9, 11), 1), ((1, 64, 40, 56), 0)]:
        a = (_rand(shape, torch.float32, 1 + sum(shape)) * 3).to(dtype).to(DEV)
        b = (_rand(shape, torch.float32, 2 + sum(shape)) * 0.01).to(dtype).to(DEV)
        if pad:
            a, b = _offset_view(a, pad), _offset_view(b, pad)
        ref = a + b
        C.reset_launch_counts()
        with torch.no_grad():
            y = ops.skip_add(a, b)
        assert C.launch_count("add_kernel") == 1
        assert y.dtype == dtype and torch.equal(y, ref), (shape, pad)
    # with gradients it is the autograd add
    a = torch.rand(1, 2, 3, 4, device=DEV, requires_grad=True)
    C.reset_launch_counts()
    y = ops.skip_add(a, torch.ones_like(a))
    assert y.requires_grad and C.launch_count("add_kernel") == 0


# ---------------------------------------------------------------------------------------------- networks
def _static(kind, setting):
    nets = amd("elastic_nn.networks")
    st = amd("imagenet_codebase.networks.sr_static")
    net = nets.OFAMobileNetS4(**KW) if kind == "s4" else nets.OFAMobileNetX4(**KW)
    net.set_active_subnet(**setting)
    return st.build_static_net(net.get_active_net_config())


def _randomize(net, seed, branch_gain=1.0, lean=0.02):
    """he_fout weights whose spatial taps lean to the top-left (an asymmetric network: its outputs under the 8 transforms
    really differ), non-trivial BN parameters and statistics; the output is then scaled to about unit spread around 0.5
    so that the uint8 image is not all clamped"""
    g = torch.Generator().manual_seed(seed)
    net.init_model("he_fout")
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d) and m.kernel_size[1] > 1:
                k = m.kernel_size[1]
                prof = torch.full((k,), float(lean))
                prof[0] = 1.0
                n0 = m.weight.flatten(1).norm(dim=1)
                m.weight.mul_((prof.view(k, 1) * prof.view(1, k)) * (1.0 + 0.3 * torch.rand(m.weight.shape, generator=g)))
                m.weight.mul_((n0 / m.weight.flatten(1).norm(dim=1)).view(-1, 1, 1, 1))
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.6 + 0.7)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) * 0.2 - 0.1)
                m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=g) * 0.2 - 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.6 + 0.7)
        for b in net.mb_blocks():
            b.mobile_inverted_conv.point_linear.bn.weight.mul_(branch_gain)
            b.mobile_inverted_conv.point_linear.bn.bias.mul_(branch_gain)
    net = net.to(DEV).eval()
    x = torch.rand(1, 3, 64, 64, generator=g).to(DEV)
    with torch.no_grad():
        y = net(x).float()
    head = net.dec_final_output_conv_block
    with torch.no_grad():
        s = float(y.std()) / 0.3
        head.conv.weight.div_(s)
        if head.use_bn:
            head.bn.running_mean.div_(s)
            head.bn.bias.add_(0.5 - float(y.mean()) / s)
    amd("ops").clear_infer_cache()
    return net


def _image(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(3, H // 8 + 2, W // 8 + 2, generator=g)
    smooth = torch.nn.functional.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0]
    img = (smooth * 200 + torch.rand(3, H, W, generator=g) * 55).clamp(0, 255).to(torch.uint8)
    return img.permute(1, 2, 0).contiguous()


@pytest.fixture(scope="module")
def small_net():
    return _randomize(_static("s4", SMALL), 1)


def _forward(net, dtype):
    def fn(x):
        with torch.no_grad(), torch.autocast("cuda", dtype=dtype if dtype != torch.float32 else torch.bfloat16,
                                            enabled=dtype != torch.float32):
            return net(x)
    return fn


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_self_ensemble_equals_torch_composition(small_net, dtype):
    ops, up = amd("ops"), amd("upscale")
    fn = _forward(small_net, dtype)
    x = _rand((1, 3, 40, 56), torch.float32, 3).clamp(0, 1).to(DEV)
    got = ops.self_ensemble(fn, x, 8)
    ys = [fn(up.d4_transform(x, t)) for t in range(8)]
    assert all(y.dtype == dtype for y in ys)           # a 16-bit forward is rounded once per transform
    ref = _ensemble_ref(ys, 8, up.d4_inverse)
    s = small_net.upscale
    assert got.dtype == torch.float32 and got.shape == (1, 3, 40 * s, 56 * s)
    assert torch.equal(got, ref)
    # the members really differ (the network is not symmetric), and k = 1 is the plain forward
    assert not torch.equal(up.d4_inverse(ys[1], 1), ys[0]) and not torch.equal(up.d4_inverse(ys[4], 4), ys[0])
    assert torch.equal(ops.self_ensemble(fn, x, 1), ys[0].float())
    for k in (2, 4):
        assert torch.equal(ops.self_ensemble(fn, x, k), _ensemble_ref(ys, k, up.d4_inverse)), k


@pytest.mark.parametrize("s", [1, 4, 7])
def test_equivariance(small_net, s):
    """ens_8(net, T_s(x)) and T_s(ens_8(net, x)) forward the same 8 inputs and differ only in the order of the 7 adds.
    Bound: each of the 7 fp32 adds rounds a partial sum of magnitude <= 8 M by at most 2^-24 * 8 M (half an ulp), the
    scale by 1 / 8 is exact, so one ensemble is within 7 * 2^-24 * M of the exact mean and two orders within
    14 * 2^-24 * M of each other; M = max_t max |y_t|."""
    ops, up = amd("ops"), amd("upscale")
    fn = _forward(small_net, torch.float32)
    x = _rand((1, 3, 40, 56), torch.float32, 5).clamp(0, 1).to(DEV)
    xs = up.d4_transform(x, s)

    def key(v):
        return (tuple(v.shape), v.cpu().numpy().tobytes())

    a_in = {key(up.d4_transform(x, t)) for t in range(8)}
    b_in = {key(up.d4_transform(xs, t)) for t in range(8)}
    assert len(a_in) == 8 and a_in == b_in
    ys = [fn(up.d4_transform(x, t)) for t in range(8)]
    M = max(float(y.abs().max()) for y in ys)
    bound = 14 * 2.0 ** -24 * M
    lhs = ops.self_ensemble(fn, xs, 8)
    rhs = up.d4_transform(ops.self_ensemble(fn, x, 8), s)
    d = float((lhs - rhs).abs().max())
    print("s", s, "M", M, "delta", d, "bound", bound)
    assert lhs.shape == rhs.shape and d <= bound, (d, bound)
    # one inverse replaced by the wrong one of the same shape (a host-side swap in the torch statement) is seen
    wrong = dict((t, t) for t in range(8))
    wrong[1] = 2
    bad = _ensemble_ref(ys, 8, lambda y, t: up.d4_inverse(y, wrong[t]))
    d_bad = float((lhs - up.d4_transform(bad, s)).abs().max())
    assert d_bad > 25 * bound, (d_bad, bound)


@pytest.mark.parametrize("kind", ["s4", "x4"])
def test_tiled_ensemble_equals_whole(kind, small_net):
    up = amd("upscale")
    net = small_net if kind == "s4" else _randomize(_static("x4", SMALL), 1)
    core = 48 if kind == "s4" else 32
    tu = up.TiledUpscaler(net, core=core, mix_prec="f32", self_ensemble=8)
    H, W = 187, 301
    if kind == "x4":
        H, W = tu.halo * 2 + 3 * 32, tu.halo * 2 + 5 * 32
    img = _image(H, W, 3)
    plan = tu.plan(H, W)
    assert len(plan) >= 6 and plan.win_h % 8 == 0 and plan.win_w % 8 == 0
    assert any(wy + plan.win_h == H and cy > wy + tu.halo for (wy, _, cy, _, _, _) in plan.windows)   # shifted windows
    whole = tu.upscale_float(img, whole=True)
    tiled = tu.upscale_float(img)
    assert whole.shape == (3, H * tu.scale, W * tu.scale) and whole.dtype == torch.float32
    err = (tiled - whole).abs().max().item()
    print(kind, "tiled vs whole", err)
    assert err <= 2e-5, err
    assert float(whole.std()) > 0.05
    # two window orientations: two captured graphs at most for the tiled path
    assert tu.graphed.captures <= 4          # whole image + windows, each in two orientations
    u_whole = tu.upscale(img, whole=True)
    u_tiled = tu.upscale(img)
    d = (u_tiled.int() - u_whole.int()).abs()
    assert int(d.max()) <= 1
    assert int((d > 0).sum()) <= 1e-4 * d.numel()
    # the ensemble is not the plain output
    plain = up.TiledUpscaler(net, core=core, mix_prec="f32")
    assert not torch.equal(plain.upscale(img), u_tiled)


def test_tiled_graph_count_and_k1_identity(small_net):
    up = amd("upscale")
    img = _image(187, 301, 3)
    base = up.TiledUpscaler(small_net, core=48).upscale(img)
    one = up.TiledUpscaler(small_net, core=48, self_ensemble=1)
    assert one.plan(187, 301).windows == up.TiledUpscaler(small_net, core=48).plan(187, 301).windows
    assert torch.equal(one.upscale(img), base)
    for k, graphs in ((4, 1), (8, 2)):
        tu = up.TiledUpscaler(small_net, core=48, self_ensemble=k)
        tu.upscale(img)
        assert tu.graphed.captures == graphs, (k, tu.graphed.captures)


# ---------------------------------------------------------------------------------------------- routing
def test_ensemble_runs_no_aten_flip_stack_mean_add(small_net):
    from torch.profiler import ProfilerActivity, profile
    up = amd("upscale")
    tu = up.TiledUpscaler(small_net, core=48, graphed=False, self_ensemble=8)
    img = _image(120, 140, 6).to(DEV)
    tu.upscale(img)                     # warm-up outside the profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        tu.upscale(img)
        torch.cuda.synchronize()
    ops_seen = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU}
    bad = [n for n in ops_seen if n in ("aten::flip", "aten::rot90", "aten::stack", "aten::mean", "aten::add",
                                        "aten::convolution", "aten::conv2d", "aten::_convolution", "aten::batch_norm",
                                        "aten::pixel_shuffle", "aten::pixel_unshuffle") or "upsample" in n]
    assert not bad, bad
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert any("d4_flip_kernel" in n for n in names) and any("d4_tr_kernel" in n for n in names), \
        "the profiler saw no d4 kernel"
    names = [n.replace("ofasr::", "") for n in names]
    # both calls, in both kernels: apply (ACC = false) and accumulate (ACC = true)
    for kern in ("d4_flip_kernel", "d4_tr_kernel"):
        assert any(kern + "<float, false" in n for n in names), "no apply launch of " + kern
        assert any(kern + "<float, true" in n for n in names), "no accumulate launch of " + kern


# ---------------------------------------------------------------------------------------------- evaluation
def test_validate_quality_self_ensemble(tmp_path, small_net):
    ops, rm, utils = amd("ops"), amd("imagenet_codebase.run_manager"), amd("utils")
    s = small_net.upscale
    key = "%dx_down_image" % s
    cfg = rm.SyntheticSRRunConfig(n_epochs=1, init_lr=1e-3, train_batch_size=1, test_batch_size=1, image_size=64,
                                  n_train_batches=1, test_sizes=[(96, 128), (64, 80), (96, 128)])
    mgr = rm.SRRunManager(str(tmp_path), small_net, cfg, init=False, num_gpus=1)
    small_net.eval()
    q = mgr.validate_quality(is_test=True, input_key=key, graphs=False, self_ensemble=8, max_batch=1)
    assert q["calls"] == 3 * 8
    fn = _forward(small_net, torch.float32)
    items = [b for b in cfg.test_loader]
    order = [t for g in utils.bucket_by_size(items, key=lambda it: it[key]) for t in g]
    assert len(order) == 3
    for i, b in enumerate(order):
        out = ops.self_ensemble(fn, b[key].to(DEV).contiguous(), 8)
        sse, ssim, count = ops.quality_y(out, b["image"].to(DEV))
        assert q["psnr_per_image"][i] == utils.psnr_from_sse(int(sse[0]), count), i
        assert q["ssim_per_image"][i] == float(ssim[0]), i
    # batched buckets give per-image numbers too, and the ensemble is not the plain score
    qb = mgr.validate_quality(is_test=True, input_key=key, graphs=False, self_ensemble=8)
    assert qb["calls"] == 2 * 8 and len(qb["psnr_per_image"]) == 3
    plain = mgr.validate_quality(is_test=True, input_key=key, graphs=False)
    one = mgr.validate_quality(is_test=True, input_key=key, graphs=False, self_ensemble=1)
    assert one == plain and plain["ssim_per_image"] != q["ssim_per_image"]
    # with graphs: the transformed inputs of all buckets in one replay, the same numbers as the eager pass
    g = mgr.validate_quality(is_test=True, input_key=key, graphs=True, self_ensemble=8)
    assert g["psnr_per_image"] == qb["psnr_per_image"] and g["ssim_per_image"] == qb["ssim_per_image"]
    assert mgr.graphed(small_net).replays == 1
    with pytest.raises(ValueError):
        mgr.validate_quality(is_test=True, input_key=key, self_ensemble=3)


# ---------------------------------------------------------------------------------------------- command line
def test_cli_self_ensemble(tmp_path):
    from PIL import Image
    up = amd("upscale")
    net = _randomize(_static("s4", SMALL), 4)
    d = tmp_path / "net"
    d.mkdir()
    (d / "net_config.json").write_text(json.dumps(net.config))
    torch.save({"state_dict": {k: v.cpu() for k, v in net.state_dict().items()}}, str(d / "static_state_dict.pth"))
    rng = np.random.RandomState(0)
    a = rng.randint(0, 256, (90, 70, 3)).astype(np.uint8)
    b = rng.randint(0, 256, (11, 13, 3)).astype(np.uint8)
    Image.fromarray(a, "RGB").save(str(tmp_path / "a.png"))
    Image.fromarray(b, "RGB").save(str(tmp_path / "b.png"))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "upscale_ofa_net_sr.py"), "--static", str(d), "--out", str(out),
           "--self-ensemble", "4", "--core", "32", str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "self-ensemble x4" in r.stdout and "MP/s" in r.stdout
    tu = up.TiledUpscaler(net, core=32, self_ensemble=4)
    plain = up.TiledUpscaler(net, core=32)
    s = tu.scale
    for name, arr in (("a", a), ("b", b)):
        got = np.asarray(Image.open(str(out / (name + ".png"))))
        assert got.shape == (arr.shape[0] * s, arr.shape[1] * s, 3)
        assert np.array_equal(got, tu.upscale(torch.from_numpy(arr)).cpu().numpy())
    assert not np.array_equal(np.asarray(Image.open(str(out / "a.png"))), plain.upscale(torch.from_numpy(a)).cpu().numpy())
