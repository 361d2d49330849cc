"""The Y-PSNR / Y-SSIM metric on the MI355X (`-m gpu`): the kernels of csrc/quality.hip against the fp64 oracle of
test_quality.py on the images the kernel sees, determinism, SRRunManager.validate_quality against validate_batched,
search.quality_fitness, the command lines end to end, and which ops a scoring pass runs."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, amd
from test_quality import image_pair, oracle_luma, oracle_quality, oracle_quant

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])
SIZES = [(11, 11), (12, 37), (64, 96), (255, 131), (150, 210)]       # the last: 5 x 7 tiles of 32 x 32 positions


def _tail(t, pad):
    """a copy of t that is the tail slice of a larger allocation starting `pad` elements earlier: a read past its end
    leaves the allocation"""
    buf = torch.empty(pad + t.numel(), dtype=t.dtype, device=DEV)
    out = buf[pad:].view(t.shape)
    out.copy_(t)
    return out


def _y_of(x):
    """the uint8 Y images [N, H, W] of an operand as the kernel sees it (host tensor: NCHW float or HWC uint8)"""
    if x.dtype == torch.uint8:
        return oracle_luma(x.numpy())[None]
    return oracle_luma(oracle_quant(x.float().numpy()))


def _check(out, tgt, shave):
    """out / tgt: host tensors; runs the kernel on plain and on tail-slice copies, compares with the oracle"""
    ops = amd("ops")
    ya, yb = _y_of(out), _y_of(tgt)
    results = []
    for pad in (0, 3):
        sse, ssim, count = ops.quality_y(_tail(out.to(DEV), pad), _tail(tgt.to(DEV), pad), shave)
        torch.cuda.synchronize()
        results.append((sse.cpu(), ssim.cpu()))
        assert sse.dtype == torch.int64 and ssim.dtype == torch.float64
        assert count == (ya.shape[1] - 2 * shave) * (ya.shape[2] - 2 * shave)
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    sse, ssim = results[0]
    for i in range(ya.shape[0]):
        e, s = oracle_quality(ya[i], yb[i], shave)
        print("image %d: sse %d oracle %d   ssim %.17g oracle %.17g  diff %.3g" % (i, int(sse[i]), e, float(ssim[i]), s,
                                                                                float(ssim[i]) - s))
        assert int(sse[i]) == e
        assert abs(float(ssim[i]) - s) <= 1e-9
        assert 0.02 < s < 0.999
    return sse, ssim


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("shave", [0, 4])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("h,w", SIZES)
def test_quality_float_output_vs_oracle(h, w, dtype, n, shave):
    out, tgt = image_pair(n, h + 2 * shave, w + 2 * shave, h * 1000 + w + n)
    assert out.min() < 0 and out.max() > 1
    _check(torch.from_numpy(out).to(dtype), torch.from_numpy(tgt), shave)


@pytest.mark.parametrize("shave", [0, 4])
@pytest.mark.parametrize("h,w", SIZES)
def test_quality_uint8_operands_vs_oracle(h, w, shave):
    out, tgt = image_pair(1, h + 2 * shave, w + 2 * shave, h * 1000 + w + 7)
    qa, qb = torch.from_numpy(oracle_quant(out)[0].copy()), torch.from_numpy(oracle_quant(tgt)[0].copy())
    a = _check(qa, qb, shave)                                     # uint8 HWC against uint8 HWC
    b = _check(qa, torch.from_numpy(tgt), shave)                  # uint8 HWC against fp32
    c = _check(torch.from_numpy(out), torch.from_numpy(tgt), shave)
    for r in (b, c):                                              # the same images in another format: the same bits
        assert torch.equal(a[0], r[0]) and torch.equal(a[1], r[1])


def test_quality_identical_and_tie_colours():
    ops, utils = amd("ops"), amd("utils")
    out, _ = image_pair(2, 40, 50, 1)
    t = torch.from_numpy(out).to(DEV)
    sse, ssim, _ = ops.quality_y(t, t.clone())
    assert sse.tolist() == [0, 0] and ssim.tolist() == [1.0, 1.0]
    # every tie colour in one image: the kernel's luma is the exact one
    v = np.arange(256, dtype=np.int64)
    r, g, b = np.meshgrid(v, v, v, indexing="ij")
    tie = (65481 * r + 128553 * g + 24966 * b) % 255000 == 127500
    cols = np.stack([r[tie], g[tie], b[tie]], axis=1).astype(np.uint8)
    assert len(cols) == 194
    img = np.zeros((14, 14, 3), dtype=np.uint8)
    img.reshape(-1, 3)[:194] = cols
    ref = np.full((14, 14, 3), 128, dtype=np.uint8)
    sse, _, _ = ops.quality_y(torch.from_numpy(img).to(DEV), torch.from_numpy(ref).to(DEV))
    assert int(sse[0]) == utils.sse_y(img, ref)[0][0] == oracle_quality(oracle_luma(img), oracle_luma(ref))[0]


def test_quality_is_deterministic():
    ops = amd("ops")
    out, tgt = image_pair(3, 255, 131, 3)
    a, b = torch.from_numpy(out).to(DEV), torch.from_numpy(tgt).to(DEV)
    r1 = ops.quality_y(a, b)
    m1 = ops.quality_mse(a, b)
    r2 = ops.quality_y(a, b)
    m2 = ops.quality_mse(a, b)
    torch.cuda.synchronize()
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1].view(torch.int64), r2[1].view(torch.int64))
    assert torch.equal(m1.view(torch.int64), m2.view(torch.int64))


def test_quality_refuses_bad_operands():
    ops, C = amd("ops"), amd("_C")
    a = torch.zeros(1, 3, 16, 16, device=DEV)
    with pytest.raises(C.OfasrError, match="window"):
        ops.quality_y(a, a, shave=3)
    with pytest.raises(C.OfasrError, match="negative shave"):
        ops.quality_y(a, a, shave=-1)
    with pytest.raises(C.OfasrError):
        ops.quality_y(a, torch.zeros(1, 3, 16, 17, device=DEV))
    with pytest.raises(C.OfasrError):
        ops.quality_y(a.double(), a)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
def test_quality_mse_vs_fp64(dtype):
    """the per-image loss: fp32 difference, fp32 square, fp64 sum.  Against the same steps on the host in numpy the only
    difference is the order of an fp64 sum of n non-negative terms: relative error <= n * 2^-53 (1e-10 leaves margin)."""
    ops = amd("ops")
    out, tgt = image_pair(3, 77, 93, 11)
    a, b = torch.from_numpy(out).to(dtype), torch.from_numpy(tgt)
    got = ops.quality_mse(_tail(a.to(DEV), 3), _tail(b.to(DEV), 1)).cpu().numpy()
    d = a.float().numpy() - b.numpy()
    ref = (d * d).astype(np.float64).reshape(3, -1).mean(axis=1)
    print(got, ref)
    assert np.all(np.abs(got - ref) <= 1e-10 * ref)


# ---------------------------------------------------------------------------------------------- the run manager
class _Recorder(torch.nn.Module):
    """the network, keeping what it returned"""

    def __init__(self, net):
        super().__init__()
        self.net, self.outputs = net, []

    def forward(self, x):
        y = self.net(x)
        self.outputs.append(y.detach().float().cpu())
        return y


def _manager(tmp_path, sizes):
    rm = amd("imagenet_codebase.run_manager")
    nets = amd("elastic_nn.networks")
    amd("elastic_nn.modules.dynamic_op").DynamicSeparableConv2d.KERNEL_TRANSFORM_MODE = 1
    torch.manual_seed(9)
    net = nets.OFAMobileNetS4(**KW)
    cfg = rm.SyntheticSRRunConfig(n_epochs=1, init_lr=1e-3, train_batch_size=1, test_batch_size=1, image_size=64,
                                  n_train_batches=1, test_sizes=sizes)
    mgr = rm.SRRunManager(str(tmp_path), net, cfg, init=True, num_gpus=1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.7, 1.3)
    net.set_active_subnet(ks=5, e=4, d=2, pixel_d=2)
    return mgr, net, cfg


def _tie_mask(u8):
    c = u8.astype(np.int64)
    return (65481 * c[..., 0] + 128553 * c[..., 1] + 24966 * c[..., 2]) % 255000 == 127500


def test_validate_quality_matches_validate_batched(tmp_path):
    utils = amd("utils")
    sizes = [(96, 128), (64, 80), (96, 128), (72, 72)]
    mgr, net, cfg = _manager(tmp_path, sizes)
    key = "4x_down_image"
    loss_b, psnr_b, calls_b = mgr.validate_batched(is_test=True, input_key=key, graphs=False)
    rec = _Recorder(net)
    q = mgr.validate_quality(net=rec, is_test=True, input_key=key, graphs=False)
    assert q["calls"] == calls_b == 3
    # loss: validate_batched reduces in fp32 on the GPU (error <= about log2(n) * 2^-24 relative), validate_quality in fp64
    print("loss", q["loss"], loss_b, "psnr", q["psnr"], psnr_b, "ssim", q["ssim"])
    assert abs(q["loss"] - loss_b) <= 1e-5 * abs(loss_b)
    # the images in the order validate_quality scored them (size buckets, first-seen order)
    items = [b["image"] for b in cfg.test_loader]
    groups = utils.bucket_by_size(items)
    hr = [t for g in groups for t in g]
    outs = [o[i:i + 1] for o in rec.outputs for i in range(o.shape[0])]
    assert len(hr) == len(outs) == len(sizes)
    lo, hi, n_ties = [], [], 0
    for i, (o, t) in enumerate(zip(outs, hr)):
        qa, qb = oracle_quant(o.numpy())[0], oracle_quant(t.numpy())[0]
        ya, yb = oracle_luma(qa).astype(np.int64), oracle_luma(qb).astype(np.int64)
        sse = int(((ya - yb) ** 2).sum())
        assert abs(q["psnr_per_image"][i] - utils.psnr_from_sse(sse, ya.size)) == 0.0
        assert abs(q["ssim_per_image"][i] - utils.ssim_y(o, t)[0]) <= 1e-9
        # the host metric may round the luma of a tie-coloured pixel the other way: |d| changes by at most 1 there
        tie = _tie_mask(qa) | _tie_mask(qb)
        n_ties += int(tie.sum())
        slack = int((2 * np.abs(ya - yb)[tie] + 1).sum())
        lo.append(utils.psnr_from_sse(sse + slack, ya.size))
        hi.append(utils.psnr_from_sse(max(sse - slack, 0), ya.size))
    print("tie-coloured pixels:", n_ties)
    if n_ties == 0:
        assert abs(q["psnr"] - psnr_b) <= 1e-12 * psnr_b
    assert sum(lo) / len(lo) - 1e-12 * psnr_b <= psnr_b <= sum(hi) / len(hi) + 1e-12 * psnr_b
    # max_batch and shave thread through
    q2 = mgr.validate_quality(is_test=True, input_key=key, graphs=False, max_batch=1, shave=4)
    assert q2["calls"] == 4 and q2["ssim"] != q["ssim"]


def test_quality_fitness_returns_validate_quality_ssim(tmp_path):
    search = amd("elastic_nn.search")
    mgr, net, cfg = _manager(tmp_path, [(64, 64), (48, 80)])
    space = search.ArchSpace(net, 4)
    arch = space.random_sample(random.Random(3))
    g = torch.Generator().manual_seed(0)
    calib = [{"image": torch.rand(2, 3, 64, 64, generator=g).to(DEV), "4x_down_image": torch.rand(2, 3, 16, 16, generator=g).to(DEV),
              "2x_down_image": torch.rand(2, 3, 32, 32, generator=g).to(DEV)} for _ in range(2)]
    before = search.bn_buffers(net)
    fit = search.quality_fitness(net, calib, cfg.test_loader, mgr, space, metric="ssim")
    got = fit(arch)
    after = search.bn_buffers(net)
    assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)
    # the same steps by hand
    snap = search.bn_buffers(net)
    space.apply(net, arch)
    amd("elastic_nn.utils").recalibrate_bn(net, calib, input_key=search.lr_key(net))
    ref = mgr.validate_quality(net=net, data_loader=cfg.test_loader, input_key=search.lr_key(net), graphs=False)
    search.restore_bn_buffers(net, snap)
    assert got == ref["ssim"] and 0.0 < got < 1.0
    assert search.quality_fitness(net, calib, cfg.test_loader, mgr, space, metric="psnr")(arch) == ref["psnr"]
    with pytest.raises(ValueError):
        search.quality_fitness(net, calib, cfg.test_loader, mgr, space, metric="lpips")


def _gpu_events(prof):
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return sorted(ev, key=lambda e: e.time_range.start)


def test_validate_quality_runs_no_aten_scoring(tmp_path):
    """from the first kernel of the first forward to the end of the pass, validate_quality runs the kernels of the
    forwards, the metric kernels and ONE small device-to-host copy: no ATen element-wise or reduction kernel and no copy of
    an image.  Checked by counting every GPU kernel of that window against a profile of the bare forwards."""
    import collections
    from torch.profiler import ProfilerActivity, profile
    utils, C = amd("utils"), amd("_C")
    mgr, net, cfg = _manager(tmp_path, [(96, 128), (64, 80), (96, 128)])
    key = "4x_down_image"
    kw = dict(is_test=True, input_key=key, graphs=False)
    items = [{k: v.to(DEV) for k, v in b.items() if torch.is_tensor(v)} for b in cfg.test_loader]
    lrs = [torch.cat([it[key] for it in g]) for g in utils.bucket_by_size(items, key=lambda it: it[key])]
    net.eval()

    def forwards():
        with torch.no_grad():
            for x in lrs:
                net(x)

    forwards()                            # warm-ups outside the profiles
    mgr.validate_quality(**kw)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof_f:
        forwards()
        torch.cuda.synchronize()
    C.reset_launch_counts()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof_q:
        q = mgr.validate_quality(**kw)
        torch.cuda.synchronize()
    assert C.launch_count("quality_y_tile_kernel") == 2 and C.launch_count("quality_mse_part_kernel") == 2

    def is_copy(n):
        return n.lower().startswith("memcpy") or n.lower().startswith("memset")

    fwd = collections.Counter(e.name for e in _gpu_events(prof_f) if not is_copy(e.name))
    assert fwd, "the profiler saw no forward kernel"
    ev = _gpu_events(prof_q)
    first = next(i for i, e in enumerate(ev) if e.name in fwd)
    window = ev[first:]
    seen = collections.Counter(e.name for e in window if not is_copy(e.name))
    metric = {n: c for n, c in seen.items() if "quality_" in n}
    assert sum(c for n, c in metric.items() if "quality_y_tile_kernel" in n) == 2
    assert sum(c for n, c in metric.items() if "quality_y_finish_kernel" in n) == 2
    assert sum(c for n, c in metric.items() if "quality_mse_part_kernel" in n) == 2
    assert sum(c for n, c in metric.items() if "quality_mse_finish_kernel" in n) == 2
    rest = collections.Counter({n: c for n, c in seen.items() if n not in metric})
    assert rest == fwd, {"only in validate_quality": rest - fwd, "only in the forwards": fwd - rest}
    copies = [e for e in window if is_copy(e.name)]
    print([e.name for e in copies])
    assert len(copies) == 1 and "dtoh" in copies[0].name.lower().replace(" ", "").replace("->", "to"), [e.name for e in copies]
    assert 0 < q["ssim"] < 1


# ---------------------------------------------------------------------------------------------- command lines
def _export_tiny(tmp_path):
    from test_hip_upscale import _randomize, _static
    net = _randomize(_static("s4", dict(ks=3, e=3, d=2, pixel_d=2)), 4)
    d = tmp_path / "net"
    d.mkdir()
    (d / "net_config.json").write_text(json.dumps(net.config))
    torch.save({"state_dict": {k: v.cpu() for k, v in net.state_dict().items()}}, str(d / "static_state_dict.pth"))
    return net, d


def test_upscale_cli_reference(tmp_path):
    from PIL import Image
    up, utils = amd("upscale"), amd("utils")
    net, d = _export_tiny(tmp_path)
    rng = np.random.RandomState(0)
    (tmp_path / "in").mkdir()
    (tmp_path / "hr").mkdir()
    tu = up.TiledUpscaler(net, core=32)
    expect = {}
    for name, (h, w) in (("a", (40, 30)), ("b", (11, 13))):
        lr = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        Image.fromarray(lr, "RGB").save(str(tmp_path / "in" / (name + ".png")))
        sr = tu.upscale(torch.from_numpy(lr))
        hr = np.clip(sr.cpu().numpy().astype(np.int64) + rng.randint(-20, 21, tuple(sr.shape)), 0, 255).astype(np.uint8)
        Image.fromarray(hr, "RGB").save(str(tmp_path / "hr" / (name + ".png")))
        q = utils.quality_y_device(sr, torch.from_numpy(hr).to(DEV), 4)
        expect[name] = (q.psnr()[0], q.ssim_list()[0], q.sse_list()[0])
        assert q.sse_list()[0] == utils.sse_y(sr.cpu().numpy(), hr, 4)[0][0]
        assert abs(q.ssim_list()[0] - utils.ssim_y(sr.cpu().numpy(), hr, 4)[0]) <= 1e-9
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "upscale_ofa_net_sr.py"), "--static", str(d), "--out", str(out), "--core", "32",
           "--reference", str(tmp_path / "hr"), "--shave", "4", str(tmp_path / "in")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Y-SSIM" in r.stdout and "mean of 2 images" in r.stdout
    rec = json.load(open(str(out / "quality.json")))
    assert rec["shave"] == 4 and len(rec["images"]) == 2
    for x in rec["images"]:
        name = os.path.splitext(os.path.basename(x["input"]))[0]
        assert (x["psnr"], x["ssim"], x["sse"]) == expect[name]
    assert rec["mean"]["ssim"] == sum(x["ssim"] for x in rec["images"]) / 2
    # a reference of another size is a clear error
    Image.fromarray(np.zeros((50, 50, 3), dtype=np.uint8), "RGB").save(str(tmp_path / "hr" / "b.png"))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "must have the output's size" in (r.stdout + r.stderr)


def test_eval_cli_ssim(tmp_path):
    net, d = _export_tiny(tmp_path)
    cmd = [sys.executable, os.path.join(ROOT, "eval_ofa_net_sr.py"), "--static", str(d), "--synthetic", "--ssim", "--shave", "4",
           "--test-sizes", "64x64,48x80,64x64", "--path", str(tmp_path / "run")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("Y-SSIM")]
    assert len(line) == 1 and "Y-PSNR" in r.stdout.replace(line[0], "")
    rm = amd("imagenet_codebase.run_manager")
    import eval_ofa_net_sr as ev
    cfg = rm.Div2K_SetXXRunConfig(n_epochs=1, init_lr=1e-3, opt_type="adam", no_decay_keys="bn#bias", label_smoothing=0.0,
                                  train_batch_size=1, test_batch_size=1, image_size=256,
                                  test_sizes=[(64, 64), (48, 80), (64, 64)], n_train_batches=1, allow_synthetic=True)
    mgr = rm.SRRunManager(str(tmp_path / "again"), ev.load_static(str(d)), cfg, init=False, mix_prec="f32", num_gpus=1)
    q = mgr.validate_quality(is_test=True, input_key="4x_down_image", shave=4)
    assert line[0].startswith("Y-SSIM %.4f  Y-PSNR %.3f dB" % (q["ssim"], q["psnr"]))
