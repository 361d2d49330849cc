"""Tiled upscaling on the MI355X (`-m gpu`): the tile kernels (csrc/tile_io.hip: ofasr_tile_gather_u8 /
ofasr_tile_scatter_u8) against torch restatements, 64-bit addressing of the scatter, tiled = whole-image parity of
upscale.TiledUpscaler on random static networks, that the halo is needed, the receptive radius seen by a real forward,
the command line end to end, and which ops a tiled upscale runs."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, amd
from placed import check, place
from test_hip_video_reuse import WILD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(ks_list=[3, 5, 7], expand_ratio_list=[3, 4, 6], depth_list=[2, 3, 4], pixelshuffle_depth_list=[1, 2])
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _tail(t, pad):
    """a copy of t that is the tail slice of a larger allocation starting `pad` elements earlier: a read past its end
    leaves the allocation"""
    buf = torch.empty(pad + t.numel(), dtype=t.dtype, device=DEV)
    out = buf[pad:].view(t.shape)
    out.copy_(t)
    return out


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("h,w", [(13, 22), (16, 24), (37, 53)])
def test_gather_matches_to_tensor(dtype, pad, h, w):
    up = amd("upscale")
    g = torch.Generator().manual_seed(h * 100 + w + pad)
    H, W = 37, 53
    img = _tail(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8), pad)
    origins = [(0, 0), (H - h, W - w), (H - h, 0), (0, W - w)]
    for _ in range(6):
        origins.append((int(torch.randint(0, H - h + 1, (1,), generator=g)), int(torch.randint(0, W - w + 1, (1,), generator=g))))
    origins += WILD                        # the kernel clamps an origin into [0, H - h] x [0, W - w]
    table = torch.tensor(origins, dtype=torch.int64, device=DEV)
    out = up.tile_gather(img, table, h, w, dtype)
    torch.cuda.synchronize()
    assert out.shape == (len(origins), 3, h, w) and out.dtype == dtype
    # the reference divides on the CPU, as the data provider's to_tensor does: a correctly rounded fp32 division (ATen's
    # GPU kernel multiplies by the rounded reciprocal instead, which differs in the last bit for about half the values)
    host, out = img.cpu(), out.cpu()
    for i, (y, x) in enumerate(origins):
        y, x = min(max(y, 0), H - h), min(max(x, 0), W - w)
        ref = (host[y:y + h, x:x + w].permute(2, 0, 1).float() / 255).to(dtype)
        assert torch.equal(out[i], ref), (i, y, x)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("OH,OW", [(64, 96), (61, 89)])
def test_scatter_matches_quantisation(dtype, pad, OH, OW):
    up = amd("upscale")
    g = torch.Generator().manual_seed(OH + OW + pad)
    plan = up.plan_windows(OH, OW, 16, 4, 1, 1, 64)
    n = len(plan)
    sh, sw = plan.win_h, plan.win_w
    vals = torch.rand(n, 3, sh, sw, generator=g) * 1.4 - 0.2
    vals[0, 0, 0, :8] = torch.tensor([0.5, 1.5, 2.5, 3.5, 254.5, 127.5, 0.0, 1.0]) / 255   # ties
    src = _tail(vals.to(dtype).to(DEV), pad)
    base = torch.randint(0, 256, (OH, OW, 3), generator=g, dtype=torch.uint8).to(DEV)
    img = _tail(base, pad)
    rows = [(cy - wy, cx - wx, cy, cx, ch, cw) for (wy, wx, cy, cx, ch, cw) in plan.windows]
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    up.tile_scatter(src, table, img, max(r[4] for r in rows), max(r[5] for r in rows))
    torch.cuda.synchronize()
    ref = base.clone()
    for i, (sy, sx, dy, dx, eh, ew) in enumerate(rows):
        v = src[i, :, sy:sy + eh, sx:sx + ew].float().clamp(0, 1) * 255.0
        ref[dy:dy + eh, dx:dx + ew] = v.round().to(torch.uint8).permute(1, 2, 0)
    assert torch.equal(img, ref)


def test_scatter_64bit_addressing():
    up = amd("upscale")
    OH, OW = 32000, 24000                  # 2.3e9 bytes
    assert OH * OW * 3 > 2 ** 31 + 2 ** 26
    img = torch.empty(OH, OW, 3, dtype=torch.uint8, device=DEV)
    try:
        img[-40:].fill_(7)
        src = torch.rand(1, 3, 20, 28, device=DEV)
        table = torch.tensor([[2, 3, OH - 17, OW - 25, 17, 25]], dtype=torch.int64, device=DEV)
        up.tile_scatter(src, table, img, 17, 25)
        got = img[OH - 40:].cpu()
        torch.cuda.synchronize()
    finally:
        del img
        torch.cuda.empty_cache()
    ref = torch.full((40, OW, 3), 7, dtype=torch.uint8)
    ref[23:, OW - 25:] = (src[0, :, 2:19, 3:28].clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0).cpu()
    assert torch.equal(got, ref)


# table rows no planner makes: every column far outside its range, up to the ends of int64
WILD_ROWS = [[-2 ** 40, 2 ** 40, -5, -5, 10 ** 12, 10 ** 12],
             [2 ** 62, -2 ** 62, 30, 40, 30, 40],
             [3, 5, 39, 55, 7, 9],
             [-2 ** 63, 2 ** 63 - 1, 2 ** 63 - 1, -2 ** 63, 2 ** 63 - 1, 2 ** 63 - 1]]
# one row whose clamped extent is non-empty and odd in every destination column: 7 x 9 at (31, 41), which a 4:2:0
# destination turns into 6 x 8 at (30, 40)
ODD_ROWS = [[3, 5, 31, 41, 7, 9]]


def _clamped_row(row, sh, sw, OH, OW, max_eh, max_ew, even):
    """the rule of the scatter kernels (csrc/tile_table.h, scatter_row), restated: offsets into [0, side], the extent
    non-negative, at most the launch's bound and at most what is left of the source window and of the destination behind
    the offsets; for a 4:2:0 destination dy, dx, eh, ew then lose their low bit"""
    sy, sx, dy, dx, eh, ew = row
    sy, sx = min(max(sy, 0), sh), min(max(sx, 0), sw)
    dy, dx = min(max(dy, 0), OH), min(max(dx, 0), OW)
    eh = min(max(eh, 0), max_eh, sh - sy, OH - dy)
    ew = min(max(ew, 0), max_ew, sw - sx, OW - dx)
    if even:
        dy, dx, eh, ew = (t - t % 2 for t in (dy, dx, eh, ew))
    return [sy, sx, dy, dx, eh, ew]


@pytest.mark.parametrize("lead", [0, 4])
@pytest.mark.parametrize("rows", [WILD_ROWS, ODD_ROWS], ids=["wild", "odd"])
@pytest.mark.parametrize("kind", ["rgb8", "yuv8", "yuv16"])
def test_scatter_clamps_wild_rows(kind, rows, lead):
    """ofasr_tile_scatter_u8 / ofasr_tile_scatter_yuv420 (uint8 and uint16 planes) on WILD_ROWS and on ODD_ROWS, source and
    destination between guard bands: the destination is what the same scatter gives on the clamped rows, and no guard
    byte changes"""
    up = amd("upscale")
    g = torch.Generator().manual_seed(11)
    rng = np.random.RandomState(11)
    n, sh, sw, OH, OW, max_eh, max_ew = 4, 20, 28, 40, 56, 16, 24
    vals = (torch.rand(n, 3, sh, sw, generator=g) * 1.4 - 0.2).to(DEV)
    src = place(vals, lead, "in", "src")                 # lead 4: no 16-byte source load is legal
    dt, top = (np.uint16, 1024) if kind == "yuv16" else (np.uint8, 256)
    shapes = [(OH, OW, 3)] if kind == "rgb8" else [(OH, OW), (OH // 2, OW // 2), (OH // 2, OW // 2)]
    base = [torch.from_numpy(rng.randint(0, top, s).astype(dt)).to(DEV) for s in shapes]   # uint16: made and copied only
    dst = [place(b, lead // 2, "out", "dst%d" % i) for i, b in enumerate(base)]   # lead 2: no dword store is legal
    for d, b in zip(dst, base):
        d.copy_(b)
    tame = [_clamped_row(r, sh, sw, OH, OW, max_eh, max_ew, kind != "rgb8") for r in rows]
    if rows is WILD_ROWS:
        assert tame[2] == ([3, 5, 39, 55, 1, 1] if kind == "rgb8" else [3, 5, 38, 54, 0, 0])
    else:
        assert tame == ([[3, 5, 31, 41, 7, 9]] if kind == "rgb8" else [[3, 5, 30, 40, 6, 8]])
    wild = torch.tensor(rows, dtype=torch.int64, device=DEV)
    if kind == "rgb8":
        up.tile_scatter(src, wild, dst[0], max_eh, max_ew)
        exp = [base[0].clone()]
        for i, (sy, sx, dy, dx, eh, ew) in enumerate(tame):
            v = vals[i, :, sy:sy + eh, sx:sx + ew].clamp(0, 1) * 255.0
            exp[0][dy:dy + eh, dx:dx + ew] = v.round().to(torch.uint8).permute(1, 2, 0)
    else:
        up.tile_scatter_yuv420(src, wild, dst[0], dst[1], dst[2], max_eh, max_ew)
        exp = [b.clone() for b in base]
        up.tile_scatter_yuv420(vals, torch.tensor(tame, dtype=torch.int64, device=DEV), exp[0], exp[1], exp[2], max_eh, max_ew)
    torch.cuda.synchronize()
    for d, e in zip(dst, exp):
        assert np.array_equal(d.cpu().numpy(), e.cpu().numpy())
        check(d)
    check(src)


# ---------------------------------------------------------------------------------------------- networks
def _static(kind, setting):
    nets = amd("elastic_nn.networks")
    st = amd("imagenet_codebase.networks.sr_static")
    net = nets.OFAMobileNetS4(**KW) if kind == "s4" else nets.OFAMobileNetX4(**KW)
    if isinstance(setting, dict):
        net.set_active_subnet(**setting)
    else:
        random.seed(setting)
        net.sample_active_subnet()
    return st.build_static_net(net.get_active_net_config())


def _randomize(net, seed, branch_gain=1.0, lean=0.02):
    """he_fout weights whose spatial taps lean to the top-left (so what lies near the edge of the receptive field
    carries weight: a halo that is too small shows), non-trivial BN parameters and statistics; the output is then scaled
    to about unit spread around 0.5 so that the uint8 image is not all clamped.  `lean` is the weight of the other rows /
    columns of taps against the top / left one (0: every conv is a pure shift plus channel mixing); branch_gain scales
    each MB block's last BN (above 1 the residual branches, not the identity shortcuts, carry the signal).  With both,
    most of an output pixel comes from inputs near the edge of its receptive field."""
    g = torch.Generator().manual_seed(seed)
    net.init_model("he_fout")
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d) and m.kernel_size[1] > 1:
                k = m.kernel_size[1]
                prof = torch.full((k,), float(lean))
                prof[0] = 1.0      # the top row and left column of taps: output pixels lean on inputs above / left
                n0 = m.weight.flatten(1).norm(dim=1)
                m.weight.mul_((prof.view(k, 1) * prof.view(1, k)) * (1.0 + 0.3 * torch.rand(m.weight.shape, generator=g)))
                m.weight.mul_((n0 / m.weight.flatten(1).norm(dim=1)).view(-1, 1, 1, 1))   # he_fout's gain kept
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
    # smooth content plus noise, like a photo more than like white noise
    base = torch.rand(3, H // 8 + 2, W // 8 + 2, generator=g)
    smooth = torch.nn.functional.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0]
    img = (smooth * 200 + torch.rand(3, H, W, generator=g) * 55).clamp(0, 255).to(torch.uint8)
    return img.permute(1, 2, 0).contiguous()


S4_NETS = [("s4", dict(ks=7, e=6, d=4, pixel_d=2)), ("s4", dict(ks=3, e=3, d=2, pixel_d=1)), ("s4", 5), ("s4", 12)]


@pytest.mark.parametrize("kind,setting", S4_NETS + [("x4", dict(ks=3, e=3, d=2, pixel_d=1))], ids=lambda v: str(v))
def test_tiled_equals_whole_fp32(kind, setting):
    up = amd("upscale")
    net = _randomize(_static(kind, setting), 1)
    tu = up.TiledUpscaler(net, core=48 if kind == "s4" else 32, mix_prec="f32")
    H, W = (187, 301) if kind == "s4" else (184, 300)
    if kind == "x4":
        H, W = tu.halo * 2 + 3 * 32, tu.halo * 2 + 5 * 32     # several windows along both axes despite the large halo
    img = _image(H, W, 3)
    plan = tu.plan(H, W)
    assert len(plan) >= 6                     # many windows, some shifted into the image at its far edges
    assert any(wy + plan.win_h == H and cy > wy + tu.halo for (wy, _, cy, _, _, _) in plan.windows)
    whole = tu.upscale_float(img, whole=True)
    tiled = tu.upscale_float(img)
    assert whole.shape == (3, H * tu.scale, W * tu.scale)
    err = (tiled - whole).abs().max().item()
    assert err <= 2e-5, err
    assert float(whole.std()) > 0.05
    u_whole = tu.upscale(img, whole=True)
    u_tiled = tu.upscale(img)
    d = (u_tiled.int() - u_whole.int()).abs()
    assert int(d.max()) <= 1
    assert int((d > 0).sum()) <= 1e-4 * d.numel()


def test_halo_matters():
    up = amd("upscale")
    net = _randomize(_static("s4", dict(ks=3, e=3, d=2, pixel_d=1)), 1, branch_gain=4.0, lean=0.0)
    tu = up.TiledUpscaler(net, core=48, mix_prec="f32")
    img = _image(187, 301, 3)
    whole = tu.upscale_float(img, whole=True)
    ok = (tu.upscale_float(img) - whole).abs().max().item()
    tu.halo = tu.radius - 2
    bad = (tu.upscale_float(img) - whole).abs().max().item()
    assert ok <= 2e-5 and bad > 25 * 2e-5, (ok, bad)


def test_tiled_bf16_error_no_worse_than_whole_bf16():
    up = amd("upscale")
    net = _randomize(_static("s4", 5), 2)
    img = _image(187, 301, 4)
    ref = up.TiledUpscaler(net, core=48, mix_prec="f32").upscale_float(img, whole=True)
    tb = up.TiledUpscaler(net, core=48, mix_prec="bf16")
    whole = tb.upscale_float(img, whole=True)
    tiled = tb.upscale_float(img)

    def rel(a):
        return float((a - ref).norm() / ref.norm())

    assert rel(whole) > 0
    assert rel(tiled) <= 1.05 * rel(whole) + 1e-4, (rel(tiled), rel(whole))


def test_receptive_radius_on_a_real_forward():
    """zero input, identity BN and positive weights: every activation is exactly 0 except where the perturbed pixel
    reaches, so even the faintest influence is seen (no absorption into O(1) values, no cancellation)"""
    up = amd("upscale")
    net = _static("s4", dict(ks=3, e=3, d=2, pixel_d=1))
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d):
                fan_in = m.weight[0].numel()
                m.weight.copy_((torch.rand(m.weight.shape, generator=g) * 0.5 + 0.5) / fan_in)
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.fill_(1.0), m.bias.zero_(), m.running_mean.zero_(), m.running_var.fill_(1.0)
    net = net.to(DEV).eval()
    amd("ops").clear_infer_cache()
    r = up.receptive_radius(net.config)
    s = net.upscale
    H = W = 2 * r + 40
    py, px = H // 2, W // 2 + 1
    x0 = torch.zeros(1, 3, H, W, device=DEV)
    x1 = x0.clone()
    x1[0, :, py, px] = 1.0
    with torch.no_grad():
        y0, y1 = net(x0), net(x1)
    assert float(y0.abs().max()) == 0.0
    ys, xs = torch.nonzero((y1 - y0).abs()[0].amax(0) > 0, as_tuple=True)
    # distances of the changed outputs from the pixel's output block [p*s, (p+1)*s)
    dy = torch.maximum(py * s - ys, ys - ((py + 1) * s - 1)).clamp(min=0)
    dx = torch.maximum(px * s - xs, xs - ((px + 1) * s - 1)).clamp(min=0)
    reach = max(int(dy.max()), int(dx.max()))
    assert reach <= s * (r + 1), (reach, s, r)
    assert reach >= s * (r - 2), (reach, s, r)


# ---------------------------------------------------------------------------------------------- command line
def test_cli_end_to_end(tmp_path):
    from PIL import Image
    up = amd("upscale")
    net = _randomize(_static("s4", dict(ks=3, e=3, d=2, pixel_d=1)), 4)
    d = tmp_path / "net"
    d.mkdir()
    import json
    (d / "net_config.json").write_text(json.dumps(net.config))
    torch.save({"state_dict": {k: v.cpu() for k, v in net.state_dict().items()}}, str(d / "static_state_dict.pth"))
    rng = np.random.RandomState(0)
    a = rng.randint(0, 256, (90, 70, 4)).astype(np.uint8)
    b = rng.randint(0, 256, (11, 13, 3)).astype(np.uint8)
    Image.fromarray(a, "RGBA").save(str(tmp_path / "a.png"))
    Image.fromarray(b, "RGB").save(str(tmp_path / "b.png"))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "upscale_ofa_net_sr.py"), "--static", str(d), "--out", str(out),
           "--core", "32", str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "MP/s" in r.stdout
    tu = up.TiledUpscaler(net, core=32)
    for name, arr in (("a", a), ("b", b)):
        rgb = np.asarray(Image.fromarray(arr).convert("RGB"))
        got = np.asarray(Image.open(str(out / (name + ".png"))))
        assert got.shape == (rgb.shape[0] * 4, rgb.shape[1] * 4, 3)
        assert np.array_equal(got, tu.upscale(torch.from_numpy(rgb)).cpu().numpy())


# ---------------------------------------------------------------------------------------------- routing
@pytest.mark.parametrize("mix_prec", ["f32", "bf16"])
def test_tiled_upscale_runs_no_aten_conv_bn_or_upsample(mix_prec):
    from torch.profiler import ProfilerActivity, profile
    up = amd("upscale")
    net = _randomize(_static("s4", 12), 5)
    tu = up.TiledUpscaler(net, core=48, mix_prec=mix_prec, graphed=False)
    img = _image(120, 140, 6).to(DEV)
    tu.upscale(img)                     # warm-up outside the profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        tu.upscale(img)
        torch.cuda.synchronize()
    ops_seen = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU}
    bad = [n for n in ops_seen if n in ("aten::convolution", "aten::conv2d", "aten::_convolution", "aten::batch_norm",
                                        "aten::pixel_shuffle", "aten::pixel_unshuffle") or "upsample" in n]
    assert not bad, bad
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert any("tile_gather_u8_kernel" in n for n in names) and any("tile_scatter_u8_kernel" in n for n in names), \
        "the profiler saw no tile kernel"
