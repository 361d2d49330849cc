"""The YUV 4:2:0 video path on the MI355X (`-m gpu`): the whole-frame conversion kernels (csrc/yuv.hip) against the host
definition (video.py), the fused tile moves against the unfused composition of the whole-frame kernels and the RGB tile
kernels, 64-bit addressing of the fused scatter, TiledUpscaler.upscale_yuv420 against the RGB path on a random static
network, which kernels the fused path launches, and the command line end to end.  Everything is bit-exact."""
import itertools
import json
import os
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
COMBOS = list(itertools.product(["bt601", "bt709"], [False, True]))


def _tail(t, pad):
    """a copy of t on the GPU that is the tail slice of a larger allocation starting `pad` elements earlier: its base is
    unaligned for pad = 1, 3, and a read past its end leaves the allocation"""
    buf = torch.empty(pad + t.numel(), dtype=t.dtype, device=DEV)
    out = buf[pad:].view(t.shape)
    out.copy_(t)
    return out


def _random_planes(H, W, seed):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 256, (H, W)).astype(np.uint8), rng.randint(0, 256, (H // 2, W // 2)).astype(np.uint8),
            rng.randint(0, 256, (H // 2, W // 2)).astype(np.uint8))


def _in_gamut_planes(H, W, seed, matrix="bt601", full=False):
    """the encode of a random RGB image: planes whose decode mostly stays clear of the clamps"""
    rng = np.random.RandomState(seed)
    return amd("video").rgb_to_yuv420_host(rng.randint(40, 216, (H, W, 3)).astype(np.uint8), matrix, full)


def _gpu_planes(planes, pad=0):
    return tuple(_tail(torch.from_numpy(np.ascontiguousarray(p)), pad) for p in planes)


# ---------------------------------------------------------------------------------------------- whole frame
@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("H,W", [(2, 2), (4, 6), (38, 54)])
def test_decode_matches_host_definition(H, W, pad):
    ops, video = amd("ops"), amd("video")
    for matrix, full in COMBOS:
        inputs = [_random_planes(H, W, H + pad), _in_gamut_planes(H, W, W + pad, matrix, full)]
        for c in (0, 255):
            inputs.append((np.full((H, W), c, np.uint8),) + (np.full((H // 2, W // 2), c, np.uint8),) * 2)
        for planes in inputs:
            y, u, v = _gpu_planes(planes, pad)
            got = ops.yuv420_to_rgb_u8(y, u, v, matrix, full)
            assert got.shape == (H, W, 3) and got.dtype == torch.uint8
            assert np.array_equal(got.cpu().numpy(), video.yuv420_to_rgb_host(*planes, matrix, full)), (matrix, full)


@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("H,W", [(2, 2), (4, 6), (38, 54)])
def test_encode_matches_host_definition(H, W, pad):
    ops, video = amd("ops"), amd("video")
    rng = np.random.RandomState(H * 7 + pad)
    for matrix, full in COMBOS:
        smooth = video.yuv420_to_rgb_host(*_in_gamut_planes(H, W, 5, matrix, full), matrix, full)
        inputs = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8), smooth, np.zeros((H, W, 3), np.uint8),
                  np.full((H, W, 3), 255, np.uint8)]
        for rgb in inputs:
            out = tuple(_tail(torch.zeros(s, dtype=torch.uint8), pad) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2)))
            got = ops.rgb_to_yuv420_u8(_tail(torch.from_numpy(rgb), pad), matrix, full, out=out)
            exp = video.rgb_to_yuv420_host(rgb, matrix, full)
            for g, e in zip(got, exp):
                assert np.array_equal(g.cpu().numpy(), e), (matrix, full)


def test_wrappers_refuse_bad_frames():
    ops, up, C = amd("ops"), amd("upscale"), amd("_C")
    y, u, v = (torch.zeros(s, dtype=torch.uint8, device=DEV) for s in ((6, 8), (3, 4), (3, 4)))
    origins = torch.zeros(1, 2, dtype=torch.int64, device=DEV)
    with pytest.raises(C.OfasrError):
        ops.yuv420_to_rgb_u8(y.cpu(), u.cpu(), v.cpu())
    with pytest.raises(ValueError):
        ops.yuv420_to_rgb_u8(y[:5], u, v)                       # odd height
    with pytest.raises(ValueError):
        ops.yuv420_to_rgb_u8(y, u[:, :3], v)                    # chroma shape (and not contiguous)
    with pytest.raises(ValueError):
        ops.yuv420_to_rgb_u8(y.float(), u, v)
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420_u8(torch.zeros(6, 7, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        up.tile_gather_yuv420(y, u, u[:2], origins, 4, 4, torch.float32)
    with pytest.raises(C.OfasrError):
        up.tile_gather_yuv420(y, u, v, origins, 7, 4, torch.float32)     # window taller than the frame
    with pytest.raises(ValueError):
        up.tile_scatter_yuv420(torch.zeros(1, 3, 4, 4, device=DEV), torch.zeros(1, 6, dtype=torch.int64, device=DEV),
                               y[:, :7].contiguous(), u, v, 4, 4)


# ---------------------------------------------------------------------------------------------- fused gather
def _origins(H, W, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    out = [(0, 0), (H - h, W - w), (H - h, 0), (0, W - w), (1, 1), (1, 2), (2, 1)]   # corners, odd/odd, odd/even, even/odd
    for _ in range(6):
        out.append((int(torch.randint(0, H - h + 1, (1,), generator=g)), int(torch.randint(0, W - w + 1, (1,), generator=g))))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("h,w", [(13, 22), (16, 24), (38, 54)])
def test_fused_gather_equals_unfused(dtype, h, w):
    ops, up = amd("ops"), amd("upscale")
    H, W = 38, 54
    table = torch.tensor(_origins(H, W, h, w, h * 100 + w), dtype=torch.int64, device=DEV)   # the kernels clamp alike
    for pad, (matrix, full), kind in zip([0, 1, 3, 0], COMBOS, [_random_planes, _in_gamut_planes] * 2):
        y, u, v = _gpu_planes(kind(H, W, pad + h), pad)
        fused = _tail(torch.zeros(table.size(0), 3, h, w, dtype=dtype), pad)
        up.tile_gather_yuv420(y, u, v, table, h, w, dtype, matrix, full, out=fused)
        rgb = ops.yuv420_to_rgb_u8(y, u, v, matrix, full)
        assert torch.equal(fused, up.tile_gather(rgb, table, h, w, dtype)), (pad, matrix, full)


def test_fused_gather_clamps_wild_origins():
    up, video = amd("upscale"), amd("video")
    H, W, h, w = 38, 54, 13, 22
    planes = _random_planes(H, W, 9)
    y, u, v = _gpu_planes(planes, 1)
    wild = [(-5, 1000), (10 ** 12, -3), (-2 ** 62, 2 ** 62), (7, W - w + 1)]
    got = up.tile_gather_yuv420(y, u, v, torch.tensor(wild, dtype=torch.int64, device=DEV), h, w, torch.float32).cpu()
    rgb = torch.from_numpy(video.yuv420_to_rgb_host(*planes))
    for i, (y0, x0) in enumerate(wild):
        y0, x0 = min(max(y0, 0), H - h), min(max(x0, 0), W - w)
        assert torch.equal(got[i], rgb[y0:y0 + h, x0:x0 + w].permute(2, 0, 1).float() / 255), i


# ---------------------------------------------------------------------------------------------- fused scatter
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("OH,OW", [(64, 96), (60, 88)])
def test_fused_scatter_equals_unfused(dtype, pad, OH, OW):
    ops, up = amd("ops"), amd("upscale")
    g = torch.Generator().manual_seed(OH + OW + pad)
    plan = up.plan_windows(OH, OW, 16, 4, 2, 1, 64)
    n = len(plan)
    sh, sw = plan.win_h, plan.win_w
    vals = torch.rand(n, 3, sh, sw, generator=g) * 1.4 - 0.2
    vals[0, 0, 0, :8] = torch.tensor([0.5, 1.5, 2.5, 3.5, 254.5, 127.5, 0.0, 1.0]) / 255   # ties
    src = _tail(vals.to(dtype), pad)
    rows = [(cy - wy, cx - wx, cy, cx, ch, cw) for (wy, wx, cy, cx, ch, cw) in plan.windows]
    assert all(t % 2 == 0 for r in rows for t in r[2:])
    skipped = {1, n - 1}                      # two cores stay unwritten: the planes there must keep their bytes
    keep = [i for i in range(n) if i not in skipped]
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    table[list(skipped), 4:] = 0              # an empty extent writes nothing
    matrix, full = COMBOS[pad % 4]
    base = _gpu_planes(_random_planes(OH, OW, pad), 0)
    y, u, v = (_tail(p.cpu(), pad) for p in base)
    up.tile_scatter_yuv420(src, table, y, u, v, max(r[4] for r in rows), max(r[5] for r in rows), matrix, full)
    img = ops.yuv420_to_rgb_u8(*base, matrix, full)
    up.tile_scatter(src, table, img, max(r[4] for r in rows), max(r[5] for r in rows))
    ref = ops.rgb_to_yuv420_u8(img, matrix, full)
    exp = [p.clone() for p in base]
    for i in keep:
        _, _, dy, dx, eh, ew = rows[i]
        exp[0][dy:dy + eh, dx:dx + ew] = ref[0][dy:dy + eh, dx:dx + ew]
        for k in (1, 2):
            exp[k][dy // 2:(dy + eh) // 2, dx // 2:(dx + ew) // 2] = ref[k][dy // 2:(dy + eh) // 2, dx // 2:(dx + ew) // 2]
    for got, e in zip((y, u, v), exp):
        assert torch.equal(got, e)
    _, _, dy, dx, eh, ew = rows[1]
    assert torch.equal(y[dy:dy + eh, dx:dx + ew], base[0][dy:dy + eh, dx:dx + ew])


def test_fused_scatter_makes_odd_table_entries_even():
    up, video = amd("upscale"), amd("video")
    base = _random_planes(12, 16, 2)
    y, u, v = _gpu_planes(base)
    src = torch.rand(1, 3, 10, 12, generator=torch.Generator().manual_seed(1)).to(DEV)
    # dy 3 -> 2, dx 5 -> 4, eh 7 -> 6, ew 9 -> 8; the source offsets stay as they are
    up.tile_scatter_yuv420(src, torch.tensor([[1, 2, 3, 5, 7, 9]], dtype=torch.int64, device=DEV), y, u, v, 7, 9)
    rgb = (src[0, :, 1:7, 2:10].clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    ey, eu, ev = video.rgb_to_yuv420_host(np.ascontiguousarray(rgb))
    exp = [p.copy() for p in base]
    exp[0][2:8, 4:12], exp[1][1:4, 2:6], exp[2][1:4, 2:6] = ey, eu, ev
    for got, e in zip((y, u, v), exp):
        assert np.array_equal(got.cpu().numpy(), e)


def test_fused_scatter_64bit_addressing():
    up, video = amd("upscale"), amd("video")
    OH, OW = 48000, 46000                    # the luma plane alone is 2.2e9 bytes
    assert OH * OW > 2 ** 31 + 2 ** 25
    y = torch.empty(OH, OW, dtype=torch.uint8, device=DEV)
    u = torch.empty(OH // 2, OW // 2, dtype=torch.uint8, device=DEV)
    v = torch.empty(OH // 2, OW // 2, dtype=torch.uint8, device=DEV)
    try:
        y[-40:].fill_(7), u[-20:].fill_(9), v[-20:].fill_(11)
        src = torch.rand(1, 3, 20, 32, device=DEV)
        table = torch.tensor([[2, 4, OH - 18, OW - 26, 18, 26]], dtype=torch.int64, device=DEV)
        up.tile_scatter_yuv420(src, table, y, u, v, 18, 26)
        got = [y[OH - 40:].cpu(), u[OH // 2 - 20:].cpu(), v[OH // 2 - 20:].cpu()]
        torch.cuda.synchronize()
    finally:
        del y, u, v
        torch.cuda.empty_cache()
    rgb = (src[0, :, 2:20, 4:30].clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    ey, eu, ev = video.rgb_to_yuv420_host(np.ascontiguousarray(rgb))
    ref = [np.full((40, OW), 7, np.uint8), np.full((20, OW // 2), 9, np.uint8), np.full((20, OW // 2), 11, np.uint8)]
    ref[0][22:, OW - 26:], ref[1][11:, OW // 2 - 13:], ref[2][11:, OW // 2 - 13:] = ey, eu, ev
    for g, r in zip(got, ref):
        assert np.array_equal(g.numpy(), r)


# ---------------------------------------------------------------------------------------------- network
def _static(setting):
    nets = amd("elastic_nn.networks")
    st = amd("imagenet_codebase.networks.sr_static")
    net = nets.OFAMobileNetS4(**KW)
    net.set_active_subnet(**setting)
    return st.build_static_net(net.get_active_net_config())


def _randomize(net, seed):
    """he_fout weights, non-trivial BN parameters and statistics, and the output scaled to about unit spread around 0.5, so
    that the 8-bit output is neither constant nor all clamped"""
    g = torch.Generator().manual_seed(seed)
    net.init_model("he_fout")
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.6 + 0.7)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) * 0.2 - 0.1)
                m.running_mean.copy_(torch.rand(m.running_mean.shape, generator=g) * 0.2 - 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.6 + 0.7)
    net = net.to(DEV).eval()
    x = torch.rand(1, 3, 64, 64, generator=g).to(DEV)
    head = net.dec_final_output_conv_block
    with torch.no_grad():
        y = net(x).float()
        s = float(y.std()) / 0.3
        head.conv.weight.div_(s)
        if head.use_bn:
            head.bn.running_mean.div_(s)
            head.bn.bias.add_(0.5 - float(y.mean()) / s)
    amd("ops").clear_infer_cache()
    return net


@pytest.fixture(scope="module")
def small_net():
    return _randomize(_static(dict(ks=3, e=3, d=2, pixel_d=1)), 4)


def _video_frames(n, H, W, seed):
    """smooth in-gamut content plus noise, as planes"""
    video = amd("video")
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        base = torch.rand(3, H // 8 + 2, W // 8 + 2, generator=g)
        smooth = torch.nn.functional.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0]
        img = (smooth * 200 + torch.rand(3, H, W, generator=g) * 55).clamp(0, 255).to(torch.uint8)
        out.append(video.rgb_to_yuv420_host(img.permute(1, 2, 0).contiguous().numpy()))
    return out


@pytest.mark.parametrize("mix_prec,k,H,W", [("f32", 1, 40, 56), ("f32", 8, 40, 56), ("bf16", 2, 40, 56), ("f32", 2, 72, 104)])
def test_upscale_yuv420_equals_the_rgb_path(small_net, mix_prec, k, H, W):
    ops, up = amd("ops"), amd("upscale")
    tu = up.TiledUpscaler(small_net, core=16, mix_prec=mix_prec, self_ensemble=k)
    wins = tu.plan(H, W).windows
    assert len(wins) >= 4
    if H == 72:      # the radius is 17: windows start at odd columns (13, 43) and are 49 rows tall
        assert any(wx % 2 for (_, wx, _, _, _, _) in wins) and tu.plan(H, W).win_h % 2 == 1
    planes = _video_frames(1, H, W, 7)[0]
    y, u, v = _gpu_planes(planes)
    got = tu.upscale_yuv420(y, u, v)
    ref = ops.rgb_to_yuv420_u8(tu.upscale(ops.yuv420_to_rgb_u8(y, u, v)))
    assert got[0].shape == (H * 4, W * 4) and got[1].shape == got[2].shape == (H * 2, W * 2)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert int(got[0].max()) - int(got[0].min()) > 30       # a picture, not a constant
    # numpy planes on the host and another matrix / range go the same way
    got = tu.upscale_yuv420(*planes, matrix="bt709", full_range=True)
    ref = ops.rgb_to_yuv420_u8(tu.upscale(ops.yuv420_to_rgb_u8(y, u, v, "bt709", True)), "bt709", True)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_upscale_yuv420_refusals(small_net):
    up = amd("upscale")
    tu = up.TiledUpscaler(small_net, core=16)
    z = torch.zeros
    with pytest.raises(ValueError, match="even sides"):
        tu.upscale_yuv420(z(39, 56, dtype=torch.uint8), z(19, 28, dtype=torch.uint8), z(19, 28, dtype=torch.uint8))
    with pytest.raises(ValueError, match="even sides"):
        tu.upscale_yuv420(z(40, 55, dtype=torch.uint8), z(20, 27, dtype=torch.uint8), z(20, 27, dtype=torch.uint8))
    with pytest.raises(ValueError):
        tu.upscale_yuv420(z(40, 56, dtype=torch.uint8), z(20, 28, dtype=torch.uint8), z(20, 27, dtype=torch.uint8))
    tu.scale = 3
    with pytest.raises(ValueError, match="even upscale factor"):
        tu.upscale_yuv420(z(40, 56, dtype=torch.uint8), z(20, 28, dtype=torch.uint8), z(20, 28, dtype=torch.uint8))


def test_fused_path_makes_no_rgb_frame(small_net):
    C, up = amd("_C"), amd("upscale")
    tu = up.TiledUpscaler(small_net, core=16)
    y, u, v = _gpu_planes(_video_frames(1, 40, 56, 8)[0])
    tu.upscale_yuv420(y, u, v)
    C.reset_launch_counts()
    tu.upscale_yuv420(y, u, v)
    torch.cuda.synchronize()
    table = C.launch_table()

    def launches(part):
        return sum(n for name, n in table.items() if part in name)

    assert launches("tile_gather_yuv420_kernel") >= 1 and launches("tile_scatter_yuv420_kernel") >= 1
    for name in ("tile_gather_u8_kernel", "tile_scatter_u8_kernel", "yuv420_to_rgb_kernel", "rgb_to_yuv420_kernel"):
        assert launches(name) == 0, (name, table)


# ---------------------------------------------------------------------------------------------- command line
def test_cli_end_to_end(small_net, tmp_path):
    up, video = amd("upscale"), amd("video")
    d = tmp_path / "net"
    d.mkdir()
    (d / "net_config.json").write_text(json.dumps(small_net.config))
    torch.save({"state_dict": {k: t.cpu() for k, t in small_net.state_dict().items()}}, str(d / "static_state_dict.pth"))
    H, W = 40, 56
    frames = _video_frames(3, H, W, 11)
    src, raw = str(tmp_path / "in.y4m"), str(tmp_path / "in.yuv")
    with video.Y4MWriter(src, W, H, fps="30000:1001", interlace="p", aspect="1:1", chroma="420mpeg2") as w, \
            video.RawYUV420Writer(raw, W, H) as r:
        for fr in frames:
            w.write_frame(*fr)
            r.write_frame(*fr)
    tu = up.TiledUpscaler(small_net, core=16)
    expect = [tuple(p.cpu().numpy() for p in tu.upscale_yuv420(*fr)) for fr in frames]

    def run(*args):
        cmd = [sys.executable, os.path.join(ROOT, "upscale_video_ofa_net_sr.py"), "--static", str(d), "--core", "16"]
        r = subprocess.run(cmd + list(args), capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    out = str(tmp_path / "out.y4m")
    text = run("--out", out, src)
    assert "frames/s" in text and "MP/s" in text
    with video.Y4MReader(out) as rd:
        assert (rd.width, rd.height, rd.fps, rd.interlace, rd.aspect, rd.chroma) == (W * 4, H * 4, "30000:1001", "p", "1:1",
                                                                                      "420mpeg2")
        got = [tuple(p.copy() for p in fr) for fr in rd]
    assert open(out, "rb").read().startswith(b"YUV4MPEG2 W224 H160 F30000:1001 ")
    assert len(got) == 3
    for a, b in zip(got, expect):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the same data headerless: the raw output is the Y4M payload; scored against the first run, every PSNR is infinite
    out_raw = str(tmp_path / "out.yuv")
    text = run("--out", out_raw, "--size", "%dx%d" % (W, H), "--reference", out, raw)
    assert open(out_raw, "rb").read() == b"".join(p.tobytes() for fr in got for p in fr)
    q = json.load(open(out_raw + ".quality.json"))
    assert len(q["frames"]) == 3
    assert all(rec["psnr_" + k] == float("inf") and rec["sse_" + k] == 0 for rec in q["frames"] for k in "yuv")
    assert all(q["mean"]["psnr_" + k] == float("inf") for k in "yuv") and "PSNR Y inf" in text
    # one frame of the three
    one = str(tmp_path / "one.y4m")
    run("--out", one, "--frames", "1:2", src)
    with video.Y4MReader(one) as rd:
        sel = [tuple(p.copy() for p in fr) for fr in rd]
    assert len(sel) == 1 and all(np.array_equal(x, y) for x, y in zip(sel[0], expect[1]))
