"""Keeping an image's mode through upscaling on the MI355X (`-m gpu`): the two kernels of csrc/mode_io.hip alone against
modes.py, the same two on misaligned, guard-banded operands, TiledUpscaler.upscale_image end to end on a small random static
network against Pillow applied to upscale() of the RGB image, which kernels launch, and the command line.  Everything is
bit-exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import placed
from conftest import ROOT, amd
from test_hip_video import _randomize, _static

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILTERS = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
# alpha plane -> target (H, W): one tile; one ragged tile; several tiles, ragged both ways (x4, x2, non-integer ratios
# and an odd target); identity on one axis
SIZES = [((1, 1), (4, 4)), ((2, 3), (8, 12)), ((9, 13), (36, 52)), ((23, 37), (92, 148)), ((23, 37), (46, 74)),
         ((23, 37), (61, 101)), ((23, 37), (23, 74)), ((23, 37), (92, 37))]
H0, W0 = 40, 52          # the end-to-end image
CORE = 8                 # its core: the network's receptive radius is 17, so a core of 32 makes ONE 40 x 52 window


def _rand(shape, seed):
    a = np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)
    a.reshape(-1)[:4] = [0, 255, 255, 0][:min(a.size, 4)]            # the extremes are there at every size
    return a


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_pack_kernel_equals_the_host_definition(size, C, filt):
    modes, ops = amd("modes"), amd("ops")
    (H, W), (TH, TW) = size
    rgb, alpha = _rand((TH, TW, 3), 3 * TH + TW), _rand((H, W), 5 * H + W)
    if C == 1:
        got = ops.mode_pack_u8(torch.from_numpy(rgb).to(DEV), 1)
        ref = modes.join_host(rgb, 1)
    else:
        vt, ht = (torch.from_numpy(t).to(DEV) for t in modes.alpha_tables(H, W, TH, TW, filt))
        got = ops.mode_pack_u8(torch.from_numpy(rgb).to(DEV), C, torch.from_numpy(alpha).to(DEV), vt, ht)
        ref = modes.join_host(rgb, C, modes.alpha_host(alpha, TH, TW, filt))
    assert got.shape == (TH, TW, C) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), ref)


@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (23, 37), (33, 67)])          # the last: more than one workgroup
def test_unpack_kernel_equals_split_host(H, W, C):
    modes, ops = amd("modes"), amd("ops")
    img = _rand((H, W, C), 7 * H + W + C)
    rgb, alpha = ops.mode_unpack_u8(torch.from_numpy(img).to(DEV))
    ref_rgb, ref_alpha = modes.split_host(img)
    assert np.array_equal(rgb.cpu().numpy(), ref_rgb)
    assert (alpha is None) == (ref_alpha is None) == (C == 1)
    if alpha is not None:
        assert np.array_equal(alpha.cpu().numpy(), ref_alpha)


def test_wrappers_refuse_bad_operands():
    modes, ops = amd("modes"), amd("ops")
    rgb = torch.zeros(8, 12, 3, dtype=torch.uint8, device=DEV)
    alpha = torch.zeros(2, 3, dtype=torch.uint8, device=DEV)
    vt, ht = (torch.from_numpy(t).to(DEV) for t in modes.alpha_tables(2, 3, 8, 12, "lanczos"))
    for bad in (lambda: ops.mode_pack_u8(rgb, 3), lambda: ops.mode_pack_u8(rgb, 4), lambda: ops.mode_pack_u8(rgb, 1, alpha, vt, ht),
                lambda: ops.mode_pack_u8(rgb, 4, alpha, ht, vt), lambda: ops.mode_pack_u8(rgb, 4, alpha, vt.long(), ht),
                lambda: ops.mode_pack_u8(rgb.float(), 1), lambda: ops.mode_pack_u8(rgb[:, ::2], 1),
                lambda: ops.mode_pack_u8(rgb, 4, torch.zeros(9, 3, dtype=torch.uint8, device=DEV), vt, ht),
                lambda: ops.mode_pack_u8(rgb, 2, alpha, vt, ht, out=torch.zeros(8, 12, 4, dtype=torch.uint8, device=DEV)),
                lambda: ops.mode_unpack_u8(rgb), lambda: ops.mode_unpack_u8(rgb[:, :, :2]),
                lambda: ops.mode_unpack_u8(torch.zeros(4, 4, 1, dtype=torch.uint8, device=DEV), alpha=alpha)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------- placement
@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("where", ["P0", "P1"])
def test_kernels_on_guard_banded_operands(where, C):
    """every operand of both kernels at an aligned base (P0: the 4-byte accesses run) and one element off it (P1: none
    is legal), between guard bands: the results are the host definition's and no byte outside a payload changed"""
    modes, ops = amd("modes"), amd("ops")
    (H, W), (TH, TW) = (23, 37), (61, 101)

    def put(arr, role, name):
        t = torch.from_numpy(arr).to(DEV)
        return placed.place(t, placed.lead_of(where, t.element_size()), role, name)

    img = _rand((H, W, C), 40 + C)
    ref_rgb, ref_alpha = modes.split_host(img)
    p_img, p_rgb = put(img, "in", "img"), put(ref_rgb, "out", "rgb")
    p_alpha = put(ref_alpha, "out", "alpha") if C != 1 else None
    ops.mode_unpack_u8(p_img, rgb=p_rgb, alpha=p_alpha)

    rgb_out = _rand((TH, TW, 3), 50 + C)
    q_rgb = put(rgb_out, "in", "rgb_out")
    q_out = put(np.zeros((TH, TW, C), np.uint8), "out", "out")
    q_alpha = q_vt = q_ht = None
    if C == 1:
        ops.mode_pack_u8(q_rgb, 1, out=q_out)
        ref = modes.join_host(rgb_out, 1)
    else:
        vt, ht = modes.alpha_tables(H, W, TH, TW, "lanczos")
        q_alpha, q_vt, q_ht = put(ref_alpha, "in", "alpha_src"), put(vt, "in", "vtab"), put(ht, "in", "htab")
        ops.mode_pack_u8(q_rgb, C, q_alpha, q_vt, q_ht, out=q_out)
        ref = modes.join_host(rgb_out, C, modes.alpha_host(ref_alpha, TH, TW, "lanczos"))
    torch.cuda.synchronize()
    placed.check_all(p_img, p_rgb, p_alpha, q_rgb, q_out, q_alpha, q_vt, q_ht)
    assert p_img.data_ptr() % 16 == q_out.data_ptr() % 16 == (0 if where == "P0" else 1)
    assert np.array_equal(p_rgb.cpu().numpy(), ref_rgb)
    if C != 1:
        assert np.array_equal(p_alpha.cpu().numpy(), ref_alpha)
    assert np.array_equal(q_out.cpu().numpy(), ref)


# ---------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def small_net():
    # init_model draws the conv weights from torch's global generator: seed it here (and put it back), so that the
    # network, and with it every value compared below, is the same whichever tests ran before
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(4)
        return _randomize(_static(dict(ks=3, e=3, d=2, pixel_d=1)), 4)


@pytest.fixture(scope="module")
def easy_net():
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(5)
        return _randomize(_static(dict(ks=3, e=3, d=2, pixel_d=0)), 5)


@pytest.fixture(scope="module")
def upscalers(small_net):
    up = amd("upscale")
    return {p: up.TiledUpscaler(small_net, core=CORE, mix_prec=p) for p in ("f32", "bf16")}


def _image(C, seed=21):
    """[H0, W0, C] uint8: smooth colour plus noise, and an alpha plane with opaque, transparent and soft regions"""
    g = torch.Generator().manual_seed(seed + C)
    base = torch.rand(4, H0 // 8 + 2, W0 // 8 + 2, generator=g)
    smooth = torch.nn.functional.interpolate(base[None], size=(H0, W0), mode="bilinear", align_corners=False)[0]
    img = (smooth * 200 + torch.rand(4, H0, W0, generator=g) * 55).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy().copy()
    img[:10, :, 3] = 255
    img[-8:, 20:, 3] = 0
    return np.ascontiguousarray({1: img[:, :, :1], 2: img[:, :, [0, 3]], 3: img[:, :, :3], 4: img}[C])


def _pil_image(img):
    return Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img, {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[img.shape[2]])


def _rgb_in(img):
    return np.array(_pil_image(img).convert("RGB"))


def _expected(img, rgb_out, filt="bicubic"):
    """Pillow and numpy only: convert("L") of the RGB output, the source alpha resized to its size"""
    C = img.shape[2]
    TH, TW = rgb_out.shape[:2]
    parts = [rgb_out] if C >= 3 else [np.asarray(Image.fromarray(rgb_out, "RGB").convert("L"))[:, :, None]]
    if C in (2, 4):
        parts.append(np.asarray(Image.fromarray(np.ascontiguousarray(img[:, :, C - 1]), "L").resize((TW, TH), FILTERS[filt]))[:, :, None])
    return np.concatenate(parts, axis=2)


def _varied(a):
    a = np.asarray(a).astype(np.int64)
    return int(a.max()) - int(a.min()) > 16


@pytest.mark.parametrize("mix_prec", ["f32", "bf16"])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_upscale_image_equals_pillow_on_the_rgb_upscale(upscalers, C, mix_prec):
    tu = upscalers[mix_prec]
    assert len(tu.plan(H0, W0)) >= 4
    img = _image(C)
    rgb_out = tu.upscale(_rgb_in(img)).cpu().numpy()
    assert _varied(rgb_out)
    got = tu.upscale_image(img)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (4 * H0, 4 * W0, C)
    assert np.array_equal(got.cpu().numpy(), _expected(img, rgb_out))
    assert torch.equal(got, tu.upscale_image(torch.from_numpy(img).to(DEV), whole=True))       # tiled = whole, GPU input
    assert torch.equal(got, tu.upscale_image(torch.from_numpy(img)))                           # and the same again
    if C != 1:
        lan = tu.upscale_image(img, alpha_resample="lanczos").cpu().numpy()
        assert np.array_equal(lan, _expected(img, rgb_out, "lanczos"))
        assert _varied(lan[:, :, C - 1]) and not np.array_equal(lan, got.cpu().numpy())


def test_upscale_image_with_one_window_at_core_32(small_net):
    up = amd("upscale")
    tu = up.TiledUpscaler(small_net, core=32)
    img = _image(4)
    got = tu.upscale_image(img)
    assert np.array_equal(got.cpu().numpy(), _expected(img, tu.upscale(_rgb_in(img)).cpu().numpy()))
    assert torch.equal(got, tu.upscale_image(img, whole=True))


@pytest.mark.parametrize("C", [1, 2, 4])
def test_upscale_image_out_size_resizes_the_source_alpha(upscalers, C):
    tu = upscalers["f32"]
    img = _image(C)
    TH, TW = 101, 131
    rgb_out = tu.upscale(_rgb_in(img), out_size=(TH, TW), resample="lanczos").cpu().numpy()
    got = tu.upscale_image(img, out_size=(TH, TW), resample="lanczos")
    assert got.shape == (TH, TW, C)
    # the alpha is the source alpha resized straight to 131 x 101, not a resize of the x4 alpha
    assert np.array_equal(got.cpu().numpy(), _expected(img, rgb_out))
    assert torch.equal(got, tu.upscale_image(img, whole=True, out_size=(TH, TW), resample="lanczos"))
    if C != 1:
        lan = tu.upscale_image(img, out_size=(TH, TW), resample="bicubic", alpha_resample="lanczos").cpu().numpy()
        rgb_bic = tu.upscale(_rgb_in(img), out_size=(TH, TW), resample="bicubic").cpu().numpy()
        assert np.array_equal(lan, _expected(img, rgb_bic, "lanczos"))
        # one axis unchanged: that axis of the alpha is not resampled
        one = tu.upscale_image(img, out_size=(H0, 4 * W0)).cpu().numpy()
        assert np.array_equal(one, _expected(img, tu.upscale(_rgb_in(img), out_size=(H0, 4 * W0)).cpu().numpy()))


@pytest.mark.parametrize("C", [2, 4])
def test_upscale_image_with_self_ensemble(small_net, C):
    up = amd("upscale")
    tu = up.TiledUpscaler(small_net, core=CORE, self_ensemble=8)
    img = _image(C)
    got = tu.upscale_image(img).cpu().numpy()
    assert np.array_equal(got, _expected(img, tu.upscale(_rgb_in(img)).cpu().numpy()))


@pytest.mark.parametrize("C", [1, 4])
def test_upscale_image_with_routing(small_net, easy_net, C):
    up = amd("upscale")
    tu = up.TiledUpscaler(small_net, core=CORE, easy_net=easy_net, easy_threshold=0)
    img = _image(C)
    act = tu.window_activity(_rgb_in(img))
    tu.set_easy_threshold(float(act.median()))
    got = tu.upscale_image(img).cpu().numpy()
    stats = dict(tu.route_stats)
    assert stats["easy"] > 0 and stats["hard"] > 0 and stats["easy"] + stats["hard"] == len(tu.plan(H0, W0))
    assert np.array_equal(got, _expected(img, tu.upscale(_rgb_in(img)).cpu().numpy()))
    assert tu.route_stats == stats


def test_three_channels_are_upscale_itself(upscalers):
    tu = upscalers["f32"]
    img = _image(3)
    assert torch.equal(tu.upscale_image(img), tu.upscale(img))
    assert torch.equal(tu.upscale_image(img, out_size=(101, 131), resample="bicubic", alpha_resample="lanczos"),
                       tu.upscale(img, out_size=(101, 131), resample="bicubic"))
    for bad in (np.zeros((8, 8, 5), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.float32)):
        with pytest.raises(ValueError):
            tu.upscale_image(bad)
    with pytest.raises(ValueError, match="resample must be one of"):
        tu.upscale_image(_image(4), alpha_resample="box")
    with pytest.raises(ValueError):
        tu.upscale(_image(4))                                         # upscale() itself still takes RGB only


def test_only_the_two_mode_kernels_are_added(upscalers):
    from torch.profiler import ProfilerActivity, profile
    C = amd("_C")
    tu = upscalers["f32"]
    img = torch.from_numpy(_image(4)).to(DEV)
    rgb = torch.from_numpy(_rgb_in(_image(4))).to(DEV)
    tu.upscale(rgb), tu.upscale_image(img)                # warm-up: graphs captured, tables uploaded
    torch.cuda.synchronize()

    def run(fn, arg):
        C.reset_launch_counts()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(arg)
            torch.cuda.synchronize()
        host = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU}
        dev = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
        return C.launch_table(), host, dev

    base, base_host, base_dev = run(tu.upscale, rgb)
    table, host, dev = run(tu.upscale_image, img)
    added = {k: n - base.get(k, 0) for k, n in table.items() if n != base.get(k, 0)}
    assert sorted(added.values()) == [1, 1] and all(k in table for k in base), (added, base)
    assert sum("mode_pack_kernel" in k for k in added) == sum("mode_unpack_kernel" in k for k in added) == 1, added
    assert any("tile_gather_u8_kernel" in k for k in table) and any("tile_scatter_u8_kernel" in k for k in table)
    # no ATen compute kernel: on the device only the two new kernels come on top of upscale()'s
    new_dev = [n for n in dev - base_dev if "mode_pack_kernel" not in n and "mode_unpack_kernel" not in n]
    assert not new_dev, new_dev
    assert any("mode_pack_kernel" in n for n in dev) and any("mode_unpack_kernel" in n for n in dev), "the profiler saw neither"
    bad = [n for n in host - base_host if n in ("aten::cat", "aten::stack", "aten::index", "aten::index_select", "aten::expand",
                                    "aten::repeat", "aten::mul", "aten::clone", "aten::permute")]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- command line
def test_cli_keep_mode_end_to_end(small_net, upscalers, tmp_path):
    cli = __import__("upscale_ofa_net_sr")
    d = tmp_path / "net"
    d.mkdir()
    (d / "net_config.json").write_text(json.dumps(small_net.config))
    torch.save({"state_dict": {k: t.cpu() for k, t in small_net.state_dict().items()}}, str(d / "static_state_dict.pth"))
    src = tmp_path / "in"
    src.mkdir()
    _pil_image(_image(4)).save(str(src / "rgba.png"))
    _pil_image(_image(2)).save(str(src / "la.png"))
    _pil_image(_image(1)).save(str(src / "l.png"))
    _pil_image(_image(3)).quantize(16).save(str(src / "pal.png"), transparency=3)
    names = {"rgba": "RGBA", "la": "LA", "l": "L", "pal": "RGBA"}
    tu = upscalers["f32"]

    def run(out, *flags):
        cmd = [sys.executable, os.path.join(ROOT, "upscale_ofa_net_sr.py"), "--static", str(d), "--out", str(out), "--core",
               str(CORE)] + list(flags) + [str(src)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    kept = run(tmp_path / "kept", "--keep-mode")
    plain = run(tmp_path / "plain")
    for name, mode in names.items():
        path = str(src / (name + ".png"))
        with Image.open(str(tmp_path / "kept" / (name + ".png"))) as im:
            assert im.mode == mode, (name, im.mode)
            got = np.asarray(im)
        got = got if got.ndim == 3 else got[:, :, None]
        img = cli.decode_keep(path)
        assert img.shape[2] == len(mode)
        assert np.array_equal(got, tu.upscale_image(img).cpu().numpy()), name
        with Image.open(str(tmp_path / "plain" / (name + ".png"))) as im:
            assert im.mode == "RGB"
            assert np.array_equal(np.asarray(im), tu.upscale(cli.decode(path)).cpu().numpy()), name
    # the printed lines do not depend on the flag, the timing line apart
    strip = lambda s: [l for l in s.splitlines() if "MP/s" not in l]
    assert strip(kept) == strip(plain) and "MP/s" in kept
