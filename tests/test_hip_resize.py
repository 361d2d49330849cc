"""Target-size output on the MI355X (`-m gpu`): the resampling scatter (csrc/resize_scatter.hip) alone against resize.py,
then TiledUpscaler's out_size end to end on a small random static network against Pillow's resize of the full-size
output, the YUV paths at both depths, the stream, which kernels launch, and the command line.  Everything is bit-exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, amd
from test_hip_video import COMBOS, DTYPES, _randomize, _static, _tail, _video_frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SH, SW = 144, 192                # the full-size frame of the kernel tests: every ratio below gives an even target
RATIOS = [((1, 1), (2, 1)), ((4, 3), (1, 1)), ((4, 3), (4, 3)), ((2, 1), (8, 3)), ((8, 3), (2, 1)), ((4, 1), (4, 1)),
          ((2, 1), (2, 1))]      # (vertical, horizontal) reduction as fractions; 1 on one axis only
SINKS = ["rgb", "yuv8", "yuv10"]
CASES = [(r, f, s) for r in RATIOS for f in ("bicubic", "lanczos") for s in SINKS]


def _np(t):
    return t.cpu().numpy() if t.dtype != torch.uint16 else t.cpu().view(torch.int16).numpy().view(np.uint16)


def _fit(tab, lo, hi, even):
    """[t0, t1): the target indices whose taps lie inside the source interval [lo, hi)"""
    ok = np.flatnonzero((tab[:, 0] >= lo) & (tab[:, 0] + tab[:, 1] <= hi))
    t0, t1 = int(ok[0]), int(ok[-1]) + 1
    assert np.array_equal(ok, np.arange(t0, t1))
    if even:
        t0, t1 = t0 + t0 % 2, t1 - t1 % 2
    return t0, t1


@pytest.fixture(scope="module")
def whole_frame():
    """a full-size float 'network output' [3, SH, SW]: values below 0 and above 1, and exact quantisation ties"""
    g = torch.Generator().manual_seed(11)
    w = torch.rand(3, SH, SW, generator=g) * 1.4 - 0.2
    w[0, 60, :8] = torch.tensor([0.5, 1.5, 2.5, 3.5, 254.5, 127.5, 0.0, 1.0]) / 255
    w[1, 2, 4:12] = torch.tensor([0.5, 1.5, 2.5, 3.5, 1022.5, 511.5, 0.0, 1.0]) / 1023
    return w


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: "%s-%s-%s" % ("x".join("%d:%d" % r for r in CASES[i][0]),
                                                                              CASES[i][1], CASES[i][2]))
def test_kernel_equals_the_host_definition(case, whole_frame):
    up, resize, video = amd("upscale"), amd("resize"), amd("video")
    ((vn, vd), (hn, hd)), filt, sink = CASES[case]
    # CASES runs through the sinks fastest: case // 3 counts (ratio, filter) pairs, so every sink meets every dtype, and
    # every (sink, dtype) pair meets every pad
    dtype, pad = DTYPES[(case // 3 + case) % 3], (0, 1, 3)[(case // 9) % 3]
    yuv = sink != "rgb"
    depth = 10 if sink == "yuv10" else 8
    TH, TW = SH * vd // vn, SW * hd // hn
    sh, sw = (25 if vn <= 2 * vd else 57), (41 if hn <= 2 * hd else 73)
    vals = whole_frame.to(dtype)
    q = resize.quantise(vals.float().numpy(), depth)
    ref = np.ascontiguousarray(np.moveaxis(resize.resize_host(q, TH, TW, filt, depth), 0, 2))        # HWC
    vt, ht = resize.axis_table(SH, TH, filt, depth), resize.axis_table(SW, TW, filt, depth)
    # window 0 at an odd origin inside the frame, window 1 against the bottom right corner (odd origin too), window 2 with
    # an empty extent; the rectangles are all the target pixels whose taps lie inside the window
    origins = [(1, 3), (SH - sh, SW - sw), (5, 7)]
    assert all(o % 2 for o in origins[0] + origins[1])
    rows, rects = [], []
    for i, (oy, ox) in enumerate(origins):
        ty0, ty1 = _fit(vt, oy, oy + sh, yuv)
        tx0, tx1 = _fit(ht, ox, ox + sw, yuv)
        assert ty1 > ty0 and tx1 > tx0
        if i == 1:
            assert ty1 == TH and tx1 == TW
            rows.append([oy, ox, ty0, tx0, ty1 - ty0 + 6, tx1 - tx0 + 6])      # cut by the frame edge
            rects.append((ty0, tx0, ty1, tx1))
        elif i == 2:
            rows.append([oy, ox, ty0, tx0, 0, tx1 - tx0])                      # empty: writes nothing
        else:
            rows.append([oy, ox, ty0, tx0, ty1 - ty0, tx1 - tx0])
            rects.append((ty0, tx0, ty1, tx1))
    src = _tail(torch.stack([vals[:, oy:oy + sh, ox:ox + sw] for (oy, ox) in origins]), pad)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    vtab, htab = torch.from_numpy(vt).to(DEV), torch.from_numpy(ht).to(DEV)
    max_eh, max_ew = max(r[2] - r[0] for r in rects), max(r[3] - r[1] for r in rects)
    rng = np.random.RandomState(case)
    if not yuv:
        base = rng.randint(0, 256, (TH, TW, 3)).astype(np.uint8)
        img = _tail(torch.from_numpy(base), pad)
        up.tile_resize_scatter(src, table, vtab, htab, img, max_eh, max_ew)
        exp = base.copy()
        for (y0, x0, y1, x1) in rects:
            exp[y0:y1, x0:x1] = ref[y0:y1, x0:x1]
        assert np.array_equal(_np(img), exp)
        return
    matrix, full = COMBOS[case % 4]
    dt = np.uint8 if depth == 8 else np.uint16
    peak = 256 if depth == 8 else 1024
    base = [rng.randint(0, peak, s).astype(dt) for s in ((TH, TW), (TH // 2, TW // 2), (TH // 2, TW // 2))]
    planes = [_tail(torch.from_numpy(b.view(np.int16) if depth == 10 else b), pad) for b in base]
    if depth == 10:
        planes = [p.view(torch.uint16) for p in planes]
    up.tile_resize_scatter_yuv420(src, table, vtab, htab, planes[0], planes[1], planes[2], max_eh, max_ew, matrix, full)
    enc = video.rgb_to_yuv420_host(ref, matrix, full, depth)
    exp = [b.copy() for b in base]
    for (y0, x0, y1, x1) in rects:
        exp[0][y0:y1, x0:x1] = enc[0][y0:y1, x0:x1]
        for k in (1, 2):
            exp[k][y0 // 2:y1 // 2, x0 // 2:x1 // 2] = enc[k][y0 // 2:y1 // 2, x0 // 2:x1 // 2]
    for got, e in zip(planes, exp):
        assert np.array_equal(_np(got), e)


def test_wild_tables_give_values_not_faults(whole_frame):
    """table rows and coefficient rows far outside every tensor: the kernel clamps them, so it writes values, wrong ones,
    into the clamped rectangles and nothing anywhere else"""
    up, resize = amd("upscale"), amd("resize")
    TH, TW = 72, 96
    src = _tail(whole_frame[None, :, :40, :56].contiguous(), 1)
    vt, ht = resize.coeff_table(SH, TH, "lanczos"), resize.coeff_table(SW, TW, "lanczos")
    vt[3] = (-10 ** 9, 10 ** 6, *vt[3, 2:])
    vt[5, :2] = (2 ** 31 - 1, -7)
    ht[2, :2] = (10 ** 9, 10 ** 9)
    ht[9, :2] = (-2 ** 31, 2 ** 31 - 1)
    table = torch.tensor([[-2 ** 40, 2 ** 40, -5, -5, 10 ** 12, 10 ** 12], [2 ** 62, -2 ** 62, 64, 80, 30, 40]],
                         dtype=torch.int64, device=DEV)
    # the destination lies 3 bytes into a zeroed allocation with 4096 bytes behind it
    n, pad, behind = TH * TW * 3, 3, 4096
    buf = torch.zeros(pad + n + behind, dtype=torch.uint8, device=DEV)
    img = buf[pad:pad + n].view(TH, TW, 3)
    up.tile_resize_scatter(src.expand(2, -1, -1, -1).contiguous(), table, torch.from_numpy(vt).to(DEV),
                           torch.from_numpy(ht).to(DEV), img, 64, 80)
    torch.cuda.synchronize()
    # row 0 clamps to the target's origin and the extent bounds (64 x 80), row 1 to what the target leaves at (64, 80)
    inside = np.zeros((TH, TW), bool)
    inside[0:64, 0:80] = True
    inside[64:72, 80:96] = True
    got = buf.cpu().numpy()
    out = got[pad:pad + n].reshape(TH, TW, 3)
    assert not got[:pad].any() and not got[pad + n:].any()
    assert not out[~inside].any()
    assert out[0:64, 0:80].any() and out[64:72, 80:96].any()


def test_wrappers_refuse_bad_arguments():
    up = amd("upscale")
    src = torch.zeros(1, 3, 8, 8, device=DEV)
    table = torch.zeros(1, 6, dtype=torch.int64, device=DEV)
    tab = torch.zeros(4, 5, dtype=torch.int32, device=DEV)
    img = torch.zeros(4, 4, 3, dtype=torch.uint8, device=DEV)
    up.tile_resize_scatter(src, table, tab, tab, img, 4, 4)
    with pytest.raises(ValueError, match="coefficient table"):
        up.tile_resize_scatter(src, table, tab[:3], tab, img, 4, 4)                    # rows != TH
    with pytest.raises(ValueError, match="coefficient table"):
        up.tile_resize_scatter(src, table, tab, torch.zeros(4, 28, dtype=torch.int32, device=DEV), img, 4, 4)   # 26 taps
    with pytest.raises(ValueError, match="int64 table"):
        up.tile_resize_scatter(src, table.int(), tab, tab, img, 4, 4)
    with pytest.raises(ValueError, match="HWC uint8"):
        up.tile_resize_scatter(src, table, tab, tab, img.float(), 4, 4)


# ---------------------------------------------------------------------------------------------- network
@pytest.fixture(scope="module")
def small_net():
    # init_model draws the conv weights from torch's global generator: seed it here (and put it back), so that the
    # network, and with it every value compared below, is the same whichever tests ran before
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(4)
        return _randomize(_static(dict(ks=3, e=3, d=2, pixel_d=1)), 4)


def _varied(a, depth=8):
    """guard against a vacuous comparison: a constant or clamped output equals its resize whatever the coefficients
    are.  A span of more than 16 8-bit levels is enough for a tap displaced by one pixel, or a side lobe of the wrong
    sign (lanczos' is about -0.09), to move the result by more than a rounding step."""
    a = np.asarray(a).astype(np.int64)
    return int(a.max()) - int(a.min()) > 16 * (1 if depth == 8 else 4)


@pytest.fixture(scope="module")
def image():
    H, W = 72, 104
    g = torch.Generator().manual_seed(21)
    base = torch.rand(3, H // 8 + 2, W // 8 + 2, generator=g)
    smooth = torch.nn.functional.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0]
    return (smooth * 200 + torch.rand(3, H, W, generator=g) * 55).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


@pytest.fixture(scope="module")
def full_size(small_net, image):
    """upscale(img) per precision, computed once"""
    up = amd("upscale")
    return {p: up.TiledUpscaler(small_net, core=16, mix_prec=p).upscale(image).cpu().numpy() for p in ("f32", "bf16", "f16")}


def _pil(arr, TH, TW, filt):
    from PIL import Image
    return np.asarray(Image.fromarray(arr).resize((TW, TH), {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[filt]))


@pytest.mark.parametrize("mix_prec", ["f32", "bf16", "f16"])
def test_upscale_out_size_equals_pillow_of_the_full_size_output(small_net, image, full_size, mix_prec):
    up = amd("upscale")
    tu = up.TiledUpscaler(small_net, core=16, mix_prec=mix_prec)
    for (TH, TW), filt in (((108, 156), "lanczos"), ((144, 208), "bicubic")):
        plan = tu.plan(72, 104, (TH, TW), filt)
        assert len(plan) >= 4 and any(w[1] % 2 for w in plan.windows) and plan.halo > tu.halo
        got = tu.upscale(image, out_size=(TH, TW), resample=filt)
        assert got.shape == (TH, TW, 3) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), _pil(full_size[mix_prec], TH, TW, filt))
        whole = tu.upscale(image, whole=True, out_size=(TH, TW), resample=filt)
        assert torch.equal(got, whole)
    assert _varied(got.cpu().numpy())
    # the network's own size: the call without out_size, and numpy input goes the same way
    assert np.array_equal(tu.upscale(image.numpy(), out_size=(288, 416)).cpu().numpy(), full_size[mix_prec])
    # anamorphic, one axis unchanged
    got = tu.upscale(image, out_size=(288, 200))
    assert np.array_equal(got.cpu().numpy(), _pil(full_size[mix_prec], 288, 200, "lanczos"))


def test_upscale_out_size_with_self_ensemble(small_net, image):
    up = amd("upscale")
    tu = up.TiledUpscaler(small_net, core=16, self_ensemble=8)
    got = tu.upscale(image, out_size=(108, 156))
    assert np.array_equal(got.cpu().numpy(), _pil(tu.upscale(image).cpu().numpy(), 108, 156, "lanczos"))


def test_upscale_out_size_refusals(small_net, image):
    up = amd("upscale")
    tu = up.TiledUpscaler(small_net, core=16)
    with pytest.raises(ValueError, match=r"width 104 \.\. 416, height 72 \.\. 288"):
        tu.upscale(image, out_size=(71, 200))
    with pytest.raises(ValueError, match=r"width 104 \.\. 416"):
        tu.upscale(image, out_size=(100, 417))
    with pytest.raises(ValueError, match="resample must be one of"):
        tu.upscale(image, out_size=(100, 200), resample="box")
    y, u, v = (torch.zeros(s, dtype=torch.uint8) for s in ((40, 56), (20, 28), (20, 28)))
    with pytest.raises(ValueError, match="even sides"):
        tu.upscale_yuv420(y, u, v, out_size=(85, 120))
    with pytest.raises(ValueError, match="even sides"):
        tu.yuv420_stream(out_size=(84, 121)).upscale(y, u, v)
    with pytest.raises(ValueError, match="resample must be one of"):
        tu.yuv420_stream(out_size=(84, 120), resample="nearest")


# ---------------------------------------------------------------------------------------------- YUV
def _full_size_float(tu, planes, matrix, full):
    """the network's fp32 output [3, H*s, W*s] for a YUV frame, assembled from the window cores of the plain plan (what
    upscale_float does for an RGB image), gathered by the fused decode"""
    up = amd("upscale")
    dev, (y, u, v), H, W = tu._yuv420_frame(*planes)
    s = tu.scale
    out = torch.empty(3, H * s, W * s, dtype=torch.float32, device=dev)

    def sink(t, real, table, wins, plan):
        for i, (wy, wx, cy, cx, ch, cw) in enumerate(wins):
            out[:, cy * s:(cy + ch) * s, cx * s:(cx + cw) * s] = \
                t[i, :, (cy - wy) * s:(cy - wy + ch) * s, (cx - wx) * s:(cx - wx + cw) * s].float()

    tu._run_windows(H, W, dev, False, sink,
                    lambda origins, h, w: up.tile_gather_yuv420(y, u, v, origins, h, w, tu.dtype, matrix, full))
    return out.cpu().numpy()


def _frames10(n, H, W, seed):
    video = amd("video")
    out = []
    for fr in _video_frames(n, H, W, seed):
        rgb = video.yuv420_to_rgb_host(*fr).astype(np.uint16) * 4 + np.random.RandomState(seed).randint(0, 4, (H, W, 3)).astype(np.uint16)
        out.append(video.rgb_to_yuv420_host(rgb, depth=10))
    return out


@pytest.mark.parametrize("in_depth,out_depth,mix_prec,matrix,full", [(8, None, "f32", "bt601", False), (8, 10, "f32", "bt709", True),
                                                                     (10, None, "bf16", "bt601", False), (8, None, "f16", "bt601", True)])
def test_upscale_yuv420_out_size_equals_the_definition(small_net, in_depth, out_depth, mix_prec, matrix, full):
    up, resize, video = amd("upscale"), amd("resize"), amd("video")
    H, W, TH, TW = 72, 104, 108, 156
    tu = up.TiledUpscaler(small_net, core=16, mix_prec=mix_prec)
    planes = (_video_frames if in_depth == 8 else _frames10)(1, H, W, 31)[0]
    depth = in_depth if out_depth is None else out_depth
    assert len(tu.plan(H, W, (TH, TW), "lanczos", True)) >= 4
    got = tu.upscale_yuv420(*planes, matrix=matrix, full_range=full, out_depth=out_depth, out_size=(TH, TW))
    q = resize.quantise(_full_size_float(tu, planes, matrix, full), depth)
    rgb = np.ascontiguousarray(np.moveaxis(resize.resize_host(q, TH, TW, "lanczos", depth), 0, 2))
    ref = video.rgb_to_yuv420_host(rgb, matrix, full, depth)
    assert got[0].shape == (TH, TW) and got[1].shape == got[2].shape == (TH // 2, TW // 2)
    for a, b in zip(got, ref):
        assert np.array_equal(_np(a), b)
    assert _varied(_np(got[0]), depth)
    if depth == 8 and in_depth == 8:
        # the same through the library's own kernels: encode of the host resize of the full-size RGB path
        ops = amd("ops")
        y, u, v = (torch.from_numpy(p).to(DEV) for p in planes)
        full_rgb = tu.upscale(ops.yuv420_to_rgb_u8(y, u, v, matrix, full)).cpu().numpy()
        small = torch.from_numpy(resize.resize_host(full_rgb, TH, TW, "lanczos", hwc=True)).to(DEV)
        for a, b in zip(got, ops.rgb_to_yuv420_u8(small, matrix, full)):
            assert torch.equal(a, b)
        whole = tu.upscale_yuv420(*planes, matrix=matrix, full_range=full, whole=True, out_size=(TH, TW))
        for a, b in zip(got, whole):
            assert torch.equal(a, b)


def test_stream_with_out_size_reuses_windows(small_net):
    up = amd("upscale")
    H, W, TH, TW = 72, 104, 108, 156
    tu = up.TiledUpscaler(small_net, core=16, batch=2)
    f0 = _video_frames(1, H, W, 41)[0]
    f2 = tuple(p.copy() for p in f0)
    f2[0][:6, :6] ^= 0x55                                     # one corner changes
    st = tu.yuv420_stream(out_size=(TH, TW), resample="bicubic")
    n = len(tu.plan(H, W, (TH, TW), "bicubic", True))
    runs = []
    for fr in (f0, f0, f2):
        got = st.upscale(*fr)
        assert got[0].shape == (TH, TW)
        for a, b in zip(got, tu.upscale_yuv420(*fr, out_size=(TH, TW), resample="bicubic")):
            assert torch.equal(a, b)
        runs.append(st.stats.run)
    assert runs[0] == n == st.stats.windows and runs[1] == 0 and 0 < runs[2] < n


def test_only_the_resampling_scatter_launches(small_net, image):
    C, up = amd("_C"), amd("upscale")
    tu = up.TiledUpscaler(small_net, core=16)
    planes = _video_frames(1, 72, 104, 51)[0]
    tu.upscale(image, out_size=(108, 156))
    tu.upscale_yuv420(*planes, out_size=(108, 156))
    C.reset_launch_counts()
    tu.upscale(image, out_size=(108, 156))
    tu.upscale_yuv420(*planes, out_size=(108, 156))
    tu.upscale_yuv420(*planes, out_size=(108, 156), out_depth=10)
    torch.cuda.synchronize()
    table = C.launch_table()

    def launches(part):
        return sum(n for name, n in table.items() if part in name)

    assert launches("tile_resize_scatter_kernel") >= 3
    for name in ("tile_scatter_u8_kernel", "tile_scatter_yuv420_kernel", "rs_horizontal_kernel", "rs_vertical_kernel",
                 "rs_coeff_kernel", "rgb_to_yuv420_kernel", "yuv420_to_rgb_kernel"):
        assert launches(name) == 0, (name, table)
    # and without out_size nothing changes: the full-size scatters, not the new one
    C.reset_launch_counts()
    tu.upscale(image)
    tu.upscale(image, out_size=(288, 416))
    torch.cuda.synchronize()
    table = C.launch_table()
    assert launches("tile_resize_scatter_kernel") == 0 and launches("tile_scatter_u8_kernel") >= 2


# ---------------------------------------------------------------------------------------------- command line
def test_cli_out_size_end_to_end(small_net, tmp_path):
    up, video = amd("upscale"), amd("video")
    d = tmp_path / "net"
    d.mkdir()
    (d / "net_config.json").write_text(json.dumps(small_net.config))
    torch.save({"state_dict": {k: t.cpu() for k, t in small_net.state_dict().items()}}, str(d / "static_state_dict.pth"))
    H, W = 40, 56
    frames = _video_frames(3, H, W, 61)
    src = str(tmp_path / "in.y4m")
    with video.Y4MWriter(src, W, H, fps="30000:1001", interlace="p", aspect="1:1", chroma="420mpeg2") as w:
        for fr in frames:
            w.write_frame(*fr)
    tu = up.TiledUpscaler(small_net, core=16)
    expect = [tuple(p.cpu().numpy() for p in tu.upscale_yuv420(*fr, out_size=(84, 120))) for fr in frames]
    out = str(tmp_path / "out.y4m")
    cmd = [sys.executable, os.path.join(ROOT, "upscale_video_ofa_net_sr.py"), "--static", str(d), "--core", "16", "--out", out,
           "--out-size", "120x84", src]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lanczos to 120x84" in r.stdout
    assert open(out, "rb").read().startswith(b"YUV4MPEG2 W120 H84 F30000:1001 ")
    with video.Y4MReader(out) as rd:
        assert (rd.width, rd.height, rd.chroma) == (120, 84, "420mpeg2")
        got = [tuple(p.copy() for p in fr) for fr in rd]
    assert len(got) == 3
    for a, b in zip(got, expect):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
