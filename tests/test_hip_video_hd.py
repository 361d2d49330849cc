"""10-bit YUV 4:2:0 on the MI355X (`-m gpu`): the 16-bit tile moves (csrc/yuv.hip on uint16 planes) and the 16-bit window
diff (csrc/reuse.hip) against the host definition (video.py with depth=10), TiledUpscaler.upscale_yuv420 at the depth
combinations 10 -> 10, 8 -> 10 and 10 -> 8 against a reference composed of pieces that hold no new kernel, YUV420Stream on
10-bit frames, and the command line.  Every plane is the tail slice of a larger allocation (pads of 0, 1 and 3 elements:
a 2-byte aligned base that is not 4-, 8- or 16-byte aligned for pad 1), so a read past its end leaves the allocation.
Everything is bit-exact.  uint16 tensors are only made, copied and moved here; they are compared as numpy arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, amd
from test_hip_video import COMBOS, DTYPES, _origins, _randomize, _static, _tail, _video_frames
from test_hip_video_reuse import GEOMETRIES, WILD, _plan_origins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xABCD                 # above 1023: no kernel stores it


def _np(t):
    return t.cpu().numpy()


def _gpu16(planes, pad=0):
    return [_tail(torch.from_numpy(np.ascontiguousarray(p)), pad) for p in planes]


def _wild_planes(H, W, seed):
    """one word in five is random over the whole 16-bit range (read as 1023 where it is above), the rest hold 10 bits"""
    rng = np.random.RandomState(seed)
    out = []
    for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2)):
        p = rng.randint(0, 65536, s)
        out.append(np.where(rng.rand(*s) < 0.8, p & 1023, p).astype(np.uint16))
    return out


def _frames10(n, H, W, seed):
    """smooth in-gamut content plus noise as 10-bit planes (bt601, limited range)"""
    video = amd("video")
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        base = torch.rand(3, H // 8 + 2, W // 8 + 2, generator=g)
        smooth = torch.nn.functional.interpolate(base[None], size=(H, W), mode="bilinear", align_corners=False)[0]
        img = (smooth * 800 + torch.rand(3, H, W, generator=g) * 223).clamp(0, 1023).to(torch.int32)
        out.append(list(video.rgb_to_yuv420_host(img.permute(1, 2, 0).contiguous().numpy().astype(np.uint16), depth=10)))
    return out


def _gather_ref(planes, origins, h, w, dtype, matrix, full):
    """the host decode at frame coordinates, / 1023 in fp32, one cast"""
    H, W = planes[0].shape
    rgb = amd("video").yuv420_to_rgb_host(*planes, matrix, full, depth=10).astype(np.float32) / np.float32(1023.0)
    out = []
    for y0, x0 in origins:
        y0, x0 = min(max(y0, 0), H - h), min(max(x0, 0), W - w)
        out.append(torch.from_numpy(np.ascontiguousarray(rgb[y0:y0 + h, x0:x0 + w].transpose(2, 0, 1))))
    return torch.stack(out).to(dtype)


def _quant_host(src, maxv):
    """round_half_even(clamp(v, 0, 1) * maxv) in fp32: [.., 3, h, w] float tensor -> [.., h, w, 3] integer array"""
    v = np.clip(src.float().cpu().numpy(), np.float32(0), np.float32(1)) * np.float32(maxv)
    assert v.dtype == np.float32
    return np.moveaxis(np.rint(v), -3, -1).astype(np.uint16 if maxv > 255 else np.uint8)


# ---------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("h,w", [(13, 22), (16, 24), (38, 54)])
def test_gather16_matches_host_definition(dtype, h, w):
    up = amd("upscale")
    H, W = 38, 54
    origins = _origins(H, W, h, w, h * 100 + w)
    table = torch.tensor(origins, dtype=torch.int64, device=DEV)
    for pad, (matrix, full) in zip([0, 1, 3, 1], COMBOS):
        planes = _wild_planes(H, W, pad + h)
        assert (planes[0] > 1023).any() and (planes[1] > 1023).any()
        y, u, v = _gpu16(planes, pad)
        got = _tail(torch.zeros(len(origins), 3, h, w, dtype=dtype), pad)
        up.tile_gather_yuv420(y, u, v, table, h, w, dtype, matrix, full, out=got)
        assert torch.equal(got.cpu(), _gather_ref(planes, origins, h, w, dtype, matrix, full)), (pad, matrix, full)
        assert float(got.float().max()) <= 1.0


@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("H,W", [(2, 2), (4, 6)])
def test_gather16_of_tiny_frames(H, W, pad):
    up = amd("upscale")
    planes = _wild_planes(H, W, H + pad)
    y, u, v = _gpu16(planes, pad)
    for h, w in ((H, W), (1, 1), (H - 1, W - 1)):
        origins = [(a, b) for a in range(H - h + 1) for b in range(W - w + 1)]
        table = torch.tensor(origins, dtype=torch.int64, device=DEV)
        for dtype in DTYPES:
            got = up.tile_gather_yuv420(y, u, v, table, h, w, dtype, "bt709", False)
            assert torch.equal(got.cpu(), _gather_ref(planes, origins, h, w, dtype, "bt709", False)), (h, w, dtype)


def test_gather16_clamps_wild_origins():
    up = amd("upscale")
    H, W, h, w = 38, 54, 13, 22
    planes = _wild_planes(H, W, 9)
    y, u, v = _gpu16(planes, 1)
    wild = [(-5, 1000), (10 ** 12, -3), (-2 ** 62, 2 ** 62), (7, W - w + 1)]
    got = up.tile_gather_yuv420(y, u, v, torch.tensor(wild, dtype=torch.int64, device=DEV), h, w, torch.float32)
    assert torch.equal(got.cpu(), _gather_ref(planes, wild, h, w, torch.float32, "bt601", False))


# ---------------------------------------------------------------------------------------------- scatter
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("OH,OW", [(64, 96), (60, 88)])
def test_scatter16_matches_host_definition(dtype, pad, OH, OW):
    up, video = amd("upscale"), amd("video")
    g = torch.Generator().manual_seed(OH + OW + pad)
    plan = up.plan_windows(OH, OW, 16, 4, 2, 1, 64)
    n = len(plan)
    sh, sw = plan.win_h, plan.win_w
    vals = torch.rand(n, 3, sh, sw, generator=g) * 1.4 - 0.2                      # below 0 and above 1 as well
    vals[0, 0, 0, :8] = torch.tensor([0.5, 1.5, 2.5, 3.5, 1022.5, 511.5, 0.0, 1023.0]) / 1023
    src = _tail(vals.to(dtype), pad)
    assert float(src.float().min()) < 0 and float(src.float().max()) > 1
    rows = [(cy - wy, cx - wx, cy, cx, ch, cw) for (wy, wx, cy, cx, ch, cw) in plan.windows]
    assert all(t % 2 == 0 for r in rows for t in r[2:])
    skipped = {1, n - 1}                      # two cores stay unwritten: the planes there must keep the sentinel
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    table[list(skipped), 4:] = 0
    matrix, full = COMBOS[pad % 4]
    y, u, v = _gpu16([np.full(s, SENTINEL, np.uint16) for s in ((OH, OW), (OH // 2, OW // 2), (OH // 2, OW // 2))], pad)
    up.tile_scatter_yuv420(src, table, y, u, v, max(r[4] for r in rows), max(r[5] for r in rows), matrix, full)
    q = _quant_host(src, 1023)
    rgb = np.zeros((OH, OW, 3), np.uint16)
    for i, (sy, sx, dy, dx, eh, ew) in enumerate(rows):
        rgb[dy:dy + eh, dx:dx + ew] = q[i, sy:sy + eh, sx:sx + ew]
    ref = video.rgb_to_yuv420_host(rgb, matrix, full, depth=10)
    exp = [np.full(p.shape, SENTINEL, np.uint16) for p in ref]
    for i, (_, _, dy, dx, eh, ew) in enumerate(rows):
        if i in skipped:
            continue
        exp[0][dy:dy + eh, dx:dx + ew] = ref[0][dy:dy + eh, dx:dx + ew]
        for k in (1, 2):
            exp[k][dy // 2:(dy + eh) // 2, dx // 2:(dx + ew) // 2] = ref[k][dy // 2:(dy + eh) // 2, dx // 2:(dx + ew) // 2]
    for got, e in zip((y, u, v), exp):
        got = _np(got)
        assert np.array_equal(got, e)
        assert ((got <= 1023) | (got == SENTINEL)).all() and (got == SENTINEL).any() and (got <= 1023).any()


def test_scatter16_makes_odd_table_entries_even():
    up, video = amd("upscale"), amd("video")
    base = [np.full(s, SENTINEL, np.uint16) for s in ((12, 16), (6, 8), (6, 8))]
    y, u, v = _gpu16(base, 1)
    src = torch.rand(1, 3, 10, 12, generator=torch.Generator().manual_seed(1)).to(DEV)
    # dy 3 -> 2, dx 5 -> 4, eh 7 -> 6, ew 9 -> 8; the source offsets stay as they are
    up.tile_scatter_yuv420(src, torch.tensor([[1, 2, 3, 5, 7, 9]], dtype=torch.int64, device=DEV), y, u, v, 7, 9)
    ey, eu, ev = video.rgb_to_yuv420_host(np.ascontiguousarray(_quant_host(src[0, :, 1:7, 2:10], 1023)), depth=10)
    exp = [p.copy() for p in base]
    exp[0][2:8, 4:12], exp[1][1:4, 2:6], exp[2][1:4, 2:6] = ey, eu, ev
    for got, e in zip((y, u, v), exp):
        assert np.array_equal(_np(got), e)


def test_p16_entry_points_refuse_bad_calls():
    up, ops, C = amd("upscale"), amd("ops"), amd("_C")
    y, u, v = _gpu16([np.zeros(s, np.uint16) for s in ((6, 8), (3, 4), (3, 4))])
    y8 = torch.zeros(6, 8, dtype=torch.uint8, device=DEV)
    origins = torch.zeros(1, 2, dtype=torch.int64, device=DEV)
    src = torch.zeros(1, 3, 4, 4, device=DEV)
    table = torch.zeros(1, 6, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        up.tile_gather_yuv420(y8, u, v, origins, 4, 4, torch.float32)            # mixed dtypes
    with pytest.raises(ValueError):
        up.tile_scatter_yuv420(src, table, y, u, y8[:3, :4].contiguous(), 4, 4)
    with pytest.raises(ValueError):
        ops.yuv420_to_rgb_u8(y, u, v)                                            # the whole-frame kernels stay 8-bit
    with pytest.raises(C.OfasrError):
        up.tile_gather_yuv420(y, u, v, origins, 7, 4, torch.float32)             # window taller than the frame
    L = C.lib()
    py, pu, pv, po, ps, pt = (t.data_ptr() for t in (y, u, v, origins, src, table))
    dec, enc = ops.yuv_table("bt601", False, False, 10), ops.yuv_table("bt601", False, True, 10)
    for depth in (8, 12, 16):
        assert L.ofasr_tile_gather_yuv420p16(py, pu, pv, 6, 8, depth, dec, po, 1, 4, 4, ps, C.F32, None) == -1
        assert L.ofasr_tile_scatter_yuv420p16(ps, 1, 4, 4, C.F32, pt, depth, enc, py, pu, pv, 6, 8, 4, 4, None) == -1
        assert L.ofasr_window_diff_yuv420p16(py, pu, pv, py, pu, pv, 6, 8, depth, po, 1, 4, 4, ps, None) == -1
    assert b"depth" in L.ofasr_last_error_string()
    assert L.ofasr_tile_gather_yuv420p16(py, pu + 1, pv, 6, 8, 10, dec, po, 1, 4, 4, ps, C.F32, None) == -1
    assert b"aligned" in L.ofasr_last_error_string()
    assert L.ofasr_tile_scatter_yuv420p16(ps, 1, 4, 4, C.F32, pt, 10, enc, py, pu, pv + 1, 6, 8, 4, 4, None) == -1
    assert L.ofasr_window_diff_yuv420p16(py, pu, pv, py + 1, pu, pv, 6, 8, 10, po, 1, 4, 4, ps, None) == -1
    assert L.ofasr_tile_gather_yuv420p16(py, pu, None, 6, 8, 10, dec, po, 1, 4, 4, ps, C.F32, None) == -1       # null pointer
    assert L.ofasr_tile_gather_yuv420p16(py, pu, pv, 5, 8, 10, dec, po, 1, 4, 4, ps, C.F32, None) == -1         # odd side
    assert L.ofasr_tile_gather_yuv420p16(py, pu, pv, 6, 8, 10, dec, po, 65536, 4, 4, ps, C.F32, None) == -2
    assert L.ofasr_tile_scatter_yuv420p16(ps, 1, 4, 4, C.F32, pt, 10, enc, py, pu, pv, 6, 8, 5, 4, None) == -1  # extent bound
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- diff kernel
def _frame16(Hh, Ww, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 65536, s).astype(np.uint16) for s in ((Hh, Ww), (Hh // 2, Ww // 2), (Hh // 2, Ww // 2))]


def _changed(up, cur, prev, table, h, w):
    flags = up.window_diff_yuv420(*cur, *prev, table, h, w)
    assert flags.dtype == torch.int32 and tuple(flags.shape) == (table.size(0), up.window_diff_slabs(h, w))
    assert bool(((flags == 0) | (flags == 1)).all())
    return flags.ne(0).any(dim=1).cpu().numpy()


def _set(plane, r, c, value):
    plane[r:r + 1, c:c + 1].copy_(torch.from_numpy(np.array([[value]], np.uint16)))


def _support_probes(video, Hh, Ww, h, w, origins):
    """(plane, row, col): for a few windows and every plane, the four corner samples of the support rectangle and the
    sample one outside each of its edges (where the plane has one), each once"""
    out = []
    for (y0, x0) in [origins[0], origins[len(origins) // 2], origins[-1]]:
        luma, chroma = video.window_support(y0, x0, h, w, Hh, Ww, depth=10)
        for p, (r0, r1, c0, c1) in ((0, luma), (1, chroma), (2, chroma)):
            R, C = (Hh, Ww) if p == 0 else (Hh // 2, Ww // 2)
            pts = [(r0, c0), (r0, c1), (r1, c0), (r1, c1), (r0 - 1, c0), (r1 + 1, c1), (r0, c0 - 1), (r1, c1 + 1)]
            out += [(p, r, c) for r, c in pts if 0 <= r < R and 0 <= c < C]
    return sorted(set(out))


@pytest.mark.parametrize("pads", [(0, 0), (1, 1), (3, 3), (1, 0), (0, 3), (3, 1)], ids=str)
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_diff16_matches_host_definition(geometry, pads):
    up, video = amd("upscale"), amd("video")
    Hh, Ww, h, w, origins = GEOMETRIES[geometry]
    plan = _plan_origins() if origins is None else origins
    origins = plan + WILD
    table = torch.tensor(origins, dtype=torch.int64, device=DEV)
    base = _frame16(Hh, Ww, len(geometry))
    cur, prev = _gpu16(base, pads[0]), _gpu16(base, pads[1])
    assert not _changed(up, cur, prev, table, h, w).any()                            # identical frames
    assert _changed(up, cur, _gpu16([p ^ 0xFFFF for p in base], pads[1]), table, h, w).all()
    probes = _support_probes(video, Hh, Ww, h, w, plan)
    assert len(probes) >= 12
    seen = set()
    for i, (p, r, c) in enumerate(probes):
        bit = 1 << ((3 * i + r + c) % 16)                                            # the low byte alone or the high byte alone
        host = [q.copy() for q in base]
        host[p][r, c] ^= bit
        _set(prev[p], r, c, int(host[p][r, c]))
        exp = video.changed_windows_host(host, base, origins, h, w, depth=10)
        got = _changed(up, cur, prev, table, h, w)
        _set(prev[p], r, c, int(base[p][r, c]))
        assert np.array_equal(got, exp), (p, r, c, bit, got.tolist(), exp.tolist())
        seen.add(bit >= 256)
    assert seen == {False, True}
    assert not _changed(up, cur, prev, table, h, w).any()


def test_diff16_is_deterministic_and_refuses_bad_calls():
    up, C = amd("upscale"), amd("_C")
    H, W, WIN_H, WIN_W = 72, 104, 49, 56
    cur, prev = _gpu16(_frame16(H, W, 5), 1), _gpu16(_frame16(H, W, 6), 3)
    table = torch.tensor(_plan_origins(), dtype=torch.int64, device=DEV)
    a = up.window_diff_yuv420(*cur, *prev, table, WIN_H, WIN_W)
    b = up.window_diff_yuv420(*cur, *prev, table, WIN_H, WIN_W)
    assert torch.equal(a, b) and bool(a.all())
    with pytest.raises(C.OfasrError):
        up.window_diff_yuv420(*cur, *prev, table, H + 1, WIN_W)                      # window taller than the frame
    with pytest.raises(ValueError):
        up.window_diff_yuv420(*cur, *_gpu16(_frame16(H, W + 2, 6)), table, WIN_H, WIN_W)
    prev8 = [torch.zeros(p.shape, dtype=torch.uint8, device=DEV) for p in prev]
    with pytest.raises(ValueError):
        up.window_diff_yuv420(*cur, *prev8, table, WIN_H, WIN_W)                     # mixed dtypes
    with pytest.raises(ValueError):
        up.window_diff_yuv420(cur[0], cur[1], prev8[2], *prev, table, WIN_H, WIN_W)
    L = C.lib()
    p = cur[0].data_ptr()
    assert L.ofasr_window_diff_yuv420p16(p, p, p, p, p, p, H - 1, W, 10, p, 1, 4, 4, p, None) == -1      # odd side
    assert L.ofasr_window_diff_yuv420p16(p, p, p, p, p, None, H, W, 10, p, 1, 4, 4, p, None) == -1       # null pointer
    assert L.ofasr_window_diff_yuv420p16(p, p, p, p, p, p, H, W, 10, p, 65536, 4, 4, p, None) == -2


# ---------------------------------------------------------------------------------------------- network
@pytest.fixture(scope="module")
def small_net():
    return _randomize(_static(dict(ks=3, e=3, d=2, pixel_d=1)), 4)


def _reference(tu, planes, in_depth, out_depth):
    """the plan's windows built by the host decode, through the upscaler's own forward, the cores encoded by the host
    definition: no kernel of this change takes part"""
    video = amd("video")
    H, W = planes[0].shape
    s = tu.scale
    maxv = 255 if in_depth == 8 else 1023
    rgb = video.yuv420_to_rgb_host(*planes, depth=in_depth).astype(np.float32) / np.float32(maxv)
    chw = torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1)))
    out = torch.zeros(3, H * s, W * s)

    def gather(origins, h, w):
        return torch.stack([chw[:, y0:y0 + h, x0:x0 + w] for y0, x0 in origins.tolist()]).to(tu.dtype).to(DEV)

    def sink(t, real, table, wins, plan):
        for i, (wy, wx, cy, cx, ch, cw) in enumerate(wins):
            out[:, cy * s:(cy + ch) * s, cx * s:(cx + cw) * s] = \
                t[i, :, (cy - wy) * s:(cy - wy + ch) * s, (cx - wx) * s:(cx - wx + cw) * s].float().cpu()

    tu._run_windows(H, W, torch.device(DEV), False, sink, gather)
    q = _quant_host(out, 255 if out_depth == 8 else 1023)
    return video.rgb_to_yuv420_host(np.ascontiguousarray(q), depth=out_depth)


@pytest.mark.parametrize("depths", [(10, 10), (8, 10), (10, 8)], ids=lambda d: "%dto%d" % d)
@pytest.mark.parametrize("mix_prec,k", [("f32", 1), ("f16", 2)])
@pytest.mark.parametrize("H,W", [(40, 56), (72, 104)])
def test_upscale_yuv420_at_depth_10(small_net, H, W, mix_prec, k, depths):
    up = amd("upscale")
    din, dout = depths
    tu = up.TiledUpscaler(small_net, core=16, mix_prec=mix_prec, self_ensemble=k)
    assert len(tu.plan(H, W)) >= 4
    planes = _video_frames(1, H, W, 7)[0] if din == 8 else _frames10(1, H, W, 7)[0]
    got = tu.upscale_yuv420(*planes, out_depth=dout)
    dt = torch.uint8 if dout == 8 else torch.uint16
    assert got[0].shape == (H * 4, W * 4) and got[1].shape == got[2].shape == (H * 2, W * 2)
    assert all(p.dtype == dt for p in got)
    got = [_np(p) for p in got]
    for a, b in zip(got, _reference(tu, planes, din, dout)):
        assert np.array_equal(a, b)
    for a, b in zip(got, tu.upscale_yuv420(*_gpu16(planes, 1), out_depth=dout)):    # planes on the GPU, unaligned
        assert np.array_equal(a, _np(b))
    assert int(got[0].max()) <= (255 if dout == 8 else 1023)
    assert int(got[0].max()) - int(got[0].min()) > (30 if dout == 8 else 120)        # a picture, not a constant
    if din == dout:                                                                  # the default is the input's depth
        for a, b in zip(got, tu.upscale_yuv420(*planes)):
            assert np.array_equal(a, _np(b))


@pytest.mark.parametrize("depths", [(10, 10), (8, 10), (10, 8)], ids=lambda d: "%dto%d" % d)
@pytest.mark.parametrize("mix_prec,k", [("f32", 1), ("f16", 2)])
@pytest.mark.parametrize("H,W", [(40, 56), (72, 104)])
def test_tiled_equals_whole_at_depth_10(small_net, H, W, mix_prec, k, depths):
    """the tiled result against one forward of the whole frame, bit for bit on all three planes.  In f16 this holds
    because the upscaler's forwards keep the fused MB kernel from splitting a small launch's mid-channel chunks
    (TiledUpscaler._forward): with the split on, the 49x56 windows and the 72x104 frame summed in different orders and
    about one sample in ten differed by one step."""
    up = amd("upscale")
    din, dout = depths
    tu = up.TiledUpscaler(small_net, core=16, mix_prec=mix_prec, self_ensemble=k)
    planes = _video_frames(1, H, W, 7)[0] if din == 8 else _frames10(1, H, W, 7)[0]
    tiled = [_np(p) for p in tu.upscale_yuv420(*planes, out_depth=dout)]
    whole = [_np(p) for p in tu.upscale_yuv420(*planes, whole=True, out_depth=dout)]
    diff = [int((a != b).sum()) for a, b in zip(tiled, whole)]
    step = [int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max()) for a, b in zip(tiled, whole)]
    print("tiled vs whole: differing samples (y, u, v) %s of %s, largest step %s" % (diff, [a.size for a in tiled], step))
    assert diff == [0, 0, 0]


def test_10_bit_output_of_a_smooth_8_bit_frame_uses_the_extra_bits(small_net):
    up, video = amd("upscale"), amd("video")
    H, W = 40, 56
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.stack([40 + 170 * xx / (W - 1), 40 + 170 * yy / (H - 1), 40 + 170 * (xx + yy) / (H + W - 2)], axis=2)
    planes = video.rgb_to_yuv420_host(np.rint(rgb).astype(np.uint8))
    tu = up.TiledUpscaler(small_net, core=16)
    y10 = _np(tu.upscale_yuv420(*planes, out_depth=10)[0])
    y8 = _np(tu.upscale_yuv420(*planes)[0])
    levels = len(np.unique(y10))
    print("distinct luma values: %d at depth 10, %d at depth 8" % (levels, len(np.unique(y8))))
    assert levels > 256
    assert tu.upscale_yuv420(*planes, out_depth=8)[0].dtype == torch.uint8
    for bad in (12, True, "10"):
        with pytest.raises(ValueError, match="out_depth"):
            tu.upscale_yuv420(*planes, out_depth=bad)


# ---------------------------------------------------------------------------------------------- stream
def _sequence10():
    H, W = 72, 104
    f0 = [p.copy() for p in _frames10(1, H, W, 21)[0]]
    f1 = [p.copy() for p in f0]
    f2 = [p.copy() for p in f1]
    f2[0][0:4, 0:4] ^= 0x155
    f3 = [p.copy() for p in f2]
    f3[1][31, 20] ^= 0x100                                 # the high byte alone
    f4 = [p.copy() for p in _frames10(1, H, W, 22)[0]]
    return [f0, f1, f2, f3, f4]


@pytest.mark.parametrize("mix_prec,k", [("f32", 1), ("f16", 2)])
def test_stream_on_10_bit_frames_equals_per_frame_upscale(small_net, mix_prec, k):
    up, video = amd("upscale"), amd("video")
    tu = up.TiledUpscaler(small_net, core=16, batch=8, mix_prec=mix_prec, self_ensemble=k)
    origins = _plan_origins()
    frames = _sequence10()
    r3 = video.changed_windows_host(frames[2], frames[3], origins, 49, 56, depth=10)
    assert 0 < int(r3.sum()) < 35
    stream = tu.yuv420_stream()
    run, changed = [], []
    captures = None
    for i, fr in enumerate(frames):
        got = [_np(p) for p in stream.upscale(*fr)]
        if i == 0:
            captures = tu.graphed.captures
        run.append(stream.stats.run)
        changed.append(stream.changed_windows())
        ref = tu.upscale_yuv420(*fr)
        for a, b in zip(got, ref):
            assert a.dtype == np.uint16 and np.array_equal(a, _np(b)), i
    assert run == [35, 0, 4, int(r3.sum()), 35]
    assert changed[1] == [] and changed[2] == [0, 1, 7, 8] and changed[3] == np.flatnonzero(r3).tolist()
    assert changed[2] == np.flatnonzero(video.changed_windows_host(frames[1], frames[2], origins, 49, 56, depth=10)).tolist()
    assert changed[0] == changed[4] == list(range(35))
    assert tu.graphed.captures == captures                                           # graph captures are not repeated


def test_stream_restarts_on_a_change_of_dtype_and_takes_out_depth(small_net):
    up = amd("upscale")
    tu = up.TiledUpscaler(small_net, core=16, batch=8)
    H, W = 40, 56
    n = len(tu.plan(H, W))
    f8 = _video_frames(1, H, W, 31)[0]
    f10 = _frames10(1, H, W, 31)[0]
    stream = tu.yuv420_stream()
    for fr, exp_run, dt in ((f8, n, np.uint8), (f8, 0, np.uint8), (f10, n, np.uint16), (f10, 0, np.uint16), (f8, n, np.uint8)):
        got = [_np(p) for p in stream.upscale(*fr)]
        assert stream.stats.run == exp_run and got[0].dtype == dt
        for a, b in zip(got, tu.upscale_yuv420(*fr)):
            assert np.array_equal(a, _np(b))
    # 8 -> 10 and 10 -> 8 in a stream: the output planes take the output depth, the previous-frame planes the input's
    for fr, dout, dt in ((f8, 10, np.uint16), (f10, 8, np.uint8)):
        stream = tu.yuv420_stream(out_depth=dout)
        for exp_run in (n, 0):
            got = [_np(p) for p in stream.upscale(*fr)]
            assert stream.stats.run == exp_run and got[0].dtype == dt
            for a, b in zip(got, tu.upscale_yuv420(*fr, out_depth=dout)):
                assert np.array_equal(a, _np(b))
    with pytest.raises(ValueError, match="out_depth"):
        tu.yuv420_stream(out_depth=12)


# ---------------------------------------------------------------------------------------------- command line
def _export(net, tmp_path):
    d = tmp_path / "net"
    d.mkdir()
    (d / "net_config.json").write_text(json.dumps(net.config))
    torch.save({"state_dict": {k: t.cpu() for k, t in net.state_dict().items()}}, str(d / "static_state_dict.pth"))
    return str(d)


def _cli(static, *args):
    cmd = [sys.executable, os.path.join(ROOT, "upscale_video_ofa_net_sr.py"), "--static", static, "--core", "16"]
    return subprocess.run(cmd + list(args), capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_cli_10_bit_in_and_out(small_net, tmp_path):
    up, video = amd("upscale"), amd("video")
    static = _export(small_net, tmp_path)
    H, W = 40, 56
    f0 = _frames10(1, H, W, 41)[0]
    f1 = [p.copy() for p in f0]
    f1[0][30:34, 0:6] ^= 0x133
    src = str(tmp_path / "in.y4m")
    with video.Y4MWriter(src, W, H, fps="25:1", chroma="420p10", depth=10) as w:
        for fr in (f0, f1):
            w.write_frame(*fr)
    tu = up.TiledUpscaler(small_net, core=16)
    expect = b"".join(b"FRAME\n" + b"".join(_np(p).astype("<u2").tobytes() for p in tu.upscale_yuv420(*fr)) for fr in (f0, f1))
    plain, reuse = str(tmp_path / "plain.y4m"), str(tmp_path / "reuse.y4m")
    r = _cli(static, "--out", plain, src)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "10 -> 10 bits" in r.stdout
    raw = open(plain, "rb").read()
    assert raw.startswith(b"YUV4MPEG2 W224 H160 F25:1 C420p10\n")
    assert raw[raw.index(b"\n") + 1:] == expect
    r = _cli(static, "--out", reuse, "--reuse-static", "--reference", plain, src)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(reuse, "rb").read() == raw
    line = [t for t in r.stdout.splitlines() if t.startswith("windows run")]
    n = len(tu.plan(H, W))
    assert len(line) == 1 and n < int(line[0].split()[2]) < 2 * n                    # a full frame and a part of one
    q = json.load(open(reuse + ".quality.json"))
    assert all(rec["psnr_" + k] == float("inf") and rec["sse_" + k] == 0 for rec in q["frames"] for k in "yuv")
    # --dump-png has no 16-bit writer: the argument parser refuses it, before any work
    for extra in (("--out-depth", "10"), ("--depth", "10", "--size", "56x40")):
        r = _cli(static, "--out", str(tmp_path / "no.y4m"), "--dump-png", str(tmp_path / "png"), *extra, src)
        assert r.returncode == 2 and "--dump-png needs an 8-bit output" in r.stderr and "usage:" in r.stderr
    assert not os.path.exists(str(tmp_path / "no.y4m")) and not os.path.exists(str(tmp_path / "png"))


def test_cli_8_bit_in_10_bit_out(small_net, tmp_path):
    up, video = amd("upscale"), amd("video")
    static = _export(small_net, tmp_path)
    H, W = 40, 56
    frames = _video_frames(2, H, W, 43)
    src = str(tmp_path / "in.y4m")
    with video.Y4MWriter(src, W, H, fps="25:1", chroma="420mpeg2") as w:
        for fr in frames:
            w.write_frame(*fr)
    tu = up.TiledUpscaler(small_net, core=16)
    out = str(tmp_path / "out.y4m")
    r = _cli(static, "--out", out, "--out-depth", "10", src)
    assert r.returncode == 0, r.stdout + r.stderr
    with video.open_reader(out) as rd:
        assert (rd.width, rd.height, rd.depth, rd.chroma, rd.fps) == (W * 4, H * 4, 10, "420p10", "25:1")
        got = [tuple(p.copy() for p in fr) for fr in rd]
    assert len(got) == 2
    for a, fr in zip(got, frames):
        for x, y in zip(a, tu.upscale_yuv420(*fr, out_depth=10)):
            assert x.dtype == np.uint16 and np.array_equal(x, _np(y))
    # a Y4M says its depth itself: --depth may not contradict it
    r = _cli(static, "--out", str(tmp_path / "no.y4m"), "--depth", "10", src)
    assert r.returncode != 0 and "C420mpeg2" in r.stderr
