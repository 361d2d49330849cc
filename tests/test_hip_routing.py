"""Content-aware routing on the MI355X (`-m gpu`): the activity kernels (csrc/route.hip) against the host definition
(routing.window_activity_host), the routing kernel against list comprehensions, the routed TiledUpscaler against the
composition of its all-easy and all-hard outputs (images, YUV frames at both depths, self-ensemble, target size), the
routed YUV420Stream against per-frame upscale_yuv420, and the command line.  Everything is bit-exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, amd
from test_hip_video import _randomize, _static, _tail, _video_frames
from test_hip_video_reuse import GEOMETRIES, WILD, _plan_origins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, WIN_H, WIN_W = 72, 104, 49, 56
HARD = dict(ks=3, e=3, d=2, pixel_d=1)                  # the small_net of the reuse tests: receptive radius 17
EASY = dict(ks=3, e=3, d=2, pixel_d=0)                  # no block behind the last PixelShuffle: cheaper, radius 16
INF = float("inf")


@pytest.fixture(scope="module")
def nets():
    hard, easy = _randomize(_static(HARD), 4), _randomize(_static(EASY), 5)
    up = amd("upscale")
    assert (up.receptive_radius(hard.config), up.receptive_radius(easy.config)) == (17, 16)
    assert hard.config["upscale"] == easy.config["upscale"] == 4
    return hard, easy


# ---------------------------------------------------------------------------------------------- activity kernels
def _source(kind, Hh, Ww, seed, board=False):
    rng = np.random.RandomState(seed)
    if board:
        cells = (np.add.outer(np.arange(Hh), np.arange(Ww)) & 1)
        if kind == "rgb":
            return np.repeat((cells * 255).astype(np.uint8)[:, :, None], 3, axis=2)
        return (cells * (255 if kind == "u8" else 1023)).astype(np.uint8 if kind == "u8" else np.uint16)
    if kind == "rgb":
        return rng.randint(0, 256, (Hh, Ww, 3)).astype(np.uint8)
    if kind == "u8":
        return rng.randint(0, 256, (Hh, Ww)).astype(np.uint8)
    return rng.randint(0, 1024, (Hh, Ww)).astype(np.uint16)


def _activity(up, src, pad, table, h, w):
    partial = up.window_activity(_tail(torch.from_numpy(src), pad), table, h, w)
    assert partial.dtype == torch.int64 and tuple(partial.shape) == (table.size(0), up.window_activity_slabs(h, w))
    return partial


@pytest.mark.parametrize("kind", ["rgb", "u8", "u16"])
@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_activity_kernel_matches_host_definition(geometry, pad, kind):
    up, routing = amd("upscale"), amd("routing")
    Hh, Ww, h, w, origins = GEOMETRIES[geometry]
    origins = (_plan_origins() if origins is None else origins) + WILD
    if geometry == "slabs":
        assert up.window_activity_slabs(h, w) > 1
    table = torch.tensor(origins, dtype=torch.int64, device=DEV)
    src = _source(kind, Hh, Ww, len(geometry) * 8 + pad)
    a = _activity(up, src, pad, table, h, w)
    exp = routing.window_activity_host(src, origins, h, w)
    assert a.sum(dim=1).cpu().numpy().tolist() == exp.tolist()
    assert bool((a >= 0).all())
    if geometry == "one":
        assert not exp.any()                             # D = 0
    else:
        assert exp.min() > 0
    b = _activity(up, src, pad, table, h, w)             # two runs: identical partials
    assert torch.equal(a, b)
    flat = np.full_like(src, 77)
    assert not bool(_activity(up, flat, pad, table, h, w).any())


@pytest.mark.parametrize("kind", ["rgb", "u8", "u16"])
def test_activity_kernel_on_the_largest_sum(kind):
    """an all-255 / 0 (all-1023 / 0) checkerboard: every difference is the peak"""
    up, routing = amd("upscale"), amd("routing")
    Hh, Ww, h, w, origins = GEOMETRIES["slabs"]
    table = torch.tensor(origins + WILD, dtype=torch.int64, device=DEV)
    src = _source(kind, Hh, Ww, 0, board=True)
    got = _activity(up, src, 1, table, h, w).sum(dim=1).cpu().numpy()
    peak = 1023 if kind == "u16" else 255
    assert got.tolist() == [peak * routing.activity_terms(h, w)] * len(got)
    assert got.tolist() == routing.window_activity_host(src, origins + WILD, h, w).tolist()


def test_activity_kernel_refuses_bad_calls():
    up, C = amd("upscale"), amd("_C")
    rgb = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    y8 = torch.zeros(H, W, dtype=torch.uint8, device=DEV)
    y16 = torch.empty(H, W, dtype=torch.uint16, device=DEV)
    table = torch.tensor(_plan_origins(), dtype=torch.int64, device=DEV)
    with pytest.raises(C.OfasrError):
        up.window_activity(rgb, table, H + 1, WIN_W)                             # window taller than the frame
    with pytest.raises(C.OfasrError):
        up.window_activity(y8.cpu(), table, WIN_H, WIN_W)
    with pytest.raises(ValueError):
        up.window_activity(y8.float(), table, WIN_H, WIN_W)
    with pytest.raises(ValueError):
        up.window_activity(y8, table.to(torch.int32), WIN_H, WIN_W)
    with pytest.raises(ValueError):
        up.window_activity(rgb[:, :, :2], table, WIN_H, WIN_W)
    with pytest.raises(ValueError):
        up.window_activity(y8, table, WIN_H, WIN_W, torch.zeros(3, dtype=torch.int64, device=DEV))
    L = C.lib()
    C.reset_launch_counts()
    p, q = y16.data_ptr(), table.data_ptr()
    assert L.ofasr_window_activity_rgb8(None, H, W, q, 1, 4, 4, p, None) == -1                   # null pointers
    assert L.ofasr_window_activity_rgb8(p, H, W, q, 1, 4, 4, None, None) == -1
    assert L.ofasr_window_activity_plane(p, H, W, 8, None, 1, 4, 4, p, None) == -1
    assert L.ofasr_window_activity_plane(p + 1, H, W, 10, q, 1, 4, 4, p, None) == -1             # odd 16-bit pointer
    assert L.ofasr_window_activity_plane(p, H, W, 8, q, 1, H + 1, 4, p, None) == -1              # window larger than the frame
    assert L.ofasr_window_activity_rgb8(p, H, W, q, 1, 4, W + 1, p, None) == -1
    for depth in (9, 12, 16, 0):
        assert L.ofasr_window_activity_plane(p, H, W, depth, q, 1, 4, 4, p, None) == -1          # depth: 8 or 10 only
    assert L.ofasr_window_activity_plane(p, H, W, 10, q, 0, 4, 4, p, None) == -1
    assert L.ofasr_window_activity_plane(p, H, W, 10, q, 65536, 4, 4, p, None) == -2             # too many windows
    assert L.ofasr_window_route(p, 65, 0, None, 0, q, q, 4, 4, p, p, p, p, None) == -1
    assert L.ofasr_window_route(p, 1, 0, None, 0, q, q, 65536, 4, p, p, p, p, None) == -2
    assert L.ofasr_window_route(p, 1, 0, None, 0, q, q, 4, 0, p, p, p, p, None) == -1
    assert L.ofasr_window_route(p, 1, 0, None, 0, q, q, 4, 4, p, p, p, None, None) == -1
    assert L.ofasr_window_route(p, 1, 0, p, 0, q, q, 4, 4, p, p, p, p, None) == -1               # flags without slabs
    assert L.ofasr_window_activity_slabs(0, 5) == 0 and L.ofasr_window_activity_slabs(WIN_H, WIN_W) == 1
    assert C.launch_table() == {}                                                # nothing was launched


# ---------------------------------------------------------------------------------------------- routing kernel
def _check_route(up, n, S, B, A, limit, changed):
    """A: numpy int64 [n, S] partials; changed: None or numpy int [n, S2]"""
    g = torch.Generator().manual_seed(n + B)
    origins = torch.randint(-50, 5000, (n, 2), generator=g, dtype=torch.int64)
    table = torch.randint(0, 10 ** 6, (n, 6), generator=g, dtype=torch.int64)
    rows = -(-n // B) * B
    out = (torch.full((2, rows, 2), -7, dtype=torch.int64, device=DEV), torch.full((2, n, 6), -7, dtype=torch.int64, device=DEV),
           torch.full((2, n), -7, dtype=torch.int64, device=DEV), torch.full((2,), -7, dtype=torch.int64, device=DEV))
    flags = None if changed is None else torch.from_numpy(changed.astype(np.int32)).to(DEV)
    got = up.window_route(torch.from_numpy(A).to(DEV), limit, origins.to(DEV), table.to(DEV), B, flags, out)
    o, t, idx, count = (x.cpu() for x in got)
    live = [i for i in range(n) if changed is None or changed[i].any()]
    lists = ([i for i in live if int(A[i].sum()) > limit], [i for i in live if int(A[i].sum()) <= limit])
    assert count.tolist() == [len(lists[0]), len(lists[1])]
    for c, keep in enumerate(lists):
        m = len(keep)
        assert idx[c, :m].tolist() == keep                                       # stable, in plan order
        assert torch.equal(t[c, :m], table[keep]) and torch.equal(o[c, :m], origins[keep])
        padded = -(-m // B) * B
        for j in range(m, padded):                                                # the class's last window, repeated
            assert o[c, j].tolist() == origins[keep[-1]].tolist()
        assert bool((o[c, padded:] == -7).all()) and bool((t[c, m:] == -7).all()) and bool((idx[c, m:] == -7).all())
    again = up.window_route(torch.from_numpy(A).to(DEV), limit, origins.to(DEV), table.to(DEV), B, flags)
    assert again[3].tolist() == count.tolist()
    return count.tolist()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("B", [1, 4, 7])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
def test_routing_kernel(n, B, S):
    up = amd("upscale")
    rng = np.random.RandomState(n * 31 + B * 7 + S)
    A = rng.randint(0, 1000, (n, S)).astype(np.int64)
    limit = int(np.median(A.sum(axis=1)))
    some = (rng.rand(n, 2) < 0.3).astype(int)
    assert _check_route(up, n, S, B, A, limit, None)[1] >= 1                      # without flags
    _check_route(up, n, S, B, A, limit, some)                                    # with flags, folded over their own slabs
    assert _check_route(up, n, S, B, A, 2 ** 63 - 1, None) == [0, n]             # all easy
    assert _check_route(up, n, S, B, A, -1, None) == [n, 0]                      # all hard
    assert _check_route(up, n, S, B, A, -1, some)[1] == 0
    assert _check_route(up, n, S, B, A, limit, np.zeros((n, 1), int)) == [0, 0]  # nothing changed
    last = np.zeros((n, 3), int)
    last[n - 1, 2] = 1
    assert sum(_check_route(up, n, S, B, A, limit, last)) == 1
    big = np.full((n, S), 2 ** 40, np.int64)                                      # sums past 32 bits
    assert _check_route(up, n, S, B, big, S * 2 ** 40, None) == [0, n]
    assert _check_route(up, n, S, B, big, S * 2 ** 40 - 1, None) == [n, 0]


# ---------------------------------------------------------------------------------------------- end to end, image
def _image(seed, flat="ramp"):
    """72 x 104 RGB: noise at the lower right, a constant or a gentle ramp elsewhere"""
    rng = np.random.RandomState(seed)
    img = np.empty((H, W, 3), np.uint8)
    if flat == "ramp":
        img[:] = (60 + np.add.outer(np.arange(H), np.arange(W)) // 4).astype(np.uint8)[:, :, None]
    else:
        img[:] = 120
    img[40:, 56:] = rng.randint(0, 256, (H - 40, W - 56, 3))
    return img


def _threshold(routing, src, origins, h, w, depth=8):
    """a decimal between two windows' mean activities, about the middle of the plan, and the host's classes for it"""
    A = np.sort(routing.mean_activity(routing.window_activity_host(src, origins, h, w), h, w, depth))
    k = len(A) // 2
    while k + 1 < len(A) and A[k] == A[k - 1]:
        k += 1
    T = "%.6f" % ((A[k - 1] + A[k]) / 2)
    easy = routing.classify_host(src, origins, h, w, T, depth)
    assert 0 < int(easy.sum()) < len(origins), (T, A.tolist())                    # both classes
    return T, easy


def _core_mask(plan, easy, s, shape, halve=False):
    """bool mask of the output pixels whose core (or target rectangle) belongs to an easy window"""
    mask = torch.zeros(shape, dtype=torch.bool)
    rects = plan.targets if hasattr(plan, "targets") else [(cy * s, cx * s, ch * s, cw * s) for (_, _, cy, cx, ch, cw) in plan.windows]
    seen = torch.zeros(shape, dtype=torch.int32)
    d = 2 if halve else 1
    for e, (dy, dx, eh, ew) in zip(easy, rects):
        mask[dy // d:(dy + eh) // d, dx // d:(dx + ew) // d] = bool(e)
        seen[dy // d:(dy + eh) // d, dx // d:(dx + ew) // d] += 1
    assert bool((seen == 1).all())                                               # the rectangles tile the output once
    return mask.to(DEV)


def _routed_three(tu, T, run):
    """(routed, all easy, all hard, stats of the routed run) of run(tu) at T, inf and -1"""
    tu.set_easy_threshold(INF)
    all_easy = run(tu)
    assert tu.route_stats["hard"] == 0 and tu.route_stats["easy"] == tu.route_stats["windows"]
    tu.set_easy_threshold(-1)
    all_hard = run(tu)
    assert tu.route_stats["easy"] == 0 and tu.route_stats["hard"] == tu.route_stats["windows"]
    tu.set_easy_threshold(T)
    return run(tu), all_easy, all_hard, dict(tu.route_stats)


@pytest.mark.parametrize("case", ["f32", "swapped", "bf16", "ensemble2", "out_size"])
def test_routed_image_is_the_composition(nets, case):
    up, routing = amd("upscale"), amd("routing")
    hard, easy = nets[::-1] if case == "swapped" else nets
    kw = dict(mix_prec="bf16") if case == "bf16" else dict(self_ensemble=2) if case == "ensemble2" else {}
    out_size = (200, 300) if case == "out_size" else None
    assert out_size is None or (H < out_size[0] < 4 * H and W < out_size[1] < 4 * W)
    img = _image(3, "const" if case == "swapped" else "ramp")
    tu = up.TiledUpscaler(hard, core=16, easy_net=easy, easy_threshold=0, **kw)
    assert (tu.radius, tu.halo) == (17, 17)                                      # the larger radius, whichever role has it
    plan = tu.plan(H, W, out_size) if out_size else tu.plan(H, W)
    origins = [(w[0], w[1]) for w in plan.windows]
    if out_size is None:
        assert origins == _plan_origins() and (plan.win_h, plan.win_w) == (WIN_H, WIN_W)
    T, cls = _threshold(routing, img, origins, plan.win_h, plan.win_w)
    routed, all_easy, all_hard, stats = _routed_three(tu, T, lambda t: t.upscale(img, out_size=out_size).clone())
    assert stats == {"windows": len(plan), "easy": int(cls.sum()), "hard": int((~cls).sum())}
    assert routed.shape == ((H * 4, W * 4, 3) if out_size is None else out_size + (3,))
    mask = _core_mask(plan, cls, 4, routed.shape[:2])
    assert torch.equal(routed, torch.where(mask[:, :, None], all_easy, all_hard))
    assert not torch.equal(all_easy, all_hard) and not torch.equal(routed, all_easy) and not torch.equal(routed, all_hard)
    act = tu.window_activity(img, out_size)
    assert act.dtype == torch.float64 and not act.is_cuda
    exp = routing.mean_activity(routing.window_activity_host(img, origins, plan.win_h, plan.win_w), plan.win_h, plan.win_w)
    assert act.numpy().tolist() == exp.tolist()
    if case in ("f32", "swapped"):                                               # tiled = whole: a larger halo changes no core
        assert torch.equal(all_hard, up.TiledUpscaler(hard, core=16).upscale(img))
        assert torch.equal(all_easy, up.TiledUpscaler(easy, core=16).upscale(img))


def test_routed_upscaler_refusals_and_the_plain_path(nets):
    up, C = amd("upscale"), amd("_C")
    hard, easy = nets
    tu = up.TiledUpscaler(hard, core=16, easy_net=easy, easy_threshold="0.5")
    img = _image(4)
    with pytest.raises(ValueError, match="nothing to route"):
        tu.upscale(img, whole=True)
    with pytest.raises(ValueError, match="nothing to route"):
        tu.upscale_yuv420(*_video_frames(1, 40, 56, 1)[0], whole=True)
    with pytest.raises(ValueError, match="without easy_net"):
        tu.upscale_float(img)
    with pytest.raises(ValueError, match="same device"):
        up.TiledUpscaler(hard, core=16, easy_net=_static(EASY), easy_threshold=1)
    with pytest.raises(ValueError):
        tu.set_easy_threshold(float("nan"))
    # without easy_net nothing of route.hip is launched
    plain = up.TiledUpscaler(hard, core=16)
    with pytest.raises(ValueError):
        plain.set_easy_threshold(1)
    plain.upscale(img)
    C.reset_launch_counts()
    plain.upscale(img)
    plain.upscale_yuv420(*_video_frames(1, 40, 56, 1)[0])
    torch.cuda.synchronize()
    assert not any("window_activity" in k or "window_route" in k for k in C.launch_table())
    assert plain.route_stats is None
    # with it: one activity launch and one routing launch per image
    tu.upscale(img)
    C.reset_launch_counts()
    tu.upscale(img)
    torch.cuda.synchronize()
    table = C.launch_table()
    assert sum(v for k, v in table.items() if "window_activity_kernel" in k) == 1
    assert sum(v for k, v in table.items() if "window_route_kernel" in k) == 1


# ---------------------------------------------------------------------------------------------- end to end, YUV
def _flat_frames(n, Hh, Ww, seed, depth=8):
    """_video_frames with the upper left of the luma plane flattened; depth 10: the 8-bit planes times 4 plus two low bits"""
    out = []
    rng = np.random.RandomState(seed)
    for fr in _video_frames(n, Hh, Ww, seed):
        fr = [p.copy() for p in fr]
        fr[0][:Hh * 5 // 9, :Ww * 7 // 13] = 90
        if depth == 10:
            fr = [(p.astype(np.uint16) << 2) | rng.randint(0, 4, p.shape).astype(np.uint16) for p in fr]
            fr[0][:Hh * 5 // 9, :Ww * 7 // 13] = 361
        out.append(fr)
    return out


def _bits(t):
    """a uint16 plane as its int16 bits (torch has few uint16 kernels); equality is the same"""
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


@pytest.mark.parametrize("depth", [8, 10])
def test_routed_yuv420_is_the_composition(nets, depth):
    up, routing, ops = amd("upscale"), amd("routing"), amd("ops")
    hard, easy = nets
    planes = _flat_frames(1, H, W, 7, depth)[0]
    tu = up.TiledUpscaler(hard, core=16, easy_net=easy, easy_threshold=0)
    plan = tu.plan(H, W)
    origins = [(w[0], w[1]) for w in plan.windows]
    T, cls = _threshold(routing, planes[0], origins, WIN_H, WIN_W, depth)
    kw = dict(out_depth=10) if depth == 10 else {}
    routed, all_easy, all_hard, stats = _routed_three(
        tu, T, lambda t: [p.clone() for p in t.upscale_yuv420(*planes, **kw)])
    assert stats == {"windows": 35, "easy": int(cls.sum()), "hard": int((~cls).sum())}
    assert routed[0].dtype == (torch.uint16 if depth == 10 else torch.uint8)
    for k in range(3):
        mask = _core_mask(plan, cls, 4, tuple(routed[k].shape), halve=k > 0)
        assert torch.equal(_bits(routed[k]), torch.where(mask, _bits(all_easy[k]), _bits(all_hard[k])))
    assert not all(torch.equal(_bits(a), _bits(b)) for a, b in zip(all_easy, all_hard))
    act = tu.window_activity(tuple(planes))
    exp = routing.mean_activity(routing.window_activity_host(planes[0], origins, WIN_H, WIN_W), WIN_H, WIN_W, depth)
    assert act.numpy().tolist() == exp.tolist()
    if depth == 8:
        # the statement upscale_yuv420 documents, with the class taken from the Y plane: the encode of the RGB path's
        # output on the decoded frame, composed from the two networks by the same mask
        rgb = ops.yuv420_to_rgb_u8(*[torch.from_numpy(p).to(DEV) for p in planes])
        tu.set_easy_threshold(INF)
        rgb_easy = tu.upscale(rgb).clone()
        tu.set_easy_threshold(-1)
        rgb_hard = tu.upscale(rgb).clone()
        mask = _core_mask(plan, cls, 4, (H * 4, W * 4))
        ref = ops.rgb_to_yuv420_u8(torch.where(mask[:, :, None], rgb_easy, rgb_hard))
        for a, b in zip(routed, ref):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- stream
def _sequence():
    f0 = _flat_frames(1, H, W, 21)[0]
    f1 = [p.copy() for p in f0]                          # repeated exactly
    f2 = [p.copy() for p in f1]
    f2[0][0:4, 0:4] ^= 0x55                              # in the flat region
    f3 = [p.copy() for p in f2]
    f3[0][60:64, 90:96] ^= 0x33                          # in the busy region
    f3[1][31, 20] ^= 0x40
    f4 = _flat_frames(1, H, W, 22)[0]
    return [f0, f1, f2, f3, f4]


def test_routed_stream_equals_per_frame_upscale(nets):
    up, routing, video = amd("upscale"), amd("routing"), amd("video")
    hard, easy = nets
    frames = _sequence()
    origins = _plan_origins()
    T, cls0 = _threshold(routing, frames[0][0], origins, WIN_H, WIN_W)
    tu = up.TiledUpscaler(hard, core=16, batch=8, easy_net=easy, easy_threshold=T)
    fresh = up.TiledUpscaler(hard, core=16, batch=8, easy_net=easy, easy_threshold=T)
    stream = tu.yuv420_stream()
    runs = []
    for i, fr in enumerate(frames):
        before = tu.graphed.replays + tu.graphed_easy.replays
        got = [p.clone() for p in stream.upscale(*fr)]
        replays = tu.graphed.replays + tu.graphed_easy.replays - before
        st = stream.stats
        cls = routing.classify_host(fr[0], origins, WIN_H, WIN_W, T)
        changed = np.ones(35, bool) if i == 0 else video.changed_windows_host(frames[i - 1], fr, origins, WIN_H, WIN_W)
        assert st.run_easy + st.run_hard == st.run == len(stream.changed_windows())
        assert stream.changed_windows() == np.flatnonzero(changed).tolist()
        assert (st.run_easy, st.run_hard) == (int((cls & changed).sum()), int((~cls & changed).sum()))
        assert (st.windows, st.batches) == (35, -(-st.run_easy // 7) + -(-st.run_hard // 7)) and replays == st.batches
        assert tu.route_stats == {"windows": 35, "easy": st.run_easy, "hard": st.run_hard}
        runs.append(st.run)
        for a, b in zip(got, fresh.upscale_yuv420(*fr)):
            assert a.shape == b.shape and torch.equal(a, b), i
    assert runs[0] == runs[4] == 35 and runs[1] == 0 and 0 < runs[2] < 35 and 0 < runs[3] < 35
    st = stream.stats
    assert (st.frames, st.frames_unchanged, st.total_windows, st.total_run) == (5, 1, 175, sum(runs))
    assert st.total_run_easy + st.total_run_hard == st.total_run and st.total_run_easy > 0 and st.total_run_hard > 0
    stream.upscale(*frames[4])
    assert stream.stats.run == 0 and stream.changed_windows() == []
    stream.reset()
    got = stream.upscale(*frames[4])
    assert stream.stats.run == 35 and stream.changed_windows() == list(range(35))
    for a, b in zip(got, fresh.upscale_yuv420(*frames[4])):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- command line
def _export(net, d):
    d.mkdir()
    (d / "net_config.json").write_text(json.dumps(net.config))
    torch.save({"state_dict": {k: t.cpu() for k, t in net.state_dict().items()}}, str(d / "static_state_dict.pth"))
    return str(d)


def test_cli_routes_and_reports(nets, tmp_path):
    up, routing, video = amd("upscale"), amd("routing"), amd("video")
    hard, easy = nets
    dh, de = _export(hard, tmp_path / "hard"), _export(easy, tmp_path / "easy")
    Hh, Ww = 40, 56
    f0, f3 = _flat_frames(2, Hh, Ww, 41)
    f2 = [p.copy() for p in f0]
    f2[0][30:34, 0:6] ^= 0x33
    clip = [f0, f0, f2, f3]
    src = str(tmp_path / "in.y4m")
    with video.Y4MWriter(src, Ww, Hh, fps="25:1") as w:
        for fr in clip:
            w.write_frame(*fr)
    tu = up.TiledUpscaler(hard, core=16, easy_net=easy, easy_threshold=0)
    plan = tu.plan(Hh, Ww)
    origins = [(w[0], w[1]) for w in plan.windows]
    T, _ = _threshold(routing, f0[0], origins, plan.win_h, plan.win_w)
    tu.set_easy_threshold(T)
    script = os.path.join(ROOT, "upscale_video_ofa_net_sr.py")
    out = str(tmp_path / "out.y4m")
    cmd = [sys.executable, script, "--static", dh, "--core", "16", "--out", out]
    r = subprocess.run(cmd + ["--easy-static", de, "--easy-threshold", T, "--reuse-static", "--route-report", src],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    with video.Y4MReader(out) as rd:
        got = [tuple(p.copy() for p in fr) for fr in rd]
    assert len(got) == 4
    for a, fr in zip(got, clip):
        for x, y in zip(a, tu.upscale_yuv420(*fr)):
            assert np.array_equal(x, y.cpu().numpy())
    lines = [t for t in r.stdout.splitlines() if t.startswith("frame ") and " easy " in t]
    assert len(lines) == 4
    n = len(plan)
    for i, (line, fr) in enumerate(zip(lines, clip)):
        cls = routing.classify_host(fr[0], origins, plan.win_h, plan.win_w, T)
        changed = np.ones(n, bool) if i == 0 else video.changed_windows_host(clip[i - 1], fr, origins, plan.win_h, plan.win_w)
        word = line.replace(":", "").replace(";", "").split()
        assert word[:2] == ["frame", str(i)]
        counts = {k: int(word[word.index(k) + 1]) for k in ("easy", "hard", "reused", "of")}
        assert counts == {"easy": int((cls & changed).sum()), "hard": int((~cls & changed).sum()),
                          "reused": int((~changed).sum()), "of": n}, line
        act = routing.mean_activity(routing.window_activity_host(fr[0], origins, plan.win_h, plan.win_w), plan.win_h, plan.win_w)
        assert word[word.index("min") + 1] == "%.3f" % act.min() and word[word.index("max") + 1] == "%.3f" % act.max()
    assert any(t.startswith("routed %d windows" % (4 * n)) for t in r.stdout.splitlines())
    # one flag without the other is an argparse error
    for args in (["--easy-static", de], ["--easy-threshold", T], ["--route-report"]):
        r = subprocess.run(cmd + args + [src], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 2 and "need" in r.stderr, r.stderr
    image_cli = os.path.join(ROOT, "upscale_ofa_net_sr.py")
    r = subprocess.run([sys.executable, image_cli, "--static", dh, "--out", str(tmp_path / "o"), "--easy-threshold", T, src],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "need each other" in r.stderr


def test_image_cli_routes_and_reports(nets, tmp_path):
    from PIL import Image
    up, routing = amd("upscale"), amd("routing")
    hard, easy = nets
    dh, de = _export(hard, tmp_path / "hard"), _export(easy, tmp_path / "easy")
    (tmp_path / "in").mkdir()
    (tmp_path / "hr").mkdir()
    img = _image(9)
    tu = up.TiledUpscaler(hard, core=16, easy_net=easy, easy_threshold=0)
    T, cls = _threshold(routing, img, _plan_origins(), WIN_H, WIN_W)
    tu.set_easy_threshold(T)
    expect = tu.upscale(img).cpu().numpy()
    Image.fromarray(img, "RGB").save(str(tmp_path / "in" / "a.png"))
    Image.fromarray(expect, "RGB").save(str(tmp_path / "hr" / "a.png"))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "upscale_ofa_net_sr.py"), "--static", dh, "--core", "16", "--out", str(out),
           "--easy-static", de, "--easy-threshold", T, "--route-report", "--reference", str(tmp_path / "hr"),
           str(tmp_path / "in")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.asarray(Image.open(str(out / "a.png")).convert("RGB")), expect)
    assert "easy %d hard %d of 35 windows; activity min" % (int(cls.sum()), int((~cls).sum())) in r.stdout
    rec = json.load(open(str(out / "quality.json")))
    assert rec["images"][0]["route"] == {"windows": 35, "easy": int(cls.sum()), "hard": int((~cls).sum())}
    assert rec["images"][0]["sse"] == 0
    r = subprocess.run(cmd + ["--whole"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "nothing to route" in r.stderr
