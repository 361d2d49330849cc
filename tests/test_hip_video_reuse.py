"""Window reuse between video frames on the MI355X (`-m gpu`): the diff kernel (csrc/reuse.hip) against the host definition
(video.changed_windows_host), the compaction kernel against a list comprehension, the premise that a window's output
does not depend on its place in the batch, YUV420Stream against per-frame upscale_yuv420, which kernels an unchanged
frame launches, the stream's behaviour and the command line.  Everything is bit-exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, amd
from test_hip_video import _randomize, _static, _tail, _video_frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, WIN_H, WIN_W = 72, 104, 49, 56


@pytest.fixture(scope="module")
def small_net():
    return _randomize(_static(dict(ks=3, e=3, d=2, pixel_d=1)), 4)


def _plan_origins():
    plan = amd("upscale").plan_windows(H, W, 16, 17, 1, 4, 64)
    assert (len(plan), plan.win_h, plan.win_w) == (35, WIN_H, WIN_W)
    return [(w[0], w[1]) for w in plan.windows]


def _frame(Hh, Ww, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (Hh, Ww)).astype(np.uint8), rng.randint(0, 256, (Hh // 2, Ww // 2)).astype(np.uint8),
            rng.randint(0, 256, (Hh // 2, Ww // 2)).astype(np.uint8)]


def _gpu(planes, pad):
    return [_tail(torch.from_numpy(np.ascontiguousarray(p)), pad) for p in planes]


def _changed(up, cur, prev, table, h, w):
    flags = up.window_diff_yuv420(*cur, *prev, table, h, w)
    assert flags.dtype == torch.int32 and tuple(flags.shape) == (table.size(0), up.window_diff_slabs(h, w))
    assert bool(((flags == 0) | (flags == 1)).all())
    return flags.ne(0).any(dim=1).cpu().numpy()


# ---------------------------------------------------------------------------------------------- diff kernel
# (frame, window, origins): the plan of the stream tests; small odd windows; windows of more than one row slab
GEOMETRIES = {
    "plan": (H, W, WIN_H, WIN_W, None),
    "odd": (14, 18, 5, 7, [(0, 0), (1, 3), (3, 5), (9, 11), (4, 2), (7, 1), (2, 10), (9, 0)]),
    "one": (14, 18, 1, 1, [(0, 0), (13, 17), (4, 2), (5, 9), (13, 0), (0, 17)]),
    "whole": (14, 18, 14, 18, [(0, 0)]),
    "slabs": (160, 256, 151, 201, [(0, 0), (9, 55), (3, 20), (8, 1)]),
}
WILD = [(-5, 1000), (10 ** 12, -3), (-2 ** 62, 2 ** 62), (7, 10 ** 6)]


def _single_byte_changes(Hh, Ww, h, w, seed):
    """(plane, row, col): the four corner samples of each plane, the neighbour-tap sample of the plan geometry, and random
    samples up to about 40"""
    out = []
    for p, (R, C) in enumerate(((Hh, Ww), (Hh // 2, Ww // 2), (Hh // 2, Ww // 2))):
        out += [(p, 0, 0), (p, 0, C - 1), (p, R - 1, 0), (p, R - 1, C - 1)]
    if (Hh, Ww) == (H, W):
        out += [(1, 31, 20), (2, 31, 20), (1, 5, 6), (0, 61, 13), (0, 62, 13)]
    rng = np.random.RandomState(seed)
    while len(out) < 40:
        p = int(rng.randint(0, 3))
        R, C = (Hh, Ww) if p == 0 else (Hh // 2, Ww // 2)
        out.append((p, int(rng.randint(0, R)), int(rng.randint(0, C))))
    return out


@pytest.mark.parametrize("pads", [(0, 0), (1, 1), (3, 3), (1, 0), (0, 3), (3, 1)], ids=str)
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_diff_kernel_matches_host_definition(geometry, pads):
    up, video = amd("upscale"), amd("video")
    Hh, Ww, h, w, origins = GEOMETRIES[geometry]
    origins = (_plan_origins() if origins is None else origins) + WILD
    if geometry == "slabs":
        assert up.window_diff_slabs(h, w) > 1
    table = torch.tensor(origins, dtype=torch.int64, device=DEV)
    base = _frame(Hh, Ww, len(geometry))
    cur, prev = _gpu(base, pads[0]), _gpu(base, pads[1])
    assert not _changed(up, cur, prev, table, h, w).any()                       # identical frames
    got = _changed(up, cur, _gpu([p ^ 0xFF for p in base], pads[1]), table, h, w)    # every byte differs
    assert got.all()
    for (p, r, c) in _single_byte_changes(Hh, Ww, h, w, pads[0] * 4 + pads[1]):
        host = [q.copy() for q in base]
        host[p][r, c] ^= 1 << ((r + c) % 8)
        prev[p][r, c] = int(host[p][r, c])
        exp = video.changed_windows_host(host, base, origins, h, w)
        got = _changed(up, cur, prev, table, h, w)
        prev[p][r, c] = int(base[p][r, c])
        assert np.array_equal(got, exp), (p, r, c, got.tolist(), exp.tolist())
        if (p, r, c) == (1, 31, 20) and geometry == "plan":                      # the neighbour tap: rows 13 .. 61
            assert exp[14:21].any() and not exp[:14].any()
    assert not _changed(up, cur, prev, table, h, w).any()


def test_diff_kernel_is_deterministic_and_refuses_bad_calls():
    up, C = amd("upscale"), amd("_C")
    base = _frame(H, W, 5)
    cur, prev = _gpu(base, 0), _gpu(_frame(H, W, 6), 0)
    table = torch.tensor(_plan_origins(), dtype=torch.int64, device=DEV)
    a = up.window_diff_yuv420(*cur, *prev, table, WIN_H, WIN_W)
    b = up.window_diff_yuv420(*cur, *prev, table, WIN_H, WIN_W)
    assert torch.equal(a, b) and bool(a.all())
    with pytest.raises(C.OfasrError):
        up.window_diff_yuv420(*cur, *prev, table, H + 1, WIN_W)                  # window taller than the frame
    with pytest.raises(ValueError):
        up.window_diff_yuv420(*cur, *_gpu(_frame(H, W + 2, 6), 0), table, WIN_H, WIN_W)
    with pytest.raises(ValueError):
        up.window_diff_yuv420(*cur, *prev, table.to(torch.int32), WIN_H, WIN_W)
    with pytest.raises(C.OfasrError):
        up.window_diff_yuv420(*[p.cpu() for p in cur], *prev, table, WIN_H, WIN_W)
    L = C.lib()
    p = cur[0].data_ptr()
    assert L.ofasr_window_diff_yuv420(p, p, p, p, p, None, H, W, p, 1, 4, 4, p, None) == -1      # null pointer
    assert L.ofasr_window_diff_yuv420(p, p, p, p, p, p, H - 1, W, p, 1, 4, 4, p, None) == -1      # odd side
    assert L.ofasr_window_diff_yuv420(p, p, p, p, p, p, H, W, p, 65536, 4, 4, p, None) == -2      # too many windows
    assert L.ofasr_window_compact(p, 1, p, p, 65536, 4, p, p, p, p, None) == -2
    assert L.ofasr_window_compact(p, 65, p, p, 4, 4, p, p, p, p, None) == -1
    assert L.ofasr_window_compact(p, 1, p, p, 4, 0, p, p, p, None, None) == -1
    assert L.ofasr_window_diff_slabs(0, 5) == 0 and L.ofasr_window_diff_slabs(WIN_H, WIN_W) == 1


# ---------------------------------------------------------------------------------------------- compaction
def _check_compact(up, n, S, B, flags):
    """flags: numpy int [n, S]"""
    g = torch.Generator().manual_seed(n + B)
    origins = torch.randint(-50, 5000, (n, 2), generator=g, dtype=torch.int64)
    table = torch.randint(0, 10 ** 6, (n, 6), generator=g, dtype=torch.int64)
    rows = -(-n // B) * B
    out = (torch.full((rows, 2), -7, dtype=torch.int64, device=DEV), torch.full((n, 6), -7, dtype=torch.int64, device=DEV),
           torch.full((n,), -7, dtype=torch.int64, device=DEV), torch.full((1,), -7, dtype=torch.int64, device=DEV))
    f = torch.from_numpy(flags.astype(np.int32)).to(DEV)
    got = up.window_compact(f, origins.to(DEV), table.to(DEV), B, out)
    o, t, idx, count = (x.cpu() for x in got)
    keep = [i for i in range(n) if flags[i].any()]
    m = len(keep)
    assert int(count) == m
    assert idx[:m].tolist() == keep                                              # stable, in plan order
    assert torch.equal(t[:m], table[keep]) and torch.equal(o[:m], origins[keep])
    padded = -(-m // B) * B
    for j in range(m, padded):                                                    # the last batch repeats the last changed window
        assert o[j].tolist() == origins[keep[-1]].tolist()
    assert bool((o[padded:] == -7).all()) and bool((t[m:] == -7).all()) and bool((idx[m:] == -7).all())   # nothing else written
    again = up.window_compact(f, origins.to(DEV), table.to(DEV), B)
    assert int(again[3]) == m and torch.equal(again[2][:m].cpu(), idx[:m])


@pytest.mark.parametrize("B", [7, 3])
def test_compaction_of_the_plan(B):
    up = amd("upscale")
    n = 35
    rng = np.random.RandomState(B)
    for flags in (np.zeros((n, 1), int), np.ones((n, 1), int), (rng.rand(n, 1) < 0.3).astype(int),
                  np.eye(n, dtype=int)[:, [34]], np.eye(n, dtype=int)[:, [0]]):
        _check_compact(up, n, 1, B, flags)
    _check_compact(up, n, 3, B, (rng.rand(n, 3) < 0.15).astype(int))             # row slabs are folded


def test_compaction_across_waves_and_rounds():
    """more windows than one wave (64) and than one round of the workgroup (256)"""
    up = amd("upscale")
    rng = np.random.RandomState(0)
    for n, S, B in ((65, 1, 4), (300, 2, 16), (777, 3, 5)):
        _check_compact(up, n, S, B, (rng.rand(n, S) < 0.25).astype(int))
        _check_compact(up, n, S, B, np.ones((n, S), int))
        last = np.zeros((n, S), int)
        last[n - 1, S - 1] = 1
        _check_compact(up, n, S, B, last)


# ---------------------------------------------------------------------------------------------- premise
@pytest.mark.parametrize("mix_prec", ["f32", "bf16"])
def test_a_windows_output_does_not_depend_on_its_place_in_the_batch(small_net, mix_prec):
    """passes without the feature: if it failed, exact reuse with compacted batches would be impossible as designed"""
    up = amd("upscale")
    tu = up.TiledUpscaler(small_net, core=16, batch=8, mix_prec=mix_prec)
    y, u, v = _gpu(_video_frames(1, H, W, 3)[0], 0)
    table = torch.tensor(_plan_origins()[7:14], dtype=torch.int64, device=DEV)
    x = up.tile_gather_yuv420(y, u, v, table, WIN_H, WIN_W, tu.dtype)
    perm = torch.tensor([3, 0, 6, 1, 5, 2, 4], device=DEV)
    with torch.no_grad():
        a = tu._forward(x).clone()
        b = tu._forward(x[perm].contiguous()).clone()
        c = tu._forward(x[[0] * 7].contiguous()).clone()
    assert a.shape[0] == 7 and float(a.float().std()) > 0
    assert torch.equal(b, a[perm])
    assert torch.equal(c, a[[0] * 7])


# ---------------------------------------------------------------------------------------------- stream
def _sequence():
    f0 = [p.copy() for p in _video_frames(1, H, W, 21)[0]]
    f1 = [p.copy() for p in f0]
    f2 = [p.copy() for p in f1]
    f2[0][0:4, 0:4] ^= 0x55
    f3 = [p.copy() for p in f2]
    f3[1][31, 20] ^= 0x40
    f4 = [p.copy() for p in _video_frames(1, H, W, 22)[0]]
    return [f0, f1, f2, f3, f4]


@pytest.mark.parametrize("mix_prec,k", [("f32", 1), ("bf16", 2)])
def test_stream_equals_per_frame_upscale(small_net, mix_prec, k):
    up, video = amd("upscale"), amd("video")
    tu = up.TiledUpscaler(small_net, core=16, batch=8, mix_prec=mix_prec, self_ensemble=k)
    origins = _plan_origins()
    frames = _sequence()
    r3 = int(video.changed_windows_host(frames[2], frames[3], origins, WIN_H, WIN_W).sum())
    assert 0 < r3 < 35
    stream = tu.yuv420_stream()
    run, replays, changed = [], [], []
    captures = None
    for i, fr in enumerate(frames):
        before = tu.graphed.replays
        got = stream.upscale(*fr)
        replays.append(tu.graphed.replays - before)
        if i == 0:
            captures = tu.graphed.captures
        run.append(stream.stats.run)
        changed.append(stream.changed_windows())
        assert (stream.stats.windows, stream.stats.batches) == (35, -(-run[-1] // 7))
        got = [p.clone() for p in got]
        ref = tu.upscale_yuv420(*fr)
        for a, b in zip(got, ref):
            assert a.shape == b.shape and torch.equal(a, b), i
    assert run == [35, 0, 4, r3, 35]
    assert changed[2] == [0, 1, 7, 8]
    assert changed[3] == np.flatnonzero(video.changed_windows_host(frames[2], frames[3], origins, WIN_H, WIN_W)).tolist()
    assert changed[0] == changed[4] == list(range(35)) and changed[1] == []
    if k == 1:
        assert replays == [5, 0, 1, -(-r3 // 7), 5]                              # the full plan is 5 batches of 7
    assert tu.graphed.captures == captures                                       # every batch replayed the first frame's graph
    st = stream.stats
    assert (st.frames, st.frames_unchanged, st.total_windows, st.total_run) == (5, 1, 175, 74 + r3)
    assert st.total_batches == 5 + 0 + 1 + -(-r3 // 7) + 5


def test_identical_frame_launches_only_the_two_new_kernels(small_net):
    C, up = amd("_C"), amd("upscale")
    tu = up.TiledUpscaler(small_net, core=16, batch=8)
    fr = _gpu(_video_frames(1, H, W, 23)[0], 0)
    stream = tu.yuv420_stream()
    first = [p.clone() for p in stream.upscale(*fr)]
    C.reset_launch_counts()
    second = stream.upscale(*fr)
    torch.cuda.synchronize()
    table = C.launch_table()
    assert sorted(table.values()) == [1, 1], table
    assert any("window_diff_yuv420_kernel" in name for name in table) and any("window_compact_kernel" in name for name in table)
    assert stream.stats.run == 0 and stream.stats.batches == 0
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_stream_behaviour(small_net):
    up, C = amd("upscale"), amd("_C")
    tu = up.TiledUpscaler(small_net, core=16, batch=8)
    stream = tu.yuv420_stream(matrix="bt709", full_range=True)
    assert stream.changed_windows() == []
    frames = _video_frames(2, H, W, 31)
    out0 = stream.upscale(*frames[0])
    ptrs = [p.data_ptr() for p in out0]
    out1 = stream.upscale(*_gpu(frames[1], 1))                                   # planes on the GPU, unaligned
    assert [p.data_ptr() for p in out1] == ptrs                                  # the stream's own buffers
    for a, b in zip(out1, tu.upscale_yuv420(*frames[1], matrix="bt709", full_range=True)):
        assert torch.equal(a, b)
    assert stream.upscale(*frames[1]) is not None and stream.stats.run == 0
    stream.reset()
    stream.upscale(*frames[1])
    assert stream.stats.run == 35 and stream.changed_windows() == list(range(35))
    # another size restarts the stream
    small = _video_frames(2, 40, 56, 32)
    for fr in (small[0], small[0], small[1]):
        got = stream.upscale(*fr)
        assert got[0].shape == (160, 224)
        for a, b in zip(got, tu.upscale_yuv420(*fr, matrix="bt709", full_range=True)):
            assert torch.equal(a, b)
    n40 = len(tu.plan(40, 56))
    assert stream.stats.windows == n40 and stream.stats.run == n40
    # and back: nothing of the old size is reused
    got = stream.upscale(*frames[1])
    assert stream.stats.run == 35
    for a, b in zip(got, tu.upscale_yuv420(*frames[1], matrix="bt709", full_range=True)):
        assert torch.equal(a, b)


def test_stream_refusals(small_net):
    up, C = amd("upscale"), amd("_C")
    tu = up.TiledUpscaler(small_net, core=16)
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8)                             # noqa: E731
    stream = tu.yuv420_stream()
    with pytest.raises(ValueError, match="even sides"):
        stream.upscale(z(39, 56), z(19, 28), z(19, 28))
    with pytest.raises(ValueError, match="even sides"):
        stream.upscale(z(40, 55), z(20, 27), z(20, 27))
    with pytest.raises(ValueError):
        stream.upscale(z(40, 56), z(20, 28), z(20, 27))
    with pytest.raises(ValueError):
        stream.upscale(z(40, 56).float(), z(20, 28), z(20, 28))
    with pytest.raises(ValueError):
        tu.yuv420_stream(matrix="bt2020")
    with pytest.raises(ValueError, match="at most 65535"):                       # 256 x 257 cores of 16 x 16
        stream.upscale(z(4096, 4100), z(2048, 2050), z(2048, 2050))
    odd = up.TiledUpscaler(small_net, core=16)
    odd.scale = 3
    with pytest.raises(ValueError, match="even upscale factor"):
        odd.yuv420_stream().upscale(z(40, 56), z(20, 28), z(20, 28))
    cpu = up.TiledUpscaler(_static(dict(ks=3, e=3, d=2, pixel_d=1)), core=16)
    with pytest.raises(C.OfasrError):
        cpu.yuv420_stream().upscale(z(40, 56), z(20, 28), z(20, 28))
    # a refused frame leaves the stream usable
    fr = _video_frames(1, 40, 56, 33)[0]
    for a, b in zip(stream.upscale(*fr), tu.upscale_yuv420(*fr)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- command line
def test_cli_reuse_static_writes_the_same_file(small_net, tmp_path):
    video = amd("video")
    d = tmp_path / "net"
    d.mkdir()
    (d / "net_config.json").write_text(json.dumps(small_net.config))
    torch.save({"state_dict": {k: t.cpu() for k, t in small_net.state_dict().items()}}, str(d / "static_state_dict.pth"))
    Hh, Ww = 40, 56
    f0, f3 = _video_frames(2, Hh, Ww, 41)
    f2 = [p.copy() for p in f0]
    f2[0][30:34, 0:6] ^= 0x33                            # inside the two windows at x 0, outside the two at x 8
    src = str(tmp_path / "in.y4m")
    with video.Y4MWriter(src, Ww, Hh, fps="25:1") as w:
        for fr in (f0, f0, f2, f3):
            w.write_frame(*fr)

    def run(out, *args):
        cmd = [sys.executable, os.path.join(ROOT, "upscale_video_ofa_net_sr.py"), "--static", str(d), "--core", "16",
               "--out", out, src]
        r = subprocess.run(cmd + list(args), capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    plain, reuse = str(tmp_path / "plain.y4m"), str(tmp_path / "reuse.y4m")
    text_plain = run(plain)
    text_reuse = run(reuse, "--reuse-static")
    assert "windows run" not in text_plain and "frames/s" in text_reuse
    line = [t for t in text_reuse.splitlines() if t.startswith("windows run")]
    assert len(line) == 1 and line[0].endswith("1 frames unchanged")
    n = int(line[0].split()[4]) // 4
    ran = int(line[0].split()[2])
    assert 2 * n < ran < 3 * n                                                   # two full frames and a part of one
    assert open(plain, "rb").read() == open(reuse, "rb").read()
    assert os.path.getsize(plain) > 4 * Hh * Ww * 16
