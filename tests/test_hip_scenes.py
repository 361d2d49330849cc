"""Scene cuts on the MI355X (`-m gpu`): the fused decode + histogram kernel and the fold (csrc/scene.hip) against the host
definition (scenes.py) at every geometry, depth, matrix, range, plane alignment and content class, between guard bands,
SceneDetector on a planted clip, and the two command lines: the map that scenes_ofa_net_sr.py writes and the output of
upscale_video_ofa_net_sr.py --scene-map against the per-scene runs joined together.  Everything is bit-exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import placed
from conftest import ROOT, amd
from test_hip_video import COMBOS, _randomize, _static, _tail

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MULTI = (90, 1922)                                       # 45 block rows in 23 slabs of 2 (the last of 1): the fold's waves
#                                                          take one or two slabs each; W % 4 == 2
LONG = (2, 8202)                                         # one block row of 2051 blocks: three trips of a workgroup, the last
#                                                          with 2 lanes
GEOMETRIES = [(2, 2), (2, 6), (6, 2), (72, 104), (70, 102), MULTI, LONG]
KINDS = ["random", "flat", "columns", "high", "board"]
NET_A = dict(ks=3, e=3, d=2, pixel_d=1)
NET_B = dict(ks=3, e=3, d=2, pixel_d=0)


def _content(kind, H, W, depth, seed):
    """planes of one content class: random; flat (one bin per channel: the wave-uniform path); two values by column pairs
    (two bins inside every lane's 2 x 4 block: the in-lane merge); stored words with bits above the tenth (depth 10; the
    extremes 0 / 255 at depth 8); a checkerboard of the extremes"""
    rng = np.random.RandomState(seed)
    dt, top = (np.uint8, 256) if depth == 8 else (np.uint16, 1024)
    shapes = ((H, W), (H // 2, W // 2), (H // 2, W // 2))
    if kind == "random":
        planes = [rng.randint(0, top, s) for s in shapes]
    elif kind == "flat":
        planes = [np.full(s, val * (top // 256)) for s, val in zip(shapes, (90, 110, 140))]
    elif kind == "columns":
        planes = [np.where((np.arange(s[1]) // 2) % 2 == 0, lo, hi)[None, :].repeat(s[0], axis=0) * (top // 256)
                  for s, (lo, hi) in zip(shapes, ((60, 200), (128, 128), (128, 128)))]
    elif kind == "high":
        planes = [rng.randint(0, top, s) | (rng.randint(0, 64, s) << 10) if depth == 10 else rng.randint(0, 2, s) * 255
                  for s in shapes]
    else:
        planes = [(np.add.outer(np.arange(s[0]), np.arange(s[1])) & 1) * (top - 1) for s in shapes]
    return tuple(np.ascontiguousarray(p).astype(dt) for p in planes)


_HOST = {}


def _host_hist(kind, H, W, depth, seed, matrix, full):
    """(planes, host histogram), computed once per case and shared"""
    key = (kind, H, W, depth, seed, matrix, full)
    if key not in _HOST:
        planes = _content(kind, H, W, depth, seed)
        _HOST[key] = (planes, amd("scenes").rgb_histogram_host(*planes, matrix, full, depth))
    return _HOST[key]


def _fold(ops, partial, prev=None):
    hist = torch.empty(3, 256, dtype=torch.int32, device=DEV)
    dist = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    ops.hist_fold_distance(partial, hist, prev, dist)
    return hist, int(dist.item())


# ---------------------------------------------------------------------------------------------- histogram kernel
@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("H,W", GEOMETRIES)
def test_histogram_kernel_matches_host_definition(H, W, depth, pad):
    ops = amd("ops")
    S = ops.rgb_hist_slabs(H, W)
    if (H, W) == MULTI:
        assert H * W <= 500000 and S > 1 and (H // 2) % S != 0
    else:
        assert S == 1
    for matrix, full in COMBOS:
        for kind in KINDS:
            planes, exp = _host_hist(kind, H, W, depth, H + W, matrix, full)
            y, u, v = (_tail(torch.from_numpy(p), pad) for p in planes)
            a = ops.rgb_hist_yuv420(y, u, v, matrix, full)
            assert a.dtype == torch.int32 and tuple(a.shape) == (S, 3, 256)
            hist, d = _fold(ops, a)
            what = (kind, matrix, full)
            assert np.array_equal(hist.cpu().numpy().astype(np.int64), exp), what
            assert hist.sum(dim=1).tolist() == [H * W] * 3 and d == 0, what
            assert bool((a >= 0).all()), what
            b = ops.rgb_hist_yuv420(y, u, v, matrix, full, out=torch.full_like(a, -1))
            assert torch.equal(a, b), what                       # two runs: identical partials, every word written
            if kind == "flat":
                assert int((exp > 0).sum()) == 3, what            # one bin per channel
            if kind == "high" and depth == 10:
                assert max(int(p.max()) for p in planes) > 1023


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("H,W", [(70, 102), MULTI])
def test_histogram_kernel_between_guard_bands(H, W, depth):
    ops, scenes = amd("ops"), amd("scenes")
    S = ops.rgb_hist_slabs(H, W)
    es = 1 if depth == 8 else 2
    for name in ("P0", "P1", "P8"):
        planes, exp = _host_hist("random", H, W, depth, 5, "bt709", False)
        y, u, v = (placed.place(torch.from_numpy(p).to(DEV), placed.lead_of(name, es), "in", n) for p, n in zip(planes, "yuv"))
        partial = placed.place(torch.empty(S, 3, 256, dtype=torch.int32, device=DEV), placed.lead_of(name, 4), "out", "partial")
        hist = placed.place(torch.empty(3, 256, dtype=torch.int32, device=DEV), placed.lead_of(name, 4), "out", "hist")
        prev = placed.place(torch.from_numpy(exp.astype(np.int32)).to(DEV).flip(1).contiguous(), placed.lead_of(name, 4), "in",
                            "prev")
        dist = placed.place(torch.empty(1, dtype=torch.int64, device=DEV), placed.lead_of("P8" if name != "P0" else "P0", 8),
                            "out", "dist")
        ops.rgb_hist_yuv420(y, u, v, "bt709", False, out=partial)
        ops.hist_fold_distance(partial, hist, prev, dist)
        torch.cuda.synchronize()
        placed.check_all(y, u, v, partial, hist, prev, dist)
        assert not bool(partial.placement.unwritten().any()) and not bool(hist.placement.unwritten().any())
        assert np.array_equal(hist.cpu().numpy().astype(np.int64), exp), name
        assert int(dist.item()) == scenes.frame_distance_host(exp[:, ::-1], exp), name


def test_histogram_wrappers_refuse_bad_calls():
    ops, C = amd("ops"), amd("_C")
    y, u, v = (torch.zeros(s, dtype=torch.uint8, device=DEV) for s in ((6, 8), (3, 4), (3, 4)))
    y16 = torch.zeros(6, 8, dtype=torch.uint16, device=DEV)
    with pytest.raises(C.OfasrError):
        ops.rgb_hist_yuv420(y.cpu(), u.cpu(), v.cpu())
    with pytest.raises(ValueError):
        ops.rgb_hist_yuv420(y[:5], u, v)                                         # odd height
    with pytest.raises(ValueError):
        ops.rgb_hist_yuv420(y16, u, v)                                           # mixed sample types
    with pytest.raises(ValueError):
        ops.rgb_hist_yuv420(y, u, v, out=torch.zeros(2, 3, 256, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.rgb_hist_yuv420(y, u, v, out=torch.zeros(1, 3, 256, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        ops.rgb_hist_yuv420(y, u, v, matrix="bt2020")
    part = torch.zeros(1, 3, 256, dtype=torch.int32, device=DEV)
    hist = torch.zeros(3, 256, dtype=torch.int32, device=DEV)
    dist = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        ops.hist_fold_distance(part[0], hist, None, dist)
    with pytest.raises(ValueError):
        ops.hist_fold_distance(part, hist.to(torch.int64), None, dist)
    with pytest.raises(ValueError):
        ops.hist_fold_distance(part, hist, None, dist.to(torch.int32))
    L = C.lib()
    C.reset_launch_counts()
    p, q = y16.data_ptr(), part.data_ptr()
    good = ops.yuv_table("bt601", False, False)
    bad = (C.ctypes.c_int32 * 6)(16, 1 << 20, 0, 0, 0, 0)
    assert L.ofasr_rgb_hist_yuv420(None, p, p, 6, 8, good, q, None) == -1                       # null pointers
    assert L.ofasr_rgb_hist_yuv420(p, p, p, 6, 8, None, q, None) == -1
    assert L.ofasr_rgb_hist_yuv420(p, p, p, 6, 8, good, None, None) == -1
    assert L.ofasr_rgb_hist_yuv420(p, p, p, 5, 8, good, q, None) == -1                          # odd sides
    assert L.ofasr_rgb_hist_yuv420(p, p, p, 6, 7, good, q, None) == -1
    assert L.ofasr_rgb_hist_yuv420(p, p, p, 0, 8, good, q, None) == -1
    assert L.ofasr_rgb_hist_yuv420(p, p, p, 6, 8, bad, q, None) == -1                           # coefficient bound
    assert L.ofasr_rgb_hist_yuv420(p, p, p, 6, 8, good, q + 2, None) == -1                      # misaligned table
    assert L.ofasr_rgb_hist_yuv420(p, p, p, 2 ** 14, 2 ** 14 + 2, good, q, None) == -2           # more than 2^28 pixels
    assert "2^28" in L.ofasr_last_error_string().decode()
    assert L.ofasr_rgb_hist_yuv420p16(p + 1, p, p, 6, 8, 10, good, q, None) == -1               # odd 16-bit pointer
    for depth in (8, 9, 12, 16):
        assert L.ofasr_rgb_hist_yuv420p16(p, p, p, 6, 8, depth, good, q, None) == -1
    assert L.ofasr_hist_fold_distance(None, 1, q, None, q, None) == -1
    assert L.ofasr_hist_fold_distance(q, 1, None, None, q, None) == -1
    assert L.ofasr_hist_fold_distance(q, 1, q, None, None, None) == -1
    assert L.ofasr_hist_fold_distance(q, 0, q, None, q, None) == -1
    assert L.ofasr_hist_fold_distance(q, 1025, q, None, q, None) == -1
    assert L.ofasr_hist_fold_distance(q, 1, q, q, q, None) == -1                                # hist_out == hist_prev
    assert L.ofasr_hist_fold_distance(q, 1, q, None, q + 4, None) == -1                         # misaligned int64
    assert C.launch_table() == {}                                                               # nothing was launched
    assert L.ofasr_rgb_hist_slabs(1080, 1920) == 270                                            # a 1080p frame fills the device
    assert L.ofasr_rgb_hist_slabs(2 ** 14, 2 ** 14) == 1024 and L.ofasr_rgb_hist_slabs(2 ** 14, 2 ** 14 + 2) == 0
    assert L.ofasr_rgb_hist_slabs(5, 8) == 0 and L.ofasr_rgb_hist_slabs(0, 8) == 0 and L.ofasr_rgb_hist_slabs(2, 2) == 1


# ---------------------------------------------------------------------------------------------- distances
@pytest.mark.parametrize("depth", [8, 10])
def test_fold_distance_matches_host_definition(depth):
    ops, scenes = amd("ops"), amd("scenes")
    H, W = MULTI
    P = H * W
    frames = [_content("random", H, W, depth, s) for s in (1, 2, 3)]
    top = 255 if depth == 8 else 1023
    dt = np.uint8 if depth == 8 else np.uint16
    k = 1 if depth == 8 else 4
    for yv in (16 * k, 235 * k):                         # bt601 limited range: black, then white
        frames.append((np.full((H, W), yv, dt), np.full((H // 2, W // 2), (top + 1) // 2, dt),
                       np.full((H // 2, W // 2), (top + 1) // 2, dt)))
    exp = scenes.distances_host(frames, "bt601", False, depth)
    assert exp[0] == 0 and exp[4] == 6 * P * P and min(exp[1:]) > 0
    got, prev = [], None
    for planes in frames:
        part = ops.rgb_hist_yuv420(*(torch.from_numpy(p).to(DEV) for p in planes))
        prev, d = _fold(ops, part, prev)
        got.append(d)
    assert got == exp
    assert _fold(ops, part, None)[1] == 0                # a null hist_prev gives 0, over whatever the word held


def test_scene_detector_on_a_planted_clip():
    scenes = amd("scenes")
    H, W = 72, 104
    rng = np.random.RandomState(7)

    def frame(lo, hi):
        return (rng.randint(lo, hi, (H, W)).astype(np.uint8), rng.randint(120, 136, (H // 2, W // 2)).astype(np.uint8),
                rng.randint(120, 136, (H // 2, W // 2)).astype(np.uint8))

    a = [frame(30, 62) for _ in range(3)]
    b = [frame(180, 212) for _ in range(3)]
    clip = [a[0], a[1], a[1], a[2], b[0], b[0], b[1], b[2]]                      # a repeated frame inside each scene
    exp = scenes.distances_host(clip)
    assert exp[2] == exp[5] == 0 and exp[1] > 0
    det = scenes.SceneDetector(H, W, 8, "bt601", False, DEV)
    assert det.distances() == []
    for y, u, v in clip:
        det.push(*(torch.from_numpy(p).to(DEV) for p in (y, u, v)))
    assert det.distances() == exp
    assert np.array_equal(det.histogram(), scenes.rgb_histogram_host(*clip[-1]))
    # inside a scene two draws of the same noise differ by about 2 P per channel, d / 6 P^2 ~ 1 / P = 1.3e-4; across the cut
    # the supports are disjoint and at most 38 + 26 + 2, 38 + 19 + 2 and 38 + 32 + 2 bins wide (luma span x cy plus the
    # chroma span x the channel's coefficients), so by Cauchy-Schwarz d / 6 P^2 >= (2/66 + 2/59 + 2/72) / 6 = 0.0153
    limit = scenes.distance_limit("0.01", det.P)
    assert max(exp[1:4] + exp[5:]) < limit < exp[4]
    assert scenes.cuts(det.distances(), limit, 1) == [(0, 4), (4, 8)]
    assert scenes.cuts(det.distances(), limit, 5) == [(0, 8)]
    with pytest.raises(ValueError):
        det.push(*(torch.from_numpy(p).to(DEV) for p in _content("random", 6, 10, 8, 0)))


def test_scene_detector_grows_its_distance_buffer():
    scenes = amd("scenes")
    H, W = 6, 10
    two = [_content("random", H, W, 10, s) for s in (1, 2)]
    hists = [scenes.rgb_histogram_host(*p, "bt709", True, 10) for p in two]
    step = scenes.frame_distance_host(*hists)
    det = scenes.SceneDetector(H, W, 10, "bt709", True, DEV)
    dev = [tuple(torch.from_numpy(p).to(DEV) for p in planes) for planes in two]
    order = [0, 1, 1, 0] * 18                                                    # 72 frames: past the first 64 slots
    for i in order:
        det.push(*dev[i])
    assert det.distances() == [0] + [step if i != j else 0 for i, j in zip(order, order[1:])]
    assert det.frames == 72 and step > 0


# ---------------------------------------------------------------------------------------------- command lines
N_FRAMES, CUT, CH, CW = 6, 3, 72, 104


def _run_all(cmds, ok=True):
    """the commands side by side, each a fresh process; [(returncode, stdout + stderr)]"""
    procs = [subprocess.Popen([sys.executable] + c, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
             for c in cmds]
    out = []
    for p in procs:
        text, _ = p.communicate(timeout=300)
        out.append((p.returncode, text))
    if ok:
        for code, text in out:
            assert code == 0, text
    return out


def _export(net, d):
    d.mkdir()
    (d / "net_config.json").write_text(json.dumps(net.config))
    torch.save({"state_dict": {k: t.cpu() for k, t in net.state_dict().items()}}, str(d / "static_state_dict.pth"))
    return str(d)


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """6 frames of 72 x 104 in two scenes of 3, two tiny random x4 exports, and the map scenes_ofa_net_sr.py wrote"""
    video, scenes = amd("video"), amd("scenes")
    tmp = tmp_path_factory.mktemp("scenes")
    rng = np.random.RandomState(3)

    def frame(lo, hi):
        return (rng.randint(lo, hi, (CH, CW)).astype(np.uint8), rng.randint(120, 136, (CH // 2, CW // 2)).astype(np.uint8),
                rng.randint(120, 136, (CH // 2, CW // 2)).astype(np.uint8))

    # the content classes of test_scene_detector_on_a_planted_clip: 1.3e-4 inside a scene, >= 0.0153 across the cut
    frames = [frame(30, 62) for _ in range(CUT)] + [frame(180, 212) for _ in range(N_FRAMES - CUT)]
    src = str(tmp / "in.y4m")
    with video.Y4MWriter(src, CW, CH, fps="25:1") as w:
        for fr in frames:
            w.write_frame(*fr)
    dirs = [_export(_randomize(_static(NET_A), 4), tmp / "net_a"), _export(_randomize(_static(NET_B), 5), tmp / "net_b")]
    path = str(tmp / "scenes.json")
    (_, text), = _run_all([[os.path.join(ROOT, "scenes_ofa_net_sr.py"), "--threshold", "0.01", "--min-scene", "2", "--top", "2",
                            "--out", path, src]])
    return dict(tmp=tmp, frames=frames, src=src, dirs=dirs, map=path, text=text,
                host=scenes.distances_host(frames))


def test_scene_tool_writes_the_planted_map(clip):
    scenes = amd("scenes")
    m = scenes.SceneMap.load(clip["map"])
    assert m.distance == clip["host"] and m.frames == N_FRAMES and m.first == 0
    assert (m.width, m.height, m.depth, m.matrix, m.range, m.threshold, m.min_scene) == (CW, CH, 8, "bt601", "tv", "0.01", 2)
    assert m.scenes == [{"first": 0, "stop": CUT}, {"first": CUT, "stop": N_FRAMES}]
    text = clip["text"]
    assert "\n0:%d\n%d:%d\n" % (CUT, CUT, N_FRAMES) in text and "frames/s" in text and "2 scenes" in text
    P = CH * CW
    norm = clip["host"][CUT] / (6.0 * P * P)
    assert "frame %d: %.6g" % (CUT, norm) in text and "max %.6g" % norm in text
    # a frame range: absolute numbers, distance[0] = 0 whatever precedes; without --threshold no scenes are written
    part = str(clip["tmp"] / "part.json")
    (_, text), = _run_all([[os.path.join(ROOT, "scenes_ofa_net_sr.py"), "--frames", "2:5", "--out", part, clip["src"]]])
    m = scenes.SceneMap.load(part)
    assert (m.first, m.frames, m.threshold, m.scenes) == (2, 3, None, [])
    assert m.distance == [0] + clip["host"][3:5] and "frame %d: " % CUT in text
    assert "threshold" not in text and not [ln for ln in text.splitlines() if ln.replace(":", "").isdigit()]


def _scene_map(clip, name, scenes_list):
    scenes = amd("scenes")
    m = scenes.SceneMap.load(clip["map"])
    m.scenes = scenes_list
    m.validate()
    path = str(clip["tmp"] / name)
    m.save(path)
    return path


@pytest.mark.parametrize("mode", ["plain", "reuse", "depth10"])
def test_scene_map_output_equals_the_per_scene_runs_joined(clip, mode):
    a, b = clip["dirs"]
    path = _scene_map(clip, "served.json", [{"first": 0, "stop": CUT}, {"first": CUT, "stop": N_FRAMES, "static": b}])
    flags = {"plain": [], "reuse": ["--reuse-static"], "depth10": ["--out-depth", "10"]}[mode]
    tool = os.path.join(ROOT, "upscale_video_ofa_net_sr.py")
    outs = [str(clip["tmp"] / ("%s_%d.yuv" % (mode, i))) for i in range(3)]
    base = [tool, "--core", "16"] + flags
    runs = _run_all([base + ["--static", a, "--scene-map", path, "--out", outs[0], clip["src"]],
                     base + ["--static", a, "--frames", "0:%d" % CUT, "--out", outs[1], clip["src"]],
                     base + ["--static", b, "--frames", "%d:%d" % (CUT, N_FRAMES), "--out", outs[2], clip["src"]]])
    got, first, second = (open(o, "rb").read() for o in outs)
    assert len(got) == N_FRAMES * CH * 4 * CW * 4 * 3 // 2 * (2 if mode == "depth10" else 1)
    assert got == first + second
    assert first[:len(second)] != second                                        # the two exports do differ
    assert "%d frames" % N_FRAMES in runs[0][1] and "1 export switches" in runs[0][1] and "2 scenes, 2 exports" in runs[0][1]
    assert "export switches" not in runs[1][1] and "scene map" not in runs[1][1]


def test_scene_map_refusals(clip):
    a, b = clip["dirs"]
    other = clip["tmp"] / "net_x2"
    other.mkdir()
    cfg = json.load(open(os.path.join(b, "net_config.json")))
    (other / "net_config.json").write_text(json.dumps(dict(cfg, upscale=2)))
    mismatch = _scene_map(clip, "mismatch.json", [{"first": 0, "stop": CUT},
                                                  {"first": CUT, "stop": N_FRAMES, "static": str(other)}])
    short = _scene_map(clip, "short.json", [{"first": 1, "stop": N_FRAMES}])
    tool = os.path.join(ROOT, "upscale_video_ofa_net_sr.py")
    out = str(clip["tmp"] / "refused.yuv")
    runs = _run_all([[tool, "--core", "16", "--static", a, "--scene-map", mismatch, "--out", out, clip["src"]],
                     [tool, "--core", "16", "--static", a, "--scene-map", short, "--out", out + "2", clip["src"]]], ok=False)
    assert runs[0][0] != 0 and "x2" in runs[0][1] and "x4" in runs[0][1] and str(other) in runs[0][1] and a in runs[0][1]
    assert runs[1][0] != 0 and "frame 0 lies outside the scene map" in runs[1][1]
    assert "Traceback" not in runs[0][1] + runs[1][1]
