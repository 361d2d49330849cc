"""Scene cuts, host side (no GPU): the histogram and the distance of scenes.py, the exact limit, the cut rule, the scene map
file and its validation, --video-scene, the refusal of --scene-map with --easy-static, and the ABI names."""
import argparse
import importlib
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT, amd

COMBOS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]


def _flat(H, W, yv, uv=128, vv=128, dt=np.uint8):
    return np.full((H, W), yv, dt), np.full((H // 2, W // 2), uv, dt), np.full((H // 2, W // 2), vv, dt)


def _random(H, W, seed, depth=8):
    rng = np.random.RandomState(seed)
    dt, top = (np.uint8, 256) if depth == 8 else (np.uint16, 1024)
    return (rng.randint(0, top, (H, W)).astype(dt), rng.randint(0, top, (H // 2, W // 2)).astype(dt),
            rng.randint(0, top, (H // 2, W // 2)).astype(dt))


# ---------------------------------------------------------------------------------------------- histogram, distance
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("H,W", [(2, 2), (6, 10), (38, 54)])
def test_histogram_counts_every_pixel_once(H, W, depth):
    scenes, video = amd("scenes"), amd("video")
    for matrix, full in COMBOS:
        planes = _random(H, W, H + W + depth, depth)
        h = scenes.rgb_histogram_host(*planes, matrix, full, depth)
        assert h.shape == (3, 256) and h.dtype == np.int64
        assert h.sum(axis=1).tolist() == [H * W] * 3
        rgb = video.yuv420_to_rgb_host(*planes, matrix, full, depth).astype(np.int64) >> (depth - 8)
        for c in range(3):
            for b in (0, 17, 128, 255):
                assert h[c, b] == int((rgb[..., c] == b).sum())


def test_ten_bit_words_above_the_tenth_bit_read_as_1023():
    scenes = amd("scenes")
    y, u, v = _random(6, 10, 3, 10)
    y2 = y.copy()
    y2[0, 0], y2[3, 7] = 0xFFFF, 0x8400
    y3 = y.copy()
    y3[0, 0] = y3[3, 7] = 1023
    assert np.array_equal(scenes.rgb_histogram_host(y2, u, v, depth=10), scenes.rgb_histogram_host(y3, u, v, depth=10))


def test_black_to_white_is_the_largest_distance():
    scenes = amd("scenes")
    H, W = 6, 10
    P = H * W
    black = scenes.rgb_histogram_host(*_flat(H, W, 16))
    white = scenes.rgb_histogram_host(*_flat(H, W, 235))
    assert black[:, 0].tolist() == [P] * 3 and white[:, 255].tolist() == [P] * 3
    assert scenes.frame_distance_host(black, white) == 6 * P * P == scenes.max_distance(P)
    assert scenes.frame_distance_host(white, white) == 0
    r = scenes.rgb_histogram_host(*_random(H, W, 1))
    assert scenes.frame_distance_host(r, r.copy()) == 0
    assert scenes.distances_host([_flat(H, W, 16), _flat(H, W, 16), _flat(H, W, 235)]) == [0, 0, 6 * P * P]


def test_distance_is_exact_at_the_pixel_cap():
    scenes = amd("scenes")
    P = 2 ** 28
    a, b = np.zeros((3, 256), np.int64), np.zeros((3, 256), np.int64)
    a[:, 0], b[:, 255] = P, P
    assert scenes.frame_distance_host(a, b) == 6 * P * P < 2 ** 63
    with pytest.raises(ValueError, match="2\\^28"):
        scenes.check_pixels(2 ** 14, 2 ** 14 + 2)
    assert scenes.check_pixels(2 ** 14, 2 ** 14) == P
    with pytest.raises(ValueError):
        scenes.frame_distance_host(a[:2], b)


def test_distance_limit_is_exact():
    scenes = amd("scenes")
    P = 2 ** 28
    top = 6 * P * P
    assert scenes.distance_limit("1", P) == scenes.distance_limit(1, P) == scenes.distance_limit(1.0, P) == top
    assert scenes.distance_limit("0", P) == scenes.distance_limit(0.0, P) == 0
    assert scenes.distance_limit("0.1", P) == top // 10                      # 0.1 the decimal, not the double
    assert scenes.distance_limit("0.3", P) == 3 * top // 10
    assert scenes.distance_limit(" 1e-3 ", P) == top // 1000
    assert scenes.distance_limit("0.000001", 1000) == 6                       # floor(6e6 * 1e-6)
    assert scenes.distance_limit("0.9999999999999999999", P) == top - 1
    assert scenes.distance_limit(0.25, 10) == 150
    for bad in ("-0.1", "1.0000001", -1, 2, "nan", "inf", float("nan"), float("inf"), "abc", "", None, True, [0.5]):
        with pytest.raises(ValueError):
            scenes.distance_limit(bad, P)
    for bad_p in (0, -4, P + 1, 2.5, True):
        with pytest.raises(ValueError):
            scenes.distance_limit("0.5", bad_p)


def test_cut_rule():
    scenes = amd("scenes")
    cuts = scenes.cuts
    assert cuts([], 5) == []
    assert cuts([0], 5) == [(0, 1)]
    assert cuts([0, 1, 5, 2], 5) == [(0, 4)]                                   # d > limit, not >=
    assert cuts([0, 1, 6, 2], 5) == [(0, 2), (2, 4)]
    assert cuts([99, 1, 1, 1], 5) == [(0, 4)]                                  # d[0] is not looked at
    assert cuts([0, 1, 1, 9], 5) == [(0, 3), (3, 4)]                           # a cut at the last frame
    assert cuts([0, 9, 9, 9], 5) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert cuts([0, 9, 9, 9], 5, 2) == [(0, 2), (2, 4)]                        # min_scene suppresses the cuts in between
    assert cuts([0, 1, 9, 9, 1, 1, 9], 5, 3) == [(0, 3), (3, 6), (6, 7)]       # frame 2 is too early, frame 3 is not
    assert cuts([0, 9, 1, 1], 5, 2) == [(0, 4)]                                # the suppressed cut is not made later
    assert cuts([0, 2 ** 62, 1], 2 ** 62 - 1) == [(0, 1), (1, 3)]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            cuts([0, 1], 5, bad)
    for d in ([0, 7, 1, 8, 8, 0, 9], [0] * 5):
        for m in (1, 2, 3):
            got = cuts(d, 5, m)
            assert got[0][0] == 0 and got[-1][1] == len(d)
            assert all(a[1] == b[0] for a, b in zip(got, got[1:])) and all(s1 > s0 for s0, s1 in got)


# ---------------------------------------------------------------------------------------------- the scene map
def _map(**over):
    base = dict(video="clip.y4m", frames=6, first=2, width=104, height=72, depth=8, matrix="bt601", range="tv",
                threshold="0.25", min_scene=1, distance=[0, 1, 2, 2 ** 62, 4, 5],
                scenes=[{"first": 2, "stop": 5}, {"first": 5, "stop": 8, "static": "exp/b"}])
    base.update(over)
    return base


def test_scene_map_round_trip(tmp_path):
    scenes = amd("scenes")
    m = scenes.SceneMap(**_map())
    path = str(tmp_path / "scenes.json")
    m.save(path)
    with open(path) as f:
        raw = json.load(f)
    assert set(raw) == set(scenes.MAP_KEYS) and raw["distance"][3] == 2 ** 62
    back = scenes.SceneMap.load(path)
    assert back.to_dict() == m.to_dict() == _map()
    assert [back.scene_of(i) for i in range(2, 8)] == [0, 0, 0, 1, 1, 1]
    assert back.frame_range(1) == (5, 8)
    for frame in (1, 8, -1):
        with pytest.raises(ValueError, match="frame %d " % frame):
            back.scene_of(frame)
    for k in (2, -1, True, "0"):
        with pytest.raises(ValueError):
            back.frame_range(k)
    bare = scenes.SceneMap(**_map(threshold=None, scenes=[]))                  # distances only
    bare.save(path)
    assert scenes.SceneMap.load(path).scenes == []
    with pytest.raises(ValueError, match="no scenes"):
        bare.scene_of(2)


@pytest.mark.parametrize("over,word", [
    (dict(scenes=[{"first": 2, "stop": 2}]), r"scenes\[0\].*empty"),
    (dict(scenes=[{"first": 2, "stop": 5}, {"first": 5, "stop": 4}]), r"scenes\[1\].*empty"),
    (dict(scenes=[{"first": 2, "stop": 5}, {"first": 4, "stop": 8}]), r"scenes\[1\].*not increasing"),
    (dict(scenes=[{"first": 2, "stop": 5}, {"first": 6, "stop": 8}]), r"scenes\[1\].*not contiguous"),
    (dict(scenes=[{"first": -1, "stop": 5}]), r"scenes\[0\].*before frame 0"),
    (dict(scenes=[{"first": 2, "stop": 5}, {"first": 5}]), r"scenes\[1\]"),
    (dict(scenes=[{"first": 2, "stop": 5, "export": "x"}]), r"scenes\[0\]"),
    (dict(scenes=[{"first": 2.0, "stop": 5}]), r"scenes\[0\].*integers"),
    (dict(scenes=[{"first": 2, "stop": 5, "static": 3}]), r"scenes\[0\].*static"),
    (dict(scenes=[[2, 5]]), r"scenes\[0\]"),
    (dict(distance=[0, 1]), "2 distances for 6 frames"),
    (dict(distance=[0, 1, 2, -3, 4, 5]), r"distance\[3\]"),
    (dict(distance=[0, 1, 2, 3.5, 4, 5]), r"distance\[3\]"),
    (dict(depth=12), "depth"),
    (dict(matrix="bt2020"), "matrix"),
    (dict(range="full"), "range"),
    (dict(width=0), "width"),
    (dict(frames=-1), "frames"),
    (dict(min_scene=0), "min_scene"),
    (dict(threshold=[1]), "threshold"),
])
def test_scene_map_validation_names_the_offender(over, word):
    scenes = amd("scenes")
    with pytest.raises(ValueError, match=word):
        scenes.SceneMap(**_map(**over))


def test_scene_map_file_errors(tmp_path):
    scenes = amd("scenes")
    path = str(tmp_path / "m.json")
    obj = _map()
    del obj["distance"]
    for content, word in ((json.dumps(obj), "missing key.*distance"), (json.dumps(dict(_map(), extra=1)), "unknown key.*extra"),
                          ("[1, 2]", "JSON object"), ("{not json", "not a JSON file"),
                          (json.dumps(_map(scenes={"first": 0})), "must be lists")):
        with open(path, "w") as f:
            f.write(content)
        with pytest.raises(ValueError, match=word) as e:
            scenes.SceneMap.load(path)
        assert path in str(e.value)


# ---------------------------------------------------------------------------------------------- command lines
def _parse_video(argv):
    vf = amd("imagenet_codebase.data_providers.video_frames")
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", default="exp")
    vf.add_video_args(ap)
    a = ap.parse_args(argv)
    return a, vf.take_video_args(a)


def test_video_scene_is_the_frame_range_of_a_scene(tmp_path):
    scenes = amd("scenes")
    path = str(tmp_path / "with:colon.json")
    scenes.SceneMap(**_map()).save(path)
    base = dict(videos=["a.y4m"], video_size=None, video_frames=None, video_valid_every=10, matrix="bt601", full_range=False)
    a, kw = _parse_video([])
    assert kw is None and a.__dict__ == {"path": "exp"}
    a, kw = _parse_video(["--video", "a.y4m"])                                  # without the flag: what it was before
    assert a.__dict__ == {"path": "exp"} and kw == base
    a, kw = _parse_video(["--video", "a.y4m", "--video-frames", "5:8"])
    by_range = kw
    a, kw = _parse_video(["--video", "a.y4m", "--video-scene", path + ":1"])
    assert a.__dict__ == {"path": "exp"} and kw == by_range == dict(base, video_frames=(5, 8))
    assert _parse_video(["--video", "a.y4m", "--video-scene", path + ":0"])[1]["video_frames"] == (2, 5)
    assert scenes.parse_video_scene(path + ":1") == (path, 1)
    for argv, word in ((["--video-scene", path + ":0"], "exactly one --video"),
                       (["--video", "a.y4m", "--video", "b.y4m", "--video-scene", path + ":0"], "exactly one --video"),
                       (["--video", "a.y4m", "--video-frames", "0:4", "--video-scene", path + ":0"], "exclude"),
                       (["--video", "a.y4m", "--video-scene", path + ":2"], "scenes 0 .. 1"),
                       (["--video", "a.y4m", "--video-scene", path], "FILE:K"),
                       (["--video", "a.y4m", "--video-scene", path + ":x"], "FILE:K"),
                       (["--video", "a.y4m", "--video-scene", str(tmp_path / "none.json") + ":0"], "none.json")):
        with pytest.raises(SystemExit, match=word):
            _parse_video(argv)


def test_scene_map_with_easy_static_is_refused_at_parsing(capsys):
    tool = importlib.import_module("upscale_video_ofa_net_sr")
    base = ["--static", "a", "--out", "o.yuv", "in.y4m"]
    assert tool.parse_args(base).scene_map is None
    assert tool.parse_args(base + ["--scene-map", "m.json", "--reuse-static", "--out-depth", "10"]).scene_map == "m.json"
    with pytest.raises(SystemExit):
        tool.parse_args(base + ["--scene-map", "m.json", "--easy-static", "b", "--easy-threshold", "1"])
    assert "--scene-map with --easy-static" in capsys.readouterr().err


def test_scene_tool_arguments(capsys):
    tool = importlib.import_module("scenes_ofa_net_sr")
    a = tool.parse_args(["in.y4m"])
    assert (a.threshold, a.min_scene, a.out, a.top, a.frames) == (None, 1, None, 10, (0, None))
    a = tool.parse_args(["--size", "104x72", "--depth", "10", "--threshold", "0.05", "--min-scene", "3", "--frames", "2:9",
                         "--out", "s.json", "--top", "4", "in.yuv"])
    assert (a.size, a.depth, a.threshold, a.min_scene, a.frames, a.top) == ((104, 72), 10, "0.05", 3, (2, 9), 4)
    for bad in (["--threshold", "1.5"], ["--threshold", "x"], ["--min-scene", "0"], ["--top", "-1"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad + ["in.y4m"])
        assert bad[0] in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------- ABI
NAMES = ("ofasr_rgb_hist_slabs", "ofasr_rgb_hist_yuv420", "ofasr_rgb_hist_yuv420p16", "ofasr_hist_fold_distance")


def test_abi_names_are_declared_and_bound():
    C = amd("_C")
    with open(os.path.join(ROOT, "include", "ofasr.h")) as f:
        hdr = f.read()
    for name in NAMES:
        assert re.search(r"^int(64_t)? %s\(" % name, hdr, re.M), name
        assert name in C.SIGNATURES
    assert int(re.search(r"#define OFASR_VERSION (\d+)", hdr).group(1)) >= 312
    with open(os.path.join(ROOT, PKG_DIR, "csrc", "build.sh")) as f:
        assert "scene.hip" in f.read()


PKG_DIR = "ofa-for-super-resolution_amd"
