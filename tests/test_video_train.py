"""Host side of training on raw YUV 4:2:0 video (data_providers/augment.py: gather_yuv420_np, apply_params_yuv420_np,
video_pool_layout; data_providers/video_frames.py: the frame split and the command-line flags).  The byte-level
definition of ofasr_aug_gather_yuv420 against the transforms applied to video.yuv420_to_rgb_host of the whole frame."""
import argparse

import numpy as np
import pytest
import torch

from conftest import amd

SHAPES = [(38, 54), (64, 64), (40, 96)]        # (H, W) of the three pooled frames
FIXED_ANGLES = [0.0, 90.0, -90.0, 180.0, 45.0, -33.3, 1e-9]
COMBOS = [("bt601", False), ("bt709", True)]


def _aug():
    return amd("imagenet_codebase.data_providers.augment")


def _vf():
    return amd("imagenet_codebase.data_providers.video_frames")


def make_frames(seed=5):
    """three frames of noise over the whole byte range (illegal luma / chroma values included: the clamps work) and the
    pool that holds them back to back as a yuv420p file would"""
    rng = np.random.RandomState(seed)
    frames = [tuple(rng.randint(0, 256, s).astype(np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
              for (h, w) in SHAPES]
    host = np.concatenate([p.reshape(-1) for f in frames for p in f])
    offs = [int(o) for o in np.cumsum([0] + [h * w * 3 // 2 for (h, w) in SHAPES])[:-1]]
    return frames, offs, host


def cases(S, seed):
    """(frame, (i, j, flip, angle)): four corners and an interior crop at odd (i, j) of every frame, flip on and off,
    every angle"""
    g = torch.Generator().manual_seed(seed)
    angles = FIXED_ANGLES + [float(torch.empty(1).uniform_(-90, 90, generator=g).item()) for _ in range(10)]
    out = []
    for k, (h, w) in enumerate(SHAPES):
        inner = (((h - S) // 2) | 1, ((w - S) // 3) | 1)
        assert inner[0] <= h - S and inner[1] <= w - S
        for (i, j) in [(0, 0), (0, w - S), (h - S, 0), (h - S, w - S), inner]:
            for flip in (False, True):
                for a in angles:
                    out.append((k, (i, j, flip, a)))
    return out


@pytest.mark.parametrize("matrix,full", COMBOS)
@pytest.mark.parametrize("S", [8, 30, 32])
def test_gather_yuv420_np_equals_transforms_of_decoded_frame(S, matrix, full):
    aug, video = _aug(), amd("video")
    frames, offs, host = make_frames()
    cs = cases(S, 100 + S)
    table = aug.make_table([(offs[k],) + SHAPES[k] + (p,) for k, p in cs], S, yuv420=True)
    got = aug.gather_yuv420_np(host, table.numpy(), S, video.yuv_coeffs(matrix, full)[0])
    assert got.shape == (len(cs), 3, S, S) and got.dtype == np.uint8
    rgb = [video.yuv420_to_rgb_host(*f, matrix=matrix, full_range=full) for f in frames]
    for n, (k, p) in enumerate(cs):
        ref = aug.apply_params_np(rgb[k], S, p).transpose(2, 0, 1)
        assert np.array_equal(got[n], ref), "S=%d frame %d params %r: %d bytes differ" % (S, k, p, int((got[n] != ref).sum()))
    for n in (0, len(cs) // 2, len(cs) - 1):
        k, p = cs[n]
        assert np.array_equal(aug.apply_params_yuv420_np(*frames[k], size=S, params=p, matrix=matrix, full_range=full),
                              got[n].transpose(1, 2, 0))


def test_chroma_comes_from_the_frame_not_the_crop():
    """decoding the crop's own planes replicates chroma at the crop's edge: that is another image"""
    aug, video = _aug(), amd("video")
    y, u, v = make_frames()[0][1]                       # the 64 x 64 frame
    whole = aug.apply_params_yuv420_np(y, u, v, 32, (16, 16, False, 0.0))
    alone = video.yuv420_to_rgb_host(y[16:48, 16:48], u[8:24, 8:24], v[8:24, 8:24])
    assert np.array_equal(whole[1:-1, 1:-1], alone[1:-1, 1:-1]) and not np.array_equal(whole, alone)


def test_make_table_refuses_odd_sides_on_the_yuv_path():
    aug = _aug()
    p = (0, 0, False, 0.0)
    assert aug.make_table([(0, 37, 53, p)], 8).shape == (1, 12)            # an RGB image may have odd sides
    for (h, w) in ((37, 54), (38, 53)):
        with pytest.raises(ValueError, match="even sides"):
            aug.make_table([(0, h, w, p)], 8, yuv420=True)
    t = aug.make_table([(7, 38, 54, (3, 5, True, 90.0))], 8, yuv420=True)
    assert torch.equal(t, aug.make_table([(7, 38, 54, (3, 5, True, 90.0))], 8))
    with pytest.raises(ValueError, match="outside"):
        aug.make_table([(0, 38, 54, (31, 0, False, 0.0))], 8, yuv420=True)


# ------------------------------------------------------------------------------------------------- frames
def test_select_frames():
    sel = _vf().select_frames
    allf = list(range(7))
    assert sel(7, None, 0) == (allf, allf, [0])
    assert sel(7, None, 1) == (allf, [], allf)
    assert sel(7, None, 3) == (allf, [1, 2, 4, 5], [0, 3, 6])
    assert sel(7, (2, 6), 0) == ([2, 3, 4, 5], [2, 3, 4, 5], [2])
    assert sel(7, (2, 6), 1) == ([2, 3, 4, 5], [], [2, 3, 4, 5])
    assert sel(7, (2, 6), 3) == ([2, 3, 4, 5], [3, 4], [2, 5])
    assert sel(7, (5, None), 3) == ([5, 6], [6], [5])
    assert sel(7, (5, 99), 3) == ([5, 6], [6], [5])
    with pytest.raises(ValueError, match="select nothing"):
        sel(7, (7, 9), 3)
    with pytest.raises(ValueError):
        sel(7, None, -1)


def _write_video(path, n=7, h=38, w=54, depth=8, seed=3, raw=False):
    video = amd("video")
    rng = np.random.RandomState(seed)
    dt, top = (np.uint8, 256) if depth == 8 else (np.uint16, 1024)
    frames = [tuple(rng.randint(0, top, s).astype(dt) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
              for _ in range(n)]
    wr = video.RawYUV420Writer(str(path), w, h, depth) if raw else \
        video.Y4MWriter(str(path), w, h, fps="25:1", chroma="420jpeg" if depth == 8 else "420p10", depth=depth)
    with wr:
        for k, f in enumerate(frames):
            wr.write_frame(*f, params="Ip" if k == 2 and not raw else "")     # a FRAME line with parameters
    return frames


def test_pool_layout_from_headers_alone(tmp_path):
    aug, video = _aug(), amd("video")
    _write_video(tmp_path / "a.y4m")
    _write_video(tmp_path / "b.yuv", n=3, h=16, w=20, raw=True)
    with video.open_reader(str(tmp_path / "a.y4m")) as r:
        assert aug.count_frames(r) == 7 and r.frames_read == 0
        assert r.read_frame() is not None                   # the reader did not move
    with video.open_reader(str(tmp_path / "b.yuv"), (20, 16)) as r:
        assert aug.count_frames(r) == 3
    src = [(str(tmp_path / "a.y4m"), None, [0, 3, 6]), (str(tmp_path / "b.yuv"), (20, 16), [1])]
    entries, paths, total, largest = aug.video_pool_layout(src, 1 << 20)
    fa, fb = 38 * 54 * 3 // 2, 16 * 20 * 3 // 2
    assert entries == [(0, 38, 54), (fa, 38, 54), (2 * fa, 38, 54), (3 * fa, 16, 20)]
    assert total == 3 * fa + fb and largest == fa and paths[1].endswith("a.y4m#3") and paths[3].endswith("b.yuv#1")
    with pytest.raises(MemoryError, match=str(total)):
        aug.video_pool_layout(src, total - 1)
    for bad in ([3, 3], [4, 2], [7], [-1]):
        with pytest.raises(ValueError, match="strictly increasing"):
            aug.video_pool_layout([(str(tmp_path / "a.y4m"), None, bad)], 1 << 20)
    with open(str(tmp_path / "a.y4m"), "r+b") as f:         # a truncated last frame is noticed without reading frames
        f.truncate(f.seek(0, 2) - 5)
    with pytest.raises(ValueError, match="truncated"):
        aug.video_pool_layout(src, 1 << 20)


def test_ten_bit_source_is_refused(tmp_path):
    aug = _aug()
    _write_video(tmp_path / "deep.y4m", n=2, depth=10)
    with pytest.raises(ValueError, match="8-bit only.*Pillow's 8-bit bicubic"):
        aug.video_pool_layout([(str(tmp_path / "deep.y4m"), None, [0])], 1 << 30)
    with pytest.raises(ValueError, match="8-bit only.*Pillow's 8-bit bicubic"):     # before the device is looked at
        aug.ResidentVideoSet([(str(tmp_path / "deep.y4m"), None, [0])], "cpu")


# ------------------------------------------------------------------------------------------------- flags
def test_shared_flag_helper():
    vf = _vf()

    def parse(argv):
        ap = argparse.ArgumentParser()
        ap.add_argument("--path", default="exp")
        vf.add_video_args(ap)
        a = ap.parse_args(argv)
        return a, vf.take_video_args(a)

    a, kw = parse([])
    assert kw is None and a.__dict__ == {"path": "exp"}           # without --video the namespace is what it was
    a, kw = parse(["--video", "a.y4m", "--video", "b.yuv", "--video-size", "54x38", "--video-frames", "2:6",
                   "--video-valid-every", "3", "--matrix", "bt709", "--range", "pc"])
    assert a.__dict__ == {"path": "exp"}
    assert kw == dict(videos=["a.y4m", "b.yuv"], video_size=(54, 38), video_frames=(2, 6), video_valid_every=3,
                      matrix="bt709", full_range=True)
    _, kw = parse(["--video", "a.y4m", "--video-frames", ":4"])
    assert kw == dict(videos=["a.y4m"], video_size=None, video_frames=(0, 4), video_valid_every=10, matrix="bt601",
                      full_range=False)
    assert parse(["--video", "a.y4m", "--video-frames", "3:"])[1]["video_frames"] == (3, None)
    for bad in (["--video-size", "53x38"], ["--video-size", "54"], ["--video-frames", "6:2"], ["--video-frames", "x"],
                ["--matrix", "bt2020"], ["--video-size", "54x38"], ["--video", "a.y4m", "--video-valid-every", "-1"]):
        with pytest.raises(SystemExit):
            parse(bad)


def test_run_config_records_the_videos():
    rm = amd("imagenet_codebase.run_manager")
    cfg = rm.VideoFramesRunConfig(["a.y4m", "b.yuv"], video_size=(54, 38), video_frames=(2, 6), video_valid_every=3,
                                  matrix="bt709", full_range=True, train_batch_size=2, image_size=16, path="x", task="depth")
    assert cfg.dataset == "video_frames: a.y4m, b.yuv" and cfg.config["dataset"] == cfg.dataset
    assert cfg.config["videos"] == ["a.y4m", "b.yuv"] and cfg.config["matrix"] == "bt709" and cfg.image_size == 16
    import json
    json.dumps(cfg.config)
