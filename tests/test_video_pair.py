"""Host side of training on paired video -- a decoded low-resolution stream and its source (data_providers/augment.py:
draw_pair_params, apply_pair_params_np, make_pair_table, gather_yuv420_pair_np, video_pair_layout;
data_providers/video_frames.py: --video-lr / --video-lr-size / --video-no-rotate).  The byte-level definition of
ofasr_aug_gather_yuv420_pair against the transforms applied to video.yuv420_to_rgb_host of the two whole frames."""
import argparse

import numpy as np
import pytest
import torch

from conftest import amd

FIXED_ANGLES = [0.0, 90.0, -90.0, 180.0, 45.0, -33.3, 1e-9]
COMBOS = [("bt601", False), ("bt709", True)]
# f -> the ((H, W), (h, w)) pairs pooled for it
PAIRS = {2: [((40, 56), (20, 28))], 4: [((64, 64), (16, 16)), ((48, 96), (12, 24))]}
SIZES = [(30, 2), (32, 2), (8, 4), (24, 4), (32, 4)]


def _aug():
    return amd("imagenet_codebase.data_providers.augment")


def _vf():
    return amd("imagenet_codebase.data_providers.video_frames")


def _noise_frame(rng, h, w):
    return tuple(rng.randint(0, 256, s).astype(np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def _pool(frames):
    host = np.concatenate([p.reshape(-1) for f in frames for p in f])
    offs = [int(o) for o in np.cumsum([0] + [f[0].size * 3 // 2 for f in frames])[:-1]]
    return offs, host


def make_pair_pools(f, seed=11):
    """per pair of PAIRS[f] one HR and one LR frame of noise over the whole byte range, and the two pools that hold
    them back to back as two yuv420p files would: {'hr', 'lr': frames, 'hr_offs', 'lr_offs', 'hr_host', 'lr_host'}"""
    rng = np.random.RandomState(seed + f)
    hr = [_noise_frame(rng, *hw) for hw, _ in PAIRS[f]]
    lr = [_noise_frame(rng, *hw) for _, hw in PAIRS[f]]
    (ho, hh), (lo, lh) = _pool(hr), _pool(lr)
    return {"hr": hr, "lr": lr, "hr_offs": ho, "lr_offs": lo, "hr_host": hh, "lr_host": lh}


def pair_cases(S, f, seed):
    """(pair index, LR-grid (i, j, flip, angle)): LR corners at the four frame corners and one odd interior corner of
    every pair, flip on and off, FIXED_ANGLES and ten drawn angles (as test_video_train.cases draws them)"""
    s = S // f
    g = torch.Generator().manual_seed(seed)
    angles = FIXED_ANGLES + [float(torch.empty(1).uniform_(-90, 90, generator=g).item()) for _ in range(10)]
    out = []
    for k, (_, (h, w)) in enumerate(PAIRS[f]):
        inner = (((h - s) // 2) | 1, ((w - s) // 3) | 1)
        assert 0 < inner[0] <= h - s and 0 < inner[1] <= w - s
        for (i, j) in [(0, 0), (0, w - s), (h - s, 0), (h - s, w - s), inner]:
            for flip in (False, True):
                for a in angles:
                    out.append((k, (i, j, flip, a)))
    return out


def pair_rows(pools, f, cs):
    return [(pools["hr_offs"][k],) + PAIRS[f][k][0] + (pools["lr_offs"][k],) + PAIRS[f][k][1] + (p,) for k, p in cs]


@pytest.mark.parametrize("matrix,full", COMBOS)
@pytest.mark.parametrize("S,f", SIZES)
def test_gather_pair_np_equals_transforms_of_the_decoded_frames(S, f, matrix, full):
    aug, video = _aug(), amd("video")
    pools = make_pair_pools(f)
    cs = pair_cases(S, f, 200 + S + f)
    table = aug.make_pair_table(pair_rows(pools, f, cs), S, f)
    assert tuple(table.shape) == (2, len(cs), 12) and table.dtype == torch.int64
    hr, lr = aug.gather_yuv420_pair_np(pools["hr_host"], pools["lr_host"], table.numpy(), S, f,
                                       video.yuv_coeffs(matrix, full)[0])
    s = S // f
    assert hr.shape == (len(cs), 3, S, S) and lr.shape == (len(cs), 3, s, s) and hr.dtype == lr.dtype == np.uint8
    hr_rgb = [video.yuv420_to_rgb_host(*fr, matrix=matrix, full_range=full) for fr in pools["hr"]]
    lr_rgb = [video.yuv420_to_rgb_host(*fr, matrix=matrix, full_range=full) for fr in pools["lr"]]
    for n, (k, p) in enumerate(cs):
        i, j, flip, angle = p
        ref_h = aug.apply_params_np(hr_rgb[k], S, (f * i, f * j, flip, angle)).transpose(2, 0, 1)
        ref_l = aug.apply_params_np(lr_rgb[k], s, p).transpose(2, 0, 1)
        assert np.array_equal(hr[n], ref_h), "HR S=%d f=%d pair %d params %r" % (S, f, k, p)
        assert np.array_equal(lr[n], ref_l), "LR S=%d f=%d pair %d params %r" % (S, f, k, p)
    for n in (0, len(cs) // 2, len(cs) - 1):
        k, p = cs[n]
        a, b = aug.apply_pair_params_np(pools["hr"][k], pools["lr"][k], S, f, p, matrix=matrix, full_range=full)
        assert np.array_equal(a, hr[n].transpose(1, 2, 0)) and np.array_equal(b, lr[n].transpose(1, 2, 0))
    # the two blocks are the sibling's tables, each with its own side's rotation
    k, p = cs[-1]
    assert tuple(table[0, -1, 6:].tolist()) == aug.rotate_coeffs(p[3], S)
    assert tuple(table[1, -1, 6:].tolist()) == aug.rotate_coeffs(p[3], s)
    assert table[0, -1, :6].tolist() == [pools["hr_offs"][k], PAIRS[f][k][0][0], PAIRS[f][k][0][1], f * p[0], f * p[1], int(p[2])]
    assert table[1, -1, :6].tolist() == [pools["lr_offs"][k], PAIRS[f][k][1][0], PAIRS[f][k][1][1], p[0], p[1], int(p[2])]


@pytest.mark.parametrize("S,f", SIZES)
def test_registration_at_angle_zero(S, f):
    """an LR frame that is the HR luma subsampled, with grey chroma on both sides, gives LR == HR[::f, ::f] at angle 0 for
    every corner: grey chroma decodes to R = G = B = g(Y), so the identity is exact.  Flipped, the two crops still cover
    the same area and the identity holds between the mirror images: the LR sample of an f x f block is its LEFT column
    in the frame, which the flip puts at the block's right, so LR == HR[::f, f-1::f] there"""
    aug = _aug()
    s = S // f
    rng = np.random.RandomState(S * 10 + f)
    for (H, W), (h, w) in PAIRS[f]:
        y = rng.randint(0, 256, (H, W)).astype(np.uint8)
        hr = (y, np.full((H // 2, W // 2), 128, np.uint8), np.full((H // 2, W // 2), 128, np.uint8))
        lr = (np.ascontiguousarray(y[::f, ::f]), np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8))
        for (i, j) in [(0, 0), (0, w - s), (h - s, 0), (h - s, w - s), ((h - s) // 2, (w - s) // 2)]:
            for flip in (False, True):
                a, b = aug.apply_pair_params_np(hr, lr, S, f, (i, j, flip, 0.0))
                assert a.shape == (S, S, 3) and b.shape == (s, s, 3)
                assert np.array_equal(b, a[::f, (f - 1 if flip else 0)::f]), ((H, W), (i, j), flip)
                assert np.array_equal(b[:, ::-1] if flip else b, (a[:, ::-1] if flip else a)[::f, ::f])
                assert np.array_equal(a[:, :, 0], a[:, :, 1]) and np.array_equal(a[:, :, 0], a[:, :, 2])


@pytest.mark.parametrize("h,w,S,f", [(20, 28, 16, 2), (16, 16, 32, 4), (16, 16, 64, 4), (12, 24, 8, 4), (270, 480, 256, 4)])
def test_draw_pair_params_draws_as_the_unpaired_path_on_the_lr_grid(h, w, S, f):
    aug = _aug()
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        want = [aug.draw_train_params(h, w, S // f) for _ in range(3)]
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        got = [aug.draw_pair_params(h, w, S, f) for _ in range(3)]
        assert got == want and torch.equal(torch.get_rng_state(), state)
        torch.manual_seed(seed)
        flat = [aug.draw_pair_params(h, w, S, f, rotate=False) for _ in range(3)]
        assert torch.equal(torch.get_rng_state(), state)                # the angle is drawn all the same
        assert [p[:3] for p in flat] == [p[:3] for p in want] and all(p[3] == 0.0 for p in flat)
        assert any(p[3] != 0.0 for p in want)
        assert all(aug.pair_hr_params(p, f) == (f * p[0], f * p[1], p[2], p[3]) for p in want)


def test_draw_and_table_refusals():
    aug = _aug()
    p = (0, 0, False, 0.0)
    with pytest.raises(ValueError, match="scale 2 or 4"):
        aug.draw_pair_params(16, 16, 24, 3)
    with pytest.raises(ValueError, match="multiple of its scale"):
        aug.draw_pair_params(16, 16, 30, 4)
    with pytest.raises(ValueError, match="larger than input image size"):
        aug.draw_pair_params(16, 16, 68, 4)
    row = (0, 64, 64, 0, 16, 16, p)
    assert tuple(aug.make_pair_table([row], 32, 4).shape) == (2, 1, 12)
    with pytest.raises(ValueError, match="scale 2 or 4"):
        aug.make_pair_table([row], 32, 1)
    with pytest.raises(ValueError, match="multiple of its scale"):
        aug.make_pair_table([row], 30, 4)
    with pytest.raises(ValueError, match="64x64 is not 2 times its LR frame of 16x16"):
        aug.make_pair_table([row], 32, 2)
    with pytest.raises(ValueError, match="is not 4 times"):
        aug.make_pair_table([(0, 64, 64, 0, 16, 18, p)], 32, 4)
    # table_row's refusals, on either side
    with pytest.raises(ValueError, match="smaller than"):
        aug.make_pair_table([row], 68, 4)
    with pytest.raises(ValueError, match="outside"):
        aug.make_pair_table([(0, 64, 64, 0, 16, 16, (9, 0, False, 0.0))], 32, 4)
    with pytest.raises(ValueError, match="outside"):
        aug.make_pair_table([(0, 64, 64, 0, 16, 16, (0, -1, False, 0.0))], 32, 4)
    with pytest.raises(ValueError, match="even sides"):
        aug.make_pair_table([(0, 60, 60, 0, 15, 15, p)], 8, 4)
    with pytest.raises(ValueError, match=r"\[2, n, 12\]"):
        aug.gather_yuv420_pair_np(np.zeros(64 * 96, np.uint8), np.zeros(16 * 24, np.uint8), np.zeros((1, 12), np.int64), 32, 4,
                                  amd("video").yuv_coeffs("bt601", False)[0])
    # built in a caller's buffer: the first 2n rows, viewed as two blocks
    buf = torch.full((6, 12), -1, dtype=torch.int64)
    t = aug.make_pair_table([row, (5, 64, 64, 7, 16, 16, (1, 3, True, 30.0))], 32, 4, out=buf)
    assert tuple(t.shape) == (2, 2, 12) and t.data_ptr() == buf.data_ptr() and t.is_contiguous()
    assert torch.equal(t, aug.make_pair_table([row, (5, 64, 64, 7, 16, 16, (1, 3, True, 30.0))], 32, 4))
    assert bool((buf[4:] == -1).all())


# ------------------------------------------------------------------------------------------------- files
def write_video(path, n, h, w, depth=8, seed=3, raw=False):
    video = amd("video")
    rng = np.random.RandomState(seed)
    dt, top = (np.uint8, 256) if depth == 8 else (np.uint16, 1024)
    frames = [tuple(rng.randint(0, top, s).astype(dt) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
              for _ in range(n)]
    wr = video.RawYUV420Writer(str(path), w, h, depth) if raw else \
        video.Y4MWriter(str(path), w, h, fps="25:1", chroma="420jpeg" if depth == 8 else "420p10", depth=depth)
    with wr:
        for f in frames:
            wr.write_frame(*f)
    return frames


def test_pair_layout_and_its_refusals(tmp_path):
    aug = _aug()
    P = lambda name: str(tmp_path / name)
    write_video(P("hr.y4m"), 6, 64, 96)
    write_video(P("lr4.y4m"), 6, 16, 24)
    write_video(P("lr2.yuv"), 6, 32, 48, raw=True)
    write_video(P("hr2.y4m"), 3, 40, 56)
    write_video(P("lr2b.y4m"), 3, 20, 28)
    idx = [0, 2, 5]
    f, hl, ll = aug.video_pair_layout([(P("hr.y4m"), None, idx)], [(P("lr4.y4m"), None, idx)], 1 << 20)
    fh, fl = 64 * 96 * 3 // 2, 16 * 24 * 3 // 2
    assert f == 4 and hl[0] == [(0, 64, 96), (fh, 64, 96), (2 * fh, 64, 96)] and ll[0] == [(0, 16, 24), (fl, 16, 24), (2 * fl, 16, 24)]
    assert hl[2] == 3 * fh and ll[2] == 3 * fl and ll[2] * 16 == hl[2]            # a x4 LR pool adds 1/16
    assert hl[1][1].endswith("hr.y4m#2") and ll[1][1].endswith("lr4.y4m#2")
    f, _, _ = aug.video_pair_layout([(P("hr.y4m"), None, idx), (P("hr2.y4m"), None, [1])],
                                    [(P("lr2.yuv"), (48, 32), idx), (P("lr2b.y4m"), None, [1])], 1 << 20)
    assert f == 2
    # both pools count against max_bytes
    aug.video_pair_layout([(P("hr.y4m"), None, idx)], [(P("lr4.y4m"), None, idx)], 3 * (fh + fl))
    with pytest.raises(MemoryError, match=str(3 * (fh + fl))):
        aug.video_pair_layout([(P("hr.y4m"), None, idx)], [(P("lr4.y4m"), None, idx)], 3 * (fh + fl) - 1)

    def refused(hr, lr, match):
        with pytest.raises(ValueError, match=match) as e:
            aug.video_pair_layout(hr, lr, 1 << 20)
        return str(e.value)

    # sides that are no exact x2 / x4: the message names the files and the sizes
    write_video(P("lr3.y4m"), 6, 22, 32)
    msg = refused([(P("hr.y4m"), None, idx)], [(P("lr3.y4m"), None, idx)], "exactly 2 or 4 times")
    assert "hr.y4m (96x64)" in msg and "lr3.y4m (32x22)" in msg
    write_video(P("lr4w.y4m"), 6, 16, 26)
    refused([(P("hr.y4m"), None, idx)], [(P("lr4w.y4m"), None, idx)], "exactly 2 or 4 times")
    write_video(P("lr8.y4m"), 6, 8, 12)
    refused([(P("hr.y4m"), None, idx)], [(P("lr8.y4m"), None, idx)], "exactly 2 or 4 times")
    refused([(P("hr.y4m"), None, idx)], [(P("hr.y4m"), None, idx)], "exactly 2 or 4 times")
    # mixed scales in one run
    msg = refused([(P("hr.y4m"), None, idx), (P("hr2.y4m"), None, [1])],
                  [(P("lr4.y4m"), None, idx), (P("lr2b.y4m"), None, [1])], "one run has one scale")
    assert "hr2.y4m (56x40)" in msg and "lr2b.y4m (28x20)" in msg and "hr.y4m (96x64)" in msg
    # different frame counts
    write_video(P("lr4short.y4m"), 5, 16, 24)
    msg = refused([(P("hr.y4m"), None, idx[:2])], [(P("lr4short.y4m"), None, idx[:2])], "6 frames against 5")
    assert "hr.y4m (96x64)" in msg and "lr4short.y4m (24x16)" in msg
    # a 10-bit file on either side
    write_video(P("hr10.y4m"), 6, 64, 96, depth=10)
    write_video(P("lr10.y4m"), 6, 16, 24, depth=10)
    refused([(P("hr10.y4m"), None, idx)], [(P("lr4.y4m"), None, idx)], "hr10.y4m is 10-bit.*8-bit only on both sides")
    refused([(P("hr.y4m"), None, idx)], [(P("lr10.y4m"), None, idx)], "lr10.y4m is 10-bit.*8-bit only on both sides")
    # the number of LR videos
    msg = refused([(P("hr.y4m"), None, idx), (P("hr2.y4m"), None, [1])], [(P("lr4.y4m"), None, idx)],
                  "1 LR videos .* for 2 HR videos")
    assert "lr4.y4m" in msg and "hr2.y4m" in msg
    refused([(P("hr.y4m"), None, idx)], [(P("lr4.y4m"), None, [0, 2, 4])], "different frame indices")
    # the set checks what the files are before it looks at the device
    with pytest.raises(ValueError, match="exactly 2 or 4 times"):
        aug.ResidentVideoPairSet([(P("hr.y4m"), None, idx)], [(P("lr3.y4m"), None, idx)], "cpu")
    with pytest.raises(amd("_C").OfasrError, match="on the GPU"):
        aug.ResidentVideoPairSet([(P("hr.y4m"), None, idx)], [(P("lr4.y4m"), None, idx)], "cpu")


# ------------------------------------------------------------------------------------------------- flags
def test_pair_flags_round_trip():
    vf = _vf()

    def parse(argv):
        ap = argparse.ArgumentParser()
        ap.add_argument("--path", default="exp")
        vf.add_video_args(ap)
        a = ap.parse_args(argv)
        return a, vf.take_video_args(a)

    base = dict(videos=["a.y4m"], video_size=None, video_frames=None, video_valid_every=10, matrix="bt601", full_range=False)
    a, kw = parse([])
    assert kw is None and a.__dict__ == {"path": "exp"}
    a, kw = parse(["--video", "a.y4m"])                          # without --video-lr: what it was before the flags existed
    assert a.__dict__ == {"path": "exp"} and kw == base
    a, kw = parse(["--video", "a.y4m", "--video-lr", "a_lr.y4m"])
    assert a.__dict__ == {"path": "exp"}
    assert kw == dict(base, videos_lr=["a_lr.y4m"], video_lr_size=None, video_rotate=True)
    a, kw = parse(["--video", "a.yuv", "--video-size", "96x64", "--video", "b.yuv", "--video-lr", "a_lr.yuv", "--video-lr",
                   "b_lr.yuv", "--video-lr-size", "24x16", "--video-no-rotate", "--video-frames", "2:6", "--matrix", "bt709",
                   "--range", "pc", "--video-valid-every", "3"])
    assert kw == dict(videos=["a.yuv", "b.yuv"], video_size=(96, 64), video_frames=(2, 6), video_valid_every=3,
                      matrix="bt709", full_range=True, videos_lr=["a_lr.yuv", "b_lr.yuv"], video_lr_size=(24, 16),
                      video_rotate=False)
    for bad in (["--video-lr", "a_lr.y4m"], ["--video", "a.y4m", "--video-no-rotate"],
                ["--video", "a.y4m", "--video-lr-size", "24x16"], ["--video-no-rotate"],
                ["--video", "a.y4m", "--video", "b.y4m", "--video-lr", "a_lr.y4m"],
                ["--video", "a.y4m", "--video-lr", "a_lr.y4m", "--video-lr", "b_lr.y4m"],
                ["--video", "a.y4m", "--video-lr", "a_lr.y4m", "--video-lr-size", "23x16"]):
        with pytest.raises(SystemExit):
            parse(bad)
    with pytest.raises(SystemExit, match="1 --video-lr .a_lr.y4m. for 2 --video .a.y4m, b.y4m."):
        parse(["--video", "a.y4m", "--video", "b.y4m", "--video-lr", "a_lr.y4m"])
    # a network whose input is the HR image has no LR input to replace
    kw = parse(["--video", "a.y4m", "--video-lr", "a_lr.y4m"])[1]
    with pytest.raises(SystemExit, match="--video-lr"):
        vf.refuse_pair_for_hr_input(kw, "image", "--net x4")
    vf.refuse_pair_for_hr_input(kw, "4x_down_image", "--net s4")
    vf.refuse_pair_for_hr_input(base, "image", "--net x4")
    vf.refuse_pair_for_hr_input(None, "image", "--net x4")


def test_run_config_records_both_files():
    rm = amd("imagenet_codebase.run_manager")
    kw = dict(train_batch_size=2, image_size=16, path="x", task="depth")
    plain = rm.VideoFramesRunConfig(["a.y4m", "b.yuv"], **kw)
    assert plain.dataset == "video_frames: a.y4m, b.yuv"
    assert not {"videos_lr", "video_lr_size", "video_rotate"} & set(plain.config)        # unchanged without LR files
    cfg = rm.VideoFramesRunConfig(["a.y4m", "b.yuv"], videos_lr=["a_lr.y4m", "b_lr.yuv"], video_lr_size=(24, 16),
                                  video_rotate=False, **kw)
    assert cfg.dataset == "video_frames: a.y4m (lr: a_lr.y4m), b.yuv (lr: b_lr.yuv)" and cfg.config["dataset"] == cfg.dataset
    assert cfg.config["videos_lr"] == ["a_lr.y4m", "b_lr.yuv"] and cfg.config["video_lr_size"] == (24, 16)
    assert cfg.config["video_rotate"] is False
    import json
    json.dumps(cfg.config)
    with pytest.raises(ValueError, match="matched by position"):
        rm.VideoFramesRunConfig(["a.y4m", "b.yuv"], videos_lr=["a_lr.y4m"], **kw)
    with pytest.raises(ValueError, match="paired video"):
        rm.VideoFramesRunConfig(["a.y4m"], video_rotate=False, **kw)
