"""The 10-bit host definition (video.py with depth=10), no GPU: depth 8 is what it was, the tables of depth 10 keep grey
grey and a grey ramp round-trips exactly, words above 1023 read as 1023, int32 suffices on extreme planes, window reuse on
uint16 frames sees a change in either byte of a word, and the Y4M C420p10 / headerless yuv420p10le readers and writers.
Everything is bit-exact."""
import itertools

import numpy as np
import pytest

from conftest import amd

COMBOS = list(itertools.product(["bt601", "bt709"], [False, True]))
H, W = 14, 18
# (y0, x0, h, w): the windows of test_video_reuse.py -- odd origins, odd sizes, a 1x1 window, the whole frame, the far edges
WINDOWS = [(0, 0, 5, 7), (1, 3, 6, 4), (3, 5, 7, 9), (4, 2, 1, 1), (0, 0, 14, 18), (9, 11, 5, 7), (7, 1, 2, 16), (13, 17, 1, 1)]


def _frame10(seed, h=H, w=W, top=1024):
    rng = np.random.RandomState(seed)
    return tuple(rng.randint(0, top, s).astype(np.uint16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


# ---------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("matrix,full", COMBOS)
def test_depth_8_is_the_default_and_unchanged(matrix, full):
    video = amd("video")
    assert video.yuv_coeffs(matrix, full) == video.yuv_coeffs(matrix, full, depth=8)
    for depth in (9, 12, 16, True, None):
        with pytest.raises(ValueError, match="depth"):
            video.yuv_coeffs(matrix, full, depth=depth)


def test_the_tables_depend_on_the_depth():
    video = amd("video")
    assert video.yuv_coeffs("bt601", False, 8)[0].cy == 19077 and video.yuv_coeffs("bt601", False, 10)[0].cy == 19133
    assert video.yuv_coeffs("bt601", False, 10)[0].yo == video.yuv_coeffs("bt601", False, 10)[1].yo == 64
    assert video.yuv_coeffs("bt709", True, 10) == video.yuv_coeffs("bt709", True, 8)       # full range: scales of 1
    biggest = max(abs(c) for m, f in COMBOS for t in video.yuv_coeffs(m, f, 10) for c in t[1:])
    assert biggest == 34711 < 2 ** 16


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_depth_10_keeps_grey_grey(matrix, full):
    video = amd("video")
    _, e = video.yuv_coeffs(matrix, full, 10)
    assert e.ur + e.ug + e.ub == 0 and e.vr + e.vg + e.vb == 0
    lo, hi = (0, 1023) if full else (64, 940)
    ramp = np.arange(lo, hi + 1, dtype=np.uint16)
    ramp = ramp[:len(ramp) // 2 * 2]
    if not full:
        assert ramp[-1] == 939
        ramp = np.concatenate([ramp, np.array([940, 940], np.uint16)])      # the last legal value in a whole block
    y = np.ascontiguousarray(np.stack([ramp, ramp[::-1]]))
    c = np.full((1, y.shape[1] // 2), 512, np.uint16)
    rgb = video.yuv420_to_rgb_host(y, c, c, matrix, full, depth=10)
    assert rgb.dtype == np.uint16 and rgb.shape == y.shape + (3,)
    assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 1], rgb[..., 2])
    assert rgb.min() == 0 and rgb.max() == 1023
    back = video.rgb_to_yuv420_host(rgb, matrix, full, depth=10)
    assert all(p.dtype == np.uint16 for p in back)
    assert np.array_equal(back[0], y) and np.array_equal(back[1], c) and np.array_equal(back[2], c)


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_words_above_1023_read_as_1023(matrix, full):
    video = amd("video")
    y, u, v = _frame10(1, top=65536)
    assert (y > 1023).any() and (u > 1023).any()
    got = video.yuv420_to_rgb_host(y, u, v, matrix, full, depth=10)
    exp = video.yuv420_to_rgb_host(np.minimum(y, 1023), np.minimum(u, 1023), np.minimum(v, 1023), matrix, full, depth=10)
    assert np.array_equal(got, exp) and got.max() <= 1023
    rgb = np.random.RandomState(2).randint(0, 65536, (H, W, 3)).astype(np.uint16)
    for a, b in zip(video.rgb_to_yuv420_host(rgb, matrix, full, depth=10),
                    video.rgb_to_yuv420_host(np.minimum(rgb, 1023), matrix, full, depth=10)):
        assert np.array_equal(a, b) and a.max() <= 1023


def test_dtype_and_depth_must_agree():
    video = amd("video")
    y8 = tuple(p.astype(np.uint8) for p in _frame10(0, top=256))
    with pytest.raises(ValueError):
        video.yuv420_to_rgb_host(*y8, depth=10)
    with pytest.raises(ValueError):
        video.yuv420_to_rgb_host(*_frame10(0))
    with pytest.raises(ValueError):
        video.rgb_to_yuv420_host(np.zeros((2, 2, 3), np.uint8), depth=10)
    with pytest.raises(ValueError):
        video.changed_windows_host(_frame10(0), y8, [(0, 0)], 2, 2, depth=10)


# ---------------------------------------------------------------------------------------------- int32 suffices
def _decode64(y, u, v, d, maxv, mid):
    """the decode written out again, every step in int64"""
    Hh, Ww = y.shape
    y, u, v = (np.minimum(p, maxv).astype(np.int64) for p in (y, u, v))

    def up(c):
        out = np.zeros((Hh, Ww), np.int64)
        for r in range(Hh):
            r0 = r >> 1
            nr = min(max(r0 - 1 if r % 2 == 0 else r0 + 1, 0), Hh // 2 - 1)
            for x in range(Ww):
                x0 = x >> 1
                nx = min(max(x0 - 1 if x % 2 == 0 else x0 + 1, 0), Ww // 2 - 1)
                out[r, x] = (9 * c[r0, x0] + 3 * c[r0, nx] + 3 * c[nr, x0] + c[nr, nx] + 8) >> 4
        return out

    yy, uu, vv = y - d.yo, up(u) - mid, up(v) - mid
    r = (d.cy * yy + d.rv * vv + 8192) >> 14
    g = (d.cy * yy + d.gu * uu + d.gv * vv + 8192) >> 14
    b = (d.cy * yy + d.bu * uu + 8192) >> 14
    sums = [d.cy * yy, d.rv * vv, d.gu * uu + d.gv * vv, d.bu * uu]
    return np.clip(np.stack([r, g, b], axis=2), 0, maxv), max(int(np.abs(t).max()) for t in sums + [r << 14, g << 14, b << 14])


def _encode64(rgb, e, maxv, mid):
    p = np.minimum(rgb, maxv).astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    Hh, Ww = r.shape
    y = np.clip(((e.yr * r + e.yg * g + e.yb * b + 8192) >> 14) + e.yo, 0, maxv)
    planes, big = [y], int(np.abs(e.yr * r + e.yg * g + e.yb * b).max())
    for cr, cg, cb in ((e.ur, e.ug, e.ub), (e.vr, e.vg, e.vb)):
        s = (cr * r + cg * g + cb * b).reshape(Hh // 2, 2, Ww // 2, 2).sum(axis=(1, 3))
        big = max(big, int(np.abs(s).max()) + (1 << 15))
        planes.append(np.clip(((s + (1 << 15)) >> 16) + mid, 0, maxv))
    return planes, big


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_int32_and_int64_agree_on_extreme_planes(matrix, full):
    video = amd("video")
    d, e = video.yuv_coeffs(matrix, full, 10)
    Hh, Ww = 6, 8
    full_y, half = (Hh, Ww), (Hh // 2, Ww // 2)
    board = lambda s, a, b: np.where(np.add.outer(np.arange(s[0]), np.arange(s[1])) % 2 == 0, a, b).astype(np.uint16)  # noqa: E731
    planes = [tuple(np.full(s, c, np.uint16) for s in (full_y, half, half)) for c in (0, 1023)]
    planes += [(np.full(full_y, a, np.uint16), np.full(half, b, np.uint16), np.full(half, c, np.uint16))
               for a, b, c in ((0, 1023, 1023), (1023, 0, 0), (1023, 0, 1023), (0, 1023, 0), (1023, 1023, 0))]
    planes += [(board(full_y, 0, 1023), board(half, 1023, 0), board(half, 0, 1023)),
               (board(full_y, 1023, 0), board(half, 0, 1023), board(half, 0, 1023))]
    biggest = 0
    for y, u, v in planes:
        exp, big = _decode64(y, u, v, d, 1023, 512)
        biggest = max(biggest, big)
        assert np.array_equal(video.yuv420_to_rgb_host(y, u, v, matrix, full, depth=10), exp)
    images = [np.full((Hh, Ww, 3), c, np.uint16) for c in (0, 1023)]
    images += [np.broadcast_to(np.array(c, np.uint16), (Hh, Ww, 3)).copy()
               for c in itertools.product((0, 1023), repeat=3)]
    images.append(np.stack([board(full_y, 0, 1023), board(full_y, 1023, 0), board(full_y, 0, 1023)], axis=2))
    for rgb in images:
        exp, big = _encode64(rgb, e, 1023, 512)
        biggest = max(biggest, big)
        for a, b in zip(video.rgb_to_yuv420_host(rgb, matrix, full, depth=10), exp):
            assert np.array_equal(a, b)
    assert biggest < 6.8e7 < 2 ** 31


# ---------------------------------------------------------------------------------------------- window reuse
def test_changed_windows_on_uint16_frames():
    video = amd("video")
    base = _frame10(0)
    rgb0 = video.yuv420_to_rgb_host(*base, depth=10)
    cases = tight = 0
    for plane in range(3):
        for r in range(base[plane].shape[0]):
            for c in range(base[plane].shape[1]):
                cur = [p.copy() for p in base]
                cur[plane][r, c] ^= 0x200
                rgb1 = video.yuv420_to_rgb_host(*cur, depth=10)
                for (y0, x0, h, w) in WINDOWS:
                    flag = bool(video.changed_windows_host(base, cur, [(y0, x0)], h, w, depth=10)[0])
                    (r0, r1, c0, c1), (s0, s1, d0, d1) = video.window_support(y0, x0, h, w, H, W, depth=10)
                    inside = (r0 <= r <= r1 and c0 <= c <= c1) if plane == 0 else (s0 <= r <= s1 and d0 <= c <= d1)
                    assert flag == inside, (plane, r, c, y0, x0, h, w)
                    same = np.array_equal(rgb0[y0:y0 + h, x0:x0 + w], rgb1[y0:y0 + h, x0:x0 + w])
                    if not flag:
                        assert same, (plane, r, c, y0, x0, h, w)
                    else:
                        tight += not same
                cases += 1
    assert cases == 14 * 18 + 2 * 7 * 9 == 378
    assert tight > 0
    assert video.window_support(1, 3, 6, 4, H, W, depth=10) == video.window_support(1, 3, 6, 4, H, W)


@pytest.mark.parametrize("bit", [0x0001, 0x0080, 0x0100, 0x8000], ids=hex)
def test_a_change_in_either_byte_of_a_word_is_seen(bit):
    """the raw words are compared: the low byte alone, the high byte alone, and a bit that the decode does not even read"""
    video = amd("video")
    base = _frame10(3)
    origins = [(0, 0), (1, 3), (9, 11), (4, 2)]
    for plane, (r, c) in ((0, (2, 4)), (1, (1, 2)), (2, (1, 2))):
        cur = [p.copy() for p in base]
        cur[plane][r, c] ^= bit
        assert (cur[plane][r, c] ^ base[plane][r, c]) == bit
        flags = video.changed_windows_host(base, cur, origins, 5, 7, depth=10).tolist()
        assert flags == [True, True, False, plane != 0], (plane, flags)      # (4, 2): luma rows 4 .. 8, chroma rows 1 .. 4
    assert not video.changed_windows_host(base, [p.copy() for p in base], origins, 5, 7, depth=10).any()


# ---------------------------------------------------------------------------------------------- files
def _frames10(n, w, h, seed=0):
    return [_frame10(seed + i, h, w) for i in range(n)]


def test_frame_bytes_and_split_frame():
    video = amd("video")
    assert video.frame_bytes(6, 4) == video.frame_bytes(6, 4, 8) == 36 and video.frame_bytes(6, 4, 10) == 3 * 6 * 4
    with pytest.raises(ValueError):
        video.frame_bytes(6, 4, 12)
    buf = np.arange(72, dtype=np.uint8)
    y, u, v = video.split_frame(buf, 6, 4, 10)
    assert (y.dtype, y.shape, u.shape, v.shape) == (np.uint16, (4, 6), (2, 3), (2, 3))
    assert y[0, 0] == 0x0100 and y[0, 1] == 0x0302 and u[0, 0] == 0x3130 and v[1, 2] == 0x4746     # little-endian words
    y[0, 0] = 0x0201
    assert buf[0] == 1 and buf[1] == 2                                                              # views, not copies
    y8, _, _ = video.split_frame(buf[:36], 6, 4)
    assert y8.dtype == np.uint8 and y8.shape == (4, 6)


def test_y4m_p10_round_trip(tmp_path):
    video = amd("video")
    w, h = 6, 4
    frames = _frames10(3, w, h)
    p = str(tmp_path / "a.y4m")
    with video.Y4MWriter(p, w, h, fps="30000:1001", interlace="p", aspect="1:1", chroma="420p10", xtags=["YSCSS=420P10"],
                         depth=10) as wr:
        for i, fr in enumerate(frames):
            wr.write_frame(*fr, params="Ip" if i == 1 else "")
    raw = open(p, "rb").read()
    assert raw.startswith(b"YUV4MPEG2 W6 H4 F30000:1001 Ip A1:1 C420p10 XYSCSS=420P10\nFRAME\n")
    assert len(raw) == raw.index(b"\n") + 1 + 3 * video.frame_bytes(w, h, 10) + 2 * len(b"FRAME\n") + len(b"FRAME Ip\n")
    first = raw[raw.index(b"FRAME\n") + 6:][:72]
    assert first == b"".join(p_.astype("<u2").tobytes() for p_ in frames[0])
    with video.Y4MReader(p, depths=(8, 10)) as rd:
        assert (rd.width, rd.height, rd.depth, rd.chroma, rd.fps, rd.interlace, rd.aspect, rd.xtags) == \
            (w, h, 10, "420p10", "30000:1001", "p", "1:1", ["YSCSS=420P10"])
        got, params = [], []
        for fr in rd:
            got.append(tuple(p_.copy() for p_ in fr))
            params.append(rd.frame_params)
    assert params == ["", "Ip", ""] and len(got) == 3
    for a, b in zip(got, frames):
        assert all(x.dtype == np.uint16 and np.array_equal(x, y) for x, y in zip(a, b))
    # into the caller's byte buffer: uint16 views of it
    buf = np.zeros(video.frame_bytes(w, h, 10), np.uint8)
    with video.Y4MReader(p, depths=(10,)) as rd:
        y, u, v = rd.read_frame(buf)
        assert y.dtype == np.uint16 and np.shares_memory(y, buf) and np.shares_memory(v, buf)
        assert np.array_equal(y, frames[0][0]) and np.array_equal(v, frames[0][2])
        assert rd.skip_frame() and rd.skip_frame() and not rd.skip_frame()
    with video.Y4MReader(p, depths=(10,)) as rd:
        with pytest.raises(ValueError, match="%d bytes" % (3 * w * h)):
            rd.read_frame(np.zeros(video.frame_bytes(w, h), np.uint8))     # a buffer of the 8-bit size
    with video.open_reader(p) as rd:
        assert isinstance(rd, video.Y4MReader) and rd.depth == 10
        assert np.array_equal(rd.read_frame()[1], frames[0][1])
    with video.open_reader(p, depth=10) as rd:
        assert rd.depth == 10
    # opt-in only, and a contradiction is an error
    with pytest.raises(ValueError, match="C420p10"):
        video.Y4MReader(p)
    with pytest.raises(ValueError, match="C420p10"):
        video.open_reader(p, depth=8)
    p8 = str(tmp_path / "b.y4m")
    with video.Y4MWriter(p8, w, h) as wr:
        wr.write_frame(*(p_.astype(np.uint8) for p_ in frames[0]))
    with pytest.raises(ValueError, match="C420jpeg"):
        video.open_reader(p8, depth=10)
    with video.open_reader(p8) as rd:
        assert rd.depth == 8 and rd.read_frame()[0].dtype == np.uint8


def test_headerless_p10_round_trip(tmp_path):
    video = amd("video")
    w, h = 6, 4
    frames = _frames10(2, w, h, 5)
    p = str(tmp_path / "a.yuv")
    with video.RawYUV420Writer(p, w, h, 10) as wr:
        for fr in frames:
            wr.write_frame(*fr)
    assert open(p, "rb").read() == b"".join(p_.astype("<u2").tobytes() for fr in frames for p_ in fr)
    with video.RawYUV420Reader(p, w, h, depth=10) as rd:
        assert rd.frames == 2 and rd.depth == 10
        got = [tuple(p_.copy() for p_ in fr) for fr in rd]
    for a, b in zip(got, frames):
        assert all(x.dtype == np.uint16 and np.array_equal(x, y) for x, y in zip(a, b))
    with video.open_reader(p, (w, h), 10) as rd:
        assert rd.skip_frame() and np.array_equal(rd.read_frame()[2], frames[1][2]) and rd.read_frame() is None
    # the same bytes are four 8-bit frames: the depth is the caller's to say
    with video.open_reader(p, (w, h)) as rd:
        assert rd.depth == 8 and rd.frames == 4


def test_truncated_last_frame_is_refused_at_depth_10(tmp_path):
    video = amd("video")
    w, h = 6, 4
    n = video.frame_bytes(w, h, 10)
    assert n == 72
    fr = _frames10(1, w, h, 7)[0]
    payload = b"".join(p_.tobytes() for p_ in fr)
    p = str(tmp_path / "t.y4m")
    open(p, "wb").write(b"YUV4MPEG2 W6 H4 C420p10\nFRAME\n" + payload + b"FRAME\n" + payload[:-1])
    with video.open_reader(p) as rd:
        assert rd.read_frame() is not None
        with pytest.raises(ValueError, match=r"frame 1 is truncated \(71 of 72 bytes\)"):
            rd.read_frame()
    raw = str(tmp_path / "t.yuv")
    open(raw, "wb").write(payload + payload[:36])       # one and a half 10-bit frames (three 8-bit ones)
    with pytest.raises(ValueError, match="108 bytes is not a whole number of 6x4 yuv420p10le frames \\(72 bytes each\\)"):
        video.RawYUV420Reader(raw, w, h, depth=10)


def test_writers_refuse_a_tag_or_planes_that_disagree_with_the_depth(tmp_path):
    video = amd("video")
    p = str(tmp_path / "w.y4m")
    with pytest.raises(ValueError, match="420p10"):
        video.Y4MWriter(p, 6, 4, chroma="420p10", depth=8)
    with pytest.raises(ValueError, match="420jpeg"):
        video.Y4MWriter(p, 6, 4, chroma="420jpeg", depth=10)
    with pytest.raises(ValueError, match="depth"):
        video.Y4MWriter(p, 6, 4, chroma="420p10", depth=12)
    fr = _frames10(1, 6, 4)[0]
    with video.Y4MWriter(p, 6, 4, chroma="420p10", depth=10) as wr:
        with pytest.raises(ValueError, match="uint16"):
            wr.write_frame(*(q.astype(np.uint8) for q in fr))
        wr.write_frame(*fr)
    with video.Y4MWriter(p, 6, 4) as wr:
        with pytest.raises(ValueError, match="uint8"):
            wr.write_frame(*fr)
