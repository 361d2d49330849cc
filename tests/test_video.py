"""The video front end on the CPU: the pinned integer YUV 4:2:0 <-> RGB definition (video.py: coefficient tables, the
properties that make it a usable definition, one frame worked out by hand), the Y4M / raw yuv420p readers and writers and
their refusals, and the evenness of the tile plan's output rectangles that the fused scatter relies on."""
import itertools

import numpy as np
import pytest

from conftest import amd

COMBOS = list(itertools.product(["bt601", "bt709"], [False, True]))


def video():
    return amd("video")


# ---------------------------------------------------------------------------------------------- coefficients
def test_coefficient_tables_pinned():
    v = video()
    d, e = v.yuv_coeffs("bt601", False)
    assert tuple(d) == (16, 19077, 26149, -6419, -13320, 33050)
    assert tuple(e) == (16, 4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170)
    d, e = v.yuv_coeffs("bt709", False)
    assert tuple(d) == (16, 19077, 29372, -3494, -8731, 34610)
    assert tuple(e) == (16, 2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660)
    assert v.yuv_coeffs() == v.yuv_coeffs("bt601", False)
    with pytest.raises(ValueError):
        v.yuv_coeffs("bt2020", False)


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_chroma_rows_sum_to_zero(matrix, full):
    d, e = video().yuv_coeffs(matrix, full)
    assert e.ur + e.ug + e.ub == 0 and e.vr + e.vg + e.vb == 0
    assert d.yo == e.yo == (0 if full else 16)
    assert all(isinstance(c, int) for c in tuple(d) + tuple(e))
    if full:
        assert d.cy == 1 << 14 and e.yr + e.yg + e.yb == 1 << 14


# ---------------------------------------------------------------------------------------------- the definition
def _ramp(full):
    lo, hi = (0, 255) if full else (16, 235)
    vals = np.arange(lo, hi + 1, dtype=np.uint8)
    n = len(vals) + len(vals) % 2
    y = np.resize(vals, (4, n)).astype(np.uint8)          # every legal luma value, even sides
    return y, np.full((2, n // 2), 128, np.uint8), np.full((2, n // 2), 128, np.uint8)


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_grey_ramp_is_exact_both_ways(matrix, full):
    v = video()
    y, cu, cv = _ramp(full)
    rgb = v.yuv420_to_rgb_host(y, cu, cv, matrix, full)
    assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 1], rgb[..., 2])
    assert rgb.min() == 0 and rgb.max() == 255             # the legal luma range maps onto the whole RGB range
    y2, u2, v2 = v.rgb_to_yuv420_host(rgb, matrix, full)
    assert np.array_equal(y2, y) and np.array_equal(u2, cu) and np.array_equal(v2, cv)


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_constant_chroma_round_trip_is_exact(matrix, full):
    v = video()
    rng = np.random.RandomState(3)
    y = rng.randint(60, 181, (12, 18)).astype(np.uint8)
    cu = np.full((6, 9), 110, np.uint8)
    cv = np.full((6, 9), 150, np.uint8)
    rgb = v.yuv420_to_rgb_host(y, cu, cv, matrix, full)
    assert 0 < rgb.min() and rgb.max() < 255               # in gamut: no clamp took part
    y2, u2, v2 = v.rgb_to_yuv420_host(rgb, matrix, full)
    assert np.array_equal(y2, y) and np.array_equal(u2, cu) and np.array_equal(v2, cv)


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_random_planes_reach_the_clamps(matrix, full):
    v = video()
    rng = np.random.RandomState(4)
    y = rng.randint(0, 256, (64, 64)).astype(np.uint8)
    cu, cv = (rng.randint(0, 256, (32, 32)).astype(np.uint8) for _ in range(2))
    rgb = v.yuv420_to_rgb_host(y, cu, cv, matrix, full)
    clipped = np.mean((rgb == 0) | (rgb == 255))
    assert 0.15 < clipped < 0.40, clipped


def test_hand_computed_frame():
    """bt601 limited, one chroma pair U = 90, V = 240 for the four pixels, so the 9-3-3-1 filter returns it unchanged
    ((16 c + 8) >> 4 = c): u = -38, v = 112.  Chroma terms: rv v = 26149 * 112 = 2928688; gu u + gv v = 243922 - 1491840
    = -1247918; bu u = -1255900.  Luma term l = 19077 (Y - 16) + 8192:
      Y =  16: l =    8192 -> R = 2936880 >> 14 = 179, G = -1239726 >> 14 < 0 -> 0, B = -1247708 >> 14 < 0 -> 0
      Y = 235: l = 4186055 -> R = 7114743 >> 14 = 434 -> 255, G = 2938137 >> 14 = 179, B = 2930155 >> 14 = 178
      Y =  81: l = 1248197 -> R = 4176885 >> 14 = 254, G = 279 >> 14 = 0, B = -7703 >> 14 = -1 (floor) -> 0
      Y = 145: l = 2469125 -> R = 5397813 >> 14 = 329 -> 255, G = 1221207 >> 14 = 74, B = 1213225 >> 14 = 74"""
    v = video()
    y = np.array([[16, 235], [81, 145]], np.uint8)
    rgb = v.yuv420_to_rgb_host(y, np.array([[90]], np.uint8), np.array([[240]], np.uint8))
    exp = np.array([[[179, 0, 0], [255, 179, 178]], [[254, 0, 0], [255, 74, 74]]], np.uint8)
    assert np.array_equal(rgb, exp)
    # and the encode of that RGB block: Y = ((4207 R + 8260 G + 1604 B + 8192) >> 14) + 16 per pixel:
    #   (179,0,0): 761245 >> 14 = 46 -> 62;  (255,179,178): 2844837 >> 14 = 173 -> 189;
    #   (254,0,0): 1076770 >> 14 = 65 -> 81;  (255,74,74): 1810913 >> 14 = 110 -> 126
    # chroma over the sum (R, G, B) = (943, 253, 252): U = ((-2428*943 - 4768*253 + 7196*252 + 32768) >> 16) + 128
    #   = (-1649748 >> 16) + 128 = -26 + 128 = 102;  V = ((7196*943 - 6026*253 - 1170*252 + 32768) >> 16) + 128
    #   = (4999178 >> 16) + 128 = 76 + 128 = 204
    y2, u2, v2 = v.rgb_to_yuv420_host(exp)
    assert np.array_equal(y2, np.array([[62, 189], [81, 126]], np.uint8))
    assert u2.tolist() == [[102]] and v2.tolist() == [[204]]


def test_chroma_filter_weights_and_edges():
    v = video()
    c = np.array([[0, 160], [80, 240]], np.uint8)
    up = v.upsample_chroma_host(c, 4, 4)
    # corners replicate: all four taps are the corner sample
    assert up[0, 0] == 0 and up[0, 3] == 160 and up[3, 0] == 80 and up[3, 3] == 240
    # pixel (1, 1): centre C[0,0], neighbours right and below: (9*0 + 3*160 + 3*80 + 240 + 8) >> 4 = 968 >> 4 = 60
    assert up[1, 1] == 60
    # pixel (0, 1): vertical neighbour clamps to row 0: (9*0 + 3*160 + 3*0 + 160 + 8) >> 4 = 648 >> 4 = 40
    assert up[0, 1] == 40


def test_host_definition_refuses_bad_frames():
    v = video()
    with pytest.raises(ValueError):
        v.yuv420_to_rgb_host(np.zeros((3, 4), np.uint8), np.zeros((1, 2), np.uint8), np.zeros((1, 2), np.uint8))
    with pytest.raises(ValueError):
        v.yuv420_to_rgb_host(np.zeros((4, 4), np.uint8), np.zeros((2, 1), np.uint8), np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError):
        v.rgb_to_yuv420_host(np.zeros((4, 5, 3), np.uint8))


# ---------------------------------------------------------------------------------------------- files
def _frames(n, W, H, seed=0):
    rng = np.random.RandomState(seed)
    return [(rng.randint(0, 256, (H, W)).astype(np.uint8), rng.randint(0, 256, (H // 2, W // 2)).astype(np.uint8),
             rng.randint(0, 256, (H // 2, W // 2)).astype(np.uint8)) for _ in range(n)]


def test_y4m_round_trip(tmp_path):
    v = video()
    frames = _frames(3, 6, 4)
    p = str(tmp_path / "a.y4m")
    with v.Y4MWriter(p, 6, 4, fps="30000:1001", interlace="p", aspect="1:1", chroma="420mpeg2", xtags=["YSCSS=420MPEG2"]) as w:
        for i, (y, cu, cv) in enumerate(frames):
            w.write_frame(y, cu, cv, params="Ip" if i == 1 else "")
    raw = open(p, "rb").read()
    assert raw.startswith(b"YUV4MPEG2 W6 H4 F30000:1001 Ip A1:1 C420mpeg2 XYSCSS=420MPEG2\nFRAME\n")
    with v.Y4MReader(p) as r:
        assert (r.width, r.height, r.fps, r.interlace, r.aspect, r.chroma) == (6, 4, "30000:1001", "p", "1:1", "420mpeg2")
        assert r.xtags == ["YSCSS=420MPEG2"]
        got, params = [], []
        for fr in r:
            got.append(tuple(p_.copy() for p_ in fr))
            params.append(r.frame_params)
        assert r.read_frame() is None
    assert params == ["", "Ip", ""] and len(got) == 3
    for a, b in zip(got, frames):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # a caller-provided buffer (the command line passes pinned memory) is filled in place
    buf = np.empty(v.frame_bytes(6, 4), np.uint8)
    with v.Y4MReader(p) as r:
        y, cu, cv = r.read_frame(buf)
        assert np.shares_memory(y, buf) and np.array_equal(cv, frames[0][2])
        assert r.skip_frame() and r.skip_frame() and not r.skip_frame()


def test_y4m_default_chroma_is_420jpeg(tmp_path):
    v = video()
    p = str(tmp_path / "b.y4m")
    y, cu, cv = _frames(1, 4, 2)[0]
    open(p, "wb").write(b"YUV4MPEG2 W4 H2 F25:1\nFRAME\n" + y.tobytes() + cu.tobytes() + cv.tobytes())
    with v.Y4MReader(p) as r:
        assert r.chroma == "420jpeg" and r.interlace is None
        assert np.array_equal(r.read_frame()[0], y)


def test_raw_round_trip(tmp_path):
    v = video()
    frames = _frames(3, 6, 4, seed=1)
    p = str(tmp_path / "a.yuv")
    with v.RawYUV420Writer(p, 6, 4) as w:
        for fr in frames:
            w.write_frame(*fr)
    assert len(open(p, "rb").read()) == 3 * 36
    with v.open_reader(p, (6, 4)) as r:
        assert isinstance(r, v.RawYUV420Reader) and r.frames == 3
        assert r.skip_frame()
        got = [tuple(p_.copy() for p_ in fr) for fr in r]
    assert len(got) == 2
    for a, b in zip(got, frames[1:]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="frame size"):
        v.open_reader(p)


@pytest.mark.parametrize("tag", ["C422", "C444", "C420p10", "Cmono"])
def test_y4m_refuses_other_chroma_formats(tmp_path, tag):
    v = video()
    p = str(tmp_path / "c.y4m")
    open(p, "wb").write(b"YUV4MPEG2 W4 H2 F25:1 " + tag.encode() + b"\nFRAME\n" + bytes(64))
    with pytest.raises(ValueError, match=tag):
        v.Y4MReader(p)
    with pytest.raises(ValueError):
        v.Y4MWriter(str(tmp_path / "d.y4m"), 4, 2, chroma=tag[1:])


def test_refusals(tmp_path):
    v = video()
    p = str(tmp_path / "odd.y4m")
    open(p, "wb").write(b"YUV4MPEG2 W5 H2 C420jpeg\nFRAME\n" + bytes(15))
    with pytest.raises(ValueError, match="W5"):
        v.Y4MReader(p)
    open(p, "wb").write(b"RIFF W4 H2\n")
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        v.Y4MReader(p)
    # a truncated last frame is an error, not the end of the video
    y, cu, cv = _frames(1, 4, 2)[0]
    one = b"FRAME\n" + y.tobytes() + cu.tobytes() + cv.tobytes()
    for tail in (one[:-1], b"FRAME\n", b"FRA"):
        open(p, "wb").write(b"YUV4MPEG2 W4 H2 C420jpeg\n" + one + tail)
        with v.Y4MReader(p) as r:
            assert r.read_frame() is not None
            with pytest.raises(ValueError, match="truncated"):
                r.read_frame()
    q = str(tmp_path / "short.yuv")
    open(q, "wb").write(bytes(2 * 12 + 5))
    with pytest.raises(ValueError, match="whole number"):
        v.RawYUV420Reader(q, 4, 2)
    with pytest.raises(ValueError):
        v.RawYUV420Reader(q, 3, 2)
    with pytest.raises(ValueError):
        v.Y4MWriter(str(tmp_path / "e.y4m"), 6, 3)


# ---------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("H,W,core,halo,align", [(40, 56, 16, 4, 1), (50, 38, 16, 5, 1), (1080, 1920, 616, 52, 1),
                                                 (64, 96, 16, 4, 2), (360, 636, 100, 33, 4)])
@pytest.mark.parametrize("scale", [2, 4])
def test_plan_output_rectangles_are_even(H, W, core, halo, align, scale):
    """cores may start at odd input pixels (50 / 4 -> cores of 13) and windows at odd origins (core start - halo), but
    with an even frame and an even scale every output rectangle starts and ends on a whole chroma sample"""
    up = amd("upscale")
    plan = up.plan_windows(H, W, core, halo, align, scale, 64)
    assert len(plan) > 1
    for (wy, wx, cy, cx, ch, cw) in plan.windows:
        assert all(t % 2 == 0 for t in (cy * scale, cx * scale, ch * scale, cw * scale))
    if (H, W, align) == (50, 38, 1):
        assert any(cy % 2 or cx % 2 for (_, _, cy, cx, _, _) in plan.windows)
        assert any(wy % 2 or wx % 2 for (wy, wx, _, _, _, _) in plan.windows)


def test_video_module_imports_no_gpu_code():
    import subprocess
    import sys
    from conftest import ROOT
    code = ("import importlib, sys; sys.path.insert(0, %r); importlib.import_module('ofa-for-super-resolution_amd.video'); "
            "assert 'ofa-for-super-resolution_amd._C' not in sys.modules and 'torch' not in sys.modules" % ROOT)
    # a fresh interpreter: in this one other tests have long imported the bindings
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_library_refuses_bad_frames_before_any_launch():
    """validation happens before a launch, so it runs on a host without a GPU: null pointers, odd sides, a coefficient table
    beyond the range for which int32 is known not to overflow, a window larger than the frame"""
    import ctypes
    C, ops = amd("_C"), amd("ops")
    L = C.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    dec, enc = ops.yuv_table("bt601", False, False), ops.yuv_table("bt601", False, True)
    assert list(dec) == [16, 19077, 26149, -6419, -13320, 33050] and len(enc) == 10
    assert L.ofasr_yuv420_to_rgb_u8(None, p, p, 4, 4, dec, p, None) == -1 and b"null" in L.ofasr_last_error_string()
    assert L.ofasr_yuv420_to_rgb_u8(p, p, p, 4, 5, dec, p, None) == -1 and b"even" in L.ofasr_last_error_string()
    assert L.ofasr_rgb_to_yuv420_u8(p, 3, 4, enc, p, p, p, None) == -1
    bad = (ctypes.c_int32 * 10)(16, 1 << 20, 0, 0, 0, 0, 0, 0, 0, 0)
    assert L.ofasr_rgb_to_yuv420_u8(p, 4, 4, bad, p, p, p, None) == -1 and b"coefficient" in L.ofasr_last_error_string()
    assert L.ofasr_tile_gather_yuv420(p, p, p, 4, 4, dec, p, 1, 6, 4, p, 0, None) == -1
    assert L.ofasr_tile_gather_yuv420(p, p, p, 4, 4, dec, p, 70000, 2, 2, p, 0, None) == -2
    assert L.ofasr_tile_scatter_yuv420(p, 1, 4, 4, 0, p, enc, p, p, p, 4, 6, 8, 4, None) == -1     # bound > source window
    assert L.ofasr_tile_scatter_yuv420(p, 1, 4, 4, 7, p, enc, p, p, p, 4, 6, 4, 4, None) == -1     # dtype
    assert L.ofasr_tile_scatter_yuv420(p, 1, 4, 4, 0, p, enc, p, p, p, 5, 6, 4, 4, None) == -1     # odd plane
