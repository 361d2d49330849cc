"""Target-size output, host side (no GPU): resize.py against the installed Pillow and against oracle/pil_bicubic.py, the
10-bit arithmetic against a big-integer restatement, the target partition and the wider halo of upscale.plan_resize, a
host-only tiled composition against the whole-frame definition, the refusals, the command lines' --out-size and the Y4M
header."""
import itertools
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, amd

SIZES = [(64, 96, 48, 54), (40, 40, 10, 10), (37, 53, 36, 30), (64, 64, 64, 32), (128, 72, 90, 72), (31, 45, 31, 45)]
FILTERS = ["bicubic", "lanczos"]


def _pil_filter(name):
    from PIL import Image
    return {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[name]


# ---------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("h,w,oh,ow", SIZES)
def test_resize_host_equals_pillow(h, w, oh, ow, filt):
    from PIL import Image
    from oracle import pil_bicubic
    resize = amd("resize")
    a = np.random.RandomState(h + w + oh).randint(0, 256, (h, w)).astype(np.uint8)
    a[0, :4] = (0, 255, 0, 255)
    got = resize.resize_host(a, oh, ow, filt)
    ref = np.asarray(Image.fromarray(a).resize((ow, oh), _pil_filter(filt)))
    assert got.dtype == np.uint8 and np.array_equal(got, ref)
    if (oh, ow) == (h, w):
        assert np.array_equal(got, a)          # ratio exactly 1: no pass runs
    if filt == "bicubic":
        assert np.array_equal(got, pil_bicubic.resize_u8(a, oh, ow))


@pytest.mark.parametrize("filt", FILTERS)
def test_resize_host_hwc_and_stacked_planes(filt):
    from PIL import Image
    resize = amd("resize")
    a = np.random.RandomState(3).randint(0, 256, (33, 47, 3)).astype(np.uint8)
    ref = np.asarray(Image.fromarray(a).resize((20, 17), _pil_filter(filt)))
    assert np.array_equal(resize.resize_host(a, 17, 20, filt, hwc=True), ref)
    planes = np.ascontiguousarray(np.moveaxis(a, 2, 0))[None]
    assert np.array_equal(resize.resize_host(planes, 17, 20, filt)[0], np.moveaxis(ref, 2, 0))


@pytest.mark.parametrize("n_in,n_out", [(96, 54), (40, 10), (53, 30), (72, 72), (64, 63)])
def test_coeff_table_equals_the_bicubic_oracle(n_in, n_out):
    from oracle import pil_bicubic
    resize = amd("resize")
    xmins, counts, kk = pil_bicubic.coeffs(n_in, n_out)
    t = resize.coeff_table(n_in, n_out, "bicubic")
    assert t.dtype == np.int32 and t.shape == (n_out, 2 + kk.shape[1]) and t.shape[1] - 2 == resize.ksize(n_in, n_out, "bicubic")
    assert np.array_equal(t[:, 0], xmins) and np.array_equal(t[:, 1], counts) and np.array_equal(t[:, 2:], kk)


def test_lanczos_taps_and_identity_table():
    resize = amd("resize")
    assert resize.ksize(400, 100, "lanczos") == resize.MAX_TAPS == 25 and resize.ksize(400, 100, "bicubic") == 17
    t = resize.coeff_table(400, 100, "lanczos")
    assert t.shape == (100, 27) and int(t[:, 1].max()) <= 25
    assert np.all(np.abs(t[:, 2:].sum(axis=1) - (1 << 22)) <= 25)           # each row sums to one, up to the roundings
    # the pass that Pillow skips, as a table: exact
    a = np.random.RandomState(0).randint(0, 256, (5, 9)).astype(np.uint8)
    assert np.array_equal(resize.apply_table(a, resize.identity_table(9), 8, -1), a)
    b = np.random.RandomState(0).randint(0, 1024, (5, 9)).astype(np.uint16)
    assert np.array_equal(resize.apply_table(b, resize.identity_table(9, 10), 10, -1), b)


def _bigint_pass(rows, in_size, out_size, filt, depth):
    """an independent restatement with Python integers: list of rows -> list of rows, along the row"""
    sup = {"bicubic": 2.0, "lanczos": 3.0}[filt]

    def f(x):
        if filt == "bicubic":
            x = abs(x)
            return (1.5 * x - 2.5) * x * x + 1 if x < 1.0 else ((((x - 5) * x + 8) * x - 4) * -0.5 if x < 2.0 else 0.0)
        if not -3.0 <= x < 3.0:
            return 0.0

        def sinc(v):
            return 1.0 if v == 0.0 else math.sin(v * math.pi) / (v * math.pi)
        return sinc(x) * sinc(x / 3)

    bits = 32 - depth - 2
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = sup * fs
    out = [[0] * out_size for _ in rows]
    extreme = 0
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = [f((x - center + 0.5) * (1.0 / fs)) for x in range(xmin, xmax)]
        ww = 0.0
        for v in w:
            ww += v
        k = [int(-0.5 + v / ww * (1 << bits)) if v / ww < 0 else int(0.5 + v / ww * (1 << bits)) for v in w]
        for r, row in enumerate(rows):
            acc = 1 << (bits - 1)
            for j, kj in enumerate(k):
                acc += int(row[xmin + j]) * kj
                extreme = max(extreme, abs(acc))
            out[r][xx] = min(max(acc >> bits, 0), (1 << depth) - 1)
    return out, extreme


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("h,w,oh,ow", [(24, 36, 13, 20), (16, 40, 16, 10), (21, 12, 6, 12)])
def test_depth10_equals_a_big_integer_restatement(h, w, oh, ow, filt):
    resize = amd("resize")
    rng = np.random.RandomState(h * w)
    a = rng.randint(0, 1024, (h, w)).astype(np.uint16)
    a[0, :6] = (0, 1023, 0, 1023, 1023, 0)
    a[1:3] = rng.choice([0, 1023], (2, w))          # the extremes side by side: the largest accumulators
    got = resize.resize_host(a, oh, ow, filt, depth=10)   # asserts int32 accumulators itself
    rows, extreme = [list(map(int, r)) for r in a], 0
    if ow != w:
        rows, e = _bigint_pass(rows, w, ow, filt, 10)
        extreme = max(extreme, e)
    if oh != h:
        cols, e = _bigint_pass([list(c) for c in zip(*rows)], h, oh, filt, 10)
        rows = [list(r) for r in zip(*cols)]
        extreme = max(extreme, e)
    assert got.dtype == np.uint16 and np.array_equal(got, np.array(rows, np.uint16))
    assert extreme < 2 ** 31 and int(got.max()) <= 1023
    assert np.array_equal(resize.coeff_table(w, ow, filt, 10)[:, :2], resize.coeff_table(w, ow, filt, 8)[:, :2])


def test_quantise_is_the_scatters_rounding():
    resize = amd("resize")
    x = np.array([-0.5, 0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 127.5 / 255, 1.0, 1.7], np.float32)
    assert resize.quantise(x).tolist() == np.rint(np.clip(x, 0, 1) * np.float32(255)).astype(np.uint8).tolist()
    assert resize.quantise(x, 10).dtype == np.uint16 and int(resize.quantise(x, 10).max()) == 1023


# ---------------------------------------------------------------------------------------------- the plan
def _ratios(L, s):
    S = L * s
    out = {L, S, -(-S * 3 // 4), (L + S) // 2, -(-S // 3) if S // 3 >= L else L, L + 1, S - 1}
    return sorted(t for t in out if L <= t <= S)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("s,radius", [(2, 9), (4, 17)])
def test_plan_targets_tile_the_target_and_stay_exact(s, radius, filt):
    up, resize = amd("upscale"), amd("resize")
    for (H, W), core, even in itertools.product([(40, 56), (72, 104), (90, 160)], [16, 24, 90], [False, True]):
        for TH, TW in zip(_ratios(H, s), reversed(_ratios(W, s))):
            if even:
                TH, TW = TH + TH % 2, TW + TW % 2
            if (TH, TW) == (H * s, W * s):
                continue
            plan = up.plan_resize(H, W, (TH, TW), filt, core, radius, 1, s, 64, False, even)   # checks every window itself
            assert isinstance(plan, up.ResizePlan) and plan.halo == radius + plan.extra
            assert plan.extra <= math.ceil(((resize.SUPPORT[filt] + 1.5) * max(H * s / TH, W * s / TW) + 1) / s)
            cover = np.zeros((TH, TW), np.int32)
            for (dy, dx, eh, ew) in plan.targets:
                assert eh >= 0 and ew >= 0
                assert not even or (dy % 2 == dx % 2 == eh % 2 == ew % 2 == 0)
                cover[dy:dy + eh, dx:dx + ew] += 1
            assert cover.min() == cover.max() == 1
            # the check again, spelled out: what each rectangle reads lies `radius` inside the window's non-image edges
            vt, ht = plan.tables(8)
            for (wy, wx, cy, cx, ch, cw), (dy, dx, eh, ew) in zip(plan.windows, plan.targets):
                if eh == 0 or ew == 0:
                    continue
                ylo, yhi = resize.needed_range(vt, dy, dy + eh)
                xlo, xhi = resize.needed_range(ht, dx, dx + ew)
                assert ylo >= (wy + (radius if wy > 0 else 0)) * s and yhi <= (wy + plan.win_h - (radius if wy + plan.win_h < H else 0)) * s
                assert xlo >= (wx + (radius if wx > 0 else 0)) * s and xhi <= (wx + plan.win_w - (radius if wx + plan.win_w < W else 0)) * s


def test_full_size_target_is_todays_plan():
    up = amd("upscale")
    for even in (False, True):
        a = up.plan_resize(72, 104, (288, 416), "lanczos", 16, 17, 1, 4, 64, False, even)
        b = up.plan_windows(72, 104, 16, 17, 1, 4, 64)
        assert type(a) is up.TilePlan and not isinstance(a, up.ResizePlan)
        assert a.windows == b.windows and (a.win_h, a.win_w, a.batch) == (b.win_h, b.win_w, b.batch)


def test_a_core_may_own_no_target_pixels():
    up = amd("upscale")
    plan = up.plan_resize(8, 64, (8, 64), "bicubic", 1, 1, 1, 2, 64, False, True)
    empties = [t for t in plan.targets if t[2] == 0 or t[3] == 0]
    assert empties and sum(t[2] * t[3] for t in plan.targets) == 8 * 64


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("even", [False, True])
def test_host_tiled_composition_equals_the_whole_frame_definition(filt, even):
    """a random float 'network output' cut into the plan's windows; each window's rectangle computed from that window
    alone, as the kernel does (taps clamped into the window), equals the definition on the whole array"""
    up, resize = amd("upscale"), amd("resize")
    H, W, s, radius = 72, 104, 4, 17
    TH, TW = 108, 150
    whole = np.random.RandomState(5).uniform(-0.2, 1.2, (3, H * s, W * s)).astype(np.float32)
    ref = resize.resize_host(resize.quantise(whole), TH, TW, filt)
    plan = up.plan_resize(H, W, (TH, TW), filt, 16, radius, 1, s, 64, False, even)
    assert len(plan) >= 4
    vt, ht = plan.tables(8)
    out = np.full((3, TH, TW), 77, np.uint8)
    for (wy, wx, _, _, _, _), (dy, dx, eh, ew) in zip(plan.windows, plan.targets):
        if eh == 0 or ew == 0:
            continue
        q = resize.quantise(whole[:, wy * s:(wy + plan.win_h) * s, wx * s:(wx + plan.win_w) * s])
        hrows = ht[dx:dx + ew].copy()
        hrows[:, 0] -= wx * s
        vrows = vt[dy:dy + eh].copy()
        vrows[:, 0] -= wy * s
        assert hrows[:, 0].min() >= 0 and (hrows[:, 0] + hrows[:, 1]).max() <= q.shape[2]
        assert vrows[:, 0].min() >= 0 and (vrows[:, 0] + vrows[:, 1]).max() <= q.shape[1]
        out[:, dy:dy + eh, dx:dx + ew] = resize.apply_table(resize.apply_table(q, hrows, 8, -1), vrows, 8, -2)
    assert np.array_equal(out, ref)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals():
    up, resize = amd("upscale"), amd("resize")
    args = ("lanczos", 16, 17, 1, 4, 64, False)
    with pytest.raises(ValueError, match=r"width 56 \.\. 224, height 40 \.\. 160"):
        up.plan_resize(40, 56, (39, 100), *args, False)          # below the input
    with pytest.raises(ValueError, match=r"width 56 \.\. 224"):
        up.plan_resize(40, 56, (100, 225), *args, False)         # above s x
    with pytest.raises(ValueError, match="even sides"):
        up.plan_resize(40, 56, (101, 100), *args, True)
    with pytest.raises(ValueError, match="even sides"):
        up.plan_resize(40, 56, (100, 101), *args, True)
    up.plan_resize(40, 56, (101, 101), *args, False)             # odd is fine for images
    with pytest.raises(ValueError, match="resample must be one of"):
        up.plan_resize(40, 56, (100, 100), "nearest", 16, 17, 1, 4, 64, False, False)
    with pytest.raises(ValueError, match="resample must be one of"):
        resize.resize_host(np.zeros((4, 4), np.uint8), 2, 2, "box")
    with pytest.raises(ValueError, match="resample must be one of"):
        resize.coeff_table(8, 4, "hamming")
    with pytest.raises(ValueError, match="depth"):
        resize.coeff_table(8, 4, "lanczos", 12)
    with pytest.raises(ValueError, match="out_size"):
        up.plan_resize(40, 56, 100, *args, False)


def test_entry_points_validate_before_launch():
    import ctypes
    C = amd("_C")
    L = C.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    enc = (ctypes.c_int32 * 10)(16, 4000, 8000, 1500, -2000, -4000, 6000, 6000, -5000, -1000)
    ok = (p, 1, 8, 8, C.F32, p, p, 5, p, 5)
    assert L.ofasr_tile_resize_scatter_u8(*ok, None, 4, 4, 4, 4, None) == -1 and b"null" in L.ofasr_last_error_string()
    assert L.ofasr_tile_resize_scatter_u8(p, 1, 8, 8, 7, p, p, 5, p, 5, p, 4, 4, 4, 4, None) == -1          # dtype
    assert L.ofasr_tile_resize_scatter_u8(p, 1, 8, 8, C.F32, p, p, 0, p, 5, p, 4, 4, 4, 4, None) == -1      # no taps
    assert L.ofasr_tile_resize_scatter_u8(p, 1, 8, 8, C.F32, p, p, 26, p, 5, p, 4, 4, 4, 4, None) == -2     # > 25 taps
    assert L.ofasr_tile_resize_scatter_u8(*ok, p, 4, 4, 5, 4, None) == -1                                    # extent bound > target
    assert L.ofasr_tile_resize_scatter_u8(*ok, p, 0, 4, 4, 4, None) == -1                                    # empty target
    assert L.ofasr_tile_resize_scatter_yuv420(*ok, enc, p, p, p, 5, 4, 4, 4, None) == -1                     # odd side
    assert b"even sides" in L.ofasr_last_error_string()
    assert L.ofasr_tile_resize_scatter_yuv420(*ok, None, p, p, p, 4, 4, 4, 4, None) == -1
    assert L.ofasr_tile_resize_scatter_yuv420p16(*ok, 12, enc, p, p, p, 4, 4, 4, 4, None) == -1              # depth
    assert L.ofasr_tile_resize_scatter_yuv420p16(*ok, 10, enc, p, p, ctypes.c_void_p(p.value + 1), 4, 4, 4, 4, None) == -1
    assert L.ofasr_version() >= 310


# ---------------------------------------------------------------------------------------------- command lines
def _cli(name):
    sys.path.insert(0, ROOT)
    import importlib
    return importlib.import_module(name)


def test_command_lines_parse_out_size():
    for name, base in (("upscale_video_ofa_net_sr", ["--static", "d", "--out", "o.y4m", "in.y4m"]),
                       ("upscale_ofa_net_sr", ["--static", "d", "--out", "o", "a.png"])):
        cli = _cli(name)
        a = cli.parse_args(base)
        assert a.out_size is None and a.resample == "lanczos"
        a = cli.parse_args(["--out-size", "3840x2160", "--resample", "bicubic"] + base)
        assert a.out_size == (3840, 2160) and a.resample == "bicubic"
        assert cli.parse_args(["--out-size", "120X84"] + base).out_size == (120, 84)
        for bad in ("3840", "3840x", "ax2", "0x10", "10x-2", "1x2x3"):
            with pytest.raises(SystemExit):
                cli.parse_args(["--out-size", bad] + base)
        with pytest.raises(SystemExit):
            cli.parse_args(["--resample", "nearest"] + base)
    assert amd("resize").parse_size("64x48") == (64, 48)


def test_video_command_line_checks_the_target_and_opens_its_writer_at_it(tmp_path):
    """the command line's own size check (upscale.check_out_size behind it) and the writer it opens for a Y4M input: the
    header carries the target size and the input's other tags.  The frames need the GPU: tests/test_hip_resize.py."""
    cli, video, up = _cli("upscale_video_ofa_net_sr"), amd("video"), amd("upscale")
    assert cli.output_size(56, 40, 4, None) == (224, 160)
    assert cli.output_size(56, 40, 4, (120, 84)) == (120, 84)
    for bad, why in (((121, 84), "even sides"), ((120, 38), r"height 40 \.\. 160"), ((226, 84), r"width 56 \.\. 224")):
        with pytest.raises(SystemExit, match=why):
            cli.output_size(56, 40, 4, bad)
        with pytest.raises(ValueError, match=why):                   # one statement of the rule, one wording
            up.check_out_size(40, 56, 4, (bad[1], bad[0]), even=True)
    src = str(tmp_path / "i.y4m")
    zeros = lambda w, h: (np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8))
    with video.Y4MWriter(src, 56, 40, fps="30000:1001") as w:
        w.write_frame(*zeros(56, 40))
    OW, OH = cli.output_size(56, 40, 4, (120, 84))
    path = str(tmp_path / "o.y4m")
    with video.open_reader(src, None, None) as reader:
        with cli.open_writer(video, reader, path, OW, OH, 8, 8) as w:
            w.write_frame(*zeros(OW, OH))
    assert open(path, "rb").read().startswith(b"YUV4MPEG2 W120 H84 F30000:1001")
    with video.Y4MReader(path) as rd:
        assert (rd.width, rd.height) == (120, 84)
    raw = str(tmp_path / "o.yuv")
    with video.open_reader(src, None, None) as reader:
        with cli.open_writer(video, reader, raw, OW, OH, 8, 8) as w:
            w.write_frame(*zeros(OW, OH))
    assert os.path.getsize(raw) == video.frame_bytes(OW, OH, 8)


def test_a_widened_halo_does_not_push_a_window_over_the_activation_limit():
    """default_core sizes the core for the plain halo: 1024 elements per pixel, radius 16 and core 688 give windows of
    720 x 720 (4 * 1024 * 720^2 < 2^31), and the halo of a target size would make them 728 (4 * 1024 * 728^2 > 2^31).
    plan_resize shrinks the core until the window fits again, and refuses where no core can."""
    up = amd("upscale")
    px, radius, core, L, s = 1024, 16, 688, 1376, 4
    assert up.default_core(radius, 1, px) == core
    plain = up.plan_windows(L, L, core, radius, 1, s, px)
    assert (plain.win_h, plain.win_w) == (720, 720) and 4 * px * 720 * 720 < up.LIMIT <= 4 * px * 728 * 728
    plan = up.plan_resize(L, L, (2 * L, 2 * L), "lanczos", core, radius, 1, s, px)
    assert plan.extra >= 1 and plan.halo == radius + plan.extra
    assert 4 * px * plan.win_h * plan.win_w < up.LIMIT
    assert plan.core < core and max(w[4] for w in plan.windows) <= plan.core and max(w[5] for w in plan.windows) <= plan.core
    cover = np.zeros((2 * L, 2 * L), np.int8)
    for (dy, dx, eh, ew) in plan.targets:
        cover[dy:dy + eh, dx:dx + ew] += 1
    assert cover.min() == cover.max() == 1
    # a core the caller chose too large for the limit already stays the caller's business, as without out_size
    big = up.plan_resize(2000, 2000, (4000, 4000), "lanczos", 1000, radius, 1, s, px)
    assert big.core == 1000 and 4 * px * big.win_h * big.win_w >= up.LIMIT
    # the smallest core: 8 + 2 * 16 = 40 fits under 300000 elements per pixel, 8 + 2 * (16 + extra) -> 48 does not
    assert 4 * 300000 * 40 * 40 < up.LIMIT <= 4 * 300000 * 48 * 48
    with pytest.raises(ValueError, match=r"--core"):
        up.plan_resize(64, 64, (128, 128), "lanczos", 8, radius, 1, s, 300000)
