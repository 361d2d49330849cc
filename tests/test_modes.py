"""Keeping an image's mode through upscaling, the host side (no GPU): modes.py against the installed Pillow (the alpha
plane's resize against getchannel("A").resize and against the A band of Pillow's own RGBA / LA resize, the luma against
convert("L")), the bounds the pack kernel relies on, --keep-mode's decoding and argument errors, and the refusals of the
two entry points through the loaded library.  Everything is bit-exact."""
import ctypes
import importlib
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT, amd

# source -> target (H, W): the enlargements of the definition; 17x5 -> 17x20 and 7x7 -> 7x7 keep an axis
SHAPES = [((9, 13), (36, 52)), ((9, 13), (18, 26)), ((9, 13), (23, 31)), ((1, 1), (4, 4)), ((2, 3), (8, 12)),
          ((17, 5), (17, 20)), ((40, 33), (95, 132)), ((7, 7), (7, 7))]
FILTERS = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
PLANES = ["random", "binary", "constant"]


def _plane(kind, H, W, seed):
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randint(0, 256, (H, W)).astype(np.uint8)
    if kind == "binary":
        return (rng.randint(0, 2, (H, W)) * 255).astype(np.uint8)
    return np.full((H, W), 93, np.uint8)


@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_alpha_host_equals_pillow(shape, filt):
    modes = amd("modes")
    (H, W), (TH, TW) = shape
    for i, kind in enumerate(PLANES):
        a = _plane(kind, H, W, 7 + i)
        got = modes.alpha_host(a, TH, TW, filt)
        assert got.shape == (TH, TW) and got.dtype == np.uint8
        rgb = np.random.RandomState(3).randint(0, 256, (H, W, 3)).astype(np.uint8)
        rgba = Image.fromarray(np.dstack([rgb, a]), "RGBA")
        assert np.array_equal(got, np.asarray(rgba.getchannel("A").resize((TW, TH), FILTERS[filt]))), kind
        # the A band of Pillow's own resize of the whole image is the resize of the A band alone
        assert np.array_equal(got, np.asarray(rgba.resize((TW, TH), FILTERS[filt]))[:, :, 3]), kind
        la = Image.fromarray(np.dstack([rgb[:, :, 0], a]), "LA")
        assert np.array_equal(got, np.asarray(la.resize((TW, TH), FILTERS[filt]))[:, :, 1]), kind
    opaque = np.full((H, W), 255, np.uint8)
    assert np.all(modes.alpha_host(opaque, TH, TW, filt) == 255)


def test_alpha_host_default_and_refusals():
    modes = amd("modes")
    a = _plane("random", 9, 13, 1)
    assert modes.ALPHA_FILTER == "bicubic"
    assert np.array_equal(modes.alpha_host(a, 36, 52), modes.alpha_host(a, 36, 52, "bicubic"))
    with pytest.raises(ValueError):
        modes.alpha_host(a, 36, 52, "box")
    with pytest.raises(ValueError):
        modes.alpha_host(a[:, :, None], 36, 52)


def test_luma_host_equals_pillow():
    modes = amd("modes")
    rgb = np.random.RandomState(5).randint(0, 256, (61, 47, 3)).astype(np.uint8)
    rgb[0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255]]
    assert np.array_equal(modes.luma_host(rgb), np.asarray(Image.fromarray(rgb, "RGB").convert("L")))
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)        # R = G = B = L stays L
    assert np.array_equal(modes.luma_host(grey)[0], np.arange(256))


def test_split_and_join_round_trip_channel_counts():
    modes = amd("modes")
    assert modes.MODES == {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}
    rng = np.random.RandomState(9)
    for C in (1, 2, 3, 4):
        img = rng.randint(0, 256, (6, 5, C)).astype(np.uint8)
        rgb, alpha = modes.split_host(img)
        assert rgb.shape == (6, 5, 3) and rgb.dtype == np.uint8 and rgb.flags.c_contiguous
        assert (alpha is None) == (C in (1, 3))
        pil = Image.fromarray(img[:, :, 0] if C == 1 else img, modes.MODES[C])
        assert np.array_equal(rgb, np.asarray(pil.convert("RGB")))                     # Pillow drops alpha, repeats L
        if alpha is not None:
            assert np.array_equal(alpha, img[:, :, C - 1]) and alpha.flags.c_contiguous
        back = modes.join_host(rgb, C, alpha)
        assert back.shape == img.shape and back.dtype == np.uint8
        assert np.array_equal(back, img)                                               # luma of (L, L, L) is L
    rgb = rng.randint(0, 256, (6, 5, 3)).astype(np.uint8)
    a = rng.randint(0, 256, (6, 5)).astype(np.uint8)
    la = modes.join_host(rgb, 2, a)
    assert np.array_equal(la[:, :, 0], modes.luma_host(rgb)) and np.array_equal(la[:, :, 1], a)
    for bad in (lambda: modes.join_host(rgb, 4), lambda: modes.join_host(rgb, 3, a), lambda: modes.join_host(rgb, 1, a),
                lambda: modes.join_host(rgb, 5), lambda: modes.join_host(rgb, 2, a[:5]),
                lambda: modes.split_host(np.zeros((4, 4, 5), np.uint8)), lambda: modes.split_host(np.zeros((4, 4), np.uint8)),
                lambda: modes.split_host(np.zeros((4, 4, 3), np.uint16))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("filt", sorted(FILTERS))
def test_alpha_tables_bounds(filt):
    modes, resize = amd("modes"), amd("resize")
    assert (modes.MAX_TAPS, modes.TILE_ROWS, modes.MAX_SOURCE_ROWS) == (7, 16, 24)
    cases = [(24, 24), (24, 32), (24, 48), (24, 64), (24, 96), (23, 61), (1, 1), (1, 4), (2, 2), (2, 8), (2, 5), (1, 3),
             (270, 1080), (37, 101)]                      # ratios 1, 4/3, 2, 8/3, 4, an odd target; sizes 1 and 2
    for n, t in cases:
        for (H, W, TH, TW) in ((n, 5, t, 20), (5, n, 20, t)):
            vt, ht = modes.alpha_tables(H, W, TH, TW, filt)
            assert np.array_equal(vt, resize.axis_table(H, TH, filt)) and np.array_equal(ht, resize.axis_table(W, TW, filt))
            for tab, S, T in ((vt, H, TH), (ht, W, TW)):
                assert tab.dtype == np.int32 and tab.shape[0] == T
                taps = tab.shape[1] - 2
                assert taps == (1 if S == T else {"bicubic": 5, "lanczos": 7}[filt]) <= modes.MAX_TAPS
                assert int(tab[:, 0].min()) >= 0 and int((tab[:, 0] + tab[:, 1]).max()) <= S and int(tab[:, 1].min()) >= 1
                for t0 in range(T):
                    lo, hi = resize.needed_range(tab, t0, min(t0 + 16, T))
                    assert hi - lo <= 24
    with pytest.raises(ValueError):
        modes.alpha_tables(8, 8, 7, 16, filt)             # a reduction is not the pack kernel's business
    with pytest.raises(ValueError):
        modes.alpha_tables(8, 8, 16, 16, "nearest")


# ---------------------------------------------------------------------------------------------- command line
def _cli():
    sys.path.insert(0, ROOT)
    return importlib.import_module("upscale_ofa_net_sr")


def test_keep_mode_decodes_every_file_into_its_mode(tmp_path):
    cli = _cli()
    rng = np.random.RandomState(2)
    H, W = 7, 9
    rgb = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    rgba = rng.randint(0, 256, (H, W, 4)).astype(np.uint8)
    grey = rng.randint(0, 256, (H, W)).astype(np.uint8)
    la = rng.randint(0, 256, (H, W, 2)).astype(np.uint8)
    bits = rng.randint(0, 2, (H, W)).astype(bool)
    pal = Image.fromarray(rgb, "RGB").quantize(8)
    i16 = Image.fromarray(rng.randint(0, 65536, (H, W)).astype(np.uint16))
    assert pal.mode == "P" and i16.mode.startswith("I;16")
    files = {}

    def save(name, im, **kw):
        files[name] = str(tmp_path / (name + ".png"))
        im.save(files[name], **kw)

    save("rgb", Image.fromarray(rgb, "RGB"))
    save("rgba", Image.fromarray(rgba, "RGBA"))
    save("l", Image.fromarray(grey, "L"))
    save("la", Image.fromarray(la, "LA"))
    save("one", Image.fromarray(bits))
    save("p", pal)
    save("p_trns", pal, transparency=2)
    save("l_trns", Image.fromarray(grey, "L"), transparency=int(grey[0, 0]))
    save("i16", i16)
    with Image.open(files["one"]) as im:
        assert im.mode == "1"
    with Image.open(files["p_trns"]) as im:
        assert im.mode == "P" and "transparency" in im.info
    with Image.open(files["l_trns"]) as im:
        assert im.mode == "L" and "transparency" in im.info
    with Image.open(files["p"]) as im:
        assert im.mode == "P" and "transparency" not in im.info

    def pil(name, mode):
        with Image.open(files[name]) as im:
            arr = np.asarray(im.convert(mode))
        return arr if arr.ndim == 3 else arr[:, :, None]

    expect = {"rgb": rgb, "rgba": rgba, "l": grey[:, :, None], "la": la, "one": pil("one", "L"), "p": pil("p", "RGB"),
              "p_trns": pil("p_trns", "RGBA"), "l_trns": pil("l_trns", "RGBA"), "i16": pil("i16", "RGB")}
    channels = {"rgb": 3, "rgba": 4, "l": 1, "la": 2, "one": 1, "p": 3, "p_trns": 4, "l_trns": 4, "i16": 3}
    for name, path in files.items():
        got = cli.decode_keep(path)
        assert got.dtype == np.uint8 and got.shape == (H, W, channels[name]) and got.flags.c_contiguous, name
        assert np.array_equal(got, expect[name]), name
        # without the flag every file is RGB, as before
        assert np.array_equal(cli.decode(path), pil(name, "RGB")), name
    assert set(np.unique(cli.decode_keep(files["one"]))) <= {0, 255}
    a = cli.decode_keep(files["p_trns"])[:, :, 3]
    assert a.min() == 0 and a.max() == 255                      # the transparent palette entry is there, and only it
    assert (cli.decode_keep(files["l_trns"])[:, :, 3] == 0).any()
    # and back: the PNG is written in the kept mode
    for name in ("rgb", "rgba", "l", "la"):
        arr = cli.decode_keep(files[name])
        dst = cli.encode_keep(arr, str(tmp_path / ("out_" + name + ".png")))
        with Image.open(dst) as im:
            assert im.mode == amd("modes").MODES[arr.shape[2]]
        assert np.array_equal(cli.decode_keep(dst), arr)


def test_keep_mode_arguments():
    cli = _cli()
    base = ["--static", "d", "--out", "o", "a.png"]
    a = cli.parse_args(base)
    assert a.keep_mode is False and a.alpha_resample is None
    a = cli.parse_args(["--keep-mode"] + base)
    assert a.keep_mode is True and a.alpha_resample is None
    assert cli.parse_args(["--keep-mode", "--alpha-resample", "lanczos"] + base).alpha_resample == "lanczos"
    assert cli.parse_args(["--keep-mode", "--alpha-resample", "bicubic"] + base).alpha_resample == "bicubic"
    with pytest.raises(SystemExit):
        cli.parse_args(["--alpha-resample", "lanczos"] + base)          # needs --keep-mode
    with pytest.raises(SystemExit):
        cli.parse_args(["--keep-mode", "--alpha-resample", "box"] + base)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_refuse_bad_arguments_without_gpu():
    # validation happens before any launch, so it can be exercised on a GPU-less host
    C = amd("_C")
    L = C.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def err():
        return L.ofasr_last_error_string()

    un = L.ofasr_mode_unpack_u8
    assert un(None, 4, p, p, 2, 2, None) == -1 and b"null" in err()
    assert un(p, 4, None, p, 2, 2, None) == -1 and b"null" in err()
    assert un(p, 4, p, None, 2, 2, None) == -1 and b"null" in err()        # RGBA and LA have an alpha plane to write
    assert un(p, 2, p, None, 2, 2, None) == -1
    assert un(p, 1, p, p, 2, 2, None) == -1 and b"alpha" in err()          # L has none
    for c in (0, 3, 5, -1):
        assert un(p, c, p, p, 2, 2, None) == -1 and b"channels" in err()
    assert un(p, 4, p, p, 0, 2, None) == -1 and un(p, 4, p, p, 2, -1, None) == -1 and b"size" in err()
    assert un(p, 4, p, p, 1 << 30, 1 << 30, None) == -2                    # beyond what the grid holds

    pk = L.ofasr_mode_pack_u8
    assert pk(None, p, p, 5, p, 5, p, 4, 2, 2, 4, 4, None) == -1 and b"null" in err()
    assert pk(p, p, p, 5, p, 5, None, 4, 2, 2, 4, 4, None) == -1 and b"null" in err()
    assert pk(p, None, p, 5, p, 5, p, 4, 2, 2, 4, 4, None) == -1 and b"null" in err()
    assert pk(p, p, None, 5, p, 5, p, 2, 2, 2, 4, 4, None) == -1
    assert pk(p, p, p, 5, None, 5, p, 2, 2, 2, 4, 4, None) == -1
    assert pk(None, None, None, 0, None, 0, p, 1, 2, 2, 4, 4, None) == -1  # L takes no alpha and no tables, but rgb
    for c in (0, 3, 5):
        assert pk(p, p, p, 5, p, 5, p, c, 2, 2, 4, 4, None) == -1 and b"channels" in err()
    for kh, kw in ((0, 5), (5, 0), (8, 5), (5, 8), (-1, 5), (25, 25)):
        assert pk(p, p, p, kh, p, kw, p, 4, 2, 2, 4, 4, None) == -2 and b"enlarges only" in err()
    assert pk(p, p, p, 5, p, 5, p, 4, 8, 2, 4, 4, None) == -2 and b"enlarges only" in err()     # a smaller target
    for sizes in ((0, 2, 4, 4), (2, 0, 4, 4), (2, 2, 0, 4), (2, 2, 4, -3)):
        assert pk(p, p, p, 5, p, 5, p, 4, *sizes, None) == -1 and b"size" in err()
    assert pk(p, p, p, 5, p, 5, p, 4, 2, 2, 1 << 30, 1 << 30, None) == -2
    assert pk(p, None, None, 0, None, 0, p, 1, 2, 2, 1 << 30, 1 << 30, None) == -2


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    ops, C = amd("ops"), amd("_C")
    with pytest.raises(C.OfasrError):
        ops.mode_unpack_u8(torch.zeros(4, 4, 4, dtype=torch.uint8))
    with pytest.raises(C.OfasrError):
        ops.mode_pack_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), 1)
    with pytest.raises(ValueError):
        ops.mode_pack_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), 3)
