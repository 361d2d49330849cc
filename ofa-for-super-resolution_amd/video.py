"""Raw 8-bit and 10-bit YUV 4:2:0 video for the upscaling path: the host definition of the colour conversion that the HIP kernels of
csrc/yuv.hip implement, the host definition of "this window's input changed between two frames" that csrc/reuse.hip
implements (window_support / changed_windows_host), and streaming readers / writers for Y4M (YUV4MPEG2) and headerless
`yuv420p` / `yuv420p10le` files.

numpy only: nothing here touches the GPU, and importing this module loads no GPU code.

The conversion is a pinned definition of this project, all of it integer arithmetic (int32 suffices: every sum stays
below 2^24 in magnitude), so host and device agree bit for bit.  With S = 14, q(v) = int(round(v * 2^S)) and >> the
arithmetic (floor) shift:

  coefficients   (Kr, Kb) = (0.299, 0.114) for bt601, (0.2126, 0.0722) for bt709, Kg = 1 - Kr - Kb; limited ("tv") range:
                 yo = 16, ys = 255/219, cs = 255/224, yi = 219/255, ci = 224/255; full ("pc") range: yo = 0, scales 1.
                 decode: cy = q(ys), rv = q(cs 2(1-Kr)), gu = q(-cs 2(1-Kb) Kb/Kg), gv = q(-cs 2(1-Kr) Kr/Kg),
                         bu = q(cs 2(1-Kb))
                 encode: yr, yg, yb = q(yi K*); ur = q(-ci Kr / (2(1-Kb))), ug = q(-ci Kg / (2(1-Kb))), ub = q(ci / 2);
                         vr = q(ci / 2), vg = q(-ci Kg / (2(1-Kr))), vb = q(-ci Kb / (2(1-Kr)))
                 (the U row and the V row each sum to exactly 0 in all four matrix x range combinations: grey stays grey)
  decode         chroma to full resolution by the centre-sited 9-3-3-1 filter, edge replication at the frame edge: for
                 pixel (y, x), cy0 = y >> 1, the vertical neighbour row is cy0 - 1 for even y and cy0 + 1 for odd y, the
                 horizontal one alike from x, both clamped into the plane, and
                     c = (9 C[cy0,cx0] + 3 C[cy0,nx] + 3 C[ny,cx0] + C[ny,nx] + 8) >> 4
                 then with y' = Y - yo, u = c_U - 128, v = c_V - 128:
                     R = clamp((cy y' + rv v + 2^13) >> 14), G = clamp((cy y' + gu u + gv v + 2^13) >> 14),
                     B = clamp((cy y' + bu u + 2^13) >> 14)
  encode         Y = clamp(((yr R + yg G + yb B + 2^13) >> 14) + yo) per pixel; chroma is the 2x2 box with one rounding:
                     U = clamp(((sum of the 4 pixels' (ur R + ug G + ub B) + 2^15) >> 16) + 128), V alike.

Chroma siting.  Every accepted 4:2:0 flavour (C420jpeg, C420mpeg2, C420paldv, plain C420) is treated as centre-sited
(the JPEG / MPEG-1 siting), which is exact for C420jpeg.  MPEG-2 siting puts the chroma sample a quarter of a luma pixel to
the left, PAL-DV co-sites Cb and Cr on alternating lines; treating them as centred shifts chroma by at most half a chroma
sample, and the output carries the input's tag, so the same convention applies on both sides of the network.

Depth 10 (`depth=10` on every function below; the default 8 is everything above, unchanged).  Planes are uint16 and a
sample s is read as min(s, 1023): the top six bits of a stored word are not trusted.  The formulas are the ones above with
maxv = 1023 for 255 and the chroma midpoint 512 for 128; limited range is yo = 64, ys = 1023/876, cs = 1023/896,
yi = 876/1023, ci = 896/1023, full range yo = 0 and scales 1.  S and q() stay, so the tables depend on the depth (bt601
limited cy is 19133 at depth 10, 19077 at depth 8); the U and V rows still sum to exactly 0 in all four tables, a grey
ramp over the legal luma range decodes to R = G = B and encodes back to the same planes, every sum stays below 6.8e7 in
magnitude (int32) and the largest coefficient is 34711.  The network sees RGB10 / 1023.0f and its output is quantised as
round_half_even(clamp(v, 0, 1) * 1023).  In files a 10-bit sample is a little-endian 16-bit word (yuv420p10le, Y4M
C420p10).  Depth 12 is not offered: with S = 14 the bt709 limited V row sums to 1 and the bt601 limited grey ramp no
longer round-trips, so 12 bits would need another S, which is another definition.
"""
import collections
import os
import sys

import numpy as np

S = 14
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}

DecodeCoeffs = collections.namedtuple("DecodeCoeffs", "yo cy rv gu gv bu")
EncodeCoeffs = collections.namedtuple("EncodeCoeffs", "yo yr yg yb ur ug ub vr vg vb")


def _q(v):
    return int(round(v * 2 ** S))


DEPTHS = (8, 10)


def _depth(depth):
    """(largest sample value, chroma midpoint, numpy sample type) of a depth; refuses any other than 8 and 10"""
    if isinstance(depth, bool) or depth not in DEPTHS:
        raise ValueError("depth must be 8 or 10, got %r" % (depth,))
    return (255, 128, np.uint8) if depth == 8 else (1023, 512, np.uint16)


def yuv_coeffs(matrix="bt601", full_range=False, depth=8):
    """(DecodeCoeffs, EncodeCoeffs): the two integer tables of one matrix / range / depth, in the field order the kernels
    take"""
    maxv = float(_depth(depth)[0])
    if matrix not in MATRICES:
        raise ValueError("matrix must be one of %s, got %r" % (sorted(MATRICES), matrix))
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    if full_range:
        yo, ys, cs, yi, ci = 0, 1.0, 1.0, 1.0, 1.0
    else:
        k = 1 << (depth - 8)                          # limited range at depth d is the 8-bit one times 2^(d - 8)
        yo, ys, cs, yi, ci = 16 * k, maxv / (219.0 * k), maxv / (224.0 * k), 219.0 * k / maxv, 224.0 * k / maxv
    dec = DecodeCoeffs(yo, _q(ys), _q(cs * 2 * (1 - kr)), _q(-cs * 2 * (1 - kb) * kb / kg),
                       _q(-cs * 2 * (1 - kr) * kr / kg), _q(cs * 2 * (1 - kb)))
    enc = EncodeCoeffs(yo, _q(yi * kr), _q(yi * kg), _q(yi * kb),
                       _q(-ci * kr / (2 * (1 - kb))), _q(-ci * kg / (2 * (1 - kb))), _q(ci / 2),
                       _q(ci / 2), _q(-ci * kg / (2 * (1 - kr))), _q(-ci * kb / (2 * (1 - kr))))
    return dec, enc


def _planes(y, u, v, depth=8):
    dt = _depth(depth)[2]
    y, u, v = (np.asarray(p) for p in (y, u, v))
    if y.ndim != 2 or y.dtype != dt or u.dtype != dt or v.dtype != dt:
        raise ValueError("a %d-bit YUV 4:2:0 frame is three 2-D %s planes" % (depth, np.dtype(dt).name))
    H, W = y.shape
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError("a YUV 4:2:0 frame needs even sides, got %dx%d" % (W, H))
    if u.shape != (H // 2, W // 2) or v.shape != (H // 2, W // 2):
        raise ValueError("chroma planes must be %dx%d for a %dx%d frame, got %s and %s"
                         % (W // 2, H // 2, W, H, u.shape, v.shape))
    return y, u, v


def upsample_chroma_host(c, H, W, depth=8):
    """[H/2, W/2] -> [H, W] int32 by the centre-sited 9-3-3-1 filter with edge replication (samples read as
    min(s, 2^depth - 1))"""
    c = np.minimum(np.asarray(c), _depth(depth)[0]).astype(np.int32)
    CH, CW = c.shape

    def taps(L, n):
        p = np.arange(L)
        c0 = p >> 1
        return c0, np.clip(np.where(p % 2 == 0, c0 - 1, c0 + 1), 0, n - 1)

    cy0, ny = taps(H, CH)
    cx0, nx = taps(W, CW)
    return (9 * c[cy0][:, cx0] + 3 * c[cy0][:, nx] + 3 * c[ny][:, cx0] + c[ny][:, nx] + 8) >> 4


def yuv420_to_rgb_host(y, u, v, matrix="bt601", full_range=False, depth=8):
    """planes y [H, W], u, v [H/2, W/2] (uint8; uint16 at depth 10) -> HWC RGB [H, W, 3] of the same type, 0 .. 2^depth - 1:
    the definition of the decode"""
    maxv, mid, dt = _depth(depth)
    y, u, v = _planes(y, u, v, depth)
    d, _ = yuv_coeffs(matrix, full_range, depth)
    H, W = y.shape
    yy = np.minimum(y, maxv).astype(np.int32) - d.yo
    uu = upsample_chroma_host(u, H, W, depth) - mid
    vv = upsample_chroma_host(v, H, W, depth) - mid
    half = 1 << (S - 1)
    r = (d.cy * yy + d.rv * vv + half) >> S
    g = (d.cy * yy + d.gu * uu + d.gv * vv + half) >> S
    b = (d.cy * yy + d.bu * uu + half) >> S
    return np.clip(np.stack([r, g, b], axis=2), 0, maxv).astype(dt)


def rgb_to_yuv420_host(rgb, matrix="bt601", full_range=False, depth=8):
    """HWC RGB [H, W, 3] (even sides; uint8, or uint16 read as min(s, 1023) at depth 10) -> planes (y [H, W], u [H/2, W/2],
    v [H/2, W/2]) of the same type: the definition of the encode"""
    maxv, mid, dt = _depth(depth)
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != dt:
        raise ValueError("rgb_to_yuv420_host takes an HWC %s RGB image at depth %d" % (np.dtype(dt).name, depth))
    H, W = rgb.shape[:2]
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError("a YUV 4:2:0 frame needs even sides, got %dx%d" % (W, H))
    _, e = yuv_coeffs(matrix, full_range, depth)
    p = np.minimum(rgb, maxv).astype(np.int32)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = np.clip(((e.yr * r + e.yg * g + e.yb * b + (1 << (S - 1))) >> S) + e.yo, 0, maxv).astype(dt)

    def box(cr, cg, cb):
        s = (cr * r + cg * g + cb * b).reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3))
        return np.clip(((s + (1 << (S + 1))) >> (S + 2)) + mid, 0, maxv).astype(dt)

    return y, box(e.ur, e.ug, e.ub), box(e.vr, e.vg, e.vb)


# ---------------------------------------------------------------------------------------------- window reuse
def window_support(y0, x0, h, w, H, W, depth=8):
    """((luma row 0, row 1, col 0, col 1), (chroma row 0, row 1, col 0, col 1)), all bounds inclusive: the samples of an
    H x W frame that the decode of the h x w window at (y0, x0) depends on -- what ofasr_tile_gather_yuv420 reads for
    it.  The origin is clamped into the frame as the gather clamps it.  Luma is the window itself; a chroma row enters
    through pixel rows y0 .. y0 + h - 1 as cy0 = y >> 1 or as its neighbour tap (cy0 - 1 for even y, cy0 + 1 for odd y,
    clamped into the plane), which together are rows max(0, (y0 - 1) >> 1) .. min(H/2 - 1, (y0 + h) >> 1); columns alike.
    The bounds count samples, so they are the same at either depth."""
    _depth(depth)
    y0, x0 = min(max(int(y0), 0), H - h), min(max(int(x0), 0), W - w)
    luma = (y0, y0 + h - 1, x0, x0 + w - 1)
    chroma = (max(0, (y0 - 1) >> 1), min(H // 2 - 1, (y0 + h) >> 1), max(0, (x0 - 1) >> 1), min(W // 2 - 1, (x0 + w) >> 1))
    return luma, chroma


def changed_windows_host(prev, cur, origins, h, w, depth=8):
    """prev, cur: (y, u, v) planes of two equally sized frames; origins: [(y0, x0)] of h x w windows -> a bool array, one
    per window: True iff any byte of the window's support (window_support) differs between the two frames, in y, u or v.
    The definition of ofasr_window_diff_yuv420 and, at depth 10, of ofasr_window_diff_yuv420p16: there the stored 16-bit
    words are compared as they are, bits above the tenth included, which flags no fewer windows than comparing
    min(s, 1023) would."""
    prev, cur = _planes(*prev, depth=depth), _planes(*cur, depth=depth)
    if prev[0].shape != cur[0].shape:
        raise ValueError("the two frames differ in size: %s and %s" % (prev[0].shape, cur[0].shape))
    H, W = cur[0].shape
    if not (0 < h <= H and 0 < w <= W):
        raise ValueError("window %dx%d does not fit the %dx%d frame" % (w, h, W, H))
    diff = [a != b for a, b in zip(prev, cur)]
    out = np.zeros(len(origins), dtype=bool)
    for i, (y0, x0) in enumerate(origins):
        (r0, r1, c0, c1), (s0, s1, d0, d1) = window_support(y0, x0, h, w, H, W, depth)
        out[i] = diff[0][r0:r1 + 1, c0:c1 + 1].any() or diff[1][s0:s1 + 1, d0:d1 + 1].any() or \
            diff[2][s0:s1 + 1, d0:d1 + 1].any()
    return out


# ---------------------------------------------------------------------------------------------- files
Y4M_MAGIC = b"YUV4MPEG2"
Y4M_CHROMA = ("420jpeg", "420mpeg2", "420paldv", "420")   # 8-bit 4:2:0, all read as centre-sited (see the module text)
Y4M_CHROMA10 = ("420p10",)                                 # 10-bit 4:2:0 in little-endian 16-bit words, read alike
_MAX_LINE = 4096


def frame_bytes(width, height, depth=8):
    _depth(depth)
    return width * height * 3 // 2 * (1 if depth == 8 else 2)


def _chroma_depth(chroma):
    """the depth a Y4M chroma tag stands for, None for a tag that is not supported"""
    return 8 if chroma in Y4M_CHROMA else 10 if chroma in Y4M_CHROMA10 else None


def _check_size(width, height, what):
    if width < 2 or height < 2 or width % 2 or height % 2:
        raise ValueError("%s: 4:2:0 needs even, positive sides, got W%d H%d" % (what, width, height))


def split_frame(buf, width, height, depth=8):
    """views (y, u, v) of one frame's bytes (a 1-D uint8 array of frame_bytes(width, height, depth): a numpy array or a
    torch tensor); at depth 10 the views are uint16, the file's little-endian words read on a little-endian host"""
    if depth != 8:
        _depth(depth)
        if sys.byteorder != "little":
            raise ValueError("10-bit frames are little-endian words; this host is not little-endian")
        buf = buf.view(np.uint16) if isinstance(buf, np.ndarray) else buf.view(sys.modules["torch"].uint16)
    n = width * height
    return (buf[:n].reshape(height, width), buf[n:n + n // 4].reshape(height // 2, width // 2),
            buf[n + n // 4:n + n // 2].reshape(height // 2, width // 2))


class _FrameReader(object):
    """one frame in memory at a time; read_frame(out=None) -> (y, u, v) views of `out` (a 1-D uint8 array of
    frame_bytes, e.g. a view of pinned memory) or of a fresh array, None at the end of the file; uint16 views at depth 10"""
    width = height = 0
    depth = 8

    def __init__(self, path):
        self.path = path
        self._f = open(path, "rb")
        self.frames_read = 0

    def _before_frame(self):
        return True

    def _payload(self, out):
        n = frame_bytes(self.width, self.height, self.depth)
        if out is None:
            out = np.empty(n, dtype=np.uint8)
        elif out.dtype != np.uint8 or out.ndim != 1 or out.size != n or not out.flags.c_contiguous:
            raise ValueError("the frame buffer must be a contiguous 1-D uint8 array of %d bytes" % n)
        got, view = 0, memoryview(out)
        while got < n:
            k = self._f.readinto(view[got:])
            if not k:
                break
            got += k
        return got, out

    def read_frame(self, out=None):
        if not self._before_frame():
            return None
        got, out = self._payload(out)
        n = frame_bytes(self.width, self.height, self.depth)
        if got == 0 and self._eof_ok_without_payload():
            return None
        if got != n:
            raise ValueError("%s: frame %d is truncated (%d of %d bytes)" % (self.path, self.frames_read, got, n))
        self.frames_read += 1
        return split_frame(out, self.width, self.height, self.depth)

    def _eof_ok_without_payload(self):
        return True

    def skip_frame(self):
        """advance past one frame without keeping it; False at the end of the file"""
        return self.read_frame() is not None

    def __iter__(self):
        while True:
            fr = self.read_frame()
            if fr is None:
                return
            yield fr

    def close(self):
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MReader(_FrameReader):
    """streaming YUV4MPEG2 reader.  Header tags: W, H (required), F (frame rate "num:den"), I (interlacing), A (pixel
    aspect), C (chroma format; absent means 420jpeg), X (comments, kept in order in `xtags`).  The parameters of the
    FRAME line of the frame read last are in `frame_params`.  Only 8-bit 4:2:0 is accepted, unless `depths` (the accepted
    depths, a tuple of 8 and / or 10) says otherwise: with 10 in it a C420p10 file is read as uint16 planes, and `depth` says
    which of the two the file is."""

    def __init__(self, path, depths=(8,)):
        for d in depths:
            _depth(d)
        super(Y4MReader, self).__init__(path)
        try:
            line = self._line()
            tags = line.split(b" ")
            if tags[0] != Y4M_MAGIC:
                raise ValueError("%s: not a YUV4MPEG2 file" % path)
            self.fps = self.interlace = self.aspect = None
            self.chroma = "420jpeg"
            self.xtags = []
            width = height = None
            for t in tags[1:]:
                if not t:
                    continue
                k, val = t[:1], t[1:].decode("ascii", "replace")
                if k == b"W":
                    width = int(val)
                elif k == b"H":
                    height = int(val)
                elif k == b"F":
                    self.fps = val
                elif k == b"I":
                    self.interlace = val
                elif k == b"A":
                    self.aspect = val
                elif k == b"C":
                    self.chroma = val
                elif k == b"X":
                    self.xtags.append(val)
                else:
                    raise ValueError("%s: unknown header tag %r" % (path, t.decode("ascii", "replace")))
            if width is None or height is None:
                raise ValueError("%s: the header has no W / H tag" % path)
            depth = _chroma_depth(self.chroma)
            if depth not in depths:
                ok = [c for c in Y4M_CHROMA + Y4M_CHROMA10 if _chroma_depth(c) in depths]
                raise ValueError("%s: chroma format C%s is not supported (%s-bit 4:2:0 only: %s)"
                                 % (path, self.chroma, " or ".join(str(d) for d in sorted(depths)),
                                    ", ".join("C" + c for c in ok)))
            self.depth = depth
            _check_size(width, height, path)
            self.width, self.height = width, height
            self.frame_params = ""
        except Exception:
            self._f.close()
            raise

    def _line(self):
        line = self._f.readline(_MAX_LINE)
        if line and not line.endswith(b"\n"):
            raise ValueError("%s: truncated or overlong header line" % self.path)
        return line[:-1]

    def _before_frame(self):
        raw = self._f.readline(_MAX_LINE)
        if not raw:
            return False
        if not raw.endswith(b"\n") or not (raw[:-1] == b"FRAME" or raw.startswith(b"FRAME ")):
            raise ValueError("%s: frame %d: bad or truncated FRAME line %r" % (self.path, self.frames_read, raw[:32]))
        self.frame_params = raw[6:-1].decode("ascii", "replace")
        return True

    def _eof_ok_without_payload(self):
        return False      # a FRAME line was read: its payload must follow


class RawYUV420Reader(_FrameReader):
    """headerless planar yuv420p (yuv420p10le at depth 10): frames of width * height * 3 / 2 samples; the file must hold
    a whole number of them"""

    def __init__(self, path, width, height, depth=8):
        _check_size(width, height, path)
        size = os.path.getsize(path)
        n = frame_bytes(width, height, depth)
        if size == 0 or size % n:
            raise ValueError("%s: %d bytes is not a whole number of %dx%d %s frames (%d bytes each)"
                             % (path, size, width, height, "yuv420p" if depth == 8 else "yuv420p10le", n))
        super(RawYUV420Reader, self).__init__(path)
        self.width, self.height, self.depth = width, height, depth
        self.frames = size // n

    def skip_frame(self):
        if self.frames_read >= self.frames:
            return False
        self._f.seek(frame_bytes(self.width, self.height, self.depth), os.SEEK_CUR)
        self.frames_read += 1
        return True


class _FrameWriter(object):
    def __init__(self, path, width, height, depth=8):
        _check_size(width, height, path)
        self._dtype = np.dtype(_depth(depth)[2]).newbyteorder("<") if depth != 8 else np.dtype(np.uint8)
        self.path, self.width, self.height, self.depth = path, width, height, depth
        self._f = open(path, "wb")
        self.frames_written = 0

    def _plane(self, p, shape):
        p = np.ascontiguousarray(p)
        if p.dtype != self._dtype or p.shape != shape:
            raise ValueError("%s: expected a %s plane of shape %s, got %s %s"
                             % (self.path, self._dtype.name, shape, p.dtype, p.shape))
        return p.astype(self._dtype, copy=False)       # little-endian words in the file, whatever the host

    def _write_planes(self, y, u, v):
        H, W = self.height, self.width
        for p, shape in ((y, (H, W)), (u, (H // 2, W // 2)), (v, (H // 2, W // 2))):
            self._f.write(memoryview(self._plane(p, shape)).cast("B"))
        self.frames_written += 1

    def close(self):
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MWriter(_FrameWriter):
    """streaming YUV4MPEG2 writer; fps / interlace / aspect / chroma / xtags as Y4MReader reports them (None: tag left
    out).  depth=10 goes with chroma="420p10" and uint16 planes; a tag that disagrees with the depth is refused."""

    def __init__(self, path, width, height, fps=None, interlace=None, aspect=None, chroma="420jpeg", xtags=(), depth=8):
        _depth(depth)
        if _chroma_depth(chroma) != depth:
            raise ValueError("chroma format C%s is not supported at depth %d (%s)"
                             % (chroma, depth, ", ".join("C" + c for c in (Y4M_CHROMA if depth == 8 else Y4M_CHROMA10))))
        super(Y4MWriter, self).__init__(path, width, height, depth)
        tags = ["W%d" % width, "H%d" % height]
        for k, val in (("F", fps), ("I", interlace), ("A", aspect), ("C", chroma)):
            if val is not None:
                tags.append(k + str(val))
        tags += ["X" + str(x) for x in xtags]
        self._f.write(Y4M_MAGIC + b" " + " ".join(tags).encode("ascii") + b"\n")

    def write_frame(self, y, u, v, params=""):
        self._f.write(b"FRAME" + ((" " + params).encode("ascii") if params else b"") + b"\n")
        self._write_planes(y, u, v)


class RawYUV420Writer(_FrameWriter):
    def write_frame(self, y, u, v, params=""):
        self._write_planes(y, u, v)


def open_reader(path, size=None, depth=None):
    """Y4MReader for *.y4m (8-bit or C420p10; with `depth` given, a file of the other depth is refused);
    RawYUV420Reader otherwise (size = (width, height) required; `depth` None means 8)"""
    if path.lower().endswith(".y4m"):
        return Y4MReader(path, DEPTHS if depth is None else (depth,))
    if size is None:
        raise ValueError("%s: a headerless yuv420p file needs its frame size (WxH)" % path)
    return RawYUV420Reader(path, size[0], size[1], 8 if depth is None else depth)
