"""The training augmentation of div2k_setxx.py -- RandomCrop(size) -> RandomHorizontalFlip -> RandomRotation((-90, 90))
-- stated once more as integer arithmetic on arrays, and the loader that runs it on the GPU over a resident training set
(csrc/augment.hip, ops.aug_gather_u8).  The PIL provider stays the reference statement; everything here is pinned to it
bit for bit (tests/test_augment.py on the host, tests/test_hip_augment.py on the GPU).

The rotation.  Image.rotate(angle, NEAREST, expand=False) reduces the angle modulo 360, copies for 0, transposes for 180
(and for 90 / 270 on a square image), and otherwise builds the 2x3 matrix of the inverse map in Python doubles rounded to
15 digits; for images below 32768 pixels per side Pillow's affine_fixed (Geometry.c) walks it in 16.16 fixed point:
    xin = (a2 + y*a1 + x*a0) >> 16,  yin = (a5 + y*a4 + x*a3) >> 16,  out[y][x] = in[yin][xin] inside the image, else 0
with a_k = floor(m_k * 65536 + 0.5) and half a pixel folded into a2 / a5.  The transposes fit the same form with integer
coefficients, so one gather serves every angle: the host computes six ints per sample (rotate_coeffs) and the kernel is
the same code for all of them.

Video.  The same gather runs on a pool of raw 8-bit YUV 4:2:0 frames with video.py's colour decode fused in
(ofasr_aug_gather_yuv420, ops.aug_gather_yuv420, ResidentVideoSet): gather_yuv420_np is its definition on the pool's
bytes and apply_params_yuv420_np the same thing said as "the transforms of the decoded whole frame"
(tests/test_video_train.py on the host, tests/test_hip_video_train.py on the GPU).

Paired video.  A source video and its decoded low-resolution stream give the HR and the LR crop of ONE draw in one launch
(ofasr_aug_gather_yuv420_pair, ops.aug_gather_yuv420_pair, ResidentVideoPairSet); the definition -- the pair, the draw,
the sample, registration -- stands before draw_pair_params below (tests/test_video_pair.py on the host,
tests/test_hip_video_pair.py on the GPU).

Best of K.  ResidentTrainLoader(candidates=K) draws K parameter sets per sample and the GPU keeps the one whose crop
rectangle holds the most luma detail (ofasr_aug_select, ops.aug_select) before the unchanged gather runs; the definition
stands before aug_select_strips below, aug_select_np restates the kernel on the pool's bytes (tests/test_crop_select.py
on the host, tests/test_hip_crop_select.py on the GPU).
"""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ... import degrade as _degrade

try:
    from PIL import Image
except ImportError:   # pragma: no cover
    Image = None

MAX_SIDE = 4096           # ofasr_aug_gather_u8's limit on the crop side (the fixed-point walk stays inside int32)
TABLE_COLS = 12           # offset, H, W, i, j, flip, a0 .. a5
DECODE_THREADS = 16       # a job may use 16 CPUs whatever os.cpu_count() says


def _fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def _matrix_coeffs(angle, w, h):
    """the six 16.16 coefficients of Pillow's generic path for a w x h canvas (angle already reduced modulo 360)"""
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return (_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
            _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def rotate_coeffs(angle, S):
    """(a0, a1, a2, a3, a4, a5) of Image.rotate(angle, NEAREST) on an S x S canvas.  Pillow's shortcut angles are exact
    integer maps: 0 is a copy, 180 is ROTATE_180, 90 / 270 on the square canvas are ROTATE_90 / ROTATE_270."""
    S = int(S)
    if not 0 < S <= MAX_SIDE:
        raise ValueError("rotate_coeffs: canvas side %d outside 1 .. %d" % (S, MAX_SIDE))
    angle = angle % 360.0
    one, half, far = 65536, 32768, (S - 1) * 65536 + 32768
    if angle == 0:
        return (one, 0, half, 0, one, half)                 # xin = x,       yin = y
    if angle == 180:
        return (-one, 0, far, 0, -one, far)                 # xin = S-1-x,   yin = S-1-y
    if angle == 90:
        return (0, -one, far, one, 0, half)                 # xin = S-1-y,   yin = x      (counter-clockwise)
    if angle == 270:
        return (0, one, half, -one, 0, far)                 # xin = y,       yin = S-1-x
    return _matrix_coeffs(angle, S, S)


def walk_fixed_np(a, coeffs):
    """the fixed-point walk itself on an [H, W] or [H, W, C] array: the numpy statement of what the kernel does"""
    a = np.asarray(a)
    h, w = a.shape[:2]
    a0, a1, a2, a3, a4, a5 = (int(c) for c in coeffs)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    xin = (a2 + y * a1 + x * a0) >> 16
    yin = (a5 + y * a4 + x * a3) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    g = a[np.clip(yin, 0, h - 1), np.clip(xin, 0, w - 1)]
    return np.where(ok if a.ndim == 2 else ok[:, :, None], g, np.zeros((), a.dtype)).astype(a.dtype)


def rotate_nearest_np(a, angle):
    """Image.fromarray(a).rotate(angle, Image.NEAREST, False, None) as numpy, any height and width below 32768"""
    a = np.asarray(a)
    h, w = a.shape[:2]
    angle = angle % 360.0
    if angle == 0:
        return a.copy()
    if angle == 180:
        return np.ascontiguousarray(a[::-1, ::-1])
    if angle in (90, 270) and w == h:
        return np.ascontiguousarray(np.rot90(a, 1 if angle == 90 else 3))
    return walk_fixed_np(a, _matrix_coeffs(angle, w, h))


def draw_train_params(h, w, size):
    """(i, j, flip, angle) drawn from the torch global RNG exactly as Compose([RandomCrop(size), RandomHorizontalFlip(),
    RandomRotation((-90, 90))]) of div2k_setxx.py draws them on an h x w image: two randint for the corner (none when
    the image already has the crop's size), rand(1) < 0.5, uniform_(-90, 90)."""
    size = int(size)
    if h < size or w < size:
        raise ValueError("Required crop size %s is larger than input image size %s" % ((size, size), (h, w)))
    i = j = 0
    if not (w == size and h == size):
        i = int(torch.randint(0, h - size + 1, size=(1,)).item())
        j = int(torch.randint(0, w - size + 1, size=(1,)).item())
    flip = bool(torch.rand(1) < 0.5)
    angle = float(torch.empty(1).uniform_(-90.0, 90.0).item())
    return i, j, flip, angle


def apply_params_np(img, size, params):
    """the three transforms on an [H, W, 3] uint8 array -> [size, size, 3]"""
    i, j, flip, angle = params
    a = np.asarray(img)[i:i + size, j:j + size]
    if flip:
        a = a[:, ::-1]
    return rotate_nearest_np(a, angle)


def table_row(offset, H, W, size, params, yuv420=False):
    """one row of the gathers' table (ofasr_aug_gather_u8; with `yuv420`, ofasr_aug_gather_yuv420, whose frames have
    even sides); refuses what the kernel would have to clamp"""
    i, j, flip, angle = params
    if H < size or W < size:
        raise ValueError("aug_gather_u8: image %dx%d is smaller than the %dx%d crop" % (H, W, size, size))
    if not (0 <= i <= H - size and 0 <= j <= W - size):
        raise ValueError("aug_gather_u8: crop corner (%d, %d) outside the %dx%d image" % (i, j, H, W))
    if yuv420 and (H % 2 or W % 2):
        raise ValueError("aug_gather_yuv420: a 4:2:0 frame needs even sides, got %dx%d" % (W, H))
    return (int(offset), int(H), int(W), int(i), int(j), int(bool(flip))) + tuple(rotate_coeffs(angle, size))


def make_table(rows, size, out=None, yuv420=False):
    """int64 [n, 12] host table from (offset, H, W, (i, j, flip, angle)) entries; `yuv420`: the entries are frames of a
    planar YUV 4:2:0 pool (offset = the Y plane's), odd sides are refused"""
    vals = [table_row(o, H, W, size, p, yuv420) for (o, H, W, p) in rows]
    t = torch.tensor(vals, dtype=torch.int64).reshape(len(vals), TABLE_COLS)
    if out is None:
        return t
    out[:len(vals)].copy_(t)
    return out[:len(vals)]


# ------------------------------------------------------------------------------------- planar YUV 4:2:0 frames
def apply_params_yuv420_np(y, u, v, size, params, matrix="bt601", full_range=False):
    """the three transforms on the decode of one frame (video.yuv420_to_rgb_host of the WHOLE frame, so chroma replicates
    at the frame's edge and its parity is the frame coordinate's) -> [size, size, 3]"""
    from ... import video
    return apply_params_np(video.yuv420_to_rgb_host(y, u, v, matrix, full_range), size, params)


def gather_yuv420_np(pool_bytes, table, S, coeffs):
    """ofasr_aug_gather_yuv420 restated on the pool's bytes (a 1-D uint8 array), clamping rules included: the
    definition.  `table`: int64 [n, 12]; `coeffs`: the six decode coefficients (video.yuv_coeffs(...)[0]).  A frame is
    Y [H, W], U [H/2, W/2], V [H/2, W/2] from its offset on.  With Se = S rounded up to even: H = clamp(H, Se, 2^24) & ~1
    and W alike, (i, j) into [0, H - S] x [0, W - S], offset into [0, pool bytes], the six rotation coefficients taken
    modulo 2^32 (the walk wraps in uint32), and every sample's byte address into [0, pool bytes - 1]."""
    pool = np.asarray(pool_bytes, dtype=np.uint8).reshape(-1)
    nb, S = int(pool.size), int(S)
    yo, cy, rv, gu, gv, bu = (int(c) for c in coeffs)
    y, x = np.mgrid[0:S, 0:S].astype(np.int64)
    Se, lim, m32 = (S + 1) & ~1, 1 << 24, 0xffffffff
    table = np.asarray(table, dtype=np.int64).reshape(-1, TABLE_COLS)
    out = np.zeros((len(table), 3, S, S), np.uint8)

    def walk(c, cy_, cx_):
        w = ((c & m32) + y * (cy_ & m32) + x * (cx_ & m32)) & m32
        return (w - ((w >> 31) << 32)) >> 16                      # as int32, arithmetic shift

    def tap(p, last):
        c0 = p >> 1
        return c0, np.clip(np.where(p & 1, c0 + 1, c0 - 1), 0, last)

    for n, row in enumerate(table):
        off, H, W, i, j, flip, a0, a1, a2, a3, a4, a5 = (int(v) for v in row)
        H, W = min(max(H, Se), lim) & ~1, min(max(W, Se), lim) & ~1
        i, j = min(max(i, 0), H - S), min(max(j, 0), W - S)
        off = min(max(off, 0), nb)
        xin, yin = walk(a2, a1, a0), walk(a5, a4, a3)
        ok = (xin >= 0) & (xin < S) & (yin >= 0) & (yin < S)
        xc, yc = np.clip(xin, 0, S - 1), np.clip(yin, 0, S - 1)
        py, px = i + yc, j + (S - 1 - xc if flip else xc)
        CH, CW = H >> 1, W >> 1
        r0, r1 = tap(py, CH - 1)
        c0, c1 = tap(px, CW - 1)

        def at(b):
            return pool[np.minimum(b, nb - 1)].astype(np.int32)

        def chroma(base):
            return ((9 * at(base + r0 * CW + c0) + 3 * at(base + r0 * CW + c1) + 3 * at(base + r1 * CW + c0)
                     + at(base + r1 * CW + c1) + 8) >> 4) - 128

        ub = off + H * W
        uu, vv = chroma(ub), chroma(ub + CH * CW)
        l = cy * (at(off + py * W + px) - yo) + (1 << 13)
        for c, val in enumerate(((l + rv * vv) >> 14, (l + gu * uu + gv * vv) >> 14, (l + bu * uu) >> 14)):
            out[n, c] = np.where(ok, np.clip(val, 0, 255), 0)
    return out


# ------------------------------------------------------------------------------------- paired HR / LR frames
# The pair.  An HR video of H x W and an LR video of h x w -- the low-resolution stream after a codec, decoded -- with
# H = f*h, W = f*w, f in {2, 4}, all four sides even, both 8-bit 4:2:0 with the same number of frames; all pairs of one
# run share one f (video_pair_layout refuses the rest and names the files and the sizes).  One colour definition
# (matrix, range) serves both sides.
#
# The draw.  draw_pair_params(h, w, S, f) needs S % f == 0, has s = S // f and draws ON THE LR GRID with the calls of
# draw_train_params(h, w, s), in that order; it returns (i, j, flip, angle) of the LR crop, and the HR crop's parameters
# are (f*i, f*j, flip, angle) at side S (pair_hr_params).  The RNG consumption is that of the unpaired path on an h x w
# image with crop s.
#
# The sample.  HR = apply_params_yuv420_np(HR frame, S, (f*i, f*j, flip, angle)), LR = apply_params_yuv420_np(LR frame,
# s, (i, j, flip, angle)): each the three PIL transforms of the decode of its OWN whole frame, so i, j may be odd and
# chroma parity and edge replication are the frame's.
#
# Registration.  With angle = 0 the LR crop [i, i+s) x [j, j+s) covers exactly the HR crop [f*i, f*i+S) x [f*j, f*j+S),
# flipped or not.  With a free angle the two nearest-neighbour rotations are PIL's on each canvas about the same centre,
# each sampling its own grid: from pixel to pixel LR and HR can then disagree by up to half an LR pixel.  rotate=False
# sets the angle to 0.0 AFTER it has been drawn, so the RNG sequence does not move: the setting for artefact restoration.
PAIR_SCALES = (2, 4)


def _pair_sides(S, f):
    S, f = int(S), int(f)
    if f not in PAIR_SCALES:
        raise ValueError("a paired sample has scale 2 or 4, got %d" % f)
    if S <= 0 or S % f:
        raise ValueError("a paired sample's crop side %d must be a positive multiple of its scale %d" % (S, f))
    return S, f, S // f


def draw_pair_params(h, w, S, f, rotate=True):
    """(i, j, flip, angle) of the LR crop of side S // f on the h x w LR frame, drawn exactly as
    draw_train_params(h, w, S // f) draws; `rotate=False` replaces the drawn angle by 0.0 afterwards"""
    S, f, s = _pair_sides(S, f)
    i, j, flip, angle = draw_train_params(h, w, s)
    return i, j, flip, (angle if rotate else 0.0)


def pair_hr_params(params, f):
    """the HR crop's parameters of the LR crop's `params`"""
    i, j, flip, angle = params
    return int(f) * i, int(f) * j, flip, angle


def apply_pair_params_np(hr_planes, lr_planes, S, f, params, matrix="bt601", full_range=False):
    """the paired sample of the LR-grid `params`: ([S, S, 3], [S/f, S/f, 3]), each side the transforms of the decode of
    its own whole frame ((y, u, v) planes)"""
    S, f, s = _pair_sides(S, f)
    return (apply_params_yuv420_np(*hr_planes, size=S, params=pair_hr_params(params, f), matrix=matrix, full_range=full_range),
            apply_params_yuv420_np(*lr_planes, size=s, params=params, matrix=matrix, full_range=full_range))


def make_pair_table(rows, S, f, out=None):
    """int64 [2, n, 12] host table of ofasr_aug_gather_yuv420_pair from (HR offset, H, W, LR offset, h, w, (i, j, flip,
    angle) on the LR grid) entries: block 0 the HR rows at side S, block 1 the LR rows at side S / f, both through
    table_row, which keeps all its refusals.  `out`: an int64 [>= 2n, 12] buffer to build it in."""
    S, f, s = _pair_sides(S, f)
    hr, lr = [], []
    for (ho, H, W, lo, h, w, p) in rows:
        if H != f * h or W != f * w:
            raise ValueError("aug_gather_yuv420_pair: an HR frame of %dx%d is not %d times its LR frame of %dx%d"
                             % (W, H, f, w, h))
        hr.append(table_row(ho, H, W, S, pair_hr_params(p, f), True))
        lr.append(table_row(lo, h, w, s, p, True))
    n = len(hr)
    t = torch.tensor(hr + lr, dtype=torch.int64).reshape(2 * n, TABLE_COLS)
    if out is None:
        return t.view(2, n, TABLE_COLS)
    out[:2 * n].copy_(t)
    return out[:2 * n].view(2, n, TABLE_COLS)


def gather_yuv420_pair_np(hr_pool, lr_pool, table, S, f, coeffs):
    """ofasr_aug_gather_yuv420_pair restated on the pools' bytes: gather_yuv420_np of each pool and its block of the
    int64 [2, n, 12] table -> (uint8 [n, 3, S, S], uint8 [n, 3, S/f, S/f])"""
    S, f, s = _pair_sides(S, f)
    table = np.asarray(table, dtype=np.int64)
    if table.ndim != 3 or table.shape[0] != 2 or table.shape[2] != TABLE_COLS:
        raise ValueError("gather_yuv420_pair_np: table is [2, n, %d], got %s" % (TABLE_COLS, table.shape))
    return gather_yuv420_np(hr_pool, table[0], S, coeffs), gather_yuv420_np(lr_pool, table[1], s, coeffs)


# ------------------------------------------------------------------------------------- best of K candidate crops
# Candidates.  For each sample of a batch, in batch order, K parameter sets (i, j, flip, angle) are drawn one after
# another with the draw the sample would have had anyway (draw_train_params; draw_pair_params of a paired set, on its LR
# grid): all K of sample 0, then all K of sample 1.  With K = 1 that is the RNG sequence of a loader without candidates.
#
# Measure.  Candidate c scores the routing.py activity A of its S x S crop rectangle in the source frame, rows
# i .. i + S - 1, columns j .. j + S - 1, BEFORE flip and rotation: the sum of absolute luma differences of horizontally
# and vertically neighbouring samples with both samples inside the rectangle (crop_activity_np; it equals
# routing.window_activity_host(src, [(i, j)], S, S)[0]).  Luma of an RGB image: (77 R + 150 G + 29 B + 128) >> 8; of a
# 4:2:0 frame: the Y plane as stored; of a paired sample: the Y plane of the HR frame at (f i, f j), side S.
# A <= 510 S^2, above 2^32 at S = 4096: int64.
#
# Choice.  The largest A wins, ties go to the lowest candidate index (a flat image keeps its first draw), and the
# winner's whole parameter set, flip and angle included, is what the gather receives (select_candidates_np).
#
# aug_select_np restates the kernel (ofasr_aug_select) on the pool's bytes, the clamps of a device table included.
MAX_CANDIDATES = 16                 # ofasr_aug_select's limit on K
SELECT_STRIP_SAMPLES = 16384        # samples of a crop rectangle per workgroup of its first launch, about
SELECT_MAX_STRIPS = 64
LAYOUT_RGB, LAYOUT_YUV420 = "rgb", "yuv420"


def aug_select_strips(S):
    """the row strips ofasr_aug_select cuts an S x S rectangle into (include/ofasr.h states the function; the workspace
    is n * K * strips int64 words)"""
    S = int(S)
    return max(1, min(-(-S * S // SELECT_STRIP_SAMPLES), SELECT_MAX_STRIPS, S))


def check_candidates(K):
    K = int(K)
    if not 1 <= K <= MAX_CANDIDATES:
        raise ValueError("crop candidates per sample: %d outside 1 .. %d" % (K, MAX_CANDIDATES))
    return K


def draw_candidates(draw, K):
    """K parameter sets of one sample, drawn one after another by `draw()`"""
    return [draw() for _ in range(check_candidates(K))]


def crop_activity_np(src, params, S):
    """A of the S x S crop rectangle at params' (i, j) in `src`, an [H, W, 3] uint8 RGB image or a 2-D uint8 luma plane"""
    from ... import routing
    L = routing.luma_plane(src)
    i, j, S = int(params[0]), int(params[1]), int(S)
    if not (0 <= i <= L.shape[0] - S and 0 <= j <= L.shape[1] - S):
        raise ValueError("crop corner (%d, %d) of side %d outside the %dx%d image" % (i, j, S, L.shape[0], L.shape[1]))
    R = L[i:i + S, j:j + S]
    return int(np.abs(np.diff(R, axis=1)).sum()) + int(np.abs(np.diff(R, axis=0)).sum())


def select_candidates_np(srcs, cands, S):
    """(choice int32 [n], activity int64 [n, K]) of the K candidates cands[s] of each sample's source srcs[s] (an RGB image,
    a Y plane; for a paired sample the HR Y plane with the HR parameters, pair_hr_params)"""
    act = np.array([[crop_activity_np(src, p, S) for p in ps] for src, ps in zip(srcs, cands)], dtype=np.int64)
    act = act.reshape(len(cands), -1)
    return np.argmax(act, axis=1).astype(np.int32), act          # argmax: the first of equal maxima


def aug_select_np(pool_bytes, cand_table, n, K, S, layout):
    """ofasr_aug_select restated on the pool's bytes (a 1-D uint8 array), clamping rules included: (choice int32 [n],
    activity int64 [n, K], table int64 [blocks, n, 12]).  `cand_table`: int64 [blocks, n * K, 12], sample-major; `layout`:
    LAYOUT_RGB (HWC images, 3 bytes a sample) or LAYOUT_YUV420 (the Y plane of a frame, 1 byte a sample).  Per candidate,
    from block 0's row: H = clamp(H, S, 2^24) and W alike (yuv420: clamp(., Se, 2^24) & ~1, Se = S rounded up to even),
    (i, j) into [0, H - S] x [0, W - S], offset into [0, pool bytes], and the address of every byte read into
    [0, pool bytes - 1]."""
    pool = np.asarray(pool_bytes, dtype=np.uint8).reshape(-1)
    nb, n, K, S = int(pool.size), int(n), check_candidates(K), int(S)
    if layout not in (LAYOUT_RGB, LAYOUT_YUV420):
        raise ValueError("aug_select_np: layout is %r or %r, got %r" % (LAYOUT_RGB, LAYOUT_YUV420, layout))
    yuv = layout == LAYOUT_YUV420
    cand = np.asarray(cand_table, dtype=np.int64)
    cand = cand.reshape(-1, n * K, TABLE_COLS)
    bps, lim, Se = (1 if yuv else 3), 1 << 24, ((S + 1) & ~1 if yuv else S)
    r, c = np.mgrid[0:S, 0:S].astype(np.int64)
    act = np.zeros((n, K), np.int64)
    for q, row in enumerate(cand[0]):
        off, H, W, i, j = (int(v) for v in row[:5])
        H, W = min(max(H, Se), lim), min(max(W, Se), lim)
        if yuv:
            H, W = H & ~1, W & ~1
        i, j = min(max(i, 0), H - S), min(max(j, 0), W - S)
        off = min(max(off, 0), nb)
        a = off + ((i + r) * W + j + c) * bps

        def at(b):
            return pool[np.minimum(b, nb - 1)].astype(np.int64)

        L = at(a) if yuv else (77 * at(a) + 150 * at(a + 1) + 29 * at(a + 2) + 128) >> 8
        act[q // K, q % K] = int(np.abs(np.diff(L, axis=1)).sum()) + int(np.abs(np.diff(L, axis=0)).sum())
    choice = np.argmax(act, axis=1).astype(np.int32)
    pick = np.arange(n) * K + choice
    return choice, act, np.ascontiguousarray(cand[:, pick])


# ------------------------------------------------------------------------------------- the resident training set
class ResidentTrainSet(object):
    """Every training image decoded once (Image.open(p).convert("RGB"), on at most 16 threads) into ONE uint8 pool on
    `device`, packed HWC images back to back; `entries[k] = (offset, H, W)` stays on the host.  The decoded size is known
    from the file headers before anything is decoded: above `max_bytes` the constructor raises, it never truncates."""

    def __init__(self, paths, device, max_bytes=32 << 30, threads=DECODE_THREADS):
        if Image is None:
            raise ImportError("ResidentTrainSet needs PIL")
        self.paths = list(paths)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            from ... import _C
            raise _C.OfasrError("ResidentTrainSet keeps the images on the GPU (got device %s)" % (self.device,))
        if not self.paths:
            raise ValueError("ResidentTrainSet: no images")
        self.entries, total = [], 0
        for p in self.paths:
            with Image.open(p) as im:     # header only
                w, h = im.size
            self.entries.append((total, h, w))
            total += h * w * 3
        if total > max_bytes:
            raise MemoryError("ResidentTrainSet: %d images decode to %d bytes (%.2f GiB), above max_bytes = %d (%.2f GiB)"
                              % (len(self.paths), total, total / 2.0 ** 30, max_bytes, max_bytes / 2.0 ** 30))
        self.nbytes = total
        self.pool = torch.empty(total, dtype=torch.uint8, device=self.device)
        workers = max(1, min(int(threads), DECODE_THREADS, len(self.paths)))
        with ThreadPoolExecutor(max_workers=workers) as ex:
            # decoded images are uploaded as they arrive, in file order, so at most `workers` + a few wait on the host
            decoded = self._bounded_map(ex, self._decode, self.paths, 2 * workers)
            for p, (off, h, w), a in zip(self.paths, self.entries, decoded):
                if a.shape != (h, w, 3):
                    raise RuntimeError("ResidentTrainSet: %s decoded to %s, its header said %s" % (p, a.shape, (h, w, 3)))
                self.pool[off:off + h * w * 3].copy_(torch.from_numpy(a).reshape(-1))

    @staticmethod
    def _decode(path):
        return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8))

    @staticmethod
    def _bounded_map(ex, fn, items, ahead):
        pending, it = [], iter(items)
        for x in it:
            pending.append(ex.submit(fn, x))
            if len(pending) >= ahead:
                yield pending.pop(0).result()
        for f in pending:
            yield f.result()

    def __len__(self):
        return len(self.paths)

    def image_np(self, k):
        """image k back on the host as [H, W, 3] (tests and debugging)"""
        off, h, w = self.entries[k]
        return self.pool[off:off + h * w * 3].cpu().numpy().reshape(h, w, 3)


class ResidentArraySet(object):
    """ResidentTrainSet's pool from images that are decoded already: [H, W, 3] uint8 arrays, packed HWC back to back in
    ONE uint8 pool on `device`, `entries[k] = (offset, H, W)`, `paths[k]` = `names[k]` (the synthetic stand-in of the
    DIV2K provider under crop_candidates, and tests)."""

    def __init__(self, images, device, names=None):
        images = [np.ascontiguousarray(a) for a in images]
        if not images:
            raise ValueError("ResidentArraySet: no images")
        for a in images:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("ResidentArraySet: an image is an [H, W, 3] uint8 array, got %s %s" % (a.shape, a.dtype))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            from ... import _C
            raise _C.OfasrError("ResidentArraySet keeps the images on the GPU (got device %s)" % (self.device,))
        self.paths = ["array#%d" % k for k in range(len(images))] if names is None else list(names)
        self.entries, total = [], 0
        for a in images:
            self.entries.append((total, a.shape[0], a.shape[1]))
            total += a.size
        self.nbytes = total
        self.pool = torch.from_numpy(np.concatenate([a.reshape(-1) for a in images])).to(self.device)

    def __len__(self):
        return len(self.entries)

    def image_np(self, k):
        off, h, w = self.entries[k]
        return self.pool[off:off + h * w * 3].cpu().numpy().reshape(h, w, 3)


# ------------------------------------------------------------------------------------- the resident video frames
def count_frames(reader):
    """the number of frames of an open video.Y4MReader / RawYUV420Reader positioned before its first frame, from the
    header, the FRAME lines and the file size alone: no frame is read and the reader does not move"""
    if hasattr(reader, "frames"):
        return reader.frames
    from ... import video
    fb = video.frame_bytes(reader.width, reader.height, reader.depth)
    size, n = os.path.getsize(reader.path), 0
    with open(reader.path, "rb") as f:
        f.seek(reader._f.tell())
        while True:
            line = f.readline(4096)
            if not line:
                return n
            if not line.startswith(b"FRAME") or not line.endswith(b"\n") or f.tell() + fb > size:
                raise ValueError("%s: frame %d: bad or truncated frame" % (reader.path, n))
            f.seek(fb, os.SEEK_CUR)
            n += 1


def video_pool_layout(sources, max_bytes):
    """(entries, paths, total bytes, largest frame's bytes) of ResidentVideoSet's pool for `sources`, from headers, FRAME
    lines and file sizes: no frame is read.  Refuses a 10-bit source (ValueError) and a pool above `max_bytes`
    (MemoryError, which names the size)."""
    from ... import video
    entries, paths, total, largest = [], [], 0, 0
    for path, size, idx in sources:
        with video.open_reader(path, size) as r:
            if r.depth != 8:
                raise ValueError("%s is %d-bit: training input is 8-bit only, because the LR images are Pillow's 8-bit "
                                 "bicubic of the HR crop (ops.lr_images_from_u8)" % (path, r.depth))
            n, fb = count_frames(r), video.frame_bytes(r.width, r.height)
            idx = [int(k) for k in idx]
            if any(b <= a for a, b in zip(idx, idx[1:])) or (idx and not 0 <= idx[0] <= idx[-1] < n):
                raise ValueError("%s: frame indices must be strictly increasing inside 0 .. %d" % (path, n - 1))
            for k in idx:
                entries.append((total, r.height, r.width))
                paths.append("%s#%d" % (path, k))
                total += fb
            largest = max(largest, fb)
    if not entries:
        raise ValueError("ResidentVideoSet: no frames")
    if total > max_bytes:
        raise MemoryError("ResidentVideoSet: %d frames take %d bytes (%.2f GiB), above max_bytes = %d (%.2f GiB)"
                          % (len(entries), total, total / 2.0 ** 30, max_bytes, max_bytes / 2.0 ** 30))
    return entries, paths, total, largest


class ResidentVideoSet(object):
    """The selected frames of raw 8-bit YUV 4:2:0 videos in ONE uint8 pool on `device`, each frame's bytes as they are in
    the file (Y [H, W], U [H/2, W/2], V [H/2, W/2]), back to back: half the bytes of an RGB pool, and no RGB frame is ever
    formed -- `gather` decodes inside the augmentation gather (ops.aug_gather_yuv420) by video.py's pinned conversion,
    the one the tile gather of the upscaler feeds the network.  `sources` is a list of (path, (width, height) or None,
    frame indices, strictly increasing), opened through video.open_reader; `entries[k] = (offset of the Y plane, H, W)`
    and `paths[k]` names frame k ("file#index"), in source order.  The pool's size is known from the headers and the file
    sizes before any frame is read: above `max_bytes` the constructor raises, it never truncates.  Frames travel through
    one pinned staging buffer; frames that are not selected are skipped (skip_frame), not read."""
    yuv420 = True           # make_table: the entries are 4:2:0 frames

    def __init__(self, sources, device, matrix="bt601", full_range=False, max_bytes=32 << 30):
        from ... import video
        video.yuv_coeffs(matrix, full_range)        # refuses an unknown matrix here, not at the first batch
        self.matrix, self.full_range = matrix, bool(full_range)
        self.sources = [(p, None if sz is None else (int(sz[0]), int(sz[1])), [int(k) for k in idx])
                        for (p, sz, idx) in sources]
        # what the files are is checked before where they would go: a 10-bit source is refused on any device
        self.entries, self.paths, total, largest = video_pool_layout(self.sources, max_bytes)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            from ... import _C
            raise _C.OfasrError("ResidentVideoSet keeps the frames on the GPU (got device %s)" % (self.device,))
        self.nbytes = total
        self.pool = torch.empty(total, dtype=torch.uint8, device=self.device)
        stage = torch.empty(largest, dtype=torch.uint8).pin_memory()
        at = 0
        for path, size, idx in self.sources:
            with video.open_reader(path, size, depth=8) as r:
                for k in idx:
                    while r.frames_read < k:
                        if not r.skip_frame():
                            raise ValueError("%s ended before frame %d" % (path, k))
                    off, h, w = self.entries[at]
                    fb = video.frame_bytes(w, h)
                    if r.read_frame(out=stage.numpy()[:fb]) is None:
                        raise ValueError("%s ended before frame %d" % (path, k))
                    self.pool[off:off + fb].copy_(stage[:fb])      # synchronous: the staging buffer is free again
                    at += 1

    def __len__(self):
        return len(self.entries)

    def frame_planes_np(self, k):
        """frame k back on the host as its (y, u, v) planes"""
        from ... import video
        off, h, w = self.entries[k]
        return video.split_frame(self.pool[off:off + video.frame_bytes(w, h)].cpu().numpy(), w, h)

    def frame_planes(self, k):
        """frame k's (y, u, v) planes as views of the pool"""
        from ... import video
        off, h, w = self.entries[k]
        return video.split_frame(self.pool[off:off + video.frame_bytes(w, h)], w, h)

    def image_np(self, k):
        """frame k as [H, W, 3] RGB by the host definition (video.yuv420_to_rgb_host)"""
        from ... import video
        return video.yuv420_to_rgb_host(*self.frame_planes_np(k), matrix=self.matrix, full_range=self.full_range)

    def gather(self, table, n, S, want_f32=False):
        from ... import ops
        return ops.aug_gather_yuv420(self.pool, table, n, S, self.matrix, self.full_range, want_f32=want_f32)


def video_pair_layout(sources, lr_sources, max_bytes):
    """(f, HR layout, LR layout) of ResidentVideoPairSet's two pools, each layout as video_pool_layout gives it, from
    headers, FRAME lines and file sizes alone.  `sources` / `lr_sources`: (path, size, frame indices) per video, matched
    by position; the LR video of a pair is read at the HR video's frame indices.  Refuses (ValueError, naming the files
    and the sizes) another number of LR videos than HR videos, a 10-bit file on either side, different frame counts,
    sides that are not exactly 2 or 4 times the LR sides, and pairs of different scales; both pools together above
    `max_bytes` raise MemoryError."""
    from ... import video
    sources, lr_sources = list(sources), list(lr_sources)
    if len(sources) != len(lr_sources):
        raise ValueError("paired video: %d LR videos (%s) for %d HR videos (%s): they are matched by position"
                         % (len(lr_sources), ", ".join(s[0] for s in lr_sources), len(sources),
                            ", ".join(s[0] for s in sources)))
    scale = None
    for (hp, hsz, hidx), (lp, lsz, lidx) in zip(sources, lr_sources):
        if [int(k) for k in hidx] != [int(k) for k in lidx]:
            raise ValueError("paired video: %s and %s are read at different frame indices" % (hp, lp))
        with video.open_reader(hp, hsz) as hr, video.open_reader(lp, lsz) as lr:
            for r in (hr, lr):
                if r.depth != 8:
                    raise ValueError("%s is %d-bit: paired training input is 8-bit only on both sides (pair %s / %s)"
                                     % (r.path, r.depth, hp, lp))
            (H, W), (h, w) = (hr.height, hr.width), (lr.height, lr.width)
            what = "%s (%dx%d) / %s (%dx%d)" % (hp, W, H, lp, w, h)
            nh, nl = count_frames(hr), count_frames(lr)
        if nh != nl:
            raise ValueError("paired video: %s: %d frames against %d" % (what, nh, nl))
        f = H // h if h else 0
        if f not in PAIR_SCALES or H != f * h or W != f * w or any(v % 2 for v in (H, W, h, w)):
            raise ValueError("paired video: %s: the HR sides must be exactly 2 or 4 times the LR sides, all even" % what)
        if scale is not None and f != scale[0]:
            raise ValueError("paired video: %s is a x%d pair but %s is a x%d pair: one run has one scale"
                             % (what, f, scale[1], scale[0]))
        scale = scale or (f, what)
    if scale is None:
        raise ValueError("ResidentVideoPairSet: no videos")
    hl = video_pool_layout(sources, max_bytes)
    ll = video_pool_layout(lr_sources, max_bytes)
    if hl[2] + ll[2] > max_bytes:
        total = hl[2] + ll[2]
        raise MemoryError("ResidentVideoPairSet: %d frame pairs take %d + %d = %d bytes (%.2f GiB), above max_bytes = %d "
                          "(%.2f GiB)" % (len(hl[0]), hl[2], ll[2], total, total / 2.0 ** 30, max_bytes, max_bytes / 2.0 ** 30))
    return scale[0], hl, ll


class ResidentVideoPairSet(object):
    """The selected frames of HR videos and, at the same frame indices, of their decoded LR streams, in two
    ResidentVideoSet pools on `device` (both count against `max_bytes`: a x4 LR pool adds 1/16).  `entries`, `paths`,
    `pool`, `frame_planes`, `image_np` are the HR set's, as a ResidentVideoSet has them; `lr_entries`, `lr_pool`,
    `lr_frame_planes`, `lr_image_np` stand beside them; `scale` is f.  `gather` is one ofasr_aug_gather_yuv420_pair
    launch.  A ResidentTrainLoader over this set draws with draw_pair_params (`rotate=False`: the drawn angle becomes
    0.0), builds the [2, n, 12] table (make_pair_table) and yields {'image_u8', 'lr_u8', 'lr_scale'} (+ 'image', 'lr',
    the fp32 batches, with want_f32)."""
    yuv420 = True
    TABLE_BLOCKS = 2        # ResidentTrainLoader: rows of pinned table per sample

    def __init__(self, sources, lr_sources, device, matrix="bt601", full_range=False, max_bytes=32 << 30, rotate=True):
        from ... import video
        video.yuv_coeffs(matrix, full_range)
        sources, lr_sources = list(sources), list(lr_sources)
        self.scale, _, _ = video_pair_layout(sources, lr_sources, max_bytes)    # what the files are, before the device
        self.rotate = bool(rotate)
        self.hr = ResidentVideoSet(sources, device, matrix, full_range, max_bytes)
        self.lr = ResidentVideoSet(lr_sources, device, matrix, full_range, max_bytes)
        self.matrix, self.full_range, self.device = self.hr.matrix, self.hr.full_range, self.hr.device
        self.sources, self.lr_sources = self.hr.sources, self.lr.sources
        self.entries, self.paths, self.pool = self.hr.entries, self.hr.paths, self.hr.pool
        self.lr_entries, self.lr_paths, self.lr_pool = self.lr.entries, self.lr.paths, self.lr.pool
        self.nbytes = self.hr.nbytes + self.lr.nbytes

    def __len__(self):
        return len(self.entries)

    def frame_planes_np(self, k):
        return self.hr.frame_planes_np(k)

    def frame_planes(self, k):
        return self.hr.frame_planes(k)

    def image_np(self, k):
        return self.hr.image_np(k)

    def lr_frame_planes_np(self, k):
        return self.lr.frame_planes_np(k)

    def lr_frame_planes(self, k):
        return self.lr.frame_planes(k)

    def lr_image_np(self, k):
        return self.lr.image_np(k)

    # ---- what ResidentTrainLoader asks a set that has them
    def check_crop(self, S):
        _pair_sides(S, self.scale)

    def draw_params(self, k, S):
        _, h, w = self.lr_entries[k]
        return draw_pair_params(h, w, S, self.scale, self.rotate)

    def make_table(self, indices, params, S, out=None):
        return make_pair_table([self.entries[k] + self.lr_entries[k] + (p,) for k, p in zip(indices, params)], S,
                               self.scale, out=out)

    def gather(self, table, n, S, want_f32=False):
        from ... import ops
        return ops.aug_gather_yuv420_pair(self.pool, self.lr_pool, table, n, S, self.scale, self.matrix, self.full_range,
                                          want_f32=want_f32)

    def as_batch(self, out, want_f32):
        if want_f32:
            return {"image_u8": out[0], "image": out[1], "lr_u8": out[2], "lr": out[3], "lr_scale": self.scale}
        return {"image_u8": out[0], "lr_u8": out[1], "lr_scale": self.scale}


class ResidentTrainLoader(object):
    """The DataLoader of the training crops, on the GPU: per batch the N parameter sets are drawn on the host in batch
    order (draw_train_params, torch global RNG), written into one pinned table, copied to the device once, and one
    ofasr_aug_gather_u8 launch writes the batch (a set with a `gather` of its own, ResidentVideoSet, is asked instead:
    one ofasr_aug_gather_yuv420 launch; everything else is the same).  Yields {'image_u8': uint8 [N, 3, S, S]} (+ 'image', the same batch as
    fp32 / 255, when `want_f32`); utils.device_batch makes the LR images from it.  `sampler` is any index sampler over the
    set (RankShardSampler with its set_epoch contract when sharded, a fresh permutation per epoch otherwise).
    The only host wait is on the pinned table of `ring` batches ago, before it is overwritten.

    A paired set (ResidentVideoPairSet) brings hooks of its own, and only such a set has them: `TABLE_BLOCKS` rows of
    pinned table per sample, `check_crop(S)`, `draw_params(k, S)` in place of draw_train_params, `make_table(indices,
    params, S, out)` in place of make_table, and `as_batch(out, want_f32)` for the batch's keys.  For every other set
    the draws, the table and the batch are what they were.

    `candidates=K` > 1: best of K candidate crops (the definition stands before aug_select_strips above).  K parameter
    sets are drawn per sample, sample-major, the candidate table -- the same rows, K per sample, built by the same
    make_table / set hook in a pinned ring of K times the rows -- is uploaded once, ops.aug_select names each sample's
    winner on the device and its table goes to the unchanged gather: two small launches more and no host read.
    `last_params` is then the list of K-lists, `last_choice` (int32 [n]) and `last_activity` (int64 [n, K]) are device
    tensors, `batch(indices, params=...)` takes a list of K parameter sets per sample, and selection_stats() reads what
    the batches since its last call accumulated.  With K = 1 none of this code runs.

    `degrade=spec` (degrade.check_spec's keys): blurred, noisy LR inputs, the blind-SR degradation model of degrade.py.
    Per batch one row per sample is drawn (degrade.draw_degrade, torch global RNG) after ALL crop draws of the batch, in
    batch order, written into a pinned int32 ring like the crop table and uploaded non-blocking; the batch carries
    'degrade' (the int32 [n, 48] device table) and 'degrade_seed', from which utils.device_batch makes the LR images
    (ops.lr_images_from_u8(degrade=)), and `last_degrade` keeps the drawn rows beside `last_params`.
    `batch(indices, degrade_rows=...)` takes the rows instead of drawing them.  A paired set brings its LR crops itself
    and refuses the option.  With degrade=None no draw is made and no key added: RNG use and batches are what they were."""

    def __init__(self, dataset, batch_size, sampler, size, drop_last=True, want_f32=False, ring=4, candidates=1,
                 degrade=None, degrade_seed=0):
        self.dataset, self.batch_size, self.sampler = dataset, int(batch_size), sampler
        self.size, self.drop_last, self.want_f32 = int(size), bool(drop_last), bool(want_f32)
        self.candidates = check_candidates(candidates)
        self.last_choice, self.last_activity, self._stats = None, None, None
        if not 0 < self.size <= MAX_SIDE:
            raise ValueError("ResidentTrainLoader: crop side %d outside 1 .. %d" % (self.size, MAX_SIDE))
        for (_, h, w), p in zip(dataset.entries, dataset.paths):
            if h < self.size or w < self.size:
                raise ValueError("Required crop size %s is larger than input image size %s (%s)"
                                 % ((self.size, self.size), (h, w), p))
        if hasattr(dataset, "check_crop"):
            dataset.check_crop(self.size)
        rows = self.batch_size * getattr(dataset, "TABLE_BLOCKS", 1) * self.candidates
        self._host = [torch.empty((rows, TABLE_COLS), dtype=torch.int64).pin_memory() for _ in range(ring)]
        self._done = [None] * ring
        self._turn = 0
        self.last_indices, self.last_params = None, None
        self.degrade, self.degrade_seed, self.last_degrade = _degrade.check_spec(degrade), int(degrade_seed), None
        if self.degrade is not None:
            if hasattr(dataset, "make_table"):
                raise ValueError("ResidentTrainLoader: degrade= with a paired set: its LR crops are the decoded LR stream's, "
                                 "there is no bicubic to degrade")
            self._dg_host = [torch.empty((self.batch_size, _degrade.TABLE_COLS), dtype=torch.int32).pin_memory()
                             for _ in range(ring)]
            self._dg_done = [None] * ring
            self._dg_turn = 0

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def batch(self, indices, params=None, degrade_rows=None):
        """the batch of images `indices`; `params` (a list of (i, j, flip, angle); with candidates = K > 1 a list of K such
        sets per sample) are drawn when not given, and so are, with degrade=, the `degrade_rows` after them"""
        out = self._batch_best_of(indices, params) if self.candidates > 1 else self._batch_plain(indices, params)
        if self.degrade is None:
            return out
        return self._add_degrade(out, len(indices), degrade_rows)

    def _add_degrade(self, out, n, rows):
        """the batch's 'degrade' table: the rows are drawn here, after every crop draw of the batch"""
        if rows is None:
            rows = [_degrade.draw_degrade(self.degrade) for _ in range(n)]
        if len(rows) != n:
            raise ValueError("ResidentTrainLoader: %d degrade rows for %d samples" % (len(rows), n))
        slot = self._dg_turn
        self._dg_turn = (slot + 1) % len(self._dg_host)
        if self._dg_done[slot] is not None:
            self._dg_done[slot].synchronize()  # the upload that last read this pinned table
        host = _degrade.degrade_table(rows, out=self._dg_host[slot])
        with torch.cuda.device(self.dataset.device):
            out["degrade"] = host.to(self.dataset.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._dg_done[slot] = ev
        out["degrade_seed"] = self.degrade_seed
        self.last_degrade = list(rows)
        return out

    def _batch_plain(self, indices, params):
        """batch() with candidates = 1"""
        from ... import ops
        ds, S = self.dataset, self.size
        draw = getattr(ds, "draw_params", None)       # a paired set draws on its LR grid
        if params is None and draw is not None:
            params = [draw(k, S) for k in indices]
        if params is None:
            params = [draw_train_params(ds.entries[k][1], ds.entries[k][2], S) for k in indices]
        slot = self._turn
        self._turn = (slot + 1) % len(self._host)
        if self._done[slot] is not None:
            self._done[slot].synchronize()     # the upload that last read this pinned table
        gather = getattr(ds, "gather", None)       # a set that decodes in its own gather (ResidentVideoSet)
        if hasattr(ds, "make_table"):                 # a paired set: [2, n, 12]
            host = ds.make_table(indices, params, S, out=self._host[slot])
        else:
            host = make_table([ds.entries[k] + (p,) for k, p in zip(indices, params)], S, out=self._host[slot],
                              yuv420=getattr(ds, "yuv420", False))
        with torch.cuda.device(ds.device):
            table = host.to(ds.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._done[slot] = ev
            if gather is not None:
                out = gather(table, len(indices), S, want_f32=self.want_f32)
            else:
                out = ops.aug_gather_u8(ds.pool, table, len(indices), S, want_f32=self.want_f32)
        self.last_indices, self.last_params = list(indices), list(params)
        if hasattr(ds, "as_batch"):
            return ds.as_batch(out, self.want_f32)
        if self.want_f32:
            return {"image_u8": out[0], "image": out[1]}
        return {"image_u8": out}

    def _batch_best_of(self, indices, params):
        """batch() with candidates = K > 1"""
        from ... import ops
        ds, S, K, n = self.dataset, self.size, self.candidates, len(indices)
        draw = getattr(ds, "draw_params", None)       # a paired set draws on its LR grid
        if params is None and draw is not None:
            params = [draw_candidates(lambda: draw(k, S), K) for k in indices]
        if params is None:
            params = [draw_candidates(lambda: draw_train_params(ds.entries[k][1], ds.entries[k][2], S), K) for k in indices]
        params = [list(ps) if isinstance(ps, (list, tuple)) else [] for ps in params]
        if len(params) != n or any(len(ps) != K or any(not isinstance(p, (list, tuple)) or len(p) != 4 for p in ps)
                                   for ps in params):
            raise ValueError("ResidentTrainLoader: with candidates=%d, params is a list of %d parameter sets per sample" % (K, K))
        rep = [k for k in indices for _ in range(K)]          # sample-major: all K of sample 0, then all K of sample 1
        flat = [p for ps in params for p in ps]
        slot = self._turn
        self._turn = (slot + 1) % len(self._host)
        if self._done[slot] is not None:
            self._done[slot].synchronize()     # the upload that last read this pinned table
        if hasattr(ds, "make_table"):                 # a paired set: [2, n * K, 12]
            host = ds.make_table(rep, flat, S, out=self._host[slot])
        else:
            host = make_table([ds.entries[k] + (p,) for k, p in zip(rep, flat)], S, out=self._host[slot],
                              yuv420=getattr(ds, "yuv420", False)).view(1, n * K, TABLE_COLS)
        with torch.cuda.device(ds.device):
            if self._stats is None:
                self._stats = torch.zeros(3, dtype=torch.int64, device=ds.device)
            cand = host.to(ds.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._done[slot] = ev
            table, choice, activity = ops.aug_select(ds.pool, cand, n, K, S, yuv420=getattr(ds, "yuv420", False),
                                                     blocks=host.size(0), stats=self._stats)
            gather = getattr(ds, "gather", None)
            if hasattr(ds, "make_table"):
                out = gather(table, n, S, want_f32=self.want_f32)
            elif gather is not None:
                out = gather(table[0], n, S, want_f32=self.want_f32)
            else:
                out = ops.aug_gather_u8(ds.pool, table[0], n, S, want_f32=self.want_f32)
        self.last_indices, self.last_params = list(indices), params
        self.last_choice, self.last_activity = choice, activity
        if hasattr(ds, "as_batch"):
            return ds.as_batch(out, self.want_f32)
        if self.want_f32:
            return {"image_u8": out[0], "image": out[1]}
        return {"image_u8": out}

    def selection_stats(self):
        """(sum of the chosen crops' activities, sum of the first candidates' activities, samples) over the batches since
        the last call, and the counters start again.  It reads the device: once per epoch, not per batch.  (0, 0, 0) with
        candidates = 1."""
        if self._stats is None:
            return 0, 0, 0
        chosen, first, count = (int(v) for v in self._stats.tolist())
        self._stats.zero_()
        return chosen, first, count

    def __iter__(self):
        chunk = []
        for k in self.sampler:
            chunk.append(int(k))
            if len(chunk) == self.batch_size:
                yield self.batch(chunk)
                chunk = []
        if chunk and not self.drop_last:
            yield self.batch(chunk)
