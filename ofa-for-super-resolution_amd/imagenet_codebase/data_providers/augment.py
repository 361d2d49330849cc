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
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

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


def table_row(offset, H, W, size, params):
    """one row of ofasr_aug_gather_u8's table; refuses what the kernel would have to clamp"""
    i, j, flip, angle = params
    if H < size or W < size:
        raise ValueError("aug_gather_u8: image %dx%d is smaller than the %dx%d crop" % (H, W, size, size))
    if not (0 <= i <= H - size and 0 <= j <= W - size):
        raise ValueError("aug_gather_u8: crop corner (%d, %d) outside the %dx%d image" % (i, j, H, W))
    return (int(offset), int(H), int(W), int(i), int(j), int(bool(flip))) + tuple(rotate_coeffs(angle, size))


def make_table(rows, size, out=None):
    """int64 [n, 12] host table from (offset, H, W, (i, j, flip, angle)) entries"""
    vals = [table_row(o, H, W, size, p) for (o, H, W, p) in rows]
    t = torch.tensor(vals, dtype=torch.int64).reshape(len(vals), TABLE_COLS)
    if out is None:
        return t
    out[:len(vals)].copy_(t)
    return out[:len(vals)]


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


class ResidentTrainLoader(object):
    """The DataLoader of the training crops, on the GPU: per batch the N parameter sets are drawn on the host in batch
    order (draw_train_params, torch global RNG), written into one pinned table, copied to the device once, and one
    ofasr_aug_gather_u8 launch writes the batch.  Yields {'image_u8': uint8 [N, 3, S, S]} (+ 'image', the same batch as
    fp32 / 255, when `want_f32`); utils.device_batch makes the LR images from it.  `sampler` is any index sampler over the
    set (RankShardSampler with its set_epoch contract when sharded, a fresh permutation per epoch otherwise).
    The only host wait is on the pinned table of `ring` batches ago, before it is overwritten."""

    def __init__(self, dataset, batch_size, sampler, size, drop_last=True, want_f32=False, ring=4):
        self.dataset, self.batch_size, self.sampler = dataset, int(batch_size), sampler
        self.size, self.drop_last, self.want_f32 = int(size), bool(drop_last), bool(want_f32)
        if not 0 < self.size <= MAX_SIDE:
            raise ValueError("ResidentTrainLoader: crop side %d outside 1 .. %d" % (self.size, MAX_SIDE))
        for (_, h, w), p in zip(dataset.entries, dataset.paths):
            if h < self.size or w < self.size:
                raise ValueError("Required crop size %s is larger than input image size %s (%s)"
                                 % ((self.size, self.size), (h, w), p))
        self._host = [torch.empty((self.batch_size, TABLE_COLS), dtype=torch.int64).pin_memory() for _ in range(ring)]
        self._done = [None] * ring
        self._turn = 0
        self.last_indices, self.last_params = None, None

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def batch(self, indices, params=None):
        """the batch of images `indices`; `params` (a list of (i, j, flip, angle)) are drawn when not given"""
        from ... import ops
        ds, S = self.dataset, self.size
        if params is None:
            params = [draw_train_params(ds.entries[k][1], ds.entries[k][2], S) for k in indices]
        slot = self._turn
        self._turn = (slot + 1) % len(self._host)
        if self._done[slot] is not None:
            self._done[slot].synchronize()     # the upload that last read this pinned table
        host = make_table([ds.entries[k] + (p,) for k, p in zip(indices, params)], S, out=self._host[slot])
        with torch.cuda.device(ds.device):
            table = host.to(ds.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._done[slot] = ev
            out = ops.aug_gather_u8(ds.pool, table, len(indices), S, want_f32=self.want_f32)
        self.last_indices, self.last_params = list(indices), list(params)
        if self.want_f32:
            return {"image_u8": out[0], "image": out[1]}
        return {"image_u8": out}

    def __iter__(self):
        chunk = []
        for k in self.sampler:
            chunk.append(int(k))
            if len(chunk) == self.batch_size:
                yield self.batch(chunk)
                chunk = []
        if chunk and not self.drop_last:
            yield self.batch(chunk)
