"""Scene cuts of a YUV 4:2:0 video by the difference of consecutive colour histograms: the host statement (numpy only;
importing this module loads no GPU code), the scene map file, and SceneDetector, which runs the HIP kernels of
csrc/scene.hip on GPU-resident frames.

Everything is an exact integer function of the frames' bytes, which is what the kernels are tested against:

  histogram h      of one frame, int64 [3, 256]: RGB = video.yuv420_to_rgb_host of the WHOLE frame; h[c][b] = the number of
                   pixels whose channel c falls into bin b, b = the value at depth 8 and value >> 2 (of the 10-bit value)
                   at depth 10.  Every channel sums to P = H * W.  These are the counts of 256 equal bins over the
                   channel's range, per channel.
  distance d       between consecutive frames: d = sum_c sum_b (h_cur[c][b] - h_prev[c][b])^2, an exact int64; the first
                   frame has d = 0.  The largest value is 6 P^2 (three channels, all mass moved from one bin to another),
                   so P <= 2^28 keeps it below 2^63: frames above that are refused.  d / (6 P^2) is the normalised
                   distance in [0, 1] a user compares with the threshold.
  limit            floor(T * 6 P^2) of the decimal T in [0, 1] the user wrote, computed exactly (fractions.Fraction).
  cuts             frame i starts a new scene iff d[i] > limit and i - (first frame of the current scene) >= min_scene.

What this is not: there is no handling of fades, dissolves or flashes, no motion, no learned detector -- one fixed
threshold and a minimum scene length.
"""
import json
import math
import os
from fractions import Fraction

import numpy as np

from . import video

MAX_PIXELS = 1 << 28
MAP_KEYS = ("video", "frames", "first", "width", "height", "depth", "matrix", "range", "threshold", "min_scene", "distance",
            "scenes")


def check_pixels(H, W):
    """P = H * W of a frame the distance is defined for"""
    P = int(H) * int(W)
    if P > MAX_PIXELS:
        raise ValueError("a %dx%d frame has more than 2^28 pixels: the distance's bound 6 P^2 would leave int64" % (W, H))
    return P


def rgb_histogram_host(y, u, v, matrix="bt601", full_range=False, depth=8):
    """int64 [3, 256]: the per-channel histogram of the decoded frame (the definition of ofasr_rgb_hist_yuv420 followed by
    the fold of its partials)"""
    rgb = video.yuv420_to_rgb_host(y, u, v, matrix, full_range, depth)
    check_pixels(*rgb.shape[:2])
    bins = rgb.astype(np.int64) >> (depth - 8)
    return np.stack([np.bincount(bins[..., c].ravel(), minlength=256) for c in range(3)]).astype(np.int64)


def _hist(h):
    h = np.asarray(h)
    if h.shape != (3, 256) or h.dtype.kind not in "iu":
        raise ValueError("a histogram is an integer [3, 256] array, got %s %s" % (h.shape, h.dtype))
    return h.astype(np.int64)


def frame_distance_host(h_prev, h_cur):
    """sum_c sum_b (h_cur - h_prev)^2 as a Python int (exact: below 2^63 for P <= 2^28)"""
    d = _hist(h_cur) - _hist(h_prev)
    return int((d * d).sum())


def distances_host(frames, matrix="bt601", full_range=False, depth=8):
    """[d] of a sequence of (y, u, v) frames; d[0] = 0"""
    out, prev = [], None
    for y, u, v in frames:
        h = rgb_histogram_host(y, u, v, matrix, full_range, depth)
        out.append(0 if prev is None else frame_distance_host(prev, h))
        prev = h
    return out


def max_distance(P):
    return 6 * int(P) * int(P)


def distance_limit(threshold, P):
    """the integer limit floor(threshold * 6 P^2) of a threshold in [0, 1]: a number, or the decimal string the user
    wrote (taken exactly)"""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, str, Fraction)):
        raise ValueError("the threshold must be a number in [0, 1], got %r" % (threshold,))
    if isinstance(P, bool) or int(P) != P or not 0 < P <= MAX_PIXELS:
        raise ValueError("P must be a pixel count in 1 .. 2^28, got %r" % (P,))
    if isinstance(threshold, Fraction):
        exact = threshold
    else:
        text = threshold.strip() if isinstance(threshold, str) else str(threshold)
        try:
            v = float(text)
        except ValueError:
            raise ValueError("the threshold must be a number in [0, 1], got %r" % (threshold,))
        if math.isnan(v) or math.isinf(v):
            raise ValueError("the threshold must be a number in [0, 1], got %r" % (threshold,))
        try:
            exact = Fraction(text)
        except (ValueError, ZeroDivisionError):
            exact = Fraction(str(v))
    if not 0 <= exact <= 1:
        raise ValueError("the threshold must lie in [0, 1], got %r" % (threshold,))
    return int(math.floor(exact * max_distance(P)))


def cuts(d, limit, min_scene=1):
    """[(first, stop)]: the scenes of frames 0 .. len(d) - 1 (relative numbers).  Frame i starts a new scene iff d[i] > limit
    and i - (first frame of the current scene) >= min_scene; d[0] belongs to no pair of frames and is not looked at."""
    if isinstance(min_scene, bool) or int(min_scene) != min_scene or min_scene < 1:
        raise ValueError("min_scene must be an integer >= 1, got %r" % (min_scene,))
    n = len(d)
    out, start = [], 0
    for i in range(1, n):
        if int(d[i]) > limit and i - start >= min_scene:
            out.append((start, i))
            start = i
    if n:
        out.append((start, n))
    return out


def normalised(d, P):
    """d / (6 P^2) as float64"""
    return np.asarray([int(x) for x in d], dtype=np.float64) / float(max_distance(P))


class SceneMap(object):
    """the scene map of one video: a JSON object with the keys MAP_KEYS.  `first` is the absolute number of the first
    analysed frame, `frames` how many were analysed, `distance` their distances (distance[0] = 0); `scenes` is a list of
    {"first": A, "stop": B} in absolute frame numbers, increasing, non-empty and contiguous, each with an optional
    "static": DIR (the export that serves the scene).  `threshold` is None and `scenes` empty in a map that holds
    distances only."""

    def __init__(self, video, frames, first, width, height, depth, matrix, range, threshold, min_scene, distance, scenes):
        self.video, self.frames, self.first, self.width, self.height = video, frames, first, width, height
        self.depth, self.matrix, self.range, self.threshold, self.min_scene = depth, matrix, range, threshold, min_scene
        self.distance = list(distance)
        self.scenes = [dict(s) if isinstance(s, dict) else s for s in scenes]
        self.validate()

    def validate(self):
        for key in ("frames", "first", "width", "height", "min_scene"):
            val = getattr(self, key)
            if isinstance(val, bool) or not isinstance(val, int) or val < (1 if key in ("width", "height", "min_scene") else 0):
                raise ValueError("scene map: %r is not a valid %s" % (val, key))
        if self.depth not in video.DEPTHS or isinstance(self.depth, bool):
            raise ValueError("scene map: depth must be 8 or 10, got %r" % (self.depth,))
        if self.matrix not in video.MATRICES:
            raise ValueError("scene map: matrix must be one of %s, got %r" % (sorted(video.MATRICES), self.matrix))
        if self.range not in ("tv", "pc"):
            raise ValueError("scene map: range must be 'tv' or 'pc', got %r" % (self.range,))
        if self.threshold is not None and (isinstance(self.threshold, bool) or not isinstance(self.threshold, (int, float, str))):
            raise ValueError("scene map: threshold must be a number, a decimal string or null, got %r" % (self.threshold,))
        if len(self.distance) != self.frames:
            raise ValueError("scene map: %d distances for %d frames" % (len(self.distance), self.frames))
        for i, d in enumerate(self.distance):
            if isinstance(d, bool) or not isinstance(d, int) or d < 0:
                raise ValueError("scene map: distance[%d] = %r is not a non-negative integer" % (i, d))
        end = self.first
        for k, s in enumerate(self.scenes):
            if not isinstance(s, dict) or set(s) - {"first", "stop", "static"} or "first" not in s or "stop" not in s:
                raise ValueError("scene map: scenes[%d] = %r is not {\"first\": A, \"stop\": B[, \"static\": DIR]}" % (k, s))
            a, b = s["first"], s["stop"]
            if any(isinstance(x, bool) or not isinstance(x, int) for x in (a, b)):
                raise ValueError("scene map: scenes[%d] = %r: first and stop must be integers" % (k, s))
            if b <= a:
                raise ValueError("scene map: scenes[%d] = %d:%d is empty" % (k, a, b))
            if k == 0 and a < 0:
                raise ValueError("scene map: scenes[0] = %d:%d starts before frame 0" % (a, b))
            if k > 0 and a < end:
                raise ValueError("scene map: scenes[%d] = %d:%d is not increasing: it starts before frame %d, where scenes[%d] "
                                 "stops" % (k, a, b, end, k - 1))
            if k > 0 and a > end:
                raise ValueError("scene map: scenes[%d] = %d:%d is not contiguous: scenes[%d] stops at frame %d"
                                 % (k, a, b, k - 1, end))
            if "static" in s and (not isinstance(s["static"], str) or not s["static"]):
                raise ValueError("scene map: scenes[%d]: static must be a directory name, got %r" % (k, s["static"]))
            end = b
        return self

    def scene_of(self, frame):
        """index of the scene that holds the absolute frame number; ValueError names a frame outside every range"""
        for k, s in enumerate(self.scenes):
            if s["first"] <= frame < s["stop"]:
                return k
        if not self.scenes:
            raise ValueError("frame %d: the scene map holds no scenes (it was written without --threshold)" % frame)
        raise ValueError("frame %d lies outside the scene map's ranges %d:%d"
                         % (frame, self.scenes[0]["first"], self.scenes[-1]["stop"]))

    def frame_range(self, k):
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < len(self.scenes):
            raise ValueError("scene %r: the map holds scenes 0 .. %d" % (k, len(self.scenes) - 1))
        return self.scenes[k]["first"], self.scenes[k]["stop"]

    def to_dict(self):
        return dict((k, getattr(self, k)) for k in MAP_KEYS)

    @classmethod
    def from_dict(cls, obj):
        if not isinstance(obj, dict):
            raise ValueError("scene map: the file does not hold a JSON object")
        missing = [k for k in MAP_KEYS if k not in obj]
        if missing:
            raise ValueError("scene map: missing key(s) %s" % ", ".join(missing))
        unknown = sorted(set(obj) - set(MAP_KEYS))
        if unknown:
            raise ValueError("scene map: unknown key(s) %s" % ", ".join(unknown))
        if not isinstance(obj["distance"], list) or not isinstance(obj["scenes"], list):
            raise ValueError("scene map: distance and scenes must be lists")
        return cls(**obj)

    def save(self, path):
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            json.dump(self.to_dict(), f, indent=1)
            f.write("\n")
        os.replace(tmp, path)

    @classmethod
    def load(cls, path):
        with open(path) as f:
            try:
                obj = json.load(f)
            except ValueError as e:
                raise ValueError("%s: not a JSON file (%s)" % (path, e))
        try:
            return cls.from_dict(obj)
        except ValueError as e:
            raise ValueError("%s: %s" % (path, e))


def parse_video_scene(text):
    """'FILE:K' -> (FILE, K): the argument of --video-scene"""
    path, sep, k = str(text).rpartition(":")
    if not sep or not path or not k.isdigit():
        raise ValueError("--video-scene takes FILE:K (a scene map and a scene index), got %r" % (text,))
    return path, int(k)


def video_scene_range(text):
    """'FILE:K' -> 'A:B', the --video-frames of scene K of that map"""
    path, k = parse_video_scene(text)
    return "%d:%d" % SceneMap.load(path).frame_range(k)


class SceneDetector(object):
    """the distances of a stream of GPU-resident frames: push(y, u, v) launches the histogram kernel and the fold into a
    two-slot histogram ring and appends the distance to a device int64 buffer that grows by doubling; nothing
    synchronises per frame.  distances() is the one read-back."""

    def __init__(self, H, W, depth=8, matrix="bt601", full_range=False, device="cuda:0"):
        import torch

        from . import ops
        self._torch, self._ops = torch, ops
        video._depth(depth)
        video.yuv_coeffs(matrix, full_range, depth)
        if H < 2 or W < 2 or H % 2 or W % 2:
            raise ValueError("a YUV 4:2:0 frame needs even sides, got %dx%d" % (W, H))
        self.H, self.W, self.P = int(H), int(W), check_pixels(H, W)
        self.depth, self.matrix, self.full_range, self.device = depth, matrix, bool(full_range), torch.device(device)
        self.slabs = ops.rgb_hist_slabs(self.H, self.W)
        self._partial = torch.empty(self.slabs, 3, 256, dtype=torch.int32, device=self.device)
        self._ring = torch.zeros(2, 3, 256, dtype=torch.int32, device=self.device)
        self._dist = torch.zeros(64, dtype=torch.int64, device=self.device)
        self.frames = 0

    def push(self, y, u, v):
        torch, ops = self._torch, self._ops
        if tuple(y.shape) != (self.H, self.W) or y.dtype != ops.YUV_DTYPES[self.depth] or y.device != self.device:
            raise ValueError("SceneDetector.push: expected %s planes of a %dx%d frame on %s"
                             % (ops.YUV_DTYPES[self.depth], self.W, self.H, self.device))
        n = self.frames
        if n == self._dist.numel():
            grown = torch.zeros(2 * n, dtype=torch.int64, device=self.device)
            grown[:n].copy_(self._dist)
            self._dist = grown
        ops.rgb_hist_yuv420(y, u, v, self.matrix, self.full_range, out=self._partial)
        ops.hist_fold_distance(self._partial, self._ring[n & 1], self._ring[(n - 1) & 1] if n else None,
                               self._dist[n:n + 1])
        self.frames = n + 1

    def distances(self):
        """[d] of the frames pushed so far, as Python ints (one device-to-host copy)"""
        return [int(x) for x in self._dist[:self.frames].cpu().tolist()]

    def histogram(self):
        """the histogram of the frame pushed last, int64 numpy [3, 256]"""
        if not self.frames:
            raise ValueError("SceneDetector.histogram: no frame has been pushed")
        return self._ring[(self.frames - 1) & 1].cpu().numpy().astype(np.int64)
