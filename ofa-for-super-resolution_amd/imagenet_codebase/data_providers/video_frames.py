"""Training, search and evaluation data straight from raw 8-bit YUV 4:2:0 video (Y4M, or headerless yuv420p with its
size): the frames stay on the GPU as they are in the file and the colour decode is fused into the augmentation gather
(augment.ResidentVideoSet, csrc/augment.hip: ofasr_aug_gather_yuv420), so the RGB the network is trained on is the RGB
it sees when upscale_video_ofa_net_sr.py feeds it the same video -- video.py's pinned conversion -- and no PNG and no
RGB frame exists anywhere.  The provider has Div2K_SetXXDataProvider's interface.

The split.  Within each video's selected frames (`frames` = (A, B): frames A .. B-1, as --frames of the upscaler), the
frames at positions 0, K, 2K, ... (K = `valid_every`) are the evaluation set and the rest are the training set;
K = 0: every frame trains and the first one evaluates.  Evaluation items are whole frames, ModCrop(4), batch 1, on
every rank, in file order.

Paired video (`videos_lr`, --video-lr): each video comes with its decoded low-resolution stream, 1/2 or 1/4 of its
sides, and the network input at that scale is the LR stream's frame of the same index instead of Pillow's bicubic of
the source (augment.ResidentVideoPairSet, ofasr_aug_gather_yuv420_pair; the definition stands in augment.py).

This module also holds the command-line flags of the entry scripts (add_video_args / take_video_args); nothing at
module level needs torch.
"""
import argparse

VIDEO_FLAGS = ("video", "video_size", "video_frames", "video_valid_every", "matrix", "range")
PAIR_FLAGS = ("video_lr", "video_lr_size", "video_no_rotate")
SCENE_FLAGS = ("video_scene",)


# ---------------------------------------------------------------------------------------------- command line
def parse_video_size(text):
    try:
        w, h = text.lower().split("x")
        w, h = int(w), int(h)
    except ValueError:
        raise argparse.ArgumentTypeError("expected WxH, got %r" % text)
    if w < 2 or h < 2 or w % 2 or h % 2:
        raise argparse.ArgumentTypeError("a 4:2:0 frame needs even, positive sides, got %r" % text)
    return w, h


def parse_video_frames(text):
    """A:B -> (A, B or None): frames A .. B-1 (the meaning of --frames of upscale_video_ofa_net_sr.py)"""
    try:
        a, b = text.split(":")
        a, b = (int(a) if a else 0), (int(b) if b else None)
    except ValueError:
        raise argparse.ArgumentTypeError("expected A:B, got %r" % text)
    if a < 0 or (b is not None and b <= a):
        raise argparse.ArgumentTypeError("empty or negative frame range %r" % text)
    return a, b


def add_video_args(ap):
    """the flags that select raw-video input, the same on every entry script"""
    g = ap.add_argument_group("raw YUV 4:2:0 video input (instead of the DIV2K image folders)")
    g.add_argument("--video", action="append", default=None, metavar="PATH",
                   help="train / calibrate / evaluate on the frames of this 8-bit YUV 4:2:0 video (*.y4m, or headerless "
                        "yuv420p with --video-size); repeatable")
    g.add_argument("--video-size", type=parse_video_size, default=None, metavar="WxH", help="frame size of headerless files")
    g.add_argument("--video-frames", type=parse_video_frames, default=None, metavar="A:B",
                   help="frames A .. B-1 of every video only")
    g.add_argument("--video-valid-every", type=int, default=10, metavar="K",
                   help="every K-th selected frame of a video evaluates, the rest train (0: all train, the first evaluates)")
    g.add_argument("--matrix", default="bt601", choices=["bt601", "bt709"])
    g.add_argument("--range", default="tv", choices=["tv", "pc"], help="tv: limited (16..235), pc: full range")
    g.add_argument("--video-lr", action="append", default=None, metavar="PATH",
                   help="the decoded low-resolution stream of the --video at the same position (1/2 or 1/4 of its sides, "
                        "8-bit 4:2:0, as many frames): the network input at that scale is its frame, not the bicubic of "
                        "the source; repeatable, one per --video")
    g.add_argument("--video-lr-size", type=parse_video_size, default=None, metavar="WxH",
                   help="frame size of headerless --video-lr files")
    g.add_argument("--video-no-rotate", action="store_true",
                   help="paired training without the random rotation (the angle is drawn and set to 0): LR and HR crops "
                        "then cover exactly the same area; needs --video-lr")
    g.add_argument("--video-scene", default=None, metavar="FILE:K",
                   help="--video-frames = the range of scene K of the scene map FILE (scenes_ofa_net_sr.py); needs exactly "
                        "one --video and excludes --video-frames")
    return ap


def take_video_args(a):
    """Remove the flags of add_video_args from the parsed namespace `a` and return them as VideoFramesRunConfig's keyword
    arguments, or None without --video (the namespace is then what it was before the flags existed; a video flag
    given without --video is an error)."""
    vals = {k: a.__dict__.pop(k) for k in VIDEO_FLAGS}
    pair = {k: a.__dict__.pop(k) for k in PAIR_FLAGS}
    scene = {k: a.__dict__.pop(k) for k in SCENE_FLAGS}["video_scene"]
    if scene is not None:     # without --video-scene everything below is what it was before the flag existed
        if not vals["video"] or len(vals["video"]) != 1:
            raise SystemExit("--video-scene needs exactly one --video")
        if vals["video_frames"] is not None:
            raise SystemExit("--video-scene and --video-frames exclude each other: the scene is the frame range")
        from ... import scenes
        try:
            vals["video_frames"] = parse_video_frames(scenes.video_scene_range(scene))
        except (ValueError, OSError) as e:
            raise SystemExit("--video-scene: %s" % e)
    if not pair["video_lr"] and (pair["video_lr_size"] is not None or pair["video_no_rotate"]):
        raise SystemExit("--video-lr-size / --video-no-rotate need --video-lr")
    if not vals["video"]:
        if vals["video_size"] is not None or vals["video_frames"] is not None:
            raise SystemExit("--video-size / --video-frames need --video")
        if pair["video_lr"]:
            raise SystemExit("--video-lr needs --video")
        return None
    if vals["video_valid_every"] < 0:
        raise SystemExit("--video-valid-every must be >= 0")
    kw = dict(videos=list(vals["video"]), video_size=vals["video_size"], video_frames=vals["video_frames"],
              video_valid_every=vals["video_valid_every"], matrix=vals["matrix"], full_range=vals["range"] == "pc")
    if pair["video_lr"]:      # without --video-lr the keyword arguments are what they were before the flag existed
        if len(pair["video_lr"]) != len(kw["videos"]):
            raise SystemExit("%d --video-lr (%s) for %d --video (%s): they are matched by position"
                             % (len(pair["video_lr"]), ", ".join(pair["video_lr"]), len(kw["videos"]),
                                ", ".join(kw["videos"])))
        kw.update(videos_lr=list(pair["video_lr"]), video_lr_size=pair["video_lr_size"],
                  video_rotate=not pair["video_no_rotate"])
    return kw


def take_crop_candidates(a, resident):
    """Remove --crop-candidates from the parsed namespace `a` and return it as the run configs' keyword argument: {} with
    K = 1 (everything is then what it was before the flag existed), {'crop_candidates': K} otherwise.  `resident`: the
    run keeps its training set on the GPU (--resident or --video); without it K > 1 is refused."""
    K = a.__dict__.pop("crop_candidates")
    if not 1 <= K <= 16:
        raise SystemExit("--crop-candidates must be 1 .. 16, got %d" % K)
    if K == 1:
        return {}
    if not resident:
        raise SystemExit("--crop-candidates %d needs --resident or --video: the selection runs on the resident pool "
                         "(the training set in GPU memory); there is no PIL-side implementation" % K)
    return {"crop_candidates": K}


def add_degrade_args(ap):
    """the training scripts' --degrade-* options (degrade.py: blurred, noisy LR inputs); take_degrade checks them"""
    ap.add_argument("--degrade-blur", default=None, metavar="LO:HI",
                    help="train on LR inputs blurred before the down-sampling: a Gaussian whose sigma (HR pixels, at most "
                         "10/3) is drawn per sample from LO .. HI; needs --resident or --video")
    ap.add_argument("--degrade-aniso", action="store_true", help="draw sigma_x and sigma_y of the blur separately")
    ap.add_argument("--degrade-noise", default=None, metavar="LO:HI",
                    help="add noise to the LR inputs after the down-sampling: its sigma (8-bit levels, at most 50) is drawn "
                         "per sample from LO .. HI; needs --resident or --video")
    ap.add_argument("--degrade-gray-prob", type=float, default=0.0, metavar="P",
                    help="the share of samples whose noise is the same in the three channels (default 0)")
    ap.add_argument("--degrade-prob", type=float, default=1.0, metavar="P",
                    help="the share of samples that are degraded at all (default 1)")
    ap.add_argument("--degrade-seed", type=int, default=0, metavar="N", help="the seed of the noise generator (default 0)")


def take_degrade(a, resident, video_kw=None, input_key=None, what=None):
    """Remove the --degrade-* options from the parsed namespace `a` and return them as the run configs' keyword
    arguments: {} when neither --degrade-blur nor --degrade-noise is given (everything is then what it was before the
    options existed), {'degrade': spec, 'degrade_seed': N} otherwise.  Every refusal names its option.  `resident`: the
    run keeps its training set on the GPU; `video_kw`: take_video_args' result; `input_key` / `what`: as
    refuse_pair_for_hr_input's."""
    from ... import degrade as dg
    d = a.__dict__
    blur, noise = d.pop("degrade_blur"), d.pop("degrade_noise")
    aniso, gray, prob, seed = d.pop("degrade_aniso"), d.pop("degrade_gray_prob"), d.pop("degrade_prob"), d.pop("degrade_seed")
    first = "--degrade-blur" if blur is not None else "--degrade-noise"
    if blur is None and noise is None:
        for opt, given in (("--degrade-aniso", aniso), ("--degrade-gray-prob", gray != 0.0), ("--degrade-prob", prob != 1.0),
                           ("--degrade-seed", seed != 0)):
            if given:
                raise SystemExit("%s needs --degrade-blur LO:HI or --degrade-noise LO:HI" % opt)
        return {}
    if aniso and blur is None:
        raise SystemExit("--degrade-aniso needs --degrade-blur LO:HI")

    def parse(opt, text):
        if text is None:
            return (0.0, 0.0)
        parts = text.split(":")
        try:
            vals = [float(p) for p in parts]
        except ValueError:
            vals = []
        if len(vals) not in (1, 2) or len(vals) != len(parts):
            raise SystemExit("%s takes LO:HI (or one number for both), got %r" % (opt, text))
        return (vals[0], vals[-1])
    try:
        spec = dg.check_spec({"blur": parse("--degrade-blur", blur), "aniso": aniso,
                              "noise": parse("--degrade-noise", noise), "gray_prob": gray, "prob": prob},
                             names={"blur": "--degrade-blur", "noise": "--degrade-noise",
                                    "gray_prob": "--degrade-gray-prob", "prob": "--degrade-prob"})
    except ValueError as e:
        raise SystemExit(str(e))
    if not 0 <= seed < 1 << 64:
        raise SystemExit("--degrade-seed must be 0 .. 2^64 - 1, got %d" % seed)
    if video_kw and video_kw.get("videos_lr"):
        raise SystemExit("%s with --video-lr: the LR inputs of paired video are the decoded LR stream's, there is no "
                         "bicubic to degrade" % first)
    if input_key == "image":
        raise SystemExit("%s: %s takes the HR image as its input ('image'), it has no LR input to degrade" % (first, what))
    if not resident:
        raise SystemExit("%s needs --resident or --video: the blur and the noise run on the GPU around the resident "
                         "loader's bicubic; there is no PIL-side implementation" % first)
    return {"degrade": spec, "degrade_seed": seed}


def refuse_pair_for_hr_input(video_kw, input_key, what):
    """the entry scripts' refusal of --video-lr for a network whose input is the HR image itself (the X4 family)"""
    if video_kw and video_kw.get("videos_lr") and input_key == "image":
        raise SystemExit("--video-lr: %s takes the HR image as its input ('image'), it has no LR input to replace" % what)


# ---------------------------------------------------------------------------------------------- the split
def select_frames(n_frames, frames=None, valid_every=10):
    """(selected, train, evaluation) frame indices of one video of `n_frames` frames: `frames` = (A, B) selects
    A .. min(B, n_frames) - 1 (None: all), then positions 0, K, 2K, ... of the selection evaluate and the rest train;
    K = 0: all train and the first evaluates.  Each list is increasing."""
    a, b = (0, None) if frames is None else frames
    K = int(valid_every)
    if K < 0:
        raise ValueError("valid_every must be >= 0, got %d" % K)
    selected = list(range(int(a), n_frames if b is None else min(int(b), n_frames)))
    if not selected:
        raise ValueError("frames %s:%s select nothing of %d frames" % (a, "" if b is None else b, n_frames))
    if K == 0:
        return selected, list(selected), selected[:1]
    return selected, [f for p, f in enumerate(selected) if p % K], selected[::K]


class _EvalFrames(object):
    """a re-iterable, len()-able loader of whole frames of a ResidentVideoSet: batch-1 dicts {'image_u8': uint8
    [1, 3, H', W']} on the GPU, H', W' = ModCrop(4) of the frame, decoded by ops.yuv420_to_rgb_u8 when iterated (the
    decoded frames are not kept).  Of a ResidentVideoPairSet of scale f the items carry 'lr_u8', the decoded LR frame
    cut to [1, 3, H'/f, W'/f], and 'lr_scale' = f beside it."""

    def __init__(self, dataset, indices):
        self.dataset, self.indices = dataset, list(indices)

    def __len__(self):
        return len(self.indices)

    def __iter__(self):
        import torch
        from ... import ops
        ds = self.dataset
        for k in self.indices:
            _, h, w = ds.entries[k]
            with torch.cuda.device(ds.device):
                rgb = ops.yuv420_to_rgb_u8(*ds.frame_planes(k), matrix=ds.matrix, full_range=ds.full_range)
                item = {"image_u8": rgb[:h - h % 4, :w - w % 4].permute(2, 0, 1).contiguous().unsqueeze(0)}
                f = getattr(ds, "scale", None)
                if f is not None:
                    lr = ops.yuv420_to_rgb_u8(*ds.lr_frame_planes(k), matrix=ds.matrix, full_range=ds.full_range)
                    item["lr_u8"] = lr[:(h - h % 4) // f, :(w - w % 4) // f].permute(2, 0, 1).contiguous().unsqueeze(0)
                    item["lr_scale"] = f
                yield item


class VideoFramesDataProvider(object):
    """`train` / `valid` / `test`, `data_shape`, `assign_active_img_size`, `build_sub_train_loader` of
    Div2K_SetXXDataProvider over the frames of `videos` (paths; `video_size` = (width, height) for headerless files).
    `train` is an augment.ResidentTrainLoader over one augment.ResidentVideoSet holding every selected frame (training
    and evaluation frames alike); `valid` is `test`.  With `videos_lr` (one per video; `video_lr_size` for headerless
    files) the set is an augment.ResidentVideoPairSet and every batch and evaluation item carries the decoded LR
    stream's crop / frame; `rotate=False` trains without the rotation.  `crop_candidates=K` > 1: every training crop is
    the most detailed of K drawn candidates (augment.ResidentTrainLoader(candidates=K); a paired set scores on its HR
    pool); the sub-train and evaluation loaders are untouched.  `degrade=spec` (`degrade_seed`; not with `videos_lr`):
    the training batches carry the table of the blind-SR degradation (degrade.py;
    augment.ResidentTrainLoader(degrade=spec)); the sub-train and evaluation loaders are untouched."""
    SUB_SEED = 937162211     # DataProvider.SUB_SEED of div2k_setxx.py

    def __init__(self, videos, video_size=None, frames=None, valid_every=10, matrix="bt601", full_range=False,
                 train_batch_size=16, test_batch_size=1, image_size=32, num_replicas=None, rank=None,
                 resident_max_bytes=32 << 30, videos_lr=None, video_lr_size=None, rotate=True, crop_candidates=1,
                 degrade=None, degrade_seed=0):
        import torch
        from ... import video
        from .augment import ResidentTrainLoader, ResidentVideoPairSet, ResidentVideoSet, count_frames
        from .div2k_setxx import RankShardSampler
        self.videos = [videos] if isinstance(videos, str) else list(videos)
        if not self.videos:
            raise ValueError("VideoFramesDataProvider: no videos")
        self.videos_lr = None if videos_lr is None else ([videos_lr] if isinstance(videos_lr, str) else list(videos_lr))
        if self.videos_lr is None and not rotate:
            raise ValueError("VideoFramesDataProvider: rotate=False is for paired video (videos_lr)")
        self.degrade, self.degrade_seed = degrade, int(degrade_seed)
        if degrade is not None and self.videos_lr is not None:
            raise ValueError("VideoFramesDataProvider: degrade= with paired video (videos_lr): the LR inputs are the decoded "
                             "LR stream's, there is no bicubic to degrade")
        if self.videos_lr is not None and len(self.videos_lr) != len(self.videos):
            raise ValueError("VideoFramesDataProvider: %d LR videos (%s) for %d videos (%s): they are matched by position"
                             % (len(self.videos_lr), ", ".join(self.videos_lr), len(self.videos), ", ".join(self.videos)))
        sizes = sorted(image_size) if isinstance(image_size, (list, tuple)) else [image_size]
        self.image_size = image_size if isinstance(image_size, int) else sizes
        self.active_img_size = sizes[-1]
        self.test_batch_size = test_batch_size       # evaluation items are whole frames, batch 1, whatever this says
        sources, self.train_indices, self.eval_indices, at = [], [], [], 0
        for path in self.videos:
            with video.open_reader(path, video_size) as r:     # header only; a 10-bit file is refused by the set below
                n = count_frames(r)
            selected, train, evaluation = select_frames(n, frames, valid_every)
            where = {f: at + p for p, f in enumerate(selected)}
            self.train_indices += [where[f] for f in train]
            self.eval_indices += [where[f] for f in evaluation]
            sources.append((path, video_size, selected))
            at += len(selected)
        if not self.train_indices:
            raise ValueError("VideoFramesDataProvider: valid_every=%d leaves no training frame among the %d selected"
                             % (valid_every, at))
        if self.videos_lr is not None:
            lr_sources = [(p, video_lr_size, idx) for p, (_, _, idx) in zip(self.videos_lr, sources)]
            self.resident_set = ResidentVideoPairSet(sources, lr_sources, torch.device("cuda", torch.cuda.current_device()),
                                                     matrix, full_range, max_bytes=resident_max_bytes, rotate=rotate)
        else:
            self.resident_set = ResidentVideoSet(sources, torch.device("cuda", torch.cuda.current_device()), matrix,
                                                 full_range, max_bytes=resident_max_bytes)
        self._shard = (num_replicas, rank) if num_replicas is not None and num_replicas > 1 else None
        if self._shard:
            sampler = RankShardSampler(self.train_indices, num_replicas, rank)
        else:
            sampler = torch.utils.data.SubsetRandomSampler(self.train_indices)
        self.crop_candidates = int(crop_candidates)
        self.train = ResidentTrainLoader(self.resident_set, train_batch_size, sampler, self.active_img_size,
                                         drop_last=True, want_f32=True,
                                         **({} if self.crop_candidates == 1 else dict(candidates=self.crop_candidates)),
                                         **({} if degrade is None else dict(degrade=degrade, degrade_seed=degrade_seed)))
        self.test = _EvalFrames(self.resident_set, self.eval_indices)
        self.valid = self.test

    @staticmethod
    def name():
        return "video_frames"

    @property
    def data_shape(self):
        return 3, self.active_img_size, self.active_img_size

    @property
    def n_classes(self):
        return 1

    def assign_active_img_size(self, new_img_size):
        """evaluation is ModCrop(4) of the whole frame at every size, as in the image provider"""
        self.active_img_size = new_img_size

    def build_sub_train_loader(self, n_images, batch_size, num_worker=None, num_replicas=None, rank=None):
        """`n_images` fixed training frames (seed SUB_SEED) as a cached list of batches, for BN re-calibration"""
        import torch
        from .augment import ResidentTrainLoader
        from .div2k_setxx import RankShardSampler
        cache = self.__dict__.setdefault("_sub_train_cache", {})
        key = (self.active_img_size, n_images, batch_size)
        if key not in cache:
            perm = torch.randperm(len(self.train_indices), generator=torch.Generator().manual_seed(self.SUB_SEED))
            chosen = [self.train_indices[p] for p in perm[:n_images].tolist()]
            if num_replicas is not None and num_replicas > 1:
                sampler = RankShardSampler(chosen, num_replicas, rank)
            else:
                sampler = torch.utils.data.SubsetRandomSampler(chosen)
            cache[key] = list(ResidentTrainLoader(self.resident_set, batch_size, sampler, self.active_img_size,
                                                  drop_last=False))
        return cache[key]
