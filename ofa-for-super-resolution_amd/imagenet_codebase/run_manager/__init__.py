"""Per-dataset run configs (mirror of reference ofa/imagenet_codebase/run_manager/__init__.py:127-232).
`Div2K_SetXXRunConfig(**args.__dict__)` keeps working; its lazy `data_provider` resolves to the real
DIV2K provider when the dataset directory exists.  A missing directory is an ERROR unless synthetic data was asked
for explicitly (`allow_synthetic=True` or OFASR_ALLOW_SYNTHETIC_DATA=1): a mistyped path must not train on noise.
`VideoFramesRunConfig` takes the images from the frames of raw YUV 4:2:0 video instead (data_providers/video_frames.py)."""
import os

from .sr_run_manager import RunConfig, SRRunManager  # noqa: F401
from ..data_providers.synthetic_sr import SyntheticSRDataProvider
from ... import degrade as _degrade


class SyntheticSRRunConfig(RunConfig):

    def __init__(self, n_epochs=1, init_lr=1e-3, lr_schedule_type="cosine", lr_schedule_param=None,
                 dataset="synthetic_sr", train_batch_size=16, test_batch_size=1, valid_size=None, opt_type="adam",
                 opt_param=None, weight_decay=3e-5, label_smoothing=0.0, no_decay_keys="bn#bias", mixup_alpha=None,
                 model_init="he_fout", validation_frequency=1, print_frequency=10, n_worker=0, image_size=256,
                 n_train_batches=4, n_test_batches=2, data_seed=0, test_sizes=None, **kwargs):
        super().__init__(n_epochs, init_lr, lr_schedule_type, lr_schedule_param, dataset, train_batch_size,
                         test_batch_size, valid_size, opt_type, opt_param, weight_decay, label_smoothing,
                         no_decay_keys, mixup_alpha, model_init, validation_frequency, print_frequency)
        self.n_worker = n_worker
        self.image_size = image_size
        self._synthetic = dict(n_train_batches=n_train_batches, n_test_batches=n_test_batches, seed=data_seed,
                               test_sizes=test_sizes)

    @property
    def data_provider(self):
        if self.__dict__.get("_data_provider", None) is None:
            from ... import distributed as dd
            self.__dict__["_data_provider"] = SyntheticSRDataProvider(
                train_batch_size=self.train_batch_size, test_batch_size=self.test_batch_size,
                image_size=self.image_size, rank=dd.rank(), num_replicas=dd.world_size(), **self._synthetic)
        return self.__dict__["_data_provider"]


class Div2K_SetXXRunConfig(SyntheticSRRunConfig):
    """reference :127-160.  `data_provider` is the real Div2K_SetXXDataProvider (data_providers/div2k_setxx.py)
    when `$OFASR_DIV2K_ROOT` (default /SSD/div2k_setxx, the reference's DEFAULT_PATH) holds `train/` and `val/`.
    Otherwise it raises, unless the caller opted into the synthetic provider of the same interface
    (`allow_synthetic=True` / OFASR_ALLOW_SYNTHETIC_DATA=1: the DIV2K/SetXX files are absent in this environment);
    the provider actually used is recorded in `self.dataset`, hence in run.config and in every checkpoint."""

    def __init__(self, n_epochs=150, init_lr=0.05, lr_schedule_type="cosine", lr_schedule_param=None,
                 dataset="div2k_setxx", train_batch_size=256, test_batch_size=500, valid_size=None, opt_type="sgd",
                 opt_param=None, weight_decay=4e-5, label_smoothing=0.1, no_decay_keys=None, mixup_alpha=None,
                 model_init="he_fout", validation_frequency=1, print_frequency=10, n_worker=32,
                 resize_scale=0.08, distort_color=None, image_size=32, allow_synthetic=None, resident=False,
                 crop_candidates=1, degrade=None, degrade_seed=0, lr_on_device=False, **kwargs):
        super().__init__(n_epochs, init_lr, lr_schedule_type, lr_schedule_param, dataset, train_batch_size,
                         test_batch_size, valid_size, opt_type, opt_param, weight_decay, label_smoothing,
                         no_decay_keys, mixup_alpha, model_init, validation_frequency, print_frequency,
                         n_worker=n_worker, image_size=image_size,
                         **{k: v for k, v in kwargs.items() if k in ("n_train_batches", "n_test_batches",
                                                                     "data_seed", "test_sizes")})
        self.resize_scale = resize_scale
        self.distort_color = distort_color
        self.resident = bool(resident)
        if int(crop_candidates) != 1:     # best of K candidate crops (data_providers/augment.py); the key exists only then
            if not self.resident:
                raise ValueError("crop_candidates=%d needs resident=True: the selection runs on the resident pool"
                                 % int(crop_candidates))
            self.crop_candidates = int(crop_candidates)
            self._synthetic["crop_candidates"] = self.crop_candidates     # the stand-in selects on a resident pool too
        if degrade is not None:           # blurred, noisy LR inputs (degrade.py); the keys exist only then
            if not self.resident:
                raise ValueError("degrade= needs resident=True: the blur and the noise run on the GPU around the resident "
                                 "loader's bicubic; there is no PIL-side implementation")
            self.degrade, self.degrade_seed = _degrade.check_spec(degrade), int(degrade_seed)
            self._synthetic.update(degrade=self.degrade, degrade_seed=self.degrade_seed)
        if lr_on_device:                  # evaluation items as {'image_u8'}: the LR images are made on the GPU
            self.lr_on_device = True
            self._synthetic["lr_on_device"] = True
        self.dataset_root = os.environ.get("OFASR_DIV2K_ROOT", "/SSD/div2k_setxx")
        self.allow_synthetic = (os.environ.get("OFASR_ALLOW_SYNTHETIC_DATA", "0") == "1") if allow_synthetic is None \
            else bool(allow_synthetic)

    @property
    def data_provider(self):
        if self.__dict__.get("_data_provider", None) is None:
            root = self.dataset_root
            if os.path.isdir(os.path.join(root, "train")) and os.path.isdir(os.path.join(root, "val")):
                from ... import distributed as dd
                from ..data_providers.div2k_setxx import Div2K_SetXXDataProvider
                ws = dd.world_size()
                self.__dict__["_data_provider"] = Div2K_SetXXDataProvider(
                    save_path=root, train_batch_size=self.train_batch_size, test_batch_size=self.test_batch_size,
                    valid_size=self.valid_size, n_worker=self.n_worker, resize_scale=self.resize_scale,
                    distort_color=self.distort_color, image_size=self.image_size,
                    num_replicas=ws if ws > 1 else None, rank=dd.rank() if ws > 1 else None,
                    resident=self.resident,
                    **({} if self.__dict__.get("crop_candidates", 1) == 1 else dict(crop_candidates=self.crop_candidates)),
                    **({} if self.__dict__.get("degrade") is None else dict(degrade=self.degrade,
                                                                            degrade_seed=self.degrade_seed)),
                    **({} if not self.__dict__.get("lr_on_device") else dict(lr_on_device=True)))
            elif self.allow_synthetic:
                from ... import distributed as dd
                if dd.rank() == 0:
                    print("WARNING: %s has no train/ + val/ -- training on SYNTHETIC images (allow_synthetic)" % root,
                          flush=True)
                self.dataset = "synthetic_sr (stand-in for div2k_setxx: %s missing)" % root
                return super().data_provider
            else:
                raise FileNotFoundError(
                    "DIV2K/SetXX dataset not found: %s must hold train/ and val/ (set OFASR_DIV2K_ROOT).  Pass "
                    "allow_synthetic=True / --synthetic or set OFASR_ALLOW_SYNTHETIC_DATA=1 to run on synthetic "
                    "images instead." % root)
        return self.__dict__["_data_provider"]


class VideoFramesRunConfig(SyntheticSRRunConfig):
    """Div2K_SetXXRunConfig's counterpart for raw 8-bit YUV 4:2:0 video: `data_provider` is a VideoFramesDataProvider
    (data_providers/video_frames.py) over `videos`, the frames resident on the GPU and decoded inside the augmentation
    gather.  `dataset` records "video_frames" and the paths, so run.config and every checkpoint say what they were
    trained on.  There is no synthetic stand-in: a missing file is an error.  `videos_lr` (one decoded LR stream per
    video; `video_lr_size`, `video_rotate`) makes it paired video: the dataset string then names the LR files too, and
    only then does the config carry these three keys."""

    def __init__(self, videos, video_size=None, video_frames=None, video_valid_every=10, matrix="bt601", full_range=False,
                 n_epochs=150, init_lr=0.05, lr_schedule_type="cosine", lr_schedule_param=None, dataset=None,
                 train_batch_size=256, test_batch_size=1, valid_size=None, opt_type="sgd", opt_param=None,
                 weight_decay=4e-5, label_smoothing=0.1, no_decay_keys=None, mixup_alpha=None, model_init="he_fout",
                 validation_frequency=1, print_frequency=10, n_worker=0, image_size=32, resident_max_bytes=32 << 30,
                 videos_lr=None, video_lr_size=None, video_rotate=True, crop_candidates=1, degrade=None, degrade_seed=0,
                 **kwargs):
        videos = [videos] if isinstance(videos, str) else list(videos)
        name = "video_frames: " + ", ".join(videos)
        if videos_lr is not None:
            videos_lr = [videos_lr] if isinstance(videos_lr, str) else list(videos_lr)
            if len(videos_lr) != len(videos):
                raise ValueError("VideoFramesRunConfig: %d LR videos (%s) for %d videos (%s): they are matched by position"
                                 % (len(videos_lr), ", ".join(videos_lr), len(videos), ", ".join(videos)))
            name = "video_frames: " + ", ".join("%s (lr: %s)" % hl for hl in zip(videos, videos_lr))
        elif not video_rotate or video_lr_size is not None:
            raise ValueError("VideoFramesRunConfig: video_rotate=False and video_lr_size are for paired video (videos_lr)")
        super().__init__(n_epochs, init_lr, lr_schedule_type, lr_schedule_param,
                         name, train_batch_size, test_batch_size, valid_size, opt_type,
                         opt_param, weight_decay, label_smoothing, no_decay_keys, mixup_alpha, model_init,
                         validation_frequency, print_frequency, n_worker=n_worker, image_size=image_size)
        self.videos = videos
        self.video_size = None if video_size is None else tuple(video_size)
        self.video_frames = None if video_frames is None else tuple(video_frames)
        self.video_valid_every = int(video_valid_every)
        self.matrix, self.full_range = matrix, bool(full_range)
        self.resident = True
        self.resident_max_bytes = int(resident_max_bytes)
        if videos_lr is not None:
            self.videos_lr = videos_lr
            self.video_lr_size = None if video_lr_size is None else tuple(video_lr_size)
            self.video_rotate = bool(video_rotate)
        if int(crop_candidates) != 1:     # best of K candidate crops; the key exists only then
            self.crop_candidates = int(crop_candidates)
        if degrade is not None:           # blurred, noisy LR inputs (degrade.py); the keys exist only then
            if videos_lr is not None:
                raise ValueError("VideoFramesRunConfig: degrade= with videos_lr: the LR inputs of paired video are the "
                                 "decoded LR stream's, there is no bicubic to degrade")
            self.degrade, self.degrade_seed = _degrade.check_spec(degrade), int(degrade_seed)

    @property
    def data_provider(self):
        if self.__dict__.get("_data_provider", None) is None:
            from ... import distributed as dd
            from ..data_providers.video_frames import VideoFramesDataProvider
            ws = dd.world_size()
            self.__dict__["_data_provider"] = VideoFramesDataProvider(
                self.videos, video_size=self.video_size, frames=self.video_frames, valid_every=self.video_valid_every,
                matrix=self.matrix, full_range=self.full_range, train_batch_size=self.train_batch_size,
                test_batch_size=self.test_batch_size, image_size=self.image_size,
                num_replicas=ws if ws > 1 else None, rank=dd.rank() if ws > 1 else None,
                resident_max_bytes=self.resident_max_bytes,
                **({} if self.__dict__.get("videos_lr") is None else dict(
                    videos_lr=self.videos_lr, video_lr_size=self.video_lr_size, rotate=self.video_rotate)),
                **({} if self.__dict__.get("crop_candidates", 1) == 1 else dict(crop_candidates=self.crop_candidates)),
                **({} if self.__dict__.get("degrade") is None else dict(degrade=self.degrade,
                                                                        degrade_seed=self.degrade_seed)))
        return self.__dict__["_data_provider"]
