"""Synthetic SR data provider: the loader-side contract of the reference's Div2K_SetXX provider
(ofa/imagenet_codebase/data_providers/div2k_setxx.py:17-225,288-298) without the dataset.

Every batch is a dict {'image': HR, '2x_down_image': HR/2, '4x_down_image': HR/4}, float32 NCHW in
[0,1] -- exactly what progressive_shrinking.train_one_epoch and SRRunManager.validate consume.  The
real provider needs torchvision + /SSD/div2k_setxx (absent here); this one
makes seeded images and bicubic(antialias) down-scales them, which is the shape- and
range-faithful stand-in used by the tests and by bench.py.
"""
import torch
import torch.nn.functional as F


class _ListLoader(object):
    """a re-iterable, len()-able list of dict batches (what the training loops need of a DataLoader)."""

    def __init__(self, batches):
        self.batches = list(batches)

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def make_batch(batch_size, hr_size, generator=None, device="cpu"):
    if isinstance(hr_size, int):
        hr_size = (hr_size, hr_size)
    hr = torch.rand((batch_size, 3, hr_size[0], hr_size[1]), generator=generator)
    x2 = F.interpolate(hr, scale_factor=0.5, mode="bicubic", antialias=True).clamp_(0, 1)
    x4 = F.interpolate(hr, scale_factor=0.25, mode="bicubic", antialias=True).clamp_(0, 1)
    return {"image": hr.to(device), "2x_down_image": x2.to(device), "4x_down_image": x4.to(device)}


class SyntheticSRDataProvider(object):
    """attributes mirror DataProvider (base_provider.py): data_shape, image_size, train/valid/test."""

    def __init__(self, train_batch_size=16, test_batch_size=1, image_size=256, n_train_batches=4,
                 n_test_batches=2, seed=0, rank=0, num_replicas=1, device="cpu", test_sizes=None, crop_candidates=1,
                 degrade=None, degrade_seed=0, lr_on_device=False):
        self.image_size = image_size
        self.active_img_size = image_size
        self.n_classes = None
        g = torch.Generator().manual_seed(seed * 1000003 + rank)
        self.crop_candidates = int(crop_candidates)
        self.degrade, self.degrade_seed = degrade, int(degrade_seed)
        if self.crop_candidates != 1 or degrade is not None:
            self.train = self._resident_train(train_batch_size, image_size, n_train_batches, g)
        else:
            self.train = _ListLoader(make_batch(train_batch_size, image_size, g, device) for _ in range(n_train_batches))
        gt = torch.Generator().manual_seed(seed * 1000003 + 7919)
        sizes = test_sizes or [image_size] * n_test_batches
        # validation runs batch-1 full images whose sides are multiples of 4 (ModCrop(4), div2k_setxx.py:182-190)
        self.test = _ListLoader(make_batch(test_batch_size, s, gt, device) for s in sizes)
        if lr_on_device:   # as Div2K_SetXXDataProvider(lr_on_device=True): the items carry the uint8 HR image alone
            self.test = _ListLoader({"image_u8": b["image"].mul(255.0).round_().to(torch.uint8)} for b in self.test)
        self.valid = self.test

    def _resident_train(self, batch_size, size, n_batches, g):
        """crop_candidates = K > 1 or degrade=spec: both run on a resident pool, so the training images -- one per
        sample of an epoch, twice the crop's side, the left half one flat grey and the right half noise -- live in an
        augment.ResidentArraySet and `train` is the resident loader over it, in file order"""
        from .augment import ResidentArraySet, ResidentTrainLoader
        images = []
        for _ in range(n_batches * batch_size):
            a = torch.randint(0, 256, (2 * size, 2 * size, 3), generator=g, dtype=torch.uint8)
            a[:, :size] = a[0, 0, 0]
            images.append(a.numpy())
        self.resident_set = ResidentArraySet(images, torch.device("cuda", torch.cuda.current_device()))
        return ResidentTrainLoader(self.resident_set, batch_size, list(range(len(images))), size, drop_last=True,
                                   want_f32=True, candidates=self.crop_candidates,
                                   **({} if self.degrade is None else dict(degrade=self.degrade,
                                                                           degrade_seed=self.degrade_seed)))

    @staticmethod
    def name():
        return "synthetic_sr"

    @property
    def data_shape(self):
        return 3, self.active_img_size, self.active_img_size

    def build_sub_train_loader(self, n_images, batch_size, num_worker=None, num_replicas=None, rank=None):
        if self.crop_candidates != 1 or self.degrade is not None:   # BN re-calibration sees plain crops: no selection, no
            # degradation, cached like the providers'
            if self.__dict__.get("_sub_train") is None:
                from .augment import ResidentTrainLoader
                t = self.train
                self._sub_train = _ListLoader(ResidentTrainLoader(t.dataset, t.batch_size, t.sampler, t.size,
                                                                  drop_last=True, want_f32=True))
            return self._sub_train
        return self.train
