"""Training ray-index samplers: mirror of sampler.py:4-38 (CPU, numpy legacy RNG so that
np.random.seed(20221028) (train.py:413) reproduces the reference's index stream), and their device-resident counterparts
(`DeviceSimpleSampler`, `DeviceThetaImportanceSampler`): the same two sampling rules drawn by a counter-based generator inside
one kernel launch together with the batch's rays and colours (ego_ray_batch_sample) - another index stream, no host work."""
import numpy as np
import torch


class SimpleSampler:
    """Permutation epochs; re-permutes when fewer than two batches remain, so the tail of every
    permutation is dropped (sampler.py:11-16)."""

    def __init__(self, total, batch):
        self.total, self.batch = total, batch
        self.curr = total
        self.ids = None

    def nextids(self):
        self.curr += self.batch
        if self.curr + self.batch > self.total:
            self.ids = torch.LongTensor(np.random.permutation(self.total))
            self.curr = 0
        return self.ids[self.curr:self.curr + self.batch]


class ThetaImportanceSampler:
    """Uniform image and column, row drawn with p ~ cos(latitude)*lambda + 1 (sampler.py:19-38)."""

    def __init__(self, theta_importance_lambda, img_len, img_wh, batch, roi):
        self.img_len, self.batch = img_len, batch
        W, H = img_wh
        self.W = int(W * (roi[3] - roi[2]))
        self.H = int(H * (roi[1] - roi[0]))
        self.weight = self.get_weight(theta_importance_lambda, H, roi)

    def get_weight(self, theta_importance_lambda, h, roi):
        rows = np.arange(h)[int(h * roi[0]):int(h * roi[1])]
        lat = -(rows - h // 2) / h * np.pi
        w = np.cos(lat) * theta_importance_lambda + 1
        return w / np.sum(w)

    def nextids(self):
        img = np.random.choice(self.img_len, self.batch)
        col = np.random.choice(self.W, self.batch)
        row = np.random.choice(self.H, self.batch, p=self.weight)
        return img * self.W * self.H + (col + row * self.W)


class _DeviceSampler:
    """Indices, rays and colours of training batch number `counter` from a `RayBank` (egonerf_amd.data), drawn on the device: every
    index is a pure function of (seed, counter, lane).  `counter` is an int64 device scalar the kernel reads, so a launch captured
    into a hipGraph draws a new batch at every replay once the counter is advanced inside the graph (GraphedTrainStep does)."""
    mode = None

    def __init__(self, bank, batch, seed=0):
        self.bank, self.batch = bank, int(batch)
        self.seed = int(seed) & (2 ** 64 - 1)
        if self.batch < 1:
            raise ValueError("batch must be >= 1")
        self.counter = torch.zeros((), dtype=torch.int64, device=bank.device)
        self.cdf = None

    def sample_into(self, idx, rays, rgb, counter=None):
        """One launch: idx [batch] int64 and (unless None) rays [batch,6], rgb [batch,3] for iteration `counter` (default: the
        sampler's own device counter, which is NOT advanced here)."""
        from .data import ray_batch_sample
        ray_batch_sample(idx, rays, rgb, self.bank, self.mode, self.seed, self.counter if counter is None else counter, self.cdf)

    def next_batch(self):
        """(idx, rays, rgb) of the current iteration; advances the counter on the device (no synchronisation)."""
        dev = self.bank.device
        idx = torch.empty(self.batch, dtype=torch.int64, device=dev)
        rays, rgb = torch.empty(self.batch, 6, device=dev), torch.empty(self.batch, 3, device=dev)
        self.sample_into(idx, rays, rgb)
        self.counter.add_(1)
        return idx, rays, rgb

    def indices_at(self, counter: int) -> torch.Tensor:
        """The indices iteration `counter` draws (pure: the sampler's own counter is untouched)."""
        dev = self.bank.device
        idx = torch.empty(self.batch, dtype=torch.int64, device=dev)
        self.sample_into(idx, None, None, torch.full((), int(counter), dtype=torch.int64, device=dev))
        return idx

    def seek(self, counter: int) -> None:
        """Positions the device counter (resuming a run at iteration `counter`)."""
        self.counter.fill_(int(counter))


class DeviceSimpleSampler(_DeviceSampler):
    """SimpleSampler's rule (sampler.py:4-16) - permutation epochs of floor(total / batch) batches, the tail of each permutation
    dropped - without a permutation in memory: position -> index through a keyed bijection of [0, total) (Feistel network with
    cycle-walking, keys from (seed, epoch))."""
    mode = 0   # EGO_BATCH_SIMPLE

    def __init__(self, bank, batch, seed=0):
        super().__init__(bank, batch, seed)
        if bank.total < 2 * self.batch:
            raise ValueError(f"DeviceSimpleSampler: {bank.total} rays do not hold two batches of {self.batch}")
        self.batches_per_epoch = bank.total // self.batch


class DeviceThetaImportanceSampler(_DeviceSampler):
    """ThetaImportanceSampler's rule (sampler.py:19-38): image and column uniform, row by inverse CDF of cos(latitude) * lambda + 1
    over the bank's ROI rows.  The weights are ThetaImportanceSampler.get_weight's; the table is their float32 cumulative sum with
    the last entry 1."""
    mode = 1   # EGO_BATCH_THETA

    def __init__(self, theta_importance_lambda, bank, batch, seed=0):
        super().__init__(bank, batch, seed)
        host = ThetaImportanceSampler(theta_importance_lambda, bank.K, (bank.W, bank.H), self.batch, bank.roi)
        if len(host.weight) != bank.n_rows:
            raise ValueError("DeviceThetaImportanceSampler: the roi rows of the weights and of the bank differ")
        self.weight = host.weight
        cdf = np.cumsum(host.weight).astype(np.float32)
        cdf[-1] = 1.0
        self.cdf_host = cdf
        self.cdf = torch.from_numpy(cdf).to(bank.device)


class DevicePatchSampler(_DeviceSampler):
    """Batches with known neighbours (no reference counterpart: its samplers draw independent pixels): `patches` patches of ph x pw pixels
    `stride` apart, then `n_random` independent uniform pixels, one launch (ego_ray_batch_sample_patches states the rule).  Row
    p ph pw + a pw + b of the batch is pixel (row0_p + a stride, col0_p + b stride) of image img_p, so `rgb[:n_patch_rays]` reads as
    [patches, ph, pw, 3] - the layout losses.patch_ssim_loss takes.  Image and origin are uniform; on a bank whose window spans the full
    width a patch may straddle the panorama's seam (columns modulo n_cols).  The indices live in the bank's index space: `bank.gather`,
    `gather_depth_into`, `gather_mask_into` and `image_of` work on them, and GraphedTrainStep(batch_source=...) takes the sampler as it
    takes the other two."""

    def __init__(self, bank, patches, patch=(8, 8), stride=1, n_random=0, seed=0):
        from .data import check_patch_shape
        self.patches, self.n_random = int(patches), int(n_random)
        if self.patches < 0 or self.n_random < 0:
            raise ValueError("DevicePatchSampler: patches and n_random must be >= 0")
        self.ph, self.pw, self.stride = check_patch_shape("DevicePatchSampler", bank, patch, stride)
        self.patch = (self.ph, self.pw)
        self.n_patch_rays = self.patches * self.ph * self.pw
        super().__init__(bank, self.n_patch_rays + self.n_random, seed)

    def sample_into(self, idx, rays, rgb, counter=None):
        """One launch: idx [batch] int64 and (unless None) rays [batch,6], rgb [batch,3] for iteration `counter` (default: the
        sampler's own device counter, which is NOT advanced here)."""
        from .data import ray_batch_sample_patches
        ray_batch_sample_patches(idx, rays, rgb, self.bank, self.seed, self.counter if counter is None else counter, self.patches, self.patch,
                                 self.stride, self.n_random)
