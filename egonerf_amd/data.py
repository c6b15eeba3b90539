"""Pose / ray ingestion for equirectangular datasets: host-side mirror of dataLoader/dataset_omniblender.py:11-95 (OmniBlender
`transform.json` + `{split}.txt` lists) with the rays generated on the HIP device (ego_erp_rays) instead of on the CPU.

Same attribute surface as the reference's dataset object where the render / training loop reads it: `poses [K,4,4]`, `img_wh`,
`near_far`, `center`, `scene_bbox [2,3]` (dataset_omniblender.py:22-32: camera-position centre +- (half diagonal of the camera
positions' extent + far)), `radius`, `all_rays`, `all_rgbs`, `image_paths`, `white_bg`, `indoor`.

`RayBank` is the device-resident alternative to `all_rays` / `all_rgbs`: the poses and the 8-bit images stay on the device and a row
of either array is computed when it is asked for (ego_ray_batch_gather), bit-equal to the materialised one.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib


class RayBank:
    """K poses + K uint8 images on the device, standing for the reference's `all_rays [K*h*w, 6]` / `all_rgbs [K*h*w, 3]`
    (dataset_omniblender.py:81-89) at 4 B per pixel + 48 B per image instead of 36 B per pixel.

    poses [K,4,4] or [K,3,4] camera-to-world; images_u8 [K,H,W,3|4] uint8 (array or tensor; RGB is stored as RGBA with A = 255);
    img_wh = (W, H); roi = (h0, h1, w0, w1) fractions as in get_rays (ray_utils.py:100-103).  Index space = the layout of
    `all_rays`: idx = img * (n_rows * n_cols) + row * n_cols + col, (row, col) inside the ROI window.  With a ROI the colours are those
    of the window's pixels, i.e. the rows of the per-image `all_rgbs` that belong to the rays (`all_rgbs` itself keeps every pixel
    of the image, as the reference's does).

    depths (optional) [K,H,W] float32 or float16 (array or tensor): one depth target per pixel of the full images, in units of distance
    along the normalised ray, 0 = no target (losses.depth_loss leaves such a ray out).  Kept on the device in its own dtype;
    `gather_depth(idx)` returns the targets of ray indices as float32.  The reference defines no depth file format (its loaders never
    fill all_depth, dataset_interface.py:41), so reading one is the caller's business.

    masks (optional) [K,H,W] uint8 (0 = ignore the pixel, 255 = full weight) or bool (stored as 0 / 255), array or tensor: one value per
    pixel of the full images - the photographer, the tripod at the nadir, the stitching seam (the Ricoh360 layout ships a mask.png next
    to its images; dataset_egocentric_video.py drops it from the file list and never builds the all_masks it reads).  Kept on the
    device as uint8; `gather_mask(idx)` returns mask / 255 of ray indices as float32, the `weight` of losses.photometric_loss.  The
    samplers do not look at the masks: masked pixels are still drawn and carry weight 0, so a nadir mask wastes the masked share of a
    batch, and the loss normalises by the sum of the weights it did get.

    A bank on device="cpu" holds the host state only (shapes, window, struct): gather / sampling need the HIP device."""

    def __init__(self, poses, images_u8, img_wh: Sequence[int], roi: Sequence[float] = (0, 1, 0, 1), normalize: bool = True, device="cuda",
                 depths=None, masks=None):
        W, H = int(img_wh[0]), int(img_wh[1])
        poses = torch.as_tensor(np.asarray(poses) if not torch.is_tensor(poses) else poses).float()
        if poses.dim() != 3 or poses.shape[1] not in (3, 4) or poses.shape[2] != 4:
            raise ValueError(f"RayBank: poses must be [K,4,4] or [K,3,4], got {tuple(poses.shape)}")
        img = images_u8 if torch.is_tensor(images_u8) else torch.from_numpy(np.ascontiguousarray(images_u8))
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[-1] not in (3, 4):
            raise ValueError(f"RayBank: images must be uint8 [K,H,W,3|4], got {img.dtype} {tuple(img.shape)}")
        K = poses.shape[0]
        if K < 1 or tuple(img.shape[:3]) != (K, H, W):
            raise ValueError(f"RayBank: {K} poses and img_wh {(W, H)} do not match images {tuple(img.shape)}")
        if img.shape[-1] == 3:
            img = torch.cat([img, torch.full_like(img[..., :1], 255)], dim=-1)
        h0, h1, w0, w1 = roi
        r0, r1, c0, c1 = int(h0 * H), int(h1 * H), int(w0 * W), int(w1 * W)     # ray_utils.py:100-103
        if not (0 <= r0 < r1 <= H and 0 <= c0 < c1 <= W):
            raise ValueError(f"RayBank: roi {list(roi)} selects no pixel of a {H} x {W} image")
        self.device = torch.device(device)
        self.poses = poses[:, :3, :].contiguous().to(self.device)
        self.images = img.contiguous().to(self.device)
        self.depths = None
        if depths is not None:
            d = depths if torch.is_tensor(depths) else torch.from_numpy(np.ascontiguousarray(depths))
            if d.dtype not in (torch.float32, torch.float16) or tuple(d.shape) != (K, H, W):
                raise ValueError(f"RayBank: depths must be float32 or float16 [K,H,W] = {(K, H, W)}, got {d.dtype} {tuple(d.shape)}")
            self.depths = d.detach().contiguous().to(self.device)
        self.masks = None
        if masks is not None:
            m = masks if torch.is_tensor(masks) else torch.from_numpy(np.ascontiguousarray(masks))
            if m.dtype not in (torch.uint8, torch.bool) or tuple(m.shape) != (K, H, W):
                raise ValueError(f"RayBank: masks must be uint8 or bool [K,H,W] = {(K, H, W)}, got {m.dtype} {tuple(m.shape)}")
            m = m.detach()
            self.masks = (m.to(torch.uint8) * 255 if m.dtype == torch.bool else m).contiguous().to(self.device)
        self.K, self.H, self.W = K, H, W
        self.r0, self.n_rows, self.c0, self.n_cols = r0, r1 - r0, c0, c1 - c0
        self.roi, self.normalize = list(roi), bool(normalize)
        self.total = K * self.n_rows * self.n_cols
        self.struct = _lib.RayBankStruct(self.poses.data_ptr(), self.images.data_ptr(), K, H, W, self.r0, self.n_rows, self.c0, self.n_cols,
                                         int(self.normalize))

    @property
    def nbytes(self) -> int:
        """Bytes the bank holds (on its device): K * H * W * 4 for the images + K * 48 for the poses (+ K * H * W * 4 or 2 for depths, + K * H * W for masks)."""
        depth = 0 if self.depths is None else self.depths.numel() * self.depths.element_size()
        mask = 0 if self.masks is None else self.masks.numel()
        return self.images.numel() * self.images.element_size() + self.poses.numel() * self.poses.element_size() + depth + mask

    def __len__(self) -> int:
        return self.total

    def image_of(self, idx: torch.Tensor) -> torch.Tensor:
        """The image index of ray indices (int64, any device): idx // (n_rows * n_cols), the index space of the class docstring."""
        return torch.div(idx, self.n_rows * self.n_cols, rounding_mode="floor")

    def gather(self, idx: torch.Tensor):
        """(rays [B,6], rgb [B,3]) = (all_rays[idx], all_rgbs[idx]) of the materialised arrays, bit for bit.  idx: int64 on the bank's
        device, every entry in [0, total) (not checked - that would synchronise; a row with an index outside comes back as NaN)."""
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous().view(-1)
        rays = torch.empty(idx.shape[0], 6, device=self.device, dtype=torch.float32)
        rgb = torch.empty(idx.shape[0], 3, device=self.device, dtype=torch.float32)
        ray_batch_gather(idx, rays, rgb, self)
        return rays, rgb

    def gather_depth(self, idx: torch.Tensor) -> torch.Tensor:
        """[B] float32: the depth targets of ray indices, bit-equal to indexing the `depths` array at the rays' pixels.  idx as in
        `gather`; an index outside [0, total) gives NaN, which losses.depth_loss treats as "no target"."""
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous().view(-1)
        out = torch.empty(idx.shape[0], device=self.device, dtype=torch.float32)
        self.gather_depth_into(idx, out)
        return out

    def gather_depth_into(self, idx: torch.Tensor, out: torch.Tensor) -> None:
        """ego_ray_batch_gather_depth into a caller-owned buffer (idx [B] int64, out [B] float32, contiguous, on the bank's device): one
        launch, no allocation - what GraphedTrainStep captures after the batch source's own launch."""
        if self.depths is None:
            raise ValueError("RayBank.gather_depth: this bank was built without depths")
        _need_hip(idx, "RayBank.gather_depth")
        if idx.dtype != torch.int64 or out.dtype != torch.float32 or idx.dim() != 1 or out.shape != idx.shape or not idx.is_contiguous() \
                or not out.is_contiguous() or out.device != idx.device:
            raise RuntimeError("RayBank.gather_depth_into: idx must be int64 [B] and out float32 [B], contiguous, on the bank's device")
        _gather_depth(idx, out, self)

    def gather_mask(self, idx: torch.Tensor) -> torch.Tensor:
        """[B] float32: mask / 255 at the pixels of ray indices, bit-equal to indexing the `masks` array there and dividing.  idx as in
        `gather`; an index outside [0, total) gives NaN, which losses.photometric_loss treats as an invalid ray."""
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous().view(-1)
        out = torch.empty(idx.shape[0], device=self.device, dtype=torch.float32)
        self.gather_mask_into(idx, out)
        return out

    def gather_mask_into(self, idx: torch.Tensor, out: torch.Tensor) -> None:
        """ego_ray_batch_gather_mask into a caller-owned buffer (idx [B] int64, out [B] float32, contiguous, on the bank's device): one
        launch, no allocation - what GraphedTrainStep captures after the batch source's own launch."""
        if self.masks is None:
            raise ValueError("RayBank.gather_mask: this bank was built without masks")
        _need_hip(idx, "RayBank.gather_mask")
        if idx.dtype != torch.int64 or out.dtype != torch.float32 or idx.dim() != 1 or out.shape != idx.shape or not idx.is_contiguous() \
                or not out.is_contiguous() or out.device != idx.device:
            raise RuntimeError("RayBank.gather_mask_into: idx must be int64 [B] and out float32 [B], contiguous, on the bank's device")
        _gather_mask(idx, out, self)


def _need_hip(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what} needs a HIP device (no CPU fallback exists); the bank lives on {t.device}")


def ray_batch_gather(idx: torch.Tensor, rays: Optional[torch.Tensor], rgb: Optional[torch.Tensor], bank: RayBank) -> None:
    """ego_ray_batch_gather into caller-owned buffers (contiguous float32 [B,6] / [B,3], either may be None)."""
    _need_hip(idx, "RayBank.gather")
    _gather(idx, rays, rgb, bank)


def ray_batch_sample(idx: torch.Tensor, rays: Optional[torch.Tensor], rgb: Optional[torch.Tensor], bank: RayBank, mode: int, seed: int,
                     counter: torch.Tensor, row_cdf: Optional[torch.Tensor]) -> None:
    """ego_ray_batch_sample into caller-owned buffers: idx [B] int64, rays [B,6] / rgb [B,3] float32 or None; counter = int64 device
    scalar holding the iteration to draw (read by the kernel, so a captured launch follows it)."""
    _need_hip(idx, "ray batch sampling")
    _sample(idx, rays, rgb, bank, mode, seed, counter, row_cdf)


def ray_batch_sample_patches(idx: torch.Tensor, rays: Optional[torch.Tensor], rgb: Optional[torch.Tensor], bank: RayBank, seed: int,
                             counter: torch.Tensor, patches: int, patch: Sequence[int], stride: int, n_random: int) -> None:
    """ego_ray_batch_sample_patches into caller-owned buffers: idx [patches * ph * pw + n_random] int64, rays / rgb float32 or None;
    counter as in `ray_batch_sample`."""
    _need_hip(idx, "patch batch sampling")
    if idx.shape[0] != patches * patch[0] * patch[1] + n_random:
        raise RuntimeError(f"patch batch sampling: idx holds {idx.shape[0]} rows, the batch {patches * patch[0] * patch[1] + n_random}")
    _sample_patches(idx, rays, rgb, bank, seed, counter, patches, patch, stride, n_random)


def check_patch_shape(what: str, bank: RayBank, patch, stride) -> tuple:
    """(ph, pw, stride) as ints, refused unless each is >= 1 and the patch's extent fits the bank's window."""
    if not (isinstance(patch, (tuple, list)) and len(patch) == 2):
        raise ValueError(f"{what}: patch must be (ph, pw), not {patch!r}")
    ph, pw, stride = int(patch[0]), int(patch[1]), int(stride)
    if ph < 1 or pw < 1 or stride < 1:
        raise ValueError(f"{what}: ph, pw and stride must be >= 1 (patch {ph} x {pw}, stride {stride})")
    ext = ((ph - 1) * stride + 1, (pw - 1) * stride + 1)
    if ext[0] > bank.n_rows or ext[1] > bank.n_cols:
        raise ValueError(f"{what}: a patch of {ext[0]} x {ext[1]} pixels does not fit the bank's window of {bank.n_rows} x {bank.n_cols}")
    return ph, pw, stride


def patch_indices(bank: RayBank, img, row0, col0, patch: Sequence[int], stride: int = 1) -> torch.Tensor:
    """The index block of patches with given origins, in DevicePatchSampler's layout: [P * ph * pw] int64 (on img's device), row
    p ph pw + a pw + b = pixel (row0[p] + a stride, col0[p] + b stride) of image img[p] in the bank's index space.  img, row0, col0: [P]
    integer tensors (or sequences), rows and columns counted inside the bank's window.  When the window spans the full width the columns
    wrap (modulo n_cols) and col0 may be any column; otherwise the patch must fit.  Pure torch: works on any device."""
    ph, pw, stride = check_patch_shape("patch_indices", bank, patch, stride)
    img, row0, col0 = (torch.as_tensor(t, dtype=torch.int64) for t in (img, row0, col0))
    if img.dim() != 1 or row0.shape != img.shape or col0.shape != img.shape:
        raise ValueError("patch_indices: img, row0 and col0 must be [P] integer tensors of one length")
    row0, col0 = row0.to(img.device), col0.to(img.device)
    wrap = bank.c0 == 0 and bank.n_cols == bank.W
    if img.numel():
        last_col = bank.n_cols - 1 if wrap else bank.n_cols - ((pw - 1) * stride + 1)
        if int(img.min()) < 0 or int(img.max()) >= bank.K or int(row0.min()) < 0 or int(row0.max()) > bank.n_rows - ((ph - 1) * stride + 1) \
                or int(col0.min()) < 0 or int(col0.max()) > last_col:
            raise ValueError("patch_indices: an origin lies outside the bank (image in [0, K), rows so that the patch fits, columns so "
                             "that it fits or, on a full-width window, any column)")
    rows = row0[:, None] + torch.arange(ph, device=img.device) * stride                 # [P, ph]
    cols = col0[:, None] + torch.arange(pw, device=img.device) * stride                 # [P, pw]
    if wrap:
        cols = cols % bank.n_cols
    idx = img[:, None, None] * (bank.n_rows * bank.n_cols) + rows[:, :, None] * bank.n_cols + cols[:, None, :]
    return idx.reshape(-1)


@_lib.device_guard
def _sample_patches(idx, rays, rgb, bank, seed, counter, patches, patch, stride, n_random):
    _lib.check(_lib.load().ego_ray_batch_sample_patches(C.byref(bank.struct), int(seed), counter.data_ptr(), int(patches), int(patch[0]),
                                                        int(patch[1]), int(stride), int(n_random), idx.data_ptr(), _lib.ptr(rays),
                                                        _lib.ptr(rgb), _lib.stream_handle()), "ego_ray_batch_sample_patches")


@_lib.device_guard
def _gather(idx, rays, rgb, bank):
    _lib.check(_lib.load().ego_ray_batch_gather(C.byref(bank.struct), idx.data_ptr(), idx.shape[0], _lib.ptr(rays), _lib.ptr(rgb),
                                                _lib.stream_handle()), "ego_ray_batch_gather")


@_lib.device_guard
def _gather_depth(idx, out, bank):
    _lib.check(_lib.load().ego_ray_batch_gather_depth(C.byref(bank.struct), bank.depths.data_ptr(), int(bank.depths.dtype == torch.float16),
                                                      idx.data_ptr(), idx.shape[0], out.data_ptr(), _lib.stream_handle()),
               "ego_ray_batch_gather_depth")


@_lib.device_guard
def _gather_mask(idx, out, bank):
    _lib.check(_lib.load().ego_ray_batch_gather_mask(C.byref(bank.struct), bank.masks.data_ptr(), idx.data_ptr(), idx.shape[0], out.data_ptr(),
                                                     _lib.stream_handle()), "ego_ray_batch_gather_mask")


@_lib.device_guard
def _sample(idx, rays, rgb, bank, mode, seed, counter, row_cdf):
    _lib.check(_lib.load().ego_ray_batch_sample(C.byref(bank.struct), int(mode), int(seed), counter.data_ptr(), _lib.ptr(row_cdf),
                                                idx.shape[0], idx.data_ptr(), _lib.ptr(rays), _lib.ptr(rgb), _lib.stream_handle()),
               "ego_ray_batch_sample")


class OmniBlenderDataset:
    def __init__(self, data_dir: str, split: str = "train", near_far: Sequence[float] = (0.1, 15.0), downsample: float = 1.0,
                 is_stack: bool = False, skip: int = 1, roi: Sequence[float] = (0, 1, 0, 1), device="cuda", load_images: bool = True,
                 **_ignored):
        self.root_dir, self.split, self.is_stack, self.skip = data_dir, split, is_stack, skip
        self.near_far, self.downsample, self.roi, self.device = list(near_far), downsample, list(roi), device
        self.white_bg = False
        self.blender2opencv = np.eye(4)                                            # dataset_interface.py:20
        self.img_wh = (int(2000 / downsample), int(1000 / downsample))              # dataset_omniblender.py:15
        self.img_list: List[str] = []
        self.image_paths: List[str] = []
        self._rays = self._rgbs = None
        self.read_meta(load_images)
        self.scene_bbox = self.get_scene_bbox()
        self.radius = (self.scene_bbox[1] - self.center).float().view(1, 1, 3)

    # dataset_omniblender.py:22-32
    def get_scene_bbox(self) -> torch.Tensor:
        cam = self.poses[:, :3, 3]
        self.center = cam.mean(0)
        trajectory_radius = (cam.max(0).values - cam.min(0).values).pow(2).sum(0).sqrt().div(2).float()
        return torch.stack([self.center - trajectory_radius - self.near_far[1], self.center + trajectory_radius + self.near_far[1]])

    # dataset_omniblender.py:34-95 (poses and image list; rays are produced by `rays()` on the device)
    def read_meta(self, load_images: bool) -> None:
        with open(os.path.join(self.root_dir, "transform.json"), "r") as f:
            self.meta = json.load(f)
        self.indoor = self.meta["indoor"]
        if self.split not in ("train", "test"):
            raise ValueError("Unknown split: {}".format(self.split))
        with open(os.path.join(self.root_dir, f"{self.split}.txt")) as f:
            self.img_list = [line.strip() for line in f if line.strip()]
        if self.split == "train":
            assert self.skip == 1, "skip must be 1 for training"
        self.img_list = self.img_list[::self.skip]
        names = [fr["file_path"].split(".")[0] for fr in self.meta["frames"]]
        poses, rgbs = [], []
        for img_name in self.img_list:
            frame = self.meta["frames"][names.index(img_name)]
            poses.append(torch.FloatTensor(np.array(frame["transform_matrix"]) @ self.blender2opencv))
            path = os.path.join(self.root_dir, "images", f"{frame['file_path']}")
            self.image_paths.append(path)
            if load_images and os.path.exists(path):
                rgbs.append(self._load_image(path))
        self.poses = torch.stack(poses)
        if rgbs:
            self._rgbs = rgbs

    def _load_image(self, path: str) -> torch.Tensor:
        """dataset_omniblender.py:66-77: PIL image (LANCZOS resize when downsampling) -> ToTensor -> [h*w, 3], alpha blended on white."""
        from PIL import Image
        img = Image.open(path)
        if self.downsample != 1.0:
            img = img.resize(self.img_wh, Image.LANCZOS)
        a = np.asarray(img)
        if a.ndim == 2:
            a = a[..., None]
        t = torch.from_numpy(np.array(a)).float().div(255.0)                        # ToTensor: uint8 HWC -> float / 255
        t = t.view(-1, t.shape[-1])
        if t.shape[-1] == 4:
            t = t[:, :3] * t[:, -1:] + (1 - t[:, -1:])
        return t

    def _load_image_u8(self, path: str) -> np.ndarray:
        """The same PIL image as `_load_image` (after the LANCZOS resize when downsampling), kept as uint8 [h, w, 3|4]."""
        from PIL import Image
        img = Image.open(path)
        if self.downsample != 1.0:
            img = img.resize(self.img_wh, Image.LANCZOS)
        a = np.array(img)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[-1] not in (3, 4):
            raise ValueError(f"ray_bank: {path} is not an 8-bit RGB / RGBA image (array {a.dtype} {a.shape})")
        return a

    def ray_bank(self, device=None, depths=None, masks=None) -> RayBank:
        """The training rays and colours as a device-resident `RayBank` (poses + uint8 images read from disk here): what
        `all_rays[idx]` / `all_rgbs[idx]` return, without materialising either array.  `depths` ([K,h,w] float32 / float16, see RayBank)
        is passed through: the reference defines no depth file format, so none is read here.  `masks` ([K,h,w] uint8 / bool, see RayBank)
        is passed through as well."""
        if self.is_stack:
            raise ValueError("ray_bank: the flat ray index space is that of is_stack=False")
        imgs = np.stack([self._load_image_u8(p) for p in self.image_paths], 0)
        return RayBank(self.poses, imgs, self.img_wh, roi=self.roi, normalize=True, device=device or self.device, depths=depths, masks=masks)

    def rays(self, idx: int, device=None) -> torch.Tensor:
        """[h*w, 6] rays of image `idx`: get_ray_directions_360 + normalisation + get_rays(roi) (dataset_omniblender.py:41-43,79),
        generated on the device."""
        from .renderer import erp_rays
        w, h = self.img_wh
        h0, h1, w0, w1 = self.roi
        r0, r1, c0, c1 = int(h0 * h), int(h1 * h), int(w0 * w), int(w1 * w)       # ray_utils.py:100-103
        rays = erp_rays(h, w, self.poses[idx][:3].numpy(), device or self.device, r0, r1 - r0, normalize=True)
        if (c0, c1) != (0, w):
            rays = rays.view(r1 - r0, w, 6)[:, c0:c1].reshape(-1, 6)
        return rays

    @property
    def all_rays(self) -> torch.Tensor:
        """[K*h*w, 6] (or [K, h*w, 6] when is_stack), like dataset_omniblender.py:82-90; materialised on the device on first use."""
        if self._rays is None:
            per = [self.rays(i) for i in range(len(self.poses))]
            self._rays = torch.stack(per, 0) if self.is_stack else torch.cat(per, 0)
        return self._rays

    @property
    def all_rgbs(self) -> Optional[torch.Tensor]:
        if self._rgbs is None:
            return []
        if isinstance(self._rgbs, list):
            w, h = self.img_wh
            self._rgbs = torch.stack(self._rgbs, 0).reshape(-1, h, w, 3) if self.is_stack else torch.cat(self._rgbs, 0)
        return self._rgbs

    def world2ndc(self, points, lindisp=None):
        return (points - self.center.to(points.device)) / self.radius.to(points.device)

    def __len__(self):
        return len(self.poses)
