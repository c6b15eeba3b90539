"""Per-image colour correction for real captures: a consumer 360 camera meters every frame, so K images of one scene differ by
exposure and white balance.  `ExposureDeltas` is the learnt correction next to `poses.PoseDeltas` (an affine map per image and channel,
applied to the RENDERED colour inside losses.photometric_loss, so the field keeps one radiance); `fit_exposure` is the closed-form
least-squares map (csrc/ego_photo.hip: ego_photo_fit), and `align` the evaluation protocol built on it: a held-out image has no learnt
correction, so PSNR against it is taken after fitting one.  No reference counterpart: there the only colour term is the plain MSE.

Apart from the fit (one kernel launch over the batch) this is plain torch on [K, 3] parameters."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .losses import _photo_args


class ExposureDeltas(torch.nn.Module):
    """One colour correction per image: `log_gain` [K, 3] and `bias` [K, 3], zero-initialised, so `affine()` starts as the identity.
    A rendered colour c of image i is compared to its target as exp(log_gain[i]) * c + bias[i].

    The field and the corrections share a gauge: scaling every gain by s and the field's radiance by 1 / s changes no residual.
    `anchor=i` removes it by keeping image i at the identity - its row of `affine()` is the constant (1, 0) and its parameters get
    exactly zero gradient, so Adam never moves them.  Without an anchor a small L2 penalty on `log_gain` and `bias` does the same."""

    def __init__(self, K: int, device=None, anchor: Optional[int] = None):
        super().__init__()
        if int(K) < 1:
            raise ValueError("ExposureDeltas: K must be >= 1")
        if anchor is not None and not 0 <= int(anchor) < int(K):
            raise ValueError(f"ExposureDeltas: anchor must be an image index in [0, {int(K)}), not {anchor!r}")
        self.K, self.anchor = int(K), (None if anchor is None else int(anchor))
        self.log_gain = torch.nn.Parameter(torch.zeros(self.K, 3, device=device))
        self.bias = torch.nn.Parameter(torch.zeros(self.K, 3, device=device))
        free = torch.ones(self.K, 1, device=device, dtype=torch.bool)
        if self.anchor is not None:
            free[self.anchor] = False
        self.register_buffer("free", free, persistent=False)

    def affine(self) -> torch.Tensor:
        """[K, 3, 2] float32 (gain, bias) = (exp(log_gain), bias); the anchor's row is (1, 0) whatever its parameters hold."""
        if self.anchor is None:
            return torch.stack([torch.exp(self.log_gain), self.bias], dim=-1)
        # the anchor's row is a constant 0 selected in its parameters' place: the gradient that comes back to them is exactly 0
        zero = torch.zeros_like(self.log_gain)
        return torch.stack([torch.exp(torch.where(self.free, self.log_gain, zero)), torch.where(self.free, self.bias, zero)], dim=-1)

    @torch.no_grad()
    def set_from_affine(self, affine: torch.Tensor) -> None:
        """Loads a fitted map ([K, 3, 2], e.g. fit_exposure's): log_gain = log(gain), bias = bias.  Gains <= 0 (or not finite) have no
        logarithm and are refused; with an anchor, the anchor's row is left at zero."""
        a = torch.as_tensor(affine)
        if tuple(a.shape) != (self.K, 3, 2):
            raise ValueError(f"ExposureDeltas.set_from_affine: affine must be [K, 3, 2] = {(self.K, 3, 2)}, got {tuple(a.shape)}")
        a = a.detach().to(self.log_gain.device, torch.float32)
        gain = a[..., 0]
        if not bool(((gain > 0) & torch.isfinite(gain)).all()):
            raise ValueError("ExposureDeltas.set_from_affine: every gain must be finite and > 0")
        self.log_gain.copy_(torch.where(self.free, torch.log(gain), torch.zeros_like(gain)))
        self.bias.copy_(torch.where(self.free, a[..., 1], torch.zeros_like(gain)))


@_lib.device_guard
def _fit(rgb, target, weight, image, K):
    out = torch.empty(K, 3, 2, device=rgb.device, dtype=torch.float32)
    _lib.check(_lib.load().ego_photo_fit(rgb.data_ptr(), target.data_ptr(), _lib.ptr(weight), _lib.ptr(image), rgb.shape[0], K,
                                         out.data_ptr(), None, _lib.stream_handle()), "ego_photo_fit")
    return out


def fit_exposure(rgb: torch.Tensor, target: torch.Tensor, image: Optional[torch.Tensor] = None, K: int = 1,
                 weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[K, 3, 2] float32: per image and channel the (gain, bias) that minimise sum w (gain * rgb + bias - target)^2 over the image's
    valid rays (photometric_loss's rule), in closed form from float64 moments.  An image without a valid ray gets (1, 0); one whose
    colours are all equal gets gain 1 and the bias that matches the means.  rgb, target [N, 3]; image [N] int (omitted: one image, K
    must be 1); weight [N] float32.  No gradient."""
    if int(K) < 1:
        raise ValueError("fit_exposure: K must be >= 1")
    if image is None and int(K) != 1:
        raise ValueError("fit_exposure: K > 1 needs image (the image index of every ray)")
    target, weight, image = _photo_args("fit_exposure", rgb, target, weight, image)
    c = rgb.detach()
    if c.dtype != torch.float32 or not c.is_contiguous():
        c = c.float().contiguous()
    return _fit(c, target, weight, image, int(K))


def apply_exposure(rgb: torch.Tensor, affine: torch.Tensor, image: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gain[image] * rgb + bias[image] for rgb [..., 3] and affine [K, 3, 2]; image: integer tensor of rgb's leading shape, or omitted
    when K = 1.  Plain torch, differentiable in both."""
    if affine.dim() != 3 or tuple(affine.shape[1:]) != (3, 2):
        raise ValueError(f"apply_exposure: affine must be [K, 3, 2], got {tuple(affine.shape)}")
    if rgb.shape[-1] != 3:
        raise ValueError(f"apply_exposure: rgb must be [..., 3], got {tuple(rgb.shape)}")
    if image is None:
        if affine.shape[0] != 1:
            raise ValueError("apply_exposure: K > 1 needs image (the image index of every colour)")
        a = affine[0]
    else:
        if tuple(image.shape) != tuple(rgb.shape[:-1]):
            raise ValueError(f"apply_exposure: image must have rgb's leading shape {tuple(rgb.shape[:-1])}, got {tuple(image.shape)}")
        a = affine[image.long()]
    return a[..., 0] * rgb + a[..., 1]


def align(pred_img: torch.Tensor, gt_img: torch.Tensor, mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The evaluation protocol for a model trained with ExposureDeltas: fit one affine colour map from a rendered image to its ground
    truth (over the pixels with mask > 0: [H, W] uint8 / bool / float, 255 or 1 = full weight) and apply it.
    pred_img, gt_img [H, W, 3] on the HIP device -> (aligned [H, W, 3] float32, affine [1, 3, 2]); metrics.psnr(aligned, gt, mask=mask)
    then measures the image, not the exposure gap."""
    if pred_img.dim() != 3 or pred_img.shape[-1] != 3 or pred_img.shape != gt_img.shape:
        raise ValueError(f"align: pred_img and gt_img must be [H, W, 3] of one shape, got {tuple(pred_img.shape)} and {tuple(gt_img.shape)}")
    w = None
    if mask is not None:
        if tuple(mask.shape) != tuple(pred_img.shape[:2]):
            raise ValueError(f"align: mask must be [H, W] = {tuple(pred_img.shape[:2])}, got {tuple(mask.shape)}")
        w = mask.to(pred_img.device)
        w = (w.float() / 255.0 if w.dtype == torch.uint8 else w.float()).reshape(-1).contiguous()
    p = pred_img.detach().float().reshape(-1, 3)
    affine = fit_exposure(p, gt_img.detach().to(p.device).float().reshape(-1, 3).contiguous(), weight=w)
    return apply_exposure(p, affine).reshape(pred_img.shape), affine
