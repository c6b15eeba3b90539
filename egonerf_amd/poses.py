"""Camera pose refinement on top of the ray gradients: per-image corrections of a RayBank's poses, optimised through
d loss / d (origin, direction) of the training render (csrc/ego_ray_grad.hip) - jointly with the field (BARF-style) or against a
frozen one (iNeRF-style localisation).  No reference counterpart: there the poses are fixed inputs.

Plain torch: the corrections are [B, 6] element-wise work next to a render of B x S samples."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

_SMALL = 1e-6   # theta^2 below which sin(theta) / theta and (1 - cos(theta)) / theta^2 come from their series (error < theta^6 / 5040)


def _rodrigues_coefficients(theta2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sin t / t, (1 - cos t) / t^2) as functions of t^2: differentiable at 0, where both branches of a naive form are 0 / 0."""
    small = theta2 < _SMALL
    t2 = torch.where(small, torch.ones_like(theta2), theta2)   # the closed form never sees 0: no NaN in its (unselected) gradient
    t = torch.sqrt(t2)
    a = torch.where(small, 1.0 - theta2 / 6.0 + theta2 * theta2 / 120.0, torch.sin(t) / t)
    b = torch.where(small, 0.5 - theta2 / 24.0 + theta2 * theta2 / 720.0, (1.0 - torch.cos(t)) / t2)
    return a, b


def rotate(w: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """exp([w]x) d for rows of axis-angle vectors w [B, 3] and vectors d [B, 3]: d + a (w x d) + b (w x (w x d)) (Rodrigues).  With
    w = 0 both cross products are zeros and the sum is d itself."""
    a, b = _rodrigues_coefficients((w * w).sum(-1, keepdim=True))
    wd = torch.cross(w, d, dim=-1)
    return d + a * wd + b * torch.cross(w, wd, dim=-1)


class PoseDeltas(torch.nn.Module):
    """One correction per image: `rot` [K, 3] (axis-angle, world frame) and `trans` [K, 3], zero-initialised.  A ray of image i becomes
    o' = o + trans[i], d' = exp([rot[i]]x) d, i.e. the camera-to-world pose [R | t] becomes [exp([rot]x) R | t + trans]."""

    def __init__(self, K: int, device=None):
        super().__init__()
        if int(K) < 1:
            raise ValueError("PoseDeltas: K must be >= 1")
        self.rot = torch.nn.Parameter(torch.zeros(int(K), 3, device=device))
        self.trans = torch.nn.Parameter(torch.zeros(int(K), 3, device=device))

    def apply(self, rays: torch.Tensor, img_idx: torch.Tensor) -> torch.Tensor:   # noqa: A003 (not nn.Module.apply(fn): named by what it does to rays)
        """rays [B, >=6] (origin, direction), img_idx [B] int64 -> corrected rays [B, 6].  At zero deltas the rays come back unchanged."""
        if callable(rays):   # nn.Module.apply(fn) keeps working (.to() / .cuda() do not go through it, but user code may)
            return super().apply(rays)
        w, t = self.rot.index_select(0, img_idx), self.trans.index_select(0, img_idx)
        return torch.cat([rays[:, :3] + t.to(rays.dtype), rotate(w.to(rays.dtype), rays[:, 3:6])], dim=-1)

    def poses(self, bank_poses: torch.Tensor) -> torch.Tensor:
        """The corrected camera-to-world poses [K, 3, 4] of bank poses [K, 3|4, 4]: what `apply` does to every ray of an image."""
        P = bank_poses[:, :3, :].to(self.rot.dtype)
        cols = [rotate(self.rot, P[:, :, c]) for c in range(3)]
        return torch.stack(cols + [P[:, :, 3] + self.trans], dim=-1)


def refine_poses(model, bank, steps: int, rays_per_step: int, lr_rot: float, lr_trans: float, train_model: bool = False, optimizer=None,
                 seed: int = 0, render_kwargs: Optional[dict] = None) -> Tuple[PoseDeltas, List[float]]:
    """Adam on per-image pose corrections of `bank` (a RayBank) against its own images -> (PoseDeltas, history).

    An eager loop of `steps` iterations: a batch of `rays_per_step` rays from DeviceSimpleSampler(bank, seed), corrected by the deltas,
    rendered with is_train semantics (`render_kwargs`: n_coarse, n_fine, resampling, ...; exp_sampling=True is implied - the ray
    gradient is defined there only), MSE against the bank's colours, backward, step.  train_model=False localises in a FROZEN field: the
    model's parameters ask for no gradient during the loop (restored afterwards), so the backward runs no scatter and no weight-gradient
    pass.  train_model=True also steps `optimizer` (the model's; required then, refused otherwise) in every iteration and refreshes the
    pooled tables when resampling, as a training iteration does.  Nothing in the loop synchronises with the host: the losses stay on the
    device and `history` (the MSE of every iteration) is read once at the end."""
    from .sampler import DeviceSimpleSampler
    if render_kwargs is None:
        raise ValueError("refine_poses needs render_kwargs (n_coarse, ...)")
    if int(steps) < 1 or int(rays_per_step) < 1:
        raise ValueError("refine_poses: steps and rays_per_step must be >= 1")
    if not (lr_rot > 0 and lr_trans > 0):
        raise ValueError("refine_poses: lr_rot and lr_trans must be > 0")
    if train_model and optimizer is None:
        raise ValueError("refine_poses(train_model=True) needs the model's optimizer")
    if optimizer is not None and not train_model:
        raise ValueError("refine_poses: an optimizer was given but train_model is False (a frozen model takes no step)")
    kw = dict(render_kwargs)
    if not kw.setdefault("exp_sampling", True):
        raise ValueError("refine_poses: ray gradients need exp_sampling=True")
    dev = bank.device
    source = DeviceSimpleSampler(bank, int(rays_per_step), seed)
    deltas = PoseDeltas(bank.K, device=dev)
    opt = torch.optim.Adam([dict(params=[deltas.rot], lr=float(lr_rot)), dict(params=[deltas.trans], lr=float(lr_trans))])
    frozen = []
    if not train_model:
        frozen = [p for p in model.parameters() if p.requires_grad]
        if model.envmap is not None and model.envmap.emission.requires_grad:
            frozen.append(model.envmap.emission)
        for p in frozen:
            p.requires_grad_(False)
    losses = []
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    try:
        for _ in range(int(steps)):
            idx, rays, target = source.next_batch()
            rays = deltas.apply(rays, bank.image_of(idx))
            jitter = torch.rand(rays.shape[0], int(kw["n_coarse"]), device=dev, generator=gen)
            u = torch.rand(rays.shape[0], int(kw.get("n_fine", 0)), device=dev, generator=gen) if kw.get("resampling") else None
            rgb = model(rays, is_train=True, jitter=jitter, u=u, **kw)[0]
            loss = torch.mean((rgb - target) ** 2)
            opt.zero_grad(set_to_none=True)
            if train_model:
                optimizer.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            if train_model:
                optimizer.step()
                if kw.get("resampling"):
                    model.update_coarse_sigma_grid()
            losses.append(loss.detach())
    finally:
        for p in frozen:
            p.requires_grad_(True)
    return deltas, torch.stack(losses).cpu().tolist()
