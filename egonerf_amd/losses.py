"""Loss terms of the reference's training step that sit next to the render (train.py:245-330), as autograd nodes over the
HIP kernels of csrc/ego_reg.hip.  Each node computes its value AND the gradient in the same pass over the tables and hands
the stored gradient (scaled by the incoming one) back in backward, so `total_loss.backward()` reads exactly like train.py.

    utils.py:155-171   TVLoss                       -> TVLoss
    utils.py:175-183   ray_entropy_loss             -> ray_entropy_loss
    EgoNeRF.py:189-228 vector_comp_diffs, density_L1, TV_loss_density / TV_loss_app  (methods of model.EgoNeRF call in here)
    (not in the reference) Mip-NeRF 360's distortion regulariser                    -> distortion_loss
    train.py:249-251   depth_loss (with the gradient the reference's lacks)          -> depth_loss, expected_depth
    train.py:261       the colour term, with weights, per-image exposure, robust kinds -> photometric_loss (csrc/ego_photo.hip)
    (not in the reference) 1 - mean SSIM over the windows of patch batches, with its gradient -> patch_ssim_loss (csrc/ego_patch_loss.hip)
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import _lib


def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: needs a HIP device tensor (the EgoNeRF path has no CPU fallback)")


def _channel_last_ptr(p: torch.Tensor, what: str) -> int:
    """Tables are (1, C, H, W) tensors whose memory is [H][W][C] (field_tables.carve_channel_last)."""
    if p.dim() != 4 or p.shape[0] != 1 or not p.permute(0, 2, 3, 1).is_contiguous() or p.dtype != torch.float32:
        raise RuntimeError(f"{what}: expected a float32 (1, C, H, W) table with channel-last memory")
    return p.data_ptr()


class _TableReg(torch.autograd.Function):
    """value = sum over tables of one regulariser term; kind in {"tv", "l1", "ortho"}; scales[i] multiplies table i's term."""

    @staticmethod
    @_lib.device_guard
    def forward(ctx, kind: str, scales: Sequence[float], *tables: torch.Tensor):
        lib, st = _lib.load(), _lib.stream_handle()
        dev = tables[0].device
        value = torch.zeros(1, dtype=torch.float64, device=dev)
        need = [t.requires_grad for t in tables]
        grads: List[torch.Tensor] = []
        for t, s, nd in zip(tables, scales, need):
            _require_cuda(t, kind)
            ptr = _channel_last_ptr(t, kind)
            _, C_, H, W = t.shape
            g = torch.zeros_like(t) if nd else None  # zeros_like keeps the channel-last strides
            gp = None if g is None else g.data_ptr()
            if kind == "tv":
                _lib.check(lib.ego_tv_plane(ptr, C_, H, W, float(s), value.data_ptr(), gp, st), "ego_tv_plane")
            elif kind == "l1":
                _lib.check(lib.ego_l1_table(ptr, t.numel(), float(s), value.data_ptr(), gp, st), "ego_l1_table")
            elif kind == "ortho":
                if W != 1:
                    raise RuntimeError("ortho: expected a (1, C, n, 1) line table")
                _lib.check(lib.ego_line_ortho(ptr, C_, H, float(s), value.data_ptr(), gp, st), "ego_line_ortho")
            else:
                raise ValueError(kind)
            grads.append(g)
        ctx.grads = grads
        return value.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, g_out):
        out = [None if g is None else g * g_out for g in ctx.grads]
        ctx.grads = None
        return (None, None, *out)


def table_regulariser(kind: str, tables: Sequence[torch.Tensor], scales: Sequence[float]) -> torch.Tensor:
    return _TableReg.apply(kind, list(scales), *tables)


class TVLoss(torch.nn.Module):
    """utils.py:155-171: TVLoss_weight * 2 * (sum dH^2 / count_h + sum dW^2 / count_w) / batch for one (1, C, H, W) plane."""

    def __init__(self, TVLoss_weight=1):
        super().__init__()
        self.TVLoss_weight = TVLoss_weight

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return table_regulariser("tv", [x], [float(self.TVLoss_weight)])


class _RayEntropy(torch.autograd.Function):
    @staticmethod
    @_lib.device_guard
    def forward(ctx, alpha: torch.Tensor):
        lib, st = _lib.load(), _lib.stream_handle()
        _require_cuda(alpha, "ray_entropy_loss")
        a = alpha.detach()
        if a.dtype != torch.float32 or a.dim() != 2 or not a.is_contiguous():
            a = a.float().contiguous()
        N, S = a.shape
        value = torch.zeros(1, dtype=torch.float64, device=a.device)
        g = torch.empty(N, S, device=a.device) if alpha.requires_grad else None
        _lib.check(lib.ego_ray_entropy(a.data_ptr(), N, S, S, value.data_ptr(), _lib.ptr(g), st), "ego_ray_entropy")
        ctx.g = g
        return value.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, g_out):
        g = ctx.g
        ctx.g = None
        return None if g is None else g * g_out


def ray_entropy_loss(alpha: torch.Tensor) -> torch.Tensor:
    """utils.py:175-183: mean over rays of the entropy (bits) of alpha / (sum alpha + 1e-10); alpha [N, S(+1)] as returned
    by EgoNeRF.forward (the envmap's trailing ones column included, like the reference)."""
    return _RayEntropy.apply(alpha)


_DIST_SPACES = {"linear": _lib.DIST_LINEAR, "log": _lib.DIST_LOG, "disparity": _lib.DIST_DISPARITY}


class _RayDistortion(torch.autograd.Function):
    @staticmethod
    @_lib.device_guard
    def forward(ctx, alpha: torch.Tensor, z: torch.Tensor, near: float, far: float, space: int):
        lib, st = _lib.load(), _lib.stream_handle()
        a = alpha.detach()
        if a.dtype != torch.float32 or not a.is_contiguous():
            a = a.float().contiguous()
        N, S = z.shape
        value = torch.zeros(1, dtype=torch.float64, device=a.device)
        g = torch.empty_like(a) if alpha.requires_grad else None
        _lib.check(lib.ego_ray_distortion(a.data_ptr(), a.shape[1], z.data_ptr(), N, S, near, far, space, value.data_ptr(), _lib.ptr(g), st),
                   "ego_ray_distortion")
        ctx.g = g
        return value.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, g_out):
        g = ctx.g
        ctx.g = None
        return (None if g is None else g * g_out), None, None, None, None


def distortion_loss(alpha: torch.Tensor, z: torch.Tensor, near_far: Sequence[float], space: str = "log") -> torch.Tensor:
    """Mip-NeRF 360's distortion regulariser in its point-sampled form (not in the reference): the mean over rays of
    sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i, with the render's weights w and the midpoints m / widths delta of the
    samples' intervals [z_i, z_{i+1}] mapped to [0, 1] by `space` ("linear", "log": equal widths for the exponential schedule,
    "disparity"); csrc/ego_reg.hip states the formula and its O(S) form.  alpha [N, S] or [N, S + 1] as returned by EgoNeRF.forward
    (an envmap's trailing ones column takes no part and gets a zero gradient); z [N, S] float32, the samples' distances of the SAME
    render: `model.last_train_z`.  z is a constant, alpha the only differentiable input."""
    if space not in _DIST_SPACES:
        raise ValueError(f"distortion_loss: space must be one of {sorted(_DIST_SPACES)}, not {space!r}")
    near, far = float(near_far[0]), float(near_far[1])
    if not far > near or (space != "linear" and not near > 0.0):
        raise ValueError(f"distortion_loss: needs near < far, and near > 0 for the {space!r} space (near_far = {near}, {far})")
    if alpha.dim() != 2 or z.dim() != 2 or alpha.shape[0] != z.shape[0] or alpha.shape[1] - z.shape[1] not in (0, 1) or z.shape[1] < 2:
        raise RuntimeError(f"distortion_loss: alpha {tuple(alpha.shape)} and z {tuple(z.shape)} must be [N, S] or [N, S + 1] and [N, S], S >= 2")
    if z.dtype != torch.float32 or z.device != alpha.device:
        raise RuntimeError("distortion_loss: z must be a float32 tensor on alpha's device")
    _require_cuda(alpha, "distortion_loss")
    return _RayDistortion.apply(alpha, z.detach().contiguous(), near, far, _DIST_SPACES[space])


_DEPTH_SPACES = {"metric": _lib.DIST_METRIC, "log": _lib.DIST_LOG, "disparity": _lib.DIST_DISPARITY}
_DEPTH_KINDS = {"l2": _lib.DEPTH_L2, "l1": _lib.DEPTH_L1}


def _depth_workspace(n_rays: int, device) -> torch.Tensor:
    """ego_ray_depth_loss's workspace (the valid-ray count and one float64 term per ray); the library states its size."""
    return torch.empty(_lib.load().ego_ray_depth_loss_workspace_bytes(n_rays) // 8, dtype=torch.float64, device=device)


class _RayDepth(torch.autograd.Function):
    @staticmethod
    @_lib.device_guard
    def forward(ctx, alpha: torch.Tensor, z: torch.Tensor, target: torch.Tensor, tail, near: float, far: float, space: int, kind: int):
        lib, st = _lib.load(), _lib.stream_handle()
        a = alpha.detach()
        if a.dtype != torch.float32 or not a.is_contiguous():
            a = a.float().contiguous()
        N, S = z.shape
        value = torch.zeros(1, dtype=torch.float64, device=a.device)
        g = torch.empty_like(a) if alpha.requires_grad else None
        ws = _depth_workspace(N, a.device)
        _lib.check(lib.ego_ray_depth_loss(a.data_ptr(), a.shape[1], z.data_ptr(), target.data_ptr(), _lib.ptr(tail), N, S, near, far, space, kind,
                                          ws.data_ptr(), value.data_ptr(), _lib.ptr(g), None, st), "ego_ray_depth_loss")
        ctx.g = g
        return value.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, g_out):
        g = ctx.g
        ctx.g = None
        return (None if g is None else g * g_out), None, None, None, None, None, None, None


def _depth_args(what: str, alpha: torch.Tensor, z: torch.Tensor, per_ray: dict):
    """The shape, dtype and device checks depth_loss and expected_depth share; -> the per-ray vectors, detached and contiguous."""
    if alpha.dim() != 2 or z.dim() != 2 or alpha.shape[0] != z.shape[0] or alpha.shape[1] - z.shape[1] not in (0, 1) or z.shape[1] < 2:
        raise RuntimeError(f"{what}: alpha {tuple(alpha.shape)} and z {tuple(z.shape)} must be [N, S] or [N, S + 1] and [N, S], S >= 2")
    if z.dtype != torch.float32 or z.device != alpha.device:
        raise RuntimeError(f"{what}: z must be a float32 tensor on alpha's device")
    out = []
    for name, t in per_ray.items():
        if t is None:
            out.append(None)
            continue
        if t.dim() != 1 or t.shape[0] != z.shape[0] or t.dtype != torch.float32 or t.device != alpha.device:
            raise RuntimeError(f"{what}: {name} must be a float32 [N] tensor on alpha's device, N = {z.shape[0]}")
        out.append(t.detach().contiguous())
    _require_cuda(alpha, what)
    return out


def depth_loss(alpha: torch.Tensor, z: torch.Tensor, target: torch.Tensor, tail: Optional[torch.Tensor] = None, space: str = "metric",
               near_far: Optional[Sequence[float]] = None, kind: str = "l2") -> torch.Tensor:
    """The depth term of train.py:249-251 / :275-283 with its gradient (the reference computes depth_map under no_grad, so its own term
    has none): the mean over the VALID rays of (D - s(target))^2 ("l2") or |D - s(target)| ("l1"), D = sum_i w_i s(z_i) +
    (1 - sum_i w_i) s(tail) with the render's weights w; csrc/ego_reg.hip states the O(S) form.  A ray is valid iff its target is finite
    and > 0 (0 = no target, as in the reference; NaN, inf and negative targets drop out too); with no valid ray the loss and the gradient
    are 0.  `space`: "metric" (s = identity, the reference's term), "log" or "disparity" (distortion_loss's normalised maps; they need
    `near_far`).  alpha [N, S] or [N, S + 1] as returned by EgoNeRF.forward, z [N, S] = `model.last_train_z` of the SAME render, target
    [N] float32 in units of distance along the normalised ray.  `tail=None` puts the mass a ray does not absorb at 0;
    `tail=rays[:, 5]` reproduces the render's own depth_map, which adds (1 - acc) * rays[..., -1].  alpha is the only differentiable
    input; the render's `depth` output is not involved and stays non-differentiable."""
    if space not in _DEPTH_SPACES:
        raise ValueError(f"depth_loss: space must be one of {sorted(_DEPTH_SPACES)}, not {space!r}")
    if kind not in _DEPTH_KINDS:
        raise ValueError(f"depth_loss: kind must be one of {sorted(_DEPTH_KINDS)}, not {kind!r}")
    near, far = 0.0, 0.0
    if space != "metric":
        if near_far is None:
            raise ValueError(f"depth_loss: the {space!r} space needs near_far")
        near, far = float(near_far[0]), float(near_far[1])
        if not (0.0 < near < far < float("inf")):
            raise ValueError(f"depth_loss: the {space!r} space needs finite 0 < near < far (near_far = {near}, {far})")
    if target is None:
        raise RuntimeError("depth_loss: target must be a float32 [N] tensor on alpha's device")
    target, tail = _depth_args("depth_loss", alpha, z, dict(target=target, tail=tail))
    return _RayDepth.apply(alpha, z.detach().contiguous(), target, tail, near, far, _DEPTH_SPACES[space], _DEPTH_KINDS[kind])


@_lib.device_guard
def _expected_depth(a, z, tail):
    pred = torch.empty(z.shape[0], device=a.device)
    _lib.check(_lib.load().ego_ray_depth_loss(a.data_ptr(), a.shape[1], z.data_ptr(), None, _lib.ptr(tail), z.shape[0], z.shape[1], 0.0, 0.0,
                                              _lib.DIST_METRIC, _lib.DEPTH_L2, None, None, None, pred.data_ptr(), _lib.stream_handle()),
               "ego_ray_depth_loss")
    return pred


def expected_depth(alpha: torch.Tensor, z: torch.Tensor, tail: Optional[torch.Tensor] = None) -> torch.Tensor:
    """D of depth_loss in the metric space, [N] float32, no target needed and no gradient: sum_i w_i z_i + (1 - sum_i w_i) tail."""
    (tail,) = _depth_args("expected_depth", alpha, z, dict(tail=tail))
    a = alpha.detach()
    if a.dtype != torch.float32 or not a.is_contiguous():
        a = a.float().contiguous()
    return _expected_depth(a, z.detach().contiguous(), tail)


_PHOTO_KINDS = {"l2": _lib.PHOTO_L2, "l1": _lib.PHOTO_L1, "huber": _lib.PHOTO_HUBER, "charbonnier": _lib.PHOTO_CHARBONNIER}
_PHOTO_PARAM = {"huber": 0.1, "charbonnier": 1e-3}   # delta, epsilon: in units of colour, [0, 1]


class _Photo(torch.autograd.Function):
    @staticmethod
    @_lib.device_guard
    def forward(ctx, rgb: torch.Tensor, affine, target: torch.Tensor, weight, image, kind: int, param: float):
        lib, st = _lib.load(), _lib.stream_handle()
        c = rgb.detach()
        if c.dtype != torch.float32 or not c.is_contiguous():
            c = c.float().contiguous()
        a = None if affine is None else affine.detach()
        if a is not None and (a.dtype != torch.float32 or not a.is_contiguous()):
            a = a.float().contiguous()
        N, K = c.shape[0], (0 if a is None else a.shape[0])
        value = torch.zeros(1, dtype=torch.float64, device=c.device)
        g_rgb = torch.empty_like(c) if rgb.requires_grad else None
        g_aff = torch.empty_like(a) if a is not None and affine.requires_grad else None
        if image is not None and a is None:
            K = 2 ** 31 - 1   # no table to stay inside: only negative indices are invalid
        ws = torch.empty(lib.ego_photo_loss_workspace_bytes(N, K if g_aff is not None else 0) // 8, dtype=torch.float64, device=c.device)
        _lib.check(lib.ego_photo_loss(c.data_ptr(), target.data_ptr(), _lib.ptr(weight), _lib.ptr(image), _lib.ptr(a), N, K, kind, param,
                                      ws.data_ptr(), value.data_ptr(), _lib.ptr(g_rgb), _lib.ptr(g_aff), st), "ego_photo_loss")
        if N == 0:   # the library's no-op writes nothing
            g_aff = None if g_aff is None else torch.zeros_like(g_aff)
        ctx.g = (g_rgb, g_aff)
        return value.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, g_out):
        g_rgb, g_aff = ctx.g
        ctx.g = None
        return (None if g_rgb is None else g_rgb * g_out), (None if g_aff is None else g_aff * g_out), None, None, None, None, None


def _photo_args(what: str, rgb: torch.Tensor, target: torch.Tensor, weight, image, affine=None):
    """The shape, dtype and device checks photometric_loss and exposure.fit_exposure share; -> (target, weight, image) detached,
    contiguous, image as int32."""
    if not torch.is_tensor(rgb) or rgb.dim() != 2 or rgb.shape[1] != 3 or not rgb.dtype.is_floating_point:
        raise RuntimeError(f"{what}: rgb must be a floating-point [N, 3] tensor")
    N = rgb.shape[0]
    if not torch.is_tensor(target) or tuple(target.shape) != (N, 3) or target.dtype != torch.float32 or target.device != rgb.device:
        raise RuntimeError(f"{what}: target must be a float32 [N, 3] tensor on rgb's device, N = {N}")
    if weight is not None and (not torch.is_tensor(weight) or tuple(weight.shape) != (N,) or weight.dtype != torch.float32
                               or weight.device != rgb.device):
        raise RuntimeError(f"{what}: weight must be a float32 [N] tensor on rgb's device, N = {N}")
    if image is not None:
        if not torch.is_tensor(image) or tuple(image.shape) != (N,) or image.dtype not in (torch.int32, torch.int64) or image.device != rgb.device:
            raise RuntimeError(f"{what}: image must be an int32 or int64 [N] tensor on rgb's device, N = {N}")
        image = image.detach().to(torch.int32).contiguous()
    if affine is not None:
        if not torch.is_tensor(affine) or affine.dim() != 3 or tuple(affine.shape[1:]) != (3, 2) or affine.shape[0] < 1 \
                or affine.dtype != torch.float32 or affine.device != rgb.device:
            raise RuntimeError(f"{what}: affine must be a float32 [K, 3, 2] tensor (gain, bias) on rgb's device, K >= 1")
        if image is None:
            raise ValueError(f"{what}: affine needs image (the image index of every ray)")
    _require_cuda(rgb, what)
    return target.detach().contiguous(), (None if weight is None else weight.detach().contiguous()), image


def photometric_loss(rgb: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, image: Optional[torch.Tensor] = None,
                     affine: Optional[torch.Tensor] = None, kind: str = "l2", param: Optional[float] = None) -> torch.Tensor:
    """The colour term of train.py:261 for real captures (csrc/ego_photo.hip states the formula): (1 / 3W) sum_valid w_n sum_c rho(r_nc),
    r = gain[image[n]] * rgb + bias[image[n]] - target, W = the sum of the valid rays' weights.  `kind`: "l2" (r^2), "l1" (|r|), "huber"
    (r^2 / 2 up to |r| = param, linear beyond; param defaults to 0.1) or "charbonnier" (sqrt(r^2 + param^2) - param; 1e-3).  A ray is
    valid iff its weight is finite and > 0, its target is finite and its image index lies inside `affine`; invalid rays add nothing and
    get the gradient 0, and with no valid ray the loss and its gradients are 0.  With the defaults it is `torch.mean((rgb - target) ** 2)`
    evaluated in float64.  rgb [N, 3]; target [N, 3] float32; weight [N] float32 (RayBank.gather_mask's output: 0 = ignore); image [N]
    int32 / int64 (RayBank.image_of); affine [K, 3, 2] float32 (ExposureDeltas.affine()), which needs `image`.  Differentiable inputs: rgb
    and affine.  Deterministic: the same inputs give the same bits."""
    if kind not in _PHOTO_KINDS:
        raise ValueError(f"photometric_loss: kind must be one of {sorted(_PHOTO_KINDS)}, not {kind!r}")
    if param is None:
        param = _PHOTO_PARAM.get(kind, 0.0)
    elif kind in _PHOTO_PARAM and not (0.0 < float(param) < float("inf")):
        raise ValueError(f"photometric_loss: {kind!r} needs a finite param > 0, not {param!r}")
    target, weight, image = _photo_args("photometric_loss", rgb, target, weight, image, affine)
    return _Photo.apply(rgb, affine, target, weight, image, _PHOTO_KINDS[kind], float(param))


class _PatchSsim(torch.autograd.Function):
    @staticmethod
    @_lib.device_guard
    def forward(ctx, rgb: torch.Tensor, target: torch.Tensor, weight, P: int, ph: int, pw: int, fs: int, sigma: float, max_val: float, k1: float,
                k2: float):
        lib, st = _lib.load(), _lib.stream_handle()
        c = rgb.detach().contiguous()   # float32 [B, 3]: patch_ssim_loss has checked
        value = torch.zeros(1, dtype=torch.float64, device=c.device)
        n = P * ph * pw
        g = None
        if rgb.requires_grad:
            g = torch.empty_like(c)
            g[n:].zero_()   # the rows behind the patches take no part: exactly 0
        ws = torch.empty(max(lib.ego_patch_ssim_workspace_bytes(P, ph, pw) // 8, 1), dtype=torch.float64, device=c.device)
        _lib.check(lib.ego_patch_ssim(c.data_ptr(), target.data_ptr(), _lib.ptr(weight), P, ph, pw, fs, sigma, max_val, k1, k2, ws.data_ptr(),
                                      value.data_ptr(), _lib.ptr(g), st), "ego_patch_ssim")
        ctx.g = g
        return value.reshape(())

    @staticmethod
    def backward(ctx, g_out):
        g = ctx.g
        ctx.g = None
        return (None if g is None else (g * g_out).to(g.dtype)), None, None, None, None, None, None, None, None, None, None


def patch_ssim_loss(rgb: torch.Tensor, target: torch.Tensor, patch: Sequence[int], n_patches: Optional[int] = None,
                    weight: Optional[torch.Tensor] = None, filter_size: int = 7, filter_sigma: float = 1.5, max_val: float = 1.0,
                    k1: float = 0.01, k2: float = 0.03) -> torch.Tensor:
    """The structural term on patch batches (not in the reference; csrc/ego_patch_loss.hip states the formulas): 1 - the mean SSIM over
    the 'valid' Gaussian windows (metrics.rgb_ssim's taps, without its rounding guards) of `n_patches` patches of patch = (ph, pw) pixels,
    a float64 device scalar.  rgb, target [B, 3]: the first n_patches * ph * pw rows are the patches, row p ph pw + a pw + b = pixel (a, b)
    of patch p (sampler.DevicePatchSampler's layout, data.patch_indices'); n_patches=None takes all of B, which must then divide evenly.
    Later rows are ignored and get exactly zero gradient.  weight [B] float32 (RayBank.gather_mask's output) is a gate: a window is valid
    iff every pixel under it has a finite weight > 0 and a finite target; invalid windows add nothing, pixels under no valid window get
    the gradient 0, and with no valid window the loss and its gradient are 0.  Envelope: 1 <= filter_size <= 15, filter_size <= ph, pw
    <= 32.  rgb (float32) is the differentiable input; its gradient is float32.  As with the other terms here the gradient is computed in the
    forward call and handed out once: a second backward through the same node (retain_graph) gets none.  Deterministic: the same inputs
    give the same bits."""
    what = "patch_ssim_loss"
    if not (isinstance(patch, (tuple, list)) and len(patch) == 2):
        raise ValueError(f"{what}: patch must be (ph, pw), not {patch!r}")
    ph, pw, fs = int(patch[0]), int(patch[1]), int(filter_size)
    if not 1 <= fs <= 15:
        raise ValueError(f"{what}: filter_size must be 1..15, not {filter_size!r}")
    if not (fs <= ph <= 32 and fs <= pw <= 32):
        raise ValueError(f"{what}: a patch must cover the filter and be at most 32 x 32 (filter_size {fs}, patch {ph} x {pw})")
    if not (0.0 < float(filter_sigma) < float("inf")):
        raise ValueError(f"{what}: filter_sigma must be finite and > 0, not {filter_sigma!r}")
    if not torch.is_tensor(rgb) or rgb.dim() != 2 or rgb.shape[1] != 3 or rgb.dtype != torch.float32:
        raise RuntimeError(f"{what}: rgb must be a float32 [B, 3] tensor")
    B = rgb.shape[0]
    if not torch.is_tensor(target) or tuple(target.shape) != (B, 3) or target.dtype != torch.float32 or target.device != rgb.device:
        raise RuntimeError(f"{what}: target must be a float32 [B, 3] tensor on rgb's device, B = {B}")
    if weight is not None and (not torch.is_tensor(weight) or tuple(weight.shape) != (B,) or weight.dtype != torch.float32
                               or weight.device != rgb.device):
        raise RuntimeError(f"{what}: weight must be a float32 [B] tensor on rgb's device, B = {B}")
    if n_patches is None:
        if B % (ph * pw) != 0:
            raise ValueError(f"{what}: {B} rows are not a whole number of {ph} x {pw} patches; pass n_patches")
        n_patches = B // (ph * pw)
    n_patches = int(n_patches)
    if n_patches < 0 or n_patches * ph * pw > B:
        raise ValueError(f"{what}: n_patches = {n_patches} patches of {ph} x {pw} do not fit {B} rows")
    _require_cuda(rgb, what)
    return _PatchSsim.apply(rgb, target.detach().contiguous(), None if weight is None else weight.detach().contiguous(), n_patches, ph, pw, fs,
                            float(filter_sigma), float(max_val), float(k1), float(k2))
