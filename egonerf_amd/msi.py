"""Multi-sphere images: a trained field baked once into L concentric RGBA shells around the capture centre, and played back from them.

`bake_msi` integrates the field along the rays of an equirectangular camera at the centre - the unchanged march and shade kernels, chunk by
chunk - and folds every ray's samples into per-layer premultiplied RGBA (csrc/ego_msi.hip: ego_msi_layers).  A `MultiSphereImage` renders
rays of ANY nearby origin from the shells alone (ego_msi_render: L sphere intersections, L bilinear taps and an "over" per ray - no tables,
no MLP) and is shaped like a model, so `FrameRenderer(msi, H, W, ...)` and `evaluation_path` take it as it is: stereo, supersampling, byte
frames and graphs included.  Playback is differentiable in float32 texels (ego_msi_render_backward), and `refine_msi` optimises a baked
image against a teacher's renders from inside a headbox.  Not part of the reference; formulas, layout and limits: DESIGN.md 3.3.
"""
from __future__ import annotations

from typing import Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .camera import camera_rays

TEXEL_TYPES = {torch.float32: _lib.MSI_F32, torch.float16: _lib.MSI_F16}


def layer_bounds(z_sched, L: int, runs: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Splits the S ascending sample distances `z_sched` into L contiguous runs -> (bounds [L + 1], radii [L]), float32, strictly
    increasing.  Layer k owns the samples with bounds[k] <= z < bounds[k + 1]: bounds[0] = z[0], an inner bound is the midpoint between
    the last sample of a run and the first of the next, the last bound lies half an interval above z[S - 1].  radii[k] is the geometric
    mean of the run's first and last z.  runs: the L run lengths (positive, summing to S); default: equal counts, the first S mod L
    runs one longer."""
    z = np.asarray(z_sched.detach().cpu() if isinstance(z_sched, torch.Tensor) else z_sched, dtype=np.float32).reshape(-1)
    S, L = z.size, int(L)
    if L < 1 or S < 2 or L > S:
        raise ValueError(f"layer_bounds: need 1 <= L <= S and S >= 2, got L = {L}, S = {S}")
    if not (np.all(np.isfinite(z)) and np.all(np.diff(z) > 0)):
        raise ValueError("layer_bounds: the sample distances must be finite and strictly increasing in float32")
    if runs is None:
        runs = [S // L + (1 if k < S % L else 0) for k in range(L)]
    runs = [int(r) for r in runs]
    if len(runs) != L or min(runs) < 1 or sum(runs) != S:
        raise ValueError(f"layer_bounds: `runs` must be {L} positive lengths summing to {S}, got {runs}")
    start = np.concatenate([[0], np.cumsum(runs)]).astype(np.int64)   # run k = samples [start[k], start[k + 1])
    z64 = z.astype(np.float64)
    bounds = np.empty(L + 1, np.float64)
    bounds[0] = z64[0]
    bounds[1:L] = 0.5 * (z64[start[1:L] - 1] + z64[start[1:L]])
    bounds[L] = z64[-1] + 0.5 * (z64[-1] - z64[-2])
    bounds = bounds.astype(np.float32)
    if not bounds[L] > z[-1]:
        bounds[L] = np.nextafter(z[-1], np.float32(np.inf))
    radii = np.sqrt(z64[start[:-1]] * z64[start[1:] - 1]).astype(np.float32)
    owner = np.searchsorted(bounds, z, side="right") - 1   # the k with bounds[k] <= z < bounds[k + 1], in float32 as the kernel compares
    if not (np.all(np.diff(bounds) > 0) and np.array_equal(owner, np.repeat(np.arange(L), runs))):
        raise ValueError("layer_bounds: neighbouring samples are too close for a float32 bound between them")
    if not (radii[0] > 0 and np.all(np.diff(radii) > 0)):
        raise ValueError("layer_bounds: the radii must be positive and strictly increasing (a first run that is the single sample z = 0?)")
    return bounds, radii


def _check_rays(rays, device, what: str) -> None:
    if not isinstance(rays, torch.Tensor) or not rays.is_cuda:
        raise ValueError(f"{what}: rays must be a device tensor (the HIP path has no CPU fallback)")
    if rays.device != device:
        raise ValueError(f"{what}: rays live on {rays.device}, the multi-sphere image on {device}")
    if rays.dtype != torch.float32:
        raise ValueError(f"{what}: rays must be float32, got {rays.dtype}")
    if rays.dim() != 2 or rays.shape[1] != 6:
        raise IndexError(f"{what}: rays must be [N, 6] (origin, direction), got {tuple(rays.shape)}")
    if not rays.is_contiguous():
        raise ValueError(f"{what}: rays must be contiguous")


class _RenderFunction(torch.autograd.Function):
    """Playback with a backward: the forward is the plain ego_msi_render call, the backward ego_msi_render_backward into zeroed float32
    gradients of the texels' layout.  depth is not differentiable; rays get no gradient."""

    @staticmethod
    def forward(ctx, msi, rays, layers, background):
        rgb, depth = msi._render(rays, layers, background)
        ctx.msi = msi
        ctx.save_for_backward(rays, layers, *(() if background is None else (background,)))
        ctx.mark_non_differentiable(depth)
        return rgb, depth

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb, _g_depth):
        msi, (rays, layers, *rest) = ctx.msi, ctx.saved_tensors
        background = rest[0] if rest else None
        g_rgb = g_rgb.to(torch.float32).contiguous()
        g_layers = torch.zeros_like(layers) if ctx.needs_input_grad[2] else None   # 1 GiB at L = 32, 1024 x 2048: only when asked for
        g_background = torch.zeros_like(background) if background is not None and ctx.needs_input_grad[3] else None
        msi._render_backward(rays, layers, background, g_rgb, g_layers, g_background)
        return None, None, g_layers, g_background


class MultiSphereImage:
    """L concentric shells of premultiplied RGBA around `center`, each an Hm x Wm equirectangular image.

    layers [L, Hm, Wm, 4] float16 or float32, contiguous (on a HIP device to render; an image in host memory can be held, converted, saved
    and loaded, and refuses to render); background [Hm, Wm, 4] of the same type or None: the shell at infinity,
    looked up by the ray's direction, its alpha taken as 1; radii [L] and bounds [L + 1] float32, ascending (bounds: the sample distances
    each layer integrated, kept for the record); center: 3 numbers; near_far: the depth range of the baked model (what `FrameRenderer`
    scales its depth image with).

    Called like a model - `msi(rays, need_alpha=False, ...)` -> (rgb [N, 3], depth [N], None, None, None) - so FrameRenderer and
    evaluation_path take it in a model's place; every other keyword of EgoNeRF.forward is accepted and ignored.  rays: [N, 6] float32,
    contiguous; the direction need not be of unit length (the pinhole cameras' is not): the kernel normalises it and reports depth in the
    given ray's parameter, as a model does.  A layer whose
    radius is not larger than the eye's distance from the centre is skipped; colours are not clamped (`finish_frame` does).

    With grad enabled and float32 `layers` (or `background`) that require grad, `render` records a graph: `rgb.backward(...)` fills
    `layers.grad` (and `background.grad`) through ego_msi_render_backward; depth stays non-differentiable.  Half texels that require
    grad are refused."""

    def __init__(self, layers: torch.Tensor, radii, bounds, center, near_far, background: Optional[torch.Tensor] = None):
        if not isinstance(layers, torch.Tensor):
            raise ValueError("MultiSphereImage: layers must be a torch tensor")
        if layers.dtype not in TEXEL_TYPES:
            raise ValueError(f"MultiSphereImage: layers must be float16 or float32, got {layers.dtype}")
        if layers.dim() != 4 or layers.shape[3] != 4 or min(layers.shape) < 1:
            raise IndexError(f"MultiSphereImage: layers must be [L, Hm, Wm, 4], got {tuple(layers.shape)}")
        if not layers.is_contiguous():
            raise ValueError("MultiSphereImage: layers must be contiguous")
        L, Hm, Wm = (int(v) for v in layers.shape[:3])
        if background is not None:
            if not isinstance(background, torch.Tensor) or background.device != layers.device or background.dtype != layers.dtype:
                raise ValueError("MultiSphereImage: background must be a tensor of the layers' device and dtype")
            if tuple(background.shape) != (Hm, Wm, 4):
                raise IndexError(f"MultiSphereImage: background must be [{Hm}, {Wm}, 4], got {tuple(background.shape)}")
            if not background.is_contiguous():
                raise ValueError("MultiSphereImage: background must be contiguous")
        r = np.asarray(radii.detach().cpu() if isinstance(radii, torch.Tensor) else radii, dtype=np.float32).reshape(-1)
        b = np.asarray(bounds.detach().cpu() if isinstance(bounds, torch.Tensor) else bounds, dtype=np.float32).reshape(-1)
        if r.size != L or b.size != L + 1:
            raise IndexError(f"MultiSphereImage: {L} layers need radii [{L}] and bounds [{L + 1}], got [{r.size}] and [{b.size}]")
        if not (np.all(np.isfinite(r)) and r[0] > 0 and np.all(np.diff(r) > 0)):
            raise ValueError("MultiSphereImage: radii must be finite, positive and strictly increasing")
        if not (np.all(np.isfinite(b)) and np.all(np.diff(b) > 0)):
            raise ValueError("MultiSphereImage: bounds must be finite and strictly increasing")
        c = np.asarray(center.detach().cpu() if isinstance(center, torch.Tensor) else center, dtype=np.float32).reshape(-1)
        if c.size != 3 or not np.all(np.isfinite(c)):
            raise ValueError("MultiSphereImage: center must be 3 finite numbers")
        nf = [float(v) for v in np.asarray(near_far, dtype=np.float64).reshape(-1)]
        if len(nf) != 2:
            raise ValueError("MultiSphereImage: near_far must be (near, far)")
        self.layers, self.background, self.device = layers, background, layers.device
        self.radii = torch.from_numpy(r.copy()).to(self.device)
        self.bounds = torch.from_numpy(b.copy()).to(self.device)
        self.center, self.near_far = c.copy(), nf
        self.L, self.Hm, self.Wm = L, Hm, Wm

    # ---- what FrameRenderer asks of a model -----------------------------------------------------------------------------------------
    def parameters(self) -> Iterator[torch.Tensor]:
        yield self.layers
        if self.background is not None:
            yield self.background

    def __call__(self, rays: torch.Tensor, need_alpha: bool = False, **ignored):
        rgb, depth = self.render(rays)
        return rgb, depth, None, None, None

    @_lib.device_guard
    def render(self, rays: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(rgb [N, 3], depth [N]) float32 of `rays` [N, 6], on the current stream (not synchronised)."""
        wants_grad = torch.is_grad_enabled() and (self.layers.requires_grad or (self.background is not None and self.background.requires_grad))
        if wants_grad and self.layers.dtype != torch.float32:
            raise ValueError("MultiSphereImage.render: half texels have no gradient; train a float32 image (msi.float()) and convert back")
        if not self.layers.is_cuda:
            raise ValueError("MultiSphereImage.render: the image must live on a HIP device (the HIP path has no CPU fallback)")
        _check_rays(rays, self.device, "MultiSphereImage.render")
        if wants_grad:
            return _RenderFunction.apply(self, rays, self.layers, self.background)
        return self._render(rays, self.layers, self.background)

    def _render(self, rays: torch.Tensor, layers: torch.Tensor, background: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        N = rays.shape[0]
        rgb = torch.empty(N, 3, device=self.device, dtype=torch.float32)
        depth = torch.empty(N, device=self.device, dtype=torch.float32)
        c = self.center
        _lib.check(_lib.load().ego_msi_render(rays.data_ptr(), N, float(c[0]), float(c[1]), float(c[2]), self.radii.data_ptr(), self.L, self.Hm,
                                              self.Wm, TEXEL_TYPES[layers.dtype], layers.data_ptr(), _lib.ptr(background),
                                              rgb.data_ptr(), depth.data_ptr(), _lib.stream_handle()), "ego_msi_render")
        return rgb, depth

    def _render_backward(self, rays, layers, background, g_rgb, g_layers, g_background) -> None:
        """g_rgb [N, 3] -> added into g_layers and g_background (either may be None, not both): float32, contiguous, the texels' shapes."""
        N, lib, c = rays.shape[0], _lib.load(), self.center
        ws = torch.empty(max(int(lib.ego_msi_render_backward_workspace_bytes(N, self.L)), 4) // 4, device=self.device, dtype=torch.float32)
        _lib.check(lib.ego_msi_render_backward(rays.data_ptr(), N, float(c[0]), float(c[1]), float(c[2]), self.radii.data_ptr(), self.L, self.Hm,
                                               self.Wm, TEXEL_TYPES[layers.dtype], layers.data_ptr(), _lib.ptr(background), g_rgb.data_ptr(),
                                               _lib.ptr(g_layers), _lib.ptr(g_background), ws.data_ptr(), ws.numel() * 4,
                                               _lib.stream_handle()), "ego_msi_render_backward")

    # ---- texel type -----------------------------------------------------------------------------------------------------------------
    def _as(self, dtype) -> "MultiSphereImage":
        if self.layers.dtype == dtype:
            return self
        bg = None if self.background is None else self.background.to(dtype)
        return MultiSphereImage(self.layers.to(dtype), self.radii, self.bounds, self.center, self.near_far, bg)

    def half(self) -> "MultiSphereImage":
        """The same image with half texels (rounded to nearest; itself if it has them)."""
        return self._as(torch.float16)

    def float(self) -> "MultiSphereImage":
        """The same image with float32 texels (exact; itself if it has them)."""
        return self._as(torch.float32)

    # ---- files ----------------------------------------------------------------------------------------------------------------------
    def save(self, path) -> None:
        """One .npz: the arrays as they are (`layers`, `radii`, `bounds`, `center`, `near_far`, and `background` if there is one); no
        pickled objects.  `load` returns the same bits."""
        arrays = dict(layers=self.layers.cpu().numpy(), radii=self.radii.cpu().numpy(), bounds=self.bounds.cpu().numpy(),
                      center=self.center, near_far=np.asarray(self.near_far, np.float64))
        if self.background is not None:
            arrays["background"] = self.background.cpu().numpy()
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path, device="cuda") -> "MultiSphereImage":
        with np.load(path, allow_pickle=False) as f:
            a = {k: f[k] for k in f.files}
        dev = torch.device(device)
        bg = torch.from_numpy(a["background"]).to(dev) if "background" in a else None
        return cls(torch.from_numpy(a["layers"]).to(dev), a["radii"], a["bounds"], a["center"], a["near_far"], bg)


@_lib.device_guard
@torch.no_grad()
def bake_msi(model, Hm: int, Wm: int, L: int, n_samples: int, center=None, dtype=torch.float16, chunk: int = 16384,
             layers: Optional[Sequence[int]] = None) -> MultiSphereImage:
    """Integrates `model` into an L-layer Hm x Wm multi-sphere image around `center` (default: the model's coordinate centre).

    Per chunk of `chunk` texels: the rays of an equirectangular camera with an identity pose at the centre (`camera_rays`), one
    ego_march_density with the model's own `n_samples` eval schedule (exponential sampling; no jitter, no resampling), ego_shade for every
    sample's colour, ego_msi_layers straight into the image.  The layers split the schedule into runs of samples (`layer_bounds`; `layers`:
    explicit run lengths).  With an envmap the background is ego_envmap_radiance of the same directions.  The bake holds the exact
    integral: the render-time approximations (`use_weight_thres`, `early_termination_eps`) do not enter it.  dtype: torch.float16 or
    torch.float32 texels.  Models that shade through the any-shape compatibility kernels raise NotImplementedError."""
    if dtype not in TEXEL_TYPES:
        raise ValueError(f"bake_msi: dtype must be torch.float16 or torch.float32, got {dtype}")
    Hm, Wm, L, S, chunk = int(Hm), int(Wm), int(L), int(n_samples), int(chunk)
    if Hm < 1 or Wm < 1 or chunk < 1:
        raise ValueError("bake_msi: Hm, Wm and chunk must be positive")
    if S < 2 or not 1 <= L <= S:
        raise ValueError(f"bake_msi: need n_samples >= 2 and 1 <= L <= n_samples, got L = {L}, n_samples = {S}")
    p = next(model.parameters())
    if not p.is_cuda:
        raise ValueError("bake_msi: the model must live on a HIP device")
    if not model.is_tuned_shape:
        raise NotImplementedError("bake_msi: this model renders through the any-shape compatibility kernels (EgoNeRF.is_tuned_shape is False: "
                                  "another appearance head or density component count); baking them is out of scope")
    model.coordinates._require_supported()
    dev = p.device
    c = np.asarray(model.coordinates.center.tolist() if center is None else
                   (center.detach().cpu() if isinstance(center, torch.Tensor) else center), dtype=np.float32).reshape(-1)
    if c.size != 3 or not np.all(np.isfinite(c)):
        raise ValueError("bake_msi: center must be 3 finite numbers")
    near = float(model.near_far[0])
    sched = model._sched(S, dev)
    z_sched = (np.float32(near) + sched.cpu().numpy().astype(np.float32)).astype(np.float32)   # the march's z = near + r_sched[s]
    bounds, radii = layer_bounds(z_sched, L, layers)
    lib, st, sc = _lib.load(), _lib.stream_handle(), model.scene()
    texels = Hm * Wm
    n = min(chunk, texels)
    if n * S >= 1 << 31:
        raise ValueError("bake_msi: chunk * n_samples must stay below 2^31")
    image = torch.empty(L, Hm, Wm, 4, device=dev, dtype=dtype)
    has_env = model.envmap is not None
    background = torch.empty(Hm, Wm, 4, device=dev, dtype=dtype) if has_env else None
    f = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
    rays, z, alpha, crd, rgb = f(n, 6), f(n, S), f(n, S), f(n, S, 4), f(n, S, 3)
    dirs, env = (f(n, 3), f(n, 3)) if has_env else (None, None)
    pose = np.concatenate([np.eye(3, dtype=np.float32), c.reshape(3, 1)], axis=1)
    pose_dev, bounds_dev = torch.from_numpy(pose).to(dev), torch.from_numpy(bounds).to(dev)
    for first in range(0, texels, n):
        count = min(n, texels - first)
        camera_rays(Hm, Wm, pose_dev, "erp", normalize=True, first=first, count=count, out=rays)
        _lib.check(lib.ego_march_density(sc, rays.data_ptr(), count, S, None, sched.data_ptr(), None, near, 0, z.data_ptr(), alpha.data_ptr(), S,
                                         None, None, crd.data_ptr(), None, None, st), "ego_march_density")
        _lib.check(lib.ego_shade(sc, rays.data_ptr(), z.data_ptr(), crd.data_ptr(), count, S, rgb.data_ptr(), None, None, st), "ego_shade")
        _lib.check(lib.ego_msi_layers(z.data_ptr(), alpha.data_ptr(), S, rgb.data_ptr(), count, S, bounds_dev.data_ptr(), L, first, texels,
                                      TEXEL_TYPES[dtype], image.data_ptr(), st), "ego_msi_layers")
        if has_env:
            dirs[:count] = rays[:count, 3:6]
            _lib.check(lib.ego_envmap_radiance(sc, dirs.data_ptr(), count, env.data_ptr(), st), "ego_envmap_radiance")
            flat = background.view(texels, 4)
            flat[first:first + count, :3] = env[:count].to(dtype)
            flat[first:first + count, 3] = 1
    return MultiSphereImage(image, radii, bounds, c, list(model.near_far), background)


def project_msi(msi: MultiSphereImage) -> None:
    """In place on float32 texels (ego_msi_project): C <- max(C, 0), A <- clamp(A, 0, 1), so that playback's transmittance stays in [0, 1]."""
    if msi.layers.dtype != torch.float32 or not msi.layers.is_cuda:
        raise ValueError("project_msi: needs float32 texels on a HIP device")
    lib, st = _lib.load(), _lib.stream_handle()
    for t in msi.parameters():
        _lib.check(lib.ego_msi_project(t.data_ptr(), t.numel() // 4, st), "ego_msi_project")
        torch.autograd.graph.increment_version(t)   # written through a raw pointer


def headbox_rays(n: int, center: torch.Tensor, headbox: float, generator: torch.Generator) -> torch.Tensor:
    """[n, 6] float32 on the device of `center` ([3] float32, a DEVICE tensor: nothing here copies from the host, so a loop that draws
    rays does not wait for its stream): origins uniform in the ball of radius `headbox` around `center`, directions uniform on the unit
    sphere."""
    device = center.device
    o = torch.randn(n, 3, device=device, generator=generator)
    o = o * (headbox * torch.rand(n, 1, device=device, generator=generator) ** (1.0 / 3.0) / o.norm(dim=1, keepdim=True).clamp_min(1e-20))
    d = torch.randn(n, 3, device=device, generator=generator)
    d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-20)
    return torch.cat([o + center, d], dim=1).contiguous()


DEFAULT_REFINE_LR = 1e-3


def refine_msi(msi: MultiSphereImage, teacher, steps: int, rays_per_step: int = 65536, headbox: Optional[float] = None,
               lr: float = DEFAULT_REFINE_LR, seed: int = 0, render_kwargs: Optional[dict] = None, log: Optional[list] = None,
               optimizer: str = "dense") -> MultiSphereImage:
    """Optimises the texels of `msi` against `teacher` (a model, or anything called like one) on rays from inside a headbox; returns a
    new image of the input's texel type, radii, bounds, centre and near_far.

    Works on a float32 copy.  Per step: `rays_per_step` rays drawn on the device from a generator seeded with `seed` (origins uniform in
    the ball of radius `headbox` - scene units, 0 < headbox < radii[0], default 0.2 radii[0] - around the centre, unit directions uniform
    on the sphere); the target `teacher(rays, is_train=False, need_alpha=False, **render_kwargs)[0]` under no_grad; the mean squared
    error of `render(rays)[0]` against it; backward (ego_msi_render_backward); one FusedAdam step at `lr`; ego_msi_project.  Nothing in
    the loop synchronises with the host; `log`, if a list, receives every step's loss as a device tensor.

    `lr`: Adam walks a texel by about 10 lr for every isolated hit, whatever the gradient's size, so the rate has to fit how often a
    texel is hit.  The default suits an image whose texels are hit in every step; a 1024 x 2048 image under 65536 rays per step
    (a texel hit once in eight steps) needs 1e-5 to 3e-5 and is made worse by 1e-3 (profiles/r13/msi_refine.json).

    `optimizer`: "dense" (the default) is the loop above.  "texel" steps only the texels a batch hit, each on its own clock
    (`optim.TexelAdam`, ego_msi_adam_step): the image is projected once before the loop; per step the same rays, target and loss, the
    loss's gradient `(rgb - target) 2 / (3 N)` handed straight to ego_msi_render_backward, which adds into gradient buffers allocated
    and zeroed once, and one fused step that updates, projects and re-zeroes exactly the texels that received a gradient - no autograd,
    no pass over the whole image to zero, step or project it.  An isolated hit then moves a texel by at most `lr` and is not walked
    on.  Use "dense" when every texel is hit in (nearly) every step - a small image, many rays - where the two rules coincide and
    "dense" is the loop the tests pin bit for bit; use "texel" when a step reaches a fraction of the texels, as a 1024 x 2048 image
    under 65536 rays does.  Measured there (DESIGN.md 3.3 "Texel Adam", profiles/r16/msi_texel_adam.json) it takes a fifth off the
    step and is 7 dB better than "dense" at 1e-3, but it does not change which rates work: 3e-5 to 1e-4 there, for either loop."""
    from .optim import FusedAdam
    steps, n = int(steps), int(rays_per_step)
    if steps < 0 or n < 1:
        raise ValueError(f"refine_msi: steps must be >= 0 and rays_per_step >= 1, got {steps} and {n}")
    if not lr > 0:
        raise ValueError(f"refine_msi: lr must be positive, got {lr}")
    if optimizer not in ("dense", "texel"):
        raise ValueError(f'refine_msi: optimizer must be "dense" or "texel", got {optimizer!r}')
    r0 = float(msi.radii[0])
    headbox = 0.2 * r0 if headbox is None else float(headbox)
    if not 0 < headbox < r0:
        raise ValueError(f"refine_msi: headbox must lie in (0, radii[0] = {r0:g}) - the eye stays inside the innermost shell - got {headbox:g}")
    if not msi.layers.is_cuda:
        raise ValueError("refine_msi: the image must live on a HIP device (the HIP path has no CPU fallback)")
    dev, kw = msi.device, dict(render_kwargs or {})
    if optimizer == "texel":
        return _refine_texel(msi, teacher, steps, n, headbox, lr, seed, kw, log)
    bg = None if msi.background is None else msi.background.detach().float().clone().requires_grad_(True)
    work = MultiSphereImage(msi.layers.detach().float().clone().requires_grad_(True), msi.radii, msi.bounds, msi.center, msi.near_far, bg)
    with torch.cuda.device(dev), torch.enable_grad():   # a caller's no_grad must not reach the loop's backward
        opt = FusedAdam(list(work.parameters()), lr=lr, betas=(0.9, 0.99))
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        center = torch.from_numpy(msi.center).to(dev)   # once, before the loop: a copy from host memory waits for the stream
        for _ in range(steps):
            rays = headbox_rays(n, center, headbox, gen)
            with torch.no_grad():
                target = teacher(rays, is_train=False, need_alpha=False, **kw)[0]
            loss = torch.mean((work.render(rays)[0] - target) ** 2)
            loss.backward()
            opt.step()
            opt.zero_grad()
            project_msi(work)
            if isinstance(log, list):
                log.append(loss.detach())
    out_bg = None if bg is None else bg.detach().to(msi.layers.dtype)
    return MultiSphereImage(work.layers.detach().to(msi.layers.dtype), msi.radii, msi.bounds, msi.center, msi.near_far, out_bg)


@torch.no_grad()
def _refine_texel(msi: MultiSphereImage, teacher, steps: int, n: int, headbox: float, lr: float, seed: int, kw: dict,
                  log: Optional[list]) -> MultiSphereImage:
    """refine_msi's "texel" loop (arguments already checked): no autograd, nothing that sweeps the whole image inside the loop."""
    from .optim import TexelAdam
    dev = msi.device
    bg = None if msi.background is None else msi.background.detach().float().clone()
    work = MultiSphereImage(msi.layers.detach().float().clone(), msi.radii, msi.bounds, msi.center, msi.near_far, bg)
    with torch.cuda.device(dev):
        project_msi(work)   # once: from here on only stepped texels move, and the step projects them
        params = list(work.parameters())
        for p in params:
            p.grad = torch.zeros_like(p)   # once: the step leaves them zero
        g_bg = None if bg is None else bg.grad
        opt = TexelAdam(params, lr=lr, betas=(0.9, 0.99), project=True, zero_grad=True)
        opt.step()   # on the all-zero gradient: touches no texel and creates the state (a copy from host memory) outside the loop
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        center = torch.from_numpy(msi.center).to(dev)   # once, before the loop: a copy from host memory waits for the stream
        scale = 2.0 / (3 * n)
        for _ in range(steps):
            rays = headbox_rays(n, center, headbox, gen)
            target = teacher(rays, is_train=False, need_alpha=False, **kw)[0]
            diff = work._render(rays, work.layers, work.background)[0] - target
            work._render_backward(rays, work.layers, work.background, diff * scale, work.layers.grad, g_bg)
            opt.step()
            if isinstance(log, list):
                log.append(torch.mean(diff ** 2))
    out_bg = None if bg is None else bg.to(msi.layers.dtype)
    for p in params:
        p.grad = None
    return MultiSphereImage(work.layers.to(msi.layers.dtype), msi.radii, msi.bounds, msi.center, msi.near_far, out_bg)
