"""Host-side mirror of the reference model surface for the volume-rendering path:

    models/tensorBase.py : raw2alpha, MLPRender_Fea, TensorBase (ctor kwargs, feature2density, save/load)
    models/EgoNeRF.py    : EgoNeRF (forward, compute_densityfeature, compute_coarse_densityfeature,
                           compute_appfeature, sample_ray_exp, update_coarse_sigma_grid,
                           get_optparam_groups, save, load)
    models/envmap.py     : EnvironmentMap

Same names, argument meaning, state-dict keys and return tuples, so the parity tests read like calls into
the reference.  All per-sample arithmetic runs in libegonerf_hip.so through the C ABI (egonerf_amd/_lib.py);
PyTorch only owns device memory, streams and parameters.  There is no CPU fallback: calling the path with
CPU tensors raises.

Parameters keep the reference's shapes ((1,C,H,W) planes, (1,C,L,1) lines) but are allocated channel-last
([H][W][C] in memory), which is the layout the kernels gather from; `state_dict()` keys and shapes are the
reference's, so checkpoints interchange.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional

import math
import numpy as np
import torch
import torch.nn

from . import _lib, field_tables, stage_autograd
from .coordinates import YinYangSphericalCoords, _require_cuda
from .losses import table_regulariser

MAT_MODE = [[0, 1], [0, 2], [1, 2]]  # models/EgoNeRF.py:30-33
VEC_MODE = [2, 1, 0]


def _call(name: str, *args) -> None:
    _lib.check(getattr(_lib.load(), name)(*args), name)


def _last_dim(t: torch.Tensor, n: int, what: str) -> None:
    """The reference indexes `[..., k]` and fails with an IndexError on a short last axis; a raw-pointer call would silently
    reinterpret the memory instead."""
    if t.dim() < 1 or t.shape[-1] != n:
        raise IndexError(f"{what}: expected [..., {n}], got {tuple(t.shape)}")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().float()


# ---------------------------------------------------------------------------------------------------
# models/tensorBase.py
# ---------------------------------------------------------------------------------------------------
@_lib.device_guard
def raw2alpha(sigma: torch.Tensor, dist: torch.Tensor):
    """alpha, weights, bg_weight of tensorBase.py:22-27 (sigma, dist: [N_rays, N_samples]).  Differentiable (to sigma and dist) when grad
    mode is on and either requires grad: the forward values are the same bits, the backward (stage_autograd.Raw2AlphaFunction) is the
    fp32-grade gradient of the reference function."""
    _require_cuda(sigma, "raw2alpha")
    if stage_autograd.needs_grad(sigma, dist):
        return stage_autograd.Raw2AlphaFunction.apply(sigma, dist)
    return _raw2alpha(sigma, dist)


def _raw2alpha(sigma: torch.Tensor, dist: torch.Tensor):
    _require_cuda(sigma, "raw2alpha")
    sigma, dist = _f32c(sigma), _f32c(dist)
    N, S = sigma.shape
    alpha, weight = torch.empty_like(sigma), torch.empty_like(sigma)
    bg = torch.empty(N, 1, device=sigma.device)
    _call("ego_raw2alpha", sigma.data_ptr(), dist.data_ptr(), N, S, alpha.data_ptr(), weight.data_ptr(), bg.data_ptr(),
          _lib.stream_handle())
    return alpha, weight, bg


class EnvironmentMap:
    """models/envmap.py:17-37: plain requires_grad tensor `emission` [3, 2h, h] (not an nn.Parameter)."""

    def __init__(self, h=1000, init_strategy="random", device="cuda"):
        if init_strategy == "random":
            self.emission = torch.rand((3, 2 * h, h), requires_grad=True, device=device)
        elif init_strategy == "zero":
            self.emission = torch.zeros((3, 2 * h, h), requires_grad=True, device=device)
        else:
            raise ValueError("Unknown environment map initialization: {}".format(init_strategy))

    @_lib.device_guard
    def get_radiance(self, direction: torch.Tensor) -> torch.Tensor:
        _require_cuda(direction, "EnvironmentMap.get_radiance")
        d = _f32c(direction)
        if torch.is_grad_enabled() and self.emission.requires_grad:  # envmap pre-training (train.py:218-236)
            from .train import EnvRadianceFunction
            return EnvRadianceFunction.apply(self.emission, d)
        out = torch.empty(d.shape[0], 3, device=d.device)
        sc = _lib.new_scene()
        em = self.emission.detach().contiguous()
        sc.envmap, sc.envmap_h = em.data_ptr(), em.shape[2]
        _call("ego_envmap_radiance", sc, d.data_ptr(), d.shape[0], out.data_ptr(), _lib.stream_handle())
        return out

    def __reduce_ex__(self, protocol):
        """Inside compat.reference_pickle_paths() (EgoNeRF.save): pickles as models.envmap.EnvironmentMap {emission}."""
        from . import compat
        if not compat.pickling_as_reference():
            return super().__reduce_ex__(protocol)
        return compat.reduce_as_reference("models.envmap", "EnvironmentMap", {"emission": self.emission})

    def load_envmap(self, emission, device):
        self.emission = torch.tensor(np.asarray(emission.detach().cpu() if torch.is_tensor(emission) else emission),
                                     requires_grad=True, device=device, dtype=torch.float32)


@_lib.device_guard
def SHRender(xyz_sampled, viewdirs: torch.Tensor, features: torch.Tensor) -> torch.Tensor:
    """models/tensorBase.py:30-34: degree-2 SH colour head, viewdirs [M,3], features [M,27] -> rgb [M,3] = relu(SH . f + 0.5).
    (`xyz_sampled` is unused, as in the reference.  The reference's EgoNeRF.forward cannot run with this head — it hands
    SHRender [N,S,3] view directions against [N*S,3,9] features and the broadcast raises — so it is offered as the stage
    function only.)  Differentiable (to viewdirs and features) when grad mode is on and either requires grad: same forward bits,
    fp32-grade backward (stage_autograd.SHRenderFunction)."""
    _require_cuda(viewdirs, "SHRender")
    if stage_autograd.needs_grad(viewdirs, features):
        return stage_autograd.SHRenderFunction.apply(viewdirs, features)
    return _sh_render(viewdirs, features)


def _sh_render(viewdirs: torch.Tensor, features: torch.Tensor) -> torch.Tensor:
    _require_cuda(viewdirs, "SHRender")
    d, f = _f32c(viewdirs.reshape(-1, 3)), _f32c(features.reshape(-1, 27))
    if d.shape[0] != f.shape[0]:
        raise RuntimeError("SHRender: viewdirs and features disagree on the number of points")
    out = torch.empty(d.shape[0], 3, device=d.device)
    _call("ego_sh_render", d.data_ptr(), f.data_ptr(), d.shape[0], out.data_ptr(), _lib.stream_handle())
    return out


class MLPRender_Fea(torch.nn.Module):
    """tensorBase.py:54-78.  The Linear layers only hold the weights (state-dict keys `mlp.{0,2,4}.*`);
    forward runs the fused PE + 150->128->128->3 + sigmoid MFMA kernel."""

    def __init__(self, inChannel, viewpe=6, feape=6, featureC=128):
        super().__init__()
        self.in_mlpC = 2 * viewpe * 3 + 2 * feape * inChannel + 3 + inChannel
        self.viewpe, self.feape = viewpe, feape
        self.mlp = torch.nn.Sequential(torch.nn.Linear(self.in_mlpC, featureC), torch.nn.ReLU(inplace=True),
                                       torch.nn.Linear(featureC, featureC), torch.nn.ReLU(inplace=True),
                                       torch.nn.Linear(featureC, 3))
        torch.nn.init.constant_(self.mlp[-1].bias, 0)
        self._owner = None  # set by the model: provides the packed weights

    @_lib.device_guard
    def forward(self, pts, viewdirs, features):
        """Differentiable (to mlp.{0,2,4}.{weight,bias}, features and viewdirs) when grad mode is on and any of them requires grad: the
        forward runs the same kernel with the model's mlp_precision (same bits), the backward (stage_autograd.MLPRenderFunction) is the
        fp32 gradient of the reference head at the fp32 weights."""
        _require_cuda(features, "MLPRender_Fea")
        if self._owner is None:
            raise RuntimeError("MLPRender_Fea must belong to an EgoNeRF model (it owns the packed MFMA weights)")
        from .stage_autograd import needs_grad
        weights = [self.mlp[0].weight, self.mlp[0].bias, self.mlp[2].weight, self.mlp[2].bias, self.mlp[4].weight, self.mlp[4].bias]
        if needs_grad(viewdirs, features, *weights):
            from .stage_autograd import MLPRenderFunction
            return MLPRenderFunction.apply(self, viewdirs, features, *weights)
        return self._forward_impl(viewdirs, features)

    def _forward_impl(self, viewdirs, features):
        _require_cuda(features, "MLPRender_Fea")
        model = self._owner()
        v = _f32c(viewdirs.reshape(-1, 3))
        f = _f32c(features.reshape(-1, features.shape[-1]))
        out = torch.empty(f.shape[0], 3, device=f.device)
        _call("ego_mlp_fea", model.scene(), v.data_ptr(), f.data_ptr(), f.shape[0], out.data_ptr(), _lib.stream_handle())
        return out.view(*features.shape[:-1], 3)


class MLPRender(MLPRender_Fea):
    """tensorBase.py:107-129 (shadingMode 'MLP'): mlp_in = [features, viewdirs, PE(viewdirs)] - MLPRender_Fea without the feature
    encoding, same state-dict keys `mlp.{0,2,4}.*`; runs the any-shape kernels (csrc/ego_generic.hip) with fea_pe = 0."""

    def __init__(self, inChannel, viewpe=6, featureC=128):
        super().__init__(inChannel, viewpe, 0, featureC)
        del self.feape   # the reference class has no such attribute


def RGBRender(xyz_sampled, viewdirs, features):
    """tensorBase.py:37-39 (shadingMode 'RGB', app_dim == 3): the colour is the appearance feature.  A plain function like the
    reference's (no parameters: `isinstance(renderModule, torch.nn.Module)` is False, EgoNeRF.py:152)."""
    return features


class TensorBase(torch.nn.Module):
    """Constructor surface and shared helpers of tensorBase.py:132-186, 206-217, 241-295, 415-419."""

    def __init__(self, aabb, gridSize, device, coordinates, density_n_comp=8, appearance_n_comp=24, app_dim=27,
                 shadingMode="MLP_PE", alphaMask=None, near_far=[2.0, 6.0], density_shift=-10, alphaMask_thres=0.001,
                 distance_scale=25, rayMarch_weight_thres=0.0001, pos_pe=6, view_pe=6, fea_pe=6, featureC=128,
                 step_ratio=2.0, fea2denseAct="softplus", use_envmap=False, envmap_res_H=1000, envmap=None,
                 coarse_sigma_grid_update_rule=None, coarse_sigma_grid_reso=None, interval_th=False):
        super().__init__()
        as_list = lambda n: list(n) if isinstance(n, (list, tuple)) else [n] * 3
        self.density_n_comp, self.app_n_comp, self.app_dim = as_list(density_n_comp), as_list(appearance_n_comp), app_dim
        self.aabb = torch.as_tensor(aabb, dtype=torch.float32)
        self.alphaMask = alphaMask
        self.device = device
        self.density_shift, self.alphaMask_thres, self.distance_scale = density_shift, alphaMask_thres, distance_scale
        self.rayMarch_weight_thres, self.fea2denseAct = rayMarch_weight_thres, fea2denseAct
        self.near_far, self.step_ratio = list(near_far), step_ratio
        self.update_stepSize(gridSize)
        self.envmap = None
        if use_envmap:
            if envmap is None:
                self.init_envmap(envmap_res_H, init_strategy="random", device=device)
            else:
                self.envmap = EnvironmentMap(h=envmap.emission.shape[2], init_strategy="zero", device=device)
                self.envmap.load_envmap(envmap.emission, device=device)
        self.shadingMode, self.pos_pe, self.view_pe, self.fea_pe, self.featureC = shadingMode, pos_pe, view_pe, fea_pe, featureC
        self.init_render_func(shadingMode, pos_pe, view_pe, fea_pe, featureC, device)
        self.coordinates = coordinates
        self.coarse_sigma_grid_update_rule = coarse_sigma_grid_update_rule

    def init_render_func(self, shadingMode, pos_pe, view_pe, fea_pe, featureC, device):
        """tensorBase.py:186-200, for the heads the reference's EgoNeRF.forward can run with: 'MLP_Fea' (every shipped config,
        configs/EgoNeRF/common.txt:34), 'MLP' and 'RGB'.  'MLP_PE' (the ctor default) and 'SH' raise inside the reference's
        EgoNeRF.forward - MLPRender_PE is handed 7-column yin-yang coordinates for a 3-column position encoding (shape error in its
        first Linear), SHRender [N,S,3] directions against [N*S,3,9] features - so they are refused here at construction
        (SHRender exists as a stage function)."""
        if shadingMode == "MLP_Fea":
            self.renderModule = MLPRender_Fea(self.app_dim, view_pe, fea_pe, featureC).to(device)
        elif shadingMode == "MLP":
            self.renderModule = MLPRender(self.app_dim, view_pe, featureC).to(device)
        elif shadingMode == "RGB":
            assert self.app_dim == 3   # tensorBase.py:198
            self.renderModule = RGBRender
        else:
            raise NotImplementedError(f"shadingMode {shadingMode!r}: EgoNeRF.forward runs with 'MLP_Fea', 'MLP' or 'RGB' (the reference's own "
                                      "forward raises with 'MLP_PE' and 'SH')")

    @property
    def head_fea_pe(self) -> int:
        """Feature-encoding frequencies of the head as built (MLPRender ignores the `fea_pe` argument, RGBRender has no network)."""
        return self.fea_pe if self.shadingMode == "MLP_Fea" else 0

    @property
    def head_in_mlpC(self) -> int:
        return self.renderModule.in_mlpC if self.shadingMode != "RGB" else 0

    @property
    def head_hidden(self) -> int:
        return self.featureC if self.shadingMode != "RGB" else 0

    def init_envmap(self, envmap_res_H, init_strategy="zero", device="cuda"):
        self.envmap = EnvironmentMap(h=envmap_res_H, init_strategy=init_strategy, device=device)

    def update_stepSize(self, gridSize):
        """tensorBase.py:206-217 (values unused by EgoNeRF.forward, kept for get_kwargs/alpha-mask parity)."""
        self.aabbSize = self.aabb[1] - self.aabb[0]
        self.invaabbSize = 2.0 / self.aabbSize
        self.gridSize = torch.LongTensor(list(gridSize))
        self.units = self.aabbSize / (self.gridSize - 1)
        self.stepSize = torch.mean(self.units) * self.step_ratio
        self.aabbHalfDiag = torch.sqrt(torch.sum(torch.square(self.aabbSize))) / 2.0
        self.nSamples = int((self.aabbHalfDiag / self.stepSize).item()) + 1

    def get_kwargs(self):
        return {"aabb": self.aabb, "gridSize": self.gridSize.tolist(), "density_n_comp": self.density_n_comp,
                "appearance_n_comp": self.app_n_comp, "app_dim": self.app_dim, "density_shift": self.density_shift,
                "alphaMask_thres": self.alphaMask_thres, "distance_scale": self.distance_scale,
                "rayMarch_weight_thres": self.rayMarch_weight_thres, "fea2denseAct": self.fea2denseAct,
                "near_far": self.near_far, "step_ratio": self.step_ratio, "shadingMode": self.shadingMode,
                "pos_pe": self.pos_pe, "view_pe": self.view_pe, "fea_pe": self.fea_pe, "featureC": self.featureC,
                "coordinates": self.coordinates, "use_envmap": self.envmap is not None, "envmap": self.envmap,
                "coarse_sigma_grid_update_rule": self.coarse_sigma_grid_update_rule}

    @_lib.device_guard
    def feature2density(self, density_features: torch.Tensor) -> torch.Tensor:
        """tensorBase.py:415-419.  Differentiable when grad mode is on and the features require grad: same forward bits, the backward
        (stage_autograd.Feature2DensityFunction) differentiates softplus (threshold 20) / relu as torch does."""
        _require_cuda(density_features, "feature2density")
        from .stage_autograd import needs_grad
        if needs_grad(density_features):
            from .stage_autograd import Feature2DensityFunction
            return Feature2DensityFunction.apply(self, density_features)
        return self._feature2density_forward(density_features)

    def _feature2density_forward(self, density_features: torch.Tensor) -> torch.Tensor:
        _require_cuda(density_features, "feature2density")
        f = _f32c(density_features)
        out = torch.empty_like(f)
        sc = _lib.new_scene()
        sc.act_softplus, sc.density_shift = int(self.fea2denseAct == "softplus"), float(self.density_shift)
        _call("ego_feature2density", sc, f.data_ptr(), f.numel(), out.data_ptr(), _lib.stream_handle())
        return out


# ---------------------------------------------------------------------------------------------------
# models/EgoNeRF.py
# ---------------------------------------------------------------------------------------------------
class YinYangAlphaGridMask(torch.nn.Module):
    """models/EgoNeRF.py:11-24: two {0,1} volumes shaped (1,1,N_phi,N_theta,N_r); sample_alpha = trilinear lookup."""

    def __init__(self, device, alpha_volume_yin, alpha_volume_yang):
        super().__init__()
        self.device = device
        self.alpha_volume_yin = alpha_volume_yin.view(1, 1, *alpha_volume_yin.shape[-3:])
        self.alpha_volume_yang = alpha_volume_yang.view(1, 1, *alpha_volume_yang.shape[-3:])
        self._bytes = self._cells = None

    def packed(self) -> torch.Tensor:
        """[2][N_phi][N_theta][N_r] uint8 (what the kernels read)."""
        if self._bytes is None:
            self._bytes = torch.stack([self.alpha_volume_yin[0, 0], self.alpha_volume_yang[0, 0]]).gt(0).to(torch.uint8).contiguous()
        return self._bytes

    def cell_or(self) -> Optional[torch.Tensor]:
        """[2][N_phi-1][N_theta-1][N_r-1] uint8: OR of every cell's eight corner voxels (ego_scene.occ_cell: the march's one-byte
        answer to "trilinear mask value > 0" for samples strictly inside a cell)."""
        vol = self.packed()
        if min(vol.shape[1:]) < 2:
            return None
        if self._cells is None:
            self._cells = torch.nn.functional.max_pool3d(vol.float()[None], kernel_size=2, stride=1)[0].to(torch.uint8).contiguous()
        return self._cells

    def fill_scene(self, sc):
        vol = self.packed()
        sc.occ = vol.data_ptr()
        sc.occ_res[:] = [vol.shape[3], vol.shape[2], vol.shape[1]]
        cells = self.cell_or()
        sc.occ_cell = None if cells is None else cells.data_ptr()

    @_lib.device_guard
    def sample_alpha(self, norm_samples):
        _require_cuda(norm_samples, "sample_alpha")
        _last_dim(norm_samples, 7, "sample_alpha")
        c = _f32c(norm_samples)
        out = torch.empty(c.shape[:-1], device=c.device)
        sc = _lib.new_scene()
        self.fill_scene(sc)
        _call("ego_alpha_mask_sample", sc, c.data_ptr(), c.numel() // 7, out.data_ptr(), _lib.stream_handle())
        return out


class _SceneEntry:
    """EgoNeRF's one cached ego_scene struct, with everything the struct points to that nobody else keeps alive."""

    def __init__(self, blobs=None, app16=None, dense=None, app_dense=None):
        self.key = None      # EgoNeRF._scene_key() the struct was built for; None: nothing cached
        self.struct = None
        self.holds = ()      # detached MLP / basis weights behind mlp_w, mlp_b, basis
        self.luts = ()       # the radius LUTs behind r_lut, r_lut_fine
        self.mask = None     # model.alphaMask at build time: its packed() / cell_or() buffers are behind occ, occ_cell
        self.blobs = {} if blobs is None else blobs   # {training: packed MLP / basis image}; outlives an invalidation
        self.app16 = app16   # (appearance table versions, [12 half tables]) behind app16; outlives an invalidation
        # {"full" / "coarse": (table versions, baked node grid)} behind density_dense / density_coarse_dense; outlives an invalidation
        self.dense = dense
        # (versions of the twelve appearance tables and both basis matrices, baked feature grid) behind app_dense; outlives an invalidation
        self.app_dense = app_dense

    def successor(self) -> "_SceneEntry":
        """An empty entry that keeps what outlives an invalidation."""
        return _SceneEntry(self.blobs, self.app16, self.dense, self.app_dense)


class EgoNeRF(TensorBase):
    supports_need_alpha = True  # forward(..., need_alpha=False): see volume_renderer(keep_alpha=False)
    supports_marched_event = True  # forward(..., marched_event=ev): see renderer._render_to_host
    def __init__(self, aabb, gridSize, device, coordinates, **kargs):
        super().__init__(aabb, gridSize, device, coordinates, **kargs)
        assert isinstance(coordinates, YinYangSphericalCoords), "EgoNeRF needs YinYangSphericalCoords (EgoNeRF.py:522)"
        self.matMode_yin = self.matMode_yang = MAT_MODE
        self.vecMode_yin = self.vecMode_yang = VEC_MODE
        self._scene = _SceneEntry()
        self._sched_cache = {}
        self.init_svd_volume(gridSize[0], device)
        if isinstance(self.renderModule, torch.nn.Module):
            self.renderModule._owner = _WeakOwner(self)
        self._last_render = self._last_shaded = None   # see forward / last_shaded_samples
        # The sample distances [N, S] of the latest TRAINING render (train.render_train: the march's own buffer, no gradient): what
        # losses.distortion_loss needs next to the returned alpha.  Eval renders leave it alone.
        self.last_train_z = None
        self._mlp_precision = "f16f6"   # inference default; differentiable calls always use the three-term fp16 split
        # Differentiable calls of the tuned head keep the activations that only feed the weight-gradient products (x, h1, h2, dh1, dh2)
        # as halves (~2^-12 relative per operand against the reference's fp32 autograd, nothing above 65504).  True (or
        # EGO_TRAIN_FP32=1 in the environment at construction) trains it through the fp32 compatibility kernels instead: the parity
        # mode, several times slower.
        self.train_fp32_head = os.environ.get("EGO_TRAIN_FP32", "0") not in ("", "0")
        # Table gradients of a differentiable call: True (default) = sort the step's samples by texel cell and write every gradient texel
        # once, in a fixed order - no atomics, two runs return the same bits (csrc/ego_scatter_sorted.hip); False (or EGO_SCATTER=atomic
        # at construction) = the float-atomic scatters of rounds 1-4 (run-to-run differences of ~1e-6 of the largest gradient).
        self.deterministic_scatter = os.environ.get("EGO_SCATTER", "sorted") != "atomic"
        self._app_table_dtype = "f32"   # "f16": inference gathers appearance taps from a half-precision copy of the tables
        # Inference of the tuned shape marches its 16-component density field from its baked node grid (csrc/ego_dense.hip): 8 taps of 16 B
        # per sample instead of 18 of 64 B, for 2 x N_r N_theta N_phi x 16 B of device memory (426 MB at [150, 172, 516]; the pooled
        # field adds an eighth).  Part of the scene key.  EGO_DENSE_DENSITY=0|1 in the environment overrides the attribute; the grid is
        # baked only while it fits EGO_DENSE_DENSITY_MAX_MB (default 1024) and a quarter of the free device memory - see _fill_dense.
        self.dense_density = True
        # ... and shades from the baked node grid of its 27 appearance features (csrc/ego_dense.hip): 8 taps of one 128-byte
        # node per sample instead of 18 table taps and the basis product, for 2 x N_r N_theta N_phi x 128 B of device memory (3.41 GB at
        # [150, 172, 516]).  Part of the scene key.  EGO_DENSE_APP=0|1 in the environment overrides the attribute; the grid is baked only
        # for fp32 appearance tables and a split arithmetic, while it fits EGO_DENSE_APP_MAX_MB (default 4096), a quarter of the free
        # device memory and 32-bit byte offsets - see _fill_app_dense.
        self.dense_appearance = True
        self._coarse_epoch = 0   # counts update_coarse_sigma_grid() calls: the pooled tables are rewritten behind torch's version counters
        # opt-in skipping (EgoNeRF.forward itself evaluates every sample; TensorBase.forward's semantics, tensorBase.py:464-487,
        # pinned to the reference by tests/golden/skip_semantics.npz; see include/egonerf_hip.h):
        self.use_alpha_mask = False          # apply self.alphaMask with TensorBase.forward's semantics (sigma = 0 where empty)
        self.early_termination_eps = 0.0     # > 0: zero the weight of samples behind transmittance < eps
        self.use_weight_thres = False        # TensorBase.forward's app skip: samples with weight <= rayMarch_weight_thres get rgb = 0
        # Exact skipping, on by default: 32-sample tiles whose weights are all exactly 0 are not shaded (ego_scene.weight_thres = 0).
        # The outputs are bit-identical - the reference adds w * rgb = 0 for such samples (EgoNeRF.py:583) - and behind an opaque
        # surface the fp32 transmittance underflows to 0 within a few samples, so this is what early termination amounts to.
        # EGO_EXACT_SKIP=0 in the environment switches it off for A/B measurements.
        self.skip_zero_weight_tiles = os.environ.get("EGO_EXACT_SKIP", "1") != "0"
        for name in field_tables.list_names("density", coarse=True):
            setattr(self, name, [None] * 3)
        if self.coarse_sigma_grid_update_rule is not None:
            if self.coarse_sigma_grid_update_rule != "conv":
                raise NotImplementedError  # EgoNeRF.py:92-94
            if torch.device(device).type == "cuda":
                self.update_coarse_sigma_grid()

    # -- parameters -------------------------------------------------------------------------------------
    def init_one_svd(self, n_component, gridSize, scale, device):
        """EgoNeRF.py:102-122, channel-last memory."""
        shapes = []
        for _grid in ("yin", "yang"):
            for i in range(3):
                m0, m1 = MAT_MODE[i]
                shapes.append((n_component[i], gridSize[m1], gridSize[m0]))
            for i in range(3):
                shapes.append((n_component[i], gridSize[VEC_MODE[i]], 1))
        views = field_tables.carve_channel_last(shapes, device)   # field_tables' order, four lists of three: one buffer per field
        for v, (C_, H, W) in zip(views, shapes):
            v.copy_(scale * torch.randn(1, C_, H, W))
        return [torch.nn.ParameterList([torch.nn.Parameter(v) for v in views[k:k + 3]]) for k in range(0, 12, 3)]

    def _apply(self, fn, *args, **kwargs):
        """nn.Module._apply re-allocates every parameter on its own; restore what the kernels rely on afterwards: one buffer per
        field (compact addressing), the non-parameter device state (pooled density tables, packed weights, half copies) on
        the new device."""
        r = super()._apply(fn, *args, **kwargs)
        self.invalidate_scene(moved=True)
        self._sched_cache = {}
        dev = self.device = self.density_plane_yin[0].device
        if dev.type == "cuda":
            for kind in ("density", "app"):
                if not field_tables.is_compact(field_tables.tables(self, kind)):
                    field_tables.recarve(self, kind, keep_parameters=True)
            stale = self.coarse_sigma_plane_yin[0] is None or self.coarse_sigma_plane_yin[0].device != dev
            if self.coarse_sigma_grid_update_rule == "conv" and stale:
                self.update_coarse_sigma_grid()
        return r

    def init_svd_volume(self, res, device):
        g = self.gridSize.tolist()
        for kind, n_comp in (("density", self.density_n_comp), ("app", self.app_n_comp)):
            for name, plist in zip(field_tables.list_names(kind), self.init_one_svd(n_comp, g, 0.1, device)):
                setattr(self, name, plist)
        self.basis_mat_yin = torch.nn.Linear(sum(self.app_n_comp), self.app_dim, bias=False).to(device)
        self.basis_mat_yang = torch.nn.Linear(sum(self.app_n_comp), self.app_dim, bias=False).to(device)

    def get_optparam_groups(self, lr_init_spatialxyz=0.02, lr_init_network=0.001, lr_init_envmap=0.1):
        """EgoNeRF.py:139-156."""
        gv = []
        for g in ("yin", "yang"):
            gv += [{"params": getattr(self, f"density_line_{g}"), "lr": lr_init_spatialxyz},
                   {"params": getattr(self, f"density_plane_{g}"), "lr": lr_init_spatialxyz},
                   {"params": getattr(self, f"app_line_{g}"), "lr": lr_init_spatialxyz},
                   {"params": getattr(self, f"app_plane_{g}"), "lr": lr_init_spatialxyz},
                   {"params": getattr(self, f"basis_mat_{g}").parameters(), "lr": lr_init_network}]
        if isinstance(self.renderModule, torch.nn.Module):   # EgoNeRF.py:152 (RGBRender is a function)
            gv += [{"params": self.renderModule.parameters(), "lr": lr_init_network}]
        if self.envmap is not None:
            gv += [{"params": self.envmap.emission, "lr": lr_init_envmap}]
        return gv

    # -- regularisers (train.py:289-304) ----------------------------------------------------------------------
    def vectorDiffs(self, vector_comps):
        """EgoNeRF.py:189-196: sum over line tables of mean |off-diagonal of the component Gram matrix|."""
        return table_regulariser("ortho", list(vector_comps), [1.0] * len(vector_comps))

    def vector_comp_diffs(self):
        """EgoNeRF.py:198-199."""
        lines = (list(self.density_line_yin) + list(self.app_line_yin) + list(self.density_line_yang) + list(self.app_line_yang))
        return table_regulariser("ortho", lines, [1.0] * len(lines))

    def density_L1(self):
        """EgoNeRF.py:206-212."""
        t = []
        for i in range(len(self.density_plane_yin)):
            t += [self.density_plane_yin[i], self.density_line_yin[i], self.density_plane_yang[i], self.density_line_yang[i]]
        return table_regulariser("l1", t, [1.0] * len(t))

    def _tv(self, reg, planes):
        w = float(getattr(reg, "TVLoss_weight", 1.0))
        return table_regulariser("tv", planes, [1e-2 * w] * len(planes))

    def TV_loss_density(self, reg):
        """EgoNeRF.py:214-220: planes only, 1e-2 each; `reg` is a TVLoss (its weight is honoured, its forward is fused here)."""
        return self._tv(reg, [p for i in range(3) for p in (self.density_plane_yin[i], self.density_plane_yang[i])])

    def TV_loss_app(self, reg):
        """EgoNeRF.py:222-228."""
        return self._tv(reg, [p for i in range(3) for p in (self.app_plane_yin[i], self.app_plane_yang[i])])

    # -- coarse-to-fine upsampling (train.py:371-385) -------------------------------------------------------------
    @torch.no_grad()
    def up_sampling_VM(self, plane_coef, line_coef, res_target):
        """EgoNeRF.py:415-426."""
        for i in range(3):
            m0, m1 = MAT_MODE[i]
            plane_coef[i] = self.coordinates.up_sampling_VM(plane_coef[i].data, res_target=res_target, ids=[m1, m0])
            line_coef[i] = self.coordinates.up_sampling_VM(line_coef[i].data, res_target=res_target, ids=[VEC_MODE[i]])
        return plane_coef, line_coef

    @torch.no_grad()
    def upsample_volume_grid(self, res_target):
        """EgoNeRF.py:428-435.  The caller then calls coordinates.set_resolution(res_target) (train.py:376-377; note that
        call resets r0 to 0.05 unless r0 is passed) and rebuilds the optimiser."""
        for g in ("yin", "yang"):   # the reference's order: app yin, density yin, app yang, density yang (tables replaced in their lists)
            for kind in ("app", "density"):
                self.up_sampling_VM(getattr(self, f"{kind}_plane_{g}"), getattr(self, f"{kind}_line_{g}"), res_target)
        field_tables.recarve(self, "app", keep_parameters=False)
        field_tables.recarve(self, "density", keep_parameters=False)
        self.update_stepSize(res_target)
        self.invalidate_scene()
        print(f"upsamping to {res_target}")

    @torch.no_grad()
    @_lib.device_guard
    def update_coarse_sigma_grid(self):
        """2x average-pooled density tables (EgoNeRF.py:124-133), kept channel-last."""
        if self.coarse_sigma_grid_update_rule != "conv":
            raise NotImplementedError
        st = _lib.stream_handle()
        srcs = field_tables.tables(self, "density")
        for src in srcs:
            _require_cuda(src, "update_coarse_sigma_grid")
        shapes = [(src.shape[1], src.shape[2] // 2, 1 if src.shape[3] == 1 else src.shape[3] // 2) for src in srcs]
        # The pooled tables are refreshed IN PLACE while their shapes stand (every training step, train.py:356-357): no allocation
        # per step, the scene struct stays valid, and a captured hipGraph of the iteration reads on replay k + 1 what replay k wrote
        # (freshly allocated tables would be invisible to the already captured forward) ...
        cur = field_tables.tables(self, "density", coarse=True)
        same = all(c is not None and c.device == src.device and tuple(c.shape) == (1, *shape) for c, shape, src in zip(cur, shapes, srcs))
        # ... and only while they still form ONE carved buffer: a caller may have assigned coarse_sigma_* one by one (separate
        # allocations have no bounded distance, and the march addresses a tap as base + 32-bit offset: ADVICE r03)
        same = same and field_tables.is_compact(cur) and all(c.dtype == torch.float32 and c.permute(0, 2, 3, 1).is_contiguous() for c in cur)
        if not same:
            field_tables.assign(self, "density", field_tables.carve_channel_last(shapes, srcs[0].device), coarse=True)
            self.invalidate_scene()
        # all 12 tables in one launch (this runs after every training step, train.py:356-357)
        fs, fd = _lib.VmField(), _lib.VmField()
        self._fill_field(fs, "density")
        self._fill_field(fd, "density", coarse=True)
        _call("ego_avgpool_field", C.byref(fs), C.byref(fd), st)
        self._coarse_epoch = getattr(self, "_coarse_epoch", 0) + 1

    @property
    def is_tuned_shape(self) -> bool:
        """True for the model shape every shipped config resolves to (head_is_tuned AND 16 density components): the MFMA / team-gather
        kernels end to end, forward and backward.  Any other shape opt.py:87-100 can produce (n_lamb_sigma / n_lamb_sh multiples of 4
        up to 48, data_dim_color <= 32, featureC 64 | 128, view_pe / fea_pe <= 8, shadingMode 'MLP' / 'RGB') renders and trains through
        the fp32 compatibility kernels for the part that differs: same results to fp32 rounding, 13-32 x slower (tools/generic_timing.py:
        8.8-21 ms against 0.67 ms per 4096 x 512 inference step, 89-167 ms against 6.4 ms per 8192-ray training step)."""
        return self.head_is_tuned and self.density_n_comp[0] == 16

    @property
    def head_is_tuned(self) -> bool:
        """The appearance head alone (= the C library's ego_shape_is_tuned): MLP_Fea 150 -> 128 -> 128 -> 3 on 48 components / app_dim 27
        with view_pe = fea_pe = 2 shades, and trains, through the MFMA kernels whatever the density field's component count (16 takes the
        tuned march / density scatter, any other multiple of 4 the compatibility march around the same shade kernels)."""
        return (self.shadingMode, self.app_dim, self.app_n_comp[0], self.featureC, self.view_pe, self.fea_pe) == ("MLP_Fea", 27, 48, 128, 2, 2)

    @property
    def mlp_precision(self) -> str:
        """Arithmetic of the basis/MLP products:
        "f16f6" (default): layers 1 and 2 with the main term in fp16 and the two correction terms on the fp6 (e2m3) path of the
                 block-scaled MFMA, per-lane block scales taken from the activations at run time; composited max |d RGB| ~1.7e-5
                 (bar: 1e-4); inference only — a differentiable call uses "f16x3";
        "f16f8": the same split with both correction terms in one block-scaled fp8 (e4m3, fixed scales) MFMA per pair of k-steps
                 (round 2's default; 3-4 % slower shade kernel, saturates above 448);
        "f16x3": three fp16 MFMAs per product, fp32-grade (2e-7);
        "f32":   fp32-input MFMA, bit-for-bit fp32 FMA chains (2.8x slower)."""
        return self._mlp_precision

    @mlp_precision.setter
    def mlp_precision(self, value: str):
        if value not in ("f16x3", "f16f8", "f16f6", "f32"):
            raise ValueError("mlp_precision must be 'f16x3', 'f16f8', 'f16f6' or 'f32'")
        self._mlp_precision = value
        self.invalidate_scene()

    @torch.no_grad()
    def check_mlp_precision(self, rays: torch.Tensor, **forward_kw) -> dict:
        """Renders `rays` with the current arithmetic and with the fp32-grade "f16x3" one and returns the largest colour
        difference.  "f16f8" is 2^-16-relative per product: its error scales with the magnitudes inside the MLP (1.4e-5 composited
        on the bench scene, 2e-5 per sample at nn.Linear-default x 3 weights, 3e-3 per sample when the logits reach +-50), so a
        trained checkpoint should be checked once on a few thousand rays and switched to "f16x3" if this exceeds its budget."""
        keep = self._mlp_precision
        try:
            got = self.forward(rays, **forward_kw)[0]
            self.mlp_precision = "f16x3"
            ref = self.forward(rays, **forward_kw)[0]
        finally:
            self.mlp_precision = keep
        d = (got - ref).abs()
        return dict(mlp_precision=keep, max_abs_rgb_diff_vs_f16x3=float(d.max()) if d.numel() else 0.0,
                    mean_abs_rgb_diff_vs_f16x3=float(d.mean()) if d.numel() else 0.0, rays=int(rays.shape[0]))

    @property
    def app_table_dtype(self) -> str:
        """Storage of the appearance tables the inference gather reads: "f32" (the parameters themselves) or "f16" (a
        half-precision shadow copy, refreshed when the parameters change; interpolation stays fp32).  Training always
        uses the fp32 tables."""
        return self._app_table_dtype

    @app_table_dtype.setter
    def app_table_dtype(self, value: str):
        if value not in ("f32", "f16"):
            raise ValueError("app_table_dtype must be 'f32' or 'f16'")
        self._app_table_dtype = value
        self.invalidate_scene()

    # -- C-ABI scene ----------------------------------------------------------------------------------------
    def _mlp_tensors(self) -> List[torch.Tensor]:
        if self.shadingMode == "RGB":   # no network: the packed blob holds the two basis matrices only
            return [self.basis_mat_yin.weight, self.basis_mat_yang.weight]
        m = self.renderModule.mlp
        return [m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias, self.basis_mat_yin.weight,
                self.basis_mat_yang.weight]

    def _fill_field(self, f: "_lib.VmField", kind: str, coarse=False, tensors=None):
        """One ego_vm_field: the tables of `kind` (coarse: the 2x pooled ones at half the resolution), or `tensors` in their place."""
        n_comp = self.density_n_comp if kind == "density" else self.app_n_comp
        if len(set(n_comp)) != 1:
            raise NotImplementedError("per-plane component counts must be equal (true for every shipped config)")
        f.n_comp = n_comp[0]
        f.res[:] = [int(v) // 2 if coarse else int(v) for v in self.gridSize.tolist()]
        field_tables.fill_pointers(f, field_tables.tables(self, kind, coarse) if tensors is None else tensors)

    def invalidate_scene(self, moved: bool = False) -> None:
        """The next scene() call builds the struct anew.  The per-mode packed blobs, the half tables and the baked density / appearance grids stay (an
        earlier struct or a captured graph may point into them; reused while device, size and table versions stand) unless the whole
        model `moved` (Module._apply)."""
        self._scene = _SceneEntry() if moved else self._scene.successor()

    def packed_blob(self, training: bool = False) -> Optional[torch.Tensor]:
        """The packed MLP / basis image of a mode as of the last scene(training) call (None before the first)."""
        return self._scene.blobs.get(bool(training))

    def _luts(self, dev) -> List[torch.Tensor]:
        co = self.coordinates
        return [co.lut_device(dev, 2)] + ([] if co.interval_th else [co.lut_device(dev, None)])

    def _dense_wanted(self) -> bool:
        """The dense density route is asked for (attribute, EGO_DENSE_DENSITY) and the model is one it serves: the tuned shape (16
        density components and the tuned head, every shipped config).  The any-shape kernels keep the factored march: their eval
        results are pinned bit for bit to a recorded build (tests/test_hip_shape_corners.py)."""
        env = os.environ.get("EGO_DENSE_DENSITY", "")
        on = bool(self.dense_density) if env == "" else env != "0"
        return on and tuple(self.density_n_comp) == (16, 16, 16) and self.is_tuned_shape

    def _app_dense_wanted(self) -> bool:
        """The dense appearance route is asked for (attribute, EGO_DENSE_APP) and the model and its settings are ones it serves: the
        tuned shape, fp32 appearance tables and a split arithmetic (the fp32-MFMA kernel and the half tables keep the factored gather)."""
        env = os.environ.get("EGO_DENSE_APP", "")
        on = bool(self.dense_appearance) if env == "" else env != "0"
        return on and self.is_tuned_shape and self._app_table_dtype == "f32" and self._mlp_precision != "f32"

    def _app_dense_versions(self) -> tuple:
        """What the baked feature grid is a function of: the (address, version) pairs of the twelve appearance tables and of both
        basis matrices."""
        src = field_tables.tables(self, "app") + [self.basis_mat_yin.weight, self.basis_mat_yang.weight]
        return tuple((t.data_ptr(), t._version) for t in src)

    @staticmethod
    def _app_dense_cap_bytes() -> float:
        raw = os.environ.get("EGO_DENSE_APP_MAX_MB", "")
        try:
            return float(raw or 4096) * 2 ** 20
        except ValueError:
            raise ValueError(f"EGO_DENSE_APP_MAX_MB must be a number of megabytes, not {raw!r}") from None

    @staticmethod
    def _app_dense_fits(nbytes: int, cap: float, fresh: int, free: int) -> bool:
        """The size gates of the dense appearance route: the grid within the cap and under the 4 GiB that 32-bit byte offsets address,
        and what has to be allocated for it (`fresh`; 0 when a buffer of that size is held) within a quarter of the free device memory."""
        return nbytes <= cap and nbytes < 2 ** 32 and (not fresh or fresh <= free // 4)

    def _dense_versions(self, coarse: bool) -> tuple:
        """What a baked node grid is a function of: the (address, version) pairs of the field's 12 tables.  The pooled tables are also
        rewritten in place behind torch's version counters: by update_coarse_sigma_grid(), which _coarse_epoch counts, and by a
        replayed GraphedTrainStep that captured it, where no Python runs at all - but such a replay has stepped the full tables, whose
        versions GraphedTrainStep bumps.  So the pooled grid's key holds the full field's pairs too: it is baked again (0.06 ms at
        [75, 86, 258]) whenever the full grid is."""
        pairs = lambda c: tuple((t.data_ptr(), t._version) for t in field_tables.tables(self, "density", c))
        return pairs(True) + (self._coarse_epoch,) + pairs(False) if coarse else pairs(False)

    @staticmethod
    def _dense_cap_bytes() -> float:
        raw = os.environ.get("EGO_DENSE_DENSITY_MAX_MB", "")
        try:
            return float(raw or 1024) * 2 ** 20
        except ValueError:
            raise ValueError(f"EGO_DENSE_DENSITY_MAX_MB must be a number of megabytes, not {raw!r}") from None

    def _scene_key(self, training: bool) -> tuple:
        """Everything the struct is a function of, as one tuple; no device work (the coordinates cache their LUTs).  Addresses stand for
        allocations, (address, version) pairs for what is copied or packed at build time: the MLP / basis weights, the appearance
        tables while their half copy is in use, and the density tables (full and pooled) while the dense route is asked for, with the
        switch and its cap.  id(alphaMask) is sound because the entry holds that mask: no other object can get its id."""
        co = self.coordinates
        copied = self._mlp_tensors() + (field_tables.tables(self, "app") if self._app_table_dtype == "f16" else [])
        dense = ()
        if not training and self._dense_wanted():
            has_coarse = self.coarse_sigma_plane_yin[0] is not None
            dense = (os.environ.get("EGO_DENSE_DENSITY_MAX_MB", ""), self._dense_versions(False),
                     self._dense_versions(True) if has_coarse else None)
        app_dense = ()
        if not training and self._app_dense_wanted():
            app_dense = (os.environ.get("EGO_DENSE_APP_MAX_MB", ""), self._app_dense_versions())
        return (tuple(p.data_ptr() for p in self.parameters()), tuple((t.data_ptr(), t._version) for t in copied),
                None if self.envmap is None else self.envmap.emission.data_ptr(), self.use_alpha_mask, id(self.alphaMask),
                float(self.early_termination_eps), float(self.rayMarch_weight_thres) if self.use_weight_thres else None,
                bool(self.skip_zero_weight_tiles), co.N_r, float(co.r0), float(co.far[0]), tuple(co.center.tolist()),
                tuple(t.data_ptr() for t in self._luts(self.density_plane_yin[0].device)), float(self.distance_scale),
                float(self.density_shift), self.fea2denseAct, self._mlp_precision, self._app_table_dtype, bool(training), dense, app_dense)

    @_lib.device_guard
    def scene(self, training: bool = False) -> "_lib.Scene":
        """The ego_scene struct for the current parameters (re-packs the MFMA weights when they changed).

        training=True is what the differentiable path asks for (train.RenderFunction, forward and backward): the fp32 tables, every
        sample shaded like EgoNeRF.forward (the appearance skip is an inference option), all three fp16 terms of every product
        (mlp_precision "f16x3"), and only the regions of the packed blob that arithmetic reads (ego_pack_mlp_for).

        The struct holds raw device pointers: to the parameter tables (optimiser steps write them in place), and to the pooled density
        tables, which `update_coarse_sigma_grid()` also refreshes IN PLACE while their shapes stand - so a struct returned earlier, or a
        captured hipGraph that embeds it, reads the refreshed values (what GraphedTrainStep relies on).  The packed MLP / basis images
        are different: a SNAPSHOT taken by this call, one blob per mode (training / inference) - a struct returned earlier keeps reading
        the weights as of its own pack (a captured graph that contains the pack kernel re-packs on every replay); call scene() again
        after the weights changed.  The baked node grids of the density fields (`dense_density`, inference structs only: density_dense
        and density_coarse_dense, which ego_march_density then reads INSTEAD of the density tables) are SNAPSHOTS too: baked by this call
        from the tables - the pooled ones as update_coarse_sigma_grid() last left them - and baked again by the next scene() call after
        a density table changed in place or the pooled tables were refreshed; a holder of an older struct, or a captured graph that
        embeds one, marches the field as last baked until scene() is called again (the bake rewrites the SAME buffers, so that call is
        all it takes).  The buffers stay allocated until the model moves or the grid changes size (_fill_dense), whatever struct is
        cached meanwhile.  A training struct never carries them.  The baked grid of the appearance features (`dense_appearance`: app_dense,
        which the inference shade kernels then read INSTEAD of the appearance tables and the basis) follows the same rules, keyed by the twelve
        appearance tables and both basis_mat weights (_fill_app_dense).  A holder that needs a frozen snapshot must copy the tables; re-allocation (another shape / device,
        tables assigned one by one) invalidates the cached struct and the next scene() call builds a new one.  One struct is cached
        (not one per mode), together with everything it points to that nobody else keeps alive (_SceneEntry)."""
        dev = self.density_plane_yin[0].device
        if dev.type != "cuda":
            raise RuntimeError(f"model parameters are on {dev}; the EgoNeRF hot path runs only on the HIP device")
        if self._scene.key != self._scene_key(training):
            self._scene = self._build_scene(training, dev)
        return self._scene.struct

    def _build_scene(self, training: bool, dev) -> "_SceneEntry":
        # Tables assigned one by one, e.g. by load_state_dict(assign=True) (.to() / .cuda() / .float() are handled in _apply), go back
        # into one buffer first.  A hit needs no such check: its key holds the addresses the tables had when they were checked here.
        for kind in ("density", "app"):
            if not field_tables.is_compact(field_tables.tables(self, kind)):
                field_tables.recarve(self, kind, keep_parameters=True)
        entry = self._scene.successor()
        sc = entry.struct = _lib.new_scene()
        entry.luts = self._luts(dev)
        self.coordinates.fill_scene(sc, dev)
        sc.act_softplus = int(self.fea2denseAct == "softplus")
        sc.density_shift, sc.distance_scale = float(self.density_shift), float(self.distance_scale)
        self._fill_field(sc.density, "density")
        self._fill_field(sc.app, "app")
        if self.coarse_sigma_plane_yin[0] is not None:
            self._fill_field(sc.density_coarse, "density", coarse=True)
        self._fill_head(sc, entry, training)
        self._pack_head(sc, entry, training, dev)
        if self._app_table_dtype == "f16" and not training:
            self._fill_app16(sc, entry)
        if not training and self._dense_wanted():
            self._fill_dense(sc, entry, dev)   # (otherwise the pointers stay NULL; grids baked earlier stay allocated, see _fill_dense)
        if not training and self._app_dense_wanted():
            self._fill_app_dense(sc, entry, dev)
        entry.mask = self.alphaMask
        if self.use_alpha_mask and self.alphaMask is not None:
            self.alphaMask.fill_scene(sc)
        sc.term_eps = float(self.early_termination_eps)
        sc.weight_thres = float(self.rayMarch_weight_thres) if self.use_weight_thres else (0.0 if self.skip_zero_weight_tiles else -1.0)
        if training:
            sc.weight_thres = -1.0
        if self.envmap is not None:
            em = self.envmap.emission.detach()
            if not em.is_contiguous():
                raise RuntimeError("envmap.emission must be contiguous [3][2h][h]")
            sc.envmap, sc.envmap_h = em.data_ptr(), em.shape[2]
        entry.key = self._scene_key(training)
        return entry

    def _fill_head(self, sc, entry, training: bool):
        holds = entry.holds = [t.detach().contiguous() for t in self._mlp_tensors()]
        if self.shadingMode == "RGB":
            sc.head = 1   # EGO_HEAD_RGB: mlp_w / mlp_b stay null, mlp_in = mlp_hidden = 0
        else:
            sc.mlp_w[:] = [holds[0].data_ptr(), holds[2].data_ptr(), holds[4].data_ptr()]
            sc.mlp_b[:] = [holds[1].data_ptr(), holds[3].data_ptr(), holds[5].data_ptr()]
        sc.basis[:] = [holds[-2].data_ptr(), holds[-1].data_ptr()]
        sc.app_dim = self.app_dim
        sc.mlp_in, sc.mlp_hidden = self.head_in_mlpC, self.head_hidden
        sc.view_pe, sc.fea_pe = (self.view_pe, self.head_fea_pe) if self.shadingMode != "RGB" else (0, 0)
        sc.mlp_precision = 0 if training else {"f16x3": 0, "f32": 1, "f16f8": 2, "f16f6": 3}[self._mlp_precision]

    def _pack_head(self, sc, entry, training: bool, dev):
        """Packed weights: the MFMA fragment layouts for the tuned shape (27 / 48 / 150 / 128 / 2 / 2, every shipped config), the fp32
        layout of the any-shape compatibility kernels otherwise (csrc/ego_generic.hip; the library reports the size for the shape).  One
        blob per mode: a training pack writes only the regions the f16x3 training kernels read, so it must never land in the
        blob an earlier INFERENCE struct (or a captured preview-render graph) points to: stale fp8 / fp6 correction terms under fresh fp16."""
        need = _lib.load().ego_packed_floats_scene(C.byref(sc))
        if need <= 0:
            raise RuntimeError("ego_packed_floats_scene rejected the scene")
        blob = entry.blobs.get(bool(training))
        if blob is None or blob.device != dev or blob.numel() != need:
            blob = entry.blobs[bool(training)] = torch.zeros(need, device=dev)
        _call("ego_pack_mlp_for", sc, blob.data_ptr(), int(training), _lib.stream_handle())
        sc.packed = blob.data_ptr()

    def _fill_app16(self, sc, entry):
        tabs = field_tables.tables(self, "app")
        ver = tuple((t.data_ptr(), t._version) for t in tabs)
        if entry.app16 is None or entry.app16[0] != ver:
            # [1,H,W,C] channel-last memory of the (1,C,H,W) parameters as halves (a cast, done when weights change), in one buffer
            halves = field_tables.carve_channel_last(field_tables.shapes_of(tabs), tabs[0].device, torch.float16)
            for hv, t in zip(halves, tabs):
                hv.copy_(t.detach())
            entry.app16 = (ver, halves)
        self._fill_field(sc.app16, "app", tensors=entry.app16[1])
        sc.app_f16 = _lib.APP_HALF

    def _fill_dense(self, sc, entry, dev):
        """The baked node grids behind density_dense / density_coarse_dense (ego_bake_density_dense), decided once per scene build:
        baked while the full field's grid is at most EGO_DENSE_DENSITY_MAX_MB (default 1024; 32-bit offsets need it under 4 GB in
        any case) and what has to be allocated is at most a quarter of the free device memory; otherwise the pointers stay NULL and
        the march gathers from the tables as before.  A grid is kept across rebuilds and baked again, IN PLACE, when its field's versions
        changed.  Lifetime: like the packed blobs and the half tables, a grid stays allocated while the model stays on its device and the
        grid keeps its size - also while a training struct is the cached one, or the switch or the cap has turned the route off - because
        an inference struct handed out earlier, or a captured graph (FrameRenderer(graph=True)), may still point into it.  It is
        released only when the model moves (Module._apply) or when a grid of another size replaces it (upsample_volume_grid: the
        holders of older structs must re-create them then anyway)."""
        res = [int(v) for v in self.gridSize.tolist()]
        has_coarse = self.coarse_sigma_plane_yin[0] is not None
        plan = [("full", False, 32 * res[0] * res[1] * res[2])]
        if has_coarse:
            plan.append(("coarse", True, 32 * (res[0] // 2) * (res[1] // 2) * (res[2] // 2)))
        cap = self._dense_cap_bytes()
        held = entry.dense if entry.dense is not None else {}
        fits = lambda h, nbytes: h is not None and h[1].device == dev and h[1].numel() * 4 == nbytes
        fresh = sum(nbytes for name, _, nbytes in plan if not fits(held.get(name), nbytes))
        if plan[0][2] > cap or plan[0][2] >= 2 ** 32 or (fresh and fresh > torch.cuda.mem_get_info(dev)[0] // 4):
            return   # pointers stay NULL; what is held stays held
        dense = dict(held)
        for name, coarse, nbytes in plan:
            h = held.get(name)
            if not fits(h, nbytes):
                h = (None, torch.empty(nbytes // 4, device=dev))
            ver = self._dense_versions(coarse)
            if h[0] != ver:
                f = _lib.VmField()
                self._fill_field(f, "density", coarse=coarse)
                _call("ego_bake_density_dense", C.byref(f), h[1].data_ptr(), _lib.stream_handle())
                h = (ver, h[1])
            dense[name] = h
        entry.dense = dense
        sc.density_dense = dense["full"][1].data_ptr()
        if has_coarse:
            sc.density_coarse_dense = dense["coarse"][1].data_ptr()

    def _fill_app_dense(self, sc, entry, dev):
        """The baked node grid of the appearance features behind app_dense (ego_bake_app_dense), decided once per scene build by
        _fill_dense's rules: baked while the grid fits EGO_DENSE_APP_MAX_MB (default 4096), 32-bit byte offsets and - where it has to
        be allocated - a quarter of the free device memory; otherwise the pointer stays NULL and the shade gathers from the tables.
        The grid is kept across rebuilds and baked again, IN PLACE, when an appearance table or a basis matrix changed; it stays allocated
        until the model moves or the grid changes size, because an inference struct handed out earlier, or a captured graph, may still
        point into it.  `last_app_bake_ms` records the time of the latest bake (None before the first)."""
        res = [int(v) for v in self.gridSize.tolist()]
        nbytes = 2 * 128 * res[0] * res[1] * res[2]
        h = entry.app_dense
        held = h is not None and h[1].device == dev and h[1].numel() * 4 == nbytes
        fresh = 0 if held else nbytes
        if not self._app_dense_fits(nbytes, self._app_dense_cap_bytes(), fresh, torch.cuda.mem_get_info(dev)[0] if fresh else 0):
            return   # pointer stays NULL; what is held stays held
        if not held:
            h = (None, torch.empty(nbytes // 4, device=dev))
        ver = self._app_dense_versions()
        if h[0] != ver:
            f = _lib.VmField()
            self._fill_field(f, "app")
            timed = not torch.cuda.is_current_stream_capturing()
            if timed:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
            _call("ego_bake_app_dense", C.byref(f), sc.basis[0], sc.basis[1], int(self.app_dim), h[1].data_ptr(), _lib.stream_handle())
            if timed:
                t1.record()
                self._app_bake_events = (t0, t1)
            h = (ver, h[1])
        entry.app_dense = h
        sc.app_dense = h[1].data_ptr()

    @property
    def last_app_bake_ms(self) -> Optional[float]:
        """Device time of the latest bake of the dense appearance grid in ms (waits for it), or None if none was timed."""
        ev = getattr(self, "_app_bake_events", None)
        if ev is None:
            return None
        ev[1].synchronize()
        return float(ev[0].elapsed_time(ev[1]))

    # -- stage methods (reference public API) ----------------------------------------------------------------
    def _sched(self, n_samples: int, device) -> torch.Tensor:
        near, far = self.near_far
        key = (n_samples, str(device), float(self.coordinates.r0), float(near), float(far),
               bool(self.coordinates.interval_th))  # set_resolution() may move r0 (coordinates.py:214)
        if key not in self._sched_cache:
            self._sched_cache[key] = self.coordinates.sample_schedule(near, far, n_samples).to(device)
        return self._sched_cache[key]

    def sample_ray_z(self, rays: torch.Tensor, n_samples: int, jitter: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Distances of TensorBase.sample_ray (tensorBase.py:308-327): aabb entry clamped to [near, far] + stepSize * (k [+ U])."""
        o, d = rays[:, :3], rays[:, 3:6]
        near, far = self.near_far
        aabb = self.aabb.to(rays.device, torch.float32)
        vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
        t_min = torch.minimum((aabb[1] - o) / vec, (aabb[0] - o) / vec).amax(-1).clamp(min=near, max=far)
        rng = torch.arange(n_samples, device=rays.device)[None].float()
        if jitter is not None:
            rng = rng.repeat(rays.shape[0], 1) + jitter.to(rays.device, torch.float32)
        step = self.stepSize.to(rays.device, torch.float32) if torch.is_tensor(self.stepSize) else float(self.stepSize)
        z = t_min[:, None] + step * rng
        return z.expand(rays.shape[0], n_samples).contiguous()

    def sample_ray(self, rays_o, rays_d, is_train=True, N_samples=-1, jitter: Optional[torch.Tensor] = None):
        """tensorBase.py:308-327 -> (rays_pts [N,S,3], interpx [N,S], inside-aabb mask [N,S])."""
        N_samples = N_samples if N_samples > 0 else self.nSamples
        if is_train and jitter is None:
            jitter = torch.rand(rays_o.shape[0], N_samples)
        z = self.sample_ray_z(torch.cat([rays_o, rays_d], -1).float(), N_samples, jitter if is_train else None)
        pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., None]
        aabb = self.aabb.to(pts.device)
        return pts, z, ~((aabb[0] > pts) | (pts > aabb[1])).any(dim=-1)

    def _plain_exp_train_z(self, n: int, jitter: torch.Tensor) -> torch.Tensor:
        """Plain exponential schedule in training (EgoNeRF.py:59-67): the noise goes into the exponent and the distances are an
        exclusive prefix sum; the reference's own expression, handed to the kernels as explicit distances [N, n]."""
        near, far = float(self.near_far[0]), float(self.near_far[1])
        ratio = 1 + (math.pi / 2.0) / n
        r0 = (far - near) * (ratio - 1) / (pow(ratio, n) - 1)
        rng = torch.arange(n, device=jitter.device)[None].float() + _f32c(jitter)
        tri = torch.tril(torch.ones(n, n, device=jitter.device), diagonal=-1).T
        return (near + torch.pow(ratio, rng) @ tri * r0).contiguous()

    @_lib.device_guard
    def sample_ray_exp(self, rays_o, rays_d, is_train=True, N_samples=-1, jitter: Optional[torch.Tensor] = None):
        """EgoNeRF.py:56-87 -> (rays_pts [N,S,3], interpx [N,S], ~mask_outbbox [N,S]).  `jitter` [N,S] pins the
        training noise (the reference draws it with torch.rand_like on the CPU generator)."""
        _require_cuda(rays_o, "sample_ray_exp")
        self.coordinates._require_supported()
        N, S = rays_d.shape[-2], N_samples
        rays = torch.cat([_f32c(rays_o), _f32c(rays_d)], -1).contiguous()
        if is_train and jitter is None:
            jitter = torch.rand(N, S).to(rays.device)
        jit = _f32c(jitter) if is_train else None
        if is_train and not self.coordinates.interval_th:
            z = self._plain_exp_train_z(S, jit.to(rays.device))
            xyz = rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]
        else:
            xyz = torch.empty(N, S, 3, device=rays.device)
            z = torch.empty(N, S, device=rays.device)
            _call("ego_sample_ray_exp", rays.data_ptr(), self._sched(S, rays.device).data_ptr(), _lib.ptr(jit),
                  float(self.near_far[0]), N, S, xyz.data_ptr(), z.data_ptr(), _lib.stream_handle())
        aabb = self.aabb.to(rays.device)
        mask_outbbox = ((aabb[0] > xyz) | (xyz > aabb[1])).any(dim=-1)
        return xyz, z, ~mask_outbbox

    @_lib.device_guard
    def _density(self, coords_sampled, coarse: int):
        params = field_tables.tables(self, "density")
        if stage_autograd.needs_grad(*params):
            return stage_autograd.DensityFeatureFunction.apply(self, coarse, coords_sampled.detach(), *params)
        return self._density_forward(coords_sampled, coarse)

    def _density_forward(self, coords_sampled, coarse: int):
        _require_cuda(coords_sampled, "compute_densityfeature")
        _last_dim(coords_sampled, 7, "compute_densityfeature")
        c = _f32c(coords_sampled)
        out = torch.empty(c.shape[:-1], device=c.device)
        _call("ego_density_feature", self.scene(), c.data_ptr(), c.numel() // 7, coarse, out.data_ptr(), _lib.stream_handle())
        return out

    def compute_densityfeature(self, coords_sampled):
        """EgoNeRF.py:291-347: [...,7] normalised coords -> [...].  Differentiable to the 12 density tables when grad mode is on and one of
        them requires grad (stage_autograd.DensityFeatureFunction): same forward bits, fp32-grade backward (grid_sample + relu), bit-
        reproducible for the shipped 16-component shape.  The coordinates receive no gradient (the reference detaches them)."""
        return self._density(coords_sampled, 0)

    def compute_coarse_densityfeature(self, coords_sampled, coarse_sigma_grid_update_rule="conv"):
        """EgoNeRF.py:232-289.  Values from the last update_coarse_sigma_grid() snapshot; differentiable to the full-resolution density
        tables through the 2x average pooling of EgoNeRF.py:124-133, like compute_densityfeature."""
        return self._density(coords_sampled, 1)

    @_lib.device_guard
    def compute_appfeature(self, coords_sampled):
        """EgoNeRF.py:349-413: [...,7] -> [..., app_dim].  Differentiable to the 12 appearance tables and basis_mat_{yin,yang}.weight when
        grad mode is on and one of them requires grad (stage_autograd.AppFeatureFunction): same forward bits (whatever app_table_dtype),
        fp32-grade backward at the fp32 tables, bit-reproducible for the shipped 48-component shape."""
        params = field_tables.tables(self, "app") + [self.basis_mat_yin.weight, self.basis_mat_yang.weight]
        if stage_autograd.needs_grad(*params):
            return stage_autograd.AppFeatureFunction.apply(self, coords_sampled.detach(), *params)
        return self._app_forward(coords_sampled)

    def _app_forward(self, coords_sampled):
        _require_cuda(coords_sampled, "compute_appfeature")
        _last_dim(coords_sampled, 7, "compute_appfeature")
        c = _f32c(coords_sampled)
        out = torch.empty(*c.shape[:-1], self.app_dim, device=c.device)
        _call("ego_app_feature", self.scene(), c.data_ptr(), c.numel() // 7, out.data_ptr(), _lib.stream_handle())
        return out

    # -- occupancy ------------------------------------------------------------------------------
    @torch.no_grad()
    def compute_alpha(self, norm_locs, length=1):
        """tensorBase.py:421-436: alpha on arbitrary normalised locations, skipping what an existing mask marks empty."""
        sigma = torch.zeros(norm_locs.shape[:-1], device=norm_locs.device)
        if self.alphaMask is not None:
            keep = self.alphaMask.sample_alpha(norm_locs) > 0
        else:
            keep = torch.ones_like(sigma, dtype=torch.bool)
        if bool(keep.any()):
            sigma[keep] = self.feature2density(self.compute_densityfeature(norm_locs[keep]))
        return 1 - torch.exp(-sigma * length)

    @torch.no_grad()
    def getDenseAlpha(self, gridSize=None):
        """EgoNeRF.py:437-465: alpha on the grid lattice of both grids, step length = stepSize (no distance_scale)."""
        g = self.gridSize.tolist() if gridSize is None else list(gridSize)
        dev = self.density_plane_yin[0].device
        lin = [torch.linspace(0, 1, n) for n in g]
        norm = (torch.stack(torch.meshgrid(*lin, indexing="ij"), -1) * 2 - 1).to(dev)
        zeros3, flag = torch.zeros_like(norm), torch.zeros_like(norm[..., :1])
        yin = torch.cat([norm, zeros3, flag], -1).view(-1, 7)
        yang = torch.cat([zeros3, norm, flag + 1], -1).view(-1, 7)
        step = float(self.stepSize)
        return self.compute_alpha(yin, step).view(g), self.compute_alpha(yang, step).view(g)

    @torch.no_grad()
    def updateAlphaMask(self, gridSize=None):
        """EgoNeRF.py:467-489: clamp, 3x3x3 max-pool, threshold at alphaMask_thres -> YinYangAlphaGridMask.  Building the
        mask does not switch it on: set `use_alpha_mask = True` to apply it."""
        g = self.gridSize.tolist() if gridSize is None else list(gridSize)
        vols = []
        for a in self.getDenseAlpha(g):
            a = a.clamp(0, 1).transpose(0, 2).contiguous()[None, None]
            a = torch.nn.functional.max_pool3d(a, kernel_size=3, padding=1, stride=1).view(g[::-1])
            vols.append((a >= self.alphaMask_thres).float())
        self.alphaMask = YinYangAlphaGridMask(self.device, vols[0], vols[1])
        self.invalidate_scene()
        return float((vols[0].sum() + vols[1].sum()) / (2 * g[0] * g[1] * g[2]))

    # -- the hot path -------------------------------------------------------------------------------------------
    @_lib.device_guard
    def forward(self, rays_chunk, white_bg=True, is_train=False, ndc_ray=False, n_coarse=-1, n_fine=0, exp_sampling=False,
                pretrain_envmap=False, pivotal_sample_th=0.0, resampling=False, use_coarse_sample=True, interval_th=False,
                jitter: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None, need_alpha: bool = True,
                marched_event: Optional["torch.cuda.Event"] = None):
        """EgoNeRF.forward (EgoNeRF.py:491-602) -> (rgb_map [N,3], depth_map [N], bg_map|None, env_map|None,
        alpha [N, S(+1)]).  `white_bg`, `pivotal_sample_th`, `interval_th` are accepted and unused, as in the
        reference.  `jitter` [N,n_coarse] / `u` [N,n_fine] pin the is_train noise.  `need_alpha=False` (eval only; what
        `volume_renderer(keep_alpha=False)` passes) returns None for the per-sample alpha, which also lets the ray march stop
        evaluating a ray once its transmittance is exactly 0 (the remaining weights are exactly 0 either way).  `marched_event` (a created
        torch.cuda.Event; volume_renderer's host hand-over passes it): recorded on the current stream behind the call's last march, ahead
        of its shade kernel (ego_render_args.marched) - or at the end of a call that takes another path.  A call that passes it keeps
        march and shade two launches where it would otherwise render in one (ego_render_forward_marches)."""
        self._last_render = self._last_shaded = None   # set again by a call that runs ego_render_forward
        _require_cuda(rays_chunk, "EgoNeRF.forward")
        if rays_chunk.dim() != 2 or rays_chunk.shape[1] < 6:
            raise IndexError(f"EgoNeRF.forward: rays_chunk must be [N, >=6] (origin, direction), got {tuple(rays_chunk.shape)}")
        marched = False   # whether the library was handed `marched_event`
        if pretrain_envmap:
            out = self.envmap.get_radiance(rays_chunk[:, 3:6])
        elif ndc_ray:
            raise NotImplementedError  # EgoNeRF.py:503-504
        else:
            rays = _f32c(rays_chunk[:, :6])
            # d loss / d rays: defined where the sample distances do not depend on the ray; refused before any launch elsewhere
            ray_grads = torch.is_grad_enabled() and rays.requires_grad
            if ray_grads and not exp_sampling and not is_train:
                raise NotImplementedError("ray gradients are not defined on the eval-mode path that measures every ray with ray 0's distances "
                                          "(exp_sampling=False, is_train=False); render with exp_sampling=True")
            if ray_grads and not exp_sampling:
                raise NotImplementedError("ray gradients need exp_sampling=True: with explicit z_coarse (TensorBase.sample_ray) the sample "
                                          "distances depend on the ray, and z is a constant of the ray gradient")
            if ray_grads and not self.coordinates.interval_th:
                raise NotImplementedError("ray gradients need the linearised exponential grid (interval_th=True): the plain exponential grid "
                                          "normalises r through a truncated logarithm, whose cell the ray-gradient kernel does not re-derive")
            z_coarse, jitter, u = self._noise_plan(rays, n_coarse, n_fine, is_train, exp_sampling, resampling, jitter, u)
            if not is_train and z_coarse is not None and rays.shape[0] and not bool((z_coarse[:, 0] == z_coarse[0, 0]).all()):
                # rays that enter the aabb at different distances: the reference places the first-pass samples per ray but
                # measures every ray with ray 0's distances (EgoNeRF.py:515-516) - evaluated the same way, stage by stage
                out = self._forward_eval_ray0_distances(rays, z_coarse, int(n_coarse), int(n_fine), bool(resampling),
                                                        bool(use_coarse_sample), need_alpha)
            elif ray_grads or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
                # any supported shape trains: the tuned one through the MFMA kernels, the others through the fp32 compatibility kernels
                from .train import render_train  # differentiable path: keeps activations, backward in HIP (egonerf_amd/train.py)
                out = render_train(self, rays, n_coarse, n_fine, resampling, use_coarse_sample, jitter, u, z_coarse)
            else:
                out, marched = self._render_forward(rays, z_coarse, jitter, u, n_coarse, n_fine, resampling, use_coarse_sample, need_alpha,
                                                    marched_event)
        if marched_event is not None and not marched:
            marched_event.record()   # a path without a march of its own (training, envmap pre-training, ...): "marched" = done
        return out

    def _noise_plan(self, rays, n_coarse, n_fine, is_train, exp_sampling, resampling, jitter=None, u=None):
        """Where the first pass samples and with what noise -> (z_coarse | None, jitter | None, u | None) as ego_render_forward and
        train.render_train take them.  Plain torch, no library call: it runs on CPU rays too.
        z_coarse [N, n_coarse]: explicit distances, for TensorBase.sample_ray's per-ray uniform schedule (exp_sampling=False,
        tensorBase.py:308-327; the noise is `rng += rand`) and for the plain exponential schedule in training (EgoNeRF.py:59-67: noise
        in the exponent); otherwise the march follows the model's schedule (_sched) plus `jitter`.
        Noise exists only with is_train; what the caller pins is used and nothing is drawn for it.  Otherwise, in this order: jitter =
        torch.rand(N, n_coarse) from the CPU generator (tensorBase.py:320, EgoNeRF.py:81); a second draw of that shape when the jitter
        went into z_coarse; with resampling, u = torch.rand(N, n_fine) from the generator of the rays' device (ray_utils.py:169)."""
        N, dev = rays.shape[0], rays.device
        if not is_train:
            return (None if exp_sampling else self.sample_ray_z(rays, n_coarse)), None, None
        drawn = jitter is None
        if drawn:
            jitter = torch.rand(N, n_coarse)
        z_coarse = None
        if not exp_sampling:
            z_coarse = self.sample_ray_z(rays, n_coarse, jitter.to(dev))
        elif not self.coordinates.interval_th:
            z_coarse = self._plain_exp_train_z(n_coarse, jitter.to(dev))
        if z_coarse is not None and drawn:
            # With z_coarse given the march never reads `jitter`: these values are never used.  The draw is kept only so that the CPU
            # generator is left in the state it has always been left in (a seeded run draws the same numbers afterwards).
            jitter = torch.rand(N, n_coarse)
        if resampling and u is None:
            u = torch.rand(N, n_fine, device=dev)
        return z_coarse, _f32c(jitter.to(dev)), _f32c(u) if resampling else None

    def _render_forward(self, rays, z_coarse, jitter, u, n_coarse, n_fine, resampling, use_coarse_sample, need_alpha, marched_event):
        """Fills ego_render_args, sizes the workspace and runs ego_render_forward -> (result, whether it took `marched_event`)."""
        N, dev = rays.shape[0], rays.device
        sc = self.scene()
        args = _lib.RenderArgs()
        args.n_coarse, args.n_fine = int(n_coarse), int(n_fine)
        args.resampling, args.use_coarse_sample = int(bool(resampling)), int(bool(use_coarse_sample))
        args.r_sched = self._sched(n_coarse, dev).data_ptr()
        args.near_ = float(self.near_far[0])
        args.z_coarse, args.jitter, args.u = _lib.ptr(z_coarse), _lib.ptr(jitter), _lib.ptr(u)
        marched = marched_event is not None and N > 0
        if marched:
            args.marched = marched_event.cuda_event
        S = _lib.sample_count(n_coarse, n_fine, resampling, use_coarse_sample)
        ws_bytes = _lib.load().ego_render_workspace_bytes(N, C.byref(args))
        if ws_bytes < 0:
            raise RuntimeError("ego_render_workspace_bytes rejected the arguments (n_coarse < 2?)")
        ws = torch.empty(max(ws_bytes, 4) // 4, device=dev)
        has_env = self.envmap is not None
        rgb_map = torch.empty(N, 3, device=dev)
        depth = torch.empty(N, device=dev)
        alpha = torch.empty(N, S + int(has_env), device=dev) if need_alpha else None
        bg_map = torch.empty(N, 3, device=dev) if has_env else None
        env_map = torch.empty(N, 3, device=dev) if has_env else None
        _call("ego_render_forward", sc, C.byref(args), rays.data_ptr(), N, ws.data_ptr(), rgb_map.data_ptr(), depth.data_ptr(),
              _lib.ptr(alpha), _lib.ptr(bg_map), _lib.ptr(env_map), _lib.stream_handle())
        if N:
            self._last_render = (N, args, ws)   # for last_shaded_samples (the workspace holds the live count / tile flags)
        return (rgb_map, depth, bg_map, env_map, alpha), marched

    @property
    def last_shaded_samples(self) -> Optional[torch.Tensor]:
        """How many samples the last forward sent through the appearance lookup and the MLP, as a 0-d int64 device tensor (no host
        synchronisation; ego_render_shaded_samples): the live samples - weight > max(weight_thres, 0), tensorBase.py:480-487's app_mask - on
        the compact path (include/egonerf_hip.h: ego_render_forward_compacts), 32 x the shaded tiles (at most N S) on the tile paths, N S
        without skipping.  None when the last forward did not run ego_render_forward (training, envmap pre-training, the ray-0-distance
        evaluation, N = 0).  Computed on first access from the workspace the forward keeps for it."""
        if self._last_render is None:
            return None
        if self._last_shaded is None:
            N, args, ws = self._last_render
            with torch.cuda.device(ws.device):
                out = torch.empty((), dtype=torch.int64, device=ws.device)
                _call("ego_render_shaded_samples", N, C.byref(args), ws.data_ptr(), out.data_ptr(), _lib.stream_handle())
            self._last_shaded = out
        return self._last_shaded

    def _forward_eval_ray0_distances(self, rays, z_pos, n_coarse, n_fine, resampling, use_coarse_sample, need_alpha):
        """Eval with exp_sampling=False and rays whose aabb entry distances differ (rays starting outside the box).  The reference
        (EgoNeRF.py:506-518) samples every ray at its OWN distances `t_min_i + k * stepSize` but then overwrites the distances of all
        rays with ray 0's: the first-pass intervals, the depth integral and - with resampling - the proposal bins and therefore the
        fine sample positions `o + d * z_fine` all come from ray 0's schedule.  Reproduced here with the stage entry points: a
        first-pass sample of ray i sits at o_i + d_i * (z_0[k] + (t_min_i - t_min_0)), i.e. on the ray with the origin moved by
        d_i * (t_min_i - t_min_0) and measured with z_0; the fine pass runs on the ORIGINAL origins with the merged distances."""
        lib, st, sc = _lib.load(), _lib.stream_handle(), self.scene()
        N, dev = rays.shape[0], rays.device
        f = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        z0 = z_pos[0:1].expand(N, n_coarse).contiguous()
        shifted = rays.clone()
        shifted[:, :3] = rays[:, :3] + rays[:, 3:6] * (z_pos[:, :1] - z_pos[0:1, :1])
        S = _lib.sample_count(n_coarse, n_fine, resampling, use_coarse_sample)
        has_env = self.envmap is not None
        astride = S + int(has_env)
        alpha = f(N, astride) if need_alpha else None
        w, bg, crd, rgb = f(N, S), f(N), f(N, S, 4), f(N, S, 3)
        use_flags = bool(sc.occ) or sc.term_eps > 0 or sc.weight_thres >= 0
        act = torch.zeros(N * S // 32 + 1, device=dev, dtype=torch.uint8) if use_flags else None
        near = float(self.near_far[0])
        if resampling:
            wc, z = f(N, n_coarse), f(N, S)
            _call("ego_march_density", sc, shifted.data_ptr(), N, n_coarse, z0.data_ptr(), None, None, near, 1, None, None, 0, wc.data_ptr(),
                  None, None, None, None, st)
            _call("ego_sample_pdf_merge", z0.data_ptr(), wc.data_ptr(), None, N, n_coarse, n_fine, int(use_coarse_sample), z.data_ptr(), None, st)
            _call("ego_march_density", sc, rays.data_ptr(), N, S, z.data_ptr(), None, None, near, 2, None, _lib.ptr(alpha), astride, w.data_ptr(),
                  bg.data_ptr(), crd.data_ptr(), None, _lib.ptr(act), st)
        else:
            z = z0
            _call("ego_march_density", sc, shifted.data_ptr(), N, S, z0.data_ptr(), None, None, near, 0, None, _lib.ptr(alpha), astride, w.data_ptr(),
                  bg.data_ptr(), crd.data_ptr(), None, _lib.ptr(act), st)
        _call("ego_shade", sc, rays.data_ptr(), z.data_ptr(), crd.data_ptr(), N, S, rgb.data_ptr(), None, _lib.ptr(act), st)
        rgb_map, depth = f(N, 3), f(N)
        bg_map, env_map = (f(N, 3), f(N, 3)) if has_env else (None, None)
        _call("ego_composite", sc, rays.data_ptr(), z.data_ptr(), w.data_ptr(), bg.data_ptr(), rgb.data_ptr(), N, S, rgb_map.data_ptr(),
              depth.data_ptr(), _lib.ptr(bg_map), _lib.ptr(env_map), None, st)
        return rgb_map, depth, bg_map, env_map, alpha

    def render_geometry(self, rays, *args, **kwargs):
        """Surface normals, accumulated weight and median depth of `rays`: geometry.render_geometry(self, rays, ...)."""
        from .geometry import render_geometry
        return render_geometry(self, rays, *args, **kwargs)

    def extract_mesh(self, lattice, level, **kwargs):
        """The triangle mesh of the surface sigma = level on `lattice`: geometry.extract_mesh(self, lattice, level, ...)."""
        from .geometry import extract_mesh
        return extract_mesh(self, lattice, level, **kwargs)

    # -- checkpoints (EgoNeRF.py:158-187) -----------------------------------------------------------------------------
    def save(self, path, global_step):
        ckpt = {"kwargs": self.get_kwargs(), "state_dict": {k: v.contiguous() for k, v in self.state_dict().items()},
                "global_step": global_step}
        if self.alphaMask is not None:  # packed bit volumes, EgoNeRF.py:161-167
            for g in ("yin", "yang"):
                vol = getattr(self.alphaMask, f"alpha_volume_{g}").bool().cpu().numpy()
                ckpt.update({f"alphaMask_{g}.shape": vol.shape, f"alphaMask_{g}.mask": np.packbits(vol.reshape(-1))})
        if self.envmap is not None:
            ckpt.update({"envmap.emission": self.envmap.emission.detach().cpu().numpy(),
                         "envmap_res_H": self.envmap.emission.shape[2]})
        from .compat import reference_pickle_paths
        with reference_pickle_paths():  # kwargs' coordinates / envmap objects go out under the reference's class paths
            torch.save(ckpt, path)

    def load(self, ckpt):
        if "alphaMask_yin.shape" in ckpt:  # EgoNeRF.py:175-180
            vols = []
            for g in ("yin", "yang"):
                shape = tuple(ckpt[f"alphaMask_{g}.shape"])
                bits = np.unpackbits(ckpt[f"alphaMask_{g}.mask"])[: int(np.prod(shape))].reshape(shape)
                vols.append(torch.from_numpy(bits).float().to(self.device))
            self.alphaMask = YinYangAlphaGridMask(self.device, vols[0], vols[1])
        if self.envmap is not None and "envmap.emission" in ckpt:
            self.envmap = EnvironmentMap(h=ckpt["envmap_res_H"], init_strategy="zero", device=self.device)
            self.envmap.load_envmap(emission=ckpt["envmap.emission"], device=self.device)
        self.load_state_dict(ckpt["state_dict"])
        self.invalidate_scene()
        if self.coarse_sigma_grid_update_rule == "conv" and self.density_plane_yin[0].is_cuda:
            self.update_coarse_sigma_grid()  # EgoNeRF.py:185-186 (a CPU-resident model only holds weights)
        return ckpt["global_step"]

    def load_state_dict(self, state_dict, strict=True):
        """Values are copied into the existing channel-last parameters (shapes/keys are the reference's)."""
        r = super().load_state_dict(state_dict, strict=strict)
        self.invalidate_scene()
        return r


class _WeakOwner:
    """Weak back-reference (keeps MLPRender_Fea out of the module graph cycle / state_dict)."""

    def __init__(self, obj):
        import weakref
        self._r = weakref.ref(obj)

    def __call__(self):
        o = self._r()
        if o is None:
            raise RuntimeError("owning EgoNeRF model was freed")
        return o
