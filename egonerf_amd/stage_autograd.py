"""Autograd of the public stage ops (the reference's own API: compute_densityfeature, compute_coarse_densityfeature, compute_appfeature,
feature2density, raw2alpha, MLPRender_Fea / MLPRender, SHRender).  In the reference these are plain autograd code
(models/EgoNeRF.py:232-413, models/tensorBase.py:22-34, :54-78, :107-129, :415-419); here each one is a torch.autograd.Function whose
forward is the op's existing kernel call - the same kernels, the same bits as without a graph - and whose backward runs the HIP
backward kernels of csrc/ego_stage_grad.hip: the fp32-grade gradient of the reference function at the fp32 parameters.

The stage methods in model.py dispatch here only when grad mode is on and an input the op differentiates requires grad; otherwise their
code path is the one without autograd.  Only the inputs are saved (coordinates, features, view directions, sigma / dist and alpha); the
backward recomputes the rest.  The parameters go through `ctx.save_for_backward`, so an in-place optimiser step between forward and
backward raises torch's version error.  Coordinates receive no gradient (the reference detaches them before grid_sample); double
backward raises (once_differentiable)."""
from __future__ import annotations

import ctypes as C
from typing import List

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import check as _chk
from .field_tables import carve_channel_last, shapes_of


def needs_grad(*tensors) -> bool:
    """The condition under which a stage op records a graph: grad mode on and any of `tensors` requiring grad."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _workspace(model, nbytes: int, device) -> torch.Tensor:
    """A byte buffer of at least `nbytes`, cached on the model (grown when a larger call comes; stream-ordered reuse)."""
    if nbytes < 0:
        raise RuntimeError("stage backward: the library rejected the scene: " + _lib.load().ego_last_error().decode(errors="replace"))
    ws = getattr(model, "_stage_ws", None)
    if ws is None or ws.device != device or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 256), device=device, dtype=torch.uint8)
        model._stage_ws = ws
    return ws


def _grad_tables(params: List[torch.Tensor]):
    """Channel-last gradient tables shaped like `params` (one buffer, like the parameters) + the ego_vm_grad struct over them."""
    gs = carve_channel_last(shapes_of(params), params[0].device)
    return gs, _lib.grad_struct(gs)


class DensityFeatureFunction(torch.autograd.Function):
    """compute_densityfeature (coarse = 0) / compute_coarse_densityfeature (coarse = 1) with gradients to the 12 density tables
    (in field_tables.tables order).  The coarse op differentiates through the 2x2 / 2x average pooling of
    EgoNeRF.py:124-133 into the full-resolution tables; its values come from the last update_coarse_sigma_grid() snapshot.  Shipped
    shape (16 components), fine op: bit-reproducible table gradients (sorted walk); otherwise float atomics."""

    @staticmethod
    @_lib.device_guard
    def forward(ctx, model, coarse: int, coords, *params):
        out = model._density_forward(coords, coarse)
        ctx.model, ctx.coarse = model, coarse
        ctx.save_for_backward(coords, *params)
        return out

    @staticmethod
    @once_differentiable
    @_lib.device_guard
    def backward(ctx, g):
        coords, *params = ctx.saved_tensors
        model, lib = ctx.model, _lib.load()
        c = coords.contiguous().float()
        M = c.numel() // 7
        sc = model.scene()
        gs, gd = _grad_tables(params)
        ws = _workspace(model, lib.ego_density_feature_backward_workspace_bytes(sc, M, ctx.coarse), c.device)
        gg = g.contiguous().float()
        _chk(lib.ego_density_feature_backward(sc, c.data_ptr(), M, ctx.coarse, gg.data_ptr(), C.byref(gd), ws.data_ptr(), ws.numel(),
                                              _lib.stream_handle()), "ego_density_feature_backward")
        return (None, None, None, *gs)


class AppFeatureFunction(torch.autograd.Function):
    """compute_appfeature with gradients to the 12 appearance tables and basis_mat_{yin,yang}.weight.  Shipped shape (48 components):
    bit-reproducible table gradients; the basis gradients are fixed-order products for every shape."""

    @staticmethod
    @_lib.device_guard
    def forward(ctx, model, coords, *params):
        out = model._app_forward(coords)
        ctx.model = model
        ctx.save_for_backward(coords, *params)
        return out

    @staticmethod
    @once_differentiable
    @_lib.device_guard
    def backward(ctx, g):
        coords, *params = ctx.saved_tensors
        tables, basis = params[:12], params[12:]
        model, lib = ctx.model, _lib.load()
        c = coords.contiguous().float()
        M = c.numel() // 7
        sc = model.scene()
        gs, ga = _grad_tables(tables)
        ws = _workspace(model, lib.ego_app_feature_backward_workspace_bytes(sc, M), c.device)
        gb = torch.empty(64, 160, device=c.device)
        gg = g.contiguous().float()
        _chk(lib.ego_app_feature_backward(sc, c.data_ptr(), M, gg.data_ptr(), C.byref(ga), gb.data_ptr(), 160, ws.data_ptr(), ws.numel(),
                                          _lib.stream_handle()), "ego_app_feature_backward")
        D, ncol = basis[0].shape
        return (None, None, *gs, gb[0:D, :ncol].contiguous(), gb[32:32 + D, :ncol].contiguous())


class MLPRenderFunction(torch.autograd.Function):
    """MLPRender_Fea / MLPRender forward with gradients to mlp.{0,2,4}.{weight,bias}, the features and the view directions (through both
    positional encodings).  The backward recomputes x, h1, h2 and the pre-sigmoid values in fp32 from the fp32 weights, whatever
    mlp_precision the forward ran with."""

    @staticmethod
    @_lib.device_guard
    def forward(ctx, module, viewdirs, features, *weights):
        out = module._forward_impl(viewdirs, features)
        ctx.module = module
        ctx.save_for_backward(viewdirs, features, *weights)
        return out

    @staticmethod
    @once_differentiable
    @_lib.device_guard
    def backward(ctx, g):
        viewdirs, features, *w = ctx.saved_tensors
        model, lib = ctx.module._owner(), _lib.load()
        v = viewdirs.reshape(-1, 3).contiguous().float()
        f = features.reshape(-1, features.shape[-1]).contiguous().float()
        M, dev = f.shape[0], f.device
        sc = _lib.Scene.from_buffer_copy(model.scene())
        wc = [t.detach().contiguous().float() for t in w]   # the saved (version-checked) fp32 weights, reference layout
        sc.mlp_w[:] = [wc[0].data_ptr(), wc[2].data_ptr(), wc[4].data_ptr()]
        sc.mlp_b[:] = [wc[1].data_ptr(), wc[3].data_ptr(), wc[5].data_ptr()]
        hid, in_c = wc[0].shape
        ld1 = (in_c + 1 + 159) // 160 * 160
        g1, g2, g3 = torch.empty(hid, ld1, device=dev), torch.empty(hid, 160, device=dev), torch.empty(32, 160, device=dev)
        d_feat = torch.empty_like(f) if ctx.needs_input_grad[2] else None
        d_dirs = torch.empty_like(v) if ctx.needs_input_grad[1] else None
        ws = _workspace(model, lib.ego_mlp_fea_backward_workspace_bytes(sc, M), dev)
        gg = g.reshape(-1, 3).contiguous().float()
        _chk(lib.ego_mlp_fea_backward(sc, v.data_ptr(), f.data_ptr(), M, gg.data_ptr(), _lib.ptr(d_feat), _lib.ptr(d_dirs), g1.data_ptr(), ld1,
                                      g2.data_ptr(), 160, g3.data_ptr(), 160, ws.data_ptr(), ws.numel(), _lib.stream_handle()),
             "ego_mlp_fea_backward")
        return (None, None if d_dirs is None else d_dirs.view(viewdirs.shape), None if d_feat is None else d_feat.view(features.shape),
                g1[:, :in_c].contiguous(), g1[:, in_c].contiguous(), g2[:, :hid].contiguous(), g2[:, hid].contiguous(),
                g3[:3, :hid].contiguous(), g3[:3, hid].contiguous())


class SHRenderFunction(torch.autograd.Function):
    """SHRender with gradients to the view directions and the SH coefficients."""

    @staticmethod
    @_lib.device_guard
    def forward(ctx, viewdirs, features):
        from .model import _sh_render
        ctx.save_for_backward(viewdirs, features)
        return _sh_render(viewdirs, features)

    @staticmethod
    @once_differentiable
    @_lib.device_guard
    def backward(ctx, g):
        viewdirs, features = ctx.saved_tensors
        d, f = viewdirs.reshape(-1, 3).contiguous().float(), features.reshape(-1, 27).contiguous().float()
        dd = torch.empty_like(d) if ctx.needs_input_grad[0] else None
        df = torch.empty_like(f) if ctx.needs_input_grad[1] else None
        gg = g.contiguous().float()
        _chk(_lib.load().ego_sh_render_backward(d.data_ptr(), f.data_ptr(), d.shape[0], gg.data_ptr(), _lib.ptr(dd), _lib.ptr(df),
                                                _lib.stream_handle()), "ego_sh_render_backward")
        return (None if dd is None else dd.view(viewdirs.shape), None if df is None else df.view(features.shape))


class Feature2DensityFunction(torch.autograd.Function):
    """feature2density: softplus(f + density_shift) (torch's threshold 20) or relu, differentiated as F.softplus / F.relu are."""

    @staticmethod
    @_lib.device_guard
    def forward(ctx, model, features):
        out = model._feature2density_forward(features)
        ctx.model = model
        ctx.save_for_backward(features)
        return out

    @staticmethod
    @once_differentiable
    @_lib.device_guard
    def backward(ctx, g):
        (features,) = ctx.saved_tensors
        f = features.contiguous().float()
        sc = _lib.new_scene()
        sc.act_softplus, sc.density_shift = int(ctx.model.fea2denseAct == "softplus"), float(ctx.model.density_shift)
        d = torch.empty_like(f)
        gg = g.contiguous().float()
        _chk(_lib.load().ego_feature2density_backward(sc, f.data_ptr(), f.numel(), gg.data_ptr(), d.data_ptr(), _lib.stream_handle()),
             "ego_feature2density_backward")
        return None, d.view(features.shape)


class Raw2AlphaFunction(torch.autograd.Function):
    """raw2alpha -> (alpha, weight, bg_weight) with gradients to sigma and dist from gradients on any of the three outputs (the cumprod
    backward as a reverse scan, exact where 1 - alpha underflows)."""

    @staticmethod
    @_lib.device_guard
    def forward(ctx, sigma, dist):
        from .model import _raw2alpha
        alpha, weight, bg = _raw2alpha(sigma, dist)
        ctx.save_for_backward(sigma, dist, alpha, weight)
        return alpha, weight, bg

    @staticmethod
    @once_differentiable
    @_lib.device_guard
    def backward(ctx, g_alpha, g_weight, g_bg):
        sigma, dist, alpha, _weight = ctx.saved_tensors
        s, d = sigma.contiguous().float(), dist.contiguous().float()
        N, S = s.shape
        ds, dd = torch.empty_like(s), torch.empty_like(d)
        f = lambda t: None if t is None else t.contiguous().float()
        ga, gw, gb = f(g_alpha), f(g_weight), f(g_bg)
        _chk(_lib.load().ego_raw2alpha_backward(s.data_ptr(), d.data_ptr(), alpha.data_ptr(), N, S, _lib.ptr(ga), _lib.ptr(gw), _lib.ptr(gb),
                                                ds.data_ptr(), dd.data_ptr(), _lib.stream_handle()), "ego_raw2alpha_backward")
        return ds, dd
