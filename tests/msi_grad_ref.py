"""torch-on-CPU restatement of multi-sphere-image playback (csrc/ego_msi.hip: k_msi_render) whose texels take part in autograd.

The geometry - intersections and bilinear footprints - is constant with respect to the texels: it is computed in numpy in the asked
arithmetic, the footprints by tests/msi_ref.erp_tap, exactly as tests/msi_ref.msi_render computes them.  The bilinear form and the "over"
are torch operations in the same order, so `torch.autograd` yields d rgb / d layers and d rgb / d background: in float64 the reference, in
float32 the roundings a float32 implementation is entitled to."""
import numpy as np
import torch

from tests import msi_ref

NP = {torch.float64: np.float64, torch.float32: np.float32}


def geometry(rays, center, radii, Hm, Wm, dtype):
    """-> (per layer: (live [N] bool, tap, t_k / |dir| [N]), the background's tap); numpy, arithmetic `dtype`."""
    rays = np.asarray(rays).astype(dtype)
    c, radii = np.asarray(center, np.float32).astype(dtype), np.asarray(radii, np.float32).astype(dtype)
    zero = dtype(0)
    p, d = rays[:, :3] - c[None], rays[:, 3:6]
    dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = d / dn[:, None]
    pp = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    b = (p[:, 0] * d[:, 0] + p[:, 1] * d[:, 1]) + p[:, 2] * d[:, 2]
    bb_pp = b * b - pp
    pn = np.sqrt(pp)
    per_layer = []
    for R in radii:
        tk = np.sqrt(np.maximum(bb_pp + R * R, zero)) - b
        per_layer.append((~(R <= pn), msi_ref.erp_tap((p + tk[:, None] * d) / R, Hm, Wm, dtype), tk / dn))
    return per_layer, msi_ref.erp_tap(d, Hm, Wm, dtype)


def bilinear(img, tap):
    """img [Hm, Wm, 4] torch -> [N, 4]: (v00 (1 - fc) + v01 fc) (1 - fr) + (v10 (1 - fc) + v11 fc) fr, the taps constants."""
    ra, rb, ca, cb = (torch.from_numpy(np.ascontiguousarray(a)) for a in tap[:4])
    fr, fc = (torch.from_numpy(np.ascontiguousarray(a)).to(img.dtype)[:, None] for a in tap[4:])
    gc, gr = 1 - fc, 1 - fr
    return (img[ra, ca] * gc + img[ra, cb] * fc) * gr + (img[rb, ca] * gc + img[rb, cb] * fc) * fr


def msi_render(rays, center, radii, layers, background=None, dtype=torch.float64):
    """rays [N, 6] numpy, layers [L, Hm, Wm, 4] and background [Hm, Wm, 4] (or None) CPU torch tensors (of any float type; they may require
    grad) -> (rgb [N, 3], depth [N]) in `dtype`, differentiable with respect to the texels."""
    L, Hm, Wm = layers.shape[:3]
    per_layer, bg_tap = geometry(rays, center, radii, Hm, Wm, NP[dtype])
    layers = layers.to(dtype)
    N = len(rays)
    T = torch.ones(N, dtype=dtype)
    rgb, depth = torch.zeros(N, 3, dtype=dtype), torch.zeros(N, dtype=dtype)
    for k in range(L):
        live, tap, t = per_layer[k]
        live, t = torch.from_numpy(live), torch.from_numpy(t)
        v = bilinear(layers[k], tap)
        rgb = torch.where(live[:, None], rgb + T[:, None] * v[:, :3], rgb)
        depth = torch.where(live, depth + (T * v[:, 3]) * t, depth)
        T = torch.where(live, T * (1 - v[:, 3]), T)
    if background is not None:
        rgb = rgb + T[:, None] * bilinear(background.to(dtype), bg_tap)[:, :3]
    return rgb, depth


def texel_gradients(rays, center, radii, layers, background, g_rgb, dtype):
    """d <g_rgb, rgb> / d (layers, background) by autograd, arithmetic `dtype` -> (float64 numpy [L, Hm, Wm, 4], [Hm, Wm, 4] or None)."""
    lt = torch.from_numpy(np.asarray(layers)).to(dtype).requires_grad_(True)
    bt = None if background is None else torch.from_numpy(np.asarray(background)).to(dtype).requires_grad_(True)
    rgb, _ = msi_render(rays, center, radii, lt, bt, dtype)
    rgb.backward(torch.from_numpy(np.asarray(g_rgb)).to(dtype))
    return lt.grad.double().numpy(), (None if bt is None else bt.grad.double().numpy())
