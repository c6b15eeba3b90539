"""numpy restatement of the two multi-sphere-image kernels (csrc/ego_msi.hip), operation by operation.

`dtype` is the arithmetic: np.float64 is the reference, np.float32 repeats the kernels' own roundings (every numpy operation on float32
arrays rounds once, nothing is fused), so the distance between the two is the rounding error the kernels are entitled to.  Inputs are taken
as they are (float32 rays, float16 or float32 texels) and converted exactly."""
import numpy as np


def msi_layers(z, alpha, rgb, bounds, dtype=np.float64):
    """z [N, S] ascending, alpha [N, S], rgb [N, S, 3], bounds [L + 1] -> [L, N, 4] premultiplied RGBA in `dtype`: per layer, over the
    samples with bounds[k] <= z < bounds[k + 1] in order, C += (t * alpha) * rgb, t *= (1 - alpha), A = 1 - t."""
    z, bounds = np.asarray(z), np.asarray(bounds)   # compared in their own type (float32), as the kernel compares them
    a, c = np.asarray(alpha).astype(dtype), np.asarray(rgb).astype(dtype)
    N, S = z.shape
    L = bounds.size - 1
    one = dtype(1)
    out = np.zeros((L, N, 4), dtype)
    for k in range(L):
        t = np.ones(N, dtype)
        C = np.zeros((N, 3), dtype)
        for s in range(S):
            m = (z[:, s] >= bounds[k]) & (z[:, s] < bounds[k + 1])
            w = t * a[:, s]
            C = np.where(m[:, None], C + w[:, None] * c[:, s], C)
            t = np.where(m, t * (one - a[:, s]), t)
        out[k, :, :3] = C
        out[k, :, 3] = one - t
    return out


def erp_tap(u, Hm, Wm, dtype):
    """Unit directions u [N, 3] -> (row0, row1, col0, col1 int64 [N], fr, fc `dtype` [N]): the bilinear footprint in an Hm x Wm
    equirectangular image; columns wrap, rows clamp."""
    one, two, half, pi = dtype(1), dtype(2), dtype(0.5), dtype(np.pi)
    theta = np.arcsin(np.clip(u[:, 1], -one, one))
    phi = np.arctan2(-u[:, 0], -u[:, 2])
    row = (one - (two * theta) / pi) * (dtype(Hm) * half) - half
    col = (one - phi / pi) * (dtype(Wm) * half) - half
    row, col = np.clip(row, -one, dtype(Hm)), np.clip(col, -one, dtype(Wm))
    r0f, c0f = np.floor(row), np.floor(col)
    r0, c0 = r0f.astype(np.int64), c0f.astype(np.int64)
    return (np.clip(r0, 0, Hm - 1), np.clip(r0 + 1, 0, Hm - 1), np.mod(c0, Wm), np.mod(c0 + 1, Wm), row - r0f, col - c0f)


def bilinear(img, tap, dtype):
    """img [Hm, Wm, 4] -> [N, 4]: (v00 (1 - fc) + v01 fc) (1 - fr) + (v10 (1 - fc) + v11 fc) fr."""
    ra, rb, ca, cb, fr, fc = tap
    img = np.asarray(img).astype(dtype)
    one = dtype(1)
    gc, gr = (one - fc)[:, None], (one - fr)[:, None]
    fr, fc = fr[:, None], fc[:, None]
    return (img[ra, ca] * gc + img[ra, cb] * fc) * gr + (img[rb, ca] * gc + img[rb, cb] * fc) * fr


def msi_render(rays, center, radii, layers, background=None, dtype=np.float64):
    """rays [N, 6], center [3], radii [L], layers [L, Hm, Wm, 4], background [Hm, Wm, 4] or None -> (rgb [N, 3], depth [N]) in `dtype`.
    The direction is normalised first; depth is in the given ray's parameter (t / |d|)."""
    rays = np.asarray(rays).astype(dtype)
    c, radii = np.asarray(center, np.float32).astype(dtype), np.asarray(radii, np.float32).astype(dtype)
    L, Hm, Wm = layers.shape[:3]
    one, zero = dtype(1), dtype(0)
    p, d = rays[:, :3] - c[None], rays[:, 3:6]
    dn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = d / dn[:, None]
    pp = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    b = (p[:, 0] * d[:, 0] + p[:, 1] * d[:, 1]) + p[:, 2] * d[:, 2]
    bb_pp = b * b - pp
    pn = np.sqrt(pp)
    N = rays.shape[0]
    T = np.ones(N, dtype)
    rgb, depth = np.zeros((N, 3), dtype), np.zeros(N, dtype)
    for k in range(L):
        R = radii[k]
        live = ~(R <= pn)
        tk = np.sqrt(np.maximum(bb_pp + R * R, zero)) - b
        u = (p + tk[:, None] * d) / R
        v = bilinear(layers[k], erp_tap(u, Hm, Wm, dtype), dtype)
        rgb = np.where(live[:, None], rgb + T[:, None] * v[:, :3], rgb)
        depth = np.where(live, depth + (T * v[:, 3]) * (tk / dn), depth)
        T = np.where(live, T * (one - v[:, 3]), T)
    if background is not None:
        v = bilinear(background, erp_tap(d, Hm, Wm, dtype), dtype)
        rgb = rgb + T[:, None] * v[:, :3]
    return rgb, depth


def over_composite(layers_rgba):
    """[L, N, 4] premultiplied, front to back -> [N, 3]: sum_k T_k C_k, T_k = prod_{j < k} (1 - A_j)."""
    T = np.ones(layers_rgba.shape[1], layers_rgba.dtype)
    out = np.zeros((layers_rgba.shape[1], 3), layers_rgba.dtype)
    for k in range(layers_rgba.shape[0]):
        out = out + T[:, None] * layers_rgba[k, :, :3]
        T = T * (1 - layers_rgba[k, :, 3])
    return out
