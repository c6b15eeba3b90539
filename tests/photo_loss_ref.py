"""numpy / torch restatement of the photometric term and of the affine colour fit (csrc/ego_photo.hip states the formulas), with the
arithmetic type as a parameter, plus the seeded inputs the host and the GPU tests share.

`autograd_direct`: the loss's definition in float64 torch on the CPU, gradients by autograd (they owe nothing to the closed forms).
`kernel_model`: the closed forms - residual, rho and rho' per element in `dtype`, every sum in float64 whatever `dtype` is.  With
dtype = float32 it says how far float32 element arithmetic alone is from float64 on given inputs; the GPU tests' bounds are 4 x that
distance (`bound`), never below 4 x the half-ulp of the float32 an output is stored in.  `fit_model` is the same for the fit (products
in `dtype`, moments and the 2 x 2 solve in float64, the result stored in `dtype`)."""
import numpy as np
import torch

KINDS = ("l2", "l1", "huber", "charbonnier")
PARAM = dict(l2=0.0, l1=0.0, huber=0.1, charbonnier=1e-3)
FLOAT32_HALF_ULP = 2.0 ** -24
DEGENERATE = 1e-9   # the fit's definition of "all colours equal": det <= DEGENERATE * W * sum w c^2


def valid_mask(target, weight=None, image=None, K=None):
    ok = np.isfinite(np.asarray(target)).all(1)
    if weight is not None:
        w = np.asarray(weight)
        ok &= np.isfinite(w) & (w > 0)
    if image is not None:
        ok &= (np.asarray(image) >= 0) & (np.asarray(image) < K)
    return ok


def _clean(rgb, target, weight, image, affine, K):
    """float64 copies with the invalid rays' data replaced by harmless values and weight 0 (NaN must not reach the arithmetic) ->
    (ok, rgb, target, w, img, gain [N,3], bias [N,3])"""
    N = rgb.shape[0]
    K = affine.shape[0] if affine is not None else K
    ok = valid_mask(target, weight, image, K)
    w = np.where(ok, np.ones(N) if weight is None else np.nan_to_num(np.asarray(weight, np.float64), nan=0.0, posinf=0.0, neginf=0.0), 0.0)
    t = np.where(ok[:, None], np.nan_to_num(np.asarray(target, np.float64)), 0.0)
    img = np.zeros(N, np.int64) if image is None else np.where(ok, image, 0).astype(np.int64)
    if affine is None:
        gain, bias = np.ones((N, 3)), np.zeros((N, 3))
    else:
        a = np.asarray(affine, np.float64)
        gain, bias = a[img, :, 0], a[img, :, 1]
    return ok, np.asarray(rgb, np.float64), t, w, img, gain, bias


def autograd_direct(rgb, target, weight=None, image=None, affine=None, kind="l2", param=None, K=None):
    """-> (value, d value / d rgb [N,3], d value / d affine [K,3,2] or None): the definition in float64 torch, gradients by autograd."""
    p = float(np.float32(PARAM[kind] if param is None else param))   # as the float32 the C ABI takes
    ok, c, t, w, img, _, _ = _clean(rgb, target, weight, image, affine, K)
    c = torch.from_numpy(c).requires_grad_(True)
    a = None if affine is None else torch.from_numpy(np.asarray(affine, np.float64)).requires_grad_(True)
    t, w, img = torch.from_numpy(t), torch.from_numpy(w), torch.from_numpy(img)
    W = w.sum()
    if float(W) == 0.0:
        return 0.0, np.zeros(c.shape), (None if a is None else np.zeros(a.shape))
    cc = c if a is None else a[img, :, 0] * c + a[img, :, 1]
    okt = torch.from_numpy(ok)[:, None]
    r = torch.where(okt, cc - t, torch.zeros_like(cc))   # a NaN rgb on an INVALID ray takes no part
    if kind == "l2":
        rho = r * r
    elif kind == "l1":
        rho = r.abs()
    elif kind == "huber":
        rho = torch.where(r.abs() <= p, 0.5 * r * r, p * (r.abs() - 0.5 * p))
    else:
        rho = torch.sqrt(r * r + p * p) - p
    value = (w[:, None] * rho).sum() / (3.0 * W)
    value.backward()
    return float(value.detach()), c.grad.numpy(), (None if a is None else a.grad.numpy())


def kernel_model(rgb, target, weight=None, image=None, affine=None, kind="l2", param=None, K=None, dtype=np.float64):
    """-> (value, g_rgb [N,3] in `dtype`, g_affine [K,3,2] in `dtype` or None) by the closed forms."""
    ty = np.dtype(dtype).type
    p = ty(np.float32(PARAM[kind] if param is None else param))
    ok, c64, t64, w, img, gain64, bias64 = _clean(rgb, target, weight, image, affine, K)
    c, t, gain, bias = c64.astype(ty), t64.astype(ty), gain64.astype(ty), bias64.astype(ty)
    with np.errstate(invalid="ignore"):
        r = np.where(ok[:, None], (gain * c + bias if affine is not None else c) - t, ty(0))
        ar = np.abs(r)
        if kind == "l2":
            rho, d = r * r, ty(2) * r
        elif kind == "l1":
            rho, d = ar, np.sign(r)
        elif kind == "huber":
            rho, d = np.where(ar <= p, ty(0.5) * r * r, p * (ar - ty(0.5) * p)), np.where(ar <= p, r, p * np.sign(r))
        else:
            root = np.sqrt(r * r + p * p)
            rho, d = root - p, r / root
    assert rho.dtype == np.dtype(dtype) and d.dtype == np.dtype(dtype)
    W = float(w.sum())
    g_aff = None if affine is None else np.zeros(np.asarray(affine).shape, ty)
    if W == 0.0:
        return 0.0, np.zeros(c.shape, ty), g_aff
    value = float((w[:, None] * rho.astype(np.float64)).sum() / (3.0 * W))
    wd = w[:, None] * d.astype(np.float64)
    g_rgb = np.where(ok[:, None], wd * gain.astype(np.float64) / (3.0 * W), 0.0).astype(ty)
    if affine is not None:
        wd = np.where(ok[:, None], wd, 0.0)
        acc = np.zeros(g_aff.shape, np.float64)
        np.add.at(acc[:, :, 0], img[ok], (wd * c.astype(np.float64))[ok])
        np.add.at(acc[:, :, 1], img[ok], wd[ok])
        g_aff = (acc / (3.0 * W)).astype(ty)
    return value, g_rgb, g_aff


def fit_model(rgb, target, weight=None, image=None, K=1, dtype=np.float64):
    """-> (affine [K,3,2] in `dtype`, W_k [K] float64): the weighted least-squares (gain, bias) per image and channel in closed form."""
    ty = np.dtype(dtype).type
    ok, c64, t64, w, img, _, _ = _clean(rgb, target, weight, image, None, K)
    c, t = c64.astype(ty), t64.astype(ty)
    out, Wk = np.zeros((K, 3, 2), ty), np.zeros(K)
    out[:, :, 0] = 1
    for k in range(K):
        sel = ok & (img == k)
        wk = w[sel]
        Wk[k] = wk.sum()
        if Wk[k] == 0.0:
            continue
        for ch in range(3):
            x, y = c[sel, ch], t[sel, ch]
            Sx, St = (wk * x.astype(np.float64)).sum(), (wk * y.astype(np.float64)).sum()
            Sxx, Sxt = (wk * (x * x).astype(np.float64)).sum(), (wk * (x * y).astype(np.float64)).sum()
            det = Wk[k] * Sxx - Sx * Sx
            if det <= DEGENERATE * (Wk[k] * Sxx):
                gain, bias = 1.0, St / Wk[k] - Sx / Wk[k]
            else:
                gain = (Wk[k] * Sxt - Sx * St) / det
                bias = (St - gain * Sx) / Wk[k]
            out[k, ch] = gain, bias
    return out, Wk


def bound(got32, want64):
    """The project's rule (tests/test_hip_depth_loss.py): 4 x max(the float32 restatement's distance from float64 relative to the largest
    float64 entry, the float32 half-ulp) -> (relative bound, scale).  A quantity that is all zeros in float64 has scale 0: it must be
    met exactly."""
    want64 = np.asarray(want64, np.float64)
    scale = float(np.abs(want64).max()) if want64.size else 0.0
    if scale == 0.0:
        return 0.0, 0.0
    e32 = float(np.abs(np.asarray(got32, np.float64) - want64).max()) / scale
    return 4.0 * max(e32, FLOAT32_HALF_ULP), scale


def make_inputs(N, K=1, seed=0, with_weight=True, with_image=True, with_affine=True):
    """Seeded float32 inputs -> dict(rgb, target, weight, image, affine, K).  rgb in [0, 1]; target = rgb + residuals on both sides of
    Huber's 0.1 and down to Charbonnier's 1e-3.  From N >= 16 on: weights hold exact 0 (rows 3, and every 7th), NaN (5), a negative
    one (6) and +inf (7), image indices -1 (9) and K (11), the target a NaN channel (12) and an inf channel (13); below that every ray
    is valid (N = 1 and 2 would have none left).  With K > N some images have no ray at all."""
    g = np.random.default_rng(1000 * N + 10 * K + seed)
    rgb = g.uniform(0, 1, (N, 3)).astype(np.float32)
    target = (rgb + g.choice([0.003, 0.05, 0.3], (N, 3)) * g.standard_normal((N, 3))).astype(np.float32)
    weight = g.uniform(0.05, 1.0, N).astype(np.float32) if with_weight else None
    image = g.integers(0, K, N).astype(np.int32) if with_image else None
    affine = None
    if with_affine:
        assert with_image
        affine = np.stack([g.uniform(0.7, 1.3, (K, 3)), g.uniform(-0.05, 0.05, (K, 3))], -1).astype(np.float32)
    if N >= 16:
        if weight is not None:
            weight[::7] = 0.0
            weight[3], weight[5], weight[6], weight[7] = 0.0, np.nan, -0.5, np.inf
        if image is not None:
            image[9], image[11] = -1, K
        target[12, 1], target[13, 2] = np.nan, np.inf
    return dict(rgb=rgb, target=target, weight=weight, image=image, affine=affine, K=K)
