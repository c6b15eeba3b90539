"""numpy / torch restatement of the structural term on patch batches (csrc/ego_patch_loss.hip states the formulas), with the arithmetic
type as a parameter, plus the seeded inputs the host and the GPU tests share.

`autograd_direct`: the definition in float64 torch on the CPU, the gradient by autograd (it owes nothing to the closed form).
`kernel_model`: the closed form as the kernel arranges it - the products x x, y y, x y, the per-window arithmetic from the moments to S and
the three coefficients, and the per-pixel combination in `dtype`; every tap-weighted sum (the moments, the transposed filter, the sum of
S) in float64 whatever `dtype` is.  With dtype = float32 it says how far float32 element arithmetic alone is from float64 on given inputs;
the GPU tests' bounds are 4 x that distance (`bound`), never below 4 x the half-ulp of float32.  `metric_guards=True` adds what
metrics.rgb_ssim has and the loss leaves out: float32 squares and products, the clamps of sxx, syy and sxy."""
import numpy as np
import torch

FLOAT32_HALF_ULP = 2.0 ** -24
DEFAULTS = dict(filter_sigma=1.5, max_val=1.0, k1=0.01, k2=0.03)


def taps(fs, sigma=1.5):
    """utils.py:117-121: the normalised Gaussian taps of rgb_ssim's window, float64"""
    hw = fs // 2
    shift = (2 * hw - fs + 1) / 2
    f = np.exp(-0.5 * ((np.arange(fs) - hw + shift) / sigma) ** 2)
    return f / f.sum()


def pixel_valid(target, weight, n):
    ok = np.isfinite(np.asarray(target[:n])).all(1)
    if weight is not None:
        w = np.asarray(weight[:n])
        ok &= np.isfinite(w) & (w > 0)
    return ok


def window_valid(target, weight, P, ph, pw, fs):
    """-> (pixel validity [P, ph, pw], window validity [P, ho, wo]): a window is valid iff every pixel under it is"""
    pv = pixel_valid(target, weight, P * ph * pw).reshape(P, ph, pw)
    win = np.lib.stride_tricks.sliding_window_view(pv, (fs, fs), axis=(1, 2))
    return pv, win.all((-1, -2))


def covered(wv, ph, pw, fs):
    """[P, ph, pw]: the pixels some valid window covers"""
    P, ho, wo = wv.shape
    out = np.zeros((P, ph, pw), bool)
    for a in range(fs):
        for b in range(fs):
            out[:, a:a + ho, b:b + wo] |= wv
    return out


def _clean(rgb, target, weight, P, ph, pw, fs):
    """float64 [P, ph, pw, 3] copies with the invalid pixels' data replaced by 0 (they lie under invalid windows only; NaN must not
    reach the arithmetic) -> (x, y, pv, wv)"""
    n = P * ph * pw
    pv, wv = window_valid(target, weight, P, ph, pw, fs)
    x = np.asarray(rgb[:n], np.float64).reshape(P, ph, pw, 3)
    y = np.asarray(target[:n], np.float64).reshape(P, ph, pw, 3)
    keep = pv[..., None]
    return np.where(keep, x, 0.0), np.where(keep, y, 0.0), pv, wv


def autograd_direct(rgb, target, patch, P, weight=None, fs=7, filter_sigma=1.5, max_val=1.0, k1=0.01, k2=0.03):
    """-> (value, d value / d rgb [B, 3]; rows behind the patches 0): the definition in float64 torch, the gradient by autograd."""
    ph, pw = patch
    x, y, pv, wv = _clean(rgb, target, weight, P, ph, pw, fs)
    grad = np.zeros((np.asarray(rgb).shape[0], 3))
    M = int(wv.sum())
    if M == 0:
        return 0.0, grad
    xt = torch.from_numpy(x).requires_grad_(True)
    yt = torch.from_numpy(y)
    g = torch.from_numpy(taps(fs, filter_sigma))
    gg = g[:, None] * g[None, :]
    win = lambda t: t.permute(0, 3, 1, 2).unfold(2, fs, 1).unfold(3, fs, 1)   # [P, 3, ho, wo, fs, fs]
    mom = lambda t: (win(t) * gg).sum((-1, -2))
    mux, muy, exx, eyy, exy = mom(xt), mom(yt), mom(xt * xt), mom(yt * yt), mom(xt * yt)
    sxx, syy, sxy = exx - mux * mux, eyy - muy * muy, exy - mux * muy
    C1, C2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    S = ((2 * mux * muy + C1) * (2 * sxy + C2)) / ((mux * mux + muy * muy + C1) * (sxx + syy + C2))
    S = torch.where(torch.from_numpy(wv)[:, None], S, torch.zeros_like(S))
    value = 1.0 - S.sum() / (3.0 * M)
    value.backward()
    grad[:P * ph * pw] = xt.grad.numpy().reshape(-1, 3)
    return float(value.detach()), grad


def coefficients(mux, muy, exx, eyy, exy, C1, C2, ty, metric_guards=False):
    """-> (S, dmu, dS/dExx, dS/dExy) from the moments, in `ty`"""
    two = ty(2)
    sxx, syy, sxy = exx - mux * mux, eyy - muy * muy, exy - mux * muy
    if metric_guards:
        sxx, syy = np.maximum(sxx, 0), np.maximum(syy, 0)
        sxy = np.sign(sxy) * np.minimum(np.sqrt(sxx * syy), np.abs(sxy))
    A1, B1 = two * (mux * muy) + C1, mux * mux + muy * muy + C1
    A2, B2 = two * sxy + C2, sxx + syy + C2
    S = (A1 * A2) / (B1 * B2)
    dmu = (A2 / B2) * (two * muy * B1 - two * mux * A1) / (B1 * B1) + two * mux * S / B2 - two * muy * A1 / (B1 * B2)
    return S, dmu, -S / B2, two * A1 / (B1 * B2)


def kernel_model(rgb, target, patch, P, weight=None, fs=7, filter_sigma=1.5, max_val=1.0, k1=0.01, k2=0.03, dtype=np.float64,
                 metric_guards=False):
    """-> (value, g_rgb [B, 3] in `dtype`; rows behind the patches 0) by the closed form."""
    ty = np.dtype(dtype).type
    ph, pw = patch
    x64, y64, pv, wv = _clean(rgb, target, weight, P, ph, pw, fs)
    g_rgb = np.zeros((np.asarray(rgb).shape[0], 3), ty)
    M = int(wv.sum())
    if M == 0:
        return 0.0, g_rgb
    ho, wo = ph - fs + 1, pw - fs + 1
    g = taps(fs, filter_sigma)
    x, y = x64.astype(ty), y64.astype(ty)
    prod = (lambda a, b: (a.astype(np.float32) * b.astype(np.float32))) if metric_guards else (lambda a, b: a * b)

    def mom(t):   # the tap-weighted sums are float64 whatever the elements are
        w = np.lib.stride_tricks.sliding_window_view(np.asarray(t, np.float64), (fs, fs), axis=(1, 2))   # [P, ho, wo, 3, fs, fs]
        return np.einsum("phwcab,a,b->phwc", w, g, g)

    m = [mom(x), mom(y), mom(prod(x, x)), mom(prod(y, y)), mom(prod(x, y))]
    C1, C2 = ty((k1 * max_val) ** 2), ty((k2 * max_val) ** 2)
    with np.errstate(all="ignore"):
        S, dmu, dxx, dxy = coefficients(*(t.astype(ty) for t in m), C1, C2, ty, metric_guards)
    assert S.dtype == np.dtype(dtype)
    keep = wv[..., None]
    S, dmu, dxx, dxy = (np.where(keep, t, ty(0)) for t in (S, dmu, dxx, dxy))
    value = 1.0 - float(S.astype(np.float64).sum()) / (3.0 * M)
    F = []
    for coef in (dmu, dxx, dxy):   # the transposed filter, float64 sums
        acc = np.zeros((P, ph, pw, 3))
        for a in range(fs):
            for b in range(fs):
                acc[:, a:a + ho, b:b + wo] += g[a] * g[b] * coef.astype(np.float64)
        F.append(acc.astype(ty))
    grad = -((F[0] + ty(2) * x * F[1]) + y * F[2]) * ty(1.0 / (3.0 * M))
    grad = np.where(covered(wv, ph, pw, fs)[..., None], grad, ty(0))
    g_rgb[:P * ph * pw] = grad.reshape(-1, 3)
    return value, g_rgb


def bound(got32, want64):
    """The project's rule (tests/photo_loss_ref.py): 4 x max(the float32 restatement's distance from float64 relative to the largest
    float64 entry, the float32 half-ulp) -> (relative bound, scale); an all-zero quantity has scale 0 and must be met exactly."""
    want64 = np.asarray(want64, np.float64)
    scale = float(np.abs(want64).max()) if want64.size else 0.0
    if scale == 0.0:
        return 0.0, 0.0
    e32 = float(np.abs(np.asarray(got32, np.float64) - want64).max()) / scale
    return 4.0 * max(e32, FLOAT32_HALF_ULP), scale


def textured(g, P, ph, pw):
    """random textured patches in [0, 1]: a per-patch gradient plus a sine texture plus noise, [P, ph, pw, 3] float64"""
    a, b = np.meshgrid(np.arange(ph), np.arange(pw), indexing="ij")
    base = g.uniform(0.2, 0.8, (P, 1, 1, 3)) + g.uniform(-0.01, 0.01, (P, 1, 1, 3)) * a[None, :, :, None] \
        + g.uniform(-0.01, 0.01, (P, 1, 1, 3)) * b[None, :, :, None]
    tex = 0.1 * np.sin(g.uniform(0.3, 2.0, (P, 1, 1, 3)) * a[None, :, :, None] + g.uniform(0.3, 2.0, (P, 1, 1, 3)) * b[None, :, :, None])
    return np.clip(base + tex + 0.05 * g.standard_normal((P, ph, pw, 3)), 0.0, 1.0)


def make_inputs(P, ph, pw, fs, with_weight=True, tail=5, seed=0, invalid=True):
    """Seeded float32 inputs -> dict(rgb [B, 3], target [B, 3], weight [B] or None), B = P ph pw + tail.  With `invalid`: from P >= 2 on
    patch 1 is invalid as a whole (and holds a NaN colour, which must stay hidden); where a patch has more than one window, patch 0 and
    every third patch lose a corner pixel (so some of their windows); the ways a pixel is invalid cycle through weight 0, weight NaN, a
    negative weight and a NaN target channel (without weights: NaN and inf targets).  The tail rows hold a NaN colour too."""
    g = np.random.default_rng(100000 * P + 1000 * ph + 10 * pw + fs + 7 * seed)
    tgt = textured(g, P, ph, pw)
    rgb = np.clip(tgt + g.choice([0.01, 0.05, 0.2], (P, 1, 1, 1)) * g.standard_normal((P, ph, pw, 3)), 0.0, 1.0)
    n, B = P * ph * pw, P * ph * pw + tail
    rgb = np.concatenate([rgb.reshape(n, 3), g.uniform(0, 1, (tail, 3))]).astype(np.float32)
    target = np.concatenate([tgt.reshape(n, 3), g.uniform(0, 1, (tail, 3))]).astype(np.float32)
    weight = g.uniform(0.05, 1.0, B).astype(np.float32) if with_weight else None
    if tail:
        rgb[n, 1] = np.nan
    if not invalid:
        return dict(rgb=rgb, target=target, weight=weight)

    def kill(e, how):
        if weight is not None and how % 4 != 3:
            weight[e] = (0.0, np.nan, -0.5)[how % 4]
        else:
            target[e, how % 3] = np.nan if how % 2 else np.inf

    per, many = ph * pw, (ph - fs + 1) * (pw - fs + 1) > 1
    if P >= 2:
        for e in range(per, 2 * per):
            kill(e, e)
        rgb[per + per // 2, 0] = np.nan
    if many:
        for p in range(0, P, 3):
            if p != 1:
                kill(p * per + (0 if p % 2 == 0 else per - 1), p // 3)
    return dict(rgb=rgb, target=target, weight=weight)
