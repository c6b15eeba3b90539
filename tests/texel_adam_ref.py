"""numpy restatement of ego_msi_adam_step (csrc/ego_msi.hip: k_msi_adam; include/egonerf_hip.h; DESIGN.md 3.3 "Texel Adam"): Adam that
steps only the texels whose gradient is not all zero, each on its own clock.

`dtype` is the arithmetic.  np.float64 is the reference: the hyper-parameters as Python floats and the bias corrections in float64,
torch.optim.Adam's own arithmetic.  np.float32 repeats the kernel operation by operation (every numpy operation on float32 arrays rounds
once, nothing is fused) on the float32 hyper-parameters and the float32 bias table the kernel is given, so the distance between the two
is the rounding error the kernel is entitled to."""
import numpy as np

PROJECT, ZERO_GRAD = 1, 2   # EGO_TEXEL_ADAM_*
INT32_MAX = np.int32(2 ** 31 - 1)


def bias_table(beta1, beta2, n, dtype=np.float64):
    """[n, 2]: entry t - 1 = {1 - beta1^t, sqrt(1 - beta2^t)} in float64, then rounded once to `dtype`."""
    t = np.arange(1, int(n) + 1, dtype=np.float64)
    return np.stack([1.0 - float(beta1) ** t, np.sqrt(1.0 - float(beta2) ** t)], axis=1).astype(dtype)


def project(p):
    """C <- max(C, 0), A <- clamp(A, 0, 1); a NaN becomes 0 (fmaxf / fminf)."""
    out = np.fmax(p, p.dtype.type(0))
    out[..., 3] = np.fmin(out[..., 3], p.dtype.type(1))
    return out


def step(texels, grad, moments, hits, lr, beta1, beta2, eps, bias, flags=0, dtype=np.float64):
    """One call: texels, grad [n, 4], moments [n, 2, 4] (m, then v), hits [n] int32, bias [n_bias, 2] of `dtype` -> the new
    (texels, grad, moments, hits); the inputs are not modified.  Untouched texels (all four gradient values compare equal to 0) come
    back as they went in."""
    f = dtype
    p, g, mo = np.asarray(texels).astype(f), np.asarray(grad).astype(f), np.asarray(moments).astype(f)
    h = np.asarray(hits).astype(np.int32)
    bias = np.asarray(bias)
    assert bias.dtype == f and bias.ndim == 2 and bias.shape[1] == 2 and len(bias) >= 1
    lr, b1, b2, eps = f(lr), f(beta1), f(beta2), f(eps)
    c1, c2 = f(1) - b1, f(1) - b2
    touched = ~np.all(g == 0, axis=1)   # a NaN compares unequal: touched
    with np.errstate(all="ignore"):
        t = np.where(h == INT32_MAX, h, h + np.int32(1)).astype(np.int32)
        c = bias[np.minimum(t, len(bias)) - 1]
        m = b1 * mo[:, 0] + c1 * g
        v = b2 * mo[:, 1] + (c2 * g) * g
        step_size = (lr / c[:, 0])[:, None]
        new = p - (step_size * m) / (np.sqrt(v) / c[:, 1][:, None] + eps)
        if flags & PROJECT:
            new = project(new)
    k = touched[:, None]
    out_p = np.where(k, new, p)
    out_m = np.where(touched[:, None, None], np.stack([m, v], axis=1), mo)
    out_h = np.where(touched, t, h).astype(np.int32)
    out_g = np.where(k, f(0), g) if flags & ZERO_GRAD else g.copy()
    return out_p.astype(f), out_g.astype(f), out_m.astype(f), out_h


def run(texels, grads, lr, beta1, beta2, eps, n_bias, flags=0, dtype=np.float64):
    """From zero moments and counts: one `step` per gradient of `grads` ([steps, n, 4]) -> (texels, moments, hits) after the last."""
    n = len(texels)
    p, mo, h = np.asarray(texels).astype(dtype), np.zeros((n, 2, 4), dtype), np.zeros(n, np.int32)
    bias = bias_table(beta1, beta2, n_bias, dtype)
    for g in grads:
        p, _, mo, h = step(p, g, mo, h, lr, beta1, beta2, eps, bias, flags, dtype)
    return p, mo, h
