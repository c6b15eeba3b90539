"""numpy / torch restatement of the depth term (csrc/ego_reg.hip states the formula), with the arithmetic type as a parameter, plus the
seeded inputs and the float64 answers the host and the GPU tests share.

Three forms: `direct`, the definition as written (weights by cumprod, D, the masked mean) in float64 numpy; `autograd_direct`, the same
in float64 torch on the CPU, whose autograd gives a gradient that owes nothing to the kernel's algebra; and `kernel_model`, the kernel's
algorithm: transmittance by a sequential product, the map s and the reverse recurrence R in `dtype`, sum w q and sum w in float64
whatever `dtype` is.  With dtype = float32 the model says how far float32 arithmetic alone is from float64 on given inputs; the GPU
tests' bounds are 4 x that distance (`case`)."""
import functools

import numpy as np
import torch

from tests import distortion_ref

NEAR, FAR = distortion_ref.NEAR, distortion_ref.FAR
SPACES = ("metric", "log", "disparity")
KINDS = ("l2", "l1")
N = 37   # not a multiple of the four rays of a block
EXACT_ROW = 5   # make_inputs: D equals the target exactly here
# A float32 output (pred, g_alpha) is off by up to 2^-24 of itself whatever the arithmetic before the rounding, and the value's 1 / V,
# 2 r / V factors are rounded to float32 as well: no bound goes below 4 x this, also where the float32 model happens to hit float64.
FLOAT32_HALF_ULP = 2.0 ** -24


def smap(x, space, dtype=np.float64, near=NEAR, far=FAR):
    """s(x) in `dtype`: identity ("metric") or distortion_ref's normalised maps (near / far as the float32 the C ABI takes, the scale
    rounded once from float64)."""
    t = np.dtype(dtype).type
    x = np.asarray(x, np.float32).astype(t)
    if space == "metric":
        return x
    n, f = np.float64(np.float32(near)), np.float64(np.float32(far))
    scale = t(1.0 / {"log": np.log(f / n), "disparity": 1.0 / n - 1.0 / f}[space])
    xc = np.maximum(x, t(n))
    out = np.log(xc / t(n)) * scale if space == "log" else (t(1) / t(n) - t(1) / xc) * scale
    assert out.dtype == np.dtype(dtype)
    return out


def valid_mask(target):
    target = np.asarray(target)
    return np.isfinite(target) & (target > 0)


def _safe(target):
    """targets with the invalid ones replaced by 1 (they take no part; NaN must not reach the arithmetic)"""
    return np.where(valid_mask(target), target, np.float32(1)).astype(np.float32)


def direct(alpha, z, target, tail=None, space="metric", kind="l2"):
    """-> (value, D [N]) by the definition, float64."""
    S = z.shape[1]
    a = np.asarray(alpha, np.float64)[:, :S]
    f = 1.0 - a + 1e-10
    T = np.concatenate([np.ones((a.shape[0], 1)), np.cumprod(f, 1)[:, :-1]], 1)
    w = a * T
    q = smap(z, space)
    qt = smap(tail, space) if tail is not None else np.zeros(a.shape[0])
    D = (w * q).sum(1) + (1.0 - w.sum(1)) * qt
    ok = valid_mask(target)
    if not ok.any():
        return 0.0, D
    r = D[ok] - smap(_safe(target), space)[ok]
    return float((r * r if kind == "l2" else np.abs(r)).mean()), D


def autograd_direct(alpha, z, target, tail=None, space="metric", kind="l2"):
    """-> (value, d value / d alpha [N][alpha's columns], D [N]): the definition in float64 torch, the gradient by autograd."""
    S = z.shape[1]
    a_all = torch.from_numpy(np.asarray(alpha, np.float64)).requires_grad_(True)
    a = a_all[:, :S]
    f = 1.0 - a + 1e-10
    T = torch.cat([torch.ones(a.shape[0], 1, dtype=torch.float64), torch.cumprod(f, 1)[:, :-1]], 1)
    w = a * T
    q = torch.from_numpy(smap(z, space))
    qt = torch.from_numpy(smap(tail, space)) if tail is not None else torch.zeros(a.shape[0], dtype=torch.float64)
    D = (w * q).sum(1) + (1.0 - w.sum(1)) * qt
    ok = torch.from_numpy(valid_mask(target))
    if not bool(ok.any()):
        return 0.0, np.zeros(a_all.shape), D.detach().numpy()
    r = D[ok] - torch.from_numpy(smap(_safe(target), space))[ok]
    value = (r * r if kind == "l2" else r.abs()).mean()
    value.backward()
    return float(value.detach()), a_all.grad.numpy(), D.detach().numpy()


def kernel_model(alpha, z, target, tail=None, space="metric", kind="l2", dtype=np.float64):
    """-> (value, g_alpha [N][alpha's columns] in `dtype`, D [N] float64) by the kernel's algorithm."""
    t = np.dtype(dtype).type
    alpha = np.asarray(alpha)
    N_, S = z.shape
    a = alpha[:, :S].astype(t)
    T, f = distortion_ref.transmittance(a, dtype)
    q = smap(z, space, dtype)
    qt = smap(tail, space, dtype) if tail is not None else np.zeros(N_, t)
    w = (a * T).astype(np.float64)
    D = (w * q.astype(np.float64)).sum(1) + (1.0 - w.sum(1)) * qt.astype(np.float64)
    G = q - qt[:, None]
    R = np.zeros_like(G)
    for i in range(S - 2, -1, -1):
        R[:, i] = G[:, i + 1] * a[:, i + 1] + f[:, i + 1] * R[:, i + 1]
    dD = T * (G - R)
    assert dD.dtype == np.dtype(dtype)
    ok = valid_mask(target)
    V = int(ok.sum())
    g = np.zeros(alpha.shape, t)
    if V == 0:
        return 0.0, g, D
    r = np.where(ok, D - smap(_safe(target), space, dtype).astype(np.float64), 0.0)
    value = float((r * r if kind == "l2" else np.abs(r)).sum() / V)
    scale = ((2.0 * r if kind == "l2" else np.sign(r)) / V).astype(t)
    g[:, :S] = dD * scale[:, None]
    g[~ok] = 0
    return value, g, D


def make_inputs(n_rays, S, seed=0, trailing_ones=False):
    """distortion_ref's alpha (exact 0s and an exact 1) and z, plus target and tail [N] float32: every third ray from row 3 on has the
    target exactly 0, rows 7, 8 and 10 have NaN, +inf and a negative one, the rest lie in [near, far].  Row EXACT_ROW is opaque at its first
    sample (alpha_0 = 1, so w_0 = 1 and D = s(z_0) whatever the tail) and its target is z_0: r = 0 exactly in every space."""
    assert n_rays >= 11 or n_rays == 1
    alpha, z = distortion_ref.make_inputs(max(n_rays, 5), S, seed=seed, trailing_ones=trailing_ones)
    first = 4 if n_rays == 1 else 0   # a single ray: row 4, an ordinary one (row 0 is empty)
    alpha, z = np.ascontiguousarray(alpha[first:first + n_rays]), np.ascontiguousarray(z[first:first + n_rays])
    rng = np.random.default_rng(77 * S + seed)
    target = rng.uniform(NEAR, FAR, size=n_rays).astype(np.float32)
    tail = rng.uniform(0.5, 2.0, size=n_rays).astype(np.float32)
    if n_rays > 1:
        target[3::3] = 0.0
        target[7], target[8], target[10] = np.nan, np.inf, -1.5
        alpha[EXACT_ROW, :S] = 0.0
        alpha[EXACT_ROW, 0] = 1.0
        target[EXACT_ROW] = z[EXACT_ROW, 0]
    return alpha, z, target, tail


class Case:
    """Inputs, the float64 answers (value, autograd's gradient, D) and the float32 model's relative distances from them."""


@functools.lru_cache(maxsize=None)
def case(S, trailing=False, space="metric", kind="l2", with_tail=True, n_rays=N):
    """Computed once per case and shared, read-only, by the tests.  `*_bound`: 4 x the float32 model's own distance from float64 on these
    inputs (value relative to |v64|, gradient to max |g64|, pred to max |D64|), never below 4 x FLOAT32_HALF_ULP."""
    c = Case()
    c.alpha, c.z, c.target, tail = make_inputs(n_rays, S, trailing_ones=trailing)
    c.tail = tail if with_tail else None
    args = (c.alpha, c.z, c.target, c.tail, space, kind)
    c.v64, c.g64, c.D64 = autograd_direct(*args)
    v32, g32, D32 = kernel_model(*args, dtype=np.float32)
    assert g32.dtype == np.float32
    c.g_scale, c.D_scale = float(np.abs(c.g64).max()), float(np.abs(c.D64).max())
    c.ev32 = abs(v32 - c.v64) / abs(c.v64) if c.v64 else 0.0
    c.eg32 = float(np.abs(g32 - c.g64).max()) / c.g_scale if c.g_scale else 0.0
    c.ep32 = float(np.abs(D32.astype(np.float32).astype(np.float64) - c.D64).max()) / c.D_scale
    c.value_bound, c.grad_bound, c.pred_bound = (4.0 * max(e, FLOAT32_HALF_ULP) for e in (c.ev32, c.eg32, c.ep32))
    for a in (c.alpha, c.z, c.target, tail, c.g64, c.D64):
        a.setflags(write=False)
    return c


# the GPU test's cases: the full cross at metric / l2 / tail, the other maps, l1 and no tail at the two sizes with carries
SIZES = (2, 63, 64, 65, 130, 512)
CASES = [(S, trailing, "metric", "l2", True) for S in SIZES for trailing in (False, True)] + \
        [(S, trailing, space, kind, with_tail) for S in (65, 130) for trailing in (False, True)
         for space, kind, with_tail in (("log", "l2", True), ("disparity", "l2", True), ("metric", "l1", True), ("metric", "l2", False),
                                        ("log", "l1", False))]
