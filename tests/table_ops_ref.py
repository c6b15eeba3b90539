"""Plain numpy restatements of the training step's table kernels (csrc/ego_reg.hip, the end of csrc/ego_stages.hip): TV / L1 / ortho
regularisers, bilinear table resampling, 2x average pooling, the multi-tensor Adam with its device clock, and the environment map's
lookup and backward.  Every operation comes in two forms:

  (a) truth: float64, a closed formula (torch-CPU autograd in float64 for the regularisers' gradients);
  (b) a float32 copy of the kernel, operation for operation.  The library is built with -ffp-contract=off and float32 `/` and `sqrtf`
      are correctly rounded, so a kernel without a reduction is determined bit for bit and (b) has its bits.

Tolerances are derived, not picked.  For a fixed chain of float32 + - * / sqrt the running-error bound holds in any order:

    |computed - exact| <= gamma_k * (sum of the absolute values of the terms),  gamma_k = k u / (1 - k u),  u = 2^-24,

with k the number of roundings on the longest path to an output.  Each restatement states its k (the K_* constants, with the count in
a comment) and returns the sum of absolute terms in float64 next to the value; `bound` adds k denormal spacings (2^-149) for results
that underflow, which the relative model does not cover.  tests/test_table_ops_host.py pins all of this on the CPU."""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
F32 = np.float32


def gamma(k):
    return k * U / (1.0 - k * U)


def bound(k, abs_terms):
    """The running-error bound for k roundings over terms of this absolute sum (array or scalar, float64)."""
    return gamma(k) * np.asarray(abs_terms, np.float64) + k * TINY


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- TV (k_tv_plane), x [H][W][C] ------------------------------------------------------------------------------------------------------
def tv_coeffs(C, H, W, scale):
    """ah, aw as ego_tv_plane rounds them: scale * 2.f / ((float)C * (float)(H - 1) * (float)W), left to right."""
    s2 = F32(scale) * F32(2)
    return s2 / (F32(C) * F32(H - 1) * F32(W)), s2 / (F32(C) * F32(H) * F32(W - 1))


K_TV_GRAD = 8    # ah: 2 products of the counts + the division (scale * 2 is exact), a difference, bh - dh, * ah, the sum, + one for aw's side
K_TV_VALUE = 9   # ah (3), the difference, its square, * ah, the sum of the two halves, float64 adds (negligible, counted once), float32 result


def tv_f32(x, scale):
    """-> per-texel float32 terms of the value [H][W][C], per-texel float32 gradient, and the gradient's absolute terms (float64)."""
    x = np.ascontiguousarray(x, F32)
    H, W, C = x.shape
    ah, aw = tv_coeffs(C, H, W, scale)
    dh, dw = np.zeros_like(x), np.zeros_like(x)
    dh[:-1] = x[1:] - x[:-1]
    dw[:, :-1] = x[:, 1:] - x[:, :-1]
    bh, bw = np.zeros_like(x), np.zeros_like(x)
    bh[1:] = x[1:] - x[:-1]
    bw[:, 1:] = x[:, 1:] - x[:, :-1]
    terms = dh * dh * ah + dw * dw * aw
    grad = F32(2) * (ah * (bh - dh) + aw * (bw - dw))
    a = lambda t: np.abs(t.astype(np.float64))
    g_abs = 2.0 * (float(ah) * (a(bh) + a(dh)) + float(aw) * (a(bw) + a(dw)))
    assert terms.dtype == F32 and grad.dtype == F32
    return terms, grad, g_abs


def tv_f64(x, scale):
    """utils.py:155-171 in float64 with autograd: value, gradient [H][W][C].  Every term of the value is >= 0: its absolute sum is the value."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, np.float64)).requires_grad_(True)
    H, W, C = t.shape
    v = float(F32(scale)) * 2.0 * ((t[1:] - t[:-1]).pow(2).sum() / (C * (H - 1) * W) + (t[:, 1:] - t[:, :-1]).pow(2).sum() / (C * H * (W - 1)))
    v.backward()
    return float(v.detach()), t.grad.numpy()


# ---- L1 (k_l1) -------------------------------------------------------------------------------------------------------------------------
K_L1_GRAD = 1    # the division scale / (float)n; the product with +-1 is exact
K_L1_VALUE = 2   # that division, and the float64 sum and product (far below u, counted once)


def l1_f32(x, scale):
    """-> a (float32), the per-element float32 terms |x|, the per-element float32 gradient a * sign(x)."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    a = F32(scale) / F32(x.size)
    sign = (x > 0).astype(F32) - (x < 0).astype(F32)
    return a, np.abs(x), a * sign


def l1_f64(x, scale):
    """EgoNeRF.py:206-212: scale * mean |x| and its gradient, float64."""
    x = np.asarray(x, np.float64).reshape(-1)
    s = float(F32(scale))
    return s * np.abs(x).sum() / x.size, s * np.sign(x) / x.size


# ---- ortho (k_line_ortho), L [n][C] ----------------------------------------------------------------------------------------------------
def k_ortho_value(n):
    return n + 3     # a product, n - 1 adds along the Gram sum, a = scale / (float)(C (C - 1)), the float64 tail counted once, float32 result


def k_ortho_grad(C):
    return C + 3     # C adds of exact products s * L, a, 2.f * a (exact) * acc, and one to spare for the accumulation into grad


def ortho_gram_f32(L):
    """G = L^T L with every entry summed sequentially over n in float32, products rounded first (np.cumsum adds in order)."""
    L = np.ascontiguousarray(L, F32)
    prods = L[:, :, None] * L[:, None, :]
    return np.cumsum(prods, axis=0, dtype=F32)[-1]


def ortho_f32(L, scale):
    """-> value (float64 sum of the float32 |G_ij| times (double)a, as the kernel forms it), float32 gradient [n][C], the absolute terms of
    the value (scalar) and of the gradient [n][C], and G."""
    L = np.ascontiguousarray(L, F32)
    n, C = L.shape
    G = ortho_gram_f32(L)
    off = ~np.eye(C, dtype=bool)
    a = F32(scale) / F32(C * (C - 1))
    value = float(np.abs(G[off]).astype(np.float64).sum()) * float(a)
    S = np.where(off, (G > 0).astype(F32) - (G < 0).astype(F32), F32(0))
    acc = np.cumsum(L[:, None, :] * S[None, :, :], axis=2, dtype=F32)[:, :, -1]     # [k][i]: sequential over j
    grad = F32(2) * a * acc
    L64 = np.abs(L.astype(np.float64))
    v_abs = float(a) * float((L64.T @ L64)[off].sum())
    g_abs = 2.0 * float(a) * (L64 @ np.abs(S.astype(np.float64)).T)
    assert grad.dtype == F32
    return value, grad, v_abs, g_abs, G


def ortho_f64(L, scale):
    """EgoNeRF.py:189-201 in float64 with autograd: scale * mean |offdiag(L^T L)|, gradient, and the float64 Gram matrix."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(L, np.float64)).requires_grad_(True)
    C = t.shape[1]
    G = t.T @ t
    off = ~torch.eye(C, dtype=torch.bool)
    v = float(F32(scale)) * G[off].abs().sum() / (C * (C - 1))
    v.backward()
    return float(v.detach()), t.grad.numpy(), G.detach().numpy()


def ortho_input(C, n, seed):
    """L[:, i] = s_i (base + 0.05 noise), s_i = +-1: every off-diagonal Gram entry is far from zero and about half are negative."""
    r = np.random.default_rng(seed)
    base = r.uniform(0.5, 1.5, (n, 1))
    s = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    return (s[None, :] * (base + 0.05 * r.uniform(-1.0, 1.0, (n, C)))).astype(F32)


def ortho_disjoint_input(n=12):
    """Three columns; columns 0 and 1 have disjoint support (G_01 is exactly 0 in any precision), column 2 overlaps both."""
    r = np.random.default_rng(5)
    L = np.zeros((n, 3), F32)
    L[: n // 2, 0] = r.uniform(0.5, 1.5, n // 2)
    L[n // 2:, 1] = r.uniform(0.5, 1.5, n - n // 2)
    L[:, 2] = -r.uniform(0.5, 1.5, n)
    return L


# ---- bilinear resampling (lin_taps, k_resample_table) -----------------------------------------------------------------------------------
def lin_taps_f32(xhat, n):
    """ego_device.h lin_taps: clamped indices i0, i1 and weights w0, w1 with the out-of-range taps zeroed; a NaN lands on (-2, -1)."""
    xhat = np.asarray(xhat, F32)
    with np.errstate(invalid="ignore"):
        sc = F32(0.5) * F32(n - 1)
        ix = (xhat + F32(1)) * sc
        fl = np.floor(ix)
        f = ix - fl
        flc = np.fmin(np.fmax(fl, F32(-2)), F32(n))     # fmax / fmin drop a NaN operand, like fmaxf / fminf
        i0 = flc.astype(np.int32)
    i1 = i0 + 1
    in0, in1 = (i0 >= 0) & (i0 < n), (i1 >= 0) & (i1 < n)
    w0 = np.where(in0, F32(1) - f, F32(0)).astype(F32)
    w1 = np.where(in1, f, F32(0)).astype(F32)
    return np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1), w0, w1


def lin_taps_f64(xhat, n):
    """The same rule in float64 from the (float32) coordinate: F.grid_sample(align_corners=True, padding_mode="zeros") on one axis.
    Also returns |ix|, the size of the unnormalised position: its rounding moves weight between the two taps."""
    x = np.asarray(xhat, np.float64)
    with np.errstate(invalid="ignore"):
        ix = (x + 1.0) * (0.5 * (n - 1))
        fl = np.floor(ix)
        f = ix - fl
        i0 = np.where(np.isnan(fl), -2.0, np.clip(fl, -2.0, float(n))).astype(np.int64)
    i1 = i0 + 1
    in0, in1 = (i0 >= 0) & (i0 < n), (i1 >= 0) & (i1 < n)
    w0, w1 = np.where(in0, 1.0 - f, 0.0), np.where(in1, f, 0.0)
    pos = np.where(np.isnan(ix), 0.0, np.abs(ix))
    return np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1), w0, w1, in0, in1, pos


K_RESAMPLE = 10   # per axis: x + 1, * sc, 1 - f (3, and 3 for the other axis); two products per tap, two adds on the longest path


def resample_f32(src, xs, ys):
    """k_resample_table without contraction: src [H][W][C], xs [W2], ys [H2] -> [H2][W2][C] float32."""
    src = np.ascontiguousarray(src, F32)
    H, W, C = src.shape
    x0, x1, wx0, wx1 = lin_taps_f32(xs, W)
    y0, y1, wy0, wy1 = lin_taps_f32(ys, H)
    X0, X1, Y0, Y1 = wx0[None, :, None], wx1[None, :, None], wy0[:, None, None], wy1[:, None, None]
    r0, r1 = src[y0], src[y1]
    out = (r0[:, x0] * X0 + r0[:, x1] * X1) * Y0 + (r1[:, x0] * X0 + r1[:, x1] * X1) * Y1
    assert out.dtype == F32
    return out


def resample_f64(src, xs, ys):
    """Truth and its absolute terms.  A tap that is in range counts with its weight PLUS the size of the unnormalised position, because
    the two roundings of that position shift that much weight (relatively) between neighbouring taps; by continuity of the interpolant
    this also covers a float32 position that falls into the neighbouring cell."""
    s = np.asarray(src, np.float64)
    H, W, C = s.shape
    x0, x1, wx0, wx1, ix0, ix1, px = lin_taps_f64(xs, W)
    y0, y1, wy0, wy1, iy0, iy1, py = lin_taps_f64(ys, H)
    out = np.zeros((len(np.atleast_1d(ys)), len(np.atleast_1d(xs)), C))
    ab = np.zeros_like(out)
    for yi, wy, iny in ((y0, wy0, iy0), (y1, wy1, iy1)):
        for xi, wx, inx in ((x0, wx0, ix0), (x1, wx1, ix1)):
            tap = s[yi][:, xi]
            out += tap * (wy[:, None, None] * wx[None, :, None])
            ab += np.abs(tap) * (np.where(iny, wy + py, 0.0)[:, None, None] * np.where(inx, wx + px, 0.0)[None, :, None])
    return out, ab


# ---- 2x average pooling (k_avgpool, k_avgpool_many), src [H][W][C] -----------------------------------------------------------------------
K_AVGPOOL = 3    # three adds; * 0.25 (or 0.5) is exact


def avgpool_f32(src):
    src = np.ascontiguousarray(src, F32)
    H, W, C = src.shape
    Ho = H // 2
    if W == 1:
        out = (src[0:2 * Ho:2] + src[1:2 * Ho:2]) * F32(0.5)
    else:
        Wo = W // 2
        a, b = src[0:2 * Ho:2, 0:2 * Wo:2], src[0:2 * Ho:2, 1:2 * Wo:2]
        c, d = src[1:2 * Ho:2, 0:2 * Wo:2], src[1:2 * Ho:2, 1:2 * Wo:2]
        out = (((a + b) + c) + d) * F32(0.25)
    assert out.dtype == F32
    return out


def avgpool_f64(src):
    """The mean of each 2 x 2 block (2 x 1 for a line; a last odd row or column is dropped) in float64, and the absolute terms."""
    s = np.asarray(src, np.float64)
    H, W, C = s.shape
    Ho, Wo, kw = H // 2, (1 if W == 1 else W // 2), (1 if W == 1 else 2)
    blocks = lambda v: v[:2 * Ho, :kw * Wo].reshape(Ho, 2, Wo, kw, C).mean(axis=(1, 3))
    return blocks(s), blocks(np.abs(s))


def l1_input(n, seed=0):
    """Exact zeros, -0.0, denormals and +-large values among ordinary ones."""
    x = np.random.default_rng(seed).normal(size=n).astype(F32)
    if n == 1:
        x[0] = -0.75
        return x
    for start, step, val in ((0, 7, 0.0), (1, 11, -0.0), (2, 13, 1e-41), (3, 17, -1e-40), (4, 19, 3e30), (5, 23, -3e30)):
        x[start::step] = F32(val)
    return x


ADAM_SIZES = (0, 1, 255, 1023, 1024, 1025, 4097)
ADAM_COUNT = 83            # launches of 40, 40 and 3 tensors
ADAM_EMPTY = (5, 39, 82)   # a zero-size tensor inside a launch, last in a launch, last overall


def adam_sizes():
    n = [ADAM_SIZES[(3 * i + i // 7) % 7] for i in range(ADAM_COUNT)]
    for i in ADAM_EMPTY:
        n[i] = 0
    return n


def adam_lr(i):
    return float(F32(1e-3 * (1 + i % 7)))


def adam_grad(n, rng, flip):
    """Ordinary values over four decades with exact zeros, 1e-30, +-1e15 among them; `flip` changes every sign (between steps)."""
    g = (rng.normal(size=n) * 10.0 ** -rng.integers(0, 4, n)).astype(F32)
    for start, step, val in ((0, 5, 0.0), (1, 7, 1e-30), (2, 11, 1e15), (3, 13, -1e15)):
        g[start::step] = F32(val)
    return -g if flip else g


# ---- Adam (k_adam, k_adam_clock) ----------------------------------------------------------------------------------------------------------
K_ADAM_M = 4     # 1 - beta1, g - m, the product, the sum
K_ADAM_V = 5     # 1 - beta2, v * beta2, (1 - beta2) g, * g, the sum
K_ADAM_P = 16    # m (4), ss (1), denom: v (5, halved by the root, rounded up to 3), the root, bc2_sqrt, the division, + eps; m / denom, * ss, p - .


def adam_host_coeffs(lr, beta1, beta2, step):
    """ego_adam_step: ss = (float)((double)lr / (1 - pow((double)b1, t))), bc2_sqrt = (float)sqrt(1 - pow((double)b2, t))."""
    b1, b2 = float(F32(beta1)), float(F32(beta2))
    ss = F32(float(F32(lr)) / (1.0 - math.pow(b1, float(step))))
    return ss, F32(math.sqrt(1.0 - math.pow(b2, float(step))))


def adam_clock_f64(clock, beta1, beta2, lr_factor):
    """k_adam_clock on clock = [t, lr scale, lr scale / (1 - beta1^t), sqrt(1 - beta2^t)] -> the next clock (float64)."""
    b1, b2 = float(F32(beta1)), float(F32(beta2))
    t = clock[0] + 1.0
    return [t, clock[1] * lr_factor, clock[1] / (1.0 - math.pow(b1, t)), math.sqrt(1.0 - math.pow(b2, t))]


def adam_graph_coeffs(lr, clock):
    """k_adam with a clock: step_size = (float)((double)lr / 1.0), ss = (float)((double)step_size * clock[2]), bc2_sqrt = (float)clock[3]."""
    return F32(float(F32(lr)) * float(clock[2])), F32(float(clock[3]))


def adam_f32(p, g, m, v, ss, bc2_sqrt, beta1, beta2, eps):
    """One step of k_adam on float32 arrays -> p, m, v (float32, the kernel's bits)."""
    p, g, m, v = (np.ascontiguousarray(a, F32) for a in (p, g, m, v))
    b1, b2, eps, ss, bc2 = F32(beta1), F32(beta2), F32(eps), F32(ss), F32(bc2_sqrt)
    with np.errstate(over="ignore", under="ignore"):
        mi = m + (g - m) * (F32(1) - b1)
        vi = v * b2 + ((F32(1) - b2) * g) * g
        denom = np.sqrt(vi) / bc2 + eps
        pn = p - ss * (mi / denom)
    assert pn.dtype == F32 and mi.dtype == F32 and vi.dtype == F32
    return pn, mi, vi


def adam_f64(p, g, m, v, lr, beta1, beta2, eps, step):
    """torch.optim.Adam's recurrence in float64, one step from a float32 state -> p, m, v and the absolute terms of each."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2, eps, lr = float(F32(beta1)), float(F32(beta2)), float(F32(eps)), np.float64(F32(lr))   # lr: scalar or per element
    mi = m + (g - m) * (1.0 - b1)
    vi = v * b2 + (1.0 - b2) * g * g
    ss = lr / (1.0 - b1 ** step)
    denom = np.sqrt(vi) / math.sqrt(1.0 - b2 ** step) + eps
    m_abs = np.abs(m) + (np.abs(g) + np.abs(m)) * (1.0 - b1)
    p_abs = np.abs(p) + ss * m_abs / denom
    return p - ss * (mi / denom), mi, vi, p_abs, m_abs, vi


# ---- environment map (envmap_taps, envmap_lookup, k_envmap_bwd); emission [3][2h][h] --------------------------------------------------------
def envmap_taps_f32(dirs, h):
    d = np.ascontiguousarray(dirs, F32)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(under="ignore"):
        nrm = np.maximum(np.sqrt((dx * dx + dy * dy) + dz * dz), F32(1e-12))
        nx, ny, nz = dx / nrm, dy / nrm, dz / nrm
    u = (nz + F32(1)) * F32(0.5)
    v = (np.arctan2(ny, nx).astype(F32) + F32(math.pi)) / F32(2.0 * math.pi)
    return lin_taps_f32(u * F32(2) - F32(1), h), lin_taps_f32(v * F32(2) - F32(1), 2 * h)


def envmap_taps_f64(dirs, h):
    """models/envmap.py:26-34 in float64 from the float32 directions: F.normalize (eps 1e-12), u = (n_z + 1) / 2, v = (atan2 + pi) / 2 pi."""
    d = np.asarray(dirs, np.float64)
    nrm = np.maximum(np.sqrt((d * d).sum(1)), 1e-12)
    n = d / nrm[:, None]
    u = (n[:, 2] + 1.0) * 0.5
    v = (np.arctan2(n[:, 1], n[:, 0]) + math.pi) / (2.0 * math.pi)
    return lin_taps_f64(u * 2.0 - 1.0, h)[:4], lin_taps_f64(v * 2.0 - 1.0, 2 * h)[:4]


def _envmap_lookup(em, X, Y, dtype):
    em = np.asarray(em, dtype)
    (x0, x1, wx0, wx1), (y0, y1, wy0, wy1) = X, Y
    w00, w01, w10, w11 = wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1
    one = dtype(1)
    out = []
    for ch in range(3):
        E = em[ch]
        s = E[y0, x0] * w00 + E[y0, x1] * w01 + E[y1, x0] * w10 + E[y1, x1] * w11
        with np.errstate(over="ignore"):
            out.append(one / (one + np.exp(-s)))
    out = np.stack(out, 1)
    assert out.dtype == dtype
    return out


def envmap_lookup_f32(em, dirs):
    return _envmap_lookup(em, *envmap_taps_f32(dirs, em.shape[2]), F32)


def envmap_lookup_f64(em, dirs):
    return _envmap_lookup(em, *envmap_taps_f64(dirs, em.shape[2]), np.float64)


def _envmap_backward(h, X, Y, g_rgb, rgb_raw, bgw, env, dtype):
    """-> d(emission) [3][2h][h] summed in float64 (the order of the atomics is free), the per-texel sum of absolute contributions and
    the per-texel number of contributions."""
    g_rgb, rgb_raw, bgw, env = (np.asarray(a, dtype) for a in (g_rgb, rgb_raw, bgw, env))
    (x0, x1, wx0, wx1), (y0, y1, wy0, wy1) = X, Y
    out, ab, cnt = np.zeros((3, 2 * h, h)), np.zeros((3, 2 * h, h)), np.zeros((3, 2 * h, h))
    for ch in range(3):
        raw = rgb_raw[:, ch]
        g = np.where((raw >= 0) & (raw <= 1), g_rgb[:, ch], dtype(0))
        e = env[:, ch]
        ge = g * bgw * e * (dtype(1) - e)
        live = ge != 0
        for yi, wy in ((y0, wy0), (y1, wy1)):
            for xi, wx in ((x0, wx0), (x1, wx1)):
                c = (ge * wy * wx).astype(np.float64)
                np.add.at(out[ch], (yi[live], xi[live]), c[live])
                np.add.at(ab[ch], (yi[live], xi[live]), np.abs(c[live]))
                np.add.at(cnt[ch], (yi[live], xi[live]), 1.0)
    return out, ab, cnt


def envmap_backward_f32(h, dirs, g_rgb, rgb_raw, bgw, env):
    return _envmap_backward(h, *envmap_taps_f32(dirs, h), g_rgb, rgb_raw, bgw, env, F32)


def envmap_backward_f64(h, dirs, g_rgb, rgb_raw, bgw, env):
    return _envmap_backward(h, *envmap_taps_f64(dirs, h), g_rgb, rgb_raw, bgw, env, np.float64)


SEAM_MARGIN = 1e-3   # rad: no random direction comes closer to atan2 = +-pi


def envmap_dirs(seed=0, n_random=300):
    """The directions of tests/test_hip_envmap.py -> (dirs [N][3] float32, number of leading special rows).  Special rows: the poles, the
    seam with both signs of zero, the zero vector, unnormalised and tiny-norm vectors (clamped norm and not)."""
    r = np.random.default_rng(seed)
    special = np.array([[0, 0, 1], [0, 0, -1], [-1, 0.0, 0], [-1, -0.0, 0], [0, 0, 0], [30, -40, 120], [3e-7, 4e-7, -1e-6],
                        [1e-25, 2e-25, 3e-25], [-3e-19, 1e-19, 2e-19], [0, 5, 0], [2, 0, 0]], np.float32)
    d = r.normal(size=(4 * n_random, 3))
    d = d[np.pi - np.abs(np.arctan2(d[:, 1], d[:, 0])) > 10 * SEAM_MARGIN][:n_random]
    d *= r.uniform(0.2, 5.0, (len(d), 1))
    return np.concatenate([special, d.astype(np.float32)]), len(special)


def envmap_tolerance(own_err, truth):
    """The project's convention for kernels that call atan2f / expf (a few ulp each, the position error multiplied by the map's slope):
    4 x the error of the float32 restatement against truth on the same inputs, never less than 4 u max|truth|."""
    return 4.0 * max(float(own_err), U * float(np.abs(truth).max()))


# ---- the cases both the host test and the GPU tests run ---------------------------------------------------------------------------------
TV_SHAPES = ((1, 2, 2), (3, 2, 5), (16, 33, 2), (48, 65, 150), (16, 257, 256))   # (C, H, W); the last is one row past 2^20 elements
L1_SIZES = (1, 255, 256, 257, 2 ** 20 + 3)
ORTHO_SHAPES = ((2, 1), (3, 7), (16, 172), (48, 516), (64, 1036))               # (C, n)
RESAMPLE_SHAPES = ((1, 1, 1), (3, 5, 1), (16, 7, 9), (48, 4, 3))                # source (C, H, W)
AVGPOOL_SHAPES = ((2, 1, 1), (5, 1, 16), (2, 2, 3), (7, 9, 16), (33, 64, 48))   # (H, W, C)
RESAMPLE_SPECIAL = (-1.0, 1.0, -1.3, 1.3, float("nan"))


def table_input(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(F32)


def resample_axis(n, mode, rng):
    """Target positions on a source axis of n nodes: every node, -1, +1, +-1.3 (zero padding), a NaN; "up" adds a finer grid and random
    positions (some outside [-1, 1]), "down" a coarser grid."""
    parts = [np.linspace(-1.0, 1.0, n), RESAMPLE_SPECIAL]
    parts += [np.linspace(-1.0, 1.0, 2 * n + 2), rng.uniform(-1.1, 1.1, n + 3)] if mode == "up" else [np.linspace(-1.0, 1.0, max(n // 2, 1))]
    return np.concatenate([np.asarray(p, np.float64) for p in parts]).astype(F32)


def resample_cases():
    """-> [(name, src [H][W][C], xs, ys)]; a source with W = 1 is resampled in the line form (xs = [-1])."""
    out = []
    for k, (C, H, W) in enumerate(RESAMPLE_SHAPES):
        for mode in ("up", "down"):
            rng = np.random.default_rng(100 + k)
            ys = resample_axis(H, mode, rng)
            xs = np.array([-1.0], F32) if W == 1 else resample_axis(W, mode, rng)
            if (len(ys) * len(xs) * C) % 256 == 0:
                ys = np.concatenate([ys, np.array([0.25], F32)])
            out.append((f"{C}x{H}x{W}-{mode}", table_input((H, W, C), 200 + k), xs, ys))
    return out
