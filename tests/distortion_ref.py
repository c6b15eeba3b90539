"""numpy restatement of the distortion regulariser (csrc/ego_reg.hip states the formula; it is not in the reference), with the
arithmetic type as a parameter, plus the seeded inputs the host and the GPU tests share.

Two forms: `direct_value`, the O(S^2) double sum as written, and `kernel_model`, the kernel's algorithm: the transmittance by a
sequential product and the interval map in `dtype`, midpoints / widths / running sums in float64 whatever `dtype` is, the reverse
recurrence R in `dtype`.  With dtype = float64 it is the ground truth the GPU tests compare with; with float32 it says how far float32
arithmetic alone is from that on given inputs (the device differs from it by its logf and division and by tree-ordered scans)."""
import numpy as np

NEAR, FAR = 0.01, 15.0
SPACES = ("linear", "log", "disparity")


def intervals(z, near, far, space, dtype=np.float64):
    """z [N][S] ascending -> (m, delta) [N][S] float64: midpoint and width of sample i's interval [z_i, z_{i+1}], z_S = z_{S-1} +
    (z_{S-1} - z_{S-2}), mapped to [0, 1].  near / far enter as the float32 values the C ABI takes; the map's scale is rounded once
    from float64, as on the host side of the kernel."""
    t = np.dtype(dtype).type
    zt = np.asarray(z, np.float32).astype(t)
    ends = np.concatenate([zt, zt[:, -1:] + (zt[:, -1:] - zt[:, -2:-1])], axis=1)
    n, f = np.float64(np.float32(near)), np.float64(np.float32(far))
    span = {"linear": f - n, "log": np.log(f / n), "disparity": 1.0 / n - 1.0 / f}[space]
    scale = t(1.0 / span)
    if space == "linear":
        s = (ends - t(n)) * scale
    elif space == "log":
        s = np.log(np.maximum(ends, t(n)) / t(n)) * scale
    else:
        s = (t(1) / t(n) - t(1) / np.maximum(ends, t(n))) * scale
    assert s.dtype == np.dtype(dtype)
    s = s.astype(np.float64)
    return 0.5 * (s[:, :-1] + s[:, 1:]), s[:, 1:] - s[:, :-1]


def transmittance(a, dtype):
    """a [N][S] -> (T, f): T_i = prod_{j<i} f_j, f = 1 - a + 1e-10 (tensorBase.py:22-27), sequentially in `dtype`."""
    t = np.dtype(dtype).type
    a = a.astype(t)
    f = (t(1) - a) + t(1e-10)
    T, cur = np.empty_like(a), np.ones(a.shape[0], t)
    for i in range(a.shape[1]):
        T[:, i] = cur
        cur = cur * f[:, i]
    return T, f


def direct_value(alpha, m, delta, dtype=np.float64):
    """(1 / N) sum_rays [ sum_ij w_i w_j |m_i - m_j| + (1 / 3) sum_i w_i^2 delta_i ]: the [N][S][S] form."""
    S = m.shape[1]
    a = np.asarray(alpha)[:, :S]
    w = (a.astype(dtype) * transmittance(a, dtype)[0]).astype(np.float64)
    pair = (w[:, :, None] * w[:, None, :] * np.abs(m[:, :, None] - m[:, None, :])).sum((1, 2))
    return float((pair + (w * w * delta).sum(1) / 3.0).mean())


def kernel_model(alpha, m, delta, dtype=np.float64):
    """-> (value, g_alpha [N][alpha's columns]) by the O(S) form; columns at or beyond S get 0."""
    t = np.dtype(dtype).type
    alpha = np.asarray(alpha)
    N, S = m.shape
    a = alpha[:, :S].astype(t)
    T, f = transmittance(a, dtype)
    w = (a * T).astype(np.float64)
    wm = w * m
    W, WM = np.cumsum(w, 1), np.cumsum(wm, 1)
    W_lt, WM_lt = W - w, WM - wm
    W_gt, WM_gt = W[:, -1:] - W, WM[:, -1:] - WM
    value = float((2.0 * w * (m * W_lt - WM_lt) + w * w * delta / 3.0).sum(1).mean())
    G = (2.0 * (m * (W_lt - W_gt) - (WM_lt - WM_gt)) + (2.0 / 3.0) * w * delta).astype(t)
    R = np.zeros_like(G)
    for i in range(S - 2, -1, -1):
        R[:, i] = G[:, i + 1] * a[:, i + 1] + f[:, i + 1] * R[:, i + 1]
    g = np.zeros(alpha.shape, t)
    g[:, :S] = T * (G - R) * t(1.0 / N)
    return value, g


def distortion(alpha, z, space, dtype=np.float64, near=NEAR, far=FAR):
    """kernel_model on the intervals of z: (value, g_alpha)."""
    return kernel_model(alpha, *intervals(z, near, far, space, dtype), dtype=dtype)


def make_inputs(N, S, seed=0, trailing_ones=False):
    """The tests' inputs: z = near (far / near)^r with r sorted uniform and one tie per ray; alpha = 0.5 u^4 with row 0 all zero, an
    exact 1.0 in row 1, row 2 zero at every even sample and, for S >= 65, row 3's whole mass in two neighbours (the case in which
    float32 running sums cancel).  -> alpha [N][S (+1)], z [N][S], float32."""
    assert N >= 4 and S >= 2
    rng = np.random.default_rng(1000 * S + seed)
    r = np.sort(rng.uniform(size=(N, S)), axis=1)
    z = (NEAR * (FAR / NEAR) ** r).astype(np.float32)
    if S > 2:
        z[:, S // 2] = z[:, S // 2 - 1]
    alpha = (0.5 * rng.uniform(size=(N, S)) ** 4).astype(np.float32)
    alpha[0] = 0.0
    alpha[1, S // 3] = 1.0
    alpha[2, 0::2] = 0.0
    if S >= 65:
        alpha[3] = 0.0
        alpha[3, 40], alpha[3, 41] = 0.5, 1.0
    if trailing_ones:
        alpha = np.concatenate([alpha, np.ones((N, 1), np.float32)], axis=1)
    assert np.all(np.diff(z, axis=1) >= 0)
    return np.ascontiguousarray(alpha), z
