"""CPU: pins tests/table_ops_ref.py, the restatements the GPU tests of the table kernels compare with (test_hip_table_ops.py,
test_hip_adam.py, test_hip_envmap.py).  The float32 copies of the kernels stay within the derived running-error bound of the float64
forms, the float64 forms agree with torch (grid_sample, avg_pool2d, torch.optim.Adam, autograd), and the inputs have the properties the
GPU tests rely on (no Gram entry near zero, no direction near the seam but the ones placed on it)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from tests import table_ops_ref as R

SCALE = 0.75


def _frac(err, bnd):
    """The largest error as a fraction of its bound (both arrays or scalars)."""
    return float(np.max(np.abs(err) / bnd))


@pytest.mark.parametrize("shape", R.TV_SHAPES)
def test_tv_copy_within_bound_of_truth(shape):
    C, H, W = shape
    x = R.table_input((H, W, C), 1)
    terms, g, g_abs = R.tv_f32(x, SCALE)
    v64, g64 = R.tv_f64(x, SCALE)
    assert _frac(terms.astype(np.float64).sum() - v64, R.bound(R.K_TV_VALUE, v64)) <= 1.0
    assert _frac(g - g64, R.bound(R.K_TV_GRAD, g_abs)) <= 1.0
    # the closed form of the gradient that autograd must reproduce, on the corner texel (forward differences only)
    xd = x.astype(np.float64)
    ch, cw = 2.0 * SCALE / (C * (H - 1) * W), 2.0 * SCALE / (C * H * (W - 1))
    assert abs(g64[0, 0, 0] - 2 * (ch * (xd[0, 0, 0] - xd[1, 0, 0]) + cw * (xd[0, 0, 0] - xd[0, 1, 0]))) <= 1e-12 * abs(g64).max()


@pytest.mark.parametrize("n", R.L1_SIZES)
def test_l1_copy_within_bound_of_truth(n):
    x = R.l1_input(n)
    a, terms, g = R.l1_f32(x, SCALE)
    v64, g64 = R.l1_f64(x, SCALE)
    assert _frac(terms.astype(np.float64).sum() * float(a) - v64, R.bound(R.K_L1_VALUE, v64)) <= 1.0
    assert _frac(g - g64, R.bound(R.K_L1_GRAD, np.abs(g64))) <= 1.0
    if n > 1:   # the inputs hold what the GPU test is about
        assert (x == 0).any() and np.signbit(x[x == 0]).any() and (np.abs(x[x != 0]) < 1e-38).any() and (np.abs(x) > 1e30).any()
        assert (g[x == 0] == 0).all() and (np.abs(g[np.abs(x) < 1e-38][x[np.abs(x) < 1e-38] != 0]) == a).all()


@pytest.mark.parametrize("shape", R.ORTHO_SHAPES)
def test_ortho_copy_within_bound_and_signs_are_safe(shape):
    C, n = shape
    L = R.ortho_input(C, n, C)
    v, g, v_abs, g_abs, G = R.ortho_f32(L, SCALE)
    v64, g64, G64 = R.ortho_f64(L, SCALE)
    off = ~np.eye(C, dtype=bool)
    # no off-diagonal Gram entry is anywhere near zero, so float32 and float64 agree on every sign and no entry needs leaving out
    assert np.abs(G64[off]).min() >= 0.5 * np.abs(G64[off]).max()
    assert np.array_equal(np.sign(G[off]), np.sign(G64[off]))
    if C > 2:
        assert 0.3 <= (G64[off] < 0).mean() <= 0.7
    assert _frac(v - v64, R.bound(R.k_ortho_value(n), v_abs)) <= 1.0
    assert _frac(g - g64, R.bound(R.k_ortho_grad(C), g_abs)) <= 1.0


def test_ortho_disjoint_columns_have_an_exactly_zero_entry():
    L = R.ortho_disjoint_input()
    v, g, v_abs, g_abs, G = R.ortho_f32(L, SCALE)
    v64, g64, G64 = R.ortho_f64(L, SCALE)
    assert G[0, 1] == 0 and G64[0, 1] == 0 and G[0, 2] < 0 and G[1, 2] < 0
    assert _frac(v - v64, R.bound(R.k_ortho_value(len(L)), v_abs)) <= 1.0
    assert _frac(g - g64, R.bound(R.k_ortho_grad(3), g_abs)) <= 1.0
    # column 0 gets nothing from column 1: its gradient is -sign * column 2 alone
    assert np.allclose(g64[:, 0], -SCALE * 2 / 6 * L[:, 2].astype(np.float64), rtol=1e-12, atol=0)


def _grid_sample_f64(src, xs, ys):
    t = torch.from_numpy(np.asarray(src, np.float64)).permute(2, 0, 1)[None]
    gx, gy = torch.from_numpy(np.asarray(xs, np.float64)), torch.from_numpy(np.asarray(ys, np.float64))
    grid = torch.stack([gx[None, :].expand(len(gy), -1), gy[:, None].expand(-1, len(gx))], -1)[None]
    return Fn.grid_sample(t, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("case", R.resample_cases(), ids=lambda c: c[0])
def test_resample_copy_within_bound_and_truth_is_grid_sample(case):
    name, src, xs, ys = case
    o32, (o64, ab) = R.resample_f32(src, xs, ys), R.resample_f64(src, xs, ys)
    assert not np.isnan(o32).any() and not np.isnan(o64).any()          # a NaN position reads as zero
    assert _frac(o32 - o64, R.bound(R.K_RESAMPLE, ab)) <= 1.0
    fin_x, fin_y = ~np.isnan(xs), ~np.isnan(ys)
    ref = _grid_sample_f64(src, xs[fin_x], ys[fin_y])
    assert np.abs(o64[fin_y][:, fin_x] - ref).max() <= 1e-13 * max(np.abs(src).max(), 1.0)
    assert (o64[~fin_y] == 0).all() and (o64[:, ~fin_x] == 0).all() and (o32[~fin_y] == 0).all() and (o32[:, ~fin_x] == 0).all()
    assert (len(xs) * len(ys) * src.shape[2]) % 256 != 0
    if src.shape[0] > 1:   # exactly on +-1: the edge nodes (+-1.3 is less than a cell outside on these axes: grid_sample above decides)
        k = 0 if src.shape[1] == 1 else int(np.flatnonzero(xs == -1)[0])
        assert np.array_equal(o32[np.flatnonzero(ys == 1)[0], k], src[-1, 0]) and np.array_equal(o32[np.flatnonzero(ys == -1)[0], k], src[0, 0])


def test_lin_taps_rules():
    i0, i1, w0, w1 = R.lin_taps_f32(np.array([-1, 1, 0, float("nan"), -1.3, 1.3, -1.1], np.float32), 9)
    assert i0.tolist() == [0, 8, 4, 0, 0, 8, 0] and i1.tolist() == [1, 8, 5, 0, 0, 8, 0]
    assert w0.tolist()[:6] == [1, 1, 1, 0, 0, 0] and w1.tolist()[:6] == [0, 0, 0, 0, 0, 0]
    assert w0[6] == 0 and abs(w1[6] - 0.6) < 1e-6                        # half a cell outside: the in-range tap keeps its weight
    i0, i1, w0, w1 = R.lin_taps_f32(np.array([-1, 0.3], np.float32), 1)   # a one-node axis: the node, whatever the position
    assert i0.tolist() == [0, 0] and w0.tolist() == [1, 1] and w1.tolist() == [0, 0]


@pytest.mark.parametrize("shape", R.AVGPOOL_SHAPES)
def test_avgpool_copy_within_bound_and_truth_is_avg_pool2d(shape):
    H, W, C = shape
    s = R.table_input(shape, 3)
    o32, (o64, ab) = R.avgpool_f32(s), R.avgpool_f64(s)
    assert o32.shape == (H // 2, 1 if W == 1 else W // 2, C)
    assert _frac(o32 - o64, R.bound(R.K_AVGPOOL, ab)) <= 1.0
    k = (2, 1) if W == 1 else 2
    ref = Fn.avg_pool2d(torch.from_numpy(s.astype(np.float64)).permute(2, 0, 1)[None], k, stride=k)[0].permute(1, 2, 0).numpy()
    assert np.abs(o64 - ref).max() <= 1e-15 * np.abs(s).max()


ADAM_SETTINGS = [((0.9, 0.99), 1e-8), ((0.9, 0.99), 1e-15), ((0.0, 0.5), 1e-8), ((0.0, 0.5), 1e-15)]
ADAM_STEPS = (1, 2, 10, 1000, 10 ** 6)


@pytest.mark.parametrize("betas,eps", ADAM_SETTINGS)
def test_adam_copy_within_bound_of_truth(betas, eps):
    rng = np.random.default_rng(7)
    n = 4097
    p, m, v = rng.normal(size=n).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst = 0.0
    for k, step in enumerate(ADAM_STEPS):
        g, lr = R.adam_grad(n, rng, k % 2), R.adam_lr(k)
        ss, bc2 = R.adam_host_coeffs(lr, *betas, step)
        pn, mn, vn = R.adam_f32(p, g, m, v, ss, bc2, *betas, eps)
        p64, m64, v64, p_abs, m_abs, v_abs = R.adam_f64(p, g, m, v, lr, *betas, eps, step)
        assert np.isfinite(pn).all() and np.isfinite(vn).all()
        worst = max(worst, _frac(pn - p64, R.bound(R.K_ADAM_P, p_abs)), _frac(mn - m64, R.bound(R.K_ADAM_M, m_abs)),
                    _frac(vn - v64, R.bound(R.K_ADAM_V, v_abs)))
        p, m, v = pn, mn, vn
    assert worst <= 1.0, worst
    assert R.adam_host_coeffs(1.0, *betas, 10 ** 6) == (np.float32(1), np.float32(1))   # 1 - beta^t has rounded to 1


def test_adam_truth_is_torch_adam_and_the_clock_follows_the_host():
    rng = np.random.default_rng(8)
    b1, b2, eps, lr = float(np.float32(0.9)), float(np.float32(0.99)), float(np.float32(1e-8)), float(np.float32(0.02))
    p = rng.normal(size=300)
    t = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([t], lr=lr, betas=(b1, b2), eps=eps)
    m, v, clock = np.zeros(300), np.zeros(300), [0.0, 1.0, 0.0, 0.0]
    for step in range(1, 7):
        g = rng.normal(size=300) * 10.0 ** -(step % 3)
        t.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = R.adam_f64(p, g, m, v, lr, b1, b2, eps, step)[:3]
        assert np.abs(p - t.detach().numpy()).max() <= 1e-13
        # the device clock's coefficients are the host path's: lr scale / (1 - beta1^t) and sqrt(1 - beta2^t), the decay following the step
        scale = clock[1]
        clock = R.adam_clock_f64(clock, b1, b2, 0.977)
        assert clock[0] == step and clock[1] == scale * 0.977
        ss_host, bc2_host = R.adam_host_coeffs(lr * scale, b1, b2, step)
        ss_clock, bc2_clock = R.adam_graph_coeffs(lr, clock)
        assert bc2_clock == bc2_host and abs(float(ss_clock) - float(ss_host)) <= 2 * R.U * float(ss_host)
    assert abs(clock[1] - 0.977 ** 6) <= 1e-15


def test_adam_case_layout():
    n = R.adam_sizes()
    assert len(n) == 83 and set(n) == set(R.ADAM_SIZES) and all(n[i] == 0 for i in R.ADAM_EMPTY)
    assert R.ADAM_EMPTY == (5, 39, 82) and n[4] > 0 and n[6] > 0 and n[40] > 0 and len({R.adam_lr(i) for i in range(83)}) == 7


@pytest.mark.parametrize("h", [2, 5, 16])
def test_envmap_copy_is_close_and_truth_is_grid_sample(h):
    dirs, n_special = R.envmap_dirs()
    em = R.table_input((3, 2 * h, h), h) * 2
    o32, o64 = R.envmap_lookup_f32(em, dirs), R.envmap_lookup_f64(em, dirs)
    own = np.abs(o32 - o64).max()
    # not zero: inputs on which float32 shows (the GPU test's tolerance is 4 x this figure).  The ceiling is no tolerance of a kernel, only
    # a guard against a copy that restates another operation: a wrong tap or weight moves a value by ~0.1, rounding by ~h u x the slope
    assert 0 < own <= 1e-4
    # models/envmap.py:6-14, 26-34 with torch in float64
    d = torch.from_numpy(dirs.astype(np.float64))
    n = Fn.normalize(d, dim=-1)
    uv = torch.stack([(n[:, 2] + 1) * 0.5, (torch.atan2(n[:, 1], n[:, 0]) + math.pi) / (2 * math.pi)], 1) * 2 - 1
    ref = torch.sigmoid(Fn.grid_sample(torch.from_numpy(em.astype(np.float64))[None], uv[None, :, None], align_corners=True))[0, :, :, 0].T.numpy()
    assert np.abs(o64 - ref).max() <= 1e-13
    # the backward restatement in float64 is autograd's gradient of that expression
    rng = np.random.default_rng(h)
    g_rgb, bgw = rng.normal(size=(len(dirs), 3)), rng.uniform(0, 1, len(dirs))
    raw = rng.uniform(-0.2, 1.2, (len(dirs), 3))
    E = torch.from_numpy(em.astype(np.float64)).requires_grad_(True)
    env = torch.sigmoid(Fn.grid_sample(E[None], uv[None, :, None], align_corners=True))[0, :, :, 0].T
    mask = torch.from_numpy(((raw >= 0) & (raw <= 1)).astype(np.float64))
    (env * torch.from_numpy(bgw)[:, None] * mask * torch.from_numpy(g_rgb)).sum().backward()
    got, ab, cnt = R.envmap_backward_f64(h, dirs, g_rgb, raw, bgw, o64)
    assert np.abs(got - E.grad.numpy()).max() <= 1e-12 * np.abs(got).max()
    b32 = R.envmap_backward_f32(h, dirs, g_rgb, raw, bgw, o32)[0]
    assert 0 < np.abs(b32 - got).max() <= 1e-4 * np.abs(got).max()


def test_envmap_directions_keep_off_the_seam():
    dirs, n_special = R.envmap_dirs()
    assert len(dirs) - n_special >= 200
    d = dirs.astype(np.float64)
    phi = np.arctan2(d[:, 1], d[:, 0])
    near = np.pi - np.abs(phi) < R.SEAM_MARGIN
    on = np.flatnonzero(near)
    assert on.tolist() == [2, 3]                                        # only the two placed on it exactly ...
    assert dirs[2].tolist() == [-1, 0, 0] and dirs[3].tolist() == [-1, 0, 0] and not np.signbit(dirs[2, 1]) and np.signbit(dirs[3, 1])
    (x32, y32), (x64, y64) = R.envmap_taps_f32(dirs[2:4], 5), R.envmap_taps_f64(dirs[2:4], 5)
    assert y32[0].tolist() == [9, 0] and y32[2].tolist() == [1, 1] and y64[0].tolist() == [9, 0]    # ... landing on opposite edges, no wrap
    # poles: u = 1 and u = 0 exactly; the zero vector and the clamped tiny one: the middle of the map
    xp, _ = R.envmap_taps_f32(dirs[[0, 1, 4]], 5)
    assert xp[0].tolist() == [4, 0, 2] and xp[2].tolist() == [1, 1, 1]
