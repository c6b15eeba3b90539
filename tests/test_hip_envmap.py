"""GPU: the environment map's lookup (ego_envmap_radiance) and its backward into the emission (ego_envmap_backward) against float64
truth (tests/table_ops_ref.py) where 64 rays of one scene never go: the poles, the seam with both signs of zero (opposite edges of the
map, no wrap, as in the reference), the zero direction, unnormalised and tiny-norm directions, `dir_stride` 3 and 6, the clamp-backward
mask at `raw` exactly 0 and 1, `bg_weight` 0, and 4096 rays adding into the same texels.

These kernels call atan2f and expf (a few ulp each), and the position error is multiplied by the map's slope, so the tolerance follows
the project's convention for such kernels: 4 x the error of the float32 restatement against truth on the same inputs, measured at run
time, never less than 4 u max|truth|.  The gradient adds the running-error bound of its float atomics, whose order is free: gamma_n
times the sum of absolute contributions of a texel with n contributions."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib
from tests import table_ops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_SHARED = 4096


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inputs(h):
    dirs, n_special = R.envmap_dirs()
    shared = np.tile(np.array([[0.3, -0.5, 0.4]], np.float32), (N_SHARED, 1))      # one direction: its four texels take all the atomics
    dirs = np.concatenate([dirs, shared])
    N = len(dirs)
    rng = np.random.default_rng(40 + h)
    em = R.table_input((3, 2 * h, h), h) * 2
    g_rgb = rng.normal(size=(N, 3)).astype(np.float32)
    lo, hi = np.nextafter(np.float32(0), np.float32(-1)), np.nextafter(np.float32(1), np.float32(2))
    raw = np.array([0.0, 1.0, lo, hi, 0.5, -0.3, 1.7, 0.25], np.float32)[(np.arange(N * 3) * 5 // 3) % 8].reshape(N, 3)
    bgw = rng.uniform(0.05, 1.0, N).astype(np.float32)
    bgw[::9] = 0
    return dirs, n_special, em, g_rgb, raw, bgw


def _scene(em_dev, h):
    sc = _lib.new_scene()
    sc.envmap, sc.envmap_h = (None if em_dev is None else em_dev.data_ptr()), h
    return sc


def _backward(h, dirs_dev, ptr, stride, g_rgb, raw, bgw, env_dev, N):
    g_em = torch.zeros(3 * 2 * h * h + 1, device=DEV)
    g_em[-1] = 777.0
    keep = [dev(g_rgb), dev(raw), dev(bgw)]
    _lib.check(_lib.load().ego_envmap_backward(_scene(None, h), ptr, stride, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(),
                                               env_dev.data_ptr(), N, g_em.data_ptr(), _lib.stream_handle()), "ego_envmap_backward")
    torch.cuda.synchronize()
    out = g_em.cpu().numpy()
    assert out[-1] == 777.0
    return out[:-1].reshape(3, 2 * h, h).astype(np.float64)


@pytest.mark.parametrize("h", [2, 5, 16])
def test_envmap_lookup_and_backward(h):
    dirs, n_special, em, g_rgb, raw, bgw = _inputs(h)
    N = len(dirs)
    em_dev, dirs_dev = dev(em), dev(dirs)
    env_dev = torch.empty(N, 3, device=DEV)
    _lib.check(_lib.load().ego_envmap_radiance(_scene(em_dev, h), dirs_dev.data_ptr(), N, env_dev.data_ptr(), _lib.stream_handle()),
               "ego_envmap_radiance")
    torch.cuda.synchronize()
    got = env_dev.cpu().numpy()
    copy, truth = R.envmap_lookup_f32(em, dirs), R.envmap_lookup_f64(em, dirs)
    own = float(np.abs(copy - truth).max())
    assert own > 0                                   # inputs on which float32 shows at all
    tol = R.envmap_tolerance(own, truth)
    err = np.abs(got - truth)
    print(f"envmap h={h}: lookup |hip - f64| {err.max():.3e} (special rows {err[:n_special].max():.3e})  |copy - f64| {own:.3e}  "
          f"tolerance {tol:.3e}  fraction {err.max() / tol:.3f}")
    assert err.max() <= tol
    # the seam rows: +0 and -0 land on opposite edges of the 2h axis, and do not wrap
    E = em.astype(np.float64)
    sig = lambda s: 1.0 / (1.0 + np.exp(-s))
    mid = 0.5 * (h - 1)
    edge = lambda row: sig(E[:, row, int(np.floor(mid))] * (1 - (mid % 1)) + E[:, row, int(np.ceil(mid))] * (mid % 1))
    assert np.abs(got[2] - edge(2 * h - 1)).max() <= tol and np.abs(got[3] - edge(0)).max() <= tol

    # backward: the kernel gets its own forward output, the restatements theirs
    truth_b, ab, cnt = R.envmap_backward_f64(h, dirs, g_rgb, raw, bgw, truth)
    copy_b = R.envmap_backward_f32(h, dirs, g_rgb, raw, bgw, copy)[0]
    own_b = float(np.abs(copy_b - truth_b).max())
    assert own_b > 0 and cnt.max() >= 1000
    tol_b = R.envmap_tolerance(own_b, truth_b) + R.gamma(cnt) * ab
    rays = np.zeros((N, 6), np.float32)
    rays[:, :3], rays[:, 3:] = 9.0, dirs             # a wrong stride or offset would read the origins
    rays_dev = dev(rays)
    for stride, ptr in ((3, dirs_dev.data_ptr()), (6, rays_dev.data_ptr() + 12)):
        got_b = _backward(h, dirs_dev, ptr, stride, g_rgb, raw, bgw, env_dev, N)
        f = float(np.max(np.abs(got_b - truth_b) / tol_b))
        print(f"envmap h={h} stride {stride}: backward |hip - f64| {np.abs(got_b - truth_b).max():.3e}  |copy - f64| {own_b:.3e}  "
              f"largest fraction of the tolerance {f:.3f}  (most contributions to one texel: {int(cnt.max())})")
        assert f <= 1.0
    # bg_weight = 0 everywhere, or every raw value outside [0, 1]: nothing arrives
    assert not _backward(h, dirs_dev, dirs_dev.data_ptr(), 3, g_rgb, raw, np.zeros_like(bgw), env_dev, N).any()
    assert not _backward(h, dirs_dev, dirs_dev.data_ptr(), 3, g_rgb, np.full_like(raw, 1.0000001), bgw, env_dev, N).any()
