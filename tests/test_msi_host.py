"""CPU: the host side of multi-sphere images (egonerf_amd/msi.py) and the float64 restatement the GPU tests compare the kernels with
(tests/msi_ref.py): layer bounds, the telescoping identity behind the bake, the .npz round trip, argument errors, the exported symbols."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth
from egonerf_amd.coordinates import YinYangSphericalCoords
from egonerf_amd.msi import MultiSphereImage, bake_msi, layer_bounds
from tests import msi_ref

UNEVEN = [1, 32, 31, 32]


def owners(bounds, z):
    """For every z the layers k with bounds[k] <= z < bounds[k + 1], compared in float32 as the kernel does."""
    z = np.asarray(z, np.float32)
    return [(np.flatnonzero((bounds[:-1] <= v) & (v < bounds[1:]))).tolist() for v in z]


def model_schedule(S):
    """near + r_sched of the tiny test scene's eval schedule: what bake_msi hands to layer_bounds."""
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    co = YinYangSphericalCoords("cpu", torch.from_numpy(cfg.aabb), exp_r=True, N_voxel=cfg.n_voxel, r0=cfg.r0, interval_th=cfg.interval_th)
    return (np.float32(cfg.near) + co.sample_schedule(cfg.near, cfg.far, S).numpy().astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("S,L,runs", [(96, 4, None), (96, 4, UNEVEN), (128, 16, None), (64, 7, None), (64, 64, None), (5, 1, None)])
def test_layer_bounds_partition_the_schedule(S, L, runs):
    z = model_schedule(S)
    bounds, radii = layer_bounds(z, L, runs)
    assert bounds.dtype == np.float32 and radii.dtype == np.float32 and bounds.shape == (L + 1,) and radii.shape == (L,)
    assert np.all(np.diff(bounds) > 0) and np.all(np.diff(radii) > 0) and radii[0] > 0
    assert bounds[0] == z[0] and bounds[-1] > z[-1]
    if runs is None:   # the default: equal counts
        runs = [S // L + (1 if k < S % L else 0) for k in range(L)]
        assert sum(runs) == S and max(runs) - min(runs) <= 1
    assert owners(bounds, z) == [[k] for k in np.repeat(np.arange(L), runs)]   # exactly one layer each, the runs as asked
    start = np.concatenate([[0], np.cumsum(runs)])
    for k in range(L):
        first, last = float(z[start[k]]), float(z[start[k + 1] - 1])
        assert radii[k] == np.float32(np.sqrt(first * last)) and first <= radii[k] <= last
        if 0 < k:
            assert bounds[k] == np.float32(0.5 * (float(z[start[k] - 1]) + first))   # the midpoint between the runs


def test_layer_bounds_refuses_bad_input():
    z = model_schedule(32)
    for bad in (lambda: layer_bounds(z, 0), lambda: layer_bounds(z, 33), lambda: layer_bounds(z, 4, [8, 8, 8]), lambda: layer_bounds(z, 4, [8, 8, 8, 9]),
                lambda: layer_bounds(z, 4, [0, 16, 8, 8]), lambda: layer_bounds(z[::-1], 4), lambda: layer_bounds(np.array([1.0, 1.0, 2.0]), 2),
                lambda: layer_bounds(np.array([0.0, 1.0, 2.0]), 3), lambda: layer_bounds(np.array([1.0, np.nan, 2.0]), 2)):
        with pytest.raises(ValueError):
            bad()
    assert layer_bounds(torch.from_numpy(z), 4)[0].tolist() == layer_bounds(z, 4)[0].tolist()   # a tensor is taken as well


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_telescoping_identity(seed):
    """The over-composite of the L layers equals sum_i w_i c_i over all samples, w from the plain cumulative product: within a layer
    t restarts at 1, and the product of the layers' (1 - A) is the transmittance in front of the next one."""
    rng = np.random.default_rng(seed)
    N, S = 50, 96
    z = np.sort(rng.uniform(0.1, 20.0, (N, S)), axis=1)   # a different ascending schedule per ray
    bounds = np.array([0.1, 0.5, 3.0, 9.0, 20.5, 30.0])     # uneven; the last layer is empty
    alpha = rng.uniform(0, 1, (N, S))
    alpha[rng.uniform(size=(N, S)) < 0.15] = 0.0
    alpha[rng.uniform(size=(N, S)) < 0.05] = 1.0
    alpha[7] = 0.0
    rgb = rng.uniform(0, 1, (N, S, 3))
    layers = msi_ref.msi_layers(z, alpha, rgb, bounds, np.float64)
    assert layers.dtype == np.float64 and np.all(layers[-1] == 0) and np.all(layers[:, 7] == 0)
    T = np.cumprod(np.concatenate([np.ones((N, 1)), 1 - alpha[:, :-1]], axis=1), axis=1)
    direct = ((alpha * T)[..., None] * rgb).sum(1)
    assert np.abs(msi_ref.over_composite(layers) - direct).max() <= 1e-12
    acc = 1 - np.prod(1 - layers[..., 3], axis=0)
    assert np.abs(acc - (alpha * T).sum(1)).max() <= 1e-12


def test_restatement_runs_in_float32_operation_by_operation():
    rng = np.random.default_rng(3)
    N, S = 9, 24
    z = np.sort(rng.uniform(0.1, 5.0, (N, S)).astype(np.float32), axis=1)
    alpha, rgb = rng.uniform(0, 1, (N, S)).astype(np.float32), rng.uniform(0, 1, (N, S, 3)).astype(np.float32)
    bounds = np.array([0.1, 1.0, 2.5, 6.0], np.float32)
    l32, l64 = msi_ref.msi_layers(z, alpha, rgb, bounds, np.float32), msi_ref.msi_layers(z, alpha, rgb, bounds, np.float64)
    assert l32.dtype == np.float32 and 0 < np.abs(l32 - l64).max() <= 26 * 2.0 ** -23
    rays = np.concatenate([rng.uniform(-0.2, 0.2, (N, 3)), rng.normal(size=(N, 3))], 1)
    rays[:, 3:] /= np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
    rays = rays.astype(np.float32)
    tex = rng.uniform(0, 1, (3, 8, 16, 4)).astype(np.float16)
    radii = np.array([1.0, 2.0, 4.0], np.float32)
    (c32, d32), (c64, d64) = (msi_ref.msi_render(rays, [0, 0, 0], radii, tex, tex[0], dt) for dt in (np.float32, np.float64))
    assert c32.dtype == np.float32 and d32.dtype == np.float32 and c64.dtype == np.float64
    assert 0 < np.abs(c32 - c64).max() < 1e-4 and np.abs(d32 - d64).max() < 1e-4


def small_image(dtype=torch.float16, background=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    layers = torch.rand(3, 4, 8, 4, generator=g).to(dtype)
    bg = torch.rand(4, 8, 4, generator=g).to(dtype) if background else None
    return MultiSphereImage(layers, [0.5, 1.5, 4.0], [0.25, 1.0, 2.5, 6.0], [0.1, -0.2, 0.3], [0.01, 15.0], bg)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("background", [True, False])
def test_npz_round_trip_is_bit_equal(tmp_path, dtype, background):
    msi = small_image(dtype, background)
    path = tmp_path / "image.npz"
    msi.save(path)
    with np.load(path, allow_pickle=False) as f:   # plain arrays only: nothing in the file needs pickle
        assert sorted(f.files) == sorted(["layers", "radii", "bounds", "center", "near_far"] + (["background"] if background else []))
        assert f["layers"].dtype == (np.float16 if dtype == torch.float16 else np.float32)
    back = MultiSphereImage.load(path, "cpu")
    assert back.layers.dtype == dtype and torch.equal(back.layers.view(torch.uint8), msi.layers.view(torch.uint8))
    assert (back.background is None) == (not background)
    if background:
        assert torch.equal(back.background.view(torch.uint8), msi.background.view(torch.uint8))
    assert torch.equal(back.radii, msi.radii) and torch.equal(back.bounds, msi.bounds)
    assert back.center.tobytes() == msi.center.tobytes() and back.near_far == msi.near_far
    assert (back.L, back.Hm, back.Wm) == (3, 4, 8)


def test_half_and_float():
    msi = small_image(torch.float32)
    h = msi.half()
    assert h.layers.dtype == torch.float16 and h.background.dtype == torch.float16 and msi.float() is msi and h.half() is h
    assert torch.equal(h.layers, msi.layers.half()) and torch.equal(h.float().layers, msi.layers.half().float())
    assert torch.equal(h.radii, msi.radii) and h.near_far == msi.near_far


def test_argument_errors():
    L, Hm, Wm = 3, 4, 8
    ok = dict(radii=[0.5, 1.5, 4.0], bounds=[0.25, 1.0, 2.5, 6.0], center=[0, 0, 0], near_far=[0.01, 15.0])
    tex = torch.zeros(L, Hm, Wm, 4, dtype=torch.float16)
    for exc, kw in ((ValueError, dict(layers=tex.double())), (ValueError, dict(layers=tex.numpy())), (IndexError, dict(layers=tex[..., :3])),
                    (IndexError, dict(layers=tex[0])), (ValueError, dict(layers=tex.transpose(1, 2))),
                    (ValueError, dict(background=torch.zeros(Hm, Wm, 4))), (IndexError, dict(background=tex[0, :2])),
                    (ValueError, dict(background=torch.zeros(Wm, Hm, 4, dtype=torch.float16).transpose(0, 1))), (IndexError, dict(radii=[0.5, 1.5])),
                    (IndexError, dict(bounds=[0.25, 1.0, 2.5])), (ValueError, dict(radii=[0.5, 0.5, 4.0])), (ValueError, dict(radii=[0.0, 1.5, 4.0])),
                    (ValueError, dict(radii=[0.5, float("nan"), 4.0])), (ValueError, dict(bounds=[0.25, 2.5, 1.0, 6.0])),
                    (ValueError, dict(center=[0, 0])), (ValueError, dict(center=[0, float("inf"), 0])), (ValueError, dict(near_far=[0.1]))):
        with pytest.raises(exc):
            MultiSphereImage(**{"layers": tex, **ok, **kw})
    msi = MultiSphereImage(tex, **ok)
    with pytest.raises(ValueError, match="no CPU fallback"):   # an image in host memory holds, converts and saves; it does not render
        msi.render(torch.zeros(5, 6))
    with pytest.raises(ValueError, match="no CPU fallback"):
        msi(torch.zeros(5, 6), need_alpha=False, n_coarse=8)


def test_ray_checks_come_before_any_pointer_is_handed_over():
    from egonerf_amd.msi import _check_rays
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="device tensor"):
        _check_rays(torch.zeros(5, 6), dev, "t")
    with pytest.raises(ValueError, match="device tensor"):
        _check_rays(np.zeros((5, 6), np.float32), dev, "t")


def test_bake_refuses_bad_arguments_before_touching_the_model():
    class Host(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

    for kw in (dict(dtype=torch.float64), dict(Hm=0), dict(chunk=0), dict(L=0), dict(L=65), dict(n_samples=1)):
        with pytest.raises(ValueError):
            bake_msi(Host(), **{**dict(Hm=4, Wm=8, L=4, n_samples=64), **kw})
    with pytest.raises(ValueError, match="HIP device"):
        bake_msi(Host(), 4, 8, 4, 64)


def test_library_refuses_bad_arguments_before_anything_is_queued():
    lib = _lib.load()
    one = 16   # a non-null, texel-aligned address: every call below fails its size checks first
    assert lib.ego_msi_layers(one, one, 0, one, 4, 8, one, 0, 0, 4, _lib.MSI_F32, one, None) == -1 and b"msi_layers" in lib.ego_last_error()
    assert lib.ego_msi_layers(one, one, 4, one, 4, 8, one, 2, 0, 4, _lib.MSI_F32, one, None) == -1   # alpha_stride < S
    assert lib.ego_msi_layers(one, one, 0, one, 4, 8, one, 2, 1, 4, _lib.MSI_F32, one, None) == -1   # [first, first + N) outside the image
    assert lib.ego_msi_layers(one, one, 0, one, 4, 8, one, 2, 0, 4, 2, one, None) == -1              # unknown texel type
    assert lib.ego_msi_layers(None, one, 0, one, 4, 8, one, 2, 0, 4, _lib.MSI_F32, one, None) == -1 and b"null" in lib.ego_last_error()
    assert lib.ego_msi_layers(one, one, 0, one, 4, 8, one, 2, 0, 4, _lib.MSI_F32, 24, None) == -1 and b"aligned" in lib.ego_last_error()
    assert lib.ego_msi_layers(None, None, 0, None, 0, 8, None, 2, 0, 4, _lib.MSI_F32, None, None) == 0   # N == 0: a no-op
    assert lib.ego_msi_render(one, 4, 0.0, 0.0, 0.0, one, 0, 4, 8, _lib.MSI_F16, one, None, one, one, None) == -1 and b"msi_render" in lib.ego_last_error()
    assert lib.ego_msi_render(one, 4, 0.0, 0.0, 0.0, one, 2, 0, 8, _lib.MSI_F16, one, None, one, one, None) == -1
    assert lib.ego_msi_render(one, 4, float("nan"), 0.0, 0.0, one, 2, 4, 8, _lib.MSI_F16, one, None, one, one, None) == -1
    assert lib.ego_msi_render(one, 4, 0.0, 0.0, 0.0, one, 2, 4, 8, 7, one, None, one, one, None) == -1
    assert lib.ego_msi_render(one, 4, 0.0, 0.0, 0.0, one, 2, 4, 8, _lib.MSI_F16, None, None, one, one, None) == -1 and b"null" in lib.ego_last_error()
    assert lib.ego_msi_render(12, 4, 0.0, 0.0, 0.0, one, 2, 4, 8, _lib.MSI_F16, one, None, one, one, None) == -1 and b"aligned" in lib.ego_last_error()
    assert lib.ego_msi_render(one, 4, 0.0, 0.0, 0.0, one, 2, 4, 8, _lib.MSI_F32, one, 8, one, one, None) == -1 and b"aligned" in lib.ego_last_error()
    assert lib.ego_msi_render(None, 0, 0.0, 0.0, 0.0, None, 2, 4, 8, _lib.MSI_F16, None, None, None, None, None) == 0     # N == 0: a no-op


def test_symbols_are_declared_and_exported():
    lib = _lib.load()
    for name in ("ego_msi_layers", "ego_msi_render"):
        assert name in _lib.header_symbols() and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.ego_abi_version() == 17 == _lib.EXPECTED_ABI_VERSION
    import egonerf_amd
    assert "msi" in egonerf_amd.__all__
