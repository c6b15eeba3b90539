"""CPU: the host side of differentiable playback and texel refinement (egonerf_amd/msi.py: MultiSphereImage.render with grad, refine_msi;
csrc/ego_msi.hip: ego_msi_render_backward, ego_msi_project) and the autograd restatement the GPU tests compare the backward kernel with
(tests/msi_grad_ref.py)."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib
from egonerf_amd.msi import MultiSphereImage, refine_msi
from tests import msi_grad_ref, msi_ref

CENTER = np.asarray([0.25, -0.5, 0.125], np.float32)


def random_rays(g, n, reach):
    o = g.standard_normal((n, 3))
    o *= (reach * g.uniform(0, 1, (n, 1)) ** (1 / 3)) / np.linalg.norm(o, axis=1, keepdims=True)
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o + CENTER, d], 1).astype(np.float32)


@pytest.mark.parametrize("with_background", [False, True])
def test_restatement_forward_is_msi_ref(with_background):
    g = np.random.default_rng(1)
    radii = np.asarray([1.0, 1.7, 3.0], np.float32)
    rays = random_rays(g, 200, 1.5)   # some eyes lie beyond the first shell
    layers = g.uniform(0, 1, (3, 5, 7, 4)).astype(np.float32)
    bg = g.uniform(0, 1, (5, 7, 4)).astype(np.float32) if with_background else None
    assert (np.linalg.norm(rays[:, :3] - CENTER, axis=1) > 1.0).any()
    want, want_d = msi_ref.msi_render(rays, CENTER, radii, layers, bg, np.float64)
    got, got_d = msi_grad_ref.msi_render(rays, CENTER, radii, torch.from_numpy(layers), None if bg is None else torch.from_numpy(bg), torch.float64)
    assert got.dtype == torch.float64
    assert np.abs(got.numpy() - want).max() <= 1e-12 and np.abs(got_d.numpy() - want_d).max() <= 1e-12
    # in float32 it repeats msi_ref's float32 roundings
    w32, _ = msi_ref.msi_render(rays, CENTER, radii, layers, bg, np.float32)
    g32, _ = msi_grad_ref.msi_render(rays, CENTER, radii, torch.from_numpy(layers), None if bg is None else torch.from_numpy(bg), torch.float32)
    assert g32.dtype == torch.float32 and np.array_equal(g32.numpy(), w32)


def test_autograd_gradient_matches_central_differences():
    g = np.random.default_rng(2)
    radii = np.asarray([1.0, 2.0], np.float32)
    rays = random_rays(g, 40, 1.3)
    layers, bg = g.uniform(0, 1, (2, 2, 4, 4)), g.uniform(0, 1, (2, 4, 4))
    g_rgb = g.standard_normal((40, 3))
    gl, gb = msi_grad_ref.texel_gradients(rays, CENTER, radii, layers, bg, g_rgb, torch.float64)

    def loss(l, b):
        return float((msi_ref.msi_render(rays, CENTER, radii, l, b, np.float64)[0] * g_rgb).sum())

    h = 1e-5   # rgb is linear in every C and multilinear in the A's of different layers: the central difference has no truncation error in C
    for arr, grad, which in ((layers, gl, 0), (bg, gb, 1)):
        num = np.zeros_like(arr)
        for idx in np.ndindex(arr.shape):
            up, dn = arr.copy(), arr.copy()
            up[idx] += h
            dn[idx] -= h
            num[idx] = (loss(up, bg) - loss(dn, bg)) / (2 * h) if which == 0 else (loss(layers, up) - loss(layers, dn)) / (2 * h)
        assert np.abs(grad).max() > 0.1 and np.abs(num - grad).max() <= 1e-8 * max(1.0, np.abs(grad).max()), np.abs(num - grad).max()
    assert np.all(gb[..., 3] == 0)   # the background's alpha is taken as 1


def test_symbols_are_declared_and_exported():
    lib = _lib.load()
    for name in ("ego_msi_render_backward", "ego_msi_render_backward_workspace_bytes", "ego_msi_project"):
        assert name in _lib.header_symbols() and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert lib.ego_abi_version() == 17 == _lib.EXPECTED_ABI_VERSION
    assert lib.ego_msi_render_backward_workspace_bytes(65536, 32) == 65536 * 32 * 4
    assert lib.ego_msi_render_backward_workspace_bytes(0, 1) == 0 and lib.ego_msi_render_backward_workspace_bytes(-1, 1) == -1
    from egonerf_amd import msi
    assert callable(msi.refine_msi) and callable(msi.project_msi)


def test_library_refuses_bad_arguments_before_anything_is_queued():
    lib = _lib.load()
    one, big = 16, 1 << 20   # a non-null, texel-aligned address; a workspace size that is always enough here

    def bwd(rays=one, N=4, cx=0.0, radii=one, L=2, Hm=4, Wm=8, tt=_lib.MSI_F32, layers=one, bg=None, g_rgb=one, g_layers=one, g_bg=None,
            ws=one, ws_bytes=big):
        return lib.ego_msi_render_backward(rays, N, cx, 0.0, 0.0, radii, L, Hm, Wm, tt, layers, bg, g_rgb, g_layers, g_bg, ws, ws_bytes, None)

    assert bwd(L=0) == -1 and b"msi_render_backward" in lib.ego_last_error()
    assert bwd(Wm=0) == -1 and bwd(N=-1) == -1 and bwd(cx=float("nan")) == -1
    assert bwd(tt=7) == -1 and b"unknown texel type" in lib.ego_last_error()
    assert bwd(tt=_lib.MSI_F16) == -1 and b"half" in lib.ego_last_error()
    assert bwd(Hm=1 << 16, Wm=1 << 15) == -1 and b"2^31" in lib.ego_last_error()
    for kw in (dict(rays=None), dict(radii=None), dict(layers=None), dict(g_rgb=None), dict(g_layers=None)):   # neither gradient asked for
        assert bwd(**kw) == -1 and b"null" in lib.ego_last_error(), kw
    assert bwd(g_bg=one) == -1 and b"without a background" in lib.ego_last_error()
    for kw in (dict(rays=12), dict(layers=24), dict(bg=8), dict(g_layers=8), dict(bg=one, g_bg=24), dict(g_rgb=18)):
        assert bwd(**kw) == -1 and b"aligned" in lib.ego_last_error(), kw
    assert bwd(ws=None) == -1 and b"workspace" in lib.ego_last_error()
    assert bwd(ws_bytes=4 * 2 * 4 - 1) == -1 and b"workspace" in lib.ego_last_error()
    assert bwd(ws=18) == -1 and b"workspace" in lib.ego_last_error()
    assert lib.ego_msi_render_backward(None, 0, 0.0, 0.0, 0.0, None, 2, 4, 8, _lib.MSI_F32, None, None, None, None, None, None, 0, None) == 0   # N == 0
    assert lib.ego_msi_project(one, -1, None) == -1 and b"msi_project" in lib.ego_last_error()
    assert lib.ego_msi_project(None, 4, None) == -1 and b"null" in lib.ego_last_error()
    assert lib.ego_msi_project(24, 4, None) == -1 and b"aligned" in lib.ego_last_error()
    assert lib.ego_msi_project(None, 0, None) == 0   # nothing to do


def host_image(dtype=torch.float32):
    g = torch.Generator().manual_seed(0)
    return MultiSphereImage(torch.rand(3, 4, 8, 4, generator=g).to(dtype), [0.5, 1.5, 4.0], [0.25, 1.0, 2.5, 6.0], [0.1, -0.2, 0.3], [0.01, 15.0],
                            torch.rand(4, 8, 4, generator=g).to(dtype))


def test_refine_refuses_bad_arguments_and_a_host_image():
    msi, teacher = host_image(), (lambda rays, **kw: (None,))
    with pytest.raises(ValueError, match="steps"):
        refine_msi(msi, teacher, -1)
    with pytest.raises(ValueError, match="rays_per_step"):
        refine_msi(msi, teacher, 1, rays_per_step=0)
    for bad in (0.5, 0.75, 0.0, -0.1, float("nan")):   # radii[0] = 0.5
        with pytest.raises(ValueError, match="headbox"):
            refine_msi(msi, teacher, 1, headbox=bad)
    with pytest.raises(ValueError, match="lr"):
        refine_msi(msi, teacher, 1, lr=0.0)
    with pytest.raises(ValueError, match="HIP device"):
        refine_msi(msi, teacher, 1, headbox=0.1)
    with pytest.raises(ValueError, match="HIP device"):
        refine_msi(msi, teacher, 0)   # even with nothing to do


def test_half_texels_that_require_grad_are_refused():
    msi = host_image(torch.float16)
    msi.layers.requires_grad_(True)
    with pytest.raises(ValueError, match=r"msi\.float\(\)"):
        msi.render(torch.zeros(5, 6))
    with torch.no_grad():   # without a graph to record, the call takes the path it always took
        with pytest.raises(ValueError, match="no CPU fallback"):
            msi.render(torch.zeros(5, 6))
    msi.layers.requires_grad_(False)
    msi.background.requires_grad_(True)
    with pytest.raises(ValueError, match=r"msi\.float\(\)"):
        msi(torch.zeros(5, 6), need_alpha=False)
