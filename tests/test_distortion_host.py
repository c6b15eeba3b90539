"""CPU: the distortion regulariser's float64 restatement (tests/distortion_ref.py) against torch's float64 autograd of the O(S^2) form,
its known answers, how far float32 arithmetic alone is from it on the GPU tests' inputs, and the argument checks of the host layer and
of the library."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib
from egonerf_amd.losses import distortion_loss
from tests import distortion_ref as ref

N = 37
SIZES = [2, 63, 65, 130, 512]
# tests/test_hip_distortion.py holds the kernel to these against the float64 restatement
GPU_VALUE_BOUND, GPU_GRAD_BOUND = 2e-6, 2e-5


def autograd_direct(alpha, m, delta):
    """value and d value / d alpha of the [N][S][S] form by torch autograd in float64."""
    S = m.shape[1]
    a = torch.from_numpy(np.asarray(alpha, np.float64)).requires_grad_(True)
    m, delta = torch.from_numpy(m), torch.from_numpy(delta)
    f = 1.0 - a[:, :S] + 1e-10
    T = torch.cat([torch.ones(a.shape[0], 1, dtype=torch.float64), torch.cumprod(f, 1)[:, :-1]], 1)
    w = a[:, :S] * T
    pair = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2))
    value = (pair + (w * w * delta).sum(1) / 3.0).mean()
    value.backward()
    return float(value.detach()), a.grad.numpy()


@pytest.mark.parametrize("space", ref.SPACES)
@pytest.mark.parametrize("S", SIZES)
def test_float64_model_equals_autograd_of_the_direct_form(S, space):
    alpha, z = ref.make_inputs(N, S, trailing_ones=(S % 2 == 1))
    m, delta = ref.intervals(z, ref.NEAR, ref.FAR, space)
    assert np.all(delta >= 0) and np.all(np.diff(m, axis=1) >= 0) and m.min() >= 0 and m.max() < 2   # z_S may pass far: s_S < 2
    if S > 2:
        assert np.all(delta[:, S // 2 - 1] == 0)   # the tie
    v_ref, g_ref = autograd_direct(alpha, m, delta)
    value, g = ref.kernel_model(alpha, m, delta, np.float64)
    assert abs(value - v_ref) <= 1e-12 and abs(ref.direct_value(alpha, m, delta) - v_ref) <= 1e-12
    assert g.shape == alpha.shape and float(np.abs(g - g_ref).max()) <= 1e-12
    assert v_ref > 0 and float(np.abs(g_ref).max()) > 0
    if alpha.shape[1] > S:
        assert np.all(g[:, S:] == 0) and np.all(g_ref[:, S:] == 0)


def test_known_answers():
    S = 9
    m, delta = ref.intervals(ref.make_inputs(4, S)[1][:1], ref.NEAR, ref.FAR, "log")
    alpha = np.zeros((1, S), np.float32)
    value, g = ref.kernel_model(alpha, m, delta)
    assert value == 0 and np.all(g == 0)                                  # nothing on the ray
    alpha[0, 4] = 1.0
    value, _ = ref.kernel_model(alpha, m, delta)
    assert abs(value - delta[0, 4] / 3.0) <= 1e-9                          # one opaque sample: its own width / 3 (T_4 = (1 + 1e-10)^4)
    alpha = ref.make_inputs(4, S, seed=1)[0][3:4]
    v0, g0 = ref.kernel_model(alpha, m, delta)
    v1, g1 = ref.kernel_model(alpha, m + 0.25, delta)
    assert v0 > 0 and abs(v0 - v1) <= 1e-14 and float(np.abs(g0 - g1).max()) <= 1e-14   # only differences of m enter


@pytest.mark.parametrize("space", ref.SPACES)
@pytest.mark.parametrize("S", SIZES)
def test_float32_arithmetic_alone_stays_within_a_quarter_of_the_gpu_bounds(S, space):
    """The condition of the GPU test's inputs: if float32 arithmetic in the kernel's own order were already near the bound, the bound
    would test the inputs, not the kernel.  Worst over these cases: printed by -s; recorded in DESIGN.md 4.2a."""
    alpha, z = ref.make_inputs(N, S)
    v64, g64 = ref.distortion(alpha, z, space, np.float64)
    v32, g32 = ref.distortion(alpha, z, space, np.float32)
    assert g32.dtype == np.float32
    ev, eg = abs(v32 - v64) / abs(v64), float(np.abs(g32 - g64).max()) / float(np.abs(g64).max())
    print(f"float32 model S={S} {space}: value {ev:.2e} gradient {eg:.2e}")
    assert ev <= GPU_VALUE_BOUND / 4 and eg <= GPU_GRAD_BOUND / 4


def test_host_layer_refuses_bad_arguments():
    a, z = torch.zeros(5, 8), torch.ones(5, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distortion_loss(a, z, [0.01, 15.0])
    for bad in (lambda: distortion_loss(a, z, [0.01, 15.0], space="sqrt"), lambda: distortion_loss(a, z, [0.0, 15.0]),
                lambda: distortion_loss(a, z, [0.0, 15.0], space="disparity"), lambda: distortion_loss(a, z, [2.0, 2.0], space="linear")):
        with pytest.raises(ValueError):
            bad()
    zeros = torch.zeros
    for al, zz in ((zeros(5, 8), zeros(4, 8)), (zeros(5, 10), zeros(5, 8)), (zeros(5, 7), zeros(5, 8)), (zeros(5, 8, 1), zeros(5, 8)),
                   (zeros(5, 1), zeros(5, 1)), (zeros(5, 8), zeros(5, 8, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match=r"must be"):
            distortion_loss(al, zz, [0.01, 15.0])


def test_library_refuses_bad_arguments_before_anything_is_queued():
    lib = _lib.load()
    one = 16   # a non-null address: every call below fails its checks first
    call = lambda alpha=one, stride=8, z=one, N=4, S=8, near=0.01, far=15.0, space=_lib.DIST_LOG, value=one, g=one: \
        lib.ego_ray_distortion(alpha, stride, z, N, S, near, far, space, value, g, None)
    for kw in (dict(S=1), dict(stride=7), dict(N=-1), dict(far=0.01), dict(far=float("nan")), dict(far=float("inf")), dict(near=0.0),
               dict(near=0.0, space=_lib.DIST_DISPARITY), dict(near=-1.0), dict(space=3), dict(space=-1), dict(alpha=None), dict(z=None),
               dict(value=None, g=None)):
        assert call(**kw) == -1 and b"ray_distortion" in lib.ego_last_error(), kw
    assert b"null" in lib.ego_last_error()
    assert call(alpha=None, z=None, N=0, value=None, g=None) == 0      # N == 0: a no-op
    assert call(S=1, N=0) == -1                                        # ... after the size checks


def test_symbol_is_declared_and_exported():
    lib = _lib.load()
    assert "ego_ray_distortion" in _lib.header_symbols() and "ego_ray_distortion" in _lib.PROTOTYPES and hasattr(lib, "ego_ray_distortion")
    assert (_lib.DIST_LINEAR, _lib.DIST_LOG, _lib.DIST_DISPARITY) == (0, 1, 2)
    assert lib.ego_abi_version() == 17 == _lib.EXPECTED_ABI_VERSION
