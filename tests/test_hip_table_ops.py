"""GPU: the regularisers (ego_tv_plane, ego_l1_table, ego_line_ortho), ego_resample_table and the average pooling (ego_avgpool_table,
ego_avgpool_field) against tests/table_ops_ref.py at the sizes where these kernels change path: every texel on an edge, one element
either side of a block, the grid-stride loops, the W = 1 forms, null `value` / `grad`, accumulation into a non-zero `grad`.  Kernels
without a float32 reduction are compared bit for bit with the float32 restatement; everything is compared with float64 truth under the
derived running-error bound (table_ops_ref.bound), with nothing added.  Each test prints its largest error as a fraction of that bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from egonerf_amd import _lib
from egonerf_amd.coordinates import YinYangSphericalCoords
from egonerf_amd.losses import TVLoss
from tests import table_ops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = 0.75   # exact in float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def frac(err, bnd):
    return float(np.max(np.abs(err) / bnd))


def prefill(n):
    """A known pattern without zeros: what `grad` holds before the call."""
    return ((np.arange(n) % 13).astype(np.float32) - np.float32(6.5)) * np.float32(0.125)


def _reg_call(fn, what, x_dev, head, want_value, want_grad, n):
    """One call of a regulariser entry point -> (value or None, grad or None); grad starts from `prefill`."""
    value = torch.zeros(1, dtype=torch.float64, device=DEV) if want_value else None
    grad = dev(prefill(n)) if want_grad else None
    _lib.check(fn(x_dev.data_ptr(), *head, SCALE, _lib.ptr(value), _lib.ptr(grad), _lib.stream_handle()), what)
    torch.cuda.synchronize()
    return (None if value is None else float(value.item())), (None if grad is None else grad.cpu().numpy())


def _check_value(got, terms_f32, coeff, truth, k, what):
    """Against the float64 sum of the restatement's float32 terms (only the order of the double adds differs: 2^-53 x term count, far
    below 1e-12 at these sizes) and against truth under the bound.  Every term is >= 0, so the absolute sum is the value."""
    copy = float(terms_f32.astype(np.float64).sum()) * coeff
    print(f"{what}: value {got:.17g}  |hip - copy| / copy {abs(got - copy) / max(copy, 1e-300):.2e}  |hip - f64| / bound "
          f"{frac(got - truth, R.bound(k, truth)):.3f}")
    assert abs(got - copy) <= 1e-12 * copy
    assert abs(got - truth) <= R.bound(k, truth)


@pytest.mark.parametrize("shape", R.TV_SHAPES)
def test_tv_plane(shape):
    C_, H, W = shape
    x = R.table_input((H, W, C_), 1)
    terms, g, g_abs = R.tv_f32(x, SCALE)
    v64, g64 = R.tv_f64(x, SCALE)
    assert frac(g - g64, R.bound(R.K_TV_GRAD, g_abs)) <= 1.0
    xd, pre = dev(x), prefill(x.size).reshape(x.shape)
    for want_value, want_grad in ((True, False), (False, True), (True, True)):
        value, grad = _reg_call(_lib.load().ego_tv_plane, "ego_tv_plane", xd, (C_, H, W), want_value, want_grad, x.size)
        if want_grad:
            assert np.array_equal(R.bits(grad.reshape(x.shape)), R.bits(pre + g)), (shape, want_value)
        if want_value:
            _check_value(value, terms, 1.0, v64, R.K_TV_VALUE, f"tv {shape}")
    # the module, with a gradient flowing in that is not 1: (1, C, H, W) tensor over [H][W][C] memory
    p = torch.nn.Parameter(dev(x)[None].permute(0, 3, 1, 2))
    v = TVLoss(TVLoss_weight=SCALE)(p)
    (v * 3.0).backward()
    assert abs(float(v.item()) - v64) <= R.bound(R.K_TV_VALUE, v64)
    got = p.grad.permute(0, 2, 3, 1).contiguous().cpu().numpy()[0]
    assert np.array_equal(got, g * np.float32(3.0))
    print(f"tv {shape}: gradient |copy - f64| / bound {frac(g - g64, R.bound(R.K_TV_GRAD, g_abs)):.3f} (hip == copy)")


@pytest.mark.parametrize("n", R.L1_SIZES)
def test_l1_table(n):
    x = R.l1_input(n)
    a, terms, g = R.l1_f32(x, SCALE)
    v64, g64 = R.l1_f64(x, SCALE)
    xd, pre = dev(x), prefill(n)
    for want_value, want_grad in ((True, False), (False, True), (True, True)):
        value, grad = _reg_call(_lib.load().ego_l1_table, "ego_l1_table", xd, (n,), want_value, want_grad, n)
        if want_grad:
            assert np.array_equal(R.bits(grad), R.bits(pre + g)), (n, want_value)
        if want_value:
            _check_value(value, terms, float(a), v64, R.K_L1_VALUE, f"l1 {n}")
    assert frac(g - g64, R.bound(R.K_L1_GRAD, np.abs(g64))) <= 1.0


def _ortho(L, want_value=True, want_grad=True):
    n, C_ = L.shape
    value = torch.zeros(1, dtype=torch.float64, device=DEV) if want_value else None
    grad = torch.zeros(n, C_, device=DEV) if want_grad else None
    _lib.check(_lib.load().ego_line_ortho(dev(L).data_ptr(), C_, n, SCALE, _lib.ptr(value), _lib.ptr(grad), _lib.stream_handle()),
               "ego_line_ortho")
    torch.cuda.synchronize()
    return (None if value is None else float(value.item())), (None if grad is None else grad.cpu().numpy())


def _check_ortho(L, what):
    n, C_ = L.shape
    copy_v, copy_g, v_abs, g_abs, G = R.ortho_f32(L, SCALE)
    v64, g64, G64 = R.ortho_f64(L, SCALE)
    value, grad = _ortho(L)
    fv, fg = frac(value - v64, R.bound(R.k_ortho_value(n), v_abs)), frac(grad - g64, R.bound(R.k_ortho_grad(C_), g_abs))
    print(f"ortho {what}: |hip - f64| / bound: value {fv:.3f} gradient {fg:.3f}; hip == copy: value {value == copy_v} "
          f"gradient {np.array_equal(grad, copy_g)}")
    assert fv <= 1.0 and fg <= 1.0
    # value-only and gradient-only calls compute the same thing
    assert _ortho(L, want_grad=False)[0] == value and np.array_equal(_ortho(L, want_value=False)[1], grad)
    return value, grad


@pytest.mark.parametrize("shape", R.ORTHO_SHAPES)
def test_line_ortho(shape):
    C_, n = shape
    _check_ortho(R.ortho_input(C_, n, C_), shape)


def test_line_ortho_exactly_zero_gram_entry():
    L = R.ortho_disjoint_input()
    value, grad = _check_ortho(L, "disjoint columns")
    # columns 0 and 1 contribute nothing to each other, on both sides
    assert np.array_equal(grad[:, 0], np.float32(2) * (np.float32(SCALE) / np.float32(6)) * -L[:, 2])


@pytest.mark.parametrize("C_", [1, 65])
def test_line_ortho_refuses_component_counts_outside_its_range(C_):
    L = torch.ones(4, C_, device=DEV)
    value = torch.zeros(1, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match=r"line_ortho: bad size \(2 <= n_comp <= 64\)"):
        _lib.check(_lib.load().ego_line_ortho(L.data_ptr(), C_, 4, SCALE, value.data_ptr(), None, _lib.stream_handle()), "ego_line_ortho")


def _resample(src, xs, ys):
    H, W, C_ = src.shape
    dst = torch.full((len(ys) * len(xs) * C_ + 1,), 777.0, device=DEV)   # one element more than the kernel may write
    sd, xd, yd = dev(src), dev(xs), dev(ys)
    _lib.check(_lib.load().ego_resample_table(sd.data_ptr(), C_, H, W, xd.data_ptr(), yd.data_ptr(), len(ys), len(xs), dst.data_ptr(),
                                              _lib.stream_handle()), "ego_resample_table")
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert out[-1] == 777.0
    return out[:-1].reshape(len(ys), len(xs), C_)


@pytest.mark.parametrize("case", R.resample_cases(), ids=lambda c: c[0])
def test_resample_table(case):
    name, src, xs, ys = case
    assert (len(xs) * len(ys) * src.shape[2]) % 256 != 0
    got = _resample(src, xs, ys)
    truth, ab = R.resample_f64(src, xs, ys)
    f = frac(got - truth, R.bound(R.K_RESAMPLE, ab))
    print(f"resample {name}: {got.shape}  |hip - f64| / bound {f:.3f}")
    assert not np.isnan(got).any()
    assert f <= 1.0
    assert (got[np.isnan(ys)] == 0).all() and (got[:, np.isnan(xs)] == 0).all()   # a NaN position masks both taps


def test_up_sampling_vm_plane_and_line():
    coords = YinYangSphericalCoords(DEV, [[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]], N_voxel=20 ** 3)
    N_r, N_th, N_ph = coords.resolution
    target = [2 * N_r - 3, N_th + 5, N_ph + 7]
    worst = 0.0
    for C_, (H, W), ids in ((16, (N_th, N_r), [1, 0]), (48, (N_ph, N_th), [2, 1]), (16, (N_r, 1), [0]), (3, (N_ph, 1), [2])):
        src = R.table_input((H, W, C_), 11 + C_)
        w = dev(src)[None].permute(0, 3, 1, 2)
        out = coords.up_sampling_VM(w, res_target=target, ids=ids)
        assert isinstance(out, torch.nn.Parameter) and out.permute(0, 2, 3, 1).is_contiguous()
        ys = coords.upsample_axis_positions(target, ids[0]).float().numpy()
        xs = coords.upsample_axis_positions(target, ids[1]).float().numpy() if len(ids) == 2 else np.array([-1.0], np.float32)
        assert tuple(out.shape) == (1, C_, len(ys), len(xs))
        truth, ab = R.resample_f64(src, xs, ys)
        worst = max(worst, frac(out.detach().permute(0, 2, 3, 1)[0].cpu().numpy() - truth, R.bound(R.K_RESAMPLE, ab)))
    print(f"up_sampling_VM: |hip - f64| / bound {worst:.3f}")
    assert worst <= 1.0


def _pooled_shape(H, W, C_):
    return H // 2, (1 if W == 1 else W // 2), C_


def _check_pooled(got, src, what):
    copy = R.avgpool_f32(src)
    truth, ab = R.avgpool_f64(src)
    assert got.shape == copy.shape and np.array_equal(R.bits(got), R.bits(copy)), what
    return frac(got - truth, R.bound(R.K_AVGPOOL, ab))


@pytest.mark.parametrize("shape", R.AVGPOOL_SHAPES)
def test_avgpool_table(shape):
    H, W, C_ = shape
    src = R.table_input(shape, 3)
    n = int(np.prod(_pooled_shape(*shape)))
    dst = torch.full((n + 1,), 777.0, device=DEV)
    _lib.check(_lib.load().ego_avgpool_table(dev(src).data_ptr(), H, W, C_, dst.data_ptr(), _lib.stream_handle()), "ego_avgpool_table")
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert out[-1] == 777.0
    f = _check_pooled(out[:-1].reshape(_pooled_shape(*shape)), src, shape)
    print(f"avgpool_table {shape}: hip == copy, |hip - f64| / bound {f:.3f}")
    assert f <= 1.0


# plane i of a field is [res[y axis]][res[x axis]][C], line i is [res[line axis]][C] (ego_device.h: matMode / vecMode)
PLANE_YX = ((1, 0), (2, 0), (2, 1))
LINE_AX = (2, 1, 0)


@pytest.mark.parametrize("res,C_", [((7, 9, 5), 3), ((6, 256, 258), 16)], ids=["odd", "strided"])
def test_avgpool_field(res, C_):
    """`strided`: plane 2 is 258 x 256 at 16 channels, 264 192 pooled elements: more than the 1024 blocks of k_avgpool_many cover at once."""
    shapes = [(res[y], res[x], C_) for y, x in PLANE_YX] + [(res[a], 1, C_) for a in LINE_AX]
    if res[0] % 2 == 0:
        assert max(int(np.prod(_pooled_shape(*s))) for s in shapes) > 1024 * 256
    fs, fd = _lib.VmField(), _lib.VmField()
    fs.n_comp = fd.n_comp = C_
    keep, srcs, dsts = [], {}, {}
    for k in range(3):
        fs.res[k], fd.res[k] = res[k], res[k] // 2
    for g in range(2):
        for i in range(6):
            shape = shapes[i]
            src = R.table_input(shape, 20 + 6 * g + i)
            sd, dd = dev(src), torch.full((int(np.prod(_pooled_shape(*shape))) + 1,), 777.0, device=DEV)
            keep += [sd, dd]
            srcs[g, i], dsts[g, i] = src, dd
            (fs.plane if i < 3 else fs.line)[g][i % 3] = sd.data_ptr()
            (fd.plane if i < 3 else fd.line)[g][i % 3] = dd.data_ptr()
    _lib.check(_lib.load().ego_avgpool_field(C.byref(fs), C.byref(fd), _lib.stream_handle()), "ego_avgpool_field")
    torch.cuda.synchronize()
    worst = 0.0
    for key, dd in dsts.items():
        out = dd.cpu().numpy()
        assert out[-1] == 777.0, key
        worst = max(worst, _check_pooled(out[:-1].reshape(_pooled_shape(*srcs[key].shape)), srcs[key], key))
    print(f"avgpool_field {res}: hip == copy, |hip - f64| / bound {worst:.3f}")
    assert worst <= 1.0
