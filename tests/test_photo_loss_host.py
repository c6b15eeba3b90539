"""No GPU: the photometric term's restatement (tests/photo_loss_ref.py) against float64 autograd and the plain MSE, the fit as the
minimiser of the L2 term, ExposureDeltas, RayBank(masks=...) validation, the masked PSNRs, and every refusal that needs no device."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib, metrics
from egonerf_amd.data import RayBank
from egonerf_amd.exposure import ExposureDeltas, align, apply_exposure, fit_exposure
from egonerf_amd.losses import photometric_loss
from tests import photo_loss_ref as ref


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("form", ["plain", "weight", "image", "all"])
def test_closed_form_gradients_equal_float64_autograd(kind, form):
    c = ref.make_inputs(257, 5, with_weight=form in ("weight", "all"), with_image=form in ("image", "all"), with_affine=form == "all")
    v, g, ga = ref.autograd_direct(c["rgb"], c["target"], c["weight"], c["image"], c["affine"], kind, K=5)
    mv, mg, mga = ref.kernel_model(c["rgb"], c["target"], c["weight"], c["image"], c["affine"], kind, K=5)
    assert v > 0 and abs(mv - v) <= 1e-13 * v
    assert np.abs(mg - g).max() <= 1e-13 * np.abs(g).max()
    if form == "all":
        assert np.abs(mga - ga).max() <= 1e-13 * np.abs(ga).max()
        assert np.abs(ga).max() > 0
    else:
        assert ga is None and mga is None
    invalid = ~ref.valid_mask(c["target"], c["weight"], c["image"], 5)
    assert invalid.sum() >= 2 and (mg[invalid] == 0).all() and (g[invalid] == 0).all()
    # the float32 restatement's distances, which the GPU tests' bounds are made of
    v32, g32, _ = ref.kernel_model(c["rgb"], c["target"], c["weight"], c["image"], c["affine"], kind, K=5, dtype=np.float32)
    print(f"{kind} {form}: float32 model value {abs(v32 - v) / v:.2e}, g_rgb {ref.bound(g32, g)[0] / 4:.2e}")


def test_the_restatement_reduces_to_the_mse():
    g = np.random.default_rng(3)
    rgb, target = g.uniform(0, 1, (300, 3)).astype(np.float32), g.uniform(0, 1, (300, 3)).astype(np.float32)
    mse = float(torch.mean((torch.from_numpy(rgb).double() - torch.from_numpy(target).double()) ** 2))
    v, grad, _ = ref.kernel_model(rgb, target)
    assert abs(v - mse) <= 1e-14 * mse
    assert np.abs(grad - 2.0 * (rgb.astype(np.float64) - target) / 900.0).max() <= 1e-17
    assert abs(ref.autograd_direct(rgb, target)[0] - mse) <= 1e-14 * mse


def test_the_fit_zeroes_the_l2_gradient_with_respect_to_affine():
    c = ref.make_inputs(4099, 3)
    affine, Wk = ref.fit_model(c["rgb"], c["target"], c["weight"], c["image"], 3)
    assert (Wk > 0).all() and np.abs(affine[:, :, 0] - 1).max() < 0.5
    _, _, ga = ref.autograd_direct(c["rgb"], c["target"], c["weight"], c["image"], affine, "l2")
    _, _, ga_id = ref.autograd_direct(c["rgb"], c["target"], c["weight"], c["image"], np.tile([1.0, 0.0], (3, 3, 1)), "l2")
    assert np.abs(ga).max() <= 1e-13 and np.abs(ga_id).max() > 1e-4   # and the identity is not the minimiser on these inputs


def test_fit_edge_cases_of_the_restatement():
    rgb = np.full((8, 3), 0.25, np.float32)
    rgb[:, 1] = np.linspace(0.1, 0.9, 8)
    target = (rgb * 1.2 + 0.1).astype(np.float32)
    image = np.array([0, 0, 0, 0, 2, 2, 2, 2], np.int32)
    affine, Wk = ref.fit_model(rgb, target, None, image, 3)
    assert list(Wk) == [4, 0, 4] and np.array_equal(affine[1], np.tile([1.0, 0.0], (3, 1)))     # no ray: the identity
    assert affine[0, 0, 0] == 1 and abs(affine[0, 0, 1] - (0.25 * 0.2 + 0.1)) < 1e-7             # all colours equal: gain 1, the means' gap
    assert abs(affine[0, 1, 0] - 1.2) < 1e-6 and abs(affine[0, 1, 1] - 0.1) < 1e-6


def test_exposure_deltas():
    d = ExposureDeltas(4)
    assert d.log_gain.shape == (4, 3) and d.bias.shape == (4, 3)
    ident = torch.tensor([1.0, 0.0]).expand(4, 3, 2)
    assert torch.equal(d.affine(), ident) and torch.equal(ExposureDeltas(4, anchor=2).affine(), ident)
    a = ExposureDeltas(4, anchor=2)
    with torch.no_grad():
        a.log_gain.add_(0.3)
        a.bias.sub_(0.1)
    aff = a.affine()
    assert torch.equal(aff[2], ident[2]) and torch.allclose(aff[0, :, 0], torch.full((3,), float(np.exp(np.float32(0.3)))))
    (aff * torch.arange(1.0, 25.0).reshape(4, 3, 2)).sum().backward()
    assert bool((a.log_gain.grad[2] == 0).all()) and bool((a.bias.grad[2] == 0).all())     # exactly zero
    assert bool((a.log_gain.grad[[0, 1, 3]] != 0).all()) and bool((a.bias.grad[[0, 1, 3]] != 0).all())
    # an upstream NaN does not leak into the anchor either
    a.zero_grad()
    (a.affine() * float("nan")).sum().backward()
    assert bool((a.log_gain.grad[2] == 0).all()) and bool((a.bias.grad[2] == 0).all())
    fit = torch.stack([torch.linspace(0.7, 1.3, 12).reshape(4, 3), torch.linspace(-0.05, 0.05, 12).reshape(4, 3)], -1)
    d.set_from_affine(fit)
    assert torch.allclose(d.affine(), fit, rtol=3e-7, atol=0)
    a.set_from_affine(fit)
    assert torch.equal(a.affine()[2], ident[2]) and torch.allclose(a.affine()[[0, 1, 3]], fit[[0, 1, 3]], rtol=3e-7, atol=0)
    bad = fit.clone()
    bad[1, 1, 0] = 0.0
    with pytest.raises(ValueError, match="gain"):
        d.set_from_affine(bad)
    with pytest.raises(ValueError, match=r"\[K, 3, 2\]"):
        d.set_from_affine(fit[:3])
    with pytest.raises(ValueError, match="K must be"):
        ExposureDeltas(0)
    with pytest.raises(ValueError, match="anchor"):
        ExposureDeltas(3, anchor=3)


def test_apply_exposure_is_the_affine_map():
    g = torch.Generator().manual_seed(0)
    rgb, aff = torch.rand(5, 7, 3, generator=g), torch.rand(4, 3, 2, generator=g)
    img = torch.randint(0, 4, (5, 7), generator=g)
    got = apply_exposure(rgb, aff, img)
    assert torch.equal(got[2, 3], aff[img[2, 3], :, 0] * rgb[2, 3] + aff[img[2, 3], :, 1])
    assert torch.equal(apply_exposure(rgb, aff[:1]), aff[0, :, 0] * rgb + aff[0, :, 1])
    with pytest.raises(ValueError, match="needs image"):
        apply_exposure(rgb, aff)
    with pytest.raises(ValueError, match="leading shape"):
        apply_exposure(rgb, aff, img[:4])


def _bank(masks, K=2, H=4, W=6):
    return RayBank(np.tile(np.eye(4, dtype=np.float32), (K, 1, 1)), np.zeros((K, H, W, 3), np.uint8), (W, H), device="cpu", masks=masks)


def test_ray_bank_validates_its_masks():
    m = np.random.default_rng(0).integers(0, 256, (2, 4, 6)).astype(np.uint8)
    bank = _bank(m)
    assert bank.masks.dtype == torch.uint8 and np.array_equal(bank.masks.numpy(), m)
    assert bank.nbytes == _bank(None).nbytes + 2 * 4 * 6 and _bank(None).masks is None
    b = _bank(torch.from_numpy(m > 100))
    assert b.masks.dtype == torch.uint8 and np.array_equal(b.masks.numpy(), np.where(m > 100, 255, 0))   # bool is stored as 0 / 255
    for wrong in (m.astype(np.float32), m[:1], m[:, :3], m.astype(np.int32)):
        with pytest.raises(ValueError, match="masks must be uint8 or bool"):
            _bank(wrong)
    with pytest.raises(ValueError, match="without masks"):
        _bank(None).gather_mask_into(torch.zeros(3, dtype=torch.int64), torch.zeros(3))
    with pytest.raises(RuntimeError, match="HIP device"):
        bank.gather_mask(torch.zeros(3, dtype=torch.int64))


def test_masked_psnr_and_ws_psnr_against_numpy():
    g = np.random.default_rng(5)
    img, gt = g.uniform(0, 1, (12, 20, 3)).astype(np.float32), g.uniform(0, 1, (12, 20, 3)).astype(np.float32)
    mask = g.integers(0, 3, (12, 20)).astype(np.uint8) * 100   # 0, 100, 200: > 0 counts
    ti, tg, tm = torch.from_numpy(img), torch.from_numpy(gt), torch.from_numpy(mask)
    keep = mask > 0
    d2 = (img.astype(np.float64) - gt) ** 2
    assert abs(metrics.psnr(ti, tg, mask=tm) - (-10 * np.log10(d2[keep].mean()))) <= 1e-5
    w = np.broadcast_to(metrics.ws_weights(12)[:, None], (12, 20))
    want = 10 * np.log10(1.0 / ((d2.sum(2) * w)[keep].sum() / (3 * w[keep].sum())))
    assert abs(metrics.ws_psnr(ti, tg, mask=tm) - want) <= 1e-10
    # without a mask: the path they took, bit for bit; a full mask is the same number
    assert metrics.psnr(ti, tg) == float(-10.0 * np.log(torch.mean((ti - tg) ** 2).item()) / np.log(10.0))
    assert abs(metrics.ws_psnr(ti, tg, mask=torch.ones(12, 20)) - metrics.ws_psnr(ti, tg)) <= 1e-10
    assert abs(metrics.psnr(ti, tg, mask=torch.ones(12, 20, dtype=torch.bool)) - metrics.psnr(ti, tg)) <= 1e-5
    assert metrics.psnr(ti, tg, mask=tm) != metrics.psnr(ti, tg)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        metrics.psnr(ti, tg, mask=tm[:5])
    with pytest.raises(ValueError, match="no pixel"):
        metrics.ws_psnr(ti, tg, mask=torch.zeros(12, 20))


def test_host_refusals_that_need_no_device():
    rgb, tgt = torch.rand(8, 3), torch.rand(8, 3)
    w, img, aff = torch.rand(8), torch.zeros(8, dtype=torch.int64), torch.ones(2, 3, 2)
    with pytest.raises(ValueError, match="kind must be one of"):
        photometric_loss(rgb, tgt, kind="l3")
    for kind in ("huber", "charbonnier"):
        for p in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite param > 0"):
                photometric_loss(rgb, tgt, kind=kind, param=p)
    with pytest.raises(RuntimeError, match=r"rgb must be a floating-point \[N, 3\]"):
        photometric_loss(rgb[:, :2], tgt)
    with pytest.raises(RuntimeError, match="target must be a float32"):
        photometric_loss(rgb, tgt[:7])
    with pytest.raises(RuntimeError, match="target must be a float32"):
        photometric_loss(rgb, tgt.double())
    with pytest.raises(RuntimeError, match="weight must be a float32"):
        photometric_loss(rgb, tgt, weight=w[:7])
    with pytest.raises(RuntimeError, match="weight must be a float32"):
        photometric_loss(rgb, tgt, weight=w.double())
    with pytest.raises(RuntimeError, match="image must be an int32 or int64"):
        photometric_loss(rgb, tgt, image=img.float())
    with pytest.raises(RuntimeError, match="affine must be a float32"):
        photometric_loss(rgb, tgt, image=img, affine=torch.ones(2, 3))
    with pytest.raises(ValueError, match="affine needs image"):
        photometric_loss(rgb, tgt, affine=aff)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        photometric_loss(rgb, tgt, weight=w, image=img, affine=aff)
    with pytest.raises(ValueError, match="K must be >= 1"):
        fit_exposure(rgb, tgt, K=0)
    with pytest.raises(ValueError, match="needs image"):
        fit_exposure(rgb, tgt, K=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_exposure(rgb, tgt, image=img, K=2)
    with pytest.raises(ValueError, match="one shape"):
        align(torch.rand(4, 5, 3), torch.rand(4, 6, 3))
    with pytest.raises(ValueError, match=r"mask must be \[H, W\]"):
        align(torch.rand(4, 5, 3), torch.rand(4, 5, 3), mask=torch.ones(5, 4))


def test_library_refusals_before_any_launch():
    """The C entry points check their arguments before they touch the device: the calls below return EGO_E_BADARG with a message and
    launch nothing (their pointers are never dereferenced)."""
    lib = _lib.load()
    P = 0x1000   # a non-null, 8-byte aligned stand-in: refused calls do not read it
    assert lib.ego_photo_loss_workspace_bytes(8192, 100) > 0 and lib.ego_photo_loss_workspace_bytes(-1, 1) < 0
    assert lib.ego_photo_loss_workspace_bytes(0, 1) >= 16

    def loss(rgb=P, target=P, weight=None, image=None, affine=None, N=8, K=1, kind=_lib.PHOTO_L2, param=0.0, ws=P, value=P, g_rgb=None,
             g_affine=None):
        return lib.ego_photo_loss(rgb, target, weight, image, affine, N, K, kind, param, ws, value, g_rgb, g_affine, None)

    def refused(code, what):
        assert code != 0
        msg = lib.ego_last_error().decode(errors="replace")
        assert what in msg, msg

    refused(loss(kind=4), "unknown kind")
    refused(loss(kind=-1), "unknown kind")
    for kind in (_lib.PHOTO_HUBER, _lib.PHOTO_CHARBONNIER):
        for p in (0.0, -0.1, float("nan"), float("inf")):
            refused(loss(kind=kind, param=p), "finite param > 0")
    refused(loss(affine=P), "affine needs image")
    refused(loss(g_affine=P), "g_affine needs image")
    refused(loss(image=P, affine=P, K=0), "K < 1")
    refused(loss(rgb=None), "null rgb or target")
    refused(loss(target=None), "null rgb or target")
    refused(loss(value=None), "no output asked for")
    refused(loss(N=-1), "N < 0")
    refused(loss(ws=None), "workspace")
    assert loss(N=0) == 0   # a no-op
    fit = lambda rgb=P, target=P, image=None, N=8, K=1, affine=P: lib.ego_photo_fit(rgb, target, None, image, N, K, affine, None, None)
    refused(fit(K=0), "K < 1")
    refused(fit(K=2), "one image")
    refused(fit(affine=None), "null affine")
    refused(fit(rgb=None), "null rgb or target")
    refused(fit(N=-1), "N < 0")
