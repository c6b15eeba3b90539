"""GPU: the photometric term for real captures (ego_photo_loss / ego_photo_fit / ego_ray_batch_gather_mask, losses.photometric_loss,
exposure.*, RayBank(masks=...), GraphedTrainStep's weight / image buffers): the kernels against the float64 definition of
tests/photo_loss_ref.py, what must be exact, bit-reproducibility across call forms, the fit's recovery of known exposures from
quantised images under a mask, the bank's mask gather, an exposure-only optimisation against float64 torch, and the term inside a
captured training step against the eager loop.

The bounds are per case and per quantity: 4 x the float32 restatement's own distance from float64 on the case's inputs, never below
4 x 2^-24 (ref.bound).  Measured on an MI355X, worst over the parity cases: value 4.0e-16 of |v64| (bounds from 2.4e-7), g_rgb 5.7e-8
of max |g64| (2.4e-7), g_affine 6.0e-8 of max |ga64| (2.4e-7); the fit 5.1e-8 of max |affine64| (2.4e-7), the L2 gradient at the fit
2.5e-8 of the terms that cancel in it (2.4e-7): the kernels work in float64 and an output is the float64 result rounded once."""
import functools

import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth
from egonerf_amd.data import RayBank
from egonerf_amd.exposure import ExposureDeltas, align, apply_exposure, fit_exposure
from egonerf_amd.losses import photometric_loss
from egonerf_amd.metrics import psnr
from egonerf_amd.optim import FusedAdam
from egonerf_amd.sampler import DeviceSimpleSampler
from egonerf_amd.train import GraphedTrainStep
from tests import photo_loss_ref as ref
from tests.test_hip_train_graph import _same_after_adam, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda"
KIND_CODE = dict(l2=_lib.PHOTO_L2, l1=_lib.PHOTO_L1, huber=_lib.PHOTO_HUBER, charbonnier=_lib.PHOTO_CHARBONNIER)
FORMS = [(w, i, a) for w in (False, True) for i, a in ((False, False), (True, False), (True, True))]   # weight, image, affine
bits = lambda t: t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def run_kernel(d, kind, want_value=True, want_rgb=True, want_affine=True, K=None):
    """One ego_photo_loss call on a dict of device tensors -> (value, g_rgb, g_affine); the gradient buffers and the workspace start as
    NaN (every element must be written, the workspace needs no clearing)."""
    lib = _lib.load()
    N, K = d["rgb"].shape[0], (d["K"] if K is None else K)
    value = torch.zeros(1, dtype=torch.float64, device=DEV) if want_value else None
    g_rgb = torch.full((N, 3), float("nan"), device=DEV) if want_rgb else None
    g_aff = torch.full((K, 3, 2), float("nan"), device=DEV) if want_affine and d["image"] is not None else None
    ws = torch.full((lib.ego_photo_loss_workspace_bytes(N, K) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(lib.ego_photo_loss(d["rgb"].data_ptr(), d["target"].data_ptr(), _lib.ptr(d["weight"]), _lib.ptr(d["image"]), _lib.ptr(d["affine"]),
                                  N, K, KIND_CODE[kind], ref.PARAM[kind], ws.data_ptr(), _lib.ptr(value), _lib.ptr(g_rgb), _lib.ptr(g_aff),
                                  _lib.stream_handle()), "ego_photo_loss")
    return value, g_rgb, g_aff


def on_device(c):
    return {k: (v if k == "K" else dev(v)) for k, v in c.items()}


def _rel(got, want, scale):
    return float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()) / scale


WORST = dict(value=0.0, g_rgb=0.0, g_affine=0.0)


@pytest.mark.parametrize("K", [1, 3, 67])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 4099])
def test_kernel_against_the_float64_definition(N, K):
    """Every kind and every combination of weight / image / affine at one (N, K): value, g_rgb and g_affine within the rule's bound of
    float64 autograd, no ray excused; invalid rays and empty images exactly 0; all call forms and a repeat return the same bits."""
    for with_weight, with_image, with_affine in FORMS:
        c = ref.make_inputs(N, K, with_weight=with_weight, with_image=with_image, with_affine=with_affine)
        d = on_device(c)
        args = (c["rgb"], c["target"], c["weight"], c["image"], c["affine"])
        ok = ref.valid_mask(c["target"], c["weight"], c["image"], K)
        assert ok.any() and (N < 16 or (~ok).sum() >= 2)
        for kind in ref.KINDS:
            v64, g64, ga64 = ref.autograd_direct(*args, kind, K=K)
            v32, g32, ga32 = ref.kernel_model(*args, kind, K=K, dtype=np.float32)
            value, g_rgb, g_aff = run_kernel(d, kind)
            v_only, _, _ = run_kernel(d, kind, want_rgb=False, want_affine=False)
            _, g_only, ga_only = run_kernel(d, kind, want_value=False)
            value2, g_rgb2, g_aff2 = run_kernel(d, kind)
            tag = f"N={N} K={K} {kind} weight={with_weight} image={with_image} affine={with_affine}"
            got_v = float(value.item())
            assert np.isfinite(got_v) and bool(torch.isfinite(g_rgb).all()), tag
            ev, bv = abs(got_v - v64) / v64, 4.0 * max(abs(v32 - v64) / v64, ref.FLOAT32_HALF_ULP)
            assert v64 > 0 and ev <= bv, (tag, got_v, v64)
            bg, sg = ref.bound(g32, g64)
            eg = _rel(g_rgb, g64, sg)
            assert sg > 0 and eg <= bg, (tag, eg, bg)
            assert bool((g_rgb[dev(~ok)] == 0).all()), tag                      # invalid rays: exactly 0
            WORST.update(value=max(WORST["value"], ev), g_rgb=max(WORST["g_rgb"], eg))
            if with_image:
                # without an affine table d value / d (gain, bias) is taken at the identity
                if not with_affine:
                    _, _, ga64 = ref.autograd_direct(*args[:4], np.tile(np.float32([1, 0]), (K, 3, 1)), kind, K=K)
                    _, _, ga32 = ref.kernel_model(*args[:4], np.tile(np.float32([1, 0]), (K, 3, 1)), kind, K=K, dtype=np.float32)
                ba, sa = ref.bound(ga32, ga64)
                ea = _rel(g_aff, ga64, sa)
                assert bool(torch.isfinite(g_aff).all()) and sa > 0 and ea <= ba, (tag, ea, ba)
                empty = np.bincount(c["image"][ok], minlength=K)[:K] == 0
                assert (K <= N or empty.any()) and bool((g_aff[dev(empty)] == 0).all()), tag   # an image without a valid ray: exactly 0
                WORST["g_affine"] = max(WORST["g_affine"], ea)
                assert torch.equal(bits(ga_only), bits(g_aff)) and torch.equal(bits(g_aff2), bits(g_aff)), tag
            else:
                assert g_aff is None
            # value-only / gradient-only = the joint call, and a repeat returns the same bits
            assert torch.equal(bits(v_only), bits(value)) and torch.equal(bits(g_only), bits(g_rgb)), tag
            assert torch.equal(bits(value2), bits(value)) and torch.equal(bits(g_rgb2), bits(g_rgb)), tag
    print(f"ego_photo_loss N={N} K={K}: worst so far value {WORST['value']:.2e} of |v64|, g_rgb {WORST['g_rgb']:.2e} of max |g64|, "
          f"g_affine {WORST['g_affine']:.2e} of max |ga64|")


@pytest.mark.parametrize("kind", ref.KINDS)
def test_a_batch_without_a_valid_ray(kind):
    c = ref.make_inputs(257, 3)
    c["weight"][:] = 0.0
    c["weight"][5], c["weight"][6] = np.nan, -1.0
    value, g_rgb, g_aff = run_kernel(on_device(c), kind)
    assert float(value.item()) == 0.0 and bool((g_rgb == 0).all()) and bool((g_aff == 0).all())   # W = 0: exactly 0, no NaN


def test_l1_is_flat_where_the_colour_is_met():
    c = ref.make_inputs(65, 1, with_image=False, with_affine=False)
    c["target"][20:30, 1] = c["rgb"][20:30, 1]
    _, g_rgb, _ = run_kernel(on_device(c), "l1")
    ok = ref.valid_mask(c["target"], c["weight"])
    assert ok[20:30].sum() >= 7 and bool((g_rgb[20:30, 1] == 0).all())
    assert bool((g_rgb[dev(ok)][:, 0] != 0).all())


@pytest.mark.parametrize("kind", ref.KINDS)
def test_rays_of_weight_zero_take_no_part(kind):
    """Other finite colours and targets on the weight-0 rays change no output bit."""
    c = ref.make_inputs(257, 3)
    zero = c["weight"] == 0
    assert zero.sum() >= 30
    a = run_kernel(on_device(c), kind)
    c["rgb"][zero], c["target"][zero] = 7.5, -3.25
    b = run_kernel(on_device(c), kind)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))


def test_host_layer_on_the_device():
    c = ref.make_inputs(257, 3)
    d = on_device(c)
    v64, g64, ga64 = ref.autograd_direct(c["rgb"], c["target"], c["weight"], c["image"], c["affine"], "huber")
    rgb, aff = d["rgb"].clone().requires_grad_(True), d["affine"].clone().requires_grad_(True)
    tgt, w = d["target"].clone().requires_grad_(True), d["weight"].clone().requires_grad_(True)
    loss = photometric_loss(rgb, tgt, weight=w, image=d["image"].long(), affine=aff, kind="huber")    # int64 indices are converted
    assert loss.dtype == torch.float32 and loss.shape == () and abs(loss.item() - v64) <= 2.0 ** -23 * v64
    (loss * 3.0).backward()
    assert _rel(rgb.grad / 3.0, g64, np.abs(g64).max()) <= 4 * 2.0 ** -23 and _rel(aff.grad / 3.0, ga64, np.abs(ga64).max()) <= 4 * 2.0 ** -23
    assert tgt.grad is None and w.grad is None                                   # rgb and affine are the differentiable inputs
    plain = photometric_loss(d["rgb"], d["target"])                              # the defaults: the MSE over the finite targets
    fin = np.isfinite(c["target"]).all(1)
    mse = float(np.mean((c["rgb"][fin].astype(np.float64) - c["target"][fin]) ** 2))
    assert not plain.requires_grad and abs(plain.item() - mse) <= 2.0 ** -23 * mse
    # image without affine: only negative indices are invalid
    v_img = photometric_loss(d["rgb"], d["target"], image=d["image"])
    keep = fin & (c["image"] >= 0)
    assert abs(v_img.item() - float(np.mean((c["rgb"][keep].astype(np.float64) - c["target"][keep]) ** 2))) <= 2.0 ** -23 * mse
    with pytest.raises(RuntimeError, match="rgb's device"):
        photometric_loss(d["rgb"], d["target"].cpu())


# ---- the fit ----
def run_fit(d, K, with_Wk=True):
    lib = _lib.load()
    out = torch.full((K, 3, 2), float("nan"), device=DEV)
    Wk = torch.full((K,), float("nan"), dtype=torch.float64, device=DEV) if with_Wk else None
    _lib.check(lib.ego_photo_fit(d["rgb"].data_ptr(), d["target"].data_ptr(), _lib.ptr(d["weight"]), _lib.ptr(d["image"]), d["rgb"].shape[0], K,
                                 out.data_ptr(), _lib.ptr(Wk), _lib.stream_handle()), "ego_photo_fit")
    return out, Wk


def _l2_affine_gradient_scale(c, affine, K):
    """The size of the terms that cancel in d L2 / d (gain, bias) = (2 / 3W) sum w (gain c + bias - t) (c, 1): (2 / 3W) sum w (|gain c| +
    |bias| + |t|) max(|c|, 1), the largest over (k, ch).  Storing the fitted map as float32 moves it by up to 2^-24 of itself, which
    moves the gradient by up to that share of this sum: the gradient at a float32 minimiser is 0 to within the rule's bound OF THIS
    SCALE, not of itself."""
    ok, x, t, w, img, _, _ = ref._clean(c["rgb"], c["target"], c["weight"], c["image"], None, K)
    a = np.asarray(affine, np.float64)
    terms = w[:, None] * (np.abs(a[img, :, 0] * x) + np.abs(a[img, :, 1]) + np.abs(t)) * np.maximum(np.abs(x), 1.0)
    acc = np.zeros((K, 3))
    np.add.at(acc, img[ok], terms[ok])
    return float(2.0 * acc.max() / (3.0 * w.sum()))


@pytest.mark.parametrize("N,K,with_weight,with_image", [(1, 1, False, False), (2, 1, True, False), (63, 3, True, True), (64, 1, False, True),
                                                        (65, 67, True, True), (257, 3, False, True), (4099, 3, True, True),
                                                        (4099, 67, True, True), (4099, 1, True, False)])
def test_fit_against_the_float64_restatement(N, K, with_weight, with_image):
    c = ref.make_inputs(N, K, with_weight=with_weight, with_image=with_image, with_affine=False)
    d = on_device(c)
    a64, W64 = ref.fit_model(c["rgb"], c["target"], c["weight"], c["image"], K)
    a32, _ = ref.fit_model(c["rgb"], c["target"], c["weight"], c["image"], K, dtype=np.float32)
    got, Wk = run_fit(d, K)
    got2, _ = run_fit(d, K, with_Wk=False)
    assert bool(torch.isfinite(got).all()) and torch.equal(bits(got), bits(got2))            # a repeat, and without W_k: the same bits
    b, s = ref.bound(a32, a64)
    e = _rel(got, a64, s)
    print(f"ego_photo_fit N={N} K={K}: {e:.2e} of max |affine64| (bound {b:.2e})")
    assert e <= b
    assert np.abs(Wk.cpu().numpy() - W64).max() <= 1e-12 * max(W64.max(), 1.0)
    empty = W64 == 0
    assert (K <= N or empty.any()) and torch.equal(got[dev(empty)], torch.tensor([1.0, 0.0], device=DEV).expand(int(empty.sum()), 3, 2))
    if N >= 63 and with_image and not empty.any():
        # the L2 term's gradient with respect to affine at the fitted values: within the rule's bound of 0
        dd = dict(d, affine=got.contiguous())
        _, _, ga = run_kernel(dd, "l2", K=K)
        _, _, ga32 = ref.kernel_model(c["rgb"], c["target"], c["weight"], c["image"], a32, "l2", K=K, dtype=np.float32)
        scale = _l2_affine_gradient_scale(c, a64, K)
        bound = 4.0 * max(float(np.abs(ga32).max()) / scale, ref.FLOAT32_HALF_ULP)
        err = float(ga.abs().max()) / scale
        print(f"  d L2 / d affine at the fit: {err:.2e} of the cancelling terms (bound {bound:.2e})")
        assert err <= bound


def test_fit_of_an_image_of_one_colour():
    rgb = np.full((130, 3), 0.25, np.float32)
    rgb[:, 1] = np.linspace(0.1, 0.9, 130)
    target = (rgb * np.float32(1.2) + np.float32(0.1)).astype(np.float32)
    image = (np.arange(130) % 2 * 2).astype(np.int32)     # images 0 and 2; image 1 has no ray
    c = dict(rgb=rgb, target=target, weight=None, image=image)
    got, Wk = run_fit(on_device(c), 3)
    a64, _ = ref.fit_model(rgb, target, None, image, 3)
    assert Wk.tolist() == [65.0, 0.0, 65.0]
    got = got.cpu().numpy()
    assert np.array_equal(got[1], np.tile(np.float32([1, 0]), (3, 1)))                            # W_k = 0: the identity
    assert got[0, 0, 0] == 1 and got[2, 2, 0] == 1                                                # equal colours: gain 1 ...
    assert abs(float(got[0, 0, 1]) - a64[0, 0, 1]) <= 2.0 ** -23 * abs(a64[0, 0, 1])              # ... and the gap of the means
    assert np.abs(got[[0, 2], 1] - a64[[0, 2], 1]).max() <= 4 * 2.0 ** -24 * 1.2
    assert torch.equal(fit_exposure(dev(rgb), dev(target), image=dev(image), K=3), dev(got))      # the host layer is this call


def test_fit_recovers_known_exposures_from_quantised_images_under_a_mask():
    """K = 3 rendered-like images of 16 x 32 random colours; the 'photographs' are those colours under a known gain and bias per image,
    quantised to 8 bits, with a block overwritten by magenta (the photographer) that the mask covers.  Fitted from the mask-weighted
    pixels, the kernel's map is as close to the truth as the float64 restatement's own fit (quantisation limits both) plus the
    kernel-vs-restatement bound; fitted without the mask it is farther."""
    g = np.random.default_rng(42)
    K, H, W = 3, 16, 32
    pred = g.uniform(0.05, 0.7, (K, H, W, 3)).astype(np.float32)
    truth = np.stack([g.uniform(0.7, 1.3, (K, 3)), g.uniform(-0.05, 0.05, (K, 3))], -1)
    photo = np.rint((truth[:, None, None, :, 0] * pred + truth[:, None, None, :, 1]) * 255.0)
    assert photo.min() >= 0 and photo.max() <= 255
    photo = photo.astype(np.uint8)
    mask = np.full((K, H, W), 255, np.uint8)
    mask[:, 10:16, 8:24] = 0
    photo[:, 10:16, 8:24] = (255, 0, 255)
    rgb, target = pred.reshape(-1, 3), (photo.astype(np.float32) / np.float32(255)).reshape(-1, 3)
    image = np.repeat(np.arange(K, dtype=np.int32), H * W)
    weight = (mask.astype(np.float32) / np.float32(255)).reshape(-1)
    a64, _ = ref.fit_model(rgb, target, weight, image, K)
    a32, _ = ref.fit_model(rgb, target, weight, image, K, dtype=np.float32)
    b, s = ref.bound(a32, a64)
    got = fit_exposure(dev(rgb), dev(target), image=dev(image), K=K, weight=dev(weight)).cpu().numpy().astype(np.float64)
    unmasked = fit_exposure(dev(rgb), dev(target), image=dev(image), K=K).cpu().numpy().astype(np.float64)
    err, err64, err_un = np.abs(got - truth).max(), np.abs(a64 - truth).max(), np.abs(unmasked - truth).max()
    print(f"recovery: kernel {err:.3e}, float64 restatement {err64:.3e} (+ {b * s:.1e}), without the mask {err_un:.3e}")
    assert err64 < 2e-3                       # 8-bit quantisation over 416 pixels per image leaves the truth this close
    assert err <= err64 + b * s
    assert err_un > 10 * err                  # the mask matters
    # the evaluation protocol: one image pair, aligned, scored under its mask
    p0, gt0 = dev(pred[1]), dev(target.reshape(K, H, W, 3)[1])
    aligned, a1 = align(p0, gt0, mask=dev(mask[1]))
    assert a1.shape == (1, 3, 2) and np.abs(a1[0].cpu().numpy() - got[1]).max() <= 2.0 ** -22 and torch.equal(aligned, apply_exposure(p0, a1))
    scored, raw = psnr(aligned, gt0, mask=dev(mask[1])), psnr(p0, gt0, mask=dev(mask[1]))
    print(f"  PSNR under the mask: {raw:.1f} dB as rendered, {scored:.1f} dB aligned")
    assert scored > 45 and scored > raw + 10      # 8-bit quantisation alone leaves 58.9 dB


# ---- the bank's masks ----
def _mask_bank(K=2, H=6, W=8, roi=(0.25, 0.75, 0.25, 1), seed=3):
    g = np.random.default_rng(seed)
    poses = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
    poses[:, :3, 3] = g.uniform(-0.2, 0.2, (K, 3))
    masks = g.integers(0, 256, (K, H, W)).astype(np.uint8)
    masks[g.uniform(size=masks.shape) < 0.3] = 0
    masks[g.uniform(size=masks.shape) < 0.3] = 255
    return RayBank(poses, g.integers(0, 256, (K, H, W, 3), dtype=np.uint8), (W, H), roi=roi, device=DEV, masks=masks), masks


def test_bank_gathers_the_mask_of_each_ray_s_pixel():
    bank, masks = _mask_bank()
    assert (bank.r0, bank.n_rows, bank.c0, bank.n_cols) == (1, 3, 2, 6) and bank.total == 36
    assert bank.nbytes == 2 * 6 * 8 * 4 + 2 * 48 + masks.nbytes
    idx = torch.arange(bank.total - 1, -1, -1, device=DEV)
    window = (masks[:, 1:4, 2:8].astype(np.float32) / np.float32(255)).reshape(-1)     # the materialised array, in all_rays' index space
    got = bank.gather_mask(idx)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.int32), window[::-1].view(np.int32))
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0 and 0.0 < float(got[got > 0].min()) < 1.0
    out = bank.gather_mask(torch.tensor([0, -1, bank.total, 35, 2 ** 40], device=DEV))
    assert np.array_equal(np.isnan(out.cpu().numpy()), [False, True, True, False, True])   # outside the bank: NaN, nothing read
    assert float(out[0]) == window[0] and float(out[3]) == window[35]
    with pytest.raises(RuntimeError, match="int64"):
        bank.gather_mask_into(idx.int(), torch.empty(bank.total, device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        bank.gather_mask_into(idx, torch.empty(bank.total - 1, device=DEV))
    # all 256 values divide as numpy divides them
    every = np.arange(256, dtype=np.uint8).reshape(1, 8, 32)
    b2 = RayBank(np.eye(4, dtype=np.float32)[None], np.zeros((1, 8, 32, 3), np.uint8), (32, 8), device=DEV, masks=every)
    got = b2.gather_mask(torch.arange(256, device=DEV)).cpu().numpy()
    assert np.array_equal(got.view(np.int32), (np.arange(256, dtype=np.float32) / np.float32(255)).view(np.int32))


# ---- exposure-only optimisation ----
def _capture(K=3, H=16, W=32, seed=8):
    """A bank of K 'photographs' with per-image exposure and a masked magenta block, and the fixed colours a perfect field would
    render for its pixels (before exposure) -> (bank, pred [K H W, 3] device, truth [K,3,2])"""
    g = np.random.default_rng(seed)
    pred = g.uniform(0.05, 0.7, (K, H, W, 3)).astype(np.float32)
    truth = np.stack([g.uniform(0.7, 1.3, (K, 3)), g.uniform(-0.05, 0.05, (K, 3))], -1)
    truth[0] = (1.0, 0.0)
    photo = np.rint((truth[:, None, None, :, 0] * pred + truth[:, None, None, :, 1]) * 255.0).astype(np.uint8)
    mask = np.full((K, H, W), 255, np.uint8)
    mask[:, 10:16, 8:24] = 0
    mask[:, 9, 8:24] = 128
    photo[:, 10:16, 8:24] = (255, 0, 255)
    q, _ = np.linalg.qr(g.standard_normal((K, 3, 3)))
    poses = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
    poses[:, :3, :3] = q
    poses[:, :3, 3] = g.uniform(-0.25, 0.25, (K, 3))
    return RayBank(poses, photo, (W, H), device=DEV, masks=mask), dev(pred.reshape(-1, 3)), truth


def test_exposure_only_adam_follows_the_float64_loop():
    """60 Adam steps on the exposure parameters alone, 256 rays each, the predicted colours fixed: the HIP term + FusedAdam against the
    same loop in float64 torch (autograd through the definition, torch's Adam), compared the way the graph tests compare parameters
    after Adam steps; the mask-weighted loss over all pixels falls."""
    STEPS, B, LR = 60, 256, 0.01
    bank, pred, _ = _capture()
    src = DeviceSimpleSampler(bank, B, seed=13)
    everything = torch.arange(bank.total, device=DEV)
    _, all_t = bank.gather(everything)
    all_w, all_i = bank.gather_mask(everything), bank.image_of(everything)
    deltas = ExposureDeltas(bank.K, device=DEV, anchor=0)
    whole = lambda: float(photometric_loss(pred, all_t, weight=all_w, image=all_i, affine=deltas.affine().detach(), kind="huber"))
    before = whole()
    opt = FusedAdam([dict(params=list(deltas.parameters()), lr=LR)], betas=(0.9, 0.99))
    d64 = ExposureDeltas(bank.K, anchor=0).double()
    opt64 = torch.optim.Adam(d64.parameters(), lr=LR, betas=(0.9, 0.99), eps=1e-8)
    p64, t64, w64 = pred.cpu().double(), all_t.cpu().double(), all_w.cpu().double()
    for k in range(STEPS):
        idx = src.indices_at(k)
        loss = photometric_loss(pred[idx], all_t[idx], weight=all_w[idx], image=all_i[idx], affine=deltas.affine(), kind="huber")
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        i = idx.cpu()
        r = apply_exposure(p64[i], d64.affine(), all_i.cpu()[i]) - t64[i]
        rho = torch.where(r.abs() <= 0.1, 0.5 * r * r, 0.1 * (r.abs() - 0.05))
        loss64 = (w64[i][:, None] * rho).sum() / (3.0 * w64[i].sum())
        opt64.zero_grad(set_to_none=True)
        loss64.backward()
        opt64.step()
        assert abs(float(loss) - float(loss64)) <= 1e-4 * float(loss64), k
    after = whole()
    print(f"exposure-only Adam, {STEPS} steps: masked loss over all pixels {before:.4e} -> {after:.4e}")
    assert after < before
    for name, a, b in (("log_gain", d64.log_gain, deltas.log_gain), ("bias", d64.bias, deltas.bias)):
        _same_after_adam(name, a.detach().float(), b.detach().cpu(), n_steps=STEPS, lr=LR)
    assert bool((deltas.log_gain[0] == 0).all()) and bool((deltas.bias[0] == 0).all())     # the anchor never moved


# ---- the captured step ----
KW = dict(n_coarse=8, n_fine=8, exp_sampling=True, resampling=True, use_coarse_sample=True)
N_IT, FACTOR, BATCH, LR_EXPOSURE = 5, 0.95, 64, 5e-3
ANCHOR_BITS = (0.125, -0.25)   # what the anchor's parameters hold: they take no part and must keep their bits


def _photo_loss_of(deltas):
    def loss_fn(rgb, gt, alpha, weight, image):
        return photometric_loss(rgb, gt, weight=weight, image=image, affine=deltas.affine(), kind="charbonnier")
    return loss_fn


def _model_and_deltas(capturable):
    _, m = _setup(6)
    deltas = ExposureDeltas(3, device=DEV, anchor=0)
    with torch.no_grad():
        deltas.log_gain[0], deltas.bias[0] = ANCHOR_BITS
    groups = m.get_optparam_groups(0.02, 1e-3) + [dict(params=list(deltas.parameters()), lr=LR_EXPOSURE)]
    opt = FusedAdam(groups, betas=(0.9, 0.99), **(dict(capturable=True, lr_factor=FACTOR) if capturable else {}))
    return m, deltas, opt


@functools.lru_cache(maxsize=None)
def _eager_run():
    """The eager loop on the bank's first N_IT batches; computed once."""
    bank, _, _ = _capture()
    src = DeviceSimpleSampler(bank, BATCH, seed=77)
    jit = torch.from_numpy(synth.hash_uniform(19, 0, BATCH * 8).reshape(BATCH, 8).astype(np.float32)).to(DEV)
    batches = []
    for k in range(N_IT):
        idx = src.indices_at(k)
        batches.append((*bank.gather(idx), bank.gather_mask(idx), bank.image_of(idx).int()))
    m, deltas, opt = _model_and_deltas(capturable=False)
    loss_fn, losses = _photo_loss_of(deltas), []
    for rays, gt, weight, image in batches:
        rgb, _d, _bg, _env, alpha = m(rays, is_train=True, jitter=jit, u=jit, **KW)
        loss = loss_fn(rgb, gt, alpha, weight, image)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        for grp in opt.param_groups:
            grp["lr"] *= FACTOR
        m.update_coarse_sigma_grid()
        losses.append(float(loss.detach()))
    params = {k: p.detach().clone() for k, p in list(m.named_parameters()) + [("exposure." + k, p) for k, p in deltas.named_parameters()]}
    return bank, jit, batches, losses, params


def _check_against_eager(step, m_g, deltas, got):
    _, _, _, ref_losses, ref_params = _eager_run()
    assert step.iterations == N_IT
    for a, b in zip(ref_losses[1:], got):
        assert abs(a - b) <= 5e-5 * max(abs(a), 1e-3), (ref_losses, got)
    pg = dict(list(m_g.named_parameters()) + [("exposure." + k, p) for k, p in deltas.named_parameters()])
    for k in ref_params:
        _same_after_adam(k, ref_params[k], pg[k].detach(), n_steps=N_IT, lr=0.02)
    moved = float(pg["exposure.log_gain"][1:].detach().abs().max())
    assert moved > LR_EXPOSURE                                                    # the exposure group is stepped by the same optimiser
    for p, v in zip((deltas.log_gain, deltas.bias), ANCHOR_BITS):
        assert torch.equal(bits(p.detach()[0]), bits(torch.full((3,), v, device=DEV)))    # the anchor row keeps its bits


def test_graphed_step_with_masks_and_exposure_fed_from_the_bank():
    """photometric_loss with the bank's masks, the rays' image indices and ExposureDeltas(anchor=0) inside the captured step, the batch,
    its weights and its image indices drawn inside the graph: four replays with pinned noise against the eager loop, at the tolerances
    of tests/test_hip_train_graph.py."""
    bank, jit, batches, _, _ = _eager_run()
    m_g, deltas, o_g = _model_and_deltas(capturable=True)
    src = DeviceSimpleSampler(bank, BATCH, seed=77)
    step = GraphedTrainStep(m_g, o_g, render_kwargs=KW, loss_fn=_photo_loss_of(deltas), warmup=1, noise_fn=lambda a, b, d: jit, batch_source=src)
    assert step.weight.dtype == torch.float32 and step.image.dtype == torch.int32
    assert torch.equal(step.weight, batches[0][2]) and torch.equal(step.image, batches[0][3])
    got = []
    for k in range(1, N_IT):
        got.append(float(step()))
        assert torch.equal(step.weight, batches[k][2]) and torch.equal(step.image, batches[k][3]) and torch.equal(step.rays, batches[k][0])
    assert any(float((b[2] == 0).sum()) > 0 for b in batches) and any(0 < float(b[2][b[2] > 0].min()) < 1 for b in batches)
    _check_against_eager(step, m_g, deltas, got)
    with pytest.raises(ValueError, match="batch_source"):
        step(weight=step.weight)


def test_graphed_step_with_masks_and_exposure_fed_from_the_host():
    bank, jit, batches, _, _ = _eager_run()
    m_g, deltas, o_g = _model_and_deltas(capturable=True)
    rays0, gt0, w0, i0 = batches[0]
    loss_fn = _photo_loss_of(deltas)
    with pytest.raises(ValueError, match="no weight source"):
        GraphedTrainStep(m_g, o_g, rays0, gt0, KW, loss_fn=loss_fn, warmup=1, image=i0)
    with pytest.raises(ValueError, match="no image source"):
        GraphedTrainStep(m_g, o_g, rays0, gt0, KW, loss_fn=loss_fn, warmup=1, weight=w0)
    with pytest.raises(ValueError, match="no image source"):
        GraphedTrainStep(m_g, o_g, rays0, gt0, KW, loss_fn=lambda rgb, gt, alpha, image: torch.mean((rgb - gt) ** 2), warmup=1)
    plain = RayBank(bank.poses.cpu().numpy(), np.zeros((3, 16, 32, 3), np.uint8), (32, 16), device=DEV)
    with pytest.raises(ValueError, match="has no masks"):
        GraphedTrainStep(m_g, o_g, render_kwargs=KW, loss_fn=loss_fn, warmup=1, batch_source=DeviceSimpleSampler(plain, BATCH, seed=1))
    with pytest.raises(ValueError, match="no parameter named `weight`"):
        GraphedTrainStep(m_g, o_g, rays0, gt0, KW, warmup=1, weight=w0)
    step = GraphedTrainStep(m_g, o_g, rays0, gt0, KW, loss_fn=loss_fn, warmup=1, noise_fn=lambda a, b, d: jit, weight=w0, image=i0.long())
    got = [float(step(rays, gt, weight=w, image=i)) for rays, gt, w, i in batches[1:]]
    _check_against_eager(step, m_g, deltas, got)
    with pytest.raises(ValueError, match="weight="):
        step(rays0, gt0, image=i0)
