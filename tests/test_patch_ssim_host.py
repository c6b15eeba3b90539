"""CPU: the structural term's float64 definition against its closed form and finite differences, the luminance limit, every refusal of
losses.patch_ssim_loss, sampler.DevicePatchSampler and data.patch_indices with its message, and properties of the patch mode's index rule
(tests/patch_batch_ref.py) at a fixed seed.  No GPU: the kernels are checked in tests/test_hip_patch_ssim.py."""
import numpy as np
import pytest
import torch

from egonerf_amd.data import RayBank, patch_indices
from egonerf_amd.losses import patch_ssim_loss
from egonerf_amd.sampler import DevicePatchSampler
from tests import patch_batch_ref as bref
from tests import patch_ssim_ref as ref


@pytest.mark.parametrize("P,ph,pw,fs,with_weight", [(1, 3, 3, 3, False), (3, 5, 7, 5, True), (4, 8, 8, 7, True), (2, 9, 9, 7, False),
                                                   (2, 4, 6, 1, True), (2, 16, 16, 11, True)])
def test_autograd_equals_the_closed_form(P, ph, pw, fs, with_weight):
    c = ref.make_inputs(P, ph, pw, fs, with_weight=with_weight)
    v, g = ref.autograd_direct(c["rgb"], c["target"], (ph, pw), P, c["weight"], fs)
    v2, g2 = ref.kernel_model(c["rgb"], c["target"], (ph, pw), P, c["weight"], fs)
    _, wv = ref.window_valid(c["target"], c["weight"], P, ph, pw, fs)
    assert wv.any() and (P < 2 or not wv[1].any())
    assert 0.0 < v < 1.0 and abs(v - v2) <= 1e-13
    assert np.abs(g).max() > 0 and np.abs(g - g2).max() <= 1e-13 * max(np.abs(g).max(), 1.0)
    assert (g[P * ph * pw:] == 0).all() and (g2[P * ph * pw:] == 0).all()
    unc = ~ref.covered(wv, ph, pw, fs).reshape(-1)
    assert (g[:P * ph * pw][unc] == 0).all() and (g2[:P * ph * pw][unc] == 0).all()


def test_closed_form_against_central_differences():
    P, ph, pw, fs = 2, 5, 7, 5
    c = ref.make_inputs(P, ph, pw, fs, with_weight=True, invalid=False, tail=0)
    rgb = c["rgb"].astype(np.float64)
    _, g = ref.kernel_model(rgb, c["target"], (ph, pw), P, c["weight"], fs)
    h = 1e-6
    for e, ch in [(0, 0), (17, 1), (34, 2), (35, 0), (52, 1), (69, 2)]:
        up, dn = rgb.copy(), rgb.copy()
        up[e, ch] += h
        dn[e, ch] -= h
        fd = (ref.kernel_model(up, c["target"], (ph, pw), P, c["weight"], fs)[0] - ref.kernel_model(dn, c["target"], (ph, pw), P, c["weight"], fs)[0]) / (2 * h)
        assert abs(fd - g[e, ch]) <= 1e-8 * np.abs(g).max() + 1e-9, (e, ch, fd, g[e, ch])


def test_a_constant_window_gives_the_luminance_term():
    a, b, fs = 0.3, 0.65, 7
    rgb, target = np.full((49, 3), a, np.float32), np.full((49, 3), b, np.float32)
    v, _ = ref.autograd_direct(rgb, target, (7, 7), 1, None, fs)
    a, b = float(np.float32(a)), float(np.float32(b))
    C1 = 0.01 ** 2
    assert abs((1.0 - v) - (2 * a * b + C1) / (a * a + b * b + C1)) <= 1e-12
    v_same, g_same = ref.autograd_direct(rgb, rgb, (7, 7), 1, None, fs)
    assert abs(v_same) <= 1e-12 and np.abs(g_same).max() <= 1e-9     # SSIM of an image with itself is 1, and that is its maximum


def test_the_taps_are_the_metric_s():
    g = ref.taps(11)
    assert abs(g.sum() - 1) < 1e-15 and np.allclose(g, g[::-1]) and g.argmax() == 5
    assert np.allclose(g[5] / g[4], np.exp(0.5 / 1.5 ** 2))
    assert np.allclose(ref.taps(4), ref.taps(4)[::-1])                 # an even window is centred between two pixels


def test_refusals_of_patch_ssim_loss():
    x, t = torch.zeros(128, 3), torch.zeros(128, 3)
    for kw, err, msg in [(dict(patch=8), ValueError, r"patch must be \(ph, pw\)"),
                         (dict(patch=(8, 8), filter_size=0), ValueError, "filter_size must be 1..15"),
                         (dict(patch=(16, 8), filter_size=16), ValueError, "filter_size must be 1..15"),
                         (dict(patch=(8, 6), filter_size=7), ValueError, "must cover the filter"),
                         (dict(patch=(33, 8)), ValueError, "at most 32 x 32"),
                         (dict(patch=(8, 8), filter_sigma=0.0), ValueError, "filter_sigma"),
                         (dict(patch=(8, 8), filter_sigma=float("nan")), ValueError, "filter_sigma"),
                         (dict(patch=(7, 7)), ValueError, "not a whole number of 7 x 7 patches"),
                         (dict(patch=(8, 8), n_patches=3), ValueError, "do not fit 128 rows"),
                         (dict(patch=(8, 8), n_patches=-1), ValueError, "do not fit"),
                         (dict(patch=(8, 8), weight=torch.zeros(127)), RuntimeError, r"weight must be a float32 \[B\]"),
                         (dict(patch=(8, 8), weight=torch.zeros(128, dtype=torch.float64)), RuntimeError, "weight must be a float32"),
                         (dict(patch=(8, 8)), RuntimeError, "needs a HIP device tensor")]:
        with pytest.raises(err, match=msg):
            patch_ssim_loss(x, t, **kw)
    with pytest.raises(RuntimeError, match=r"rgb must be a float32 \[B, 3\]"):
        patch_ssim_loss(torch.zeros(128, 4), t, (8, 8))
    with pytest.raises(RuntimeError, match=r"rgb must be a float32 \[B, 3\]"):
        patch_ssim_loss(x.double(), t, (8, 8))
    with pytest.raises(RuntimeError, match=r"target must be a float32 \[B, 3\]"):
        patch_ssim_loss(x, t.double(), (8, 8))
    with pytest.raises(RuntimeError, match="target must be a float32"):
        patch_ssim_loss(x, t[:64], (8, 8))


def _bank(roi=(0, 1, 0, 1), K=3, H=16, W=32):
    poses = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
    return RayBank(poses, np.zeros((K, H, W, 3), np.uint8), (W, H), roi=roi, device="cpu")


def test_refusals_of_the_sampler_and_of_patch_indices():
    bank = _bank()
    for kw, msg in [(dict(patches=-1), "patches and n_random must be >= 0"), (dict(patches=2, n_random=-3), "patches and n_random must be >= 0"),
                    (dict(patches=2, patch=(0, 4)), "ph, pw and stride must be >= 1"), (dict(patches=2, patch=(4, 4), stride=0), "must be >= 1"),
                    (dict(patches=2, patch=4), r"patch must be \(ph, pw\)"),
                    (dict(patches=2, patch=(17, 4)), "17 x 4 pixels does not fit the bank's window of 16 x 32"),
                    (dict(patches=2, patch=(4, 12), stride=3), "10 x 34 pixels does not fit"),     # also on a window that wraps
                    (dict(patches=0, n_random=0), "batch must be >= 1")]:
        with pytest.raises(ValueError, match=msg):
            DevicePatchSampler(bank, **kw)
    s = DevicePatchSampler(bank, patches=5, patch=(3, 5), stride=2, n_random=7, seed=-1)
    assert (s.n_patch_rays, s.batch, s.patch, s.stride, s.seed) == (75, 82, (3, 5), 2, 2 ** 64 - 1) and s.counter.dtype == torch.int64
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        s.indices_at(0)
    roi_bank = _bank(roi=(0.25, 1, 0.25, 0.75))
    assert (roi_bank.n_rows, roi_bank.n_cols) == (12, 16)
    for args, msg in [(([0], [0], [0], (0, 2)), "must be >= 1"), (([0], [0], [0], (13, 2)), "does not fit"),
                      (([0, 1], [0], [0], (2, 2)), "one length"), (([3], [0], [0], (2, 2)), "outside the bank"),
                      (([0], [11], [0], (2, 2)), "outside the bank"), (([0], [0], [15], (2, 2)), "outside the bank"),
                      (([0], [-1], [0], (2, 2)), "outside the bank")]:
        with pytest.raises(ValueError, match=msg):
            patch_indices(roi_bank, *args)
    with pytest.raises(ValueError, match="outside the bank"):
        patch_indices(bank, [0], [0], [32], (2, 2))
    got = patch_indices(bank, [2], [14], [31], (2, 2))                               # a full-width window wraps
    assert got.tolist() == [2 * 512 + 14 * 32 + 31, 2 * 512 + 14 * 32, 2 * 512 + 15 * 32 + 31, 2 * 512 + 15 * 32]
    got = patch_indices(roi_bank, [1], [9], [11], (2, 3), stride=2).view(2, 3)        # the last origin that fits a window that does not wrap
    assert got.tolist() == [[192 + 144 + 11, 192 + 144 + 13, 192 + 144 + 15], [192 + 176 + 11, 192 + 176 + 13, 192 + 176 + 15]]


@pytest.mark.parametrize("roi", [(0, 1, 0, 1), (0.25, 1, 0.25, 0.75)])
@pytest.mark.parametrize("patch,stride", [((4, 4), 1), ((3, 5), 2)])
def test_properties_of_the_index_rule(roi, patch, stride):
    """Over 200 iterations on a 3-image 16 x 32 bank: every patch inside the ROI, seam-crossing patches iff the window spans the full
    width, every image and every admissible origin row drawn; the restatement's index block is data.patch_indices' of its origins."""
    bank = _bank(roi)
    K, nr, nc = bank.K, bank.n_rows, bank.n_cols
    wrap = bref.wraps(bank.c0, nc, bank.W)
    assert wrap == (roi == (0, 1, 0, 1))
    ph, pw = patch
    P, R, seed = 6, 37, 20221028
    imgs, rows0, seam = set(), set(), 0
    for c in range(200):
        img, row0, col0 = bref.patch_origins(K, nr, nc, wrap, P, patch, stride, seed, c)
        rows, cols = bref.patch_pixels(nc, wrap, row0, col0, patch, stride)
        assert img.min() >= 0 and img.max() < K and rows.min() >= 0 and rows.max() < nr and cols.min() >= 0 and cols.max() < nc
        assert (np.diff(rows, axis=1) == stride).all()
        crossing = (np.diff(cols, axis=1) != stride).any(1)
        assert (np.diff(cols, axis=1)[~crossing] == stride).all()
        seam += int(crossing.sum())
        imgs |= set(img.tolist())
        rows0 |= set(row0.tolist())
        idx = bref.patch_batch_indices(K, nr, nc, wrap, P, patch, stride, R, seed, c)
        assert idx.shape == (P * ph * pw + R,) and idx.min() >= 0 and idx.max() < bank.total
        assert np.array_equal(idx[:P * ph * pw], patch_indices(bank, img, row0, col0, patch, stride).numpy())
        if c == 0:
            first = idx
        elif c == 1:
            assert not np.array_equal(idx, first)
    assert (seam > 0) == wrap
    assert imgs == set(range(K)) and rows0 == set(range(nr - (ph - 1) * stride))
    again = bref.patch_batch_indices(K, nr, nc, wrap, P, patch, stride, R, seed, 0)
    assert np.array_equal(again, first)
    other = bref.patch_batch_indices(K, nr, nc, wrap, P, patch, stride, R, seed + 1, 0)
    assert not np.array_equal(other, first)
    # the trailing rows cover the window: every row and column of it is drawn over the iterations' 200 x 37 pixels
    rr = np.concatenate([np.stack(bref.random_pixels(K, nr, nc, R, seed, c)) for c in range(200)], 1)
    assert set(rr[0].tolist()) == set(range(K)) and set(rr[1].tolist()) == set(range(nr)) and set(rr[2].tolist()) == set(range(nc))
