"""GPU: device-resident training batches - RayBank.gather against the materialised all_rays / all_rgbs (bit for bit) and the
reference's own arrays, the device index generator against its numpy restatement (tests/ray_bank_ref.py), the distribution of the
theta_importance draws, and GraphedTrainStep(batch_source=...) - the batch drawn inside the replayed graph - against the host-fed
step on the same batches."""
import numpy as np
import pytest
import torch

from egonerf_amd import synth
from egonerf_amd.data import OmniBlenderDataset, RayBank
from egonerf_amd.optim import FusedAdam
from egonerf_amd.renderer import erp_rays
from egonerf_amd.sampler import DeviceSimpleSampler, DeviceThetaImportanceSampler
from egonerf_amd.train import GraphedTrainStep
from tests import ray_bank_ref as ref
from tests.helpers import make_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
KW = dict(n_coarse=16, n_fine=16, exp_sampling=True, resampling=True, use_coarse_sample=True)
ROI = [0.25, 1.0, 0.0, 0.5]
SEED = 0x5EEDFACE12345678
COUNTERS = (0, 1, 2, (1 << 40) + 12345)


def _build(fx, d):
    """The omniblender fixture as a dataset directory (as tests/test_data_ingestion.py::_build does)."""
    import os
    from PIL import Image
    os.makedirs(os.path.join(d, "images"))
    open(os.path.join(d, "transform.json"), "w").write(str(fx["frames_json"]))
    open(os.path.join(d, "train.txt"), "w").write(str(fx["train_list"]))
    open(os.path.join(d, "test.txt"), "w").write(str(fx["test_list"]))
    for k in fx.files:
        if k.startswith("png/"):
            Image.fromarray(fx[k], "RGBA").save(os.path.join(d, "images", k[4:] + ".png"))
    return str(d)


def _random_poses(K, g, extent=0.25):
    q, _ = np.linalg.qr(g.standard_normal((K, 3, 3)))
    poses = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
    poses[:, :3, :3] = q
    poses[:, :3, 3] = g.uniform(-extent, extent, (K, 3))
    return poses


def _synthetic_bank(K=16, H=250, W=500, roi=(0, 1, 0, 1), seed=7, channels=4):
    g = np.random.default_rng(seed)
    return RayBank(_random_poses(K, g), g.integers(0, 256, (K, H, W, channels), dtype=np.uint8), (W, H), roi=roi, device=DEV)


def _reference_rgb(images_u8):
    """dataset_omniblender.py:75-80 on the CPU: ToTensor's u8 / 255, then the blend on white, as separate ATen operations."""
    t = images_u8.cpu().float().div(255.0)
    return t[..., :3] * t[..., -1:] + (1 - t[..., -1:])


def _window(x, bank):
    """[K, H, W, c] -> the rows of the bank's index space."""
    return x[:, bank.r0:bank.r0 + bank.n_rows, bank.c0:bank.c0 + bank.n_cols].reshape(bank.total, -1)


# ---- gather ------------------------------------------------------------------------------------------------------------------------

def test_gather_equals_materialised_arrays_on_the_fixture(golden, tmp_path):
    fx = golden("omniblender")
    d = _build(fx, tmp_path)
    ds = OmniBlenderDataset(d, split="train", near_far=[0.01, 15.0], downsample=250.0, device=DEV)
    bank = ds.ray_bank()
    assert ds._rays is None                                            # building the bank materialised nothing
    assert bank.nbytes == 2 * 4 * 8 * 4 + 2 * 48 and bank.total == 64 and (bank.n_rows, bank.n_cols) == (4, 8)
    rays, rgb = bank.gather(torch.arange(bank.total, device=DEV))
    assert torch.equal(rays, ds.all_rays) and torch.equal(rgb.cpu(), ds.all_rgbs)
    assert np.array_equal(rgb.cpu().numpy(), fx["train/all_rgbs"])    # the reference's own colours, exactly
    assert float((rays.cpu() - torch.from_numpy(fx["train/all_rays"])).abs().max()) <= 1e-6
    # a permuted, repeating index list addresses the same rows
    idx = torch.from_numpy(np.random.default_rng(1).integers(0, 64, 200)).to(DEV)
    r2, c2 = bank.gather(idx)
    assert torch.equal(r2, ds.all_rays[idx]) and torch.equal(c2.cpu(), ds.all_rgbs[idx.cpu()])
    assert bank.gather(torch.empty(0, dtype=torch.int64, device=DEV))[0].shape == (0, 6)


def test_gather_equals_materialised_arrays_with_roi(golden, tmp_path):
    """roi = [0.25, 1.0, 0.0, 0.5]: all_rays holds the window's rays (get_rays crops, ray_utils.py:100-110) while all_rgbs - here as in
    the reference, dataset_omniblender.py:75-81 - keeps every pixel of every image; the bank's colours are those of the rays' own
    pixels, i.e. the window's rows of all_rgbs."""
    fx = golden("omniblender")
    ds = OmniBlenderDataset(_build(fx, tmp_path), split="train", near_far=[0.01, 15.0], downsample=250.0, roi=ROI, device=DEV)
    bank = ds.ray_bank()
    assert ds._rays is None and (bank.r0, bank.n_rows, bank.c0, bank.n_cols) == (1, 3, 0, 4) and bank.total == 24
    assert bank.nbytes == 2 * 4 * 8 * 4 + 2 * 48
    rays, rgb = bank.gather(torch.arange(bank.total, device=DEV))
    assert torch.equal(rays, ds.all_rays)
    assert float((rays.cpu() - torch.from_numpy(fx["roi/all_rays"])).abs().max()) <= 1e-6
    assert ds.all_rgbs.shape == (64, 3)
    assert torch.equal(rgb.cpu(), _window(ds.all_rgbs.view(2, 4, 8, 3), bank))
    assert np.array_equal(rgb.cpu().numpy(), _window(torch.from_numpy(fx["train/all_rgbs"]).view(2, 4, 8, 3), bank).numpy())


@pytest.mark.parametrize("roi,channels", [((0, 1, 0, 1), 4), (tuple(ROI), 4), ((0, 1, 0, 1), 3)])
def test_gather_equals_materialised_arrays_on_a_synthetic_bank(roi, channels):
    bank = _synthetic_bank(roi=roi, channels=channels)
    assert bank.nbytes == 16 * 250 * 500 * 4 + 16 * 48
    want_rays = []
    for k in range(bank.K):                                            # OmniBlenderDataset.rays: ego_erp_rays per image, columns cropped
        r = erp_rays(bank.H, bank.W, bank.poses[k].cpu().numpy(), DEV, bank.r0, bank.n_rows, normalize=True)
        want_rays.append(r.view(bank.n_rows, bank.W, 6)[:, bank.c0:bank.c0 + bank.n_cols].reshape(-1, 6))
    want_rays = torch.cat(want_rays, 0)
    want_rgb = _window(_reference_rgb(bank.images), bank)
    rays, rgb = bank.gather(torch.arange(bank.total, device=DEV))
    assert torch.equal(rays, want_rays) and torch.equal(rgb.cpu(), want_rgb)
    if channels == 3:                                                  # A = 255: exactly u8 / 255
        assert torch.equal(rgb.cpu(), _window(bank.images.cpu()[..., :3].float().div(255.0), bank))
    idx = torch.from_numpy(np.random.default_rng(2).integers(0, bank.total, 8192)).to(DEV)
    r2, c2 = bank.gather(idx)
    assert torch.equal(r2, want_rays[idx]) and torch.equal(c2.cpu(), want_rgb[idx.cpu()])


def test_gather_marks_rows_outside_the_contract():
    bank = _synthetic_bank(K=2, H=8, W=16)
    rays, rgb = bank.gather(torch.tensor([0, -1, bank.total, bank.total - 1], device=DEV))
    bad = torch.tensor([False, True, True, False], device=DEV)
    assert torch.equal(torch.isnan(rays).all(1), bad) and torch.equal(torch.isnan(rgb).all(1), bad)
    assert not bool(torch.isnan(rays[~bad]).any())


# ---- the index generator -----------------------------------------------------------------------------------------------------------

def _banks_for_indices(golden, tmp_path):
    fx = golden("omniblender")
    ds = OmniBlenderDataset(_build(fx, tmp_path), split="train", near_far=[0.01, 15.0], downsample=250.0, device=DEV, load_images=False)
    return [(ds.ray_bank(), 12), (_synthetic_bank(), 4096), (_synthetic_bank(K=3, H=40, W=30, roi=ROI), 500)]


def test_simple_indices_equal_the_numpy_restatement(golden, tmp_path):
    for bank, batch in _banks_for_indices(golden, tmp_path):
        s = DeviceSimpleSampler(bank, batch, seed=SEED)
        per_epoch = bank.total // batch
        for c in COUNTERS + (per_epoch - 1, per_epoch, 3 * per_epoch + 1):
            got = s.indices_at(c).cpu().numpy()
            assert np.array_equal(got, ref.simple_indices(bank.total, batch, SEED, c)), (bank.total, batch, c)
        assert int(s.counter) == 0                                     # indices_at is pure


def test_simple_epoch_has_no_duplicate_and_the_next_one_differs():
    bank = _synthetic_bank(K=3, H=40, W=30)                           # 3600 rays, batch 250: 14 batches per epoch, 100 rays dropped
    s = DeviceSimpleSampler(bank, 250, seed=3)
    assert s.batches_per_epoch == 14
    drawn = [s.next_batch() for _ in range(15)]
    assert int(s.counter) == 15
    epoch = torch.cat([d[0] for d in drawn[:14]])
    assert int(epoch.min()) >= 0 and int(epoch.max()) < bank.total and len(torch.unique(epoch)) == 14 * 250
    assert not torch.equal(drawn[14][0], drawn[0][0])
    assert len(torch.unique(torch.cat([drawn[14][0], drawn[0][0]]))) > 250
    for c, (idx, rays, rgb) in enumerate(drawn):                       # next_batch = indices_at(counter) + gather, in one launch
        assert torch.equal(idx, s.indices_at(c))
        r2, c2 = bank.gather(idx)
        assert torch.equal(rays, r2) and torch.equal(rgb, c2)


def test_theta_indices_equal_the_numpy_restatement(golden, tmp_path):
    for bank, batch in _banks_for_indices(golden, tmp_path):
        s = DeviceThetaImportanceSampler(5.0, bank, batch, seed=SEED)
        for c in COUNTERS:
            got = s.indices_at(c).cpu().numpy()
            want = ref.theta_indices(bank.K, bank.n_rows, bank.n_cols, s.cdf_host, batch, SEED, c)
            assert np.array_equal(got, want), (bank.total, batch, c)
            assert got.min() >= 0 and got.max() < bank.total
        idx, rays, rgb = s.next_batch()
        assert torch.equal(idx, s.indices_at(0)) and int(s.counter) == 1
        r2, c2 = bank.gather(idx)
        assert torch.equal(rays, r2) and torch.equal(rgb, c2)


def _chi2_quantile(dof, p_upper=1e-6):
    """The 1 - p_upper quantile of chi-square with `dof` degrees of freedom."""
    try:
        from scipy.stats import chi2
        return float(chi2.isf(p_upper, dof))
    except ImportError:
        z = 4.753424308822899                                          # standard normal quantile of 1 - 1e-6
        assert p_upper == 1e-6
        return dof * (1 - 2 / (9 * dof) + z * (2 / (9 * dof)) ** 0.5) ** 3   # Wilson-Hilferty


def _pearson(counts, p):
    n = counts.sum()
    return float(((counts - n * p) ** 2 / (n * p)).sum())


def test_theta_importance_distribution():
    """2^20 draws, fixed seed (deterministic: a failure is bias, not luck): rows follow cos(lat) * lambda + 1, images and columns are
    uniform - Pearson chi-square of each histogram below the 1 - 1e-6 quantile."""
    bank = _synthetic_bank()
    n = 1 << 20
    s = DeviceThetaImportanceSampler(5.0, bank, n, seed=20221028)
    idx = s.indices_at(0).cpu().numpy()
    img, rem = idx // (bank.n_rows * bank.n_cols), idx % (bank.n_rows * bank.n_cols)
    row, col = rem // bank.n_cols, rem % bank.n_cols
    for name, v, p in (("row", row, s.weight), ("image", img, np.full(bank.K, 1 / bank.K)), ("column", col, np.full(bank.n_cols, 1 / bank.n_cols))):
        counts = np.bincount(v, minlength=len(p)).astype(np.float64)
        assert len(counts) == len(p)
        x2, bound = _pearson(counts, np.asarray(p, np.float64)), _chi2_quantile(len(p) - 1)
        print(f"theta_importance {name}: chi2 = {x2:.1f} ({len(p) - 1} dof), bound {bound:.1f}")
        assert x2 < bound, (name, x2, bound)
    # ... and a uniform row draw would not pass for these weights (the test can see the difference)
    assert _pearson(np.full(bank.n_rows, n / bank.n_rows), s.weight) > 100 * _chi2_quantile(bank.n_rows - 1)


# ---- the feed: batches drawn inside the replayed training graph -------------------------------------------------------------------------

def _same_after_adam(name, a, b, n_steps, lr):
    """tests/test_hip_train_graph.py::_same_after_adam, restated: what that file asks of two runs of the same iterations when the
    table scatters of the shape at hand use float atomics (the small test model's do)."""
    scale = max(float(a.abs().max()), 1e-3)
    err = (a - b).abs()
    assert float(err.mean()) <= 1e-5 * scale, (name, float(err.mean()))
    n_off = int((err > 2e-4 * scale).sum())
    assert n_off <= 8 + 1e-3 * err.numel(), (name, n_off, float(err.max()))
    assert float(err.max()) <= 2.0 * n_steps * lr, (name, float(err.max()))


def _setup(seed, **cfg_kw):
    cfg = synth.SceneConfig(n_voxel=20 ** 3, **cfg_kw)
    model = make_model(cfg, synth.make_weights(cfg, seed=seed), DEV)
    model.train()
    model.update_coarse_sigma_grid()
    return cfg, model


def _train_bank():
    return _synthetic_bank(K=4, H=32, W=64, seed=11)                  # 8192 rays; batch 192: 42 batches per epoch


def _source(kind, bank, batch, seed=77):
    return DeviceSimpleSampler(bank, batch, seed=seed) if kind == "simple" else DeviceThetaImportanceSampler(5.0, bank, batch, seed=seed)


def _graphed(model_seed, noise, factor=0.9, **kw):
    _, m = _setup(model_seed)
    o = FusedAdam(m.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=factor)
    return m, GraphedTrainStep(m, o, render_kwargs=KW, warmup=1, noise_fn=noise, **kw)


@pytest.mark.parametrize("kind,start", [("simple", 0), ("simple", 40), ("theta", 0), ("theta", 7)])
def test_graphed_step_draws_its_batches_inside_the_graph(kind, start):
    N, n = 192, 5
    bank = _train_bank()
    src = _source(kind, bank, N)
    jit = torch.from_numpy(synth.hash_uniform(9, 0, N * 16).reshape(N, 16).astype(np.float32)).to(DEV)
    _, step = _graphed(3, lambda a, b, dev: jit, batch_source=src, start_iteration=start)

    def check(k):
        idx = src.indices_at(k)
        rays, rgb = bank.gather(idx)
        assert torch.equal(step.idx, idx) and torch.equal(step.rays, rays) and torch.equal(step.target, rgb), k

    assert int(src.counter) == start + 1 and step.schedule.iteration() == start + 1
    check(start)                                                       # the warm-up iteration drew what indices_at(start) says
    seen = [step.idx.clone()]
    for _ in range(n):                                                 # start = 40: the replays cross the epoch boundary at 42
        k = int(src.counter)
        loss = step()
        assert bool(torch.isfinite(loss))
        assert int(src.counter) == k + 1
        check(k)
        assert not torch.equal(step.idx, seen[-1])
        seen.append(step.idx.clone())
    assert step.iterations == n + 1 and step.schedule.iteration() == start + n + 1
    with pytest.raises(ValueError, match="batch_source"):
        step(step.rays, step.target)
    with pytest.raises(ValueError, match="batch_source"):
        GraphedTrainStep(step.model, step.opt, step.rays, step.target, KW, batch_source=src)


def test_host_fed_step_still_needs_its_batch():
    N = 64
    rays = torch.from_numpy(synth.make_rays(N, seed=1)).to(DEV)
    _, m = _setup(4)
    o = FusedAdam(m.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True)
    with pytest.raises(ValueError, match="example batch"):
        GraphedTrainStep(m, o, render_kwargs=KW)
    step = GraphedTrainStep(m, o, rays, torch.zeros(N, 3, device=DEV), KW, warmup=1)
    with pytest.raises(ValueError, match="without a batch_source"):
        step()


@pytest.mark.parametrize("kind", ["simple", "theta"])
def test_training_through_the_device_feed_equals_the_host_fed_step(kind):
    """Model A: n replays of step() with the batch drawn in the graph.  Models B, B': host-fed steps given bank.gather(indices_at(k))
    for the same counters, same pinned noise.  If B and B' end bit-equal (gradients bit-reproducible on this shape) A must equal B bit
    for bit; otherwise A vs B is held to what tests/test_hip_train_graph.py asks of two runs of the same iterations."""
    N, n, factor = 192, 5, 0.9
    bank = _train_bank()
    jit = torch.from_numpy(synth.hash_uniform(9, 0, N * 16).reshape(N, 16).astype(np.float32)).to(DEV)
    noise = lambda a, b, dev: jit
    src = _source(kind, bank, N)
    m_a, step_a = _graphed(3, noise, factor, batch_source=src)
    losses_a = [float(step_a()) for _ in range(n)]
    batches = [bank.gather(src.indices_at(k)) for k in range(n + 1)]

    def host_fed():
        m, step = _graphed(3, noise, factor, rays=batches[0][0], target=batches[0][1])
        return m, [float(step(r, t)) for r, t in batches[1:]]

    (m_b, losses_b), (m_b2, _) = host_fed(), host_fed()
    pa, pb, pb2 = (dict(m.named_parameters()) for m in (m_a, m_b, m_b2))
    reproducible = all(torch.equal(pb[k].detach(), pb2[k].detach()) for k in pb)
    print(f"host-fed runs bit-equal: {reproducible}")
    for k in pb:
        if reproducible:
            assert torch.equal(pa[k].detach(), pb[k].detach()), k
        else:
            _same_after_adam(k, pa[k].detach(), pb[k].detach(), n_steps=n + 1, lr=0.02)
    for a, b in zip(losses_a, losses_b):
        assert (a == b) if reproducible else (abs(a - b) <= 2e-5 * max(abs(b), 1e-3)), (losses_a, losses_b)
    fresh = dict(_setup(3)[1].named_parameters())
    assert any(not torch.equal(pa[k].detach(), fresh[k].detach()) for k in pa)   # it did train
