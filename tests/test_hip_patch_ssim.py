"""GPU: patch batches and the structural term (ego_ray_batch_sample_patches / ego_patch_ssim, sampler.DevicePatchSampler,
data.patch_indices, losses.patch_ssim_loss): the kernel against the float64 definition of tests/patch_ssim_ref.py, what must be exact,
bit-reproducibility across call forms, the term against the whole-image metric, the sampler against the numpy restatement of its rule
(tests/patch_batch_ref.py), an optimisation against float64 torch, and the term inside a captured training step against the eager loop.

The bounds are per case and per quantity: 4 x the float32 restatement's own distance from float64 on the case's inputs, never below
4 x 2^-24 (ref.bound).  Measured on an MI355X, worst over the parity cases: value 6.4e-13 of |v64| (bounds from 2.4e-7), g_rgb 4.8e-8
of max |g64| (bounds from 3.9e-6): the kernel works in float64 and an output is the float64 result rounded once.  Against the metric:
the two float64 restatements are 4.2e-8, 1.1e-8, 6.0e-8 and 1.2e-7 apart on the four image pairs, and 1 - loss and rgb_ssim on the
device are apart by those same amounts (the bound is 4 x each)."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth
from egonerf_amd.data import RayBank, patch_indices
from egonerf_amd.losses import patch_ssim_loss
from egonerf_amd.metrics import rgb_ssim
from egonerf_amd.optim import FusedAdam
from egonerf_amd.sampler import DevicePatchSampler
from egonerf_amd.train import GraphedTrainStep
from tests import patch_batch_ref as bref
from tests import patch_ssim_ref as ref
from tests.test_hip_train_graph import _same_after_adam, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda"
bits = lambda t: t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def run_kernel(d, P, ph, pw, fs, want_value=True, want_grad=True):
    """One ego_patch_ssim call on a dict of device tensors -> (value, g_rgb); the value, the gradient buffer and the workspace start as
    NaN (the value and every gradient element of the patches must be written, the workspace needs no clearing)."""
    lib = _lib.load()
    value = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV) if want_value else None
    g_rgb = torch.full_like(d["rgb"], float("nan")) if want_grad else None
    nbytes = lib.ego_patch_ssim_workspace_bytes(P, ph, pw)
    assert nbytes == 16 * P
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(lib.ego_patch_ssim(d["rgb"].data_ptr(), d["target"].data_ptr(), _lib.ptr(d["weight"]), P, ph, pw, fs, 1.5, 1.0, 0.01, 0.03,
                                  ws.data_ptr(), _lib.ptr(value), _lib.ptr(g_rgb), _lib.stream_handle()), "ego_patch_ssim")
    return value, g_rgb


WORST = dict(value=0.0, g_rgb=0.0)
SHAPES = [(3, 3, 3), (7, 7, 7), (4, 6, 1), (5, 7, 5), (8, 8, 5), (8, 8, 7), (9, 9, 7), (16, 16, 11), (32, 32, 15), (32, 5, 5)]


@pytest.mark.parametrize("ph,pw,fs", SHAPES)
def test_kernel_against_the_float64_definition(ph, pw, fs):
    """Value and g_rgb within the rule's bound of float64 autograd at every patch count, with and without weights, no pixel excused;
    pixels under no valid window exactly 0, the rows behind the patches untouched; all call forms and a repeat return the same bits."""
    for P in ((1, 3) if (ph, pw) == (32, 32) else (1, 2, 65, 257)):
        for with_weight in (False, True):
            c = ref.make_inputs(P, ph, pw, fs, with_weight=with_weight)
            d = {k: dev(v) for k, v in c.items()}
            n = P * ph * pw
            tag = f"{ph}x{pw} fs={fs} P={P} weight={with_weight}"
            _, wv = ref.window_valid(c["target"], c["weight"], P, ph, pw, fs)
            assert wv.any() and (P < 2 or not wv[1].any()), tag                         # at least one whole patch is invalid
            assert P < 2 or ph * pw == fs * fs or (~wv[0]).any(), tag                   # ... and some windows of a valid patch
            v64, g64 = ref.autograd_direct(c["rgb"], c["target"], (ph, pw), P, c["weight"], fs)
            v32, g32 = ref.kernel_model(c["rgb"], c["target"], (ph, pw), P, c["weight"], fs, dtype=np.float32)
            value, g_rgb = run_kernel(d, P, ph, pw, fs)
            v_only, _ = run_kernel(d, P, ph, pw, fs, want_grad=False)
            _, g_only = run_kernel(d, P, ph, pw, fs, want_value=False)
            value2, g_rgb2 = run_kernel(d, P, ph, pw, fs)
            got_v, got_g = float(value.item()), g_rgb[:n].cpu().numpy().astype(np.float64)
            assert np.isfinite(got_v) and np.isfinite(got_g).all(), tag
            ev, bv = abs(got_v - v64) / v64, 4.0 * max(abs(v32 - v64) / v64, ref.FLOAT32_HALF_ULP)
            bg, sg = ref.bound(g32, g64)
            eg = float(np.abs(got_g - g64[:n]).max()) / sg
            print(f"ego_patch_ssim {tag}: value {ev:.2e} of |v64| (bound {bv:.2e}), g_rgb {eg:.2e} of max |g64| (bound {bg:.2e})")
            assert v64 > 0 and ev <= bv, (tag, got_v, v64)
            assert sg > 0 and eg <= bg, (tag, eg, bg)
            unc = ~ref.covered(wv, ph, pw, fs).reshape(-1)
            assert (P < 2 or unc.sum() >= ph * pw) and bool((g_rgb[:n][dev(unc)] == 0).all()), tag       # under no valid window: exactly 0
            assert bool(torch.isnan(g_rgb[n:]).all()), tag                               # the rows behind the patches are not touched
            WORST.update(value=max(WORST["value"], ev), g_rgb=max(WORST["g_rgb"], eg))
            assert torch.equal(bits(v_only), bits(value)) and torch.equal(bits(g_only), bits(g_rgb)), tag
            assert torch.equal(bits(value2), bits(value)) and torch.equal(bits(g_rgb2), bits(g_rgb)), tag
    print(f"worst so far: value {WORST['value']:.2e} of |v64|, g_rgb {WORST['g_rgb']:.2e} of max |g64|")


@pytest.mark.parametrize("with_weight", [False, True])
def test_a_batch_without_a_valid_window(with_weight):
    P, ph, pw, fs = 65, 8, 8, 7
    c = ref.make_inputs(P, ph, pw, fs, with_weight=with_weight, invalid=False)
    if with_weight:
        c["weight"][3::16] = 0.0                    # a pixel of every window
        c["weight"][3], c["weight"][19] = np.nan, -1.0
    else:
        c["target"][3::16, 1] = np.nan
    assert not ref.window_valid(c["target"], c["weight"], P, ph, pw, fs)[1].any()
    value, g_rgb = run_kernel({k: dev(v) for k, v in c.items()}, P, ph, pw, fs)
    assert float(value.item()) == 0.0 and bool((g_rgb[:P * ph * pw] == 0).all())       # M = 0: exactly 0, no NaN


def test_a_non_finite_colour_under_a_valid_window_is_not_hidden():
    P, ph, pw, fs = 2, 8, 8, 7
    c = ref.make_inputs(P, ph, pw, fs, with_weight=False, invalid=False, tail=0)
    c["rgb"][64 + 9, 2] = np.nan
    value, g_rgb = run_kernel({k: dev(v) for k, v in c.items()}, P, ph, pw, fs)
    assert np.isnan(float(value.item())) and bool(torch.isnan(g_rgb[64:, 2]).any())
    assert bool(torch.isfinite(g_rgb[:64]).all()) and bool(torch.isfinite(g_rgb[64:, :2]).all())     # the other patch and channels are not touched by it


def test_host_layer_on_the_device():
    P, ph, pw, fs = 5, 8, 8, 7
    c = ref.make_inputs(P, ph, pw, fs, with_weight=True, tail=11)
    d = {k: dev(v) for k, v in c.items()}
    v64, g64 = ref.autograd_direct(c["rgb"], c["target"], (ph, pw), P, c["weight"], fs)
    rgb = d["rgb"].clone().requires_grad_(True)
    tgt, w = d["target"].clone().requires_grad_(True), d["weight"].clone().requires_grad_(True)
    loss = patch_ssim_loss(rgb, tgt, (ph, pw), n_patches=P, weight=w)
    assert loss.dtype == torch.float64 and loss.shape == () and abs(loss.item() - v64) <= 1e-12
    (loss * 3.0).backward()
    n = P * ph * pw
    assert rgb.grad.dtype == torch.float32 and bool((rgb.grad[n:] == 0).all())          # the ignored rows (one holds a NaN colour): exactly 0
    assert float(np.abs(rgb.grad.cpu().numpy() / 3.0 - g64).max()) <= 4 * 2.0 ** -23 * np.abs(g64).max()
    assert tgt.grad is None and w.grad is None
    plain = patch_ssim_loss(d["rgb"][:n], d["target"][:n], (ph, pw))                    # n_patches defaults to all of B
    assert not plain.requires_grad and abs(plain.item() - ref.autograd_direct(c["rgb"][:n], c["target"][:n], (ph, pw), P, None, fs)[0]) <= 1e-12
    assert float(patch_ssim_loss(d["rgb"], d["target"], (ph, pw), n_patches=0)) == 0.0
    with pytest.raises(RuntimeError, match="rgb's device"):
        patch_ssim_loss(d["rgb"], d["target"].cpu(), (ph, pw), n_patches=P)
    lib = _lib.load()
    ws = torch.empty(16, dtype=torch.float64, device=DEV)
    args = lambda **k: (d["rgb"].data_ptr(), d["target"].data_ptr(), None, k.get("P", 1), k.get("ph", 8), k.get("pw", 8), k.get("fs", 7), 1.5, 1.0,
                        0.01, 0.03, k.get("ws", ws.data_ptr()), k.get("value", ws.data_ptr()), None, None)
    for k, msg in [(dict(fs=16, ph=16, pw=16), "filter_size must be 1..15"), (dict(ph=6), "must cover the filter"), (dict(pw=33), "at most 32 x 32"),
                   (dict(P=-1), "P < 0"), (dict(value=None), "no output asked for"), (dict(ws=None), "workspace")]:
        assert lib.ego_patch_ssim(*args(**k)) != 0 and msg in lib.ego_last_error().decode(), k
    assert lib.ego_patch_ssim_workspace_bytes(3, 33, 8) == -1 and lib.ego_patch_ssim_workspace_bytes(0, 8, 8) == 0


def test_against_the_metric():
    """One 16 x 16 patch, fs = 11, random textured images, no weight: 1 - loss against metrics.rgb_ssim within 4 x the distance between
    the float64 restatements with and without the metric's float32 squares and clamps."""
    ph = pw = 16
    worst = 0.0
    for seed in range(4):
        c = ref.make_inputs(1, ph, pw, 11, with_weight=False, invalid=False, tail=0, seed=seed)
        plain, _ = ref.kernel_model(c["rgb"], c["target"], (ph, pw), 1, None, 11)
        guarded, _ = ref.kernel_model(c["rgb"], c["target"], (ph, pw), 1, None, 11, metric_guards=True)
        dist = abs(plain - guarded)
        loss = float(patch_ssim_loss(dev(c["rgb"]), dev(c["target"]), (ph, pw), filter_size=11))
        metric = rgb_ssim(dev(c["rgb"]).view(ph, pw, 3), dev(c["target"]).view(ph, pw, 3), 1.0)
        print(f"seed {seed}: 1 - loss {1 - loss:.12f}, rgb_ssim {metric:.12f}, apart {abs(1 - loss - metric):.2e}; the restatements {dist:.2e}")
        assert dist > 0 and abs((1.0 - loss) - metric) <= 4.0 * dist
        worst = max(worst, dist)
    print(f"largest distance between the restatements: {worst:.2e}")


# ---- the sampler ----
def _bank(roi=(0, 1, 0, 1), K=3, H=16, W=32, seed=5, masks=False):
    g = np.random.default_rng(seed)
    q, _ = np.linalg.qr(g.standard_normal((K, 3, 3)))
    poses = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
    poses[:, :3, :3] = q
    poses[:, :3, 3] = g.uniform(-0.25, 0.25, (K, 3))
    m = None
    if masks:
        m = np.full((K, H, W), 255, np.uint8)
        m[:, 13:16, 6:14] = 0
        m[:, 12, 6:14] = 128
    return RayBank(poses, g.integers(0, 256, (K, H, W, 3), dtype=np.uint8), (W, H), roi=roi, device=DEV, masks=m)


@pytest.mark.parametrize("roi", [(0, 1, 0, 1), (0.25, 1, 0.25, 0.75)])
@pytest.mark.parametrize("patch,stride", [((4, 4), 1), ((3, 5), 2), ((4, 4), 2), ((3, 5), 1)])
@pytest.mark.parametrize("n_random", [0, 37])
def test_sampler_against_the_numpy_restatement(roi, patch, stride, n_random):
    bank = _bank(roi)
    wrap = bref.wraps(bank.c0, bank.n_cols, bank.W)
    P, seed = 70, 20221028 + (1 << 40)
    src = DevicePatchSampler(bank, patches=P, patch=patch, stride=stride, n_random=n_random, seed=seed)
    assert src.n_patch_rays == P * patch[0] * patch[1] and src.batch == src.n_patch_rays + n_random
    want = lambda c: bref.patch_batch_indices(bank.K, bank.n_rows, bank.n_cols, wrap, P, patch, stride, n_random, seed, c)
    for c in (0, 1, 2, 1000, 2 ** 33 + 5):
        assert np.array_equal(src.indices_at(c).cpu().numpy(), want(c)), c
    assert int(src.counter) == 0                                                     # indices_at is pure
    assert not np.array_equal(want(0), want(1))
    img, row0, col0 = bref.patch_origins(bank.K, bank.n_rows, bank.n_cols, wrap, P, patch, stride, seed, 2)
    assert torch.equal(src.indices_at(2)[:src.n_patch_rays], patch_indices(bank, dev(img), dev(row0), dev(col0), patch, stride))
    idx = torch.full((src.batch,), -1, dtype=torch.int64, device=DEV)
    rays, rgb = torch.full((src.batch, 6), float("nan"), device=DEV), torch.full((src.batch, 3), float("nan"), device=DEV)
    src.seek(7)
    src.sample_into(idx, rays, rgb)
    assert np.array_equal(idx.cpu().numpy(), want(7)) and int(src.counter) == 7      # sample_into does not advance
    r2, c2 = bank.gather(idx)
    assert torch.equal(bits(rays), bits(r2)) and torch.equal(bits(rgb), bits(c2))
    i1, rays1, rgb1 = src.next_batch()
    i2, _, _ = src.next_batch()
    assert int(src.counter) == 9 and torch.equal(i1, idx) and torch.equal(bits(rays1), bits(rays)) and torch.equal(bits(rgb1), bits(rgb))
    assert np.array_equal(i2.cpu().numpy(), want(8)) and not torch.equal(i1, i2)
    src.seek(7)
    assert torch.equal(src.next_batch()[0], i1)                                      # the same counter: the same batch
    lib, e = _lib.load(), torch.empty(4, dtype=torch.int64, device=DEV)
    import ctypes as C
    call = lambda P_=1, ph=2, pw=2, st=1, nr=0, ctr=e.data_ptr(), ix=e.data_ptr(): lib.ego_ray_batch_sample_patches(
        C.byref(bank.struct), 0, ctr, P_, ph, pw, st, nr, ix, None, None, None)
    for kw, msg in [(dict(P_=-1), "P < 0 or n_random < 0"), (dict(nr=-1), "P < 0 or n_random < 0"), (dict(ph=0), "must be >= 1"),
                    (dict(st=0), "must be >= 1"), (dict(ph=17), "does not"), (dict(pw=17, st=2), "does not"), (dict(ctr=None), "null counter or idx"),
                    (dict(ix=None), "null counter or idx")]:
        assert call(**kw) != 0 and msg in lib.ego_last_error().decode(), kw
    assert call(P_=0, nr=0, ctr=None, ix=None) == 0                                  # B == 0: a no-op


# ---- optimisation ----
def test_adam_on_a_free_batch_follows_the_float64_loop():
    """A free [B, 3] tensor driven towards a target by patch_ssim_loss under torch Adam for 30 steps.  Step by step, the loss and the
    gradient the device loop sees are within the rule's bound of the float64 definition at the loop's own parameters; the same loop run
    in float64 (autograd through the definition, torch's Adam) from the same start ends at the same parameters, compared the way the
    graph tests compare parameters after Adam steps (Adam's normalisation lets single elements whose gradient nearly vanishes part ways);
    the loss falls in both."""
    P, ph, pw, fs, STEPS, LR = 6, 8, 8, 7, 30, 0.01
    c = ref.make_inputs(P, ph, pw, fs, with_weight=True, tail=9)
    start = np.nan_to_num(c["rgb"], nan=0.5)
    n = P * ph * pw
    tgt, w = dev(c["target"]), dev(c["weight"])
    x = dev(start).clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=LR)
    x64 = torch.from_numpy(start.astype(np.float64)).requires_grad_(True)
    opt64 = torch.optim.Adam([x64], lr=LR)
    losses, losses64 = [], []
    for k in range(STEPS):
        here = x.detach().cpu().numpy()
        loss = patch_ssim_loss(x, tgt, (ph, pw), n_patches=P, weight=w)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        v64, g64 = ref.autograd_direct(here, c["target"], (ph, pw), P, c["weight"], fs)
        v32, g32 = ref.kernel_model(here, c["target"], (ph, pw), P, c["weight"], fs, dtype=np.float32)
        bg, sg = ref.bound(g32, g64)
        assert abs(float(loss.detach()) - v64) <= 4.0 * max(abs(v32 - v64), ref.FLOAT32_HALF_ULP * v64), (k, float(loss.detach()), v64)
        assert float(np.abs(x.grad.cpu().numpy() - g64).max()) <= bg * sg, k
        opt.step()
        v, g = ref.autograd_direct(x64.detach().numpy(), c["target"], (ph, pw), P, c["weight"], fs)
        x64.grad = torch.from_numpy(g)
        opt64.step()
        losses.append(float(loss.detach()))
        losses64.append(v)
    print(f"patch_ssim_loss under Adam, {STEPS} steps: {losses[0]:.4f} -> {losses[-1]:.4f} (float64 loop: {losses64[0]:.4f} -> {losses64[-1]:.4f})")
    assert losses[-1] < 0.8 * losses[0] and losses64[-1] < 0.8 * losses64[0]
    _same_after_adam("x", x64.detach().float(), x.detach().cpu(), n_steps=STEPS, lr=LR)
    assert torch.equal(bits(x.detach()[n:]), bits(dev(start)[n:]))                     # the ignored rows never moved


# ---- the captured step ----
KW = dict(n_coarse=8, n_fine=8, exp_sampling=True, resampling=True, use_coarse_sample=True)
N_IT, FACTOR, LAM, PATCHES, N_RANDOM = 4, 0.95, 0.2, 3, 16


def _loss_fn(masked):
    if masked:
        def loss_fn(rgb, tgt, alpha, weight):
            from egonerf_amd.losses import photometric_loss
            return (1 - LAM) * photometric_loss(rgb, tgt, weight=weight) + LAM * patch_ssim_loss(rgb, tgt, (8, 8), n_patches=PATCHES, weight=weight)
        return loss_fn
    return lambda rgb, tgt, alpha: (1 - LAM) * torch.mean((rgb - tgt) ** 2) + LAM * patch_ssim_loss(rgb, tgt, (8, 8), n_patches=PATCHES)


@pytest.mark.parametrize("masked", [False, True])
def test_graphed_step_with_patch_batches_equals_the_eager_loop(masked):
    """GraphedTrainStep(batch_source=DevicePatchSampler) with MSE + SSIM (with a masked bank: both terms gated by the bank's masks, filled by
    name): the parameters after 3 replays against the eager loop that draws indices_at(k) and calls the same functions, at the
    tolerances of tests/test_hip_train_graph.py."""
    bank = _bank(masks=masked, seed=9)
    B = PATCHES * 64 + N_RANDOM
    jit = torch.from_numpy(synth.hash_uniform(19, 0, B * 8).reshape(B, 8).astype(np.float32)).to(DEV)
    loss_fn = _loss_fn(masked)
    src = DevicePatchSampler(bank, patches=PATCHES, patch=(8, 8), n_random=N_RANDOM, seed=31)
    assert src.batch == B
    _, m_ref = _setup(6)
    o_ref = FusedAdam(m_ref.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    ref_losses, ssim_terms, zero_weights = [], [], 0
    for k in range(N_IT):
        idx = src.indices_at(k)
        rays, gt = bank.gather(idx)
        rgb, _d, _bg, _env, alpha = m_ref(rays, is_train=True, jitter=jit, u=jit, **KW)
        extra = dict(weight=bank.gather_mask(idx)) if masked else {}
        zero_weights += int((extra["weight"] == 0).sum()) if masked else 0
        loss = loss_fn(rgb, gt, alpha, **extra)
        ssim_terms.append(float(patch_ssim_loss(rgb.detach(), gt, (8, 8), n_patches=PATCHES, **extra)))
        o_ref.zero_grad(set_to_none=True)
        loss.backward()
        o_ref.step()
        for grp in o_ref.param_groups:
            grp["lr"] *= FACTOR
        m_ref.update_coarse_sigma_grid()
        ref_losses.append(float(loss.detach()))
    assert (zero_weights > 0) == masked
    assert all(0.0 < s < 2.0 for s in ssim_terms)                                     # the term takes part: some window of every batch is valid
    _, m_g = _setup(6)
    o_g = FusedAdam(m_g.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=FACTOR)
    step = GraphedTrainStep(m_g, o_g, render_kwargs=KW, loss_fn=loss_fn, warmup=1, noise_fn=lambda a, b, d: jit, batch_source=src)
    assert (step.weight is not None) == masked
    got = []
    for k in range(1, N_IT):
        got.append(float(step()))
        assert torch.equal(step.idx, src.indices_at(k))
    assert step.iterations == N_IT and int(src.counter) == N_IT
    for a, b in zip(ref_losses[1:], got):
        assert abs(a - b) <= 5e-5 * max(abs(a), 1e-3), (ref_losses, got)
    pg = dict(m_g.named_parameters())
    for k, p in m_ref.named_parameters():
        _same_after_adam(k, p.detach(), pg[k].detach(), n_steps=N_IT, lr=0.02)
