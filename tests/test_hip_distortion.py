"""GPU: the distortion regulariser (ego_ray_distortion, losses.distortion_loss, model.last_train_z): the kernel against the float64
restatement of tests/distortion_ref.py, its gradient through the training render into the density tables, inside a captured
training step against the eager loop, and as the only loss term of a short optimisation."""
import functools

import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth
from egonerf_amd.losses import distortion_loss
from egonerf_amd.optim import FusedAdam
from egonerf_amd.train import GraphedTrainStep
from tests import distortion_ref as ref
from tests.test_hip_train_graph import _same_after_adam, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 37   # not a multiple of the four rays of a block
KW = dict(n_coarse=16, n_fine=16, exp_sampling=True, resampling=True, use_coarse_sample=True)
SPACE_CODE = dict(linear=_lib.DIST_LINEAR, log=_lib.DIST_LOG, disparity=_lib.DIST_DISPARITY)
# About 20 x the worst of float32 arithmetic in the kernel's own order on these inputs (tests/test_distortion_host.py: 6.1e-8 / 4.7e-7):
# the margin is for the device's logf and division and the tree-ordered scans; a wrong carry, a missing 1/3 term or float32 running
# sums are orders of magnitude beyond it.  Measured on an MI355X, worst over the cases below: value 6.9e-8, gradient 3.5e-7.
VALUE_BOUND, GRAD_BOUND = 2e-6, 2e-5


def value_slack(v64, n_rays):
    """What a float32 loss of the kernel's float64 value may be off by: the kernel's bound, the float32 rounding of the result, and the
    kernel's rounding of each ray's term to a multiple of 2^-51 (include/egonerf_hip.h; it matters only for a value near 0)."""
    return (VALUE_BOUND + 2.0 ** -24) * abs(v64) + n_rays * 2.0 ** -52


@functools.lru_cache(maxsize=None)
def case(S, space, trailing):
    """Inputs and the float64 restatement's answer, computed once per case and shared (read-only) by the tests."""
    alpha, z = ref.make_inputs(N, S, trailing_ones=trailing)
    v64, g64 = ref.distortion(alpha, z, space, np.float64)
    for a in (alpha, z, g64):
        a.setflags(write=False)
    return alpha, z, v64, g64


def run_kernel(alpha, z, space, want_value=True, want_grad=True):
    value = torch.zeros(1, dtype=torch.float64, device=DEV) if want_value else None
    g = torch.full_like(alpha, float("nan")) if want_grad else None   # every element must be written
    _lib.check(_lib.load().ego_ray_distortion(alpha.data_ptr(), alpha.shape[1], z.data_ptr(), z.shape[0], z.shape[1], ref.NEAR, ref.FAR,
                                              SPACE_CODE[space], _lib.ptr(value), _lib.ptr(g), _lib.stream_handle()), "ego_ray_distortion")
    return value, g


@pytest.mark.parametrize("trailing", [False, True], ids=["stride=S", "stride=S+1"])
@pytest.mark.parametrize("space", ref.SPACES)
@pytest.mark.parametrize("S", [2, 63, 64, 65, 130, 512])   # one pass, the pass edges, carries, the largest shipped S
def test_kernel_against_the_float64_restatement(S, space, trailing):
    alpha_np, z_np, v64, g64 = case(S, space, trailing)
    alpha, z = torch.from_numpy(alpha_np.copy()).to(DEV), torch.from_numpy(z_np.copy()).to(DEV)
    value, g = run_kernel(alpha, z, space)
    v_only, _ = run_kernel(alpha, z, space, want_grad=False)
    _, g_only = run_kernel(alpha, z, space, want_value=False)
    value2, g2 = run_kernel(alpha, z, space)
    torch.cuda.synchronize()
    got_v, got_g = float(value.item()), g.cpu().numpy().astype(np.float64)
    ev, eg = abs(got_v - v64) / abs(v64), float(np.abs(got_g - g64).max()) / float(np.abs(g64).max())
    print(f"ego_ray_distortion N={N} S={S} {space} stride={alpha.shape[1]}: value {ev:.2e} of |f64|, gradient {eg:.2e} of max |g64|")
    assert not np.isnan(got_g).any()
    assert ev <= VALUE_BOUND, (got_v, v64)
    assert eg <= GRAD_BOUND
    if trailing:
        assert bool((g[:, S:] == 0).all())   # the envmap's ones column: exactly 0
    bits = lambda t: t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)
    assert torch.equal(bits(v_only), bits(value)) and torch.equal(bits(g_only), bits(g))   # value-only / gradient-only = the joint call
    assert torch.equal(bits(g2), bits(g)) and torch.equal(bits(value2), bits(value))        # and a repeat returns the same bits


def test_host_layer_on_the_device():
    alpha_np, z_np, v64, g64 = case(65, "log", True)
    alpha, z = torch.from_numpy(alpha_np.copy()).to(DEV).requires_grad_(True), torch.from_numpy(z_np.copy()).to(DEV)
    loss = distortion_loss(alpha, z, [ref.NEAR, ref.FAR])   # "log" is the default
    assert loss.dtype == torch.float32 and loss.shape == () and abs(loss.item() - v64) <= value_slack(v64, N)
    (loss * 3.0).backward()
    assert float(np.abs(alpha.grad.cpu().numpy().astype(np.float64) / 3.0 - g64).max()) <= GRAD_BOUND * float(np.abs(g64).max())
    assert not distortion_loss(alpha.detach(), z, [ref.NEAR, ref.FAR], space="linear").requires_grad
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distortion_loss(alpha.detach().cpu(), z.cpu(), [ref.NEAR, ref.FAR])
    with pytest.raises(RuntimeError, match="alpha's device"):
        distortion_loss(alpha, z.cpu(), [ref.NEAR, ref.FAR])


def _scene(seed, envmap):
    return _setup(seed, **(dict(use_envmap=True, envmap_res_H=16) if envmap else {}))


def _batch(n, seed):
    rays = torch.from_numpy(synth.make_rays(n, seed=seed)).to(DEV)
    jit = torch.from_numpy(synth.hash_uniform(seed + 1, 0, n * 16).reshape(n, 16).astype(np.float32)).to(DEV)
    return rays, jit


def test_last_train_z_is_the_march_s_own_schedule():
    cfg, model = _scene(6, envmap=False)
    assert model.last_train_z is None
    rays, jit = _batch(64, 21)
    with torch.no_grad():
        model(rays, n_coarse=16, exp_sampling=True)
    assert model.last_train_z is None                      # an eval render does not touch it
    model(rays, is_train=True, n_coarse=16, exp_sampling=True, jitter=torch.zeros_like(jit))
    z = model.last_train_z
    assert z.shape == (64, 16) and z.dtype == torch.float32 and not z.requires_grad
    want = np.float32(cfg.near) + model._sched(16, DEV).cpu().numpy()
    assert np.array_equal(z.cpu().numpy(), np.broadcast_to(want, (64, 16)))   # zero jitter, no resampling: near + schedule
    before = z
    with torch.no_grad():
        model(rays, n_coarse=24, exp_sampling=True)
    assert model.last_train_z is before


@pytest.mark.parametrize("envmap", [False, True], ids=["plain", "envmap"])
def test_gradient_through_the_render_reaches_the_density_tables(envmap):
    """The plumbing into ego_march_backward: backward of the loss = the render's own backward fed with the float64 restatement's
    d loss / d alpha of the same alpha and z (two renders of the same batch: a render's backward runs once)."""
    _, model = _scene(6, envmap)
    rays, jit = _batch(64, 31)
    render = lambda: model(rays, is_train=True, jitter=jit, u=jit, **KW)[4]
    alpha = render()
    z = model.last_train_z
    S = 32
    assert alpha.shape == (64, S + int(envmap)) and z.shape == (64, S) and not z.requires_grad
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    loss = distortion_loss(alpha, z, model.near_far)
    v64, g64 = ref.distortion(alpha.detach().cpu().numpy(), z.cpu().numpy(), "log", np.float64, *model.near_far)
    assert v64 > 0 and abs(loss.item() - v64) <= value_slack(v64, 64)
    model.zero_grad(set_to_none=True)
    loss.backward()
    names, params = zip(*[(k, p) for k, p in model.named_parameters() if p.requires_grad])
    alpha2 = render()
    assert torch.equal(alpha2.detach(), alpha.detach()) and torch.equal(model.last_train_z, z)
    want = torch.autograd.grad(alpha2, params, grad_outputs=torch.from_numpy(g64.astype(np.float32)).to(DEV), allow_unused=True)
    reached = []
    for k, p, w in zip(names, params, want):
        scale = 0.0 if w is None else float(w.abs().max())
        got = torch.zeros_like(p) if p.grad is None else p.grad
        if scale == 0.0:
            assert float(got.abs().max()) == 0.0, k
            continue
        assert float((got - w).abs().max()) <= 2e-4 * scale, k
        reached.append(k)
    assert any(k.startswith("density_") for k in reached), reached
    assert all(k.startswith("density_") for k in reached), reached   # alpha depends on nothing else


def test_graphed_step_with_the_distortion_term():
    """mse + 1e-2 * distortion inside the captured step, last_train_z read inside loss_fn: five iterations with pinned noise against the
    eager loop, at the tolerances tests/test_hip_train_graph.py uses for the entropy term."""
    n, factor, n_it = 128, 0.95, 5
    batches = [(torch.from_numpy(synth.make_rays(n, seed=50 + i)).to(DEV),
                torch.from_numpy(synth.hash_uniform(90 + i, 0, n * 3).reshape(n, 3).astype(np.float32)).to(DEV)) for i in range(n_it)]
    jit = torch.from_numpy(synth.hash_uniform(19, 0, n * 16).reshape(n, 16).astype(np.float32)).to(DEV)
    terms = []

    def loss_of(m):
        def loss_fn(rgb, gt, alpha):
            d = distortion_loss(alpha, m.last_train_z, m.near_far)
            terms.append(d.detach())
            return torch.mean((rgb - gt) ** 2) + 1e-2 * d
        return loss_fn

    _, m_ref = _setup(6)
    loss_ref = loss_of(m_ref)
    o_ref = FusedAdam(m_ref.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    ref_losses = []
    for rays, gt in batches:
        rgb, _d, _bg, _env, alpha = m_ref(rays, is_train=True, jitter=jit, u=jit, **KW)
        loss = loss_ref(rgb, gt, alpha)
        o_ref.zero_grad(set_to_none=True)
        loss.backward()
        o_ref.step()
        for grp in o_ref.param_groups:
            grp["lr"] *= factor
        m_ref.update_coarse_sigma_grid()
        ref_losses.append(float(loss.detach()))
    assert all(float(t) > 0 for t in terms)   # the term is there
    _, m_g = _setup(6)
    o_g = FusedAdam(m_g.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=factor)
    step = GraphedTrainStep(m_g, o_g, batches[0][0], batches[0][1], KW, loss_fn=loss_of(m_g), warmup=1, noise_fn=lambda a, b, dev: jit)
    got = [float(step(rays, gt)) for rays, gt in batches[1:]]
    assert step.iterations == n_it
    for a, b in zip(ref_losses[1:], got):
        assert abs(a - b) <= 5e-5 * max(abs(a), 1e-3), (ref_losses, got)
    pr, pg = dict(m_ref.named_parameters()), dict(m_g.named_parameters())
    for k in pr:
        _same_after_adam(k, pr[k].detach(), pg[k].detach(), n_steps=n_it, lr=0.02)


def test_the_term_alone_falls_under_adam():
    _, model = _scene(6, envmap=False)
    rays, jit = _batch(64, 41)
    opt = FusedAdam(model.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    seen = []
    for _ in range(30):
        alpha = model(rays, is_train=True, jitter=jit, u=jit, **KW)[4]
        loss = distortion_loss(alpha, model.last_train_z, model.near_far)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        model.update_coarse_sigma_grid()
        seen.append(loss.detach())
    seen = [float(t) for t in seen]
    assert seen[0] > 0 and seen[-1] < seen[0], seen
