"""GPU: depth supervision (ego_ray_depth_loss, losses.depth_loss / expected_depth, RayBank(depths=...), GraphedTrainStep's depth
targets, TrainSchedule.stepped): the kernel against the float64 definition of tests/depth_loss_ref.py, its prediction against the
render's own depth_map, its gradient through the training render into the density tables, the bank's depth gather, the term inside a
captured training step against the eager loop, and as the only loss term of a short optimisation."""
import functools

import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth
from egonerf_amd.data import RayBank
from egonerf_amd.losses import depth_loss, expected_depth
from egonerf_amd.optim import FusedAdam
from egonerf_amd.sampler import DeviceSimpleSampler
from egonerf_amd.train import GraphedTrainStep
from tests import depth_loss_ref as ref
from tests.helpers import make_oracle
from tests.test_hip_train_graph import _same_after_adam, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda"
KW = dict(n_coarse=16, n_fine=16, exp_sampling=True, resampling=True, use_coarse_sample=True)
SPACE_CODE = dict(metric=_lib.DIST_METRIC, log=_lib.DIST_LOG, disparity=_lib.DIST_DISPARITY)
KIND_CODE = dict(l2=_lib.DEPTH_L2, l1=_lib.DEPTH_L1)
# The bounds are per case: 4 x the float32 model's own distance from float64 on the case's inputs (ref.case; the distances are printed by
# tests/test_depth_loss_host.py, worst 1.1e-7 / 1.0e-6 / 2.9e-7 for value / gradient / pred), never below 4 x 2^-24.
# Measured on an MI355X, worst over the cases below: value 3.1e-8 of |v64|, gradient 6.6e-7 of max |g64| (S = 130, "log"; its bound is
# 4.1e-6), pred 4.6e-7 of max |D64| (S = 512; bound 8.2e-7); the render's depth_map 1.6e-7 and expected_depth 1.3e-7 (bound 6.0e-7).
bits = lambda t: t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def run_kernel(alpha, z, target, tail, space="metric", kind="l2", want_value=True, want_grad=True, want_pred=True):
    """One ego_ray_depth_loss call on device tensors -> (value, g_alpha, pred); the gradient buffer starts as NaN (every element must be
    written) and so does the workspace (it needs no clearing)."""
    lib = _lib.load()
    N, S = z.shape
    value = torch.zeros(1, dtype=torch.float64, device=DEV) if want_value else None
    g = torch.full_like(alpha, float("nan")) if want_grad else None
    pred = torch.full((N,), float("nan"), device=DEV) if want_pred else None
    ws = torch.full((lib.ego_ray_depth_loss_workspace_bytes(N) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(lib.ego_ray_depth_loss(alpha.data_ptr(), alpha.shape[1], z.data_ptr(), _lib.ptr(target), _lib.ptr(tail), N, S, ref.NEAR, ref.FAR,
                                      SPACE_CODE[space], KIND_CODE[kind], ws.data_ptr(), _lib.ptr(value), _lib.ptr(g), _lib.ptr(pred),
                                      _lib.stream_handle()), "ego_ray_depth_loss")
    return value, g, pred


@pytest.mark.parametrize("case_id", ref.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_kernel_against_the_float64_definition(case_id):
    S, trailing, space, kind, _ = case_id
    c = ref.case(*case_id)
    alpha, z, target, tail = dev(c.alpha), dev(c.z), dev(c.target), dev(c.tail)
    value, g, pred = run_kernel(alpha, z, target, tail, space, kind)
    v_only, _, _ = run_kernel(alpha, z, target, tail, space, kind, want_grad=False, want_pred=False)
    _, g_only, _ = run_kernel(alpha, z, target, tail, space, kind, want_value=False, want_pred=False)
    value2, g2, pred2 = run_kernel(alpha, z, target, tail, space, kind)
    _, _, p_only = run_kernel(alpha, z, None, tail, space, kind, want_value=False, want_grad=False)
    torch.cuda.synchronize()
    got_v, got_g, got_p = float(value.item()), g.cpu().numpy().astype(np.float64), pred.cpu().numpy().astype(np.float64)
    ev, eg, ep = abs(got_v - c.v64) / abs(c.v64), float(np.abs(got_g - c.g64).max()) / c.g_scale, float(np.abs(got_p - c.D64).max()) / c.D_scale
    print(f"ego_ray_depth_loss N={ref.N} S={S} stride={alpha.shape[1]} {space} {kind} tail={c.tail is not None}: value {ev:.2e} of |f64| "
          f"(bound {c.value_bound:.2e}), gradient {eg:.2e} of max |g64| ({c.grad_bound:.2e}), pred {ep:.2e} of max |D64| ({c.pred_bound:.2e})")
    assert not np.isnan(got_g).any() and not np.isnan(got_p).any() and not np.isnan(got_v)
    assert ev <= c.value_bound, (got_v, c.v64)
    assert eg <= c.grad_bound
    assert ep <= c.pred_bound
    if trailing:
        assert bool((g[:, S:] == 0).all())   # the envmap's ones column: exactly 0
    invalid = torch.from_numpy(~ref.valid_mask(c.target)).to(DEV)
    assert int(invalid.sum()) >= 14 and bool((g[invalid] == 0).all())   # target 0, NaN, inf, negative: exactly 0
    assert bool((g[ref.EXACT_ROW] == 0).all())                              # D = target: r = 0
    assert torch.equal(bits(v_only), bits(value)) and torch.equal(bits(g_only), bits(g))   # value-only / gradient-only = the joint call
    assert torch.equal(bits(g2), bits(g)) and torch.equal(bits(value2), bits(value))        # and a repeat returns the same bits
    assert torch.equal(bits(pred2), bits(pred)) and torch.equal(bits(p_only), bits(pred))   # pred needs no target


@pytest.mark.parametrize("kind", ref.KINDS)
def test_a_batch_without_a_valid_ray(kind):
    c = ref.case(65, True)
    target = np.array(c.target)
    target[ref.valid_mask(target)] = 0.0
    target[1], target[2] = -np.inf, -0.0
    value, g, pred = run_kernel(dev(c.alpha), dev(c.z), dev(target), dev(c.tail), kind=kind)
    assert float(value.item()) == 0.0 and bool((g == 0).all())      # V = 0: exactly 0, no NaN
    assert float(np.abs(pred.cpu().numpy().astype(np.float64) - c.D64).max()) <= c.pred_bound * c.D_scale   # pred is D whatever the targets


@pytest.mark.parametrize("S", [2, 130])
def test_a_single_ray(S):
    c = ref.case(S, True, "metric", "l2", True, 1)
    assert c.alpha.shape == (1, S + 1) and c.v64 > 0
    value, g, pred = run_kernel(dev(c.alpha), dev(c.z), dev(c.target), dev(c.tail))
    assert abs(float(value.item()) - c.v64) <= c.value_bound * c.v64
    assert float(np.abs(g.cpu().numpy().astype(np.float64) - c.g64).max()) <= c.grad_bound * c.g_scale
    assert abs(float(pred.item()) - c.D64[0]) <= c.pred_bound * c.D_scale


def test_host_layer_on_the_device():
    c = ref.case(65, True, "log", "l2", True)
    alpha, z, target, tail = dev(c.alpha).requires_grad_(True), dev(c.z), dev(c.target), dev(c.tail)
    loss = depth_loss(alpha, z, target, tail, space="log", near_far=[ref.NEAR, ref.FAR])
    assert loss.dtype == torch.float32 and loss.shape == () and abs(loss.item() - c.v64) <= (c.value_bound + 2.0 ** -24) * c.v64
    (loss * 3.0).backward()
    assert float(np.abs(alpha.grad.cpu().numpy().astype(np.float64) / 3.0 - c.g64).max()) <= c.grad_bound * c.g_scale
    assert not z.requires_grad and target.grad is None and tail.grad is None
    m = ref.case(65, True)   # "metric", "l2" are the defaults
    a = dev(m.alpha)
    plain = depth_loss(a, dev(m.z), dev(m.target), dev(m.tail))
    assert not plain.requires_grad and abs(plain.item() - m.v64) <= (m.value_bound + 2.0 ** -24) * m.v64
    # inputs that ask for a gradient get none: alpha is the only differentiable one
    zg, tg = dev(m.z).requires_grad_(True), dev(m.target).requires_grad_(True)
    a2 = dev(m.alpha).requires_grad_(True)
    depth_loss(a2, zg, tg, dev(m.tail), kind="l1").backward()
    assert a2.grad is not None and zg.grad is None and tg.grad is None
    pred = expected_depth(a, dev(m.z), tail=dev(m.tail))
    assert pred.shape == (ref.N,) and pred.dtype == torch.float32 and not pred.requires_grad
    assert float(np.abs(pred.cpu().numpy().astype(np.float64) - m.D64).max()) <= m.pred_bound * m.D_scale
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        depth_loss(a.cpu(), dev(m.z).cpu(), dev(m.target).cpu())
    with pytest.raises(RuntimeError, match="alpha's device"):
        depth_loss(a, dev(m.z).cpu(), dev(m.target))
    with pytest.raises(RuntimeError, match="alpha's device"):
        depth_loss(a, dev(m.z), dev(m.target).cpu())
    with pytest.raises(ValueError, match="near_far"):
        depth_loss(a, dev(m.z), dev(m.target), space="disparity")


def _scene(seed, envmap):
    return _setup(seed, **(dict(use_envmap=True, envmap_res_H=16) if envmap else {}))


def _batch(n, seed):
    rays = torch.from_numpy(synth.make_rays(n, seed=seed)).to(DEV)
    jit = torch.from_numpy(synth.hash_uniform(seed + 1, 0, n * 16).reshape(n, 16).astype(np.float32)).to(DEV)
    return rays, jit


def _targets(n, near_far, seed):
    """[n] float32 in [near, far], every fourth exactly 0"""
    t = (near_far[0] + (near_far[1] - near_far[0]) * synth.hash_uniform(seed, 0, n)).astype(np.float32)
    t[::4] = 0.0
    return t


@pytest.mark.parametrize("envmap", [False, True], ids=["plain", "envmap"])
def test_expected_depth_is_the_render_s_depth_map(envmap):
    """expected_depth with tail = rays[:, 5] restates the render's depth_map (EgoNeRF.py:597: sum w z + (1 - acc) rays[..., -1]); both
    within the pred bound (4 x the float32 model's distance on this alpha and z) of the float64 value.  The render's own output is as
    non-differentiable as it was."""
    _, model = _scene(6, envmap)
    rays, jit = _batch(64, 31)
    _rgb, depth_map, _bg, _env, alpha = model(rays, is_train=True, jitter=jit, u=jit, **KW)
    z = model.last_train_z
    assert not depth_map.requires_grad and alpha.requires_grad and alpha.shape == (64, 32 + int(envmap))
    pred = expected_depth(alpha, z, tail=rays[:, 5])
    assert not pred.requires_grad
    a_np, z_np, tail_np = alpha.detach().cpu().numpy(), z.cpu().numpy(), rays[:, 5].cpu().numpy()
    none = np.zeros(64, np.float32)
    _, D64 = ref.direct(a_np, z_np, none, tail_np)
    _, _, D32 = ref.kernel_model(a_np, z_np, none, tail_np, dtype=np.float32)
    scale = float(np.abs(D64).max())
    bound = 4.0 * max(float(np.abs(D32.astype(np.float32).astype(np.float64) - D64).max()) / scale, ref.FLOAT32_HALF_ULP)
    e_pred = float(np.abs(pred.cpu().numpy().astype(np.float64) - D64).max()) / scale
    e_map = float(np.abs(depth_map.cpu().numpy().astype(np.float64) - D64).max()) / scale
    print(f"envmap={envmap}: expected_depth {e_pred:.2e}, the render's depth_map {e_map:.2e} of max |D64| (bound {bound:.2e})")
    assert scale > 0.1 and e_pred <= bound and e_map <= bound


@pytest.mark.parametrize("envmap", [False, True], ids=["plain", "envmap"])
def test_gradient_through_the_render_reaches_the_density_tables(envmap):
    """The plumbing into ego_march_backward: backward of the loss = the render's own backward fed with the float64 definition's
    d loss / d alpha of the same alpha and z (two renders of the same batch: a render's backward runs once)."""
    _, model = _scene(6, envmap)
    rays, jit = _batch(64, 31)
    render = lambda: model(rays, is_train=True, jitter=jit, u=jit, **KW)[4]
    alpha = render()
    z = model.last_train_z
    S = 32
    assert alpha.shape == (64, S + int(envmap)) and z.shape == (64, S) and not z.requires_grad
    target = _targets(64, model.near_far, 5)
    loss = depth_loss(alpha, z, dev(target), tail=rays[:, 5])
    v64, g64, _ = ref.autograd_direct(alpha.detach().cpu().numpy(), z.cpu().numpy(), target, rays[:, 5].cpu().numpy())
    # the kernel's accuracy is pinned above; here the float32 loss only has to be the float64 value of THIS alpha, z and target
    assert v64 > 0 and abs(loss.item() - v64) <= 1e-5 * v64
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


# ---- the bank's depth targets ----
K, H, W, ROI = 2, 6, 8, (0.25, 0.75, 0.25, 1)   # window: rows [1, 4), columns [2, 8)


def _depth_bank(dtype, K=K, H=H, W=W, roi=ROI, seed=3):
    g = np.random.default_rng(seed)
    poses = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))
    poses[:, :3, 3] = g.uniform(-0.2, 0.2, (K, 3))
    depths = g.uniform(0.5, 9.0, (K, H, W)).astype(dtype)
    depths[g.uniform(size=depths.shape) < 0.3] = 0
    return RayBank(poses, g.integers(0, 256, (K, H, W, 3), dtype=np.uint8), (W, H), roi=roi, device=DEV, depths=depths), depths


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["float32", "float16"])
def test_bank_gathers_the_depth_of_each_ray_s_pixel(dtype):
    bank, depths = _depth_bank(dtype)
    assert (bank.r0, bank.n_rows, bank.c0, bank.n_cols) == (1, 3, 2, 6) and bank.total == 36
    assert bank.depths.dtype == (torch.float16 if dtype == np.float16 else torch.float32)
    assert bank.nbytes == K * H * W * 4 + K * 48 + depths.nbytes
    idx = torch.arange(bank.total - 1, -1, -1, device=DEV)
    window = depths[:, 1:4, 2:8].astype(np.float32).reshape(-1)     # the materialised array, in the index space of all_rays
    got = bank.gather_depth(idx)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.int32), window[::-1].view(np.int32))
    assert float(got.min()) == 0.0 and float(got.max()) > 1.0
    out = bank.gather_depth(torch.tensor([0, -1, bank.total, 35, 2 ** 40], device=DEV))
    assert np.array_equal(np.isnan(out.cpu().numpy()), [False, True, True, False, True])   # outside the bank: NaN, nothing read
    assert float(out[0]) == window[0] and float(out[3]) == window[35]
    with pytest.raises(RuntimeError, match="int64"):
        bank.gather_depth_into(idx.int(), torch.empty(bank.total, device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        bank.gather_depth_into(idx, torch.empty(bank.total - 1, device=DEV))


def test_sampler_batches_come_with_their_depths():
    bank, depths = _depth_bank(np.float16, K=3, H=12, W=16, roi=(0.25, 0.75, 0.25, 1))
    window = torch.from_numpy(depths[:, 3:9, 4:16].astype(np.float32).reshape(-1)).to(DEV)
    src = DeviceSimpleSampler(bank, 32, seed=5)
    for _ in range(3):
        idx, rays, _rgb = src.next_batch()
        assert torch.equal(bank.gather_depth(idx), window[idx])
        assert torch.equal(bank.gather(idx)[0], rays)


# ---- the captured step ----
W0, RATE, STEP, END = 0.3, 0.5, 2, 3
N_IT, FACTOR, BATCH = 5, 0.95, 128


def _step_bank():
    g = np.random.default_rng(11)
    q, _ = np.linalg.qr(g.standard_normal((4, 3, 3)))
    poses = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))
    poses[:, :3, :3] = q
    poses[:, :3, 3] = g.uniform(-0.25, 0.25, (4, 3))
    depths = g.uniform(0.5, 6.0, (4, 32, 64)).astype(np.float32)
    depths[g.uniform(size=depths.shape) < 0.3] = 0
    return RayBank(poses, g.integers(0, 256, (4, 32, 64, 4), dtype=np.uint8), (64, 32), device=DEV, depths=depths)   # 8192 rays


def _loss_of(m, weights):
    def loss_fn(rgb, gt, alpha, sched, depth):
        w = sched.stepped(W0, RATE, STEP, end_iter=END)
        weights.copy_(w)   # inside the graph too: the weight each replay used
        return torch.mean((rgb - gt) ** 2) + w * depth_loss(alpha, m.last_train_z, depth)
    return loss_fn


@functools.lru_cache(maxsize=None)
def _eager_run():
    """The eager loop on the bank's first N_IT batches with the Python formula for the weight; computed once, read by both step tests."""
    bank = _step_bank()
    src = DeviceSimpleSampler(bank, BATCH, seed=77)
    jit = torch.from_numpy(synth.hash_uniform(19, 0, BATCH * 16).reshape(BATCH, 16).astype(np.float32)).to(DEV)
    batches = []
    for k in range(N_IT):
        idx = src.indices_at(k)
        batches.append((*bank.gather(idx), bank.gather_depth(idx)))
    _, m = _setup(6)
    opt = FusedAdam(m.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    losses, terms = [], []
    for it, (rays, gt, depth) in enumerate(batches):
        rgb, _d, _bg, _env, alpha = m(rays, is_train=True, jitter=jit, u=jit, **KW)
        w = 0.0 if it > END else W0 * RATE ** int(it / STEP)     # train.py:276-281
        d = depth_loss(alpha, m.last_train_z, depth)
        loss = torch.mean((rgb - gt) ** 2) + w * d
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        for grp in opt.param_groups:
            grp["lr"] *= FACTOR
        m.update_coarse_sigma_grid()
        losses.append(float(loss.detach()))
        terms.append(float(d.detach()))
    assert all(t > 0 for t in terms)   # the term is there
    return bank, jit, batches, losses, {k: p.detach().clone() for k, p in m.named_parameters()}


def _check_against_eager(step, m_g, got, seen_w):
    _, _, _, ref_losses, ref_params = _eager_run()
    assert step.iterations == N_IT
    assert seen_w == [np.float32(0.0 if it > END else W0 * RATE ** int(it / STEP)) for it in range(N_IT)], seen_w
    assert seen_w[0] > seen_w[2] > 0 and seen_w[4] == 0      # across a step boundary and past end_iter
    for a, b in zip(ref_losses[1:], got):
        assert abs(a - b) <= 5e-5 * max(abs(a), 1e-3), (ref_losses, got)
    pg = dict(m_g.named_parameters())
    for k in ref_params:
        _same_after_adam(k, ref_params[k], pg[k].detach(), n_steps=N_IT, lr=0.02)


def test_graphed_step_with_the_depth_term_fed_from_the_bank():
    """mse + stepped(...) * depth_loss inside the captured step, the batch AND its depth targets drawn inside the graph: five iterations
    with pinned noise against the eager loop, at the tolerances tests/test_hip_train_graph.py uses."""
    bank, jit, batches, _, _ = _eager_run()
    _, m_g = _setup(6)
    o_g = FusedAdam(m_g.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=FACTOR)
    weights = torch.zeros((), device=DEV)
    src = DeviceSimpleSampler(bank, BATCH, seed=77)
    step = GraphedTrainStep(m_g, o_g, render_kwargs=KW, loss_fn=_loss_of(m_g, weights), warmup=1, noise_fn=lambda a, b, d: jit, batch_source=src)
    assert torch.equal(step.depth, batches[0][2])
    seen_w, got = [float(weights)], []
    for k in range(1, N_IT):
        got.append(float(step()))
        seen_w.append(float(weights))
        assert torch.equal(step.depth, batches[k][2]) and torch.equal(step.rays, batches[k][0])
    _check_against_eager(step, m_g, got, seen_w)
    with pytest.raises(ValueError, match="batch_source"):
        step(depth=step.depth)


def test_graphed_step_with_the_depth_term_fed_from_the_host():
    _, jit, batches, _, _ = _eager_run()
    _, m_g = _setup(6)
    o_g = FusedAdam(m_g.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=FACTOR)
    weights = torch.zeros((), device=DEV)
    with pytest.raises(ValueError, match="no depth source"):
        GraphedTrainStep(m_g, o_g, batches[0][0], batches[0][1], KW, loss_fn=_loss_of(m_g, weights), warmup=1)
    step = GraphedTrainStep(m_g, o_g, batches[0][0], batches[0][1], KW, loss_fn=_loss_of(m_g, weights), warmup=1, noise_fn=lambda a, b, d: jit,
                            depth=batches[0][2])
    seen_w, got = [float(weights)], []
    for rays, gt, depth in batches[1:]:
        got.append(float(step(rays, gt, depth=depth)))
        seen_w.append(float(weights))
    _check_against_eager(step, m_g, got, seen_w)
    with pytest.raises(ValueError, match="depth="):
        step(batches[0][0], batches[0][1])


# ---- the term alone ----
def test_the_term_alone_pulls_a_student_towards_the_teacher_s_depth():
    """Teacher: scene 6's eval depth_map on 64 rays; student: another seed, the depth term alone, 30 FusedAdam steps.  The condition is
    that the loss falls (as in the distortion test).  That it should is checked first where nothing of the HIP path takes part: the same
    loop on the float64 oracle on the CPU, torch autograd through the definition, torch's Adam on the density tables."""
    cfg, teacher = _scene(6, envmap=False)
    rays, jit = _batch(64, 41)
    with torch.no_grad():
        target = teacher(rays, **KW)[1].clone()
    assert bool((target > 0).all()) and bool(torch.isfinite(target).all())
    tail = rays[:, 5].contiguous()

    oracle = make_oracle(cfg, synth.make_weights(cfg, seed=7), dtype=torch.float64)
    dens = [v.requires_grad_(True) for k, v in oracle.w.items() if k.startswith("density_")]
    adam = torch.optim.Adam(dens, lr=0.02, betas=(0.9, 0.99))
    r64, j64, t64 = rays.cpu().double(), jit.cpu().double(), target.cpu().double()
    seen64 = []
    for _ in range(30):
        out, inter = oracle.forward(r64, is_train=True, jitter=j64, u=j64, keep=True, **KW)
        w = inter["weight"]
        D = (w * inter["z"]).sum(-1) + (1.0 - w.sum(-1)) * r64[:, 5]
        loss = torch.mean((D - t64) ** 2)
        adam.zero_grad(set_to_none=True)
        loss.backward()
        adam.step()
        oracle.update_coarse_sigma_grid()
        seen64.append(float(loss.detach()))
    assert seen64[0] > 0 and seen64[-1] < seen64[0], seen64

    _, student = _setup(7)
    opt = FusedAdam(student.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    seen = []
    for _ in range(30):
        alpha = student(rays, is_train=True, jitter=jit, u=jit, **KW)[4]
        loss = depth_loss(alpha, student.last_train_z, target, tail=tail)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        student.update_coarse_sigma_grid()
        seen.append(loss.detach())
    seen = [float(t) for t in seen]
    print(f"depth term alone, 30 steps: HIP {seen[0]:.4g} -> {seen[-1]:.4g} (ratio {seen[-1] / seen[0]:.3f}); "
          f"float64 oracle {seen64[0]:.4g} -> {seen64[-1]:.4g} (ratio {seen64[-1] / seen64[0]:.3f})")
    assert seen[0] > 0 and seen[-1] < seen[0], seen
