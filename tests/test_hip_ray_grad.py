"""Ray gradients on the GPU (csrc/ego_ray_grad.hip, egonerf_amd/train.py, egonerf_amd/poses.py): d loss / d rays of the
training render against the float64 oracle's autograd, the per-sample positional gradient through the C ABI on hand-placed points, bit
reproducibility, the frozen-model backward, the refusals, the unchanged no-grad paths, and pose refinement on a tiny scene.

Measured on an MI355X, worst ray of every case relative to max |g64| of the half judged (origin / direction): README, "Ray gradients"."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from egonerf_amd import synth
from tests import ray_grad_ref as ref
from tests.helpers import make_model, make_oracle

T = torch.from_numpy
pytestmark = pytest.mark.gpu


def _render(model, rays, fwd, jitter, u, **more):
    return model(rays, is_train=True, exp_sampling=True, jitter=jitter.cuda(), u=None if u is None else u.cuda(), **fwd, **more)


def _hip_ray_grad(name, freeze=False):
    """(rays.grad [N,6], chart [N,S], rgb, model) of the case: MSE against the hashed targets, backward."""
    cfg, w, rays, fwd, jitter, u, gt = ref.case_inputs(name)
    model = make_model(cfg, w, "cuda")
    model.train()
    if freeze:
        for p in model.parameters():
            p.requires_grad_(False)
        if model.envmap is not None:
            model.envmap.emission.requires_grad_(False)
    r = rays.cuda().requires_grad_(True)
    rgb = _render(model, r, fwd, jitter, u)[0]
    assert rgb.requires_grad
    chart = rgb.grad_fn.saved["coords"][..., 3].detach().cpu().clone()    # the forward's choice of chart per sample
    torch.mean((rgb - gt.cuda()) ** 2).backward()
    return r.grad, chart, rgb.detach(), model


@functools.lru_cache(maxsize=None)
def _reference(name, chart_bytes):
    """{f64, f32: (g_rays, rgb)} for the chart the kernel chose: computed once per case, shared, never modified."""
    cfg, w, rays, fwd, jitter, u, gt = ref.case_inputs(name)
    S = (fwd["n_coarse"] if fwd.get("use_coarse_sample", True) else 0) + fwd.get("n_fine", 0) if fwd.get("resampling") else fwd["n_coarse"]
    chart = T(np.frombuffer(chart_bytes, np.float32).reshape(rays.shape[0], S).copy()).long()
    return {tag: ref.oracle_ray_grad(cfg, w, rays, fwd, jitter, u, gt, chart, dt) for tag, dt in (("f64", torch.float64), ("f32", torch.float32))}


@pytest.mark.parametrize("name", list(ref.CASES))
def test_ray_gradient_against_float64(name):
    g, chart, rgb, _ = _hip_ray_grad(name)
    N = g.shape[0]
    assert g.shape == (N, 6) and bool(torch.isfinite(g).all())
    if N >= 64:
        assert 0 < int((chart != 0).sum()) < chart.numel(), "both charts must occur"
    R = _reference(name, chart.numpy().astype(np.float32).tobytes())
    (g64, rgb64), (g32, _) = R["f64"], R["f32"]
    assert float((rgb.cpu().double() - rgb64).abs().max()) <= 1e-4           # the same render
    assert float(g64[:, :3].abs().max()) > 0 and float(g64[:, 3:].abs().max()) > 0
    well = name in ref.WELL_CONDITIONED
    j = ref.RayJudge(name)
    j.check("origin", g[:, :3], g32[:, :3], g64[:, :3], factor=0.2 if well else 1.0)
    j.check("direction", g[:, 3:], g32[:, 3:], g64[:, 3:], factor=0.2 if well else 1.0)
    j.finish(N, may_excuse=not well)


# ---- per-sample d_xyz through the C ABI -----------------------------------------------------------------------------------------------
def _slot_order(dfe27):
    """[M,27] feature gradients -> ego_shade_backward's [M,32] column order (ego_train_layout(2))."""
    from egonerf_amd import _lib
    buf = (C.c_int32 * 32)()
    _lib.check(_lib.load().ego_train_layout(2, buf, 32), "ego_train_layout")
    out = torch.zeros(dfe27.shape[0], 32)
    for col, f in enumerate(buf):
        if 0 <= f < dfe27.shape[1]:
            out[:, col] = dfe27[:, f]
    return out


def test_per_sample_gradient_on_hand_placed_points():
    # the tiny scene, and one with three unequal axis resolutions, one of them odd: a mixed-up axis in the kernel's tap addresses or
    # in the derivative's factor (n - 1) / 2 shows only there (the tiny scene has N_r = N_theta).  Its 4 density components leave 12 of
    # a row's 16 lanes idle in plane_terms, its 20 appearance components need a second, partial pass of 16.
    for cfg in (synth.SceneConfig(n_voxel=20 ** 3),
                synth.SceneConfig(n_voxel=20 ** 3, grid=[6, 5, 8], density_n_comp=(4, 4, 4), app_n_comp=(20, 20, 20))):
        _per_sample_gradient(cfg)


def _per_sample_gradient(cfg):
    from egonerf_amd import _lib
    w = synth.make_weights(cfg, seed=1234)
    o64, o32 = make_oracle(cfg, w, dtype=torch.float64), make_oracle(cfg, w)
    xyz, yang = ref.hand_placed_points(o64)
    n_in = len(yang)
    # three more: beyond far_r by three widths of the last radius cell (r^ > 1 + 2 / (n_r - 1): every r tap masked), and two ordinary
    # points whose coordinates are then overridden with r^ < -1 - 2 / (n_r - 1) and with NaN
    G = o64.r_lut.double().numpy()
    far_pt = o64.center.double().numpy() + np.array([float(o64.far_r) + 3 * (G[-1] - G[-2]), 0.0, 0.0])
    xyz = np.concatenate([xyz, far_pt[None].astype(np.float32), xyz[:1], xyz[n_in // 2:n_in // 2 + 1]])
    yang = np.concatenate([yang, [False, yang[0], yang[n_in // 2]]])
    M = len(yang)
    xyz_t, yang_t = T(xyz), T(yang)
    dfeat = T(synth.hash_uniform(21, 1, M).astype(np.float32)) - 0.5
    dfe = T(synth.hash_uniform(21, 2, M * cfg.app_dim).reshape(M, cfg.app_dim).astype(np.float32)) - 0.5
    g64, _ = ref.sample_grad_reference(o64, xyz_t, yang_t, dfeat, dfe)
    g32, coords = ref.sample_grad_reference(o32, xyz_t, yang_t, dfeat, dfe)
    assert float(g64[n_in].abs().max()) == 0.0                       # the reference agrees about the point beyond far_r
    assert float(coords[n_in, 0]) > 1 + 2 / (cfg.grid[0] - 1)
    coords = coords.float().contiguous()
    coords[n_in + 1, 0] = -1.5
    coords[n_in + 2, :3] = float("nan")
    ref_dist = float((g32.double() - g64)[:n_in].abs().max())
    scale = float(g64[:n_in].abs().max())
    assert scale > 0 and ref_dist > 0

    model = make_model(cfg, w, "cuda")
    sc, lib, st = model.scene(training=True), _lib.load(), _lib.stream_handle()
    rays = torch.cat([xyz_t, T(synth.make_rays(M, seed=9))[:, 3:]], 1).cuda().contiguous()     # z = 0: the sample sits at the origin of its ray
    z = torch.zeros(M, 1, device="cuda")
    dfe64 = torch.zeros(M, 64)
    for m in range(M):
        dfe64[m, 32 * int(yang[m]):32 * int(yang[m]) + cfg.app_dim] = dfe[m]
    for ld, d in ((32, _slot_order(dfe)), (64, dfe64)):
        d_xyz, g_rays = torch.full((M, 3), 7.0, device="cuda"), torch.full((M, 6), 7.0, device="cuda")
        cd, fd, dd = coords.cuda(), dfeat.cuda(), d.cuda().contiguous()
        _lib.check(lib.ego_ray_grad(sc, rays.data_ptr(), z.data_ptr(), cd.data_ptr(), fd.data_ptr(), dd.data_ptr(), ld, None, None, None, None, None,
                                    M, 1, 0, d_xyz.data_ptr(), g_rays.data_ptr(), st), "ego_ray_grad")
        torch.cuda.synchronize()
        err = float((d_xyz.cpu().double() - g64)[:n_in].abs().max())
        print(f"ldfe {ld}: |hip - f64| {err:.3e}  |oracle f32 - f64| {ref_dist:.3e}  (max |g64| {scale:.3e}); tolerance 4 x the latter")
        assert err <= 4 * ref_dist
        assert torch.equal(d_xyz[n_in:].cpu(), torch.zeros(3, 3)), d_xyz[n_in:]           # exact zeros, no NaN
        assert torch.equal(g_rays[:, :3], d_xyz) and torch.equal(g_rays[:, 3:], torch.zeros(M, 3, device="cuda"))
    # N = 0 returns at once
    _lib.check(lib.ego_ray_grad(sc, None, None, None, None, None, 32, None, None, None, None, None, 0, 1, 0, None, None, st), "ego_ray_grad")


# ---- bits ---------------------------------------------------------------------------------------------------------------------------------
def test_two_backward_calls_return_the_same_bits_and_parameter_gradients_are_untouched():
    """The shipped shape, where the parameter gradients are reproducible today (sorted scatters, fixed-order weight gradients)."""
    g1, _, rgb1, m1 = _hip_ray_grad("tiny_resampled")
    g2, _, rgb2, m2 = _hip_ray_grad("tiny_resampled")
    assert torch.equal(g1, g2) and torch.equal(rgb1, rgb2)
    cfg, w, rays, fwd, jitter, u, gt = ref.case_inputs("tiny_resampled")
    m3 = make_model(cfg, w, "cuda")
    m3.train()
    rgb3 = _render(m3, rays.cuda(), fwd, jitter, u)[0]                    # rays that ask for nothing: the parent's step
    torch.mean((rgb3 - gt.cuda()) ** 2).backward()
    assert torch.equal(rgb3.detach(), rgb1)
    for (k, p), q in zip(m1.named_parameters(), m3.parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k


def test_frozen_model(monkeypatch):
    from egonerf_amd import train
    calls = []
    real = train._scatter_tables
    monkeypatch.setattr(train, "_scatter_tables", lambda *a, **k: (calls.append(a[4]), real(*a, **k))[1])
    for name in ("tiny_resampled", "tiny_envmap", "mlp_head", "rgb_head"):
        g_open, _, _, _ = _hip_ray_grad(name)
        assert calls, "the spy sees the unfrozen backward's scatters"
        calls.clear()
        g_frozen, _, _, model = _hip_ray_grad(name, freeze=True)
        assert not calls, calls
        assert all(p.grad is None for p in model.parameters())
        assert model.envmap is None or model.envmap.emission.grad is None
        assert torch.equal(g_frozen, g_open), name


def test_double_backward_raises():
    cfg, w, rays, fwd, jitter, u, gt = ref.case_inputs("n7_s33")
    model = make_model(cfg, w, "cuda")
    r = rays.cuda().requires_grad_(True)
    rgb = _render(model, r, fwd, jitter, u)[0]
    g, = torch.autograd.grad((rgb ** 2).sum(), r, create_graph=True)   # the incoming gradient 2 rgb depends on the rays itself
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):
        g.sum().backward()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    from egonerf_amd import _lib, train
    from egonerf_amd.optim import FusedAdam
    cfg, w, rays, fwd, jitter, u, gt = ref.case_inputs("n7_s33")
    model = make_model(cfg, w, "cuda")
    r = rays.cuda().requires_grad_(True)
    launched = []
    monkeypatch.setattr(train, "_march", lambda *a, **k: launched.append("march"))
    with pytest.raises(NotImplementedError, match="explicit z_coarse"):
        model(r, is_train=True, exp_sampling=False, n_coarse=8)
    with pytest.raises(NotImplementedError, match="ray 0's distances"):
        model(r, is_train=False, exp_sampling=False, n_coarse=8)
    plain = synth.SceneConfig(n_voxel=20 ** 3, interval_th=False)
    with pytest.raises(NotImplementedError, match="plain exponential grid"):
        make_model(plain, synth.make_weights(plain, seed=1234), "cuda")(r, is_train=True, exp_sampling=True, n_coarse=8)
    assert not launched
    monkeypatch.undo()
    opt = FusedAdam(model.get_optparam_groups(), capturable=True, lr_factor=1.0)
    with pytest.raises(NotImplementedError, match="rays that require grad"):
        train.GraphedTrainStep(model, opt, r, gt.cuda(), render_kwargs=dict(fwd, exp_sampling=True))
    with torch.no_grad():   # grad mode off: rays that carry the flag ask for nothing, and nothing is refused
        model(r, is_train=True, exp_sampling=False, n_coarse=8)


# ---- calls without ray gradients take the paths they took --------------------------------------------------------------------------------
def test_no_grad_calls_are_unchanged(monkeypatch):
    from egonerf_amd import train
    cfg, w, rays, fwd, jitter, u, gt = ref.case_inputs("tiny_resampled")
    model = make_model(cfg, w, "cuda")
    kw = dict(exp_sampling=True, **fwd)
    with torch.no_grad():
        base = model(rays.cuda(), **kw)                                     # the inference path (ego_render_forward)
    seen = []
    real = train.render_train
    monkeypatch.setattr(train, "render_train", lambda *a, **k: (seen.append(1), real(*a, **k))[1])
    for p in model.parameters():
        p.requires_grad_(False)
    out = model(rays.cuda(), **kw)                                          # grad mode on, nothing asks: still the inference path
    assert not seen and not out[0].requires_grad
    assert torch.equal(out[0], base[0]) and torch.equal(out[4], base[4]) and torch.equal(out[1], base[1])
    out = model(rays.cuda().requires_grad_(True), **kw)                     # the rays ask: the differentiable path, eval semantics
    assert seen and out[0].requires_grad
    assert float((out[0].detach() - base[0]).abs().max()) <= 1e-5
    # training render: the rays' flag changes no bit of the forward
    for p in model.parameters():
        p.requires_grad_(True)
    a = _render(model, rays.cuda(), fwd, jitter, u)
    b = _render(model, rays.cuda().requires_grad_(True), fwd, jitter, u)
    assert torch.equal(a[0], b[0]) and torch.equal(a[4], b[4]) and torch.equal(a[1], b[1])


# ---- pose refinement ---------------------------------------------------------------------------------------------------------------------
def pose_scene():
    """(cfg, weights, true poses [K,3,4], perturbed poses [K,3,4], H, W, render kw) of the refinement test: K = 3 panoramas of 16 x 32
    around the centre, every pose off by the same 0.03 rad rotation and a 0.03 translation."""
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    w = synth.make_weights(cfg, seed=1234)
    from egonerf_amd.poses import rotate
    eye = torch.eye(3)
    axes = torch.tensor([[0.0, 0.4, 0.0], [0.3, -0.2, 0.1], [-0.2, 0.1, 0.5]])
    R = torch.stack([torch.stack([rotate(axes[k:k + 1], eye[c:c + 1])[0] for c in range(3)], -1) for k in range(3)])
    t = torch.tensor([[0.1, 0.0, -0.05], [-0.08, 0.06, 0.02], [0.0, -0.1, 0.1]])
    truth = torch.cat([R, t[:, :, None]], -1)
    dw = torch.tensor([[0.02, -0.018, 0.012]])
    dR = torch.stack([rotate(dw, eye[c:c + 1])[0] for c in range(3)], -1)
    start = torch.cat([dR[None] @ R, (t + torch.tensor([0.02, -0.018, 0.013]))[:, :, None]], -1)
    return cfg, w, truth, start, 16, 32, dict(n_coarse=32)


def test_refine_poses_on_the_tiny_scene():
    """Localisation in a frozen field: the all-pixel MSE and the pose error (mean rotation angle in radians + mean translation distance)
    both end strictly lower than they start.  Perturbation, rates and step count: the same loop on the float64 oracle descends on the
    CPU (x 6.4 and x 4.2 there; README states the factors an MI355X reached; none is asserted)."""
    from egonerf_amd.data import RayBank
    from egonerf_amd.poses import refine_poses
    from egonerf_amd.renderer import erp_rays
    cfg, w, truth, start, H, W, fwd = pose_scene()
    model = make_model(cfg, w, "cuda")
    K = truth.shape[0]
    kw = dict(exp_sampling=True, **fwd)

    def frames(poses):
        with torch.no_grad():
            return torch.stack([model(erp_rays(H, W, poses[k].numpy(), "cuda", 0, H, normalize=True), **kw)[0] for k in range(K)])

    images = (frames(truth).clamp(0, 1) * 255).to(torch.uint8).view(K, H, W, 3)
    target = images.float() / 255
    bank = RayBank(start, images.cpu(), (W, H), device="cuda")
    mse = lambda poses: float(((frames(poses).view(K, H, W, 3) - target) ** 2).mean())
    err = lambda poses: sum(ref.pose_error(poses, truth))
    mse0, err0 = mse(start), err(start)
    requires = [p.requires_grad for p in model.parameters()]
    deltas, history = refine_poses(model, bank, steps=REFINE["steps"], rays_per_step=REFINE["rays_per_step"], lr_rot=REFINE["lr_rot"],
                                   lr_trans=REFINE["lr_trans"], seed=0, render_kwargs=fwd)
    assert [p.requires_grad for p in model.parameters()] == requires and all(p.grad is None for p in model.parameters())
    assert len(history) == REFINE["steps"] and all(np.isfinite(history))
    with torch.no_grad():
        refined = deltas.poses(bank.poses).cpu()
    mse1, err1 = mse(refined), err(refined)
    print(f"refine_poses: all-pixel MSE {mse0:.3e} -> {mse1:.3e} (x {mse0 / mse1:.1f}), pose error {err0:.3e} -> {err1:.3e} (x {err0 / err1:.1f})")
    assert mse1 < mse0 and err1 < err0


REFINE = dict(steps=60, rays_per_step=256, lr_rot=2e-3, lr_trans=2e-3)
