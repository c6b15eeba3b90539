"""Autograd of the public stage ops (egonerf_amd/stage_autograd.py, csrc/ego_stage_grad.hip): a graph is recorded exactly when a
parameter / input requires grad, the forward bits do not change, and the gradients match the oracle's float64 autograd of the reference
expressions (bar: max|d| / max|truth| <= max(1e-4, 4 x the float32 oracle's own error), the idiom of test_hip_train.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from egonerf_amd import synth
from egonerf_amd.model import SHRender, raw2alpha
from tests.helpers import make_model, make_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
DENSITY = [f"density_{w}_{g}.{i}" for g in ("yin", "yang") for w in ("plane", "line") for i in range(3)]
APP = [f"app_{w}_{g}.{i}" for g in ("yin", "yang") for w in ("plane", "line") for i in range(3)] + ["basis_mat_yin.weight", "basis_mat_yang.weight"]
MLP = [f"renderModule.mlp.{l}.{t}" for l in (0, 2, 4) for t in ("weight", "bias")]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def tiny(golden):
    fx = golden("tiny")
    cfg = synth.SceneConfig(n_voxel=int(fx["n_voxel"]))
    w = synth.make_weights(cfg, seed=int(fx["seed_weights"]))
    return fx, cfg, w, make_model(cfg, w, DEV)


def coords_of(fx):
    """Sample coordinates of the golden scene + out-of-range lookups (zero padding) + points on the yin / yang border."""
    c = np.concatenate([fx["st_c7n"].reshape(-1, 7), fx["lk_coords"].reshape(-1, 7)]).astype(np.float32)
    rng = np.random.default_rng(3)
    b = rng.uniform(-1, 1, (256, 7)).astype(np.float32)
    b[:, [1, 4]] = rng.choice([-1.0, -0.999, 0.999, 1.0], (256, 2))   # theta at the edge of either grid
    b[:, 6] = rng.integers(0, 2, 256)
    return np.concatenate([c, b])


def oracle_grads(cfg, w, keys, fn):
    """{dtype: {key: grad float64}} of fn(oracle) for float32 and float64 oracles."""
    out = {}
    for dt in (torch.float32, torch.float64):
        o = make_oracle(cfg, w, dtype=dt)
        for k in keys:
            o.w[k].requires_grad_(True)
        fn(o, dt).backward()
        out[dt] = {k: (torch.zeros_like(o.w[k]) if o.w[k].grad is None else o.w[k].grad).double() for k in keys}
    return out


def check(model, got: dict, ref: dict, keys, floor=1e-4):
    params = dict(model.named_parameters())
    for k in keys:
        g = got[k] if k in got else params[k].grad
        assert g is not None, k
        truth = ref[torch.float64][k]
        scale = max(float(truth.abs().max()), 1e-30)
        e = float((g.detach().cpu().double() - truth).abs().max()) / scale
        e32 = float((ref[torch.float32][k] - truth).abs().max()) / scale
        assert e <= max(floor, 4 * e32), (k, e, e32)


def zero_grads(model):
    for p in model.parameters():
        p.grad = None
    if getattr(model, "envmap", None) is not None:
        model.envmap.emission.grad = None


def graded(model):
    """name -> tensor of every differentiable tensor of the model (parameters, and the envmap's emission, a plain tensor)."""
    out = dict(model.named_parameters())
    if model.envmap is not None:
        out["envmap.emission"] = model.envmap.emission
    return out


# ---- 1 + 2: graph recorded exactly when needed; forward bits unchanged ------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f16f8", "f16f6", "f32"])
def test_graph_recorded_and_forward_bits_unchanged(tiny, precision):
    fx, cfg, _, model = tiny
    model.mlp_precision = precision
    c = T(coords_of(fx))
    feats = T(fx["st_sigma_feat"])
    rng = np.random.default_rng(1)
    vd = T(rng.normal(size=(c.shape[0], 3)).astype(np.float32))
    sig = T(rng.uniform(0, 5, (8, 32)).astype(np.float32))
    dist = T(rng.uniform(0, 0.2, (8, 32)).astype(np.float32))
    shf = T(rng.normal(size=(c.shape[0], 27)).astype(np.float32))
    ops = {
        "density": lambda: model.compute_densityfeature(c),
        "coarse": lambda: model.compute_coarse_densityfeature(c),
        "app": lambda: model.compute_appfeature(c),
        "f2d": lambda: model.feature2density(feats.requires_grad_(torch.is_grad_enabled())),
        "raw2alpha": lambda: raw2alpha(sig.requires_grad_(torch.is_grad_enabled()), dist)[1],
        "mlp": lambda: model.renderModule(None, vd, model.compute_appfeature(c).detach()),
        "sh": lambda: SHRender(None, vd, shf.requires_grad_(torch.is_grad_enabled())),
    }
    try:
        for name, op in ops.items():
            with_graph = op()
            assert with_graph.requires_grad and with_graph.grad_fn is not None, name
            with torch.no_grad():
                plain = op()
            assert not plain.requires_grad, name
            assert torch.equal(with_graph.detach(), plain), name
        model.app_table_dtype = "f16"
        with_graph = model.compute_appfeature(c)
        with torch.no_grad():
            plain = model.compute_appfeature(c)
        assert with_graph.requires_grad and torch.equal(with_graph.detach(), plain)
    finally:
        model.app_table_dtype = "f32"
        model.mlp_precision = "f16f6"
    # nothing requires grad: no graph, today's path
    for p in model.parameters():
        p.requires_grad_(False)
    try:
        assert not model.compute_densityfeature(c).requires_grad
        assert not model.compute_appfeature(c).requires_grad
        assert not model.renderModule(None, vd, shf).requires_grad
        assert not model.feature2density(feats.detach()).requires_grad
    finally:
        for p in model.parameters():
            p.requires_grad_(True)


# ---- 3: per-op gradients against the float64 oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("coarse", [False, True])
def test_density_gradients(tiny, coarse):
    fx, cfg, w, model = tiny
    c = coords_of(fx)
    g = np.random.default_rng(5).normal(size=c.shape[0]).astype(np.float32)
    zero_grads(model)
    out = (model.compute_coarse_densityfeature if coarse else model.compute_densityfeature)(T(c))
    (out * T(g)).sum().backward()

    def ref(o, dt):
        if coarse:
            o.update_coarse_sigma_grid()
        return (o.density_feature(torch.from_numpy(c).to(dt), coarse=coarse) * torch.from_numpy(g).to(dt)).sum()
    check(model, {}, oracle_grads(cfg, w, DENSITY, ref), DENSITY)


def test_app_gradients(tiny):
    fx, cfg, w, model = tiny
    c = coords_of(fx)
    g = np.random.default_rng(6).normal(size=(c.shape[0], 27)).astype(np.float32)
    zero_grads(model)
    (model.compute_appfeature(T(c)) * T(g)).sum().backward()
    ref = oracle_grads(cfg, w, APP, lambda o, dt: (o.app_feature(torch.from_numpy(c).to(dt)) * torch.from_numpy(g).to(dt)).sum())
    check(model, {}, ref, APP)


@pytest.mark.parametrize("act", ["softplus", "relu"])
def test_feature2density_gradients(tiny, act):
    _, _, _, model = tiny
    f = torch.linspace(-40, 40, 4001, dtype=torch.float64)   # crosses the softplus threshold (x + shift = 20) and relu's kink
    f = torch.cat([f, torch.tensor([28.0, 28.0 + 1e-5, 27.99999, 0.0])]).double()
    g = torch.from_numpy(np.random.default_rng(7).normal(size=f.shape[0]))
    keep = model.fea2denseAct
    model.fea2denseAct = act
    try:
        x = f.float().to(DEV).requires_grad_(True)
        (model.feature2density(x) * g.float().to(DEV)).sum().backward()
    finally:
        model.fea2denseAct = keep
    xr = f.float().double().requires_grad_(True)
    y = F.softplus(xr + model.density_shift) if act == "softplus" else F.relu(xr)
    (y * g).sum().backward()
    assert float((x.grad.cpu().double() - xr.grad).abs().max()) <= 1e-6 * float(g.abs().max())


def test_raw2alpha_gradients():
    rng = np.random.default_rng(8)
    N, S = 64, 96
    sigma = rng.uniform(0, 3, (N, S))
    sigma[:8, 10:20] = 1e4    # opaque samples: 1 - alpha underflows to 0 (+1e-10)
    sigma[8:12] = 0.0
    dist = rng.uniform(0.001, 0.3, (N, S))
    ga, gw, gb = rng.normal(size=(N, S)), rng.normal(size=(N, S)), rng.normal(size=(N, 1))
    s_ = torch.tensor(sigma, dtype=torch.float32, device=DEV, requires_grad=True)
    d_ = torch.tensor(dist, dtype=torch.float32, device=DEV, requires_grad=True)
    a, wt, bg = raw2alpha(s_, d_)
    ((a * T(ga.astype(np.float32))).sum() + (wt * T(gw.astype(np.float32))).sum() + (bg * T(gb.astype(np.float32))).sum()).backward()
    from oracle.egonerf_oracle import OracleScene
    ref = {}
    for dt in (torch.float32, torch.float64):
        s, d = torch.tensor(sigma, dtype=dt, requires_grad=True), torch.tensor(dist, dtype=dt, requires_grad=True)
        a, wt, bg = OracleScene.raw2alpha(s, d)
        ((a * torch.tensor(ga, dtype=dt)).sum() + (wt * torch.tensor(gw, dtype=dt)).sum() + (bg * torch.tensor(gb, dtype=dt)).sum()).backward()
        ref[dt] = (s.grad.double(), d.grad.double())
    for j, got in enumerate((s_.grad, d_.grad)):
        truth = ref[torch.float64][j]
        scale = float(truth.abs().max())
        e = float((got.cpu().double() - truth).abs().max()) / scale
        e32 = float((ref[torch.float32][j] - truth).abs().max()) / scale
        assert e <= max(1e-5, 4 * e32), (j, e, e32)


def _mlp_case(model, cfg, w, seed):
    rng = np.random.default_rng(seed)
    M = 777
    vd = rng.normal(size=(M, 3)).astype(np.float32)
    vd /= np.linalg.norm(vd, axis=1, keepdims=True)
    feat = (rng.normal(size=(M, cfg.app_dim)) * 0.5).astype(np.float32)
    g = rng.normal(size=(M, 3)).astype(np.float32)
    zero_grads(model)
    v_, f_ = T(vd).requires_grad_(True), T(feat).requires_grad_(True)
    (model.renderModule(None, v_, f_) * T(g)).sum().backward()
    ins = {}

    def ref(o, dt):
        v, f = torch.from_numpy(vd).to(dt).requires_grad_(True), torch.from_numpy(feat).to(dt).requires_grad_(True)
        ins[dt] = (v, f)
        return (o.mlp_fea(v, f) * torch.from_numpy(g).to(dt)).sum()
    r = oracle_grads(cfg, w, MLP, ref)
    for dt in ins:
        r[dt]["viewdirs"], r[dt]["features"] = ins[dt][0].grad.double(), ins[dt][1].grad.double()
    check(model, {"viewdirs": v_.grad, "features": f_.grad}, r, MLP + ["viewdirs", "features"])


def test_mlp_fea_gradients(tiny):
    _, cfg, w, model = tiny
    _mlp_case(model, cfg, w, 9)


def test_sh_render_gradients():
    rng = np.random.default_rng(10)
    M = 2000
    vd, feat, g = rng.normal(size=(M, 3)), rng.normal(size=(M, 27)) * 0.3, rng.normal(size=(M, 3))
    v_, f_ = torch.tensor(vd, dtype=torch.float32, device=DEV, requires_grad=True), torch.tensor(feat, dtype=torch.float32, device=DEV, requires_grad=True)
    (SHRender(None, v_, f_) * T(g.astype(np.float32))).sum().backward()

    def sh(d, f):   # sh.py:87-112 degree 2 + tensorBase.py:30-34
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        C1, C2 = 0.4886025119029199, [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
        Y = torch.stack([torch.full_like(x, 0.28209479177387814), -C1 * y, C1 * z, -C1 * x, C2[0] * x * y, C2[1] * y * z,
                         C2[2] * (2 * z * z - x * x - y * y), C2[3] * x * z, C2[4] * (x * x - y * y)], -1)
        return torch.relu((Y[:, None] * f.view(-1, 3, 9)).sum(-1) + 0.5)
    ref = {}
    for dt in (torch.float32, torch.float64):
        d, f = torch.tensor(vd, dtype=dt, requires_grad=True), torch.tensor(feat, dtype=dt, requires_grad=True)
        (sh(d, f) * torch.tensor(g, dtype=dt)).sum().backward()
        ref[dt] = (d.grad.double(), f.grad.double())
    for j, got in enumerate((v_.grad, f_.grad)):
        truth = ref[torch.float64][j]
        scale = float(truth.abs().max())
        e = float((got.cpu().double() - truth).abs().max()) / scale
        assert e <= max(1e-5, 4 * float((ref[torch.float32][j] - truth).abs().max()) / scale), (j, e)


# ---- 4: the sparsity term of train.py:266-272 with 7-column points ----------------------------------------------------------------
@pytest.mark.parametrize("scene", ["tiny", "full"])
def test_sparsity_term(tiny, scene):
    if scene == "tiny":
        _, cfg, w, model = tiny
    else:   # the full-size 27e6-voxel synthetic scene ([150, 172, 516] grid)
        cfg = synth.SceneConfig()
        w = synth.make_weights(cfg, seed=41)
        model = make_model(cfg, w, DEV)
    rng = np.random.default_rng(11)
    pts = rng.uniform(-1, 1, (10000, 7)).astype(np.float32)
    pts[:, 6] = rng.integers(0, 2, 10000)
    zero_grads(model)
    loss = 1 - torch.exp(-0.2 * model.feature2density(model.compute_densityfeature(T(pts)))).mean()
    loss.backward()
    ref = oracle_grads(cfg, w, DENSITY, lambda o, dt: 1 - torch.exp(-0.2 * o.feature2density(o.density_feature(torch.from_numpy(pts).to(dt)))).mean())
    check(model, {}, ref, DENSITY)


# ---- 6: another model shape and the MLP head -------------------------------------------------------------------------------------
def test_other_shape_and_mlp_head():
    # Three unequal axis resolutions, one of them odd: a mixed-up axis in a table size or a tap address (vm_plane_x / _y / vm_line_ax,
    # vm_plane_elems / vm_line_elems of csrc/ego_device.h) shows here and nowhere on a grid with equal axes.  The pooled field is
    # (3, 2, 4): floor-mode pooling drops the odd axis's last row.  4 density components leave 12 of a row's 16 lanes idle in
    # k_scatter_generic, 20 appearance components need a second, partial pass; 3000 samples are no multiple of 64.
    cfg = synth.SceneConfig(n_voxel=20 ** 3, grid=[6, 5, 8], density_n_comp=(4, 4, 4), app_n_comp=(20, 20, 20), app_dim=16, featureC=64,
                            view_pe=3, fea_pe=1, shadingMode="MLP")
    w = synth.make_weights(cfg, seed=21)
    model = make_model(cfg, w, DEV)
    assert model.gridSize.tolist() == [6, 5, 8] and tuple(model.coarse_sigma_plane_yin[0].shape[2:]) == (2, 3)
    rng = np.random.default_rng(12)
    c = rng.uniform(-1.1, 1.1, (3000, 7)).astype(np.float32)
    c[:, 6] = rng.integers(0, 2, 3000)
    gd, ga = rng.normal(size=3000).astype(np.float32), rng.normal(size=(3000, 16)).astype(np.float32)
    keys = DENSITY + APP

    def oracle_loss(coarse):
        def fn(o, dt):
            if coarse:
                o.update_coarse_sigma_grid()
            return ((o.density_feature(torch.from_numpy(c).to(dt), coarse=coarse) * torch.from_numpy(gd).to(dt)).sum()
                    + (o.app_feature(torch.from_numpy(c).to(dt)) * torch.from_numpy(ga).to(dt)).sum())
        return fn
    for coarse in (False, True):   # the full tables, then the pooled ones (the scatter at the pooled resolution + the pooling's backward)
        zero_grads(model)
        density = (model.compute_coarse_densityfeature if coarse else model.compute_densityfeature)(T(c))
        ((density * T(gd)).sum() + (model.compute_appfeature(T(c)) * T(ga)).sum()).backward()
        check(model, {}, oracle_grads(cfg, w, keys, oracle_loss(coarse)), keys)
    _mlp_case(model, cfg, w, 13)


# ---- 7: bit-reproducible on the tuned shape ---------------------------------------------------------------------------------------
def test_backward_is_bit_reproducible(tiny):
    fx, _, _, model = tiny
    c = T(coords_of(fx))
    rng = np.random.default_rng(14)
    vd, g = T(rng.normal(size=(c.shape[0], 3)).astype(np.float32)), T(rng.normal(size=(c.shape[0], 3)).astype(np.float32))
    runs = []
    for _ in range(2):
        zero_grads(model)
        rgb = model.renderModule(None, vd, model.compute_appfeature(c))
        loss = (rgb * g).sum() + model.compute_densityfeature(c).square().sum()
        loss.backward()
        runs.append({k: p.grad.clone() for k, p in model.named_parameters()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


# ---- 8: contract details ----------------------------------------------------------------------------------------------------------
def test_contract_details(tiny):
    fx, _, _, model = tiny
    c = T(coords_of(fx)).requires_grad_(True)
    out = model.compute_densityfeature(c)
    out.sum().backward()
    assert c.grad is None   # coordinates are detached, as in the reference
    # double backward
    f = T(fx["st_sigma_feat"]).requires_grad_(True)
    y = model.feature2density(f)
    (gf,) = torch.autograd.grad((y * y).sum(), f, create_graph=True)
    with pytest.raises(RuntimeError):
        gf.sum().backward()
    # an in-place parameter edit between forward and backward
    out = model.compute_appfeature(c.detach())
    with torch.no_grad():
        model.app_plane_yin[0].add_(0.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
    # errors with grad mode on are the same as without
    with pytest.raises(RuntimeError):
        model.compute_densityfeature(torch.zeros(4, 7))
    with pytest.raises(IndexError):
        model.compute_densityfeature(torch.zeros(4, 3, device=DEV))
    with pytest.raises(IndexError):
        model.compute_appfeature(torch.zeros(4, 6, device=DEV))
    with pytest.raises(RuntimeError):
        raw2alpha(torch.zeros(2, 3, requires_grad=True), torch.zeros(2, 3))


# ---- 5: a render composed of the public stage ops = the fused training render ------------------------------------------------------
@pytest.mark.parametrize("n_voxel,use_envmap", [(20 ** 3, False), (40 ** 3, True)])
def test_stage_composed_render_matches_fused_and_oracle(n_voxel, use_envmap):
    """The non-resampling branch of EgoNeRF.forward (EgoNeRF.py:505-598) rebuilt from the stage ops, pinned jitter, MSE loss: every
    parameter gradient agrees with model(rays, is_train=True)'s (the fused HIP path) and with the oracle's float64 autograd.  With an
    envmap, the background term bg_weight x envmap (EgoNeRF.py:587-590) comes from raw2alpha's third output."""
    cfg = synth.SceneConfig(n_voxel=n_voxel, use_envmap=use_envmap, envmap_res_H=64)
    w = synth.make_weights(cfg, seed=31)
    model = make_model(cfg, w, DEV)
    N, S = 256, 64
    rays_np = synth.make_rays(N, seed=32)
    rng = np.random.default_rng(33)
    jit_np, gt_np = rng.uniform(0, 1, (N, S)).astype(np.float32), rng.uniform(0, 1, (N, 3)).astype(np.float32)
    rays, jit, gt = T(rays_np), T(jit_np), T(gt_np)
    xyz, z, _ = model.sample_ray_exp(rays[:, :3], rays[:, 3:6], is_train=True, N_samples=S, jitter=jit)
    d = torch.cat([z[:, 1:] - z[:, :-1], z[:, -1:] - z[:, -2:-1]], -1)
    c7n = model.coordinates.normalize_coord(model.coordinates.from_cartesian(xyz))
    _, wt, bg = raw2alpha(model.feature2density(model.compute_densityfeature(c7n)), d * cfg.distance_scale)
    rgb = model.renderModule(None, rays[:, None, 3:6].expand(N, S, 3).reshape(-1, 3), model.compute_appfeature(c7n).reshape(-1, cfg.app_dim))
    rgb_map = (wt[..., None] * rgb.view(N, S, 3)).sum(-2)
    if use_envmap:
        rgb_map = rgb_map + bg * model.envmap.get_radiance(rays[:, 3:6])
    rgb_map = rgb_map.clamp(0, 1)
    zero_grads(model)
    torch.mean((rgb_map - gt) ** 2).backward()
    composed = {k: p.grad.clone() for k, p in graded(model).items()}
    zero_grads(model)
    fused_rgb, *_ = model(rays, is_train=True, n_coarse=S, exp_sampling=True, jitter=jit)
    assert float((fused_rgb - rgb_map).detach().abs().max()) <= 1e-4
    torch.mean((fused_rgb - gt) ** 2).backward()
    for k, p in graded(model).items():
        scale = max(float(p.grad.abs().max()), 1e-30)
        assert float((composed[k] - p.grad).abs().max()) / scale <= 2e-4, k
    ref = oracle_grads(cfg, w, list(composed), lambda o, dt: torch.mean(
        (o.forward(torch.from_numpy(rays_np), n_coarse=S, is_train=True, jitter=torch.from_numpy(jit_np))[0] - torch.from_numpy(gt_np).to(dt)) ** 2))
    check(model, composed, ref, list(composed), floor=2e-4)
