"""The any-shape kernels (csrc/ego_generic.hip, the 160-column weight-gradient blocks of train.py) at the corners of the envelope their
header promises - n_comp a multiple of 4 up to 48, app_dim 1..32, featureC 64 | 128, view_pe / fea_pe 0..8 - where a wrong slab row, a
wrong tail of a 2-k-step pipeline or a lost bias column would give plausible numbers that are wrong for that one shape:

  max_encoding    app_dim 32 on featureC 64 (the parked cosines fill the slab, feat[32] / basisT rows / dfe64 are full), eight
                  frequencies of both encodings: 595 MLP inputs = 18 chunks of layer 1, 4 blocks of the weight-gradient product
  min_everything  4 / 4 components, app_dim 1, no encoding: 4 MLP inputs, pipelines shorter than their prefetch depth
  one_feature     app_dim 1 through eight feature frequencies (one half-empty k-step per chunk), 44 components (ragged last line group)
  in160 / in320   the bias column alone in an extra 160-column block; in160 on the SHIPPED 16 / 48 tables: blocked dv + sorted walk
  in159           the bias column is the last column of block 0
  view_only       eight view frequencies and no feature encoding, 44 density components

Everything on the GPU is judged against oracle/egonerf_oracle.py in FLOAT64.  Bounds are the project's (tests/test_model_shapes.py);
where high-frequency encodings make float32 itself inaccurate the oracle's own float32 run says by how much, and a quantity may then
sit within 8x that error (the rule of test_training_gradients_on_other_shapes_vs_reference_autograd) - never for the three
well-conditioned corners, never for features / alpha / depth, and for at most half of a corner's gradient tensors.  The oracle itself is
pinned to the reference at two corners by tests/golden/shape_corners.npz (oracle/capture_golden.py::capture_shape_corners).

Measured on an MI355X, |HIP - f64| (|oracle f32 - f64|) per corner: the table of DESIGN.md 4.5."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from egonerf_amd import synth
from tests.helpers import make_model, make_oracle

T = torch.from_numpy
SEED_WEIGHTS, SEED_RAYS, N_RAYS, M_STAGE = 11, 5, 67, 257
#                  density / appearance n_comp, app_dim, featureC, view_pe, fea_pe, envmap               -> mlp_in
CORNERS = {   # oracle/capture_golden.py::SHAPE_CORNERS captures max_encoding and one_feature from the reference: keep in step
    "max_encoding": (dict(density_n_comp=(48,) * 3, app_n_comp=(48,) * 3, app_dim=32, featureC=64, view_pe=8, fea_pe=8, use_envmap=True), 595),
    "min_everything": (dict(density_n_comp=(4,) * 3, app_n_comp=(4,) * 3, app_dim=1, featureC=64, view_pe=0, fea_pe=0), 4),
    "one_feature": (dict(density_n_comp=(4,) * 3, app_n_comp=(44,) * 3, app_dim=1, featureC=128, view_pe=0, fea_pe=8), 20),
    "in160": (dict(density_n_comp=(16,) * 3, app_n_comp=(48,) * 3, app_dim=29, featureC=128, view_pe=2, fea_pe=2), 160),
    "in159": (dict(density_n_comp=(12,) * 3, app_n_comp=(12,) * 3, app_dim=12, featureC=64, view_pe=0, fea_pe=6), 159),
    "in320": (dict(density_n_comp=(20,) * 3, app_n_comp=(36,) * 3, app_dim=23, featureC=128, view_pe=3, fea_pe=6), 320),
    "view_only": (dict(density_n_comp=(44,) * 3, app_n_comp=(8,) * 3, app_dim=3, featureC=64, view_pe=8, fea_pe=0, use_envmap=True), 54),
}
WELL_CONDITIONED = ("min_everything", "in160", "view_only")   # the float32 oracle alone stays 5x inside every bound: nothing is excused
# the project's bounds (tests/test_model_shapes.py): stage features, per-sample colour, rgb map / alpha, depth, gradients (of the largest entry)
B_FEAT, B_COLOUR, B_MAP, B_DEPTH, B_GRAD = 2e-5, 1e-5, 1e-4, 1e-3, 2e-4


def _cfg(name, **kw):
    return synth.SceneConfig(n_voxel=20 ** 3, envmap_res_H=16, **CORNERS[name][0], **kw)


def _weights(cfg):
    return synth.make_weights(cfg, seed=SEED_WEIGHTS)


def stage_inputs(cfg, M=M_STAGE):
    """oracle/capture_golden.py::corner_stage_inputs: coordinates drawn like capture_shapes' (+-1.3: zero padding included; the grid flag
    from a seventh uniform, so both grids meet inside every 64-sample unit), a few rows moved exactly onto -1, +1 and onto lattice
    planes, and unit directions.  257 = four 64-sample units and one lane."""
    u = T(synth.hash_uniform(98, 0, M * 7).reshape(M, 7).astype(np.float32))
    q = u * 2.6 - 1.3
    q[:, 6] = (u[:, 6] > 0.5).float()
    node = lambda axis, k: -1.0 + 2.0 * k / (cfg.grid[axis] - 1)
    for row, g in ((5, 0), (70, 1)):
        b = 3 * g
        q[row, 6], q[row, b:b + 3] = g, -1.0
        q[row + 1, 6], q[row + 1, b:b + 3] = g, 1.0
        q[row + 2, 6], q[row + 2, b:b + 3] = g, torch.tensor([node(0, 3), node(1, 4), node(2, 7)])
        q[row + 3, 6], q[row + 3, b] = g, node(0, 1)
    dirs = torch.nn.functional.normalize(T(synth.hash_uniform(97, 0, M * 3).reshape(M, 3).astype(np.float32)) * 2 - 1, dim=-1)
    return q, dirs


def train_inputs(N=N_RAYS):
    """jitter [N,16], u [N,16], gt [N,3]: three draws of one seeded torch.Generator (oracle/capture_golden.py::corner_train_inputs)."""
    g = torch.Generator().manual_seed(5)
    return torch.rand(N, 16, generator=g), torch.rand(N, 16, generator=g), torch.rand(N, 3, generator=g)


def _rays():
    return T(synth.make_rays(N_RAYS, seed=SEED_RAYS))


class Judge:
    """hip against the float64 oracle in one norm: passes within the project's bound; or - only where `excusable`, and only if the
    float32 oracle itself misses half that bound - within 8x the float32 oracle's own error.  Every figure is printed."""

    def __init__(self, corner):
        self.corner, self.excused, self.bad, self.n = corner, {}, {}, 0

    def check(self, what, hip, f32, f64, bound, excusable, relative=False):
        hip, f32, f64 = (np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float64) for t in (hip, f32, f64))
        assert hip.shape == f64.shape == f32.shape, (what, hip.shape, f32.shape, f64.shape)
        scale = max(float(np.abs(f64).max()), 1e-12) if relative else 1.0
        hip_err, ref_err = float(np.abs(hip - f64).max()) / scale, float(np.abs(f32 - f64).max()) / scale
        self.n += 1
        print(f"{self.corner:15s} {what:34s} |hip - f64| {hip_err:.2e}   |oracle f32 - f64| {ref_err:.2e}   bound {bound:.0e}")
        if hip_err <= bound:
            return
        if excusable and ref_err > 0.5 * bound and hip_err <= 8 * ref_err:
            self.excused[what] = (float(f"{hip_err:.3g}"), float(f"{ref_err:.3g}"))
        else:
            self.bad[what] = (hip_err, ref_err, bound)

    def finish(self, most_excused=None):
        if self.excused:
            print(f"{self.corner}: excused (|hip - f64|, |oracle f32 - f64|):", self.excused)
        assert not self.bad, self.bad
        if self.corner in WELL_CONDITIONED:
            assert not self.excused, self.excused
        if most_excused is not None:
            assert len(self.excused) <= most_excused, (len(self.excused), most_excused, self.excused)


# ---- the references: computed once per corner, shared, never modified -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stage_reference(name):
    cfg = _cfg(name)
    w = _weights(cfg)
    q, dirs = stage_inputs(cfg)
    out = {}
    with torch.no_grad():
        o64 = make_oracle(cfg, w, dtype=torch.float64)
        feat = o64.app_feature(q.double()).float()   # the head's input: the float64 features, rounded to float32
        for tag, o, c in (("f64", o64, lambda t: t.double()), ("f32", make_oracle(cfg, w), lambda t: t)):
            out[tag] = dict(density=o.density_feature(c(q)), density_coarse=o.density_feature(c(q), coarse=True), app=o.app_feature(c(q)),
                            colour=o.mlp_fea(c(dirs), c(feat)), colour_x8=o.mlp_fea(c(dirs), c(feat * 8)))
    return q, dirs, feat, out


@functools.lru_cache(maxsize=None)
def _render_reference(name):
    out = {}
    with torch.no_grad():
        for variant, kw, fwd in (("resampled", {}, dict(n_coarse=16, n_fine=16, resampling=True)), ("opaque", dict(density_shift=0.0), dict(n_coarse=37))):
            cfg = _cfg(name, **kw)
            w = _weights(cfg)
            for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
                out[variant, tag] = make_oracle(cfg, w, dtype=dt).forward(_rays(), **fwd)
    return out


@functools.lru_cache(maxsize=None)
def _grad_reference(name):
    """{f64, f32: (rgb, {parameter: gradient})} of the is_train render + MSE through the oracle's autograd."""
    cfg = _cfg(name)
    w = _weights(cfg)
    jit, u, gt = train_inputs()
    out = {}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        o = make_oracle(cfg, w, dtype=dt)
        for v in o.w.values():
            v.requires_grad_(True)
        o.update_coarse_sigma_grid()
        rgb = o.forward(_rays(), n_coarse=16, n_fine=16, resampling=True, is_train=True, jitter=jit.to(dt), u=u.to(dt))[0]
        torch.mean((rgb - gt.to(dt)) ** 2).backward()
        out[tag] = (rgb.detach(), {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach() for k, v in o.w.items()})
    return out


# ---- no GPU: the table above, the inputs, and the oracle against the reference at two corners ---------------------------------------
@pytest.mark.parametrize("name", list(CORNERS))
def test_corner_table_and_inputs(name):
    cfg = _cfg(name)
    assert cfg.in_mlpC == CORNERS[name][1]
    assert cfg.use_envmap == (name in ("max_encoding", "view_only"))
    assert (cfg.in_mlpC // 160 + 1) * 160 - cfg.in_mlpC >= 1          # a padding column for the bias gradient, whatever the block edge
    q, dirs = stage_inputs(cfg)
    assert q.shape == (M_STAGE, 7) and dirs.shape == (M_STAGE, 3)
    for u0 in range(0, M_STAGE - 1, 64):                               # both grids inside every 64-sample unit
        assert 0 < int(q[u0:u0 + 64, 6].sum()) < 64
    for g in (0, 1):
        mine = q[q[:, 6] == g][:, 3 * g:3 * g + 3]
        assert bool((mine == -1).all(-1).any()) and bool((mine == 1).all(-1).any())
    assert float((dirs.norm(dim=-1) - 1).abs().max()) < 1e-6


@pytest.mark.parametrize("name", ["max_encoding", "one_feature"])
def test_oracle_reproduces_the_reference_at_the_corners(golden, name):
    """The float32 oracle against the real reference (shape_corners.npz), with the tolerances of
    test_oracle_reproduces_the_reference_on_other_shapes / test_oracle_autograd_reproduces_the_reference_gradients_on_other_shapes.
    These are same-arithmetic tolerances: the oracle keeps the reference's ATen op sequence, so on the kind of host the fixture was
    captured on the two agree to the last bits, while float32 itself is 2e-5 from float64 on these renders - a host whose BLAS sums in
    another order moves the 24-sample render of max_encoding by 4.8e-6 (measured) against the 2e-6 asked here."""
    fx = golden("shape_corners")
    assert (int(fx["seed_weights"]), int(fx["seed_rays"])) == (SEED_WEIGHTS, SEED_RAYS)
    cfg = _cfg(name)
    q, dirs = stage_inputs(cfg)
    jit, u, gt = train_inputs()
    for mine, key in ((q, "coords"), (dirs, "dirs"), (jit, "jitter"), (u, "u"), (gt, "gt")):   # the capture and this module draw the same inputs
        assert np.array_equal(mine.numpy(), fx[f"{name}/{key}"]), key
    sc = make_oracle(cfg, _weights(cfg))
    rays = _rays()
    with torch.no_grad():
        assert float((sc.density_feature(q) - T(fx[f"{name}/density"])).abs().max()) <= 2e-5
        assert float((sc.density_feature(q, coarse=True) - T(fx[f"{name}/density_coarse"])).abs().max()) <= 2e-5
        assert float((sc.app_feature(q) - T(fx[f"{name}/app"])).abs().max()) <= 2e-5
        # the head on the features the reference's head saw: eight frequencies amplify a last-bit difference of a feature 128-fold
        assert float((sc.mlp_fea(dirs, T(fx[f"{name}/app"])) - T(fx[f"{name}/rgb_samples"])).abs().max()) <= 2e-6
        rgb, depth, _, _, alpha = sc.forward(rays, n_coarse=24)
        assert float((rgb - T(fx[f"{name}/nr_rgb"])).abs().max()) <= 2e-6 and float((alpha - T(fx[f"{name}/nr_alpha"])).abs().max()) <= 1e-5
        rgb, depth, *_ = sc.forward(rays, n_coarse=16, n_fine=16, resampling=True)
        assert float((rgb - T(fx[f"{name}/rs_rgb"])).abs().max()) <= 5e-6 and float((depth - T(fx[f"{name}/rs_depth"])).abs().max()) <= 5e-5
    rgb, grads = _grad_reference(name)["f32"]
    assert float((rgb - T(fx[f"{name}/rgb"])).abs().max()) <= 2e-6
    for k in ("density_plane_yin.0", "app_line_yang.2", "basis_mat_yin.weight", "renderModule.mlp.0.weight", "renderModule.mlp.4.bias"):
        ref = fx[f"{name}/grad/{k}"]
        assert float((grads[k] - T(ref)).abs().max()) <= 2e-5 * max(float(np.abs(ref).max()), 1e-12), k


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _model(name, **kw):
    cfg = _cfg(name, **kw)
    model = make_model(cfg, _weights(cfg), "cuda")
    assert not model.is_tuned_shape
    assert model.head_in_mlpC == CORNERS[name][1]
    if name == "in160":   # the shipped table shape under another head: what selects the blocked-dv / sorted-walk route
        assert model.density_n_comp[0] == 16 and model.app_n_comp[0] == 48 and not model.head_is_tuned
    return cfg, model


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CORNERS))
def test_stage_ops_at_the_corners(name):
    cfg, model = _model(name)
    q, dirs, feat, ref = _stage_reference(name)
    f64, f32 = ref["f64"], ref["f32"]
    qd, dd = q.cuda(), dirs.cuda()
    j = Judge(name)
    with torch.no_grad():
        j.check("compute_densityfeature", model.compute_densityfeature(qd), f32["density"], f64["density"], B_FEAT, False)
        j.check("compute_coarse_densityfeature", model.compute_coarse_densityfeature(qd), f32["density_coarse"], f64["density_coarse"], B_FEAT, False)
        af = model.compute_appfeature(qd)
        assert af.shape == (M_STAGE, cfg.app_dim)
        j.check("compute_appfeature", af, f32["app"], f64["app"], B_FEAT, False)
        j.check("renderModule", model.renderModule(None, dd, feat.cuda()), f32["colour"], f64["colour"], B_COLOUR, True)
        # features x 8: the fea_pe = 8 arguments reach ~1e3 rad (gen_sincos's reduction far beyond the first period)
        j.check("renderModule(8 x features)", model.renderModule(None, dd, (feat * 8).cuda()), f32["colour_x8"], f64["colour_x8"], B_COLOUR, True)
    j.finish()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CORNERS))
def test_renders_at_the_corners(name):
    """67 rays x (16 + 16) = 2144 samples: the last 64-sample unit holds one 32-sample tile; 67 x 37 on an opaque field: tiles straddle
    rays and the zero-weight tile skip is active."""
    ref = _render_reference(name)
    rays = _rays().cuda()
    j = Judge(name)
    with torch.no_grad():
        for variant, kw, fwd in (("resampled", {}, dict(n_coarse=16, n_fine=16, resampling=True)), ("opaque", dict(density_shift=0.0), dict(n_coarse=37))):
            cfg, model = _model(name, **kw)
            got = model(rays, exp_sampling=True, **fwd)
            f64, f32 = ref[variant, "f64"], ref[variant, "f32"]
            assert (got[3] is not None) == cfg.use_envmap
            j.check(f"{variant} rgb", got[0], f32[0], f64[0], B_MAP, True)
            j.check(f"{variant} depth", got[1], f32[1], f64[1], B_DEPTH, False)
            j.check(f"{variant} alpha", got[4], f32[4], f64[4], B_MAP, False)
    j.finish()


@pytest.mark.gpu
@pytest.mark.parametrize("scatter", ["default_scatter", "flipped_scatter"])
@pytest.mark.parametrize("name", list(CORNERS))
def test_training_gradients_at_the_corners(name, scatter):
    """is_train render (pinned noise) + MSE: every parameter's gradient against the float64 oracle's autograd, with
    model.deterministic_scatter as it defaults and flipped (float-atomic ego_weight_grad and the fixed-order one, on the multi-block
    layer-1 product and on the block that holds nothing but the bias column)."""
    cfg, model = _model(name)
    if scatter == "flipped_scatter":
        model.deterministic_scatter = not model.deterministic_scatter
    model.train()
    jit, u, gt = train_inputs()
    rgb, depth, _, _, alpha = model(_rays().cuda(), is_train=True, n_coarse=16, n_fine=16, exp_sampling=True, resampling=True, use_coarse_sample=True,
                                    jitter=jit.cuda(), u=u.cuda())
    assert rgb.requires_grad
    torch.mean((rgb - gt.cuda()) ** 2).backward()
    ref = _grad_reference(name)
    (rgb64, g64), (rgb32, g32) = ref["f64"], ref["f32"]
    jr = Judge(name)
    jr.check("is_train rgb", rgb, rgb32, rgb64, B_MAP, True)
    jr.finish()
    named = dict(model.named_parameters())
    if cfg.use_envmap:
        named["envmap.emission"] = model.envmap.emission
    assert set(named) == set(g64)
    j = Judge(name)
    for k, p in named.items():
        assert p.grad is not None, k
        assert bool(torch.isfinite(p.grad).all()), k
        if bool((g64[k] != 0).any()):
            assert bool((p.grad != 0).any()), f"{k}: gradient identically zero"
        j.check(k, p.grad, g32[k], g64[k], B_GRAD, True, relative=True)
    if name in ("in160", "in320", "max_encoding"):   # the column a 160-column block edge can lose
        k = "renderModule.mlp.0.bias"
        scale = float(g64[k].abs().max())
        assert scale > 0 and k not in j.bad
        hip_err = float((named[k].grad.cpu().double() - g64[k]).abs().max()) / scale
        assert hip_err <= B_GRAD or k in j.excused, (k, hip_err)
    j.finish(most_excused=len(named) // 2)


# ---- the any-shape kernels bit for bit against a recorded build ---------------------------------------------------------------------
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generic_digests.json")
DIGEST_M = (3, 43)              # 129 samples: three 64-sample units, the last holding one lane
DIGEST_BIG = 4097 * 64 + 1      # both kernels' unit loops take a second trip (grids of 2048 x 2 and 4096 waves)
DIGEST_MODELS = {**{name: (name, {}, 160) for name in CORNERS}, "rgb_head": (None, dict(shadingMode="RGB", app_dim=3), 160),
                 "in160 blocked dv": ("in160", {}, 0)}   # case -> (corner, SceneConfig keywords, ldv of the backward; 0 = the tuned scatters' blocked dv)


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _digest_coords(cfg, M):
    """stage_inputs' coordinates with the grid flag overridden: samples 0..63 yin, 64..127 yang, the rest as drawn (mixed).  A unit then
    meets any_yang == false, one meets any_yin == false; with M = 129 the third unit holds one lane (its idle lanes repeat it), so the
    unit that meets both grids is every later unit of the large case.  -> c7n [M][7], coords [M][4] (the sample's own grid's triple), dirs"""
    q, dirs = stage_inputs(cfg, M)
    q[:64, 6], q[64:128, 6] = 0.0, 1.0
    g = q[:, 6] != 0
    coords = torch.cat([torch.where(g[:, None], q[:, 3:6], q[:, 0:3]), q[:, 6:7]], -1).contiguous()
    return q, coords, dirs


def _train_pair_digests(model, cfg, N, S, ldx, ldh, ldv_fwd, ldv_bwd):
    """ego_shade_train_generic, then ego_shade_backward_generic on its dumps, through the C ABI: the digest of every output buffer."""
    from egonerf_amd import _lib
    lib, st, M = _lib.load(), _lib.stream_handle(), N * S
    sc = model.scene(training=True)
    _, coords, _ = _digest_coords(cfg, M)
    coords = coords.cuda()
    rays = T(synth.make_rays(N, seed=SEED_RAYS)).cuda()
    hid, mlp = model.head_hidden, cfg.shadingMode != "RGB"
    z = lambda *shape: torch.zeros(*shape, device="cuda")
    rgb, v = z(M, 3), z(M, ldv_fwd)
    x, h1, h2 = (z(M, ldx), z(M, ldh), z(M, ldh)) if mlp else (None, None, None)
    _lib.check(lib.ego_shade_train_generic(sc, rays.data_ptr(), coords.data_ptr(), N, S, rgb.data_ptr(), _lib.ptr(x), ldx, _lib.ptr(h1), _lib.ptr(h2), ldh,
                                           v.data_ptr(), ldv_fwd, st), "ego_shade_train_generic")
    dc = (T(synth.hash_uniform(96, 0, M * 3).reshape(M, 3).astype(np.float32)) - 0.5).cuda()
    dh2, dh1 = (z(M, hid), z(M, hid)) if mlp else (None, None)
    dfe, dv = z(M, 64), z(M, ldv_bwd) if ldv_bwd else z((M + 31) // 32 * 32, 144)
    _lib.check(lib.ego_shade_backward_generic(sc, coords.data_ptr(), dc.data_ptr(), rgb.data_ptr(), _lib.ptr(x), ldx, _lib.ptr(h1), _lib.ptr(h2), ldh,
                                              _lib.ptr(dh2), _lib.ptr(dh1), dfe.data_ptr(), dv.data_ptr(), ldv_bwd, N, S, st), "ego_shade_backward_generic")
    torch.cuda.synchronize()
    named = dict(rgb=rgb, x=x, h1=h1, h2=h2, v=v, dc=dc, dh2=dh2, dh1=dh1, dfe64=dfe, dv=dv)
    return {k: _sha(t) for k, t in named.items() if t is not None}


def generic_digests():
    """case -> {buffer: sha256 of its bytes} for direct calls of the any-shape kernels: ego_shade_train_generic (rgb, x, h1, h2, v) and
    ego_shade_backward_generic (dc, dh2, dh1, dfe64, dv) on 3 x 43 samples, compute_appfeature, renderModule and an eval forward with
    n_coarse = 37 (rgb, depth, alpha), for the seven CORNERS, one shadingMode "RGB" model and in160 with the blocked dv (ldv = 0); and
    the training pair once more on min_everything with 4097 x 64 + 1 samples (tight leading dimensions: every buffer under 100 MB).
    ego_scatter_generic adds floats in arrival order and is left out.  tools/capture_digests.py records this from another build."""
    out = {}
    with torch.no_grad():
        for case, (corner, kw, ldv_bwd) in DIGEST_MODELS.items():
            cfg = _cfg(corner) if corner else synth.SceneConfig(n_voxel=20 ** 3, **kw)
            model = make_model(cfg, _weights(cfg), "cuda")
            assert not model.is_tuned_shape
            ldx = (model.head_in_mlpC // 160 + 1) * 160
            out[case] = d = _train_pair_digests(model, cfg, *DIGEST_M, ldx, 160, 160, ldv_bwd)
            if ldv_bwd == 0:
                continue   # the same model's stage ops and render are digested under its corner's name
            q, _, dirs = _digest_coords(cfg, DIGEST_M[0] * DIGEST_M[1])
            feat = model.compute_appfeature(q.cuda())
            rgb, depth, _, _, alpha = model(_rays().cuda(), n_coarse=37, exp_sampling=True)
            d.update(compute_appfeature=_sha(feat), renderModule=_sha(model.renderModule(None, dirs.cuda(), feat)), eval_rgb=_sha(rgb),
                     eval_depth=_sha(depth), eval_alpha=_sha(alpha))
        cfg = _cfg("min_everything")
        model = make_model(cfg, _weights(cfg), "cuda")
        out[f"min_everything M={DIGEST_BIG}"] = _train_pair_digests(model, cfg, DIGEST_BIG, 1, model.head_in_mlpC, model.head_hidden, 12, 12)
    return out


@pytest.mark.gpu
def test_generic_bits_match_recorded():
    """The head kernels have no atomics, so a rewrite that keeps their arithmetic returns the recorded build's bytes: equality, no
    tolerance.  The fixture names the commit it was recorded from (never the tree under test)."""
    recorded = json.load(open(DIGESTS))["digests"]
    got = generic_digests()
    assert len(got) == len(DIGEST_MODELS) + 1 == 10 and {c: sorted(d) for c, d in got.items()} == {c: sorted(d) for c, d in recorded.items()}
    differs = [f"{case}: {name}" for case in got for name in got[case] if got[case][name] != recorded[case][name]]
    assert not differs, differs


@pytest.mark.gpu
@pytest.mark.parametrize("what,kw", [
    ("app_dim 33", dict(app_dim=33)),
    ("n_comp 52", dict(density_n_comp=(52,) * 3, app_n_comp=(52,) * 3)),
    ("n_comp 6", dict(density_n_comp=(6,) * 3, app_n_comp=(6,) * 3)),
    ("density n_comp 52", dict(density_n_comp=(52,) * 3)),
    ("density n_comp 6", dict(density_n_comp=(6,) * 3)),
    ("featureC 96", dict(featureC=96)),
    ("view_pe 9", dict(view_pe=9)),
    ("fea_pe 9", dict(fea_pe=9)),
])
def test_shapes_just_outside_the_envelope_are_refused(what, kw):
    """Construction or the first render / stage op / training step raises with the library's message: it comes from the host checks
    (check_generic_shape, ego_generic_march, ego_density_feature), which return before anything is launched - a launch with these
    shapes would index past feat[32], the slab or a table row."""
    base = dict(density_n_comp=(8,) * 3, app_n_comp=(24,) * 3, app_dim=27, featureC=64, view_pe=2, fea_pe=2)
    base.update(kw)
    cfg = synth.SceneConfig(n_voxel=20 ** 3, **base)
    w = _weights(cfg)
    rays = T(synth.make_rays(5, seed=SEED_RAYS)).cuda()
    q, dirs = stage_inputs(cfg)

    def render():
        with torch.no_grad():
            return make_model(cfg, w, "cuda")(rays, n_coarse=8, exp_sampling=True)

    def train():
        model = make_model(cfg, w, "cuda")
        model.train()
        return model(rays, is_train=True, n_coarse=8, exp_sampling=True)

    def stages():
        with torch.no_grad():
            model = make_model(cfg, w, "cuda")
            model.compute_densityfeature(q.cuda())
            feat = model.compute_appfeature(q.cuda())
            return model.renderModule(None, dirs.cuda(), feat)

    for call in (render, train, stages):
        with pytest.raises((RuntimeError, NotImplementedError), match=r"supported: ") as e:
            call()
        assert "failed (code" in str(e.value), e.value     # the C library's own refusal, passed on by the host layer
    torch.cuda.synchronize()                                 # and the device is as it was
