"""The dense density route on the device: the bake kernel against its float64 reference, the dense march against the factored one
through ego_march_density on one scene (pointer set / cleared), and the eval forward with the route on, off and re-baked."""
import ctypes
import os

import numpy as np
import pytest
import torch

from egonerf_amd import _lib, field_tables, synth
from egonerf_amd.model import YinYangAlphaGridMask
from tests import dense_density_ref as ref
from tests.helpers import make_model, make_oracle, maxerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
RGB_TOL = 1e-4            # tests/test_hip_parity.py
DEPTH_TOL = 1e-3 * 15.0   # ... its depth bar for the far = 15 scenes
WEIGHT_TOL = 1e-6         # ... its bar on alpha / weight / bg_weight (test_stage_density_alpha_mlp)


# ---- the bake kernel ------------------------------------------------------------------------------------------------------------------
def _device_field(tables, res):
    views = field_tables.carve_channel_last([t.shape[1:] for t in tables], DEV)
    for v, t in zip(views, tables):
        v.copy_(torch.from_numpy(t))
    f = _lib.VmField()
    f.n_comp = tables[0].shape[1]
    f.res[:] = list(res)
    field_tables.fill_pointers(f, views)
    return f, views


def _bake_on_device(f, res):
    out = torch.full((2, res[2], res[1], res[0], 4), float("nan"), device=DEV)
    _lib.check(_lib.load().ego_bake_density_dense(ctypes.byref(f), out.data_ptr(), _lib.stream_handle()), "bake")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_bake(got, tables, res):
    G, A = ref.bake(tables, res)
    assert got.shape == G.shape                      # [grid][N_phi][N_theta][N_r][4]: the reference indexes exactly that order
    assert np.array_equal(got[..., 3], np.zeros_like(got[..., 3]))
    err, bound = np.abs(got[..., :3].astype(np.float64) - G[..., :3]), 16 * 2.0 ** -23 * A
    print("bake", res, "max err", float(err.max()), "max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert float(np.abs(G[..., :3]).max()) > 0.5 and len({float(G[g, 1, 2, 3, i]) for g in range(2) for i in range(3)}) == 6


def test_bake_kernel_against_float64():
    res = [5, 6, 7]
    tables = ref.random_tables(res, seed=11)
    f, _keep = _device_field(tables, res)
    _check_bake(_bake_on_device(f, res), tables, res)


def test_bake_kernel_on_the_pooled_field():
    full, res = [12, 14, 18], [6, 7, 9]
    tables = ref.random_tables(full, seed=12)
    fs, _keep = _device_field(tables, full)
    fd, pooled = _device_field([np.zeros((1, 16, max(t.shape[2] // 2, 1), max(t.shape[3] // 2, 1)), np.float32) for t in tables], res)
    _lib.check(_lib.load().ego_avgpool_field(ctypes.byref(fs), ctypes.byref(fd), _lib.stream_handle()), "avgpool")
    torch.cuda.synchronize()
    _check_bake(_bake_on_device(fd, res), [p.cpu().numpy() for p in pooled], res)


def test_bake_refuses_what_the_march_cannot_read():
    res = [5, 6, 7]
    f, _keep = _device_field(ref.random_tables(res, seed=13, n_comp=8), res)
    out = torch.zeros(2 * 5 * 6 * 7 * 4 + 1, device=DEV)
    lib = _lib.load()
    assert lib.ego_bake_density_dense(ctypes.byref(f), out.data_ptr(), None) == -2 and b"n_comp" in lib.ego_last_error()
    f16, _keep16 = _device_field(ref.random_tables(res, seed=13), res)
    assert lib.ego_bake_density_dense(ctypes.byref(f16), out.data_ptr() + 4, None) == -1 and b"aligned" in lib.ego_last_error()


# ---- the march: dense against factored on one scene -----------------------------------------------------------------------------------
N_RAYS = 5   # the last workgroup is ragged (4 rays per workgroup, 2 when a ray is split over two waves)


def _rays():
    rays = synth.make_rays(N_RAYS, seed=5)
    rays[3:, 3:6] *= 2.0   # twice the reach: these rays leave the radius LUT's last knot behind (normalised r > 1: zero-padded taps)
    return torch.from_numpy(rays).to(DEV)


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name, shift in (("masked", -8.0), ("masked_other_res", -8.0), ("opaque", 0.0)):
        cfg = synth.SceneConfig(n_voxel=20 ** 3, density_shift=shift)
        w = synth.make_weights(cfg, seed=7)
        model = make_model(cfg, w, DEV)
        if name != "opaque":
            n_r, n_th, n_ph = cfg.grid
            if name == "masked_other_res":    # a mask that is not at the field's resolution: the dense march sets its taps up separately
                n_r, n_th, n_ph = n_r + 3, n_th + 2, n_ph - 3
            vol = torch.ones(2, n_ph, n_th, n_r, device=DEV)
            vol[:, :, :, : (8 * n_r) // 10] = 0.0   # the inner shells are empty: whole passes of a ray's first samples are masked out
            vol[1, : n_ph // 3] = 0.0               # ... and a wedge of the yang grid
            model.alphaMask = YinYangAlphaGridMask(DEV, vol[0], vol[1])
            model.use_alpha_mask = True
        out[name] = (cfg, model, make_oracle(cfg, w, dtype=torch.float64))
    return out


def _march(sc, model, cfg, rays, S, with_sigma, with_alpha=False):
    lib, st = _lib.load(), _lib.stream_handle()
    N = rays.shape[0]
    sched = model._sched(S, rays.device)
    z, w, bg = torch.zeros(N, S, device=DEV), torch.zeros(N, S, device=DEV), torch.zeros(N, device=DEV)
    crd = torch.zeros(N, S, 4, device=DEV)
    sigma = torch.zeros(N, S, device=DEV) if with_sigma else None
    alpha = torch.zeros(N, S + 1, device=DEV) if with_alpha else None
    act = torch.zeros((N * S + 31) // 32, device=DEV, dtype=torch.uint8)
    _lib.check(lib.ego_march_density(sc, rays.data_ptr(), N, S, None, sched.data_ptr(), None, cfg.near, 0, z.data_ptr(), _lib.ptr(alpha),
                                     S + 1 if with_alpha else 0, w.data_ptr(), bg.data_ptr(), crd.data_ptr(), _lib.ptr(sigma), act.data_ptr(), st),
               "march")
    torch.cuda.synchronize()
    return dict(z=z, weight=w, bg=bg, alpha=alpha, act=act, crd=crd, sigma=sigma)


def _two_routes(model):
    """The model's inference scene with the baked grids, and a copy of the same struct with the two pointers cleared."""
    dense = model.scene()
    assert dense.density_dense and dense.density_coarse_dense
    factored = _lib.Scene.from_buffer_copy(dense)
    factored.density_dense = None
    factored.density_coarse_dense = None
    return dense, factored


@pytest.mark.parametrize("S,split", [(77, None), (128, None), (256, "1"), (256, "2")])
@pytest.mark.parametrize("which", ["masked", "masked_other_res", "opaque"])
def test_dense_march_against_factored(scenes, which, S, split, monkeypatch):
    """Everything is held against the oracle in float64 at the kernel's own coordinates and distances (density_feature, feature2density,
    raw2alpha: EgoNeRF.py:291-347, tensorBase.py:415-419, :22-27).
    sigma: the dense route's largest error against a float64 evaluation of the factored formula at the kernel's own coordinates is
    at most twice the factored route's against the same values (two rounding stages, the bake and the interpolation, against one).
    Measured on MI355X, dense / factored: 0.80 - 1.39 behind either mask (errors 3.5e-7 - 9.6e-7), 1.00 - 1.10 on the opaque field
    (3.9e-6 - 4.4e-6); each case prints its figures."""
    cfg, model, oracle = scenes[which]
    rays = _rays()
    if split is None:
        monkeypatch.delenv("EGO_MARCH_SPLIT", raising=False)
    else:
        monkeypatch.setenv("EGO_MARCH_SPLIT", split)
    sc_d, sc_f = _two_routes(model)
    assert bool(sc_d.occ) == (which != "opaque")
    assert which == "opaque" or (list(sc_d.occ_res) != list(cfg.grid)) == (which == "masked_other_res")
    d, f = _march(sc_d, model, cfg, rays, S, with_sigma=True), _march(sc_f, model, cfg, rays, S, with_sigma=True)
    assert torch.equal(d["z"], f["z"]) and torch.equal(d["crd"], f["crd"])
    crd = f["crd"].cpu().double()
    assert crd[..., 3].min() == 0.0 and crd[..., 3].max() == 1.0 and crd[..., 0].max() > 1.0   # both grids; beyond the last radial knot
    yang = crd[..., 3:4]
    c7n = torch.cat([crd[..., :3] * (1 - yang), crd[..., :3] * yang, yang], -1)
    sigma64 = oracle.feature2density(oracle.density_feature(c7n)).numpy()
    sig_d, sig_f = d["sigma"].cpu().numpy().astype(np.float64), f["sigma"].cpu().numpy().astype(np.float64)
    empty = sig_f == 0.0                                         # softplus is never 0: exactly the samples the mask removed
    assert np.array_equal(sig_d == 0.0, empty)
    if which != "opaque":
        passes = [empty[n, p * 64:(p + 1) * 64].all() for n in range(N_RAYS) for p in range((S + 63) // 64)]
        assert empty.any() and not all(passes) and not empty.all(-1).any()   # masked samples, and occupied ones on every ray
        assert any(passes) or which != "masked"                              # ... a fully masked pass among them
    else:
        assert not empty.any()
    sigma64[empty] = 0.0
    err_d, err_f = float(np.abs(sig_d - sigma64).max()), float(np.abs(sig_f - sigma64).max())
    print(f"sigma {which} S={S} split={split}: dense err {err_d:.3e} factored err {err_f:.3e} ratio {err_d / max(err_f, 1e-300):.2f}")
    assert err_d <= 2.0 * err_f
    # weights and background weight against the float64 composite of those sigmas (tensorBase.py:22-27) at the kernel's distances
    z = f["z"].cpu().numpy().astype(np.float64)
    dist = np.concatenate([z[:, 1:] - z[:, :-1], z[:, -1:] - z[:, -2:-1]], -1) * cfg.distance_scale
    a64, w64, bg64 = oracle.raw2alpha(torch.from_numpy(sigma64), torch.from_numpy(dist))
    for name, r in (("dense", d), ("factored", f)):
        assert maxerr(r["weight"], w64) <= WEIGHT_TOL and maxerr(r["bg"], bg64[:, 0]) <= WEIGHT_TOL, name
    assert float(a64.max()) > 0.01
    # tile flags (the scene's exact skip): every tile that holds a weight above 0 is flagged - exactly those when tiles are whole pass
    # halves; where tiles straddle rays (S = 77) a pass half flags each tile it touches - and both routes flag the same tiles
    for r in (d, f):
        flat = torch.nn.functional.pad(r["weight"].reshape(-1), (0, (-N_RAYS * S) % 32)).reshape(-1, 32)
        need, got = (flat > 0).any(-1), r["act"].bool()
        assert torch.equal(got, need) if S % 32 == 0 else bool((got | ~need).all())
    assert torch.equal(d["act"], f["act"])


@pytest.mark.parametrize("which", ["masked", "opaque"])
@pytest.mark.parametrize("with_alpha", [False, True])
def test_dense_march_split_returns_the_same_bits(scenes, which, with_alpha, monkeypatch):
    """What tests/test_hip_march_split.py demands of the factored route, of the dense one: distances, weights, background weight, alpha
    and tile flags bit for bit, coordinates wherever a colour is read (the one-wave form stops behind an exactly opaque prefix)."""
    cfg, model, _oracle = scenes[which]
    rays, S, out = _rays(), 256, {}
    sc_d, sc_f = _two_routes(model)
    for split in ("1", "2"):
        monkeypatch.setenv("EGO_MARCH_SPLIT", split)
        out[split] = _march(sc_d, model, cfg, rays, S, with_sigma=False, with_alpha=with_alpha)
    a, b = out["1"], out["2"]
    for k in ("z", "weight", "bg", "alpha", "act"):
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), k
    shaded = a["weight"] > 0
    assert bool(shaded.any()) and torch.equal(a["crd"][shaded], b["crd"][shaded])
    if which == "opaque" and not with_alpha:
        assert bool((a["weight"] == 0).any())
    # ... and against the factored route in that mode: the same distances, the same coordinates wherever both read a colour
    fz = _march(sc_f, model, cfg, rays, S, with_sigma=False, with_alpha=with_alpha)
    both = shaded & (fz["weight"] > 0)
    assert torch.equal(fz["z"], a["z"]) and torch.equal(fz["crd"][both], a["crd"][both])
    assert maxerr(fz["weight"], a["weight"]) <= 2 * WEIGHT_TOL


# ---- the eval forward -------------------------------------------------------------------------------------------------------------------
KWS = [dict(n_coarse=64), dict(n_coarse=32, n_fine=32, resampling=True)]


@pytest.fixture()
def clean_env(monkeypatch):
    for k in ("EGO_DENSE_DENSITY", "EGO_DENSE_DENSITY_MAX_MB", "EGO_MARCH_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _render(model, rays, kw):
    with torch.no_grad():
        return model(rays, exp_sampling=True, **kw)


@pytest.mark.parametrize("kw", KWS)
def test_eval_forward_with_the_dense_route(clean_env, kw):
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    w = synth.make_weights(cfg, seed=7)
    model, plain = make_model(cfg, w, DEV), make_model(cfg, w, DEV)
    plain.dense_density = False
    rays = torch.from_numpy(synth.make_rays(64, seed=21))
    ref_out = make_oracle(cfg, w).forward(rays, **kw)
    rays = rays.to(DEV)
    got, fac = _render(model, rays, kw), _render(plain, rays, kw)
    sc = model.scene()
    assert sc.density_dense and sc.density_coarse_dense and not plain.scene().density_dense and not plain.scene().density_coarse_dense
    for name, out in (("dense", got), ("factored", fac)):
        print(name, kw, "rgb err", maxerr(out[0], ref_out[0]), "depth err", maxerr(out[1], ref_out[1]))
        assert maxerr(out[0], ref_out[0]) <= RGB_TOL and maxerr(out[1], ref_out[1]) <= DEPTH_TOL, name
    # a batch equals the concatenation of its pieces, and a second call the first, bit for bit
    again, head, tail = _render(model, rays, kw), _render(model, rays[:23], kw), _render(model, rays[23:], kw)
    for k in (0, 1):
        assert torch.equal(got[k], again[k]) and torch.equal(got[k], torch.cat([head[k], tail[k]]))
    # switched off by the environment, or capped out: NULL pointers, and the factored build's render
    for key, value in (("EGO_DENSE_DENSITY", "0"), ("EGO_DENSE_DENSITY_MAX_MB", "0")):
        clean_env.setenv(key, value)
        off = _render(model, rays, kw)
        sc = model.scene()
        assert not sc.density_dense and not sc.density_coarse_dense, key
        assert torch.equal(off[0], fac[0]) and torch.equal(off[1], fac[1]), key
        clean_env.delenv(key)
    assert model.scene().density_dense                                            # back on: the choice follows the switch
    tr = model.scene(training=True)
    assert not tr.density_dense and not tr.density_coarse_dense                   # a training scene never bakes
    assert torch.equal(_render(model, rays, kw)[0], got[0])


def test_eval_render_follows_an_in_place_change_of_a_density_table(clean_env):
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    w = synth.make_weights(cfg, seed=7)
    model = make_model(cfg, w, DEV)
    rays = torch.from_numpy(synth.make_rays(64, seed=21)).to(DEV)
    before = [_render(model, rays, kw) for kw in KWS]
    grid_at = model.scene().density_dense
    with torch.no_grad():
        model.density_plane_yin[0].add_(0.25)
        model.density_line_yang[2].add_(-0.125)
    changed = dict(w)
    changed["density_plane_yin.0"] = w["density_plane_yin.0"] + np.float32(0.25)
    changed["density_line_yang.2"] = w["density_line_yang.2"] + np.float32(-0.125)
    fresh = make_model(cfg, changed, DEV)
    after, want = _render(model, rays, KWS[0]), _render(fresh, rays, KWS[0])
    assert model.scene().density_dense == grid_at                                  # the same buffer, baked again
    assert torch.equal(after[0], want[0]) and torch.equal(after[1], want[1])
    assert float((after[0] - before[0][0]).abs().max()) > 1e-3                     # the change is visible at all
    # the pooled tables are a snapshot of their own (EgoNeRF.py:124-133): refreshed, their grid is baked again too
    model.update_coarse_sigma_grid()
    after, want = _render(model, rays, KWS[1]), _render(fresh, rays, KWS[1])
    assert torch.equal(after[0], want[0]) and torch.equal(after[1], want[1])
    assert float((after[0] - before[1][0]).abs().max()) > 1e-3


def test_pooled_grid_follows_a_replayed_training_graph(clean_env):
    """A GraphedTrainStep with resampling refreshes the pooled tables INSIDE its graph: a replay rewrites them through raw pointers
    with no Python in between.  An eval render after further replays must march the pooled field as it then is: bit for bit the render
    of freshly baked grids, and the factored route's render to rounding (the two routes differ by fp32 rounding of sigma; an Adam step
    at lr 0.02 moves the image by more than 1e-3)."""
    from egonerf_amd.model import _SceneEntry
    from egonerf_amd.optim import FusedAdam
    from egonerf_amd.train import GraphedTrainStep
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    model = make_model(cfg, synth.make_weights(cfg, seed=3), DEV)
    model.train()
    N, kw = 192, dict(n_coarse=16, n_fine=16, exp_sampling=True, resampling=True, use_coarse_sample=True)
    batch = lambda i: (torch.from_numpy(synth.make_rays(N, seed=40 + i)).to(DEV),
                       torch.from_numpy(synth.hash_uniform(70 + i, 0, N * 3).reshape(N, 3).astype(np.float32)).to(DEV))
    opt = FusedAdam(model.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), capturable=True, lr_factor=0.9)
    step = GraphedTrainStep(model, opt, *batch(0), kw, warmup=1)
    step(*batch(1))
    rays = torch.from_numpy(synth.make_rays(64, seed=21)).to(DEV)
    model.eval()
    first = _render(model, rays, KWS[1])
    grids = (model.scene().density_dense, model.scene().density_coarse_dense)
    assert all(grids)
    model.train()
    for i in (2, 3, 4):
        step(*batch(i))
    model.eval()
    got = _render(model, rays, KWS[1])
    assert (model.scene().density_dense, model.scene().density_coarse_dense) == grids      # the same buffers, baked again
    assert float((got[0] - first[0]).abs().max()) > 1e-3                                    # the replays moved the field visibly
    model._scene = _SceneEntry()                                                            # nothing carried over: both grids baked anew
    fresh = _render(model, rays, KWS[1])
    assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
    model.dense_density = False
    fac = _render(model, rays, KWS[1])
    assert not model.scene().density_dense
    print("after replays: dense against factored rgb", maxerr(got[0], fac[0]), "depth", maxerr(got[1], fac[1]))
    assert maxerr(got[0], fac[0]) <= 2e-5 and maxerr(got[1], fac[1]) <= 2e-4


def test_baked_grids_outlive_the_structs_that_stop_using_them(clean_env):
    """An inference struct handed out earlier (or a captured graph) may still point into the grids: a training struct, the switch or
    the cap must not release them; the route comes back into the same buffers."""
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    model = make_model(cfg, synth.make_weights(cfg, seed=7), DEV)
    rays = torch.from_numpy(synth.make_rays(64, seed=21)).to(DEV)
    old = _lib.Scene.from_buffer_copy(model.scene())
    buffers = {k: v[1] for k, v in model._scene.dense.items()}
    assert old.density_dense == buffers["full"].data_ptr() and old.density_coarse_dense == buffers["coarse"].data_ptr()
    want = _render(model, rays, KWS[1])
    model.scene(training=True)
    assert {k: v[1].data_ptr() for k, v in model._scene.dense.items()} == {k: b.data_ptr() for k, b in buffers.items()}
    clean_env.setenv("EGO_DENSE_DENSITY", "0")
    assert not model.scene().density_dense and model._scene.dense["full"][1] is buffers["full"]
    clean_env.delenv("EGO_DENSE_DENSITY")
    clean_env.setenv("EGO_DENSE_DENSITY_MAX_MB", "0")
    assert not model.scene().density_dense and model._scene.dense["coarse"][1] is buffers["coarse"]
    clean_env.setenv("EGO_DENSE_DENSITY_MAX_MB", "lots")
    with pytest.raises(ValueError, match="EGO_DENSE_DENSITY_MAX_MB"):
        model.scene()
    clean_env.delenv("EGO_DENSE_DENSITY_MAX_MB")
    sc = model.scene()
    assert (sc.density_dense, sc.density_coarse_dense) == (old.density_dense, old.density_coarse_dense)
    got = _render(model, rays, KWS[1])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
