"""The dense appearance route on the device: the bake kernel against its float64 restatement, the features through ego_app_feature on
one scene (pointer set / cleared) against the float64 oracle, eval renders in the plain, folded and compact forms and the three split
arithmetics with the route on and off, the snapshot rules of the baked grid, and the repeatability of the folded dense kernel."""
import ctypes
import os

import numpy as np
import pytest
import torch

from egonerf_amd import _lib, field_tables, synth
from egonerf_amd.model import YinYangAlphaGridMask
from tests import dense_appearance_ref as ref
from tests.dense_density_ref import random_tables
from tests.helpers import make_model, make_oracle, maxerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
RGB_TOL = 1e-4            # tests/test_hip_parity.py
FAR = 15.0
DEPTH_TOL = 1e-3 * FAR    # ... its depth bar for the far = 15 scenes
FEATURE_TOL = 2e-5        # the appearance features against float64
PRECISIONS = ("f16x3", "f16f8", "f16f6")
ENV_KEYS = ("EGO_DENSE_APP", "EGO_DENSE_APP_MAX_MB", "EGO_RENDER_FOLD", "EGO_RENDER_COMPACT")


@pytest.fixture()
def clean_env(monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


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


def test_bake_kernel_against_float64():
    res = [5, 6, 7]
    tables, basis = random_tables(res, seed=21, n_comp=48), ref.random_basis(seed=22)
    f, _keep = _device_field(tables, res)
    bd = [torch.from_numpy(b).to(DEV) for b in basis]
    out = torch.full((2, res[2], res[1], res[0], 32), float("nan"), device=DEV)
    _lib.check(_lib.load().ego_bake_app_dense(ctypes.byref(f), bd[0].data_ptr(), bd[1].data_ptr(), 27, out.data_ptr(), _lib.stream_handle()), "bake")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    F, A = ref.bake(tables, basis, res)
    assert np.array_equal(got[..., ref.PAD_FLOATS], np.zeros_like(got[..., ref.PAD_FLOATS]))   # exactly 0, not -0 or NaN
    assert not np.signbit(got[..., ref.PAD_FLOATS]).any()
    feat = ref.unpack_nodes(got).astype(np.float64)
    # one float32 rounding of the value + the float64 running error of the chain (the restatement counts K_BAKE)
    half_ulp = 0.5 * np.spacing(np.maximum(np.abs(feat), np.abs(F)).astype(np.float32)).astype(np.float64)
    err, bound = np.abs(feat - F), half_ulp + ref.gamma(ref.K_BAKE) * A
    print("bake", res, "max err", float(err.max()), "max err / bound", float((err / bound).max()), "max |F|", float(np.abs(F).max()))
    assert (err <= bound).all()
    assert float(np.abs(F).max()) > 1.0 and len({float(F[g, 1, 2, 3, k]) for g in range(2) for k in range(27)}) == 54


def test_bake_refusals():
    res = [5, 6, 7]
    lib = _lib.load()
    bd = [torch.from_numpy(b).to(DEV) for b in ref.random_basis(seed=23)]
    out = torch.zeros(2 * 5 * 6 * 7 * 32 + 4, device=DEV)
    f16, _k16 = _device_field(random_tables(res, seed=24, n_comp=16), res)
    assert lib.ego_bake_app_dense(ctypes.byref(f16), bd[0].data_ptr(), bd[1].data_ptr(), 27, out.data_ptr(), None) == -2
    assert b"n_comp" in lib.ego_last_error()
    f, _k = _device_field(random_tables(res, seed=24, n_comp=48), res)
    assert lib.ego_bake_app_dense(ctypes.byref(f), bd[0].data_ptr(), bd[1].data_ptr(), 3, out.data_ptr(), None) == -2
    assert b"app_dim" in lib.ego_last_error()
    assert lib.ego_bake_app_dense(ctypes.byref(f), bd[0].data_ptr(), bd[1].data_ptr(), 27, out.data_ptr() + 4, None) == -1
    assert b"aligned" in lib.ego_last_error()
    # 4 GiB: decided from the resolutions alone, before anything is read or launched (2 x 128 B x 16 777 216 nodes = 2^32)
    for big, refused in (([256, 256, 256], True), ([300, 346, 1036], True)):
        f.res[:] = big
        assert (lib.ego_bake_app_dense(ctypes.byref(f), bd[0].data_ptr(), bd[1].data_ptr(), 27, out.data_ptr(), None) == -1) == refused
        assert b"4 GB" in lib.ego_last_error()
    out[:] = 0   # nothing was launched: the buffer is still addressable and untouched
    torch.cuda.synchronize()


# ---- one masked scene for features and renders ----------------------------------------------------------------------------------------
N_RAYS = 5   # the last workgroup is ragged


def _rays():
    rays = synth.make_rays(N_RAYS, seed=5)
    rays[3:, 3:6] *= 2.0   # twice the reach: these rays leave the radius LUT's last knot behind (normalised r > 1: zero-padded taps)
    return torch.from_numpy(rays)


@pytest.fixture(scope="module")
def scene():
    cfg = synth.SceneConfig(n_voxel=20 ** 3, density_shift=-8.0)
    assert cfg.far == FAR
    w = synth.make_weights(cfg, seed=7)
    model = make_model(cfg, w, DEV)
    n_r, n_th, n_ph = cfg.grid
    vol = torch.ones(2, 1, 1, n_ph, n_th, n_r)
    vol[..., (3 * n_r) // 10:(5 * n_r) // 10] = 0.0   # an empty slab of shells inside every ray
    vol[1, :, :, : n_ph // 3] = 0.0                    # ... and a wedge of the yang grid
    model.alphaMask = YinYangAlphaGridMask(DEV, vol[0].to(DEV), vol[1].to(DEV))
    model.use_alpha_mask = True
    oracle = make_oracle(cfg, w, dtype=torch.float64)
    oracle.alpha_mask = (vol[0].double(), vol[1].double())
    return cfg, w, model, oracle


def _two_routes(model):
    """The model's inference scene with the baked feature grid, and a copy of the same struct with the pointer cleared."""
    dense = model.scene()
    assert dense.app_dense
    tables = _lib.Scene.from_buffer_copy(dense)
    tables.app_dense = None
    return dense, tables


def _feature_points(res):
    """257 normalised points: on nodes, on the faces +-1, beyond +1 (one and both taps of an axis out of range) and inside; the grid
    flag alternates, so every 32-sample tile holds both grids."""
    rng = np.random.default_rng(31)
    node = lambda a, k: 2.0 * k / (res[a] - 1) - 1.0
    pts = rng.uniform(-1.0, 1.0, (257, 3))
    for k in range(0, 60):
        pts[k, k % 3] = node(k % 3, rng.integers(0, res[k % 3]))
    for k in range(60, 80):
        pts[k] = [node(a, rng.integers(0, res[a])) for a in range(3)]
    for k in range(80, 130):
        pts[k, k % 3] = 1.0 if (k // 3) % 2 else -1.0
    for k in range(130, 190):
        a = k % 3
        pts[k, a] = 1.0 + [0.3, 0.999, 1.6][(k // 3) % 3] * 2.0 / (res[a] - 1)
    return pts.astype(np.float32), np.arange(257) % 2


def test_features_against_the_factored_formula(scene, clean_env):
    cfg, _w, model, oracle = scene
    model.mlp_precision = "f16x3"
    sc_d, sc_t = _two_routes(model)
    pts, yang = _feature_points(cfg.grid)
    c7n = torch.from_numpy(ref.c7n_of(pts, yang))
    want = oracle.app_feature(c7n.double()).numpy()
    dev_c = c7n.to(DEV)
    got = {}
    for name, sc in (("dense", sc_d), ("tables", sc_t)):
        out = torch.full((257, 27), float("nan"), device=DEV)
        _lib.check(_lib.load().ego_app_feature(sc, dev_c.data_ptr(), 257, out.data_ptr(), _lib.stream_handle()), name)
        torch.cuda.synchronize()
        got[name] = out.cpu().numpy().astype(np.float64)
    err_d, err_t = float(np.abs(got["dense"] - want).max()), float(np.abs(got["tables"] - want).max())
    print(f"features: dense err {err_d:.3e} tables err {err_t:.3e} ratio {err_d / max(err_t, 1e-300):.2f} scale {float(np.abs(want).max()):.3f}")
    assert float(np.abs(want).max()) > 0.05 and (pts > 1.0).any(1).sum() >= 60
    assert err_d <= FEATURE_TOL and err_t <= FEATURE_TOL
    assert err_d <= 2.0 * err_t


FORMS = {"plain": dict(EGO_RENDER_FOLD="0", EGO_RENDER_COMPACT="0"), "fold": dict(EGO_RENDER_FOLD="1", EGO_RENDER_COMPACT="0"),
         "compact": dict(EGO_RENDER_FOLD="0", EGO_RENDER_COMPACT="1")}


def _render(model, rays, S, env, form):
    for k, v in FORMS[form].items():
        env.setenv(k, v)
    sc, lib, N = model.scene(), _lib.load(), rays.shape[0]
    assert bool(lib.ego_render_forward_folds(sc, N, S)) == (form == "fold")
    assert bool(lib.ego_render_forward_compacts(sc, N, S)) == (form == "compact")
    with torch.no_grad():
        out = model(rays, exp_sampling=True, n_coarse=S)
    torch.cuda.synchronize()
    return out[0].clone(), out[1].clone()


_ORACLE_RENDERS = {}


@pytest.mark.parametrize("S", [32, 96, 77])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_renders_in_every_form(scene, clean_env, prec, S):
    """With the route on, the plain, folded and compact forms return the same bits (what tests/test_hip_compact_shading.py and
    tests/test_hip_march_split.py assert of the table route); against the float64 oracle the route's colour error is at most twice
    the table route's on the same rays, and both stay within the project's bars."""
    cfg, _w, model, oracle = scene
    rays = _rays()
    if S not in _ORACLE_RENDERS:
        o = oracle.forward(rays.double(), n_coarse=S)
        _ORACLE_RENDERS[S] = (o[0].numpy(), o[1].numpy())
    want = _ORACLE_RENDERS[S]
    rays = rays.to(DEV)
    model.mlp_precision = prec
    forms = ("plain", "fold", "compact") if S % 32 == 0 else ("plain",)
    out = {}
    for route in (True, False):
        model.dense_appearance = route
        assert bool(model.scene().app_dense) == route
        for form in forms:
            out[route, form] = _render(model, rays, S, clean_env, form)
    model.dense_appearance = True
    for route in (True, False):
        for form in forms[1:]:
            assert torch.equal(out[route, form][0], out[route, "plain"][0]) and torch.equal(out[route, form][1], out[route, "plain"][1]), (route, form)
    err = {route: (maxerr(out[route, "plain"][0], want[0]), maxerr(out[route, "plain"][1], want[1])) for route in (True, False)}
    print(f"render {prec} S={S}: dense rgb err {err[True][0]:.3e} depth {err[True][1]:.3e}; tables rgb err {err[False][0]:.3e} depth {err[False][1]:.3e}")
    assert float(np.abs(want[0]).max()) > 0.05
    for route in (True, False):
        assert err[route][0] <= RGB_TOL and err[route][1] <= DEPTH_TOL, route
    assert err[True][0] <= 2.0 * err[False][0]


# ---- snapshot rules ---------------------------------------------------------------------------------------------------------------------
KW = dict(n_coarse=64)


def _forward(model, rays):
    with torch.no_grad():
        out = model(rays, exp_sampling=True, **KW)
    return out[0].clone(), out[1].clone()


def test_grid_follows_in_place_changes_of_tables_and_basis(clean_env):
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    w = synth.make_weights(cfg, seed=7)
    model = make_model(cfg, w, DEV)
    rays = torch.from_numpy(synth.make_rays(64, seed=21)).to(DEV)
    before = _forward(model, rays)
    grid_at = model.scene().app_dense
    assert grid_at and model.last_app_bake_ms is not None and model.last_app_bake_ms > 0.0
    changed = dict(w)
    for step, (name, key, delta) in enumerate((("app_plane_yang", "app_plane_yang.1", 0.25), ("basis_mat_yin", "basis_mat_yin.weight", 0.125))):
        with torch.no_grad():
            (getattr(model, name)[1] if step == 0 else getattr(model, name).weight).add_(delta)
        changed[key] = changed[key] + np.float32(delta)
        fresh = make_model(cfg, changed, DEV)
        after, want = _forward(model, rays), _forward(fresh, rays)
        assert model.scene().app_dense == grid_at                                    # the same buffer, baked again
        assert torch.equal(after[0], want[0]) and torch.equal(after[1], want[1]), name
        assert float((after[0] - before[0]).abs().max()) > 1e-3, name                # the change is visible at all
        before = after


def test_switch_cap_and_training_scene(clean_env):
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    w = synth.make_weights(cfg, seed=7)
    model, plain = make_model(cfg, w, DEV), make_model(cfg, w, DEV)
    plain.dense_appearance = False
    rays = torch.from_numpy(synth.make_rays(64, seed=21)).to(DEV)
    got, tab = _forward(model, rays), _forward(plain, rays)
    assert model.scene().app_dense and not plain.scene().app_dense
    assert not model.scene(training=True).app_dense                                  # a training scene never carries the grid
    for key, value in (("EGO_DENSE_APP", "0"), ("EGO_DENSE_APP_MAX_MB", "0")):
        clean_env.setenv(key, value)
        off = _forward(model, rays)
        assert not model.scene().app_dense, key
        assert torch.equal(off[0], tab[0]) and torch.equal(off[1], tab[1]), key      # the bits of a model built with the route off
        clean_env.delenv(key)
    for attr, value, back in (("app_table_dtype", "f16", "f32"), ("mlp_precision", "f32", "f16f6")):
        setattr(model, attr, value)
        assert not model.scene().app_dense, attr                                      # half tables / the fp32 kernel keep the tables
        setattr(model, attr, back)
    assert model.scene().app_dense
    again = _forward(model, rays)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_grid_outlives_the_structs_that_stop_using_it(clean_env):
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    model = make_model(cfg, synth.make_weights(cfg, seed=7), DEV)
    rays = torch.from_numpy(synth.make_rays(64, seed=21)).to(DEV)
    old = _lib.Scene.from_buffer_copy(model.scene())
    buf = model._scene.app_dense[1]
    assert old.app_dense == buf.data_ptr()
    want = _forward(model, rays)
    model.scene(training=True)
    assert model._scene.app_dense[1] is buf
    clean_env.setenv("EGO_DENSE_APP", "0")
    assert not model.scene().app_dense and model._scene.app_dense[1] is buf
    clean_env.delenv("EGO_DENSE_APP")
    model.app_table_dtype = "f16"
    assert not model.scene().app_dense and model._scene.app_dense[1] is buf
    model.app_table_dtype = "f32"
    assert model.scene().app_dense == old.app_dense                                   # back into the same buffer, nothing baked anew
    got = _forward(model, rays)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- repeatability ------------------------------------------------------------------------------------------------------------------------
def test_folded_dense_kernel_repeats_its_bits(clean_env):
    """200 launches of the folded dense kernel on 4096 rays x 32 samples (two waves on every SIMD) return the same bits."""
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    model = make_model(cfg, synth.make_weights(cfg, seed=7), DEV)
    rays = torch.from_numpy(synth.make_rays(4096, seed=33)).to(DEV)
    clean_env.setenv("EGO_RENDER_FOLD", "1")
    sc = model.scene()
    assert sc.app_dense and _lib.load().ego_render_forward_folds(sc, 4096, 32) == 1
    first = _forward_s(model, rays, 32)
    bad = torch.zeros((), device=DEV, dtype=torch.int64)
    for _ in range(200):
        out = _forward_s(model, rays, 32)
        bad += (out[0] != first[0]).any().long() + (out[1] != first[1]).any().long()
    assert int(bad) == 0 and float(first[0].std()) > 1e-3


def _forward_s(model, rays, S):
    with torch.no_grad():
        out = model(rays, exp_sampling=True, n_coarse=S)
    return out[0].clone(), out[1].clone()


def test_launch_refuses_a_grid_it_cannot_address(scene, clean_env):
    """EGO_APP_DENSE with no grid, a misaligned grid, or a grid baked at another resolution: refused before any launch."""
    _cfg, _w, model, _oracle = scene
    model.mlp_precision = "f16f6"
    sc_d, _sc_t = _two_routes(model)
    lib = _lib.load()
    c7n, out = torch.zeros(32, 7, device=DEV), torch.zeros(32, 27, device=DEV)
    call = lambda sc: lib.ego_app_feature(sc, c7n.data_ptr(), 32, out.data_ptr(), _lib.stream_handle())
    bad = _lib.Scene.from_buffer_copy(sc_d)
    bad.app16.plane[0][0] = None
    assert call(bad) == -1 and b"null" in lib.ego_last_error()
    bad = _lib.Scene.from_buffer_copy(sc_d)
    bad.app16.plane[0][0] = sc_d.app_dense + 4
    assert call(bad) == -1 and b"aligned" in lib.ego_last_error()
    bad = _lib.Scene.from_buffer_copy(sc_d)
    bad.app16.res[1] += 1
    assert call(bad) == -1 and b"resolution" in lib.ego_last_error()
    assert call(sc_d) == 0
    torch.cuda.synchronize()
