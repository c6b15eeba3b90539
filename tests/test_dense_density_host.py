"""The dense density route without a GPU: the identity it rests on (the factored VM feature of one lookup is the trilinear interpolation
of a node grid of channel-summed products, zero padding included) in float64, the ABI additions, and the scene key's part in it."""
import ctypes

import numpy as np
import torch

from egonerf_amd import _lib, synth
from tests import dense_density_ref as ref
from tests.helpers import make_model

RES = [5, 6, 7]


def test_factored_feature_is_the_trilinear_interpolation_of_the_baked_grid():
    tables = ref.random_tables(RES, seed=3)
    G, A = ref.bake(tables, RES)
    assert G.shape == (2, 7, 6, 5, 4) and not G[..., 3].any() and (A >= np.abs(G[..., :3])).all()
    pts, yang = ref.probe_points(RES, seed=4)
    want = ref.factored_feature(tables, RES, pts, yang)
    got = ref.dense_feature(G, RES, pts, yang)
    assert float(np.abs(want).max()) > 0.5 and (want > 0).mean() > 0.5          # a real signal, most points past a ReLU
    outside = (np.abs(pts) > 1).any(-1)
    assert outside.sum() >= 100 and float(np.abs(want[outside]).max()) > 0.05   # partly padded points still see the inner taps
    assert float(np.abs(got - want).max()) <= 1e-13
    # one grid for the SUM over lookups would not do: the ReLU is per lookup
    summed = np.maximum(ref.dense_feature(G.sum(-1, keepdims=True).repeat(4, -1) / 3.0, RES, pts, yang), 0.0)
    assert float(np.abs(summed - want).max()) > 0.1


def test_reference_of_the_factored_formula_agrees_with_the_oracle():
    from oracle.egonerf_oracle import OracleScene
    tables = ref.random_tables(RES, seed=5)
    names = [f"density_{what}_{g}.{i}" for g in ("yin", "yang") for what in ("plane", "line") for i in range(3)]
    oracle = OracleScene(synth.SceneConfig(grid=list(RES)), dict(zip(names, tables)), dtype=torch.float64)
    pts, yang = ref.probe_points(RES, seed=6)
    c7n = np.zeros((pts.shape[0], 7))
    c7n[yang == 0, 0:3] = pts[yang == 0]
    c7n[yang == 1, 3:6] = pts[yang == 1]
    c7n[:, 6] = yang
    want = oracle.density_feature(torch.from_numpy(c7n)).numpy()
    assert float(np.abs(ref.factored_feature(tables, RES, pts, yang) - want).max()) <= 1e-12


def test_abi_additions_and_argument_checks_need_no_gpu():
    lib = _lib.load()
    fields = [n for n, _t in _lib.Scene._fields_]
    assert fields[-2:] == ["density_dense", "density_coarse_dense"] and lib.ego_abi_version() == 17
    assert lib.ego_sizeof(0) == ctypes.sizeof(_lib.Scene)
    sc = _lib.new_scene()
    assert not sc.density_dense and not sc.density_coarse_dense          # NULL = off
    f = _lib.VmField()
    assert lib.ego_bake_density_dense(None, None, None) == -1
    assert lib.ego_bake_density_dense(ctypes.byref(f), 256, None) == -1 and b"null" in lib.ego_last_error()   # no tables


def test_scene_key_follows_the_dense_switch_and_the_density_tables(monkeypatch):
    monkeypatch.delenv("EGO_DENSE_DENSITY", raising=False)
    monkeypatch.delenv("EGO_DENSE_DENSITY_MAX_MB", raising=False)
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    model = make_model(cfg, synth.make_weights(cfg, seed=1), "cpu")
    assert model.dense_density is True and model._dense_wanted()
    k0, t0 = model._scene_key(False), model._scene_key(True)
    with torch.no_grad():
        model.density_line_yang[1].add_(0.0)
    k1 = model._scene_key(False)
    assert k1 != k0 and model._scene_key(True) == t0      # an in-place write re-bakes the eval scene; a training scene never bakes
    monkeypatch.setenv("EGO_DENSE_DENSITY_MAX_MB", "0")
    k2 = model._scene_key(False)
    assert k2 not in (k0, k1)
    monkeypatch.setenv("EGO_DENSE_DENSITY", "0")
    k3 = model._scene_key(False)
    assert not model._dense_wanted() and k3 not in (k0, k1, k2)
    with torch.no_grad():
        model.density_line_yang[1].add_(0.0)
    assert model._scene_key(False) == k3                  # route off: the tables are read through their pointers again
    monkeypatch.setenv("EGO_DENSE_DENSITY", "1")
    model.dense_density = False
    assert model._dense_wanted()                          # the environment overrides the attribute, either way
    monkeypatch.delenv("EGO_DENSE_DENSITY")
    assert not model._dense_wanted() and model._scene_key(False) == k3
    other = synth.SceneConfig(n_voxel=20 ** 3, density_n_comp=(8, 8, 8))
    assert not make_model(other, synth.make_weights(other, seed=1), "cpu")._dense_wanted()   # the dense march is the 16-component one
    other = synth.SceneConfig(n_voxel=20 ** 3, featureC=64)
    assert not make_model(other, synth.make_weights(other, seed=1), "cpu")._dense_wanted()   # ... of the tuned shape
