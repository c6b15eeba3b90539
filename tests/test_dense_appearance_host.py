"""The dense appearance route without a device: the identity it rests on (trilinear interpolation of the baked feature grid = the
factored formula) against the float64 oracle, the node layout, and the switch / gate logic of the model."""
import os

import numpy as np
import pytest
import torch

from egonerf_amd import synth
from egonerf_amd.model import EgoNeRF
from tests import dense_appearance_ref as ref
from tests.helpers import make_model, make_oracle

FIELD = ("plane_yin", "line_yin", "plane_yang", "line_yang")


def _tables_of(w):
    return [w[f"app_{name}.{i}"] for name in FIELD for i in range(3)]


def _points(res, seed):
    """On nodes (all three axes at once, and one axis at a time), on the faces +-1, beyond +1 (one and both taps out of range), the
    box corners, and random points inside; both grids alternate."""
    rng = np.random.default_rng(seed)
    node = lambda a, k: 2.0 * k / (res[a] - 1) - 1.0
    on_nodes = np.array([[node(a, rng.integers(0, res[a])) for a in range(3)] for _ in range(60)])
    one_axis = rng.uniform(-1, 1, (60, 3))
    for k in range(60):
        one_axis[k, k % 3] = node(k % 3, rng.integers(0, res[k % 3]))
    faces = rng.uniform(-1, 1, (60, 3))
    for k in range(60):
        faces[k, k % 3] = 1.0 if (k // 3) % 2 else -1.0
    beyond = rng.uniform(-1, 1, (90, 3))
    for k in range(90):
        a = k % 3
        step = 2.0 / (res[a] - 1)
        beyond[k, a] = 1.0 + [0.3, 0.999, 1.6][(k // 3) % 3] * step
    corners = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    pts = np.concatenate([on_nodes, one_axis, faces, beyond, corners, rng.uniform(-1, 1, (300, 3))])
    return pts, np.arange(pts.shape[0]) % 2


def test_trilinear_of_the_baked_grid_is_the_factored_feature():
    cfg = synth.SceneConfig(grid=[10, 12, 34])
    assert len(set(cfg.grid)) == 3
    w = synth.make_weights(cfg, seed=5)
    tables, basis = _tables_of(w), [w["basis_mat_yin.weight"], w["basis_mat_yang.weight"]]
    F, _A = ref.bake(tables, basis, cfg.grid)
    pts, yang = _points(cfg.grid, seed=6)
    assert (pts > 1.0).any(1).sum() >= 90 and set(yang.tolist()) == {0, 1}
    dense = ref.dense_feature(F, cfg.grid, pts, yang)
    oracle = make_oracle(cfg, w, dtype=torch.float64)
    want = oracle.app_feature(torch.from_numpy(_c7n64(pts, yang))).numpy()
    err = float(np.abs(dense - want).max())
    print("max |trilinear(baked) - oracle.app_feature| =", err, "feature scale", float(np.abs(want).max()))
    assert float(np.abs(want).max()) > 0.05 and err <= 1e-12
    # ... and the restatement's own factored formula is the oracle's
    assert float(np.abs(ref.factored_feature(tables, basis, cfg.grid, pts, yang) - want).max()) <= 1e-12


def _c7n64(pts, yang):
    y = np.asarray(yang, np.float64)[:, None]
    return np.concatenate([pts * (1 - y), pts * y, y], -1)


def test_node_layout_round_trip():
    assert len(set(ref.FEATURE_FLOATS.tolist())) == 27 and len(ref.PAD_FLOATS) == 5
    feat = np.arange(1, 28, dtype=np.float32)
    node = ref.pack_nodes(feat)
    assert np.array_equal(ref.unpack_nodes(node), feat) and not node[ref.PAD_FLOATS].any()
    # quad 2 q + h holds slots 4 q .. 4 q + 3 of half h; slot s of half h is feature 2 s + h
    for h in range(2):
        for s in range(16):
            v = node[(2 * (s // 4) + h) * 4 + s % 4]
            assert v == (2 * s + h + 1 if 2 * s + h < 27 else 0)
    # a lane half's 14 slots are bytes [32 q + 16 h, + 16) of the node for q = 0..2 and the first 8 bytes of quad 3's piece
    assert [ref.node_float(f) for f in (0, 1, 2, 8, 9, 24, 25, 26)] == [0, 4, 1, 8, 12, 24, 28, 25]


def test_size_gates():
    fits = EgoNeRF._app_dense_fits
    gib = 2 ** 30
    headline = 2 * 128 * 150 * 172 * 516
    assert headline < 2 ** 32 and fits(headline, 4096 * 2 ** 20, headline, 64 * gib)
    assert not fits(headline, 1024 * 2 ** 20, headline, 64 * gib)            # over the cap
    assert not fits(headline, 4096 * 2 ** 20, headline, 4 * headline - 4)     # more than a quarter of the free memory
    assert fits(headline, 4096 * 2 ** 20, 0, 0)                               # a held buffer needs no free memory
    assert not fits(2 ** 32, 8192 * 2 ** 20, 0, 0)                            # 32-bit byte offsets end at 4 GiB
    assert not fits(2 * 128 * 300 * 346 * 1036, 1e12, 0, 0)                   # the 216e6-voxel grid: 27.5 GB


def test_cap_comes_from_the_environment(monkeypatch):
    monkeypatch.delenv("EGO_DENSE_APP_MAX_MB", raising=False)
    assert EgoNeRF._app_dense_cap_bytes() == 4096 * 2 ** 20
    monkeypatch.setenv("EGO_DENSE_APP_MAX_MB", "0.5")
    assert EgoNeRF._app_dense_cap_bytes() == 2 ** 19
    monkeypatch.setenv("EGO_DENSE_APP_MAX_MB", "plenty")
    with pytest.raises(ValueError, match="EGO_DENSE_APP_MAX_MB"):
        EgoNeRF._app_dense_cap_bytes()


def test_switches(monkeypatch):
    monkeypatch.delenv("EGO_DENSE_APP", raising=False)
    cfg = synth.SceneConfig(n_voxel=12 ** 3)
    model = make_model(cfg, synth.make_weights(cfg, seed=3), "cpu")
    assert model.dense_appearance and model._app_dense_wanted()
    model.dense_appearance = False
    assert not model._app_dense_wanted()
    monkeypatch.setenv("EGO_DENSE_APP", "1")
    assert model._app_dense_wanted()                      # the environment overrides the attribute, both ways
    model.dense_appearance = True
    monkeypatch.setenv("EGO_DENSE_APP", "0")
    assert not model._app_dense_wanted()
    monkeypatch.delenv("EGO_DENSE_APP")
    model.app_table_dtype = "f16"                         # half tables keep the factored gather ...
    assert not model._app_dense_wanted()
    model.app_table_dtype = "f32"
    assert model._app_dense_wanted()
    for prec, want in (("f32", False), ("f16x3", True), ("f16f8", True), ("f16f6", True)):   # ... and so does the fp32-MFMA kernel
        model.mlp_precision = prec
        assert model._app_dense_wanted() == want, prec
    # the snapshot key: the twelve appearance tables and both basis matrices, by (address, version)
    ver = model._app_dense_versions()
    assert len(ver) == 14
    with torch.no_grad():
        model.basis_mat_yang.weight.mul_(1.5)
    changed = model._app_dense_versions()
    assert changed[:13] == ver[:13] and changed[13] != ver[13]
    with torch.no_grad():
        model.app_line_yin[1].add_(0.1)
    moved = [a != b for a, b in zip(model._app_dense_versions(), changed)]   # (tables carved from one buffer share a version counter)
    assert moved[4] and not moved[12] and not moved[13]
    assert model._scene_key(False) != model._scene_key(True)


def test_abi_addition_and_argument_checks_need_no_gpu():
    import ctypes
    from egonerf_amd import _lib
    lib = _lib.load()
    # no member was added to ego_scene: the grid travels as app_f16 = EGO_APP_DENSE + app16.plane[0][0], so sizes and the version stand
    assert "app_dense" not in [n for n, _t in _lib.Scene._fields_] and lib.ego_abi_version() == 17
    assert lib.ego_sizeof(0) == ctypes.sizeof(_lib.Scene)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egonerf_hip.h")).read()
    assert "#define EGO_APP_DENSE 2" in hdr and (_lib.APP_TABLES, _lib.APP_HALF, _lib.APP_DENSE) == (0, 1, 2)
    sc = _lib.new_scene()
    assert sc.app_dense is None and sc.app_f16 == 0                           # off
    sc.app.n_comp = 48
    sc.app.res[:] = [5, 6, 7]
    sc.app_dense = 4096
    assert sc.app_dense == 4096 and sc.app_f16 == 2 and sc.app16.plane[0][0] == 4096 and list(sc.app16.res) == [5, 6, 7] and sc.app16.n_comp == 48
    copy = _lib.Scene.from_buffer_copy(sc)
    copy.app_dense = None
    assert copy.app_dense is None and copy.app_f16 == 0 and not copy.app16.plane[0][0] and sc.app_dense == 4096
    half = _lib.new_scene()
    half.app_f16, half.app16.plane[0][0] = 1, 8192                            # half tables are not the grid, and clearing the grid leaves them
    half.app_dense = None
    assert half.app_dense is None and half.app_f16 == 1 and half.app16.plane[0][0] == 8192
    assert "ego_bake_app_dense" in _lib.header_symbols()
    f = _lib.VmField()
    assert lib.ego_bake_app_dense(None, None, None, 27, None, None) == -1
    f.n_comp = 16
    assert lib.ego_bake_app_dense(ctypes.byref(f), 256, 256, 27, 256, None) == -2 and b"n_comp" in lib.ego_last_error()
    f.n_comp = 48
    assert lib.ego_bake_app_dense(ctypes.byref(f), 256, 256, 26, 256, None) == -2 and b"app_dim" in lib.ego_last_error()
    f.res[:] = [256, 256, 256]                                               # 2 x 128 B x 2^24 nodes = 4 GiB: from the resolutions alone
    assert lib.ego_bake_app_dense(ctypes.byref(f), 256, 256, 27, 256, None) == -1 and b"4 GB" in lib.ego_last_error()
    f.res[:] = [5, 6, 7]
    assert lib.ego_bake_app_dense(ctypes.byref(f), 256, 256, 27, 260, None) == -1 and b"aligned" in lib.ego_last_error()
    assert lib.ego_bake_app_dense(ctypes.byref(f), 256, 256, 27, 256, None) == -1 and b"null" in lib.ego_last_error()   # no tables
