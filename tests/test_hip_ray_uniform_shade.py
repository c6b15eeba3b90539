"""The folded shade kernel makes what a ray's tiles share once per ray (the view encodings of its dense instances) and every shade form
finishes two colour channels per lane half instead of three.  Neither may change a bit: the folded, the plain and the compact form
return the same five outputs on rays whose neighbours point elsewhere (a value left over from the previous ray would show), on rays
whose first tiles, or all tiles, the tile mask skips, with and without an environment map, in the three split arithmetics and with
the baked feature grid on and off; one case per arithmetic is held to the float64 oracle as well."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth
from egonerf_amd.model import YinYangAlphaGridMask
from tests.helpers import make_model, make_oracle, maxerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
RGB_TOL = 1e-4            # tests/test_hip_dense_appearance.py (tests/test_hip_parity.py)
FAR = 15.0
DEPTH_TOL = 1e-3 * FAR    # ... its depth bar for the far = 15 scenes
PRECISIONS = ("f16x3", "f16f8", "f16f6")
ENV_KEYS = ("EGO_DENSE_APP", "EGO_DENSE_APP_MAX_MB", "EGO_RENDER_FOLD", "EGO_RENDER_COMPACT")
FORMS = {"fold": dict(EGO_RENDER_FOLD="1", EGO_RENDER_COMPACT="0"), "plain": dict(EGO_RENDER_FOLD="0", EGO_RENDER_COMPACT="0"),
         "compact": dict(EGO_RENDER_FOLD="0", EGO_RENDER_COMPACT="1")}
# one tile per ray and two; one ray (one wave of the grid has work), three (a wave's rays follow each other), 2049 (every wave of
# the 2048 owns a ray and the first one two: the values of the first ray must not reach the second)
SHAPES = [(S, N) for S in (32, 64) for N in (1, 3, 2049)]
# density_shift 0: surfaces hide what lies behind them, the weights of a ray's tail are exactly zero
FIELDS = {"default": dict(density_shift=-8.0), "opaque_masked": dict(density_shift=0.0)}


@pytest.fixture()
def clean_env(monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _rays(n):
    """Neighbours point in opposite directions, and every second ray reaches 1.5 times as far (its direction is no unit vector)."""
    r = synth.make_rays(n, seed=5)
    r[1::2, 3:6] = -r[0:2 * (n // 2):2, 3:6] * np.float32(1.5)
    return torch.from_numpy(r)


def _mask_volumes(cfg):
    """The inner half of the shells is empty (the first tile of many rays holds no weight) and so is a wedge of the yang grid at every
    radius (rays that hold none at all)."""
    n_r, n_th, n_ph = cfg.grid
    vol = torch.ones(2, 1, 1, n_ph, n_th, n_r)
    vol[..., : n_r // 2] = 0.0
    vol[1, :, :, : n_ph // 3] = 0.0
    return vol


_SCENES = {}


def _scene(field, envmap):
    if (field, envmap) not in _SCENES:
        kw = dict(use_envmap=True, envmap_res_H=16) if envmap else {}
        cfg = synth.SceneConfig(n_voxel=20 ** 3, **FIELDS[field], **kw)
        assert cfg.far == FAR
        w = synth.make_weights(cfg, seed=7)
        model = make_model(cfg, w, DEV)
        if field == "opaque_masked":
            vol = _mask_volumes(cfg)
            model.alphaMask = YinYangAlphaGridMask(DEV, vol[0].to(DEV), vol[1].to(DEV))
            model.use_alpha_mask = True
        _SCENES[field, envmap] = (cfg, w, model)
    return _SCENES[field, envmap]


_ORACLE = {}


def _oracle_render(field, S, N):
    """float64 oracle of the scene without an environment map: computed once per (field, shape), never changed"""
    if (field, S, N) not in _ORACLE:
        cfg, w, _model = _scene(field, False)
        oracle = make_oracle(cfg, w, dtype=torch.float64)
        if field == "opaque_masked":
            vol = _mask_volumes(cfg)
            oracle.alpha_mask = (vol[0].double(), vol[1].double())
        o = oracle.forward(_rays(N).double(), n_coarse=S)
        _ORACLE[field, S, N] = (o[0].numpy(), o[1].numpy())
    return _ORACLE[field, S, N]


def _render(model, rays, S, env, form):
    for k, v in FORMS[form].items():
        env.setenv(k, v)
    sc, lib, N = model.scene(), _lib.load(), rays.shape[0]
    assert bool(lib.ego_render_forward_folds(sc, N, S)) == (form == "fold"), form
    assert bool(lib.ego_render_forward_compacts(sc, N, S)) == (form == "compact"), form
    with torch.no_grad():
        out = model(rays, exp_sampling=True, n_coarse=S)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.clone() for t in out)


def _skipped_tiles(alpha):
    """From a 64-sample render's alpha: rays whose first tile is empty and whose second is not, rays that are empty, and rays that
    are opaque before their second tile (so that its weights are exactly zero)."""
    a = alpha[:, :64].double().cpu()
    first = ((a[:, :32] == 0).all(1) & (a[:, 32:] > 0).any(1)).sum()
    empty = (a == 0).all(1).sum()
    tail = (((1.0 - a[:, :32].float()).prod(1) == 0) & (a[:, :32] > 0).any(1)).sum()
    return int(first), int(empty), int(tail)


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("envmap", [False, True])
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_forms_return_the_same_bits(clean_env, field, envmap, prec, dense):
    _cfg, _w, model = _scene(field, envmap)
    model.mlp_precision = prec
    model.dense_appearance = dense
    try:
        assert bool(model.scene().app_dense) == dense
        for S, N in SHAPES:
            rays = _rays(N).to(DEV)
            out = {form: _render(model, rays, S, clean_env, form) for form in FORMS}
            assert len(out["fold"]) == 5
            for form in ("plain", "compact"):
                for k in range(5):
                    a, b = out["fold"][k], out[form][k]
                    assert (a is None) == (b is None), (S, N, form, k)
                    if a is not None:
                        assert torch.equal(a, b), (S, N, form, k, float((a - b).abs().max()))
            rgb, depth, bg_map, env_map, alpha = out["fold"]
            assert (bg_map is not None) == envmap and (env_map is not None) == envmap
            assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(depth).all())
            if N > 1:
                assert float((rgb[0] - rgb[1]).abs().max()) > 1e-3 or field == "opaque_masked"   # the neighbours do differ
            if (S, N) == (64, 2049) and field == "opaque_masked":
                first, empty, tail = _skipped_tiles(alpha)
                print(f"{field} env={int(envmap)} {prec} dense={int(dense)}: first tile empty {first}, all empty {empty}, opaque before tile 2 {tail}")
                assert first > 0 and empty > 0 and tail > 0
            if not envmap and (S, N) == (64, 3):   # one shape per arithmetic, route and field against float64
                want = _oracle_render(field, S, N)
                e_rgb, e_d = maxerr(rgb, want[0]), maxerr(depth, want[1])
                print(f"{field} {prec} dense={int(dense)} S={S} N={N}: rgb err {e_rgb:.3e} depth err {e_d:.3e}")
                assert float(np.abs(want[0]).max()) > 0.05
                assert e_rgb <= RGB_TOL and e_d <= DEPTH_TOL
    finally:
        model.dense_appearance = True
