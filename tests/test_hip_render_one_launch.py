"""ego_render_forward's one-launch eval render (include/egonerf_hip.h: ego_render_forward_marches): the folded dense shade kernel whose
waves march the rays they shade themselves.  EGO_RENDER_MARCH=1 against =0 (ego_march_density + ego_shade_composite) through
ego_render_forward: the five outputs and the workspace's distances, weights and background weights bit for bit, the coordinates
wherever a colour is read (behind an exactly opaque prefix the one-wave march leaves zeros, the two-wave march the coordinates:
tests/test_hip_march_split.py).  S = 160 has a ragged last pass and an odd pass count for two and four passes side by side; N = 1, 3,
2049 leave waves of the grid without a ray, with one and with two, and workgroups whose waves partly have none.  The opaque field
drives the transmittance to exactly 0 inside rays, asked with the per-sample alpha (no early stop) and without it (store_stopped)."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth
from egonerf_amd.model import YinYangAlphaGridMask
from tests.helpers import make_model, make_oracle, maxerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
RGB_TOL = 1e-4            # tests/test_hip_parity.py
FAR = 15.0
DEPTH_TOL = 1e-3 * FAR
PRECISIONS = ("f16x3", "f16f8", "f16f6")
ENV_KEYS = ("EGO_DENSE_APP", "EGO_DENSE_APP_MAX_MB", "EGO_DENSE_DENSITY", "EGO_DENSE_DENSITY_MAX_MB", "EGO_RENDER_FOLD", "EGO_RENDER_COMPACT",
            "EGO_RENDER_MARCH", "EGO_MARCH_SPLIT")
SAMPLES = (32, 64, 160, 512)
RAYS = (1, 3, 2049)
# density_shift 0: surfaces hide what lies behind them, the transmittance reaches exactly 0 inside a ray
FIELDS = {"default": dict(density_shift=-8.0), "opaque": dict(density_shift=0.0)}


@pytest.fixture()
def clean_env(monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("EGO_RENDER_FOLD", "1")   # both sides fold (2049 x 512 is not balanced): the same sums in the same order
    return monkeypatch


_RAYS = {}


def _rays(n):
    if n not in _RAYS:
        _RAYS[n] = torch.from_numpy(synth.make_rays(n, seed=11))
    return _RAYS[n]


_SCENES = {}


def _scene(field, envmap):
    if (field, envmap) not in _SCENES:
        kw = dict(use_envmap=True, envmap_res_H=16) if envmap else {}
        cfg = synth.SceneConfig(n_voxel=20 ** 3, **FIELDS[field], **kw)
        assert cfg.far == FAR
        w = synth.make_weights(cfg, seed=7)
        _SCENES[field, envmap] = (cfg, w, make_model(cfg, w, DEV))
    return _SCENES[field, envmap]


def _align64(v):
    return (v + 63) & ~63


def _workspace(model, N, S, explicit_z):
    """z, weight, bg, coords of the last ego_render_forward (csrc/ego_render.hip: make_plan without resampling)"""
    n, _args, ws = model._last_render
    assert n == N
    w0 = _align64(N * S)
    bg0 = _align64(w0 + N * S)
    rgb0 = _align64(bg0 + N)
    crd0 = _align64(rgb0 + 3 * N * S)
    return dict(z=None if explicit_z else ws[:N * S].clone(), weight=ws[w0:w0 + N * S].view(N, S).clone(), bg=ws[bg0:bg0 + N].clone(),
                coords=ws[crd0:crd0 + 4 * N * S].view(N, S, 4).clone())


def _poisoned_empty(real_empty):
    """torch.empty whose float32 blocks come filled with NaN: the caching allocator hands a render the block an earlier render of the
    same shape filled with the right values, and a workspace slot or an output that a kernel fails to write would compare equal."""
    def empty(*a, **kw):
        t = real_empty(*a, **kw)
        if t.dtype == torch.float32 and t.is_cuda:
            t.fill_(float("nan"))
        return t
    return empty


def _render(model, rays, S, env, march, need_alpha=True, explicit_z=False):
    env.setenv("EGO_RENDER_MARCH", "1" if march else "0")
    sc, lib, N = model.scene(), _lib.load(), rays.shape[0]
    assert lib.ego_render_forward_folds(sc, N, S) == 1
    assert lib.ego_render_forward_marches(sc, N, S) == (1 if march else 0)
    with torch.no_grad(), env.context() as m:
        m.setattr(torch, "empty", _poisoned_empty(torch.empty))
        out = model(rays, exp_sampling=not explicit_z, n_coarse=S, need_alpha=need_alpha)
    torch.cuda.synchronize()
    assert model._last_render is not None   # the call went through ego_render_forward
    return tuple(None if t is None else t.clone() for t in out), _workspace(model, N, S, explicit_z)


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert torch.equal(a, b), (what, float((a - b).abs().max()))


def _compare(model, rays, S, env, what, **kw):
    got, ws_got = _render(model, rays, S, env, True, **kw)
    want, ws_want = _render(model, rays, S, env, False, **kw)
    assert len(got) == 5
    for k, name in enumerate(("rgb_map", "depth", "bg_map", "env_map", "alpha")):
        _same(got[k], want[k], (what, name))
    for name in ("z", "weight", "bg"):
        _same(ws_got[name], ws_want[name], (what, "workspace " + name))
        assert ws_got[name] is None or not bool(torch.isnan(ws_got[name]).any()), (what, "workspace " + name + " not written")
    read = ws_want["weight"] > 0
    assert torch.equal(ws_got["coords"][read], ws_want["coords"][read]), (what, "workspace coords where a colour is read")
    return got, ws_got


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("envmap", [False, True])
def test_one_launch_returns_the_bits_of_two(clean_env, envmap, prec):
    for field in sorted(FIELDS):
        _cfg, _w, model = _scene(field, envmap)
        model.mlp_precision = prec
        for S in SAMPLES:
            for N in RAYS:
                rays = _rays(N).to(DEV)
                for explicit_z in (False, True):
                    for need_alpha in ((True, False) if field == "opaque" else (True,)):
                        what = (field, envmap, prec, S, N, "z_coarse" if explicit_z else "schedule", need_alpha)
                        got, ws = _compare(model, rays, S, clean_env, what, need_alpha=need_alpha, explicit_z=explicit_z)
                        rgb, depth, bg_map, env_map, alpha = got
                        assert (bg_map is not None) == envmap and (env_map is not None) == envmap and (alpha is not None) == need_alpha
                        assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(depth).all())
                        if alpha is not None:
                            assert alpha.shape == (N, S + int(envmap))
                            if envmap:
                                assert bool((alpha[:, S] == 1).all())   # the envmap's column of ones
                        if field == "opaque" and N == 2049 and S >= 64:
                            # the carry reaches exactly 0 inside rays: zero background weight, weights of exactly 0 behind the surface
                            stopped = (ws["bg"] == 0) & (ws["weight"][:, -1] == 0) & (ws["weight"] > 0).any(1)
                            assert int(stopped.sum()) > 0, what


@pytest.mark.parametrize("prec", PRECISIONS)
def test_one_launch_without_tile_flags(clean_env, prec):
    """The exact skip of all-zero tiles switched off (ego_scene.weight_thres < 0: no tile flags, every sample shaded)."""
    for field in sorted(FIELDS):
        _cfg, _w, model = _scene(field, False)
        model.mlp_precision = prec
        model.skip_zero_weight_tiles = False
        try:
            assert model.scene().weight_thres < 0
            for S, N in ((64, 3), (160, 2049)):
                _compare(model, _rays(N).to(DEV), S, clean_env, (field, prec, S, N, "no flags"))
        finally:
            model.skip_zero_weight_tiles = True


@pytest.mark.parametrize("prec", PRECISIONS)
def test_one_launch_against_float64(clean_env, prec):
    S, N = 64, 3
    cfg, w, model = _scene("default", False)
    model.mlp_precision = prec
    oracle = make_oracle(cfg, w, dtype=torch.float64)
    o = oracle.forward(_rays(N).double(), n_coarse=S)
    want_rgb, want_depth = o[0].numpy(), o[1].numpy()
    (rgb, depth, *_), _ws = _render(model, _rays(N).to(DEV), S, clean_env, True)
    e_rgb, e_d = maxerr(rgb, want_rgb), maxerr(depth, want_depth)
    print(f"{prec} S={S} N={N}: rgb err {e_rgb:.3e} depth err {e_d:.3e}")
    assert float(np.abs(want_rgb).max()) > 0.05
    assert e_rgb <= RGB_TOL and e_d <= DEPTH_TOL


def test_other_scenes_keep_their_launches(clean_env):
    """A masked scene and a scene without baked grids report no one-launch render, whatever the override says, and still render."""
    cfg, _w, model = _scene("default", False)
    model.mlp_precision = "f16f6"
    lib, S, N = _lib.load(), 64, 3
    rays = _rays(N).to(DEV)
    clean_env.setenv("EGO_RENDER_MARCH", "1")
    assert lib.ego_render_forward_marches(model.scene(), N, S) == 1
    with torch.no_grad():
        want = model(rays, exp_sampling=True, n_coarse=S)[0].clone()
    # without the baked density grid, without the baked appearance grid
    for attr in ("dense_density", "dense_appearance"):
        setattr(model, attr, False)
        try:
            assert lib.ego_render_forward_marches(model.scene(), N, S) == 0
            with torch.no_grad():
                rgb = model(rays, exp_sampling=True, n_coarse=S)[0]
            assert maxerr(rgb, want.cpu().numpy()) <= RGB_TOL
        finally:
            setattr(model, attr, True)
    # with an occupancy mask (all ones: the same picture)
    n_r, n_th, n_ph = cfg.grid
    vol = torch.ones(2, 1, 1, n_ph, n_th, n_r)
    model.alphaMask = YinYangAlphaGridMask(DEV, vol[0].to(DEV), vol[1].to(DEV))
    model.use_alpha_mask = True
    try:
        assert lib.ego_render_forward_marches(model.scene(), N, S) == 0
        with torch.no_grad():
            rgb = model(rays, exp_sampling=True, n_coarse=S)[0]
        assert maxerr(rgb, want.cpu().numpy()) <= RGB_TOL
    finally:
        model.use_alpha_mask = False
        model.alphaMask = None
    assert lib.ego_render_forward_marches(model.scene(), N, S) == 1
    assert lib.ego_render_forward_marches(None, N, S) == 0


def test_a_marched_event_keeps_its_place(clean_env):
    """ego_render_args.marched is promised behind the march and ahead of the shade: a call that passes it renders with two launches
    (the same bits), and the event is recorded.  This does NOT prove the routing: both routes return these bits and record the event,
    and ego_render_forward_marches answers for a call without the event; where the event is recorded is read in ego_render_forward."""
    _cfg, _w, model = _scene("default", False)
    model.mlp_precision = "f16f6"
    S, N = 64, 2049
    rays = _rays(N).to(DEV)
    clean_env.setenv("EGO_RENDER_MARCH", "1")
    assert _lib.load().ego_render_forward_marches(model.scene(), N, S) == 1
    ev = torch.cuda.Event()
    ev.record()
    with torch.no_grad():
        want = model(rays, exp_sampling=True, n_coarse=S)
        got = model(rays, exp_sampling=True, n_coarse=S, marched_event=ev)
    torch.cuda.synchronize()
    assert ev.query()
    for a, b in zip(got, want):
        _same(a, b, "marched event")
