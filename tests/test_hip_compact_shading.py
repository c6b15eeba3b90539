"""The compact shading path of ego_render_forward (include/egonerf_hip.h: ego_render_forward_compacts): with an occupancy mask or a
weight threshold, only the live samples (weight > max(weight_thres, 0), tensorBase.py:480-487's app_mask) are shaded, in tiles cut
from a list of them.  It must return the bits of the tile path (EGO_RENDER_COMPACT=0) and of the folded path where that applies, and
report exactly the live count as the number of shaded samples."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth
from egonerf_amd.renderer import erp_rays, volume_renderer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
THRES = 1e-4
PRECISIONS = ("f16f6", "f16f8", "f16x3", "f32")


class _env:
    """Set (or, with None, remove) environment variables for the duration of a block."""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


_MODELS = {}


def scene_model(kind, env, shading="MLP_Fea"):
    """kind: 'carved' (transparent field with real empty space, mask applied), 'thres' (the same field unmasked, rayMarch_weight_thres
    on), 'opaque0' / 'opaque4' (density_shift 0 / +4: surfaces hide what lies behind them, carved and masked as well)."""
    key = (kind, env, shading)
    if key not in _MODELS:
        shift = {"carved": -10.0, "thres": -10.0, "opaque0": 0.0, "opaque4": 4.0}[kind]
        cfg = synth.SceneConfig(n_voxel=40 ** 3, near=0.1, far=300.0, r0=0.05, density_shift=shift, use_envmap=env, envmap_res_H=64,
                                shadingMode=shading)
        w = synth.make_weights(cfg, seed=1234)
        if kind != "thres":
            w = synth.carve_empty_space(w, cfg)
        model = synth.build_model(cfg, w, DEV)
        with torch.no_grad():
            if kind == "thres":
                model.use_weight_thres, model.rayMarch_weight_thres = True, THRES
            else:
                frac = model.updateAlphaMask()
                assert 0.0 < frac <= 1.0
                # at this grid size the mask of the carved field is nearly full: clear two slabs so that it bites inside the rays
                from egonerf_amd.model import YinYangAlphaGridMask
                vols = [model.alphaMask.alpha_volume_yin.clone(), model.alphaMask.alpha_volume_yang.clone()]
                for v in vols:
                    d = v.shape[-1]
                    v[..., d // 3:d // 2] = 0
                    v[0, 0, :v.shape[2] // 2, :, 2 * d // 3:] = 0
                model.alphaMask = YinYangAlphaGridMask(DEV, vols[0], vols[1])
                model.use_alpha_mask = True
                model.invalidate_scene()
        _MODELS[key] = model
    return _MODELS[key]


def sphere_rays(H=32, W=64):
    """Every view direction of an equirectangular camera: the rays cross the yin/yang borders, so tiles cut from the live list mix
    samples of both grids."""
    return erp_rays(H, W, np.eye(4, dtype=np.float32)[:3], DEV)


def render(model, rays, compact, fold=None, **kw):
    with _env(EGO_RENDER_COMPACT=compact, EGO_RENDER_FOLD=fold), torch.no_grad():
        out = model(rays, exp_sampling=True, **kw)
        n = model.last_shaded_samples
        torch.cuda.synchronize()
    return out, (None if n is None else int(n))


def assert_same(a, b, what):
    for name, x, y in zip(("rgb_map", "depth", "bg_map", "env_map", "alpha"), a, b):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x, y), (what, name, float((x - y).abs().max()))


def marched_weights(model, rays, n_coarse, n_fine, resampling):
    """The weights ego_render_forward's last march computes for these rays (stage entry points, the same launches)."""
    lib, st, sc = _lib.load(), _lib.stream_handle(), model.scene()
    N = rays.shape[0]
    S = n_coarse + n_fine if resampling else n_coarse
    f = lambda *shape: torch.empty(*shape, device=DEV, dtype=torch.float32)
    sched, near = model._sched(n_coarse, DEV), float(model.near_far[0])
    zc, w = f(N, n_coarse), f(N, S)
    if resampling:
        wc, z = f(N, n_coarse), f(N, S)
        _lib.check(lib.ego_march_density(sc, rays.data_ptr(), N, n_coarse, None, sched.data_ptr(), None, near, 1, zc.data_ptr(), None, 0,
                                         wc.data_ptr(), None, None, None, None, st), "march coarse")
        _lib.check(lib.ego_sample_pdf_merge(zc.data_ptr(), wc.data_ptr(), None, N, n_coarse, n_fine, 1, z.data_ptr(), None, st), "pdf merge")
        _lib.check(lib.ego_march_density(sc, rays.data_ptr(), N, S, z.data_ptr(), None, None, near, 2, None, None, 0, w.data_ptr(), f(N).data_ptr(),
                                         f(N, S, 4).data_ptr(), None, None, st), "march fine")
    else:
        _lib.check(lib.ego_march_density(sc, rays.data_ptr(), N, S, None, sched.data_ptr(), None, near, 0, zc.data_ptr(), None, 0, w.data_ptr(),
                                         f(N).data_ptr(), f(N, S, 4).data_ptr(), None, None, st), "march")
    torch.cuda.synchronize()
    return w


SAMPLING = {"rs": dict(n_coarse=64, n_fine=64, resampling=True, use_coarse_sample=True), "nr": dict(n_coarse=128)}


@pytest.mark.parametrize("kind", ["carved", "thres", "opaque0", "opaque4"])
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("sampling", ["rs", "nr"])
@pytest.mark.parametrize("env", [False, True])
def test_compact_is_bit_equal(kind, prec, sampling, env):
    model = scene_model(kind, env)
    model.mlp_precision = prec
    rays = sphere_rays()
    kw = SAMPLING[sampling]
    N, S = rays.shape[0], kw["n_coarse"] + kw.get("n_fine", 0)
    sc = model.scene()
    lib = _lib.load()
    with _env(EGO_RENDER_COMPACT=None):
        assert lib.ego_render_forward_compacts(sc, N, S) == 1   # the default takes the list on every masked / thresholded call
    tiles, n_tiles = render(model, rays, "0", **kw)
    comp, n_live = render(model, rays, "1", **kw)
    assert_same(tiles, comp, "compact vs tiles")
    assert 0 < n_live <= n_tiles <= N * S
    with _env(EGO_RENDER_FOLD="1", EGO_RENDER_COMPACT="0"):
        folds = bool(lib.ego_render_forward_folds(sc, N, S))
    if folds:
        folded, _ = render(model, rays, "0", fold="1", **kw)
        assert_same(folded, comp, "compact vs folded")


@pytest.mark.parametrize("prec", ("f16f6", "f16f8", "f16x3"))
@pytest.mark.parametrize("kind", ["carved", "thres"])
def test_compact_with_half_tables(prec, kind):
    model = scene_model(kind, True)
    model.mlp_precision, model.app_table_dtype = prec, "f16"
    try:
        rays = sphere_rays()
        tiles, _ = render(model, rays, "0", **SAMPLING["rs"])
        comp, _ = render(model, rays, "1", **SAMPLING["rs"])
        assert_same(tiles, comp, "app_f16")
    finally:
        model.app_table_dtype = "f32"


@pytest.mark.parametrize("prec", PRECISIONS)
def test_compact_ragged(prec):
    """S = 100 (tiles straddle rays), N = 1000 (not a multiple of the shade's wave count)."""
    model = scene_model("carved", False)
    model.mlp_precision = prec
    rays = sphere_rays(40, 25)
    assert rays.shape[0] == 1000
    tiles, _ = render(model, rays, "0", n_coarse=100)
    comp, n_live = render(model, rays, "1", n_coarse=100)
    assert_same(tiles, comp, "ragged")
    w = marched_weights(model, rays, 100, 0, False)
    assert n_live == int((w > 0).sum())   # this scene skips exactly: weight_thres = 0


@pytest.mark.parametrize("kind", ["carved", "thres", "opaque4"])
@pytest.mark.parametrize("sampling", ["rs", "nr"])
def test_shaded_count_is_the_live_count(kind, sampling):
    model = scene_model(kind, False)
    model.mlp_precision = "f16f6"
    rays = sphere_rays()
    kw = SAMPLING[sampling]
    N, S = rays.shape[0], kw["n_coarse"] + kw.get("n_fine", 0)
    thr = max(float(model.scene().weight_thres), 0.0)
    w = marched_weights(model, rays, kw["n_coarse"], kw.get("n_fine", 0), kw.get("resampling", False))
    live = (w > thr).reshape(-1)
    _, n_default = render(model, rays, None, **kw)
    assert n_default == int(live.sum())
    _, n_tiles = render(model, rays, "0", **kw)
    active = live.reshape(-1, 32).any(1)
    assert n_tiles == min(32 * int(active.sum()), N * S)
    assert n_default < n_tiles   # the point of the list: dead samples between live ones no longer ride along
    # the list's tiles do mix yin and yang samples on these rays (the border-straddling MFMA pass of the shade kernels)
    crd = torch.empty(N, S, 4, device=DEV)
    lib, st, sc = _lib.load(), _lib.stream_handle(), model.scene()
    if not kw.get("resampling", False):
        zc = torch.empty(N, S, device=DEV)
        _lib.check(lib.ego_march_density(sc, rays.data_ptr(), N, S, None, model._sched(S, DEV).data_ptr(), None, float(model.near_far[0]), 0,
                                         zc.data_ptr(), None, 0, torch.empty(N, S, device=DEV).data_ptr(), torch.empty(N, device=DEV).data_ptr(),
                                         crd.data_ptr(), None, None, st), "march")
        torch.cuda.synchronize()
        yang = crd.reshape(-1, 4)[:, 3][live] != 0
        n = yang.numel() // 32 * 32
        per_tile = yang[:n].reshape(-1, 32)
        assert bool((per_tile.any(1) & ~per_tile.all(1)).any())


def test_unmasked_default_keeps_the_tile_path():
    model = synth.build_model(synth.SceneConfig(n_voxel=40 ** 3), synth.make_weights(synth.SceneConfig(n_voxel=40 ** 3), seed=7), DEV)
    rays = torch.from_numpy(synth.make_rays(512, seed=3)).to(DEV)
    lib = _lib.load()
    with _env(EGO_RENDER_COMPACT=None):
        assert lib.ego_render_forward_compacts(model.scene(), 512, 128) == 0
    a, n = render(model, rays, None, n_coarse=128)
    b, n0 = render(model, rays, "0", n_coarse=128)
    assert_same(a, b, "unmasked default")
    assert n == n0
    w = marched_weights(model, rays, 128, 0, False)
    assert n == min(32 * int((w > 0).reshape(-1, 32).any(1).sum()), 512 * 128)
    model.skip_zero_weight_tiles = False   # no skipping at all: every sample is shaded
    _, n_all = render(model, rays, None, n_coarse=128)
    assert n_all == 512 * 128


def test_handover_and_repeat_are_bit_equal():
    model = scene_model("carved", True)
    model.mlp_precision = "f16f6"
    rays = sphere_rays(64, 128)
    kw = dict(chunk=2048, n_coarse=64, n_fine=64, exp_sampling=True, resampling=True, use_coarse_sample=True, device=DEV, keep_alpha=False)
    with torch.no_grad():
        res = volume_renderer(rays, model, **kw)
        again = volume_renderer(rays, model, **kw)
        host = volume_renderer(rays, model, empty_gpu_cache=True, **kw)
        torch.cuda.synchronize()
    for x, y, z in zip(res, again, host):
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y)
            assert np.array_equal(x.cpu().numpy(), np.asarray(z))


def test_mlp_head_falls_back():
    model = scene_model("carved", False, shading="MLP")
    rays = sphere_rays()
    lib = _lib.load()
    with _env(EGO_RENDER_COMPACT="1"):
        assert lib.ego_render_forward_compacts(model.scene(), rays.shape[0], 128) == 0
    a, _ = render(model, rays, "0", n_coarse=128)
    b, _ = render(model, rays, "1", n_coarse=128)
    assert_same(a, b, "MLP head")


def test_compact_scan_with_runs_of_two_blocks():
    """65 537 rays make 1025 blocks of the live count: every thread of the one-workgroup scan then owns a run of two entries, and the last
    run holds one.  The list must still be the tile path's samples in the tile path's order, and its length the live count."""
    model = scene_model("thres", False)
    model.mlp_precision = "f16f6"
    N, S = 65537, 16
    rays = erp_rays(257, 256, np.eye(4, dtype=np.float32)[:3], DEV)[:N].contiguous()
    assert rays.shape[0] == N and (N + 63) // 64 == 1025
    lib = _lib.load()
    with _env(EGO_RENDER_COMPACT=None):
        assert lib.ego_render_forward_compacts(model.scene(), N, S) == 1
    tiles, n_tiles = render(model, rays, "0", n_coarse=S)
    # The render's workspace comes from torch's caching allocator: a second render of the same size gets the block of the first, the
    # tile path's colours still in it, and a sample missing from the list would find its colour already there.  So let the model drop
    # that block (a small render replaces the workspace it keeps) and fill the free blocks of that size with NaN.
    render(model, rays[:64].contiguous(), "0", n_coarse=S)
    args = _lib.RenderArgs(n_coarse=S, n_fine=0, resampling=0, use_coarse_sample=1)
    ws_floats = int(lib.ego_render_workspace_bytes(N, C.byref(args))) // 4
    assert ws_floats > N * S * 9
    poison = [torch.full((ws_floats,), float("nan"), device=DEV) for _ in range(2)]
    torch.cuda.synchronize()
    del poison
    comp, n_live = render(model, rays, "1", n_coarse=S)
    assert_same(tiles, comp, "compact vs tiles, 1025 blocks")
    thr = max(float(model.scene().weight_thres), 0.0)
    w = marched_weights(model, rays, S, 0, False)
    print(f"live {n_live} of {N * S}")
    assert n_live == int((w > thr).sum())
    assert 0 < n_live <= n_tiles <= N * S
    # live samples sit in both entries of the scan's runs, first and last included
    per_block = (w > thr).sum(1)[:1024 * 64].reshape(1024, 64).sum(1)
    assert int(per_block[0]) > 0 and int(per_block[1]) > 0 and int(per_block[-1]) > 0 and int((w[1024 * 64:] > thr).sum()) > 0
