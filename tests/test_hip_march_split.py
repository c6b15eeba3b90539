"""ego_march_density with a ray's passes dealt to two waves (few rounds of wave slots, long rays: the 4096 x 512 headline) must return
the bits of the one-wave-per-ray form: weights, background weight, alpha, distances, tile flags (the coordinates of samples behind an
exactly opaque prefix are the one documented difference: the one-wave form never evaluates them and writes zeros).  And every form of it
(factored / dense, one / two waves per ray, the any-shape kernel) and ego_raw2alpha must return the bytes of a recorded build
(tests/golden/march_digests.json)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth

pytestmark = pytest.mark.gpu


def march(model, cfg, rays, S, with_alpha, term_eps=0.0):
    lib, st = _lib.load(), _lib.stream_handle()
    model.early_termination_eps = term_eps
    sc = model.scene()
    N = rays.shape[0]
    dev = rays.device
    sched = model._sched(S, dev)
    z, w, bg = torch.zeros(N, S, device=dev), torch.zeros(N, S, device=dev), torch.zeros(N, device=dev)
    crd = torch.zeros(N, S, 4, device=dev)
    alpha = torch.zeros(N, S + 1, device=dev) if with_alpha else None
    act = torch.zeros((N * S + 31) // 32, device=dev, dtype=torch.uint8)
    _lib.check(lib.ego_march_density(sc, rays.data_ptr(), N, S, None, sched.data_ptr(), None, cfg.near, 0, z.data_ptr(), _lib.ptr(alpha), S + 1 if with_alpha else 0,
                                     w.data_ptr(), bg.data_ptr(), crd.data_ptr(), None, act.data_ptr(), st), "march")
    torch.cuda.synchronize()
    return z, w, bg, alpha, act, crd


@pytest.mark.parametrize("S,n_rays,density_shift", [(512, 4096, None), (300, 1001, None), (256, 130, 0.0), (449, 67, 0.0)])
@pytest.mark.parametrize("with_alpha", [False, True])
def test_two_waves_per_ray_return_the_same_bits(S, n_rays, density_shift, with_alpha):
    cfg = synth.SceneConfig(n_voxel=40 ** 3) if density_shift is None else synth.SceneConfig(n_voxel=40 ** 3, density_shift=density_shift)
    model = synth.build_model(cfg, synth.make_weights(cfg, seed=7), "cuda")
    rays = torch.from_numpy(synth.make_rays(n_rays, seed=5)).cuda()
    out = {}
    try:
        for split in ("1", "2"):
            os.environ["EGO_MARCH_SPLIT"] = split
            out[split] = march(model, cfg, rays, S, with_alpha, term_eps=1e-4 if S == 449 else 0.0)
    finally:
        os.environ.pop("EGO_MARCH_SPLIT", None)
    a, b = out["1"], out["2"]
    for k, name in enumerate(("z", "weight", "bg", "alpha", "tile flags")):
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), (name, S, n_rays)
    assert float(a[1].sum()) > 0.0
    shaded = a[1] > 0
    assert torch.equal(a[5][shaded], b[5][shaded])   # coordinates wherever a colour is read
    if density_shift is not None and not with_alpha:   # opaque field: the one-wave form stops behind exact zero transmittance
        assert bool((a[1] == 0).any())


# ---- the march bit for bit against a recorded build -----------------------------------------------------------------------------------
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "march_digests.json")
# (field, N, S, coarse, outputs, mask): every value of every column appears with both forms and, where the ray has two passes, both splits.
#   field    "default" | "opaque" (density_shift 0.0: the transmittance reaches exactly 0, so a march that stores neither alpha nor sigma stops)
#   N        5: the last workgroup holds one live ray at one wave per ray, and a dead ray pair that must still reach the barriers at two;  67
#   S        2 (the minimum) | 65 (a one-lane tail pass; tiles straddle rays: the set-only flag rule) | 256 (whole tiles, split 2 + 2) |
#            449 (8 passes = MARCH_MAXP per deferred half, ragged tail; marched with early_termination_eps = 1e-4)
#   coarse   0 schedule + jitter | 1 the pooled tables (never masked) | 2 explicit distances, the fine LUT
#   outputs  "all": alpha with the appended column (alpha_stride = S + 1) and sigma | "few": neither
#   mask     None | "same": updateAlphaMask() at the field's resolution (the dense form's shared-tap test) | "other": at another one
MARCH_CASES = [
    ("default", 5, 2, 0, "all", None), ("default", 67, 65, 0, "all", "same"), ("default", 5, 256, 2, "all", "other"),
    ("default", 67, 449, 1, "all", None), ("opaque", 5, 449, 0, "few", None), ("opaque", 67, 256, 0, "few", None),
    ("default", 67, 256, 0, "few", "same"), ("default", 5, 65, 1, "few", None), ("default", 67, 2, 2, "few", "other"),
    ("opaque", 5, 65, 2, "few", None), ("default", 5, 449, 2, "all", "same"), ("default", 67, 449, 0, "few", "other"),
    ("opaque", 67, 65, 0, "all", None),
]
MASK_QUANTILE = 0.98   # the mask keeps the cells around the densest 2 % of the lattice (3 x 3 x 3 max-pool): a partial mask on any field


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _digest_model(field, mask, **kw):
    cfg = synth.SceneConfig(n_voxel=40 ** 3, **kw) if field == "default" else synth.SceneConfig(n_voxel=40 ** 3, density_shift=0.0, **kw)
    model = synth.build_model(cfg, synth.make_weights(cfg, seed=7), "cuda")
    if mask is not None:
        n_r, n_th, n_ph = cfg.grid
        grid = [n_r, n_th, n_ph] if mask == "same" else [n_r + 3, n_th + 2, n_ph - 3]
        model.alphaMask_thres = float(torch.quantile(torch.cat([a.flatten() for a in model.getDenseAlpha(grid)]), MASK_QUANTILE))
        kept = model.updateAlphaMask(grid)
        assert 0.02 < kept < 0.98, (field, mask, kept)
        model.use_alpha_mask = True
    return cfg, model


def _digest_march(model, cfg, dense, N, S, coarse, outputs):
    """One ego_march_density with every output buffer zero-initialised -> {buffer: sha256 of all of it}"""
    lib, st, dev = _lib.load(), _lib.stream_handle(), "cuda"
    model.early_termination_eps = 1e-4 if S == 449 else 0.0
    model.invalidate_scene()
    sc = _lib.Scene.from_buffer_copy(model.scene())
    if not dense:
        sc.density_dense = sc.density_coarse_dense = None
    assert bool(sc.density_coarse_dense if coarse & 1 else sc.density_dense) == dense
    rays = torch.from_numpy(synth.make_rays(N, seed=5)).to(dev)
    sched = model._sched(S, dev)
    u = torch.from_numpy(synth.hash_uniform(31, S, N * S).reshape(N, S).astype(np.float32)).to(dev)
    z_in = torch.sort(cfg.near + sched[None] + 0.01 * u, 1).values.contiguous() if coarse == 2 else None
    jitter = u if coarse == 0 else None
    z, w, bg, crd = torch.zeros(N, S, device=dev), torch.zeros(N, S, device=dev), torch.zeros(N, device=dev), torch.zeros(N, S, 4, device=dev)
    alpha, sigma = (torch.zeros(N, S + 1, device=dev), torch.zeros(N, S, device=dev)) if outputs == "all" else (None, None)
    act = torch.zeros((N * S + 31) // 32, device=dev, dtype=torch.uint8)
    _lib.check(lib.ego_march_density(sc, rays.data_ptr(), N, S, _lib.ptr(z_in), None if coarse == 2 else sched.data_ptr(), _lib.ptr(jitter), cfg.near,
                                     coarse, z.data_ptr(), _lib.ptr(alpha), S + 1 if alpha is not None else 0, w.data_ptr(), bg.data_ptr(),
                                     crd.data_ptr(), _lib.ptr(sigma), act.data_ptr(), st), "march")
    torch.cuda.synchronize()
    print(f"  N={N} S={S} coarse={coarse} {outputs} dense={int(dense)} split={os.environ.get('EGO_MARCH_SPLIT')}: weight sum {float(w.sum()):.4f}, "
          f"weights == 0: {float((w == 0).float().mean()):.3f}, tiles flagged {float(act.float().mean()):.3f}")
    named = dict(z=z, weight=w, bg=bg, alpha=alpha, sigma=sigma, coords=crd, tile_flags=act)
    return {k: _sha(t) for k, t in named.items() if t is not None}


def march_digests():
    """case -> {buffer: sha256 of its bytes}: MARCH_CASES through ego_march_density in the factored and the dense form, with one and
    (two passes or more) two waves per ray; the same entry point on a field of 8 density components (k_march_generic) behind a mask;
    ego_raw2alpha on 5 x 65.  tools/capture_digests.py records this from another build."""
    out, models = {}, {}
    old = os.environ.get("EGO_MARCH_SPLIT")
    try:
        for field, N, S, coarse, outputs, mask in MARCH_CASES:
            if (field, mask) not in models:
                models[field, mask] = _digest_model(field, mask)
            cfg, model = models[field, mask]
            for dense in (False, True):
                for split in ("1", "2") if S > 64 else ("1",):
                    os.environ["EGO_MARCH_SPLIT"] = split
                    out[f"{field} N={N} S={S} coarse={coarse} {outputs} mask={mask} dense={int(dense)} split={split}"] = \
                        _digest_march(model, cfg, dense, N, S, coarse, outputs)
        os.environ.pop("EGO_MARCH_SPLIT", None)
        cfg, model = _digest_model("default", "same", density_n_comp=(8, 8, 8))
        out["8 components N=5 S=65 coarse=0 all mask=same"] = _digest_march(model, cfg, False, 5, 65, 0, "all")
    finally:
        os.environ.pop("EGO_MARCH_SPLIT", None)
        if old is not None:
            os.environ["EGO_MARCH_SPLIT"] = old
    N, S = 5, 65
    sigma = torch.from_numpy((synth.hash_uniform(32, 0, N * S) * 40.0).reshape(N, S).astype(np.float32)).cuda()
    dist = torch.from_numpy((synth.hash_uniform(32, 1, N * S) * 0.05).reshape(N, S).astype(np.float32)).cuda()
    alpha, w, bg = torch.zeros(N, S, device="cuda"), torch.zeros(N, S, device="cuda"), torch.zeros(N, device="cuda")
    _lib.check(_lib.load().ego_raw2alpha(sigma.data_ptr(), dist.data_ptr(), N, S, alpha.data_ptr(), w.data_ptr(), bg.data_ptr(), _lib.stream_handle()),
               "raw2alpha")
    torch.cuda.synchronize()
    out["raw2alpha N=5 S=65"] = dict(alpha=_sha(alpha), weight=_sha(w), bg=_sha(bg))
    return out


def test_march_bits_match_recorded():
    """The march kernels have no atomics on their outputs, so a rewrite that keeps their arithmetic returns the recorded build's bytes:
    equality, no tolerance.  The fixture names the commit it was recorded from (never the tree under test)."""
    recorded = json.load(open(DIGESTS))["digests"]
    got = march_digests()
    n_tuned = sum(2 * (2 if S > 64 else 1) for _, _, S, *_ in MARCH_CASES)
    assert len(got) == n_tuned + 2 and {c: sorted(d) for c, d in got.items()} == {c: sorted(d) for c, d in recorded.items()}
    differs = [f"{case}: {name}" for case in got for name in got[case] if got[case][name] != recorded[case][name]]
    assert not differs, differs


@pytest.mark.parametrize("kw", [dict(n_coarse=512), dict(n_coarse=64, n_fine=64, resampling=True), dict(n_coarse=96)])
@pytest.mark.parametrize("prec", ["f16f6", "f16f8", "f16x3"])
@pytest.mark.parametrize("envmap", [False, True])
def test_folded_compositing_equals_the_two_launch_form(kw, prec, envmap):
    """EGO_RENDER_FOLD=1: ego_render_forward shades and composites in one launch (ego_shade_composite) wherever the scene allows it;
    =0: ego_shade + ego_composite (the default picks by balance: ego_render_forward_folds).  Same products AND - since round 5, when
    ego_composite took over the folded kernel's summation order - the same sums: all five outputs bit for bit, so a batch renders identically
    whichever form its size selects."""
    cfg = synth.SceneConfig(n_voxel=40 ** 3, use_envmap=envmap, envmap_res_H=64) if envmap else synth.SceneConfig(n_voxel=40 ** 3)
    model = synth.build_model(cfg, synth.make_weights(cfg, seed=11), "cuda")
    model.mlp_precision = prec
    rays = torch.from_numpy(synth.make_rays(333, seed=9)).cuda()
    out = {}
    try:
        for fold in (True, False):
            os.environ["EGO_RENDER_FOLD"] = "1" if fold else "0"
            with torch.no_grad():
                out[fold] = model(rays, exp_sampling=True, **kw)
    finally:
        os.environ.pop("EGO_RENDER_FOLD", None)
    for k in range(5):
        a, b = out[True][k], out[False][k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert torch.equal(a, b), (k, float((a - b).abs().max()))
    assert float(out[True][0].max()) > 0.05


def test_default_fold_decision_follows_the_balance_of_whole_rays():
    """ego_render_forward_folds: the folded kernel deals whole rays to its 2048 waves, so it is taken by default only where that costs
    nothing against the tile-granular two-launch form (round 5: it is 3.5 % faster there); the environment overrides either way."""
    from egonerf_amd import _lib
    lib = _lib.load()
    cfg = synth.SceneConfig(n_voxel=40 ** 3)
    model = synth.build_model(cfg, synth.make_weights(cfg, seed=11), "cuda")
    sc = model.scene()
    old = os.environ.pop("EGO_RENDER_FOLD", None)
    try:
        q = lambda N, S: int(lib.ego_render_forward_folds(sc, N, S))
        assert q(4096, 512) == 1 and q(16384, 256) == 1 and q(8192, 256) == 1 and q(1 << 21, 256) == 1
        assert q(4097, 512) == 0 and q(333, 512) == 0 and q(256, 64) == 0 and q(4096, 500) == 0 and q(0, 512) == 0
        os.environ["EGO_RENDER_FOLD"] = "0"
        assert q(4096, 512) == 0
        os.environ["EGO_RENDER_FOLD"] = "1"
        assert q(333, 512) == 1 and q(4096, 500) == 0     # forced, but only where the scene and the sample count qualify
        model.mlp_precision = "f32"
        assert int(lib.ego_render_forward_folds(model.scene(), 4096, 512)) == 0
    finally:
        os.environ.pop("EGO_RENDER_FOLD", None)
        if old is not None:
            os.environ["EGO_RENDER_FOLD"] = old
