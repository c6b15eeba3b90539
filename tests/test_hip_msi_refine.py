"""GPU: differentiable playback and texel refinement of multi-sphere images (egonerf_amd/msi.py: MultiSphereImage.render with grad,
refine_msi; csrc/ego_msi.hip: ego_msi_render_backward, ego_msi_project).

1. the texel gradients against float64 autograd of the restatement (tests/msi_grad_ref.py), allowed per tensor 4 x the distance of the
   float32 restatement from it (floor 1e-6 of the largest reference value), as the forward test allows;
2. a saturated (A = 1) and an empty (A = 0) layer: everything finite, exactly 0 behind the saturated layer;
3. thousands of rays on a handful of texels, and on one: no add is lost;
4. the forward is untouched by recording a graph;
5. refine_msi lowers the error against the teacher on held-out rays of the headbox and keeps the texels in range."""
import numpy as np
import pytest
import torch

from egonerf_amd import synth
from egonerf_amd.camera import FrameRenderer
from egonerf_amd.msi import MultiSphereImage, bake_msi, headbox_rays, refine_msi
from tests import msi_grad_ref
from tests.helpers import make_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
RADII = np.asarray([1.0, 1.7, 3.0, 6.0, 12.0], np.float32)
CENTER = np.asarray([0.25, -0.5, 0.125], np.float32)
HM, WM, N_RAYS = 6, 8, 600


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ball_rays(g, n, reach):
    o = g.standard_normal((n, 3))
    o *= (reach * g.uniform(0, 1, (n, 1)) ** (1 / 3)) / np.linalg.norm(o, axis=1, keepdims=True)
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o + CENTER, d], 1).astype(np.float32)


def hit_coordinates(rays, radii, Wm):
    """float64: (max |u.y| over the crossed layers and the direction itself, whether a bilinear tap of the ray wraps around the seam)."""
    p, d = rays[:, :3].astype(np.float64) - CENTER, rays[:, 3:].astype(np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    b, pp = (p * d).sum(1), (p * p).sum(1)
    uy, seam = np.abs(d[:, 1]), np.zeros(len(rays), bool)
    for R in radii.astype(np.float64):
        live = R > np.sqrt(pp)
        t = -b + np.sqrt(np.maximum(b * b - pp + R * R, 0))
        u = (p + t[:, None] * d) / R
        col = (1 - np.arctan2(-u[:, 0], -u[:, 2]) / np.pi) * Wm / 2 - 0.5
        uy = np.where(live, np.maximum(uy, np.abs(u[:, 1])), uy)
        seam |= live & ((col < 0) | (col >= Wm - 1))
    return uy, seam


def gradient_case(saturate):
    """600 rays (more than two blocks of 256, no multiple of 64) on L = 5, 6 x 8 texels around an off-origin centre, and the float64 and
    float32 autograd gradients with and without a background.  saturate: layer 1 holds A = 1 everywhere, layer 3 A = 0."""
    g = np.random.default_rng(29)
    cand = ball_rays(g, 3000, 0.6 * RADII[0])
    cand[0, :3] = CENTER + [1.3, 0.0, 0.0]        # between radius 0 and radius 1: layer 0 is skipped
    cand[1, :3] = CENTER + [0.0, 5.0, -12.5]      # outside every shell: only the background sees this ray
    phi = np.pi + g.uniform(-0.05, 0.05, 60)      # 60 candidates that look at the phi = +-pi seam
    th = g.uniform(-1.0, 1.0, 60)
    cand[2:62, 3:] = np.stack([-np.cos(th) * np.sin(phi), np.sin(th), -np.cos(th) * np.cos(phi)], -1)
    uy, seam = hit_coordinates(cand, RADII, WM)
    keep = np.flatnonzero(uy <= 0.999)            # away from the poles, where asin is ill-conditioned; the poles themselves follow
    assert keep[0] == 0 and keep[1] == 1
    poles = np.asarray([[*CENTER, 0, 1, 0], [*CENTER, 0, -1, 0], [*CENTER, 0.0, 1.0, -0.0], [*CENTER, -0.0, -1.0, 0.0]], np.float32)
    rays = np.concatenate([cand[keep[:N_RAYS - 4]], poles]).astype(np.float32)
    seam = seam[keep[:N_RAYS - 4]]
    rays[100:164, 3:] *= np.float32(2.5)          # a pinhole camera's directions are not normalised
    assert rays.shape == (N_RAYS, 6) and int(seam.sum()) >= 20, int(seam.sum())
    assert RADII[0] < np.linalg.norm(rays[0, :3] - CENTER) < RADII[1] and np.linalg.norm(rays[1, :3] - CENTER) > RADII[-1]
    layers = g.uniform(0, 1, (len(RADII), HM, WM, 4)).astype(np.float32)
    background = g.uniform(0, 1, (HM, WM, 4)).astype(np.float32)
    if saturate:
        layers[1, ..., 3], layers[3, ..., 3] = 1.0, 0.0
    g_rgb = g.standard_normal((N_RAYS, 3)).astype(np.float32)
    refs = {bg: {dt: msi_grad_ref.texel_gradients(rays, CENTER, RADII, layers, background if bg else None, g_rgb, dt)
                 for dt in (torch.float64, torch.float32)} for bg in (False, True)}
    return rays, layers, background, g_rgb, refs


@pytest.fixture(scope="module")
def plain_case():
    return gradient_case(False)


@pytest.fixture(scope="module")
def saturated_case():
    return gradient_case(True)


def image(radii, layers, background):
    bounds = np.concatenate([[0.5 * radii[0]], radii + 0.1]).astype(np.float32)
    return MultiSphereImage(T(layers), radii, bounds, CENTER, [0.1, 15.0], None if background is None else T(background))


def kernel_gradients(msi, rays, g_rgb, through="autograd"):
    """(g_layers, g_background or None) float64 numpy: through `render` and `backward`, or from ego_msi_render_backward called on zeroed
    buffers ("call")."""
    if through == "autograd":
        for p in msi.parameters():
            p.requires_grad_(True)
        rgb, _ = msi.render(T(rays))
        rgb.backward(T(g_rgb))
        return msi.layers.grad.double().cpu().numpy(), (None if msi.background is None else msi.background.grad.double().cpu().numpy())
    gl = torch.zeros_like(msi.layers)
    gb = None if msi.background is None else torch.zeros_like(msi.background)
    msi._render_backward(T(rays), msi.layers, msi.background, T(g_rgb), gl, gb)
    return gl.double().cpu().numpy(), (None if gb is None else gb.double().cpu().numpy())


def check_against_reference(got, refs, label):
    """Per tensor: |kernel - ref64| <= max(4 max |ref32 - ref64|, 1e-6 max |ref64|); prints every figure before it asserts."""
    ok = True
    for name, mine, want, f32 in zip(("layers", "background"), got, refs[torch.float64], refs[torch.float32]):
        if want is None:
            assert mine is None
            continue
        dev32, top = float(np.abs(f32 - want).max()), float(np.abs(want).max())
        tol, err = max(4 * dev32, 1e-6 * top), float(np.abs(mine - want).max())
        print(f"{label} d {name}: float32 restatement vs float64 {dev32:.3e}, kernel vs float64 {err:.3e}, tolerance {tol:.3e}, max |ref64| {top:.3e}")
        assert np.all(np.isfinite(mine))
        ok = ok and err <= tol
    assert ok


# ---- 1. the gradient against float64 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_background", [False, True])
@pytest.mark.parametrize("through", ["call", "autograd"])
def test_gradient_against_the_float64_restatement(plain_case, through, with_background):
    rays, layers, background, g_rgb, refs = plain_case
    msi = image(RADII, layers, background if with_background else None)
    got = kernel_gradients(msi, rays, g_rgb, through)
    check_against_reference(got, refs[with_background], f"{through} background={with_background}")
    want = refs[with_background][torch.float64]
    assert float(np.abs(want[0]).max()) > 1.0 and np.count_nonzero(want[0][0]) and np.count_nonzero(want[0][-1])   # the case is not trivial
    if with_background:
        assert np.all(got[1][..., 3] == 0) and np.count_nonzero(got[1][..., :3])   # the background's alpha gets nothing


# ---- 2. saturated and empty layers -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_background", [False, True])
def test_nothing_passes_a_saturated_layer(saturated_case, with_background):
    rays, layers, background, g_rgb, refs = saturated_case
    assert np.all(layers[1, ..., 3] == 1) and np.all(layers[3, ..., 3] == 0)
    msi = image(RADII, layers, background if with_background else None)
    got = kernel_gradients(msi, rays, g_rgb, "call")
    check_against_reference(got, refs[with_background], f"saturated background={with_background}")
    # every eye but ray 1's lies inside layer 1, and ray 1 lies outside every shell: whatever reaches layers 2 - 4 has passed A = 1
    assert int((np.linalg.norm(rays[:, :3] - CENTER, axis=1) >= RADII[1]).sum()) == 1
    assert np.count_nonzero(got[0][0]) and np.count_nonzero(got[0][1]) and np.all(got[0][2:] == 0)
    if with_background:   # ray 1 sees the background alone; without it the background lies behind the saturated layer for every ray
        assert np.count_nonzero(got[1])
        rest = np.arange(N_RAYS) != 1
        gl, gb = kernel_gradients(msi, rays[rest], g_rgb[rest], "call")
        assert np.all(np.isfinite(gl)) and np.all(gl[2:] == 0) and np.all(gb == 0)


# ---- 3. contention ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 4), (1, 1)])
def test_no_add_is_lost_under_contention(shape):
    """4099 rays on 8 texels, and on one.  A lost add is of the size of one ray's share of a texel, |g| w ~ 0.1, against a tolerance of
    the order of 1e-4 to 1e-3.  Measured on an MI355X over 200 runs of this call (tools/probe_msi_contention.py ->
    profiles/r13/msi_contention.json), error over tolerance: on one texel at most 0.18 (layers) and 0.40 (background); on 2 x 4 texels
    the background at most 0.64, the layers 0.66 in the median and 1.11 AT MOST - the 2 x 4 case can fail on a run.  No add is lost
    then: some 2000 float32 shares per texel and channel, added in arrival order, wander as far from float64 as the one sequential
    float32 sum that sets the tolerance."""
    g = np.random.default_rng(31)
    radii, n = RADII[:2], 4099
    rays = ball_rays(g, n, 0.6 * radii[0])
    layers = g.uniform(0, 1, (2, *shape, 4)).astype(np.float32)
    background = g.uniform(0, 1, (*shape, 4)).astype(np.float32)
    g_rgb = g.standard_normal((n, 3)).astype(np.float32)
    refs = {dt: msi_grad_ref.texel_gradients(rays, CENTER, radii, layers, background, g_rgb, dt) for dt in (torch.float64, torch.float32)}
    got = kernel_gradients(image(radii, layers, background), rays, g_rgb)
    check_against_reference(got, refs, f"contention {shape}")


# ---- 4. the forward is untouched -------------------------------------------------------------------------------------------------------

def test_recording_a_graph_leaves_the_forward_untouched(plain_case):
    rays, layers, background, _, _ = plain_case
    msi, tr = image(RADII, layers, background), T(rays)
    with torch.no_grad():
        rgb0, depth0 = msi.render(tr)
    assert rgb0.grad_fn is None
    msi.layers.requires_grad_(True)
    with torch.no_grad():
        rgb1, depth1 = msi.render(tr)
    assert rgb1.grad_fn is None and not rgb1.requires_grad and torch.equal(rgb1, rgb0)
    rgb, depth = msi.render(tr)
    assert torch.equal(rgb, rgb0) and torch.equal(depth, depth0)
    assert rgb.grad_fn is not None and rgb.requires_grad and not depth.requires_grad
    rgb.sum().backward()
    assert msi.layers.grad is not None and msi.layers.grad.shape == msi.layers.shape and msi.layers.grad.dtype == torch.float32
    assert msi.background.grad is None and float(msi.layers.grad.abs().max()) > 0
    msi.background.requires_grad_(True)   # both parameters; a non-contiguous, float64 incoming gradient
    msi.layers.grad = None
    (msi.render(tr)[0].double() * torch.ones(3, N_RAYS, device=DEV, dtype=torch.float64).t()).sum().backward()
    assert msi.background.grad.shape == msi.background.shape and float(msi.background.grad.abs().max()) > 0
    # the background alone: its gradient is the same sum of the same adds in another order, and no layer gradient is made
    only = image(RADII, layers, background)
    only.background.requires_grad_(True)
    only.render(tr)[0].sum().backward()
    assert only.layers.grad is None
    assert float((only.background.grad - msi.background.grad).abs().max()) <= 1e-5 * float(msi.background.grad.abs().max())
    half = image(RADII, layers, None).half()
    half.layers.requires_grad_(True)
    with pytest.raises(ValueError, match=r"msi\.float\(\)"):
        half.render(tr)


# ---- 5. refinement ---------------------------------------------------------------------------------------------------------------------

BH, BW, S_BAKE = 16, 32, 64
BAKE_RUNS = [3, 20, 9, 32]


def test_refinement_lowers_the_error_inside_the_headbox(golden):
    fx = golden("tiny")
    cfg = synth.SceneConfig(n_voxel=int(fx["n_voxel"]), use_envmap=True, envmap_res_H=16)
    model = make_model(cfg, synth.make_weights(cfg, seed=int(fx["seed_weights"])), DEV)
    msi = bake_msi(model, BH, BW, 4, S_BAKE, dtype=torch.float32, chunk=200, layers=BAKE_RUNS)
    kw = dict(n_coarse=S_BAKE, exp_sampling=True)
    headbox = 0.2 * float(msi.radii[0])
    held_out = headbox_rays(2048, T(msi.center), headbox, torch.Generator(device=DEV).manual_seed(977))
    with torch.no_grad():
        target = model(held_out, is_train=False, need_alpha=False, **kw)[0]

    def mse(m):
        with torch.no_grad():
            return float(torch.mean((m.render(held_out)[0] - target) ** 2))

    log = []
    refined = refine_msi(msi, model, 40, rays_per_step=4096, headbox=headbox, seed=0, render_kwargs=kw, log=log)
    before, after = mse(msi), mse(refined)
    print(f"held-out MSE against the teacher: {before:.4e} before, {after:.4e} after 40 steps of 4096 rays; "
          f"training loss {float(log[0]):.4e} -> {float(log[-1]):.4e}")
    assert after < before
    assert len(log) == 40 and all(t.is_cuda and t.dim() == 0 for t in log)
    for t in refined.parameters():
        assert bool(torch.isfinite(t).all()) and float(t[..., 3].min()) >= 0 and float(t[..., 3].max()) <= 1 and float(t[..., :3].min()) >= 0
    assert refined.layers.dtype == msi.layers.dtype and not refined.layers.requires_grad and refined.layers.data_ptr() != msi.layers.data_ptr()
    assert torch.equal(refined.radii, msi.radii) and torch.equal(refined.bounds, msi.bounds)
    assert refined.center.tobytes() == msi.center.tobytes() and refined.near_far == msi.near_far
    assert not torch.equal(refined.layers, msi.layers)
    pose = np.concatenate([np.eye(3, dtype=np.float32), (msi.center + [0.5 * headbox, 0, 0]).astype(np.float32).reshape(3, 1)], axis=1)
    rgb8, depth8 = FrameRenderer(refined, 16, 32, camera="erp").render(pose)
    assert rgb8.shape == (16, 32, 3) and rgb8.dtype == torch.uint8 and len(torch.unique(rgb8)) > 4
    # the input's texel type comes back: a half image is refined in float32 and rounded once
    with torch.no_grad():   # a caller's no_grad does not reach the loop
        half = refine_msi(msi.half(), model, 2, rays_per_step=512, headbox=headbox, render_kwargs=kw)
    assert half.layers.dtype == torch.float16 and half.background.dtype == torch.float16
