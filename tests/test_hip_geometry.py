"""Ray geometry on the GPU (csrc/ego_geometry.hip, egonerf_amd/geometry.py): ego_ray_geometry against the float64
restatement of tests/geometry_ref.py on the stage march's own samples, hand-placed points, exact zeros, bit reproducibility, a radius LUT
that does not fit the kernel's LDS copy, render_geometry end to end against the float64 oracle's own render, frames and point clouds."""
import functools

import numpy as np
import pytest
import torch

from egonerf_amd import geometry, synth
from tests import geometry_ref as gref
from tests import ray_grad_ref as rg
from tests.helpers import make_model, make_oracle

T = torch.from_numpy
pytestmark = pytest.mark.gpu


def _np2(t):
    a = np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float64)
    return a.reshape(a.shape[0], -1)


def _judge(j, what, hip, f32, f64, bound, relative=False):
    """RayJudge.check with `bound` absolute (or relative to max |f64|) instead of B_GRAD max |f64|."""
    hip, f32, f64 = _np2(hip), _np2(f32), _np2(f64)
    scale = max(float(np.abs(f64).max()), 1e-30)
    j.check(what, hip, f32, f64, factor=bound / rg.B_GRAD if relative else bound / (rg.B_GRAD * scale))


def _finish(j, n_rays):
    excused = {n for _, n in j.excused}
    assert len(excused) <= gref.MOST_EXCUSED_PER_64 * ((n_rays + 63) // 64), j.excused
    j.finish(n_rays, may_excuse=True)


def _references(cfg, w, rays, z, wt, yang, quantile=0.5):
    """{(dtype tag, normalize): geometry_reference(...)} on the given float32 samples."""
    out = {}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        o = make_oracle(cfg, w, dtype=dt)
        for normalize in (False, True):
            out[tag, normalize] = gref.geometry_reference(o, rays, z, wt, yang, normalize, quantile)
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's model, its stage march on the GPU (z, weight, coords) and the restatements on those samples: computed once, shared,
    never modified."""
    cfg, w, rays, fwd, *_ = rg.case_inputs(name)
    model = make_model(cfg, w, "cuda")
    r = rays.cuda().contiguous()
    z, wt, crd = geometry.march_samples(model, r, **fwd)
    torch.cuda.synchronize()
    yang = (crd[..., 3] != 0).cpu()
    return model, r, z, wt, crd, yang, _references(cfg, w, rays, z.cpu(), wt.cpu(), yang)


def _check_quantile(name, zq_hip, z, cum64, quantile):
    """z_quantile equals z[s*] of the float64 running sum exactly, on the rays whose running sum keeps clear of the quantile."""
    clear = ((cum64 - quantile).abs() >= gref.QUANTILE_MARGIN).all(-1)
    left_out = int((~clear).sum())
    print(f"{name}: quantile {quantile}: {left_out} of {len(clear)} rays left out; smallest margin {float((cum64 - quantile).abs().min()):.2e}")
    assert left_out <= gref.MOST_LEFT_OUT * len(clear)
    want = gref.quantile_depth(z.cpu(), cum64, quantile)
    assert torch.equal(zq_hip.cpu()[clear], want[clear])
    assert bool((zq_hip.cpu()[clear][~(cum64 >= quantile).any(-1)[clear]] == 0).all())


@pytest.mark.parametrize("name", gref.CASES)
def test_kernel_against_restatement(name):
    model, r, z, wt, crd, yang, R = _case(name)
    N, S = z.shape
    if N >= 64:
        assert 0 < int(yang.sum()) < yang.numel(), "both charts must occur"
    j = rg.RayJudge(name)
    for normalize in (False, True):
        hip = geometry.ray_geometry(model, r, z, crd, wt, normalize, 0.5, gradients=True)
        n64, a64, _, g64, cum64 = R["f64", normalize]
        n32, a32, _, g32, _ = R["f32", normalize]
        assert bool(torch.isfinite(hip.normal).all()) and float(n64.abs().max()) > 0
        _judge(j, "normalised" if normalize else "normal", hip.normal, n32, n64, gref.B_KERNEL)
    _judge(j, "acc", hip.acc[:, None], a32[:, None], a64[:, None], gref.B_KERNEL)
    _judge(j, "gradients", hip.gradients, g32, g64, gref.B_KERNEL, relative=True)
    _finish(j, N)
    _check_quantile(name, hip.z_median, z, cum64, 0.5)
    # without normalisation the length is at most acc (a convex combination of unit vectors, up to rounding)
    un = geometry.ray_geometry(model, r, z, crd, wt, False, 0.5)
    assert bool((un.normal.norm(dim=-1) <= un.acc + 1e-6).all())


@pytest.mark.parametrize("quantile", [0.1, 0.9])
def test_other_quantiles(quantile):
    model, r, z, wt, crd, yang, R = _case("tiny")
    hip = geometry.ray_geometry(model, r, z, crd, wt, True, quantile, normal=False, acc=False)
    assert hip.normal is None and hip.acc is None
    _check_quantile("tiny", hip.z_median, z, R["f64", True][4], quantile)


def _one_sample_rays(xyz, M):
    return torch.cat([T(xyz), T(synth.make_rays(M, seed=9))[:, 3:]], 1).cuda().contiguous()   # z = 0: the sample sits at the origin of its ray


def test_gradient_on_hand_placed_points():
    """24 points per chart inside cells, as one-sample rays: no kink is near, nothing is excused.  The tiny scene, and three unequal axis
    resolutions with an odd one and 4 components (12 of a row's 16 lanes idle)."""
    for cfg in (synth.SceneConfig(n_voxel=20 ** 3),
                synth.SceneConfig(n_voxel=20 ** 3, grid=[6, 5, 8], density_n_comp=(4, 4, 4), app_n_comp=(20, 20, 20))):
        w = synth.make_weights(cfg, seed=1234)
        o64, o32 = make_oracle(cfg, w, dtype=torch.float64), make_oracle(cfg, w)
        xyz, yang = rg.hand_placed_points(o64)
        M = len(yang)
        one, none = torch.ones(M), torch.zeros(M, cfg.app_dim)
        g64, _ = rg.sample_grad_reference(o64, T(xyz), T(yang), one, none)
        _, coords = rg.sample_grad_reference(o32, T(xyz), T(yang), one, none)
        scale = float(g64.abs().max())
        assert scale > 0
        model = make_model(cfg, w, "cuda")
        rays = _one_sample_rays(xyz, M)
        hip = geometry.ray_geometry(model, rays, torch.zeros(M, 1, device="cuda"), coords.float().view(M, 1, 4).contiguous().cuda(),
                                    torch.ones(M, 1, device="cuda"), False, 0.5, gradients=True)
        err = float((hip.gradients.cpu().double().view(M, 3) - g64).abs().max())
        print(f"grid {cfg.grid}: |hip - f64| {err / scale:.3e} relative to max |g64| {scale:.3e} (bound {gref.B_KERNEL:.1e})")
        assert err <= gref.B_KERNEL * scale
        # one sample of weight 1: normal = -g / |g|, acc = 1, the median is reached at sample 0 (z = 0)
        length = g64.norm(dim=-1, keepdim=True)   # 0 at a point where every plane's relu is dead: n = 0 there
        unit = torch.where(length > 0, -g64 / length.clamp(min=1e-300), torch.zeros_like(g64))
        assert float(length.max()) > 0 and float((hip.normal.cpu().double() - unit).abs().max()) <= gref.B_KERNEL
        assert torch.equal(hip.acc.cpu(), torch.ones(M)) and torch.equal(hip.z_median.cpu(), torch.zeros(M))


def _bits_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def test_exact_zeros():
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    w = synth.make_weights(cfg, seed=1234)
    o64 = make_oracle(cfg, w, dtype=torch.float64)
    # rays that start four widths of the last radius cell beyond far_r and point outwards: r^ > 1 + 2 / (n_r - 1), every r tap masked
    G = o64.r_lut.double().numpy()
    d = synth.make_rays(16, seed=5)[:, 3:]
    outside = T(np.concatenate([o64.center.numpy()[None] + d * (float(o64.far_r) + 4 * (G[-1] - G[-2])), d], 1).astype(np.float32)).cuda()
    inside = T(synth.make_rays(16, seed=7)).cuda()
    dead = dict(w)   # every plane's sum_c P_c L_c is negative: the relu of every plane is dead everywhere
    for k in w:
        if k.startswith("density_plane"):
            dead[k] = -np.abs(w[k]) - 0.1
        elif k.startswith("density_line"):
            dead[k] = np.abs(w[k]) + 0.1
    for weights, rays in ((w, outside), (dead, inside)):
        for act in ("softplus", "relu"):
            model = make_model(cfg, weights, "cuda")
            model.fea2denseAct = act
            for fwd in (dict(n_coarse=37), dict(n_coarse=16, n_fine=16, resampling=True)):
                z, wt, crd = geometry.march_samples(model, rays, **fwd)
                for normalize in (False, True):
                    g = geometry.ray_geometry(model, rays, z, crd, wt, normalize, 0.5, gradients=True)
                    assert _bits_zero(g.normal) and _bits_zero(g.gradients)
                    assert _bits_zero(g.z_median)                       # the feature is 0: sigma = softplus(shift) is tiny, or 0 with relu
                    if act == "relu":
                        # sigma = relu(0) = 0: no weight at all (the march writes them as -0.0: -expm1(-0)); acc is +0.0 bit for bit
                        assert bool((wt == 0).all()) and _bits_zero(g.acc)
                    else:
                        assert float(g.acc.max()) < 0.5
                same = geometry.render_geometry(model, rays, **fwd)
                assert _bits_zero(same.normal) and _bits_zero(same.z_median)


def test_bits():
    model, r, z, wt, crd, _, _ = _case("tiny_resampled")
    wz = wt.clone()
    wz[:, ::3] = 0            # exact zeros among live samples: the skipped samples
    wz[5] = 0                 # a ray without any live sample
    for weights in (wt, wz):
        a = geometry.ray_geometry(model, r, z, crd, weights, True, 0.5, gradients=True)
        b = geometry.ray_geometry(model, r, z, crd, weights, True, 0.5, gradients=True)
        c = geometry.ray_geometry(model, r, z, crd, weights, True, 0.5)                        # grad_out null: w == 0 samples are not gathered
        d = geometry.ray_geometry(model, r, z, crd, weights, True, 0.5, acc=False, z_quantile=False)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert c.gradients is None and torch.equal(c.normal, a.normal) and torch.equal(c.acc, a.acc) and torch.equal(c.z_median, a.z_median)
        assert torch.equal(d.normal, a.normal)
        un_a = geometry.ray_geometry(model, r, z, crd, weights, False, 0.5, gradients=True)
        un_c = geometry.ray_geometry(model, r, z, crd, weights, False, 0.5)
        assert torch.equal(un_a.normal, un_c.normal)
    full = geometry.ray_geometry(model, r, z, crd, wt, True, 0.5, gradients=True)
    zeroed = geometry.ray_geometry(model, r, z, crd, wz, True, 0.5, gradients=True)
    assert torch.equal(full.gradients, zeroed.gradients)      # the raw gradient does not depend on the weights
    assert _bits_zero(zeroed.normal[5]) and _bits_zero(zeroed.acc[5:6]) and _bits_zero(zeroed.z_median[5:6])
    # the sum over the live samples only, in the restatement
    cfg, w, rays, *_ = rg.case_inputs("tiny_resampled")
    n64 = gref.geometry_reference(make_oracle(cfg, w, dtype=torch.float64), rays, z.cpu(), wz.cpu(), (crd[..., 3] != 0).cpu(), False, 0.5)[0]
    un = geometry.ray_geometry(model, r, z, crd, wz, False, 0.5)
    assert float((un.normal.cpu().double() - n64).abs().max()) <= gref.B_KERNEL


def test_radius_lut_beyond_the_lds_copy():
    """N_r = 1100: the LUT (N_r + 1 entries) is walked in memory.  The march takes no LUT of that length, so the samples are the float32
    oracle's own (distances, weights, normalised coordinates and charts), and the kernel is judged on them like a case."""
    cfg = synth.SceneConfig(n_voxel=20 ** 3, grid=[1100, 5, 6], density_n_comp=(4, 4, 4), app_n_comp=(4, 4, 4))
    w = synth.make_weights(cfg, seed=1234)
    rays = T(synth.make_rays(70, seed=7))
    fwd = dict(n_coarse=19)
    o32 = make_oracle(cfg, w)
    z, wt, yang = gref.oracle_samples(o32, rays, fwd)
    with torch.no_grad():
        xyz = rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]
        c7n = o32.normalize_coord(o32.from_cartesian(xyz, yang.long()), downsample=None)
        coords = torch.cat([torch.where(yang[..., None], c7n[..., 3:6], c7n[..., 0:3]), yang[..., None].float()], -1).contiguous()
    assert 0 < int(yang.sum()) < yang.numel()
    R = _references(cfg, w, rays, z, wt, yang)
    model = make_model(cfg, w, "cuda")
    j = rg.RayJudge("lut_1101")
    for normalize in (False, True):
        hip = geometry.ray_geometry(model, rays.cuda(), z.cuda(), coords.cuda(), wt.cuda(), normalize, 0.5, gradients=True)
        _judge(j, "normalised" if normalize else "normal", hip.normal, R["f32", normalize][0], R["f64", normalize][0], gref.B_KERNEL)
    _judge(j, "acc", hip.acc[:, None], R["f32", True][1][:, None], R["f64", True][1][:, None], gref.B_KERNEL)
    _judge(j, "gradients", hip.gradients, R["f32", True][3], R["f64", True][3], gref.B_KERNEL, relative=True)
    assert float(R["f64", True][3].abs().max()) > 0
    _finish(j, rays.shape[0])
    _check_quantile("lut_1101", hip.z_median, z, R["f64", True][4], 0.5)


@pytest.mark.parametrize("name", gref.CASES)
def test_render_geometry_end_to_end(name):
    """render_geometry on the factored march against the float64 oracle's OWN render: its weights, distances and charts."""
    cfg, w, rays, fwd, *_ = rg.case_inputs(name)
    model = make_model(cfg, w, "cuda")
    model.dense_density = False
    o64, o32 = make_oracle(cfg, w, dtype=torch.float64), make_oracle(cfg, w)
    z64, w64, y64 = gref.oracle_samples(o64, rays, fwd)
    z32, w32, y32 = gref.oracle_samples(o32, rays, fwd)
    # a sample within a few float32 ulps of pi of a chart border lands on either chart, whose tables are independent: such rays are left out
    r64 = rays.double()
    margin = o64.yin_margin(r64[:, None, :3] + r64[:, None, 3:6] * z64[..., None]).abs().amin(-1)
    keep = margin >= 2e-6
    assert int((~keep).sum()) <= gref.MOST_LEFT_OUT * len(keep), margin
    j = rg.RayJudge(name)
    for normalize in (False, True):
        hip = model.render_geometry(rays.cuda(), normalize=normalize, **fwd)
        assert hip.gradients is None
        n64, a64, *_ = gref.geometry_reference(o64, rays, z64, w64, y64, normalize, 0.5)
        n32, a32, *_ = gref.geometry_reference(o32, rays, z32, w32, y32, normalize, 0.5)
        _judge(j, "normalised" if normalize else "normal", hip.normal[keep.cuda()], n32[keep], n64[keep], gref.B_END_TO_END)
    _judge(j, "acc", hip.acc[keep.cuda(), None], a32[keep, None], a64[keep, None], gref.B_END_TO_END)
    _finish(j, rays.shape[0])


def test_render_geometry_with_the_dense_route():
    """dense_density on (the default) on the tuned-shape tiny scene: the weights come from the baked node grid, the normals from the
    factored tables; render_geometry returns what the kernel returns on that march's samples (judged in test_kernel_against_restatement)."""
    model, r, z, wt, crd, _, _ = _case("tiny_resampled")
    cfg, w, rays, fwd, *_ = rg.case_inputs("tiny_resampled")
    assert model._dense_wanted() and model.scene().density_dense
    got = geometry.render_geometry(model, r, sample_gradients=True, **fwd)
    want = geometry.ray_geometry(model, r, z, crd, wt, True, 0.5, gradients=True)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert got.gradients.shape == (r.shape[0], z.shape[1], 3)


def _pose(k):
    from egonerf_amd.poses import rotate
    eye = torch.eye(3)
    axis = torch.tensor([[0.3 - 0.2 * k, 0.4, 0.1 * k]])
    R = torch.stack([rotate(axis, eye[c:c + 1])[0] for c in range(3)], -1)
    return torch.cat([R, torch.tensor([[0.1 * k], [-0.05], [0.02]])], -1).numpy().astype(np.float32)


@pytest.mark.parametrize("H,W,camera,focal", [(8, 16, "erp", None), (12, 12, "pinhole", 9.0)])
def test_geometry_frame(H, W, camera, focal):
    from egonerf_amd.camera import camera_rays
    model = _case("tiny_resampled")[0]
    kw = dict(n_coarse=16, n_fine=16, resampling=True)
    pose = _pose(1)
    fr = geometry.geometry_frame(model, H, W, pose, camera=camera, focal=focal, chunk=50, **kw)     # 50 divides neither frame
    rays = camera_rays(H, W, pose, model=camera, focal=focal)
    whole = geometry.render_geometry(model, rays, **kw)
    assert fr["normal"].shape == (H, W, 3) and fr["acc"].shape == (H, W) and fr["z_median"].shape == (H, W) and fr["points"].shape == (H, W, 3)
    assert torch.equal(fr["normal"].view(-1, 3), whole.normal) and torch.equal(fr["acc"].view(-1), whole.acc)
    assert torch.equal(fr["z_median"].view(-1), whole.z_median)
    assert torch.equal(fr["points"].view(-1, 3), rays[:, :3] + rays[:, 3:6] * whole.z_median[:, None])
    img = geometry.normal_image(fr["normal"])
    assert img.dtype == torch.uint8 and img.shape == (H, W, 3)
    want = ((fr["normal"] * 0.5 + 0.5).clamp(0, 1) * 255).to(torch.uint8)
    assert torch.equal(img, want)


def test_export_point_cloud(tmp_path):
    from egonerf_amd.camera import camera_rays
    model = _case("tiny_resampled")[0]
    kw = dict(n_coarse=16, n_fine=16, resampling=True)
    H, W, poses, min_acc = 8, 16, [_pose(0), _pose(2)], 0.6
    path = tmp_path / "cloud.ply"
    n = geometry.export_point_cloud(model, poses, H, W, path, min_acc=min_acc, **kw)
    xyz, nrm, rgb = [], [], []
    for pose in poses:
        fr = geometry.geometry_frame(model, H, W, pose, **kw)
        keep = (fr["acc"] >= min_acc).view(-1)
        with torch.no_grad():
            col = model(camera_rays(H, W, pose), exp_sampling=True, need_alpha=False, **kw)[0]
        xyz.append(fr["points"].view(-1, 3)[keep])
        nrm.append(fr["normal"].view(-1, 3)[keep])
        rgb.append((col[keep].clamp(0, 1) * 255).to(torch.uint8))
    xyz, nrm, rgb = (torch.cat(t).cpu().numpy() for t in (xyz, nrm, rgb))
    assert 0 < n == len(xyz) < 2 * H * W
    back = geometry.read_ply(path)
    assert np.array_equal(back["xyz"], xyz) and np.array_equal(back["normal"], nrm) and np.array_equal(back["rgb"], rgb)
    assert geometry.export_point_cloud(model, poses, H, W, tmp_path / "s.ply", min_acc=min_acc, stride=2, **kw) <= n
    with pytest.raises(ValueError, match="below the quantile"):
        geometry.export_point_cloud(model, poses, H, W, path, min_acc=0.3, **kw)
