"""GPU: stereo panoramas and supersampled frames (egonerf_amd/camera.py, csrc/ego_camera.hip: ego_camera_rays_ex, ego_resolve_frame) -
the eyes' origins against a float64 evaluation of the omnidirectional-stereo formula and against their own geometry, sub-pixel samples
against the rays of the fine camera bit for bit, the resolve kernel against a float32 numpy restatement byte for byte, and
FrameRenderer's top-bottom and supersampled frames against camera_rays -> model -> finish_frame with the same chunk boundaries."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib
from egonerf_amd.camera import FrameRenderer, camera_rays, depth_range, finish_frame
from tests import camera_ref as ref
from tests.test_hip_camera_path import KW_RESAMPLE, bits, env_model, make_poses

pytestmark = pytest.mark.gpu
DEV = "cuda"
IPD = 0.13


def a_pose():
    """A non-trivial rotation (QR of a seeded normal matrix) and translation."""
    p = make_poses(1, seed=17)[0]
    p[:, 3] = np.asarray([0.31, -0.22, 0.17], np.float32)
    return p


# ---- 1. omnidirectional-stereo rays ------------------------------------------------------------------------------------------------

def ods_origins_f64(H, W, pose, ipd, sign):
    """o = R o_cam + t with o_cam = sign * ipd / 2 * (cos phi, 0, -sin phi), phi = (1 - 2 (col + 0.5) / W) pi, in float64."""
    col = np.tile(np.arange(W, dtype=np.float64), H)
    phi = (1.0 - 2.0 * (col + 0.5) / W) * np.pi
    o_cam = sign * ipd / 2 * np.stack([np.cos(phi), np.zeros_like(phi), -np.sin(phi)], -1)
    R, t = pose[:, :3].astype(np.float64), pose[:, 3].astype(np.float64)
    return o_cam @ R.T + t


def test_ods_rays_origins_directions_and_geometry():
    H, W, pose = 8, 16, a_pose()
    R, t = pose[:, :3].astype(np.float64), pose[:, 3].astype(np.float64)
    tol = 1e-6 * (np.abs(t).max() + IPD / 2)
    centre = camera_rays(H, W, pose, model="erp", device=DEV)
    eyes = {}
    for eye, sign in (("left", -1.0), ("right", 1.0)):
        rays = camera_rays(H, W, pose, model="erp", eye=eye, ipd=IPD, device=DEV)
        assert rays.shape == (H * W, 6)
        # (a) the directions are the centre eye's
        assert np.array_equal(bits(rays[:, 3:]), bits(centre[:, 3:])), eye
        o = rays[:, :3].cpu().numpy().astype(np.float64)
        d = rays[:, 3:].cpu().numpy().astype(np.float64)
        # (b) the origins against the formula
        err = np.abs(o - ods_origins_f64(H, W, pose, IPD, sign)).max()
        print(f"{eye}: max |o - formula| = {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol
        # (c) on the viewing circle, at right angles to the horizontal part of the direction
        off = (o - t) @ R                                        # R^T (o - t): the offset in camera space
        d_cam = d @ R
        d_h = d_cam * np.asarray([1.0, 0.0, 1.0])
        radius = np.abs(np.linalg.norm(o - t, axis=1) - IPD / 2).max()
        dot = np.abs((off * d_h).sum(-1)).max()
        print(f"{eye}: max | |o - t| - ipd / 2 | = {radius:.3e}, max |(o - t) . d_h| = {dot:.3e}")
        assert radius <= tol and dot <= tol
        eyes[eye] = (o, d_h)
        # (e) a window equals the same rows of the whole frame
        win = camera_rays(H, W, pose, model="erp", eye=eye, ipd=IPD, first=37, count=50, device=DEV)
        assert win.shape == (50, 6) and np.array_equal(bits(win), bits(rays[37:87]))
    # (c) right - left = ipd * (forward x up) with forward the horizontal viewing direction and up = +y of the camera
    fwd = eyes["left"][1] / np.linalg.norm(eyes["left"][1], axis=1, keepdims=True)
    want = IPD * np.cross(fwd, np.asarray([0.0, 1.0, 0.0])) @ R.T
    base = np.abs((eyes["right"][0] - eyes["left"][0]) - want).max()
    print(f"max |(o_right - o_left) - ipd forward x up| = {base:.3e} (tolerance {tol:.3e})")
    assert base <= tol
    # (d) no distance between the eyes: the centre rays
    for eye in ("left", "right"):
        zero = camera_rays(H, W, pose, model="erp", eye=eye, ipd=0.0, device=DEV)
        assert bool((zero == centre).all())


def _rays_ex(H, W, pose, model=_lib.CAM_ERP, eye=0, half_ipd=0.0, ss=1, focal=(0.0, 0.0), center=(0.0, 0.0), first=0, count=None):
    """ego_camera_rays_ex as it is (H, W, focal, center: the FINE camera's)."""
    count = (H // ss) * (W // ss) - first if count is None else count
    out = torch.empty(count * ss * ss, 6, device=DEV)
    dev_pose = torch.from_numpy(np.ascontiguousarray(pose.reshape(-1)[:12])).to(DEV)
    _lib.check(_lib.load().ego_camera_rays_ex(model, H, W, focal[0], focal[1], center[0], center[1], 1, dev_pose.data_ptr(), first, count,
                                              eye, half_ipd, ss, out.data_ptr(), _lib.stream_handle()), "ego_camera_rays_ex")
    return out


def test_the_new_entry_point_at_its_defaults_is_camera_rays():
    H, W, pose = 8, 16, a_pose()
    centre = camera_rays(H, W, pose, model="erp", device=DEV)
    assert np.array_equal(bits(_rays_ex(H, W, pose)), bits(centre))                               # eye == 0, ss == 1
    assert np.array_equal(bits(_rays_ex(H, W, pose, eye=_lib.EYE_LEFT, half_ipd=0.0)), bits(centre))
    assert np.array_equal(bits(_rays_ex(H, W, pose, half_ipd=0.065)), bits(centre))               # the centre eye ignores half_ipd
    pin = camera_rays(H, W, pose, model="pinhole", focal=(7.3, 6.9), center=(8.4, 3.4), device=DEV)
    assert np.array_equal(bits(_rays_ex(H, W, pose, model=_lib.CAM_PINHOLE, focal=(7.3, 6.9), center=(8.4, 3.4))), bits(pin))


# ---- 2. sub-pixel samples ------------------------------------------------------------------------------------------------------------

def unpermute(rays, H, W, ss):
    """[H W ss^2, 6] in sample order -> [(ss H) (ss W), 6] in the fine camera's row-major order."""
    return rays.view(H, W, ss, ss, 6).permute(0, 2, 1, 3, 4).reshape(H * ss * W * ss, 6)


@pytest.mark.parametrize("H,W,ss", [(4, 8, 2), (2, 4, 3)])
@pytest.mark.parametrize("model", ["erp", "pinhole", "pinhole_blender"])
def test_sub_pixel_samples_are_the_fine_cameras_rays(model, H, W, ss):
    pose, focal, center = a_pose(), (7.3, 6.9), (4.2, 1.7)
    got = camera_rays(H, W, pose, model=model, focal=focal, center=center, supersample=ss, device=DEV)
    assert got.shape == (H * W * ss * ss, 6)
    if model == "erp":
        fine = camera_rays(ss * H, ss * W, pose, model="erp", device=DEV)
    else:
        fine = camera_rays(ss * H, ss * W, pose, model=model, focal=tuple(ss * f for f in focal), center=tuple(ss * c for c in center), device=DEV)
    assert np.array_equal(bits(unpermute(got, H, W, ss)), bits(fine))
    # the default centre scales as well: (W / 2, H / 2) of the output frame is the fine camera's default
    if model != "erp":
        got = camera_rays(H, W, pose, model=model, focal=focal, supersample=ss, device=DEV)
        fine = camera_rays(ss * H, ss * W, pose, model=model, focal=tuple(ss * f for f in focal), device=DEV)
        assert np.array_equal(bits(unpermute(got, H, W, ss)), bits(fine))
    # a window of output pixels is the same rows: the samples of a pixel are contiguous
    first, count = 5, H * W - 6
    win = camera_rays(H, W, pose, model=model, focal=focal, center=center, supersample=ss, first=first, count=count, device=DEV)
    whole = camera_rays(H, W, pose, model=model, focal=focal, center=center, supersample=ss, device=DEV)
    assert np.array_equal(bits(win), bits(whole[first * ss * ss:(first + count) * ss * ss]))


def test_sub_pixel_samples_of_an_eye_and_bad_factors():
    H, W, ss, pose = 4, 8, 2, a_pose()
    for eye in ("left", "right"):
        got = camera_rays(H, W, pose, eye=eye, ipd=IPD, supersample=ss, device=DEV)
        fine = camera_rays(ss * H, ss * W, pose, eye=eye, ipd=IPD, device=DEV)
        assert np.array_equal(bits(unpermute(got, H, W, ss)), bits(fine))
    for bad in (0, 5, -1):
        with pytest.raises(ValueError):
            camera_rays(H, W, pose, supersample=bad, device=DEV)
    with pytest.raises(RuntimeError):
        _rays_ex(9, 16, pose, ss=2)                                    # a fine camera that is no multiple of ss
    with pytest.raises(RuntimeError):
        _rays_ex(8, 16, pose, ss=5)
    with pytest.raises(RuntimeError):
        camera_rays(H, W, pose, model="pinhole", focal=5.0, eye="left", ipd=IPD, device=DEV)


# ---- 3. resolve ----------------------------------------------------------------------------------------------------------------------

NEAR_FAR = [0.1, 15.0]
RH, RW = 4, 8


def resolve_ref(rgb, depth, near_far, palette, ss):
    """rgb [n, ss^2, 3], depth [n, ss^2] float32 -> (rgb8 [n, 3], idx8 [n], depth8 [n, 3]): clamp (a NaN colour is 0) / nan_to_num per
    sample, float32 sum in sample order, one division by float32(ss^2), then finish_frame's arithmetic (tests/camera_ref.py)."""
    assert rgb.dtype == np.float32 and depth.dtype == np.float32
    c = np.where(np.isnan(rgb), np.float32(0), np.clip(rgb, np.float32(0), np.float32(1))).astype(np.float32)
    x = np.nan_to_num(depth)
    acc, dacc = c[:, 0], x[:, 0]
    with np.errstate(over="ignore"):
        for s in range(1, ss * ss):
            acc, dacc = acc + c[:, s], dacc + x[:, s]
        acc, dacc = acc / np.float32(ss * ss), dacc / np.float32(ss * ss)
    assert acc.dtype == np.float32 and dacc.dtype == np.float32
    rgb8 = (acc * np.float32(255)).astype(np.uint8)
    _, idx8, depth8 = ref.finish_ref(np.zeros_like(acc), dacc, near_far, palette)
    return rgb8, idx8, depth8


def resolve_inputs(ss):
    g = np.random.default_rng(100 + ss)
    n, s2 = RH * RW, ss * ss
    rgb = g.uniform(-0.3, 1.3, (n, s2, 3)).astype(np.float32)
    depth = g.uniform(0.02, 17.0, (n, s2)).astype(np.float32)
    rgb[0] = 1.0                                  # every sample at 1: the average is exactly 1 -> 255
    rgb[1] = -2.0
    rgb[2, 0] = np.nan                            # one NaN sample counts as 0
    rgb[3, :, 1] = np.nan
    rgb[4, 1:] = 7.5                              # above 1
    rgb[5] = np.float32(128 / 255.0)
    depth[0] = 0.05                               # below near
    depth[1] = 16.0                               # above far
    depth[2, 0] = np.nan
    depth[3] = np.nan
    depth[4, :2] = np.inf                         # the sum overflows
    depth[5, 0], depth[5, -1] = np.inf, -np.inf   # +-FLT_MAX cancel (one sample: -inf)
    depth[6, -1] = -np.inf
    depth[7] = 15.0
    assert (rgb < 0).any() and (rgb > 1).any() and (depth < NEAR_FAR[0]).any() and (depth > NEAR_FAR[1]).any()
    return rgb, depth


def _resolve(rgb, depth, first, count, ss, pal, sbs, bufs):
    """ego_resolve_frame as it is, for `count` pixels from `first` on of the RH x RW frame in `bufs`."""
    mi, den = depth_range(NEAR_FAR)
    _lib.check(_lib.load().ego_resolve_frame(rgb.data_ptr(), depth.data_ptr(), first, count, RH, RW, ss, float(mi), float(den), _lib.ptr(pal),
                                             int(sbs), bufs[0].data_ptr(), bufs[1].data_ptr() if len(bufs) > 1 else None,
                                             _lib.stream_handle()), "ego_resolve_frame")


@pytest.mark.parametrize("ss", [2, 4])
def test_resolve_equals_the_numpy_restatement_in_all_layouts(ss):
    rgb, depth = resolve_inputs(ss)
    pal = np.random.default_rng(2).integers(0, 256, (256, 3)).astype(np.uint8)
    want8, widx, wpal = resolve_ref(rgb, depth, NEAR_FAR, pal, ss)
    want8, widx, wpal = want8.reshape(RH, RW, 3), widx.reshape(RH, RW), wpal.reshape(RH, RW, 3)
    assert want8[0, 0].tolist() == [255, 255, 255] and want8[0, 1].tolist() == [0, 0, 0] and widx[0, 0] == 0 and widx[0, 1] == 255
    assert widx[0, 4] == 255 and len(np.unique(widx)) > 8 and len(np.unique(want8)) > 16
    t_rgb = torch.from_numpy(rgb).to(DEV).view(RH, RW, ss * ss, 3)
    t_depth = torch.from_numpy(depth).to(DEV).view(RH, RW, ss * ss)
    rgb8, idx8 = finish_frame(t_rgb, t_depth, NEAR_FAR, palette=False, supersample=ss)
    assert rgb8.shape == (RH, RW, 3) and idx8.shape == (RH, RW) and rgb8.dtype == torch.uint8
    assert np.array_equal(rgb8.cpu().numpy(), want8) and np.array_equal(idx8.cpu().numpy(), widx)
    rgb8, depth8 = finish_frame(t_rgb, t_depth, NEAR_FAR, palette=pal, supersample=ss)
    assert np.array_equal(rgb8.cpu().numpy(), want8) and np.array_equal(depth8.cpu().numpy(), wpal)
    rgbd = finish_frame(t_rgb, t_depth, NEAR_FAR, palette=pal, side_by_side=True, supersample=ss)
    assert rgbd.shape == (RH, 2 * RW, 3) and np.array_equal(rgbd.cpu().numpy(), np.concatenate((want8, wpal), axis=1))
    # flat input, flat output
    f8, fi = finish_frame(t_rgb.reshape(-1, 3), t_depth.reshape(-1), NEAR_FAR, palette=False, supersample=ss)
    assert np.array_equal(f8.cpu().numpy(), want8.reshape(-1, 3)) and np.array_equal(fi.cpu().numpy(), widx.reshape(-1))


def test_resolve_of_one_sample_is_finish_frame():
    rgb, depth = resolve_inputs(1)
    pal = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (256, 3)).astype(np.uint8)).to(DEV)
    t_rgb, t_depth = torch.from_numpy(rgb).to(DEV).view(RH, RW, 3), torch.from_numpy(depth).to(DEV).view(RH, RW)
    n = RH * RW
    for palette, sbs in ((False, False), (pal, False), (pal, True)):
        want = finish_frame(t_rgb, t_depth, NEAR_FAR, palette=palette, side_by_side=sbs)
        want = [want] if sbs else list(want)
        got = [torch.zeros_like(w) for w in want]
        _resolve(t_rgb, t_depth, 0, n, 1, None if palette is False else pal, sbs, got)
        for w, g_ in zip(want, got):
            assert torch.equal(w, g_)


@pytest.mark.parametrize("ss", [2, 4])
@pytest.mark.parametrize("first,count", [(5, 13), (3, 2), (8, 9), (0, 31)])
def test_resolve_of_a_window_off_the_groups_of_four(ss, first, count):
    """The same bytes as the whole frame at the window's pixels, nothing written elsewhere."""
    rgb, depth = resolve_inputs(ss)
    pal = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (256, 3)).astype(np.uint8)).to(DEV)
    t_rgb = torch.from_numpy(rgb).to(DEV).view(RH, RW, ss * ss, 3)
    t_depth = torch.from_numpy(depth).to(DEV).view(RH, RW, ss * ss)
    s2 = ss * ss
    w_rgb = t_rgb.reshape(-1, 3)[first * s2:(first + count) * s2].contiguous()
    w_depth = t_depth.reshape(-1)[first * s2:(first + count) * s2].contiguous()
    inside = torch.zeros(RH * RW, dtype=torch.bool, device=DEV)
    inside[first:first + count] = True
    inside = inside.view(RH, RW)
    for palette, sbs in ((False, False), (pal, False), (pal, True)):
        whole = finish_frame(t_rgb, t_depth, NEAR_FAR, palette=palette, side_by_side=sbs, supersample=ss)
        whole = [whole] if sbs else list(whole)
        got = [torch.full_like(w, 0xAB) for w in whole]
        _resolve(w_rgb, w_depth, first, count, ss, None if palette is False else pal, sbs, got)
        for w, g_ in zip(whole, got):
            if sbs:
                mask = torch.cat((inside, inside), dim=1)
            else:
                mask = inside
            mask = mask if w.dim() == 2 else mask.unsqueeze(-1).expand_as(w)
            assert torch.equal(g_[mask], w[mask])
            assert bool((g_[~mask] == 0xAB).all())


# ---- 4. frames -----------------------------------------------------------------------------------------------------------------------

FH, FW, CHUNK = 8, 16, 48


def _eye_by_hand(model, pose, eye, ss, **finish):
    """camera_rays(eye) -> model -> finish_frame with FrameRenderer's chunk boundaries."""
    n, rgbs, depths = FH * FW, [], []
    with torch.no_grad():
        for first in range(0, n, CHUNK):
            rays = camera_rays(FH, FW, pose, model="erp", eye=eye, ipd=IPD, supersample=ss, first=first, count=min(CHUNK, n - first), device=DEV)
            rgb, depth = model(rays, need_alpha=False, **KW_RESAMPLE)[:2]
            rgbs.append(rgb.clone())
            depths.append(depth.clone())
    rgb, depth = torch.cat(rgbs), torch.cat(depths)
    if ss == 1:
        return finish_frame(rgb.view(FH, FW, 3), depth.view(FH, FW), model.near_far, **finish)
    return finish_frame(rgb.view(FH, FW, ss * ss, 3), depth.view(FH, FW, ss * ss), model.near_far, supersample=ss, **finish)


@pytest.mark.parametrize("ss", [1, 2])
def test_top_bottom_frame_is_the_two_eyes_frames(ss):
    model, pose = env_model(), make_poses(1, seed=21)[0]
    fr = FrameRenderer(model, FH, FW, stereo="top_bottom", ipd=IPD, chunk=CHUNK, supersample=ss, **KW_RESAMPLE)
    rgb8, depth8 = fr.render(pose)
    assert rgb8.shape == (2 * FH, FW, 3) and depth8.shape == (2 * FH, FW, 3) and rgb8.dtype == torch.uint8
    left, right = _eye_by_hand(model, pose, "left", ss), _eye_by_hand(model, pose, "right", ss)
    assert torch.equal(rgb8[:FH], left[0]) and torch.equal(depth8[:FH], left[1])
    assert torch.equal(rgb8[FH:], right[0]) and torch.equal(depth8[FH:], right[1])
    # the two eyes see the near field from different places
    assert not torch.equal(rgb8[:FH], rgb8[FH:])
    assert len(torch.unique(rgb8)) > 16
    # the index image and the side-by-side layout of the same frame
    r2, idx8 = FrameRenderer(model, FH, FW, stereo="top_bottom", ipd=IPD, chunk=CHUNK, supersample=ss, palette=False, **KW_RESAMPLE).render(pose)
    assert idx8.shape == (2 * FH, FW) and torch.equal(r2, rgb8) and torch.equal(idx8, depth8[..., 0])
    rgbd = FrameRenderer(model, FH, FW, stereo="top_bottom", ipd=IPD, chunk=CHUNK, supersample=ss, side_by_side=True, **KW_RESAMPLE).render(pose)
    assert rgbd.shape == (2 * FH, 2 * FW, 3) and torch.equal(rgbd, torch.cat((rgb8, depth8), dim=1))
    host = fr.render_to_host(pose)
    assert np.array_equal(host[0], rgb8.cpu().numpy()) and np.array_equal(host[1], depth8.cpu().numpy())


def test_supersampled_mono_frame():
    model, pose = env_model(), make_poses(1, seed=21)[0]
    rgb8, depth8 = FrameRenderer(model, FH, FW, chunk=CHUNK, supersample=2, **KW_RESAMPLE).render(pose)
    n, rgbs, depths = FH * FW, [], []
    with torch.no_grad():
        for first in range(0, n, CHUNK):
            rays = camera_rays(FH, FW, pose, supersample=2, first=first, count=min(CHUNK, n - first), device=DEV)
            rgb, depth = model(rays, need_alpha=False, **KW_RESAMPLE)[:2]
            rgbs.append(rgb.clone())
            depths.append(depth.clone())
    want = finish_frame(torch.cat(rgbs).view(FH, FW, 4, 3), torch.cat(depths).view(FH, FW, 4), model.near_far, supersample=2)
    assert rgb8.shape == (FH, FW, 3) and torch.equal(rgb8, want[0]) and torch.equal(depth8, want[1])
    plain = FrameRenderer(model, FH, FW, chunk=CHUNK, **KW_RESAMPLE).render(pose)
    assert not torch.equal(plain[0], rgb8)                             # four rays per pixel are not one


@pytest.mark.parametrize("ss", [1, 2])
def test_captured_stereo_frame_equals_the_eager_frame(ss):
    model, poses = env_model(), make_poses(2, seed=31)
    kw = dict(stereo="top_bottom", ipd=IPD, chunk=CHUNK, supersample=ss, **KW_RESAMPLE)
    eager, graphed = FrameRenderer(model, FH, FW, **kw), FrameRenderer(model, FH, FW, graph=True, **kw)
    want = [tuple(t.clone() for t in eager.render(p)) for p in poses]
    got = [graphed.render(p) for p in poses]
    for w, g_ in zip(want, got):
        assert torch.equal(w[0], g_[0]) and torch.equal(w[1], g_[1])
    assert not torch.equal(want[0][0], want[1][0])
    host = graphed.render_to_host(poses[0])
    assert np.array_equal(host[0], want[0][0].cpu().numpy()) and np.array_equal(host[1], want[0][1].cpu().numpy())


def test_render_path_yields_the_stereo_frames_in_order():
    model, poses = env_model(), make_poses(3, seed=41)
    fr = FrameRenderer(model, FH, FW, stereo="top_bottom", ipd=IPD, chunk=CHUNK, supersample=2, side_by_side=True, **KW_RESAMPLE)
    want = [fr.render_to_host(p).copy() for p in poses]
    got = [frame.copy() for frame in fr.render_path(poses)]
    assert len(got) == 3 and got[0].shape == (2 * FH, 2 * FW, 3)
    for k, (w, g_) in enumerate(zip(want, got)):
        assert np.array_equal(w, g_), f"frame {k}"
    assert not np.array_equal(want[0], want[1])


def test_evaluation_path_writes_the_taller_frames(tmp_path):
    import types
    from PIL import Image
    from egonerf_amd.camera import evaluation_path
    model, poses = env_model(), make_poses(2, seed=51)
    ds = types.SimpleNamespace(img_wh=(FW, FH), near_far=[0.01, 15.0])
    with pytest.warns(UserWarning, match="mp4"):
        frames = evaluation_path(ds, model, poses, None, savePath=str(tmp_path / "out"), prtx="p_", exp_sampling=True, stereo="top_bottom",
                                 ipd=IPD, supersample=2, n_coarse=32, n_fine=32, resampling=True, chunk=CHUNK)
    assert len(frames) == 2 and all(f.shape == (2 * FH, 2 * FW, 3) and f.dtype == np.uint8 for f in frames)
    for k, f in enumerate(frames):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"p_{k:03d}.png")), f[:, :FW])
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "rgbd" / f"p_{k:03d}.png")), f)
    fr = FrameRenderer(model, FH, FW, near_far=ds.near_far, side_by_side=True, chunk=CHUNK, stereo="top_bottom", ipd=IPD, supersample=2,
                       exp_sampling=True, n_coarse=32, n_fine=32, resampling=True)
    assert np.array_equal(fr.render_to_host(poses[1]), frames[1])
