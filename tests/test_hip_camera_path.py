"""GPU: camera paths (egonerf_amd/camera.py, csrc/ego_camera.hip) - pinhole rays against the reference's (tests/golden/camera_rays.npz,
tools/capture_camera_golden.py), ERP rays against ego_erp_rays bit for bit, the pose read from device memory, the frame products
against their numpy restatement (tests/camera_ref.py) byte for byte, FrameRenderer against volume_renderer + finish_frame, the
captured frame against the eager one, render_path's double-buffered hand-over, and evaluation_path's files."""
import types

import numpy as np
import pytest
import torch

from egonerf_amd import synth
from egonerf_amd.renderer import FrameRenderer, camera_rays, erp_rays, evaluation_path, finish_frame, volume_renderer
from tests import camera_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
KW_RESAMPLE = dict(n_coarse=32, n_fine=32, exp_sampling=True, resampling=True, use_coarse_sample=True)
KW_PLAIN = dict(n_coarse=64, exp_sampling=True)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_poses(K, seed=3, extent=0.2):
    g = np.random.default_rng(seed)
    q, _ = np.linalg.qr(g.standard_normal((K, 3, 3)))
    p = np.zeros((K, 3, 4), np.float32)
    p[:, :, :3] = q
    p[:, :, 3] = g.uniform(-extent, extent, (K, 3))
    return p


_MODEL = {}


def env_model():
    if "m" not in _MODEL:
        cfg = synth.SceneConfig(n_voxel=40 ** 3, use_envmap=True, envmap_res_H=64)
        _MODEL["m"] = synth.build_model(cfg, synth.make_weights(cfg, seed=1234), DEV)
    return _MODEL["m"]


# ---- 1. pinhole rays against the fixture -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["small", "big"])
@pytest.mark.parametrize("model", ["pinhole", "pinhole_blender"])
def test_pinhole_rays_against_the_reference(golden, case, model):
    fx = golden("camera_rays")
    H, W, focal, index = int(fx[f"{case}/H"]), int(fx[f"{case}/W"]), fx[f"{case}/focal"], fx[f"{case}/index"]
    center = None if np.isnan(fx[f"{case}/center"]).any() else fx[f"{case}/center"]
    dirs, poses, want = fx[f"{case}/dirs/{model}"], fx[f"{case}/poses"], fx[f"{case}/rays/{model}"]
    for k, pose in enumerate(poses):
        got = camera_rays(H, W, pose, model=model, focal=focal, center=center, device=DEV).cpu().numpy()[index]
        assert np.array_equal(bits(got[:, :3]), bits(want[k][:, :3])), "origins"
        if k == 0:   # R = I: the dot product adds exact zeros only, the world direction IS the camera-space direction
            assert np.array_equal(bits(got[:, 3:]), bits(dirs)), "camera-space direction"
            assert np.array_equal(bits(got[:, 3:]), bits(want[0][:, 3:]))
        # ATen's [HW, 3] @ [3, 3] may fuse multiplies or reorder the three-term sum: |delta| <= 4 * 2^-24 * sum_k |dir_k R_jk|, per element
        R = pose[:, :3].astype(np.float64)
        bound = 4 * EPS * (np.abs(dirs.astype(np.float64))[:, None, :] * np.abs(R)[None]).sum(-1)
        delta = np.abs(got[:, 3:].astype(np.float64) - want[k][:, 3:].astype(np.float64))
        print(f"{case}/{model} pose {k}: max |delta| / bound = {float((delta / bound).max()):.3f}")
        assert (delta <= bound).all()


# ---- 2. ERP mode, windows and chunks -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [True, False])
def test_erp_rows_are_bit_equal_to_erp_rays(normalize):
    H, W = 48, 96
    for pose in make_poses(2):
        want = erp_rays(H, W, pose, DEV, normalize=normalize)
        got = camera_rays(H, W, pose, model="erp", normalize=normalize, device=DEV)
        assert got.shape == (H * W, 6) and np.array_equal(bits(got), bits(want))
        win = camera_rays(H, W, pose, model="erp", normalize=normalize, first=1234, count=777, device=DEV)
        assert np.array_equal(bits(win), bits(want[1234:1234 + 777]))
    assert camera_rays(H, W, pose, model="erp", first=H * W, count=0, device=DEV).shape == (0, 6)


@pytest.mark.parametrize("model", ["erp", "pinhole", "pinhole_blender"])
def test_chunks_at_arbitrary_boundaries_concatenate_to_the_image(model):
    H, W, pose = 37, 53, make_poses(1, seed=9)[0]
    kw = dict(model=model, focal=(41.3, 39.7), center=(25.2, 19.6), device=DEV)
    full = camera_rays(H, W, pose, **kw)
    cuts = [0, 1, 54, 55, 700, 701, 1333, H * W - 1, H * W]   # not aligned to rows
    buf = torch.full((800, 6), float("nan"), device=DEV)
    parts = [camera_rays(H, W, pose, first=a, count=b - a, out=buf, **kw).clone() for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(bits(torch.cat(parts)), bits(full))
    with pytest.raises(RuntimeError):
        camera_rays(H, W, pose, first=H * W - 3, count=4, **kw)
    with pytest.raises(RuntimeError):
        camera_rays(H, W, pose, model="pinhole", device=DEV)   # no focal length


# ---- 3. the pose is read from device memory ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["erp", "pinhole"])
def test_the_same_launch_follows_the_pose_buffer(model):
    H, W, (p0, p1) = 24, 40, make_poses(2, seed=5)
    kw = dict(model=model, focal=30.0, device=DEV)
    pose = torch.from_numpy(p0).to(DEV)
    buf = torch.empty(H * W, 6, device=DEV)
    first = camera_rays(H, W, pose, out=buf, **kw).clone()
    pose.copy_(torch.from_numpy(p1))
    second = camera_rays(H, W, pose, out=buf, **kw).clone()       # the same arguments: pointer, sizes, output
    assert np.array_equal(bits(first), bits(camera_rays(H, W, p0, **kw)))
    assert np.array_equal(bits(second), bits(camera_rays(H, W, p1, **kw)))
    assert not np.array_equal(bits(first), bits(second))
    pose4 = torch.eye(4, device=DEV)
    pose4[:3] = torch.from_numpy(p1).to(DEV)
    assert np.array_equal(bits(camera_rays(H, W, pose4, **kw)), bits(second))   # a [4][4] pose: its first three rows


# ---- 4. finish_frame -----------------------------------------------------------------------------------------------------------------

NEAR_FAR = [0.1, 15.0]


def _finish_inputs(H=250, W=404):
    g = np.random.default_rng(11)
    n = H * W
    rgb = g.uniform(-0.1, 1.1, (n, 3)).astype(np.float32)
    depth = g.uniform(0.05, 15.5, n).astype(np.float32)
    edge = [0.0, 1.0, 0.5, -0.25, 1.75, 0.999999, 1e-9]
    for k in range(256):
        v = np.float32(k / 255.0)
        edge += [float(np.nextafter(v, np.float32(-1))), float(v), float(np.nextafter(v, np.float32(2)))]
    rgb[:len(edge)] = np.asarray(edge, np.float32)[:, None]
    dedge = np.asarray([0.1, 15.0, np.nan, 0.0, 0.05, 20.0, 1e30, np.inf, -np.inf, 7.55, -3.0, 15.000001, 0.099999], np.float32)
    depth[:dedge.size] = dedge
    mi, den = ref.depth_range(NEAR_FAR)
    ks = np.arange(1, 256, dtype=np.float64)   # depths at and next to the index steps
    steps = (mi + ks / 255.0 * float(den)).astype(np.float32)
    depth[100:100 + 255] = steps
    depth[400:400 + 255] = np.nextafter(steps, np.float32(0))
    return rgb.reshape(H, W, 3), depth.reshape(H, W)


def test_finish_frame_equals_the_numpy_restatement():
    rgb, depth = _finish_inputs()
    assert rgb.shape[0] * rgb.shape[1] >= 100_000
    pal = (np.random.default_rng(2).integers(0, 256, (256, 3))).astype(np.uint8)
    want8, widx, wpal = ref.finish_ref(rgb, depth, NEAR_FAR, pal)
    t_rgb, t_depth = torch.from_numpy(rgb).to(DEV), torch.from_numpy(depth).to(DEV)
    rgb8, idx8 = finish_frame(t_rgb, t_depth, NEAR_FAR, palette=False)
    assert rgb8.dtype == torch.uint8 and rgb8.shape == rgb.shape and idx8.shape == depth.shape
    assert np.array_equal(rgb8.cpu().numpy(), want8) and np.array_equal(idx8.cpu().numpy(), widx)
    # saturation below near / above far (the reference's cast would wrap)
    flat_d, flat_i = depth.reshape(-1), idx8.cpu().numpy().reshape(-1)
    assert (flat_i[np.nan_to_num(flat_d) < NEAR_FAR[0]] == 0).all() and (flat_i[np.nan_to_num(flat_d) > NEAR_FAR[1]] == 255).all()
    assert (np.nan_to_num(flat_d) < NEAR_FAR[0]).sum() > 100 and (np.nan_to_num(flat_d) > NEAR_FAR[1]).sum() > 100
    # palette gather, default gray ramp
    _, depth8 = finish_frame(t_rgb, t_depth, NEAR_FAR, palette=pal)
    assert np.array_equal(depth8.cpu().numpy(), wpal) and np.array_equal(wpal, pal[widx])
    _, gray = finish_frame(t_rgb, t_depth, NEAR_FAR)
    assert np.array_equal(gray.cpu().numpy(), np.repeat(widx[..., None], 3, -1))
    # side by side = np.concatenate(axis=1)
    rgbd = finish_frame(t_rgb, t_depth, NEAR_FAR, palette=pal, side_by_side=True)
    assert np.array_equal(rgbd.cpu().numpy(), np.concatenate((want8, wpal), axis=1))
    # [n, 3] / [n] in, [n, 3] / [n] out
    f8, fi = finish_frame(t_rgb.view(-1, 3), t_depth.view(-1), NEAR_FAR, palette=False)
    assert np.array_equal(f8.cpu().numpy(), want8.reshape(-1, 3)) and np.array_equal(fi.cpu().numpy(), widx.reshape(-1))


@pytest.mark.parametrize("H,W", [(7, 13), (5, 6), (9, 8)])
def test_finish_frame_widths_that_are_not_multiples_of_four(H, W):
    """Rows that end inside a group of four pixels, and side-by-side halves that start off a word boundary."""
    g = np.random.default_rng(H * W)
    rgb, depth = g.uniform(-0.1, 1.1, (H, W, 3)).astype(np.float32), g.uniform(0.0, 16.0, (H, W)).astype(np.float32)
    pal = g.integers(0, 256, (256, 3)).astype(np.uint8)
    want8, widx, wpal = ref.finish_ref(rgb, depth, NEAR_FAR, pal)
    t_rgb, t_depth = torch.from_numpy(rgb).to(DEV), torch.from_numpy(depth).to(DEV)
    a, b = finish_frame(t_rgb, t_depth, NEAR_FAR, palette=pal)
    assert np.array_equal(a.cpu().numpy(), want8) and np.array_equal(b.cpu().numpy(), wpal)
    assert np.array_equal(finish_frame(t_rgb, t_depth, NEAR_FAR, palette=False)[1].cpu().numpy(), widx)
    rgbd = finish_frame(t_rgb, t_depth, NEAR_FAR, palette=pal, side_by_side=True)
    assert np.array_equal(rgbd.cpu().numpy(), np.concatenate((want8, wpal), axis=1))


@pytest.mark.parametrize("side_by_side", [False, True])
def test_finish_frame_into_mapped_pinned_memory(side_by_side):
    rgb, depth = _finish_inputs(H=64, W=100)
    t_rgb, t_depth = torch.from_numpy(rgb).to(DEV), torch.from_numpy(depth).to(DEV)
    dev = finish_frame(t_rgb, t_depth, NEAR_FAR, side_by_side=side_by_side)
    dev = [dev] if side_by_side else list(dev)
    host = [torch.zeros(d.shape, dtype=torch.uint8, pin_memory=True) for d in dev]
    got = finish_frame(t_rgb, t_depth, NEAR_FAR, side_by_side=side_by_side, out=host[0] if side_by_side else host)
    torch.cuda.synchronize()
    got = [got] if side_by_side else list(got)
    for h, g_, d in zip(host, got, dev):
        assert g_.data_ptr() == h.data_ptr() and np.array_equal(h.numpy(), d.cpu().numpy())


# ---- 5. FrameRenderer.render against volume_renderer + finish_frame -----------------------------------------------------------------

def _by_hand(model, H, W, pose, cam, kw, chunk, **finish):
    rays = camera_rays(H, W, pose, device=DEV, **cam)
    with torch.no_grad():
        rgb, depth = volume_renderer(rays, model, chunk=chunk, device=DEV, keep_alpha=False, **kw)[:2]
    return finish_frame(rgb.view(H, W, 3), depth.view(H, W), model.near_far, **finish)


CAMS = {"erp": (64, 128, dict(model="erp")), "pinhole": (96, 96, dict(model="pinhole", focal=60.0))}


def _renderer(model, name, kw, **extra):
    H, W, cam = CAMS[name]
    return FrameRenderer(model, H, W, camera=cam["model"], focal=cam.get("focal"), chunk=extra.pop("chunk", 3000), **extra, **kw)


@pytest.mark.parametrize("kw", [KW_RESAMPLE, KW_PLAIN], ids=["resampling", "plain"])
@pytest.mark.parametrize("name", ["erp", "pinhole"])
def test_frame_renderer_equals_volume_renderer_and_finish_frame(name, kw):
    model = env_model()
    H, W, cam = CAMS[name]
    pose = make_poses(1, seed=21)[0]
    fr = _renderer(model, name, kw)
    rgb8, depth8 = fr.render(pose)
    want8, wdepth8 = _by_hand(model, H, W, pose, cam, kw, chunk=3000)
    assert rgb8.shape == (H, W, 3) and depth8.shape == (H, W, 3) and rgb8.dtype == torch.uint8
    assert torch.equal(rgb8, want8) and torch.equal(depth8, wdepth8)
    assert len(torch.unique(rgb8)) > 16 and len(torch.unique(depth8)) > 1          # an image, not a constant
    # index image and side-by-side products of the same frame; a device pose
    r2, idx8 = _renderer(model, name, kw, palette=False).render(torch.from_numpy(pose).to(DEV))
    assert idx8.shape == (H, W) and torch.equal(r2, want8) and torch.equal(idx8, wdepth8[..., 0])
    rgbd = _renderer(model, name, kw, side_by_side=True).render(pose)
    assert torch.equal(rgbd, torch.cat((want8, wdepth8), dim=1))
    host = fr.render_to_host(pose)
    assert np.array_equal(host[0], want8.cpu().numpy()) and np.array_equal(host[1], wdepth8.cpu().numpy())


def test_frame_renderer_with_an_occupancy_mask():
    from tests.test_hip_compact_shading import scene_model
    model = scene_model("carved", True)
    assert model.use_alpha_mask
    pose = make_poses(1, seed=4, extent=0.05)[0]
    for name in ("erp", "pinhole"):
        H, W, cam = CAMS[name]
        rgb8, depth8 = _renderer(model, name, KW_RESAMPLE).render(pose)
        want8, wdepth8 = _by_hand(model, H, W, pose, cam, KW_RESAMPLE, chunk=3000)
        assert torch.equal(rgb8, want8) and torch.equal(depth8, wdepth8)


# ---- 6. graph mode -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["erp", "pinhole"])
def test_captured_frame_equals_the_eager_frame(name):
    model = env_model()
    poses = make_poses(4, seed=31)
    eager, graphed = _renderer(model, name, KW_RESAMPLE), _renderer(model, name, KW_RESAMPLE, graph=True)
    want = [tuple(t.clone() for t in eager.render(p)) for p in poses]
    got = [graphed.render(p) for p in poses]
    for w, g_ in zip(want, got):
        assert torch.equal(w[0], g_[0]) and torch.equal(w[1], g_[1])
    assert not torch.equal(want[0][0], want[1][0])
    again = graphed.render(poses[0])
    assert torch.equal(again[0], want[0][0]) and torch.equal(again[1], want[0][1])
    host = graphed.render_to_host(poses[2])
    assert np.array_equal(host[0], want[2][0].cpu().numpy()) and np.array_equal(host[1], want[2][1].cpu().numpy())


# ---- 7. render_path ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_render_path_yields_every_frame_in_order(graph):
    model = env_model()
    poses = make_poses(6, seed=41)
    fr = _renderer(model, "erp", KW_RESAMPLE, graph=graph)
    want = [tuple(a.copy() for a in fr.render_to_host(p)) for p in poses]
    got = [tuple(a.copy() for a in frame) for frame in fr.render_path(poses)]
    assert len(got) == 6
    for k, (w, g_) in enumerate(zip(want, got)):
        assert np.array_equal(w[0], g_[0]) and np.array_equal(w[1], g_[1]), f"frame {k}"
    assert not np.array_equal(want[0][0], want[1][0])
    assert list(fr.render_path([])) == []
    one = list(fr.render_path(poses[:1]))
    assert len(one) == 1 and np.array_equal(one[0][0], want[0][0])


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_leaving_render_path_early_leaves_nothing_pending(graph):
    model = env_model()
    poses = make_poses(5, seed=43)
    fr = _renderer(model, "erp", KW_RESAMPLE, graph=graph, side_by_side=True)
    want = fr.render_to_host(poses[3]).copy()
    gen = fr.render_path(poses)
    first = next(gen).copy()            # frame 0 is out, frame 1 is queued
    gen.close()
    del gen
    torch.cuda.synchronize()
    assert np.array_equal(first, fr.render_to_host(poses[0]))
    assert np.array_equal(fr.render(poses[3]).cpu().numpy(), want)
    for k, frame in enumerate(fr.render_path(poses)):   # ... and by breaking out of a loop
        if k == 2:
            break
    torch.cuda.synchronize()
    assert np.array_equal(fr.render_to_host(poses[3]), want)


# ---- 8. evaluation_path --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("camera", ["erp", "pinhole"])
def test_evaluation_path_writes_the_frames_it_returns(tmp_path, camera):
    from PIL import Image
    model = env_model()
    H, W = (32, 64) if camera == "erp" else (40, 48)
    ds = types.SimpleNamespace(img_wh=(W, H), near_far=[0.01, 15.0], focal=[36.0, 35.0])
    poses = make_poses(3, seed=51)
    with pytest.warns(UserWarning, match="mp4"):
        frames = evaluation_path(ds, model, poses, None, savePath=str(tmp_path / "out"), prtx="p_", exp_sampling=True, camera=camera,
                                 n_coarse=32, n_fine=32, resampling=True, chunk=1000)
    assert len(frames) == 3 and all(f.shape == (H, 2 * W, 3) and f.dtype == np.uint8 for f in frames)
    for k, f in enumerate(frames):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"p_{k:03d}.png")), f[:, :W])
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "rgbd" / f"p_{k:03d}.png")), f)
    fr = FrameRenderer(model, H, W, camera=camera, focal=ds.focal, near_far=ds.near_far, side_by_side=True, chunk=1000, exp_sampling=True,
                       n_coarse=32, n_fine=32, resampling=True)
    assert np.array_equal(fr.render_to_host(poses[1]), frames[1])
    assert np.array_equal(evaluation_path(ds, model, poses[:2], fr)[1], frames[1])   # a ready FrameRenderer, no files
    with pytest.raises(NotImplementedError):
        evaluation_path(ds, model, poses, ndc_ray=True)
