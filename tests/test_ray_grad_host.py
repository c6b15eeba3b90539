"""Host side of the ray gradients and of pose refinement (no GPU): the closed-form Jacobians of tests/ray_grad_ref.py against float64
autograd of the oracle's coordinate maps on both charts, PoseDeltas on CPU tensors, RayBank.image_of, refine_poses' argument checks
and the new symbols of the C ABI."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth
from egonerf_amd.data import RayBank
from egonerf_amd.poses import PoseDeltas, refine_poses, rotate
from tests import ray_grad_ref as ref
from tests.helpers import make_oracle

T = torch.from_numpy


def _oracle():
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    return make_oracle(cfg, synth.make_weights(cfg, seed=1234), dtype=torch.float64)


@pytest.mark.parametrize("yang", [False, True])
def test_closed_form_jacobians_against_float64_autograd(yang):
    o = _oracle()
    xyz, flags = ref.hand_placed_points(o)
    xyz = T(xyz[flags == yang]).double()
    x = xyz.clone().requires_grad_(True)
    choice = torch.full((x.shape[0],), int(yang))
    c7 = o.from_cartesian(x, choice)
    c7n = o.normalize_coord(c7, downsample=None)
    base = 3 if yang else 0
    p = (xyz - o.center.double()).numpy()
    J, Jn = ref.chart_jacobian(p, yang), ref.normalized_jacobian(o, p, yang)
    for row in range(3):
        g, = torch.autograd.grad(c7[:, base + row].sum(), x, retain_graph=True)
        gn, = torch.autograd.grad(c7n[:, base + row].sum(), x, retain_graph=True)
        assert np.abs(J[:, row] - g.numpy()).max() <= 1e-12 * max(np.abs(g.numpy()).max(), 1.0), row
        assert np.abs(Jn[:, row] - gn.numpy()).max() <= 1e-12 * max(np.abs(gn.numpy()).max(), 1.0), row
    # inside its own domain a chart has rho >= r / sqrt 2: no pole
    q = ref.chart_of(p, yang)
    assert bool((np.hypot(q[:, 0], q[:, 1]) >= np.sqrt((q * q).sum(-1)) / np.sqrt(2) - 1e-9).all())


def test_hand_placed_points_sit_inside_cells_of_both_charts():
    o = _oracle()
    xyz, yang = ref.hand_placed_points(o)
    assert 0 < int(yang.sum()) < len(yang)
    c7n = o.normalize_coord(o.from_cartesian(T(xyz).double(), T(yang).long()), downsample=None)
    mine = torch.where(T(yang)[:, None], c7n[:, 3:6], c7n[:, 0:3])
    ix = (mine + 1) * (torch.tensor(o.grid, dtype=torch.float64) - 1) / 2
    frac = ix - ix.floor()
    assert float(frac.min()) >= 0.1 - 1e-4 and float(frac.max()) <= 0.9 + 1e-4
    assert bool(((ix >= 0) & (ix <= torch.tensor(o.grid) - 1)).all())


def test_pose_deltas_zero_is_the_identity_bit_for_bit():
    rays = T(synth.make_rays(50, seed=3))
    idx = T(np.arange(50) % 4)
    pd = PoseDeltas(4)
    assert torch.equal(pd.rot, torch.zeros(4, 3)) and torch.equal(pd.trans, torch.zeros(4, 3))
    out = pd.apply(rays, idx)
    assert out.dtype == rays.dtype and torch.equal(out, rays)
    assert np.array_equal(out.detach().numpy().view(np.uint32), rays.numpy().view(np.uint32))
    poses = T(np.random.default_rng(0).normal(size=(4, 3, 4)).astype(np.float32))
    assert torch.equal(pd.poses(poses), poses)
    assert torch.equal(pd.poses(torch.cat([poses, torch.zeros(4, 1, 4)], 1)), poses)   # [K,4,4] accepted


def test_pose_deltas_rotate_and_differentiate():
    g = torch.Generator().manual_seed(0)
    # exp([w]x) against the matrix exponential, small and large angles, and across the series threshold
    for scale in (1e-9, 1e-4, 9e-4, 1.1e-3, 0.3, 3.0):
        w = (torch.rand(6, 3, generator=g, dtype=torch.float64) - 0.5) * scale
        d = torch.rand(6, 3, generator=g, dtype=torch.float64) - 0.5
        K = torch.zeros(6, 3, 3, dtype=torch.float64)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
        want = (torch.linalg.matrix_exp(K) @ d[:, :, None])[:, :, 0]
        assert float((rotate(w, d) - want).abs().max()) <= 1e-14, scale
    rays = T(synth.make_rays(7, seed=4)).double()
    idx = torch.tensor([0, 2, 1, 1, 0, 2, 2])   # repeated images: the index_select backward adds
    for rot0 in (torch.zeros(3, 3, dtype=torch.float64), (torch.rand(3, 3, generator=g, dtype=torch.float64) - 0.5) * 0.4):
        rot = rot0.clone().requires_grad_(True)
        trans = ((torch.rand(3, 3, generator=g, dtype=torch.float64) - 0.5) * 0.2).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda r, t: _apply(r, t, rays, idx), (rot, trans), eps=1e-6, atol=1e-7)


def _apply(rot, trans, rays, idx):
    """PoseDeltas.apply as a function of (rot, trans): the module's own code on substituted parameters."""
    pd = PoseDeltas(rot.shape[0]).double()
    del pd._parameters["rot"], pd._parameters["trans"]
    pd.rot, pd.trans = rot, trans
    return pd.apply(rays, idx)


def test_poses_composes_as_apply_does():
    """Rays generated from the corrected poses equal the corrected rays of the original poses."""
    from oracle.egonerf_oracle import erp_rays_reference
    g = torch.Generator().manual_seed(1)
    K, H, W = 3, 4, 8
    A = torch.rand(K, 3, 3, generator=g, dtype=torch.float64) - 0.5
    R = torch.linalg.matrix_exp(A - A.transpose(1, 2))
    poses = torch.cat([R, torch.rand(K, 3, 1, generator=g, dtype=torch.float64)], -1)
    pd = PoseDeltas(K).double()
    with torch.no_grad():
        pd.rot.copy_((torch.rand(K, 3, generator=g, dtype=torch.float64) - 0.5) * 0.5)
        pd.trans.copy_((torch.rand(K, 3, generator=g, dtype=torch.float64) - 0.5) * 0.3)
    with torch.no_grad():
        new = pd.poses(poses)
        assert new.shape == (K, 3, 4)
        eye = new[:, :, :3] @ new[:, :, :3].transpose(1, 2)
        assert float((eye - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-14          # still rotations
        for k in range(K):
            rays = erp_rays_reference(H, W, poses[k].float()).double()
            got = pd.apply(rays, torch.full((H * W,), k))
            want = erp_rays_reference(H, W, new[k].float()).double()
            assert float((got - want).abs().max()) <= 2e-6   # erp_rays_reference works in float32: ~1e-7 per operation


def test_image_of_with_a_roi():
    K, H, W = 3, 8, 16
    bank = RayBank(np.tile(np.eye(4, dtype=np.float32)[None], (K, 1, 1)), np.zeros((K, H, W, 3), np.uint8), (W, H), roi=(0.25, 0.75, 0.5, 1.0),
                   device="cpu")
    assert (bank.n_rows, bank.n_cols) == (4, 8) and bank.total == K * 32
    idx = torch.arange(bank.total)
    img = bank.image_of(idx)
    assert img.dtype == torch.int64 and torch.equal(img, idx // 32)
    assert torch.equal(bank.image_of(torch.tensor([0, 31, 32, 95])), torch.tensor([0, 0, 1, 2]))


def test_refine_poses_argument_errors():
    K, H, W = 2, 4, 8
    bank = RayBank(np.tile(np.eye(4, dtype=np.float32)[None], (K, 1, 1)), np.zeros((K, H, W, 3), np.uint8), (W, H), device="cpu")
    kw = dict(n_coarse=8)
    with pytest.raises(ValueError, match="render_kwargs"):
        refine_poses(None, bank, 1, 4, 1e-3, 1e-3)
    with pytest.raises(ValueError, match="steps and rays_per_step"):
        refine_poses(None, bank, 0, 4, 1e-3, 1e-3, render_kwargs=kw)
    with pytest.raises(ValueError, match="steps and rays_per_step"):
        refine_poses(None, bank, 1, 0, 1e-3, 1e-3, render_kwargs=kw)
    with pytest.raises(ValueError, match="lr_rot and lr_trans"):
        refine_poses(None, bank, 1, 4, 0.0, 1e-3, render_kwargs=kw)
    with pytest.raises(ValueError, match="needs the model's optimizer"):
        refine_poses(None, bank, 1, 4, 1e-3, 1e-3, train_model=True, render_kwargs=kw)
    with pytest.raises(ValueError, match="train_model is False"):
        refine_poses(None, bank, 1, 4, 1e-3, 1e-3, optimizer=object(), render_kwargs=kw)
    with pytest.raises(ValueError, match="exp_sampling=True"):
        refine_poses(None, bank, 1, 4, 1e-3, 1e-3, render_kwargs=dict(kw, exp_sampling=False))
    with pytest.raises(ValueError, match="do not hold two batches"):
        refine_poses(None, bank, 1, 40, 1e-3, 1e-3, render_kwargs=kw)
    with pytest.raises(ValueError, match="K must be"):
        PoseDeltas(0)


def test_new_symbols_are_declared_and_bound():
    syms = _lib.header_symbols()
    for name in ("ego_ray_grad", "ego_view_grad"):
        assert name in syms and name in _lib.PROTOTYPES, name
    assert len(_lib.PROTOTYPES["ego_ray_grad"][1]) == 18 and len(_lib.PROTOTYPES["ego_view_grad"][1]) == 9
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib.os.path.dirname(_lib.os.path.abspath(_lib.__file__))), "include", "egonerf_hip.h")).read()
    assert "#define EGO_ABI_VERSION 17" in hdr
