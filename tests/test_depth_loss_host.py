"""CPU: the depth term's restatement (tests/depth_loss_ref.py): the kernel's recurrence against torch's float64 autograd of the
definition, how far float32 arithmetic alone is from float64 on the GPU tests' inputs (the GPU bounds are 4 x these distances), and
the argument checks of losses.depth_loss, TrainSchedule.stepped, RayBank(depths=...) and the library."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib
from egonerf_amd.data import RayBank
from egonerf_amd.losses import depth_loss, expected_depth
from egonerf_amd.train import TrainSchedule
from tests import depth_loss_ref as ref


@pytest.mark.parametrize("case_id", ref.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_float64_model_equals_autograd_of_the_definition(case_id):
    c = ref.case(*case_id)
    S, space, kind = case_id[0], case_id[2], case_id[3]
    value, g, D = ref.kernel_model(c.alpha, c.z, c.target, c.tail, space, kind, np.float64)
    v_direct, D_direct = ref.direct(c.alpha, c.z, c.target, c.tail, space, kind)
    assert c.v64 > 0 and c.g_scale > 0
    assert abs(value - c.v64) <= 1e-12 * c.v64 and abs(v_direct - c.v64) <= 1e-12 * c.v64
    assert float(np.abs(D - c.D64).max()) <= 1e-12 * c.D_scale and float(np.abs(D_direct - c.D64).max()) <= 1e-12 * c.D_scale
    assert g.shape == c.alpha.shape and float(np.abs(g - c.g64).max()) <= 1e-12 * c.g_scale
    ok = ref.valid_mask(c.target)
    assert 20 <= int(ok.sum()) < ref.N and not ok[[3, 6, 7, 8, 10]].any() and ok[0] and ok[ref.EXACT_ROW]
    assert np.all(g[~ok] == 0) and np.all(c.g64[~ok] == 0)
    assert np.all(g[ref.EXACT_ROW] == 0) and np.all(c.g64[ref.EXACT_ROW] == 0)   # r = 0 exactly: no gradient in either kind
    assert D[ref.EXACT_ROW] == ref.smap(c.target, space)[ref.EXACT_ROW]
    if c.alpha.shape[1] > S:
        assert np.all(g[:, S:] == 0) and np.all(c.g64[:, S:] == 0)


def test_float32_model_distances_on_the_gpu_tests_inputs():
    """What the GPU bounds are built from (4 x each): printed by -s.  If float32 arithmetic alone were far from float64 on these inputs
    the bound would test the inputs, not the kernel: each distance stays below 1e-5."""
    worst = [0.0, 0.0, 0.0]
    for cid in ref.CASES:
        c = ref.case(*cid)
        print(f"float32 model {cid}: value {c.ev32:.2e} of |v64|, gradient {c.eg32:.2e} of max |g64|, pred {c.ep32:.2e} of max |D64|")
        worst = [max(a, b) for a, b in zip(worst, (c.ev32, c.eg32, c.ep32))]
        assert c.ev32 <= 1e-5 and c.eg32 <= 1e-5 and c.ep32 <= 1e-5
        assert c.value_bound >= 4 * c.ev32 and c.value_bound >= 2.0 ** -22
    print(f"worst: value {worst[0]:.2e}, gradient {worst[1]:.2e}, pred {worst[2]:.2e}")


def test_known_answers():
    S = 9
    _, z, _, _ = ref.make_inputs(11, S)
    z, tail = z[:2], np.array([2.0, 3.0], np.float32)
    alpha = np.zeros((2, S), np.float32)
    target = np.array([4.0, 0.0], np.float32)
    value, g, D = ref.kernel_model(alpha, z, target, tail)
    assert np.array_equal(D, [2.0, 3.0]) and value == 4.0            # nothing on the rays: D = tail; one valid ray, r = -2
    alpha[0, 4] = 1.0
    value, g, D = ref.kernel_model(alpha, z, target, None)
    assert abs(D[0] - z[0, 4]) <= 1e-8 and abs(value - (D[0] - 4.0) ** 2) <= 1e-12   # one opaque sample: its z (T_4 = (1 + 1e-10)^4)
    assert np.all(g[1] == 0) and float(np.abs(g[0, 5:]).max()) <= 1e-8   # the invalid ray; behind the opaque sample T <= 1e-10
    value, g, D = ref.kernel_model(alpha, z, np.array([np.nan, -1.0], np.float32), tail)
    assert value == 0.0 and np.all(g == 0) and not np.isnan(D).any()   # V = 0


def test_host_layer_refuses_bad_arguments():
    a, z, t = torch.zeros(5, 8), torch.ones(5, 8), torch.ones(5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        depth_loss(a, z, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        expected_depth(a, z, tail=t)
    for bad in (lambda: depth_loss(a, z, t, space="sqrt"), lambda: depth_loss(a, z, t, space="linear"), lambda: depth_loss(a, z, t, kind="huber"),
                lambda: depth_loss(a, z, t, space="log"), lambda: depth_loss(a, z, t, space="disparity", near_far=[0.0, 15.0]),
                lambda: depth_loss(a, z, t, space="log", near_far=[2.0, 2.0]), lambda: depth_loss(a, z, t, space="log", near_far=[0.1, float("inf")])):
        with pytest.raises(ValueError):
            bad()
    zeros = torch.zeros
    for al, zz in ((zeros(5, 8), zeros(4, 8)), (zeros(5, 10), zeros(5, 8)), (zeros(5, 7), zeros(5, 8)), (zeros(5, 8, 1), zeros(5, 8)),
                   (zeros(5, 1), zeros(5, 1)), (zeros(5, 8), zeros(5, 8, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match=r"must be"):
            depth_loss(al, zz, t)
    for tt in (zeros(4), zeros(5, 1), zeros(5, dtype=torch.float64), None):
        with pytest.raises(RuntimeError, match=r"target must be"):
            depth_loss(a, z, tt)
    with pytest.raises(RuntimeError, match=r"tail must be"):
        depth_loss(a, z, t, tail=zeros(6))
    with pytest.raises(RuntimeError, match=r"tail must be"):
        expected_depth(a, z, tail=zeros(5, dtype=torch.float16))


def test_library_refuses_bad_arguments_before_anything_is_queued():
    lib = _lib.load()
    one = 16   # a non-null, 8-byte aligned address: every call below fails its checks first
    call = lambda alpha=one, stride=8, z=one, target=one, tail=None, N=4, S=8, near=0.01, far=15.0, space=_lib.DIST_LOG, kind=_lib.DEPTH_L2, ws=one, \
        value=one, g=one, pred=None: lib.ego_ray_depth_loss(alpha, stride, z, target, tail, N, S, near, far, space, kind, ws, value, g, pred, None)
    for kw in (dict(S=1), dict(stride=7), dict(stride=10), dict(N=-1), dict(far=0.01), dict(far=float("nan")), dict(far=float("inf")),
               dict(near=0.0), dict(near=0.0, space=_lib.DIST_DISPARITY), dict(near=-1.0), dict(space=_lib.DIST_LINEAR), dict(space=4),
               dict(space=-1), dict(kind=2), dict(kind=-1), dict(alpha=None), dict(z=None), dict(value=None, g=None), dict(target=None),
               dict(ws=None), dict(ws=20), dict(target=None, value=None)):
        assert call(**kw) == -1 and b"ray_depth_loss" in lib.ego_last_error(), kw
    assert call(alpha=None, z=None, N=0, value=None, g=None) == 0      # N == 0: a no-op
    assert call(S=1, N=0) == -1                                        # ... after the size checks
    assert call(space=_lib.DIST_LOG, near=0.0, N=0) == -1
    assert lib.ego_ray_depth_loss_workspace_bytes(0) == 16 and lib.ego_ray_depth_loss_workspace_bytes(37) == 16 + 8 * 37
    assert lib.ego_ray_depth_loss_workspace_bytes(-1) == -1
    bank = RayBank(np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)), np.zeros((2, 6, 8, 3), np.uint8), (8, 6), device="cpu")
    gather = lambda depth=one, idx=one, B=4, out=one, half=0: lib.ego_ray_batch_gather_depth(bank.struct, depth, half, idx, B, out, None)
    for kw in (dict(depth=None), dict(idx=None), dict(out=None), dict(B=-1), dict(depth=18), dict(depth=17, half=1)):
        assert gather(**kw) == -1 and b"ray_batch_gather_depth" in lib.ego_last_error(), kw
    assert gather(depth=None, idx=None, out=None, B=0) == 0


def test_symbols_are_declared_and_exported():
    lib = _lib.load()
    for name in ("ego_ray_depth_loss", "ego_ray_depth_loss_workspace_bytes", "ego_ray_batch_gather_depth"):
        assert name in _lib.header_symbols() and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert (_lib.DIST_LINEAR, _lib.DIST_LOG, _lib.DIST_DISPARITY, _lib.DIST_METRIC) == (0, 1, 2, 3)   # the existing values keep their numbers
    assert (_lib.DEPTH_L2, _lib.DEPTH_L1) == (0, 1)
    assert lib.ego_abi_version() == 17 == _lib.EXPECTED_ABI_VERSION


def test_stepped_weight_follows_the_reference_s_formula():
    """train.py:276 and :279-281: depth_lambda * depth_rate ** int(iteration / depth_step_size), 0 once iteration > depth_end_iter."""
    w0, rate, step, end = 0.3, 0.5, 3, 7
    sched = TrainSchedule("cpu", start_iteration=1)
    for it in range(1, 11):
        got, free = sched.stepped(w0, rate, step, end_iter=end), sched.stepped(w0, rate, step)
        assert got.dtype == torch.float32 and got.shape == () and sched.iteration() == it
        want = np.float32(w0 * rate ** int(it / step))
        assert float(free) == want
        assert float(got) == (0.0 if it > end else want)
        sched.it.add_(1.0)
    assert float(TrainSchedule("cpu", 5).stepped(2.0, 0.1, 2.5)) == np.float32(2.0 * 0.1 ** 2)
    with pytest.raises(ValueError):
        sched.stepped(w0, rate, 0)


def test_ray_bank_depths_on_the_host():
    poses, imgs = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)), np.zeros((2, 6, 8, 3), np.uint8)
    plain = RayBank(poses, imgs, (8, 6), device="cpu")
    assert plain.depths is None and plain.nbytes == 2 * 6 * 8 * 4 + 2 * 48
    with pytest.raises(ValueError, match="without depths"):
        plain.gather_depth_into(torch.zeros(3, dtype=torch.int64), torch.zeros(3))
    for dtype, size in ((np.float32, 4), (np.float16, 2)):
        bank = RayBank(poses, imgs, (8, 6), roi=(0.25, 0.75, 0.25, 1), device="cpu", depths=np.ones((2, 6, 8), dtype))
        assert bank.depths.dtype == (torch.float32 if size == 4 else torch.float16) and tuple(bank.depths.shape) == (2, 6, 8)
        assert bank.nbytes == plain.nbytes + 2 * 6 * 8 * size
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            bank.gather_depth(torch.zeros(3, dtype=torch.int64))
    bank = RayBank(poses, imgs, (8, 6), device="cpu", depths=torch.ones(2, 6, 8, dtype=torch.float16))
    assert bank.depths.dtype == torch.float16
    for bad in (np.ones((2, 6, 8), np.float64), np.ones((2, 6, 8), np.int32), np.ones((2, 8, 6), np.float32), np.ones((1, 6, 8), np.float32),
                np.ones((2, 6, 8, 1), np.float32), np.ones((2, 3, 8), np.float32)):   # the window's shape is not the array's
        with pytest.raises(ValueError, match="depths must be"):
            RayBank(poses, imgs, (8, 6), roi=(0.25, 0.75, 0, 1), device="cpu", depths=bad)
