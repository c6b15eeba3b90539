"""CPU: Adam that steps only the texels a batch hit (csrc/ego_msi.hip: ego_msi_adam_step; egonerf_amd/optim.py: TexelAdam, adam_bias_table;
DESIGN.md 3.3 "Texel Adam") - the restatement the GPU tests compare the kernel with (tests/texel_adam_ref.py) against torch.optim.Adam,
what the rule is for (an isolated hit), and everything the library and the optimiser refuse before a device is needed."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib
from egonerf_amd.optim import BIAS_TABLE_CAP, TexelAdam, adam_bias_table
from tests import texel_adam_ref as ref

LR, B1, B2, EPS = 1e-3, 0.9, 0.99, 1e-8


def torch_adam(p0, grads):
    """p0 [..., 4], grads [steps, ..., 4] float64 -> the parameter after torch.optim.Adam(betas=(0.9, 0.99)) has seen every gradient."""
    p = torch.from_numpy(np.array(p0, np.float64)).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=LR, betas=(B1, B2), eps=EPS)
    for g in grads:
        p.grad = torch.from_numpy(np.array(g, np.float64))
        opt.step()
    return p.detach().numpy()


def test_every_texel_touched_is_torch_adam():
    g = np.random.default_rng(3)
    p0 = g.uniform(0, 1, (37, 4))
    grads = g.standard_normal((20, 37, 4)) * 10.0 ** g.uniform(-6, 3, (20, 37, 1))
    assert np.all(np.any(grads != 0, axis=2))
    got, _, hits = ref.run(p0, grads, LR, B1, B2, EPS, n_bias=20, dtype=np.float64)
    want = torch_adam(p0, grads)
    assert np.all(hits == 20) and np.abs(want - p0).max() > 5 * LR
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()


def test_a_touch_mask_gives_every_texel_its_own_adam():
    g = np.random.default_rng(4)
    n, steps = 9, 20
    p0 = g.uniform(0, 1, (n, 4))
    grads = g.standard_normal((steps, n, 4))
    mask = g.uniform(0, 1, (steps, n)) < 0.3
    mask[:, 0], mask[:, 1] = True, False   # one texel always, one never
    grads = grads * mask[..., None]
    grads[mask & (np.arange(n) == 2)[None], :3] = 0   # one texel whose alpha gradient alone is non-zero
    got, moments, hits = ref.run(p0, grads, LR, B1, B2, EPS, n_bias=steps, dtype=np.float64)
    assert np.array_equal(hits, mask.sum(0)) and hits[1] == 0 and 0 < hits[2] < steps
    assert np.array_equal(got[1], p0[1]) and not moments[1].any()
    for i in range(n):
        want = torch_adam(p0[i], grads[mask[:, i], i])   # only the steps that touched texel i
        assert np.abs(got[i] - want).max() <= 1e-12, (i, np.abs(got[i] - want).max())


@pytest.mark.parametrize("size", [1e-6, 0.02, 1e3])
def test_an_isolated_hit_moves_a_texel_by_one_step_not_by_a_walk(size):
    """One hit, then seven steps without a gradient.  On the texel's own clock: m / (1 - b1) = g and sqrt(v) / sqrt(1 - b2) = |g| at
    its first step, so it moves by lr g / (|g| + eps), and the empty steps do not exist for it.  Dense Adam walks on on the hit's
    momentum: the sum over k = 0 .. 7 of lr (0.9^k / (1 - 0.9^(k+1))) / (0.99^(k/2) / sqrt(1 - 0.99^(k+1))) sign(g), more than 3 lr."""
    hit = np.array([[size, -size, 0.5 * size, -2 * size]])
    grads = np.concatenate([hit[None], np.zeros((7, 1, 4))])
    p0 = np.full((1, 4), 0.5)
    got, _, hits = ref.run(p0, grads, LR, B1, B2, EPS, n_bias=8, dtype=np.float64)
    assert hits[0] == 1
    want = p0 - LR * hit / (np.abs(hit) + EPS)
    assert np.abs(got - want).max() <= 1e-12 * LR, np.abs(got - want).max()
    dense = torch_adam(p0, grads)
    walk = np.abs(dense - p0) / LR
    print(f"|g| = {size:g}: own clock moves {np.abs(got - p0).max() / LR:.4f} lr, dense Adam {walk.min():.3f} to {walk.max():.3f} lr")
    assert np.abs(got - p0).max() <= LR and walk.min() > 3.0
    assert np.all(np.sign(dense - p0) == -np.sign(hit))


def test_bias_table_entries_and_length():
    for b1, b2 in ((0.9, 0.99), (0.8, 0.999), (0.0, 0.0), (0.5, 0.0)):
        table = adam_bias_table(b1, b2)
        n = len(table)
        assert table.dtype == np.float32 and table.shape == (n, 2) and table.flags["C_CONTIGUOUS"] and 1 <= n <= BIAS_TABLE_CAP
        t = np.arange(1, n + 1, dtype=np.float64)
        assert np.array_equal(table[:, 0], (1.0 - b1 ** t).astype(np.float32))
        assert np.array_equal(table[:, 1], np.sqrt(1.0 - b2 ** t).astype(np.float32))
        assert np.array_equal(table, ref.bias_table(b1, b2, n, np.float32))
        # the table ends at the FIRST t at which both entries round to 1.0f
        both = (table == np.float32(1)).all(axis=1)
        assert both[-1] and not both[:-1].any(), (b1, b2, n)
    assert len(adam_bias_table(0.0, 0.0)) == 1
    assert 100 < len(adam_bias_table(0.9, 0.99)) < 3000       # 0.99^t < 2^-24 from t of about 1700 on
    capped = adam_bias_table(0.9, 1.0 - 1e-9)                  # would need some 2e10 entries
    assert len(capped) == BIAS_TABLE_CAP == 1 << 20 and capped[-1, 1] < 1
    for bad in ((1.0, 0.5), (0.5, 1.0), (-0.1, 0.5), (float("nan"), 0.5)):
        with pytest.raises(ValueError, match="betas"):
            adam_bias_table(*bad)


def test_symbol_is_declared_bound_and_exported():
    lib = _lib.load()
    assert "ego_msi_adam_step" in _lib.header_symbols() and "ego_msi_adam_step" in _lib.PROTOTYPES and hasattr(lib, "ego_msi_adam_step")
    assert lib.ego_abi_version() == 17 == _lib.EXPECTED_ABI_VERSION
    assert (_lib.TEXEL_ADAM_PROJECT, _lib.TEXEL_ADAM_ZERO_GRAD) == (1, 2) == (ref.PROJECT, ref.ZERO_GRAD)


def test_library_refuses_bad_arguments_before_anything_is_queued():
    lib = _lib.load()
    one = 32   # a non-null address aligned for every argument

    def call(texels=one, grad=one, moments=one, hits=one, n=4, lr=1e-3, b1=0.9, b2=0.99, eps=1e-8, bias=one, n_bias=3, flags=3):
        return lib.ego_msi_adam_step(texels, grad, moments, hits, n, lr, b1, b2, eps, bias, n_bias, flags, None)

    for kw in (dict(texels=None), dict(grad=None), dict(moments=None), dict(hits=None), dict(bias=None)):
        assert call(**kw) == -1 and b"msi_adam_step" in lib.ego_last_error() and b"null" in lib.ego_last_error(), kw
    for kw in (dict(texels=24), dict(grad=8), dict(moments=48 + 4), dict(hits=18), dict(bias=36)):
        assert call(**kw) == -1 and b"aligned" in lib.ego_last_error(), kw
    assert call(n_bias=0) == -1 and b"n_bias" in lib.ego_last_error()
    assert call(n_bias=-5) == -1
    for kw in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=1.5), dict(b2=-1e-3), dict(b1=float("nan")), dict(b2=float("nan"))):
        assert call(**kw) == -1 and b"betas" in lib.ego_last_error(), kw
    for eps in (0.0, -1e-8, float("nan")):
        assert call(eps=eps) == -1 and b"eps" in lib.ego_last_error(), eps
    for flags in (4, 8, 7, -1):
        assert call(flags=flags) == -1 and b"flag" in lib.ego_last_error(), flags
    assert call(n=-1) == -1 and b"n_texels" in lib.ego_last_error()
    assert call(n=(1 << 31) * 256) == -1 and b"too large" in lib.ego_last_error()
    # nothing to do: no pointer is looked at - but the settings still are
    assert lib.ego_msi_adam_step(None, None, None, None, 0, 1e-3, 0.9, 0.99, 1e-8, None, 1, 0, None) == 0
    assert call(n=0, b1=1.0) == -1 and call(n=0, flags=4) == -1


def test_texel_adam_refuses_what_the_kernel_cannot_step():
    with pytest.raises(ValueError, match="HIP device"):
        TexelAdam([torch.zeros(3, 5, 4)])
    with pytest.raises(ValueError, match="float32"):
        TexelAdam([torch.zeros(3, 5, 4, dtype=torch.float16)])
    with pytest.raises(ValueError, match="float32"):
        TexelAdam([torch.zeros(3, 5, 4, dtype=torch.float64)])
    with pytest.raises(ValueError, match="last dimension must be 4"):
        TexelAdam([torch.zeros(3, 4, 5)])
    with pytest.raises(ValueError, match="contiguous"):
        TexelAdam([torch.zeros(4, 5, 3).permute(2, 1, 0)])   # [3, 5, 4], strided
    for kw in (dict(betas=(1.0, 0.5)), dict(betas=(0.5, -0.1)), dict(eps=0.0)):
        with pytest.raises(ValueError, match="betas / eps"):
            TexelAdam([torch.zeros(3, 4)], **kw)
    import inspect
    sig = inspect.signature(TexelAdam.__init__)
    assert [(k, v.default) for k, v in sig.parameters.items()][2:] == [("lr", 1e-3), ("betas", (0.9, 0.99)), ("eps", 1e-8), ("project", False),
                                                                       ("zero_grad", False)]


def test_refine_refuses_an_unknown_optimizer():
    from egonerf_amd.msi import MultiSphereImage, refine_msi
    g = torch.Generator().manual_seed(0)
    msi = MultiSphereImage(torch.rand(3, 4, 8, 4, generator=g), [0.5, 1.5, 4.0], [0.25, 1.0, 2.5, 6.0], [0.1, -0.2, 0.3], [0.01, 15.0])
    with pytest.raises(ValueError, match="optimizer"):
        refine_msi(msi, (lambda rays, **kw: (None,)), 1, headbox=0.1, optimizer="nope")
    for name in ("dense", "texel"):   # both known: the refusal is the host image's
        with pytest.raises(ValueError, match="HIP device"):
            refine_msi(msi, (lambda rays, **kw: (None,)), 1, headbox=0.1, optimizer=name)
