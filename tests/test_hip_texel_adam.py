"""GPU: Adam that steps only the texels a batch hit (csrc/ego_msi.hip: ego_msi_adam_step; egonerf_amd/optim.py: TexelAdam;
egonerf_amd/msi.py: refine_msi(optimizer="texel"); DESIGN.md 3.3 "Texel Adam").

1. the rule against the float64 restatement (tests/texel_adam_ref.py): counts exact, texels and moments within, per tensor,
   max(4 x max |float32 restatement - float64|, 1e-6 max |float64|), the rule of tests/test_hip_msi_refine.py;
2. untouched texels keep their bits; 3. the flags, reproducibility, tiny sizes; 4. the end of the bias table;
5. TexelAdam on two parameters and through a checkpoint; 6. a captured step; 7. refine_msi with the texel loop where every texel is
   hit in every step, and 8. where a step reaches an eighth of them."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth
from egonerf_amd.msi import MultiSphereImage, bake_msi, headbox_rays, project_msi, refine_msi
from egonerf_amd.optim import TexelAdam, adam_bias_table
from tests import texel_adam_ref as ref
from tests.helpers import make_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, EPS = 1e-3, 1e-8


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


class Texels:
    """Device state of one tensor of texels for direct calls of ego_msi_adam_step."""

    def __init__(self, p, moments=None, hits=None):
        n = len(p)
        self.n = n
        self.p = T(np.asarray(p, np.float32))
        self.mo = T(np.zeros((n, 2, 4), np.float32) if moments is None else np.asarray(moments, np.float32))
        self.h = T(np.zeros(n, np.int32) if hits is None else np.asarray(hits, np.int32))

    def step(self, grad, bias, betas=(0.9, 0.99), flags=0, lr=LR):
        """-> the gradient buffer after the call (device)."""
        g, b = T(np.asarray(grad, np.float32)), T(np.asarray(bias, np.float32))
        _lib.check(_lib.load().ego_msi_adam_step(self.p.data_ptr(), g.data_ptr(), self.mo.data_ptr(), self.h.data_ptr(), self.n, lr,
                                                 betas[0], betas[1], EPS, b.data_ptr(), len(b), flags, _lib.stream_handle()), "ego_msi_adam_step")
        torch.cuda.synchronize()   # `b` and `g` stay alive until the kernel is done
        return g

    def snapshot(self):
        return bits(self.p), bits(self.mo), self.h.cpu().numpy().copy()


def check(label, got, want64, want32):
    """Per tensor: |kernel - ref64| <= max(4 max |ref32 - ref64|, 1e-6 max |ref64|); prints every figure before it asserts."""
    ok = True
    for name, mine, w64, w32 in zip(("texels", "moments"), got, want64, want32):
        mine = np.asarray(mine, np.float64)
        dev32, top = float(np.abs(w32.astype(np.float64) - w64).max()), float(np.abs(w64).max())
        tol, err = max(4 * dev32, 1e-6 * top), float(np.abs(mine - w64).max())
        same = int((mine.astype(np.float32).view(np.int32) != w32.astype(np.float32).view(np.int32)).sum())
        print(f"{label} {name}: float32 restatement vs float64 {dev32:.3e}, kernel vs float64 {err:.3e}, tolerance {tol:.3e}, "
              f"max |ref64| {top:.3e}; {same} of {mine.size} values differ in bits from the float32 restatement")
        assert np.all(np.isfinite(mine))
        ok = ok and err <= tol
    assert ok


# ---- 1. the rule against float64 ---------------------------------------------------------------------------------------------------------

N_RULE, STEPS_RULE = 4099, 12   # more than sixteen blocks' worth of lanes in no multiple of 256


def rule_case():
    """Texels and 12 steps of gradients: a fresh random eighth touched per step with magnitudes from 1e-6 to 1e3, texel 0 in every
    step, the last texel never, texel 1 always with its alpha gradient alone."""
    g = np.random.default_rng(41)
    p0 = g.uniform(0, 1, (N_RULE, 4)).astype(np.float32)
    grads = (g.standard_normal((STEPS_RULE, N_RULE, 4)) * 10.0 ** g.uniform(-6, 3, (STEPS_RULE, N_RULE, 1))).astype(np.float32)
    touch = g.uniform(0, 1, (STEPS_RULE, N_RULE)) < 0.125
    touch[:, 0], touch[:, 1], touch[:, -1] = True, True, False
    grads = grads * touch[..., None]
    grads[:, 1, :3] = 0
    touched = np.any(grads != 0, axis=2)
    assert np.array_equal(touched, touch) and np.all(grads[:, 1, 3] != 0)
    return p0, grads, touched


@pytest.fixture(scope="module")
def rule():
    return rule_case()


@pytest.mark.parametrize("betas", [(0.9, 0.99), (0.8, 0.999)])
def test_rule_against_the_float64_restatement(rule, betas):
    p0, grads, touched = rule
    for s in range(STEPS_RULE):   # the case holds touched and untouched texels in every step
        assert 0.08 * N_RULE < touched[s].sum() < 0.18 * N_RULE and touched[s, 0] and not touched[s, -1]
    mags = np.abs(grads[grads != 0])
    assert mags.min() < 1e-5 and mags.max() > 1e2
    want64 = ref.run(p0, grads, LR, *betas, EPS, STEPS_RULE, dtype=np.float64)
    want32 = ref.run(p0, grads, LR, *betas, EPS, STEPS_RULE, dtype=np.float32)
    bias = ref.bias_table(*betas, STEPS_RULE, np.float32)
    dev = Texels(p0)
    for s in range(STEPS_RULE):
        left = dev.step(grads[s], bias, betas)
        assert torch.equal(left, T(grads[s]))   # without ZERO_GRAD the gradient is only read
    hits = dev.h.cpu().numpy()
    assert np.array_equal(hits, touched.sum(0)) and np.array_equal(hits, want64[2]) and hits[0] == STEPS_RULE and hits[-1] == 0
    check(f"rule betas={betas}", (dev.p.cpu().numpy(), dev.mo.cpu().numpy()), want64[:2], want32[:2])
    assert np.array_equal(bits(dev.p)[-1], p0[-1].view(np.int32)) and not dev.mo[-1].any()
    assert float(np.abs(want64[0] - p0).max()) > 5 * LR   # texel 0 has walked


# ---- 1b. the strided launch: every look-ahead body and a second round ----------------------------------------------------------------------

STRIDE = 2048 * 256          # the launch never has more workgroups (csrc/ego_msi.hip: ADAM_MAX_BLOCKS): a lane's texels lie this far apart
AHEAD = 4                    # gradients a lane loads before it looks at the first (ADAM_AHEAD)
N_STRIDED = 2_200_003        # just above AHEAD * STRIDE = 2097152 and no multiple of anything: 35 MB of texels


def test_rule_where_a_lane_takes_several_texels():
    """Up to 524288 texels only the first of the four look-ahead bodies ever holds a texel and the loop runs once; a 1024 x 2048 image
    uses all four over many rounds.  2200003 texels: texel i belongs to round i // (4 stride) and body (i // stride) % 4; round 0 fills
    all four bodies, round 1 the first body with 102851 texels, and its bodies 1 to 3 lie wholly past the end.  One step, an eighth
    touched; the last texel and the first of every body among them."""
    g = np.random.default_rng(71)
    n, steps = N_STRIDED, 1   # one step: what is checked here is which texel a lane takes, and the restatement of 2.2 million texels costs a second per step
    p0 = g.uniform(0, 1, (n, 4)).astype(np.float32)
    touch = g.uniform(0, 1, (steps, n)) < 0.125
    edges = np.asarray([j * STRIDE + d for j in range(AHEAD + 1) for d in (-1, 0, 1) if 0 <= j * STRIDE + d < n] + [n - 1])
    touch[:, edges] = True
    touch[:, edges[1:-1] + 2] = False
    grads = (g.standard_normal((steps, n, 4)) * 10.0 ** g.uniform(-3, 1, (steps, n, 1))).astype(np.float32) * touch[..., None]
    assert np.array_equal(np.any(grads != 0, axis=2), touch)
    idx = np.arange(n)
    rounds, body = idx // (AHEAD * STRIDE), (idx // STRIDE) % AHEAD
    assert rounds.max() == 1 and (rounds == 1).sum() == n - AHEAD * STRIDE == 102851 and set(body[rounds == 1]) == {0}
    for s in range(steps):   # touched and untouched texels in every body of the first round and in the second round
        for r, j in [(0, j) for j in range(AHEAD)] + [(1, 0)]:
            here = (rounds == r) & (body == j)
            assert 0.1 < touch[s, here].mean() < 0.15, (s, r, j)
    want64 = ref.run(p0, grads, LR, 0.9, 0.99, EPS, steps, ref.PROJECT | ref.ZERO_GRAD, np.float64)
    want32 = ref.run(p0, grads, LR, 0.9, 0.99, EPS, steps, ref.PROJECT | ref.ZERO_GRAD, np.float32)
    bias = ref.bias_table(0.9, 0.99, steps, np.float32)
    dev = Texels(p0)
    for s in range(steps):
        assert int(torch.count_nonzero(dev.step(grads[s], bias, flags=ref.PROJECT | ref.ZERO_GRAD))) == 0
    hits = dev.h.cpu().numpy()
    assert np.array_equal(hits, touch.sum(0)) and np.array_equal(hits, want64[2])
    assert hits[-1] == steps and hits[AHEAD * STRIDE] == steps and hits[AHEAD * STRIDE + 2] == 0
    got_p, got_m = dev.p.cpu().numpy(), dev.mo.cpu().numpy()
    never = hits == 0
    assert 0.7 * n < never.sum() and np.array_equal(got_p[never].view(np.int32), p0[never].view(np.int32)) and not got_m[never].any()
    check("strided", (got_p, got_m), want64[:2], want32[:2])
    for r, j in [(0, j) for j in range(AHEAD)] + [(1, 0)]:   # every region on its own: a slip in one body does not hide behind the others
        here = (rounds == r) & (body == j) & ~never
        assert float(np.abs(got_p[here] - want32[0][here]).max()) <= 1e-6, (r, j)
        assert float(np.abs(want64[0][here] - p0[here]).max()) > 0.5 * LR, (r, j)


# ---- 2. untouched means untouched ----------------------------------------------------------------------------------------------------------

def test_untouched_texels_keep_their_bits():
    g = np.random.default_rng(43)
    n = 1000
    touched = g.uniform(0, 1, n) < 0.125
    touched[0], touched[-1] = True, False
    # sentinels a projection would change: a negative colour, alpha 1.5, a NaN
    p0 = np.tile(np.asarray([-0.25, 2.0, np.nan, 1.5], np.float32), (n, 1))
    mo0 = g.standard_normal((n, 2, 4)).astype(np.float32)
    mo0[:, 1] = np.abs(mo0[:, 1])
    h0 = np.where(np.arange(n) % 2 == 0, 5, 0).astype(np.int32)
    grad = (g.standard_normal((n, 4)) * touched[:, None]).astype(np.float32)
    grad[~touched] = np.where(np.arange((~touched).sum())[:, None] % 2 == 0, np.float32(0.0), np.float32(-0.0))   # -0 compares equal to 0
    dev = Texels(p0, mo0, h0)
    before = dev.snapshot()
    left = dev.step(grad, ref.bias_table(0.9, 0.99, 8, np.float32), flags=ref.PROJECT | ref.ZERO_GRAD)
    after = dev.snapshot()
    u = ~touched
    assert u.sum() > 800 and touched.sum() > 80
    for a, b in zip(before, after):
        assert np.array_equal(a[u], b[u])
    assert np.array_equal(after[2][u], h0[u]) and (after[2][u] == 0).sum() > 300   # never touched: still 0
    assert np.array_equal(after[2][touched], h0[touched] + 1)
    assert not np.array_equal(before[0][touched], after[0][touched])
    pt = dev.p.cpu().numpy()[touched]
    assert np.all(pt[:, :3] >= 0) and np.all(pt[:, 3] >= 0) and np.all(pt[:, 3] <= 1)   # the touched ones were projected, NaN -> 0
    assert int(torch.count_nonzero(left)) == 0


# ---- 3. flags, reproducibility, tiny sizes -------------------------------------------------------------------------------------------------

def flag_case(n=3001):
    g = np.random.default_rng(47)
    p0 = g.uniform(0, 1, (n, 4)).astype(np.float32)          # in range: a projection leaves the untouched ones alone
    p0[::3] = np.asarray([0.0, 1e-4, 1.0, 1.0], np.float32)  # on the edge: a step of lr leaves the range
    touched = g.uniform(0, 1, n) < 0.3
    grad = (g.standard_normal((n, 4)) * touched[:, None]).astype(np.float32)
    mo0 = np.abs(g.standard_normal((n, 2, 4))).astype(np.float32) * 1e-2
    h0 = g.integers(0, 6, n).astype(np.int32)
    return p0, mo0, h0, grad, ref.bias_table(0.9, 0.99, 4, np.float32)


def test_project_flag_is_the_step_followed_by_ego_msi_project():
    p0, mo0, h0, grad, bias = flag_case()
    fused, plain = Texels(p0, mo0, h0), Texels(p0, mo0, h0)
    fused.step(grad, bias, flags=ref.PROJECT)
    plain.step(grad, bias, flags=0)
    unprojected = plain.p.clone()
    _lib.check(_lib.load().ego_msi_project(plain.p.data_ptr(), plain.n, _lib.stream_handle()), "ego_msi_project")
    torch.cuda.synchronize()
    assert not torch.equal(unprojected, plain.p)   # the projection had something to do
    for a, b in zip(fused.snapshot(), plain.snapshot()):
        assert np.array_equal(a, b)


def test_zero_grad_flag_zeroes_the_gradient_and_nothing_else():
    p0, mo0, h0, grad, bias = flag_case()
    zeroing, plain = Texels(p0, mo0, h0), Texels(p0, mo0, h0)
    left = zeroing.step(grad, bias, flags=ref.ZERO_GRAD)
    kept = plain.step(grad, bias, flags=0)
    assert int(torch.count_nonzero(left)) == 0 and torch.equal(kept, T(grad)) and int(torch.count_nonzero(kept)) > 1000
    for a, b in zip(zeroing.snapshot(), plain.snapshot()):
        assert np.array_equal(a, b)
    again = Texels(p0, mo0, h0)   # the same call twice: the same bits
    again.step(grad, bias, flags=ref.ZERO_GRAD)
    for a, b in zip(zeroing.snapshot(), again.snapshot()):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n", [1, 257])
def test_tiny_sizes(n):
    g = np.random.default_rng(53 + n)
    p0 = g.uniform(0, 1, (n, 4)).astype(np.float32)
    grads = g.standard_normal((3, n, 4)).astype(np.float32)
    if n > 1:
        grads[:, 1::2] = 0
    want64 = ref.run(p0, grads, LR, 0.9, 0.99, EPS, 3, ref.PROJECT | ref.ZERO_GRAD, np.float64)
    want32 = ref.run(p0, grads, LR, 0.9, 0.99, EPS, 3, ref.PROJECT | ref.ZERO_GRAD, np.float32)
    guard = torch.full((n + 2, 4), 7.0, device=DEV)   # the texels sit between two guard texels: nothing is written past the ends
    dev = Texels(p0)
    dev.p = guard[1:n + 1]
    dev.p.copy_(T(p0))
    for s in range(3):
        assert int(torch.count_nonzero(dev.step(grads[s], ref.bias_table(0.9, 0.99, 3, np.float32), flags=ref.PROJECT | ref.ZERO_GRAD))) == 0
    assert bool((guard[0] == 7).all()) and bool((guard[-1] == 7).all())
    assert np.array_equal(dev.h.cpu().numpy(), want64[2])
    check(f"n={n}", (dev.p.cpu().numpy(), dev.mo.cpu().numpy()), want64[:2], want32[:2])


# ---- 4. the end of the bias table ----------------------------------------------------------------------------------------------------------

def test_hits_past_the_table_use_its_last_entry():
    g = np.random.default_rng(59)
    p0 = g.uniform(0, 1, (5, 4)).astype(np.float32)
    grads = g.standard_normal((6, 5, 4)).astype(np.float32)
    grads[:, 1:] = 0   # six hits on texel 0, none elsewhere
    want64, want32 = (ref.run(p0, grads, LR, 0.9, 0.99, EPS, 3, dtype=dt) for dt in (np.float64, np.float32))
    full64 = ref.run(p0, grads, LR, 0.9, 0.99, EPS, 6, dtype=np.float64)
    dev = Texels(p0)
    for s in range(6):
        dev.step(grads[s], ref.bias_table(0.9, 0.99, 3, np.float32))
    assert dev.h.cpu().tolist() == [6, 0, 0, 0, 0]
    check("n_bias=3", (dev.p.cpu().numpy(), dev.mo.cpu().numpy()), want64[:2], want32[:2])
    # a table of six entries gives another texel: the comparison above tells the two apart
    gap, tol = float(np.abs(full64[0] - want64[0]).max()), 4 * float(np.abs(want32[0] - want64[0]).max())
    print(f"texel with entry 3 at steps 4 - 6 vs with its own entries: {gap:.3e} apart, tolerance {tol:.3e}")
    assert gap > 100 * tol


# ---- 5. TexelAdam --------------------------------------------------------------------------------------------------------------------------

def optimiser_case():
    g = np.random.default_rng(61)
    shapes = [(5, 6, 8, 4), (6, 8, 4)]
    p0 = [g.uniform(0, 1, s).astype(np.float32) for s in shapes]
    grads = [[(g.standard_normal(s) * (g.uniform(0, 1, s[:-1]) < 0.25)[..., None]).astype(np.float32) for s in shapes] for _ in range(4)]
    return shapes, p0, grads


def run_optimiser(p0, grads, split_at=None):
    params = [T(p).requires_grad_(True) for p in p0]
    opt = TexelAdam(params, lr=LR, project=True, zero_grad=True)
    for s, gs in enumerate(grads):
        if s == split_at:   # through a checkpoint into a new optimiser
            saved = opt.state_dict()
            opt = TexelAdam(params, lr=LR, project=True, zero_grad=True)
            opt.load_state_dict(saved)
            assert all(st["hits"].dtype == torch.int32 and st["moments"].dtype == torch.float32 for st in opt.state.values())
        for p, gr in zip(params, gs):
            p.grad = T(gr)
        versions = [p._version for p in params]
        opt.step()
        assert all(p._version > v for p, v in zip(params, versions))
        assert all(int(torch.count_nonzero(p.grad)) == 0 for p in params)
    return params, opt


def test_texel_adam_steps_two_parameters_and_survives_a_checkpoint():
    shapes, p0, grads = optimiser_case()
    params, opt = run_optimiser(p0, grads[:3])
    n_bias = len(adam_bias_table(0.9, 0.99))
    for i, (p, s) in enumerate(zip(params, shapes)):
        flat = [gs[i].reshape(-1, 4) for gs in grads[:3]]
        want64 = ref.run(p0[i].reshape(-1, 4), flat, LR, 0.9, 0.99, EPS, n_bias, ref.PROJECT, np.float64)
        want32 = ref.run(p0[i].reshape(-1, 4), flat, LR, 0.9, 0.99, EPS, n_bias, ref.PROJECT, np.float32)
        st = opt.state[p]
        assert st["moments"].shape == (*s[:-1], 2, 4) and st["hits"].shape == s[:-1] and st["hits"].dtype == torch.int32
        assert st["bias"].shape == (n_bias, 2) and "step" not in st
        assert np.array_equal(st["hits"].cpu().numpy().reshape(-1), want64[2]) and 0 < want64[2].max() <= 3 and want64[2].min() == 0
        check(f"TexelAdam parameter {i}", (p.detach().cpu().numpy().reshape(-1, 4), st["moments"].cpu().numpy().reshape(-1, 2, 4)),
              want64[:2], want32[:2])
    # other betas in the group: the next step builds the table they ask for
    saved = opt.state[params[0]]["bias"]
    opt.param_groups[0]["betas"] = (0.8, 0.999)
    for p, gr in zip(params, grads[3]):
        p.grad = T(gr * 0)   # touches nothing
    opt.step()
    for p in params:
        assert opt.state[p]["bias_betas"] == (0.8, 0.999) and opt.state[p]["bias"].shape[0] == len(adam_bias_table(0.8, 0.999))
        assert np.array_equal(opt.state[p]["bias"].cpu().numpy(), adam_bias_table(0.8, 0.999))
    opt.param_groups[0]["betas"] = (0.9, 0.99)
    opt.step()
    assert torch.equal(opt.state[params[0]]["bias"], saved)
    # a parameter without a gradient is skipped
    params[1].grad = None
    params[0].grad = T(grads[3][0])
    kept = bits(params[1])
    opt.step()
    assert np.array_equal(bits(params[1]), kept)
    # state_dict -> a new optimiser -> load_state_dict, one more step: the bits of the uninterrupted run
    straight, opt_a = run_optimiser(p0, grads)
    resumed, opt_b = run_optimiser(p0, grads, split_at=3)
    for a, b in zip(straight, resumed):
        assert np.array_equal(bits(a), bits(b))
        for key in ("moments", "hits", "bias"):
            assert torch.equal(opt_a.state[a][key], opt_b.state[b][key]), key
        assert opt_a.state[a]["bias_betas"] == opt_b.state[b]["bias_betas"] == (0.9, 0.99)
    with pytest.raises(ValueError, match="gradient"):
        params[0].grad = None
        params[0].grad = torch.zeros(5, 6, 8, 4, device=DEV).transpose(0, 1).contiguous().transpose(0, 1)   # of the shape, strided
        opt.step()


# ---- 6. capture ----------------------------------------------------------------------------------------------------------------------------

def test_a_captured_step_replays_as_eager_steps():
    g = np.random.default_rng(67)
    shape = (3, 10, 12, 4)
    p0 = g.uniform(0, 1, shape).astype(np.float32)
    grads = [(g.standard_normal(shape) * (g.uniform(0, 1, shape[:-1]) < 0.25)[..., None]).astype(np.float32) for _ in range(3)]

    def fresh():
        p = T(p0).requires_grad_(True)
        p.grad = torch.zeros_like(p)
        opt = TexelAdam([p], lr=LR, project=True, zero_grad=True)
        opt.step()   # an all-zero gradient touches nothing: the state exists, every clock still stands at 0
        assert int(opt.state[p]["hits"].abs().max()) == 0 and np.array_equal(bits(p), p0.view(np.int32))
        return p, opt

    eager, opt_e = fresh()
    for gr in grads:
        eager.grad.copy_(T(gr))
        opt_e.step()
    p, opt = fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(bits(p), p0.view(np.int32))   # capturing runs nothing
    for gr in grads:
        p.grad.copy_(T(gr))
        graph.replay()
        assert int(torch.count_nonzero(p.grad)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(p), bits(eager)) and not np.array_equal(bits(p), p0.view(np.int32))
    for key in ("moments", "hits"):
        assert torch.equal(opt.state[p][key], opt_e.state[eager][key])
    assert int(opt.state[p]["hits"].max()) >= 2


# ---- 7. refinement where every texel is hit in every step ----------------------------------------------------------------------------------

BH, BW, S_BAKE = 16, 32, 64
BAKE_RUNS = [3, 20, 9, 32]


def test_texel_refinement_lowers_the_error_inside_the_headbox(golden):
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
    refined = refine_msi(msi, model, 40, rays_per_step=4096, headbox=headbox, seed=0, render_kwargs=kw, log=log, optimizer="texel")
    before, after = mse(msi), mse(refined)
    print(f"held-out MSE against the teacher: {before:.4e} before, {after:.4e} after 40 texel steps of 4096 rays; "
          f"training loss {float(log[0]):.4e} -> {float(log[-1]):.4e}")
    assert after < before
    assert len(log) == 40 and all(t.is_cuda and t.dim() == 0 for t in log)
    for t in refined.parameters():
        assert bool(torch.isfinite(t).all()) and float(t[..., 3].min()) >= 0 and float(t[..., 3].max()) <= 1 and float(t[..., :3].min()) >= 0
        assert t.grad is None and not t.requires_grad
    assert refined.layers.dtype == msi.layers.dtype and refined.layers.data_ptr() != msi.layers.data_ptr()
    assert refined.background is not None and refined.background.dtype == msi.background.dtype
    assert torch.equal(refined.radii, msi.radii) and torch.equal(refined.bounds, msi.bounds)
    assert refined.center.tobytes() == msi.center.tobytes() and refined.near_far == msi.near_far
    assert not torch.equal(refined.layers, msi.layers)
    # the log holds the MSE: the first entry is that of the projected input on the first batch of the seed
    start = msi.float()
    start = MultiSphereImage(start.layers.clone(), msi.radii, msi.bounds, msi.center, msi.near_far, start.background.clone())
    project_msi(start)
    first = headbox_rays(4096, T(msi.center), headbox, torch.Generator(device=DEV).manual_seed(0))
    with torch.no_grad():
        want = float(torch.mean((start.render(first)[0] - model(first, is_train=False, need_alpha=False, **kw)[0]) ** 2))
    assert abs(want - float(log[0])) <= 1e-5 * want
    with torch.no_grad():
        half = refine_msi(msi.half(), model, 2, rays_per_step=512, headbox=headbox, render_kwargs=kw, optimizer="texel")
    assert half.layers.dtype == torch.float16 and half.background.dtype == torch.float16
    with pytest.raises(ValueError, match="optimizer"):
        refine_msi(msi, model, 1, headbox=headbox, render_kwargs=kw, optimizer="nope")


# ---- 8. refinement where a step reaches an eighth of the texels ----------------------------------------------------------------------------

SPARSE_RADII = np.asarray([1.0, 1.7, 3.0, 6.0], np.float32)
SPARSE_CENTER = np.asarray([0.25, -0.5, 0.125], np.float32)
SPARSE_AMPLITUDE, SPARSE_STEPS, SPARSE_RAYS = 0.02, 200, 256


def smooth_texels(seed, L=4, Hm=64, Wm=128):
    """[L, Hm, Wm, 4] float32 in [0.1, 0.9]: random 8 x 16 images, bilinearly enlarged (CPU torch: the same values everywhere)."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(L, 4, 8, 16, generator=g)
    fine = torch.nn.functional.interpolate(coarse, size=(Hm, Wm), mode="bilinear", align_corners=False)
    return (0.1 + 0.8 * fine).permute(0, 2, 3, 1).contiguous().numpy().astype(np.float32)


def test_texel_refinement_works_where_a_step_reaches_an_eighth_of_the_texels():
    """The teacher is itself a multi-sphere image (L = 4, 64 x 128 smooth texels in [0.1, 0.9]); the student is the teacher plus a
    perturbation uniform in +-0.02 per value, projected.  256 rays per step put their 1024 taps on about an eighth of a layer's 8192
    texels (measured on the CPU: 11.6 % of the texels receive a gradient per step), lr = 1e-3.

    Amplitude and step count were fixed on the CPU first, with tests/msi_grad_ref.py's float64 gradients, tests/texel_adam_ref.py's
    float64 step (projecting, zeroing) and rays of headbox_rays' distribution from numpy: held-out MSE (2048 rays) 1.466e-4 before,
    5.84e-5 after 100 steps, 3.12e-5 after 200 (0.21 of the start: at most half, as wanted), 1.15e-5 after 400.  200 steps it is.
    The assertion is after < before for "texel"; the dense loop's figure on the same student is printed for the record."""
    teacher_texels = smooth_texels(11)
    g = np.random.default_rng(5)
    student_texels = ref.project((teacher_texels + g.uniform(-SPARSE_AMPLITUDE, SPARSE_AMPLITUDE, teacher_texels.shape)).astype(np.float32))
    bounds = np.concatenate([[0.5 * SPARSE_RADII[0]], SPARSE_RADII + 0.1]).astype(np.float32)
    teacher = MultiSphereImage(T(teacher_texels), SPARSE_RADII, bounds, SPARSE_CENTER, [0.1, 15.0])
    student = MultiSphereImage(T(student_texels), SPARSE_RADII, bounds, SPARSE_CENTER, [0.1, 15.0])
    headbox = 0.2 * float(SPARSE_RADII[0])
    held_out = headbox_rays(2048, T(SPARSE_CENTER), headbox, torch.Generator(device=DEV).manual_seed(977))
    with torch.no_grad():
        target = teacher.render(held_out)[0]

    def mse(m):
        with torch.no_grad():
            return float(torch.mean((m.render(held_out)[0] - target) ** 2))

    before = mse(student)
    out = {name: mse(refine_msi(student, teacher, SPARSE_STEPS, rays_per_step=SPARSE_RAYS, headbox=headbox, lr=1e-3, seed=0, optimizer=name))
           for name in ("texel", "dense")}
    print(f"held-out MSE against the teacher image, {SPARSE_STEPS} steps of {SPARSE_RAYS} rays at lr 1e-3: {before:.4e} before, "
          f"{out['texel']:.4e} after with optimizer='texel', {out['dense']:.4e} with optimizer='dense' (not asserted)")
    assert 1.0e-4 < before < 2.0e-4   # the student the figures above were worked out for
    assert out["texel"] < before
