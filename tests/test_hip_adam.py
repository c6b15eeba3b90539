"""GPU: the multi-tensor Adam (ego_adam_step, ego_adam_step_graph, FusedAdam) beyond one launch.  A launch takes 40 tensors, so 83
tensors make two full launches and one of 3: the later launches use re-based block tables and a shorter count.  Sizes sit on either
side of the 1024-element block, with empty tensors inside a launch, last in a launch and last overall.  After every step p, m and v
have the bits of the float32 restatement (tests/table_ops_ref.py) and stay within the derived running-error bound of the float64
recurrence started from the same float32 state; the element past every tensor is a sentinel that must survive."""
import numpy as np
import pytest
import torch

from egonerf_amd import _lib
from egonerf_amd.optim import FusedAdam
from tests import table_ops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = np.float32(-7777.25)
SETTINGS = [((0.9, 0.99), 1e-8), ((0.9, 0.99), 1e-15), ((0.0, 0.5), 1e-8), ((0.0, 0.5), 1e-15)]
STEPS = (1, 2, 10, 1000, 10 ** 6)


class Bank:
    """83 tensors laid end to end, each followed by one sentinel element, for p, g, m and v alike."""

    def __init__(self, seed):
        self.sizes = R.adam_sizes()
        self.offs = np.cumsum([0] + [n + 1 for n in self.sizes])[:-1]
        self.total = int(sum(self.sizes) + len(self.sizes))
        self.guard = np.zeros(self.total, bool)
        self.owner = np.zeros(self.total, np.int64)
        for i, (o, n) in enumerate(zip(self.offs, self.sizes)):
            self.guard[o + n] = True
            self.owner[o:o + n + 1] = i
        self.rng = np.random.default_rng(seed)
        self.lr = np.array([R.adam_lr(i) for i in range(len(self.sizes))], np.float32)
        self.p = self._guarded(self.rng.normal(size=self.total).astype(np.float32))
        self.m, self.v = self._guarded(np.zeros(self.total, np.float32)), self._guarded(np.zeros(self.total, np.float32))
        self.dev = {k: torch.from_numpy(getattr(self, k)).to(DEV) for k in "pmv"}
        self.dev["g"] = torch.empty(self.total, device=DEV)

    def _guarded(self, a):
        a[self.guard] = SENTINEL
        return a

    def tensors(self):
        ts = [_lib.AdamTensor(*(self.dev[k].data_ptr() + 4 * int(o) for k in "pgmv"), int(n), float(lr), 0)
              for o, n, lr in zip(self.offs, self.sizes, self.lr)]
        return (_lib.AdamTensor * len(ts))(*ts)

    def new_grad(self, flip):
        g = self._guarded(R.adam_grad(self.total, self.rng, flip))
        self.dev["g"].copy_(torch.from_numpy(g))
        return g

    def read(self):
        torch.cuda.synchronize()
        return tuple(self.dev[k].cpu().numpy() for k in "pmv")

    def check(self, got, want, what):
        live = ~self.guard
        for name, a, b in zip("pmv", got, want):
            assert (a[self.guard] == SENTINEL).all(), (what, name, "wrote past a tensor")
            bad = np.flatnonzero((R.bits(a) != R.bits(b)) & live)
            assert bad.size == 0, (what, name, "tensor", int(self.owner[bad[0]]), "of size", self.sizes[int(self.owner[bad[0]])], bad.size)


def _frac(err, bnd, live):
    return float(np.max((np.abs(err) / bnd)[live]))


@pytest.mark.parametrize("betas,eps", SETTINGS)
def test_adam_step_c_abi(betas, eps):
    bank = Bank(seed=3)
    lib, arr = _lib.load(), bank.tensors()
    live, worst = ~bank.guard, 0.0
    for k, step in enumerate(STEPS):
        g = bank.new_grad(k % 2)
        coeffs = {float(lr): R.adam_host_coeffs(lr, *betas, step) for lr in set(bank.lr.tolist())}
        ss = np.array([coeffs[float(lr)][0] for lr in bank.lr], np.float32)[bank.owner]
        bc2 = next(iter(coeffs.values()))[1]
        want = R.adam_f32(bank.p, g, bank.m, bank.v, ss, bc2, *betas, eps)
        p64, m64, v64, p_abs, m_abs, v_abs = R.adam_f64(bank.p, g, bank.m, bank.v, bank.lr[bank.owner], *betas, eps, step)
        _lib.check(lib.ego_adam_step(arr, len(bank.sizes), betas[0], betas[1], eps, step, _lib.stream_handle()), "ego_adam_step")
        got = bank.read()
        bank.check(got, want, (betas, eps, step))
        worst = max(worst, _frac(got[0] - p64, R.bound(R.K_ADAM_P, p_abs), live), _frac(got[1] - m64, R.bound(R.K_ADAM_M, m_abs), live),
                    _frac(got[2] - v64, R.bound(R.K_ADAM_V, v_abs), live))
        bank.p, bank.m, bank.v = got
    if step == 10 ** 6:
        assert bc2 == np.float32(1) and R.adam_host_coeffs(1.0, *betas, step)[0] == np.float32(1)   # 1 - beta^t has rounded to 1
    print(f"adam {betas} eps {eps}: hip == copy over {len(STEPS)} steps; |hip - f64| / bound {worst:.3f}")
    assert worst <= 1.0


def test_adam_step_graph_clock():
    """ego_adam_step_graph: the step count and the learning-rate scale live on the device.  t and the scale are exact (an increment, a
    product of doubles); the two derived coefficients go through the device's pow, which may differ from the host's in the last places:
    they are held to 4 x 2^-53 x (1 + beta^t / (1 - beta^t)), the last-place error of beta^t carried through 1 - beta^t.  The parameters
    have the bits of the float32 restatement driven by the clock the device computed."""
    betas, eps, factor = (0.9, 0.99), 1e-8, 0.977
    bank = Bank(seed=4)
    lib, arr = _lib.load(), bank.tensors()
    clock = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=DEV)
    ref = [0.0, 1.0, 0.0, 0.0]
    b1, b2 = float(np.float32(betas[0])), float(np.float32(betas[1]))
    worst = 0.0
    for k in range(5):
        g = bank.new_grad(k % 2)
        _lib.check(lib.ego_adam_step_graph(arr, len(bank.sizes), betas[0], betas[1], eps, factor, clock.data_ptr(), _lib.stream_handle()),
                   "ego_adam_step_graph")
        got = bank.read()
        dclock = clock.cpu().numpy()
        ref = R.adam_clock_f64(ref, *betas, factor)
        assert dclock[0] == ref[0] == k + 1 and dclock[1] == ref[1]
        for j, b in ((2, b1), (3, b2)):
            pw = b ** (k + 1)
            tol = 4 * 2.0 ** -53 * (1 + pw / (1 - pw)) * abs(ref[j])
            worst = max(worst, abs(dclock[j] - ref[j]) / tol)
            assert abs(dclock[j] - ref[j]) <= tol, (k, j, dclock[j], ref[j])
        ss = np.array([R.adam_graph_coeffs(lr, dclock)[0] for lr in bank.lr], np.float32)[bank.owner]
        want = R.adam_f32(bank.p, g, bank.m, bank.v, ss, R.adam_graph_coeffs(1.0, dclock)[1], *betas, eps)
        bank.check(got, want, ("graph", k))
        bank.p, bank.m, bank.v = got
    print(f"adam clock: t and lr scale exact, derived coefficients |hip - f64| / bound {worst:.3f}; parameters hip == copy over 5 steps")


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
def test_fused_adam_45_parameters_match_torch_adam(capturable):
    """Three groups of 15 (two launches per step), channel-last 4-D parameters among them, per-group lr with the reference's per-step decay
    (train.py:328-329; on the device in capturable mode) against torch.optim.Adam on the CPU: test_hip_train_extras.py's form and tolerance."""
    g = torch.Generator().manual_seed(2)
    kinds = [(1, 16, 10, 12), (1, 48, 30, 1), (27, 144), (128,), (3, 128), (1025,), (3, 32, 16), (1,), (1024,)]
    shapes = [kinds[i % len(kinds)] for i in range(45)]
    cpu = [torch.randn(*s, generator=g).requires_grad_(True) for s in shapes]
    dev = []
    for t in cpu:
        d = t.detach().to(DEV)
        if d.dim() == 4:
            d = d.contiguous(memory_format=torch.channels_last)
        dev.append(d.requires_grad_(True))
    groups = lambda ps: [dict(params=ps[:15], lr=0.02), dict(params=ps[15:30], lr=1e-3), dict(params=ps[30:], lr=0.1)]
    o_ref = torch.optim.Adam(groups(cpu), betas=(0.9, 0.99))
    o_dev = FusedAdam(groups(dev), betas=(0.9, 0.99), capturable=capturable, lr_factor=0.977 if capturable else 1.0)
    for it in range(6):
        for a, b in zip(cpu, dev):
            gr = torch.randn(a.shape, generator=g) * (10.0 ** -(it % 4))
            if it == 3:
                gr[..., ::2] = 0
            a.grad = gr
            b.grad = gr.to(DEV)
        o_ref.step(), o_dev.step()
        for grp_r, grp_d in zip(o_ref.param_groups, o_dev.param_groups):
            grp_r["lr"] *= 0.977
            if not capturable:
                grp_d["lr"] *= 0.977
        for i, (a, b) in enumerate(zip(cpu, dev)):
            assert float((a.detach() - b.detach().cpu()).abs().max()) <= 2e-6, (it, i, a.shape)
    assert o_dev.steps_taken() == 6 and abs(o_dev.current_lrs()[0] - 0.02 * 0.977 ** 6) <= 1e-9
