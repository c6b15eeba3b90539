"""GPU: inverse-CDF resampling (ego_sample_pdf_merge) on BOTH of its kernels - one wave per ray up to 256 + 256, one workgroup per ray
up to Sc + n_fine = 2048 - and ego_raw2alpha, at the sizes where a per-ray scan goes wrong: pass boundaries of the 64-wide scans, ragged
tails, the dispatch switch between the two kernels, equal keys in the merge, and the fallback sorting networks.

Truth is the oracle's sample_pdf / raw2alpha evaluated in float64.  Every fine sample is judged with the conditioning-aware bound of
tests/test_hip_parity.py::test_stage_sample_pdf (clause c): a float32 cdf carries ~1e-7 of rounding, which (u - cdf_lo) / denom turns
into 4e-7 / denom of the bin's width.  The inputs keep every cdf step clear of the reference's `denom < 1e-5` switch, so no entry is
excused; that the inputs are that well conditioned is itself asserted (the float32 oracle must stay within half of the bound)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from egonerf_amd import synth
from tests.helpers import make_model, make_oracle, maxerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
RGB_TOL = 1e-4
N = 7   # rays per case: the wave kernel's last block of four has one idle wave

WAVE = [(3, 1), (4, 2),      # minimum sizes; n_fine == 1 takes the linspace's special case
        (66, 65),            # nw = 64: exactly one full scan pass; the fine run is one past a 64-lane stride
        (67, 64),            # nw = 65: the second pass holds one element and reads the carry
        (130, 100),          # two full passes + none left over; fine sort padded 100 -> 128
        (256, 256)]          # the wave kernel's largest size: its LDS rows are full
WORKGROUP = [(257, 16), (16, 257),   # each side of the dispatch condition alone
             (258, 257),             # nw = 256: one full stride of the 256 threads
             (300, 700),             # n_out = 1000, padded to 1024 in the bitonic fallback
             (1024, 1024),           # n_out = 2048 = the kernel's capacity, no padding
             (2045, 3)]              # the longest cdf: 32 scan passes
WORST = {}   # kernel -> worst err / bound seen (printed; DESIGN.md 5 quotes it)


def hu(seed, stream, *shape):
    return torch.from_numpy(synth.hash_uniform(seed, stream, int(np.prod(shape))).reshape(shape).astype(np.float32))


def make_inputs(Sc, n_fine, seed=None):
    """The well-conditioned recipe of test_stage_sample_pdf: z sorted in [0, 12), interior weights in [0.05, 1), end weights 0, row 2
    all zero (uniform pdf); u hash-uniform in [0, 1)."""
    seed = 50 + Sc if seed is None else seed
    z = torch.sort(hu(seed, 0, N, Sc) * 12, -1)[0]
    w = torch.zeros(N, Sc)
    if Sc > 2:
        w[:, 1:-1] = 0.05 + 0.95 * hu(seed, 1, N, Sc - 2)
    w[2] = 0
    return z, w, hu(seed, 2, N, n_fine)


def eval_u(n_fine):
    """What the kernel uses for u = NULL: torch.linspace in float32."""
    return torch.linspace(0.0, 1.0, n_fine).expand(N, n_fine).contiguous()


def truth_and_bound(z, w, u):
    """float64 sample_pdf of (z, w) at u, and per entry 1e-5 + 4e-7 / denom * |width| from the float64 cdf's bin."""
    from oracle.egonerf_oracle import OracleScene
    n = u.shape[-1]
    mids = 0.5 * (z[:, 1:] + z[:, :-1])
    truth = OracleScene.sample_pdf(mids.double(), w[:, 1:-1].double(), n, u.double())
    w64 = w[:, 1:-1].double() + 1e-5
    cdf = torch.cat([torch.zeros(z.shape[0], 1, dtype=torch.float64), torch.cumsum(w64 / w64.sum(-1, keepdim=True), -1)], -1)
    uu = u.double().contiguous()
    idx = torch.searchsorted(cdf, uu, right=True)
    lo, hi = (idx - 1).clamp(min=0), idx.clamp(max=cdf.shape[-1] - 1)
    denom = torch.gather(cdf, -1, hi) - torch.gather(cdf, -1, lo)
    width = (torch.gather(mids.double(), -1, hi) - torch.gather(mids.double(), -1, lo)).abs()
    # every bin the truth uses is far from the reference's `denom < 1e-5 -> 1` switch (lo == hi only at u == 1: width 0, value = the bin)
    assert bool(((denom > 4e-5) | (lo == hi)).all()), float(denom[lo != hi].min())
    return truth, 1e-5 + 4e-7 / denom.clamp(min=1e-12) * width


def oracle32_ratio(z, w, u):
    """Worst err / bound of the float32 oracle against the float64 one: how well conditioned the inputs are."""
    from oracle.egonerf_oracle import OracleScene
    truth, bound = truth_and_bound(z, w, u)
    mids = 0.5 * (z[:, 1:] + z[:, :-1])
    z32 = OracleScene.sample_pdf(mids, w[:, 1:-1], u.shape[-1], u)
    return float(((z32.double() - truth).abs() / bound).max())


def run_kernel(z, w, u, use_coarse):
    """ego_sample_pdf_merge through the C ABI -> (z_out, z_new), both on the host."""
    from egonerf_amd import _lib
    lib = _lib.load()
    n, Sc = z.shape
    n_fine = u.shape[-1] if isinstance(u, torch.Tensor) else int(u)
    ud = u.to(DEV).contiguous() if isinstance(u, torch.Tensor) else None
    zt, wt = z.to(DEV).contiguous(), w.to(DEV).contiguous()
    z_out = torch.full((n, (Sc if use_coarse else 0) + n_fine), float("nan"), device=DEV)
    z_new = torch.full((n, n_fine), float("nan"), device=DEV)
    _lib.check(lib.ego_sample_pdf_merge(zt.data_ptr(), wt.data_ptr(), _lib.ptr(ud), n, Sc, n_fine, use_coarse, z_out.data_ptr(),
                                        z_new.data_ptr(), _lib.stream_handle()), "ego_sample_pdf_merge")
    torch.cuda.synchronize()
    return z_out.cpu(), z_new.cpu()


def check_case(z, w, u_or_none, n_fine, use_coarse, tag):
    """One launch: every fine sample within its bound of float64, and z_out the exact sort.  -> z_new."""
    u_ref = eval_u(n_fine) if u_or_none is None else u_or_none
    truth, bound = truth_and_bound(z, w, u_ref)
    z_out, z_new = run_kernel(z, w, n_fine if u_or_none is None else u_or_none, use_coarse)
    ratio = (z_new.double() - truth).abs() / bound
    worst = float(ratio.max())
    kernel = "wave" if z.shape[1] <= 256 and n_fine <= 256 else "workgroup"
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    print(f"sample_pdf {tag} Sc={z.shape[1]} n_fine={n_fine} use_coarse={use_coarse} [{kernel}]: worst err/bound {worst:.3f}, "
          f"worst |err| {float((z_new.double() - truth).abs().max()):.2e}, largest bound {float(bound.max()):.2e}")
    assert bool(torch.isfinite(z_new).all()) and worst <= 1.0, (tag, worst, int(ratio.argmax()))
    merged = torch.sort(torch.cat([z, z_new], -1) if use_coarse else z_new, -1)[0]
    assert torch.equal(z_out, merged), (tag, int((z_out != merged).sum()))   # the sort itself is exact (NaN = a slot left unwritten)
    return z_new


# ---- 1. stage op against float64, every entry, both kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("Sc,n_fine", WAVE + WORKGROUP)
def test_sample_pdf_vs_float64(Sc, n_fine, mode):
    z, w, u = make_inputs(Sc, n_fine)
    u_ref = eval_u(n_fine) if mode == "eval" else u
    r32 = oracle32_ratio(z, w, u_ref)
    assert r32 <= 0.5, r32    # the inputs are honest: float32 arithmetic alone stays within half of the bound
    if mode == "train" and n_fine > 2:
        zn = truth_and_bound(z, w, u)[0]
        assert bool((zn[:, 1:] < zn[:, :-1]).any())   # random u: the fine run comes out unsorted and reaches the sorting networks
    for use_coarse in (1, 0):
        check_case(z, w, None if mode == "eval" else u, n_fine, use_coarse, mode)
    print("worst err/bound so far:", WORST, " float32 oracle on this case:", round(r32, 3))


# ---- 1b. the same launches, bit for bit, against a recorded build -------------------------------------------------------------------
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_digests.json")


def sample_pdf_digests():
    """case -> [sha256 of z_out's bytes, sha256 of z_new's bytes] for every shape above, u = NULL and hash-uniform u, use_coarse 0 and 1.
    tools/capture_digests.py records this from another build of the library."""
    out = {}
    for Sc, n_fine in WAVE + WORKGROUP:
        z, w, u = make_inputs(Sc, n_fine)
        for mode in ("eval", "train"):
            for use_coarse in (0, 1):
                got = run_kernel(z, w, n_fine if mode == "eval" else u, use_coarse)
                out[f"{Sc}+{n_fine} {mode} use_coarse={use_coarse}"] = [hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest() for t in got]
    return out


def test_sample_pdf_bits_match_recorded():
    """Both kernels are deterministic (no atomics, every float operation an explicit _rn intrinsic or a double add in a fixed order), so a
    rewrite that keeps the arithmetic returns the recorded build's bytes: equality, no tolerance.  The fixture names its commit."""
    recorded = json.load(open(DIGESTS))["digests"]
    got = sample_pdf_digests()
    assert len(got) == 48 and sorted(got) == sorted(recorded)
    differs = [f"{case}: {name}" for case in got for name, a, b in zip(("z_out", "z_new"), got[case], recorded[case]) if a != b]
    assert not differs, differs


# ---- 2. ties and an unsorted coarse run --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sc,n_fine", [(130, 100), (300, 700)])
def test_sample_pdf_ties(Sc, n_fine):
    """Many equal coarse keys (z on a 0.25 grid: zero-width bins whose fine samples ARE a coarse key), equal fine keys (u on a 1/8 grid),
    one ray with a uniform pdf.  The merge ranks coarse keys before equal fine ones, each side by its own binary search: a slot written
    twice leaves another unwritten, which the exact comparison with the sort sees.  u as drawn (unsorted fine run: the wave kernel sorts it
    and merges, the workgroup kernel sorts everything), u sorted along the ray and u = NULL (both kernels merge)."""
    z, w, u = make_inputs(Sc, n_fine)
    z = torch.sort(torch.round(z * 4) / 4, -1)[0]
    u = torch.floor(u * 8) / 8
    w[5, 1:-1] = 1.0
    assert int((z[:, 1:] == z[:, :-1]).sum()) > N * Sc // 2 and int((z[:, 2:] == z[:, :-2]).sum()) > N * Sc // 4
    for tag, uu in (("ties", u), ("ties-sorted-u", torch.sort(u, -1)[0]), ("ties-eval", None)):
        u_ref = eval_u(n_fine) if uu is None else uu
        assert oracle32_ratio(z, w, u_ref) <= 0.5
        z_new = check_case(z, w, uu, n_fine, 1, tag)
        fine_on_coarse = (z_new[:, :, None] == z[:, None, :]).any(-1)
        equal_fine = torch.sort(z_new, -1)[0]
        # the case is what it claims to be: in every ray fine keys equal to coarse keys, and fine keys equal to one another
        assert bool((fine_on_coarse.sum(-1) >= 3).all()), fine_on_coarse.sum(-1)
        assert bool(((equal_fine[:, 1:] == equal_fine[:, :-1]).sum(-1) >= 3).all())
        check_case(z, w, uu, n_fine, 0, tag)


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("Sc,n_fine", [(130, 100), (300, 700)])
def test_sample_pdf_unsorted_coarse_run(Sc, n_fine, mode):
    """Two neighbouring coarse distances swapped in every ray: the wave kernel sorts everything (its `any_c` branch), the workgroup kernel
    takes its bitonic fallback.  The reference formula does not need sorted bins; the bound takes |width|."""
    z, w, u = make_inputs(Sc, n_fine)
    for r in range(N):
        k = 1 + (r * 37) % (Sc - 3)    # a different place in every ray, first / last pair included over the rays
        assert z[r, k] < z[r, k + 1]
        z[r, k], z[r, k + 1] = z[r, k + 1].clone(), z[r, k].clone()
    assert bool((z[:, 1:] < z[:, :-1]).any(-1).all())
    u_ref = eval_u(n_fine) if mode == "eval" else u
    assert oracle32_ratio(z, w, u_ref) <= 0.5
    check_case(z, w, None if mode == "eval" else u, n_fine, 1, "swapped-" + mode)


# ---- 3. host refusals (nothing is launched) ------------------------------------------------------------------------------------------
def test_sample_pdf_refusals():
    from egonerf_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4 * 2049, device=DEV)
    out = torch.full((4 * 2049,), 7.0, device=DEV)
    call = lambda n, Sc, nf: lib.ego_sample_pdf_merge(buf.data_ptr(), buf.data_ptr(), None, n, Sc, nf, 1, out.data_ptr(), None,
                                                      _lib.stream_handle())
    for Sc, nf, word in ((2, 4, b"Sc"), (8, 0, b"Sc"), (1025, 1024, b"2048"), (2046, 3, b"2048"), (3, 2046, b"2048")):
        assert call(4, Sc, nf) == -1, (Sc, nf)             # EGO_E_BADARG
        assert word in lib.ego_last_error(), (Sc, nf, lib.ego_last_error())
    assert call(0, 8, 8) == 0                               # EGO_OK: an empty batch is not an error
    assert call(1, 2045, 3) == 0 and call(1, 3, 2045) == 0  # ... and the largest sizes are accepted
    torch.cuda.synchronize()
    assert bool((out[2048:] == 7.0).all())                  # one ray was written, nothing behind it


def test_model_refuses_oversized_resampling():
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    model = make_model(cfg, synth.make_weights(cfg, seed=1234), DEV)
    rays = torch.from_numpy(synth.make_rays(4, seed=21)).to(DEV)
    with torch.no_grad(), pytest.raises(RuntimeError, match="2048"):   # an error, not images
        model(rays, n_coarse=1100, n_fine=1100, exp_sampling=True, resampling=True)
    torch.cuda.synchronize()
    with torch.no_grad():   # the model is usable afterwards
        rgb, *_ = model(rays, n_coarse=16, n_fine=16, exp_sampling=True, resampling=True)
    assert bool(torch.isfinite(rgb).all())


# ---- 4. whole render across the dispatch switch ----------------------------------------------------------------------------------------
RENDER = dict(n_coarse=260, n_fine=260, resampling=True)
RENDER_SEEDS = dict(weights=1234, rays=21, noise=61)   # chosen so that the two host conditions below hold (real weights are ill-conditioned
                                                       # for sample_pdf: thin cdf steps move float32 samples); both are asserted


@pytest.fixture(scope="module")
def render_case():
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    w = synth.make_weights(cfg, seed=RENDER_SEEDS["weights"])
    rays = torch.from_numpy(synth.make_rays(5, seed=RENDER_SEEDS["rays"]))
    jit, u = hu(RENDER_SEEDS["noise"], 0, 5, 260), hu(RENDER_SEEDS["noise"], 1, 5, 260)
    ref = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        o = make_oracle(cfg, w, dtype=dt)
        ref[name, "eval"] = o.forward(rays, **RENDER)
        out, inter = o.forward(rays, is_train=True, jitter=jit, u=u, keep=True, **RENDER)
        ref[name, "train"] = (out, inter["z"])
    return cfg, w, rays, jit, u, ref


def test_render_260_260_vs_oracle(render_case):
    cfg, w, rays, jit, u, ref = render_case
    # host conditions on the chosen seeds: float32 against float64 within half of each bound, fewer than 1 % of the samples moved
    for mode in ("eval", "train"):
        a = ref["f32", mode][0] if mode == "train" else ref["f32", mode]
        b = ref["f64", mode][0] if mode == "train" else ref["f64", mode]
        assert maxerr(a[0], b[0].float()) <= 0.5 * RGB_TOL and maxerr(a[1], b[1].float()) <= 0.5 * 1e-3 * 15.0, mode
    moved = (ref["f32", "train"][1].double() - ref["f64", "train"][1]).abs() > 1e-4
    assert float(moved.float().mean()) < 0.01
    model = make_model(cfg, w, DEV)
    with torch.no_grad():
        rgb, depth, *_ = model(rays.to(DEV), exp_sampling=True, **RENDER)
    want = ref["f32", "eval"]
    print("260+260 eval: rgb", maxerr(rgb, want[0]), "depth", maxerr(depth, want[1]))
    assert maxerr(rgb, want[0]) <= RGB_TOL and maxerr(depth, want[1]) <= 1e-3 * 15.0
    rgb, depth, *_ = model(rays.to(DEV), is_train=True, exp_sampling=True, jitter=jit.to(DEV), u=u.to(DEV), **RENDER)
    want, z_want = ref["f32", "train"]
    z = model.last_train_z
    assert z.shape == (5, 520) and bool((z[:, 1:] >= z[:, :-1]).all())
    share = float(((z.cpu() - z_want).abs() > 1e-4).float().mean())
    print("260+260 train: rgb", maxerr(rgb, want[0]), "depth", maxerr(depth, want[1]), "moved share", share)
    assert maxerr(rgb, want[0]) <= RGB_TOL and maxerr(depth, want[1]) <= 1e-3 * 15.0
    assert share <= 0.02


# ---- 5. ego_raw2alpha across its 64-sample passes ----------------------------------------------------------------------------------------
def test_raw2alpha_across_passes():
    """One wave per ray, the transmittance carried from pass to pass: one pass with a ragged tail (1, 63), exactly full (64), one element
    in the second pass (65), two passes + tail (130), nine passes (513).  As close to float64 as float32 arithmetic is, within a factor."""
    from egonerf_amd.model import raw2alpha
    from oracle.egonerf_oracle import OracleScene
    for S in (1, 63, 64, 65, 130, 513):
        sigma = hu(500 + S, 0, N, S) * 3
        if S >= 63:
            sigma[1, 60:min(S, 70)] = 1e4    # opaque run across the first pass boundary: 1 - alpha underflows to 0 (+1e-10)
        else:
            sigma[1] = 1e4
        sigma[4] = 0.0
        dist = 0.001 + 0.299 * hu(500 + S, 1, N, S)
        got = raw2alpha(sigma.to(DEV), dist.to(DEV))
        truth = OracleScene.raw2alpha(sigma.double(), dist.double())
        ref32 = OracleScene.raw2alpha(sigma, dist)
        errs = []
        for name, g, t, r in zip(("alpha", "weight", "bg_weight"), got, truth, ref32):
            assert g.shape == t.shape, (S, name)
            e, e32 = float((g.cpu().double() - t).abs().max()), float((r.double() - t).abs().max())
            errs.append(f"{name} {e:.1e} (float32 oracle {e32:.1e})")
            assert e <= max(1e-6, 4 * e32), (S, name, e, e32)
        print(f"raw2alpha S={S}: " + ", ".join(errs))
        assert bool((got[0][4] == 0).all()) and bool((got[1][4] == 0).all()) and float(got[2][4]) == 1.0   # the empty ray, exactly
