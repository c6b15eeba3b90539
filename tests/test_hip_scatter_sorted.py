"""GPU: the atomic-free, bit-reproducible table-gradient scatter (csrc/ego_scatter_sorted.hip; SURVEY 5 "sorted-segment mode", VERDICT r04
item 3) against the float-atomic scatter of rounds 1-4 (same mathematics, another summation order) and against itself (same bits twice).
Backward of F.grid_sample in compute_densityfeature / compute_appfeature (models/EgoNeRF.py:291-347, :349-413) under train.py:312-314."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from egonerf_amd import _lib, synth, train
from egonerf_amd.train import _grad_struct, table_params
from tests.helpers import make_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _scatter_both(model, coords, dfeat, dv, N, S):
    """-> {"atomic": (density grads, app grads), "sorted": ...} through the C ABI on explicit inputs."""
    lib, st = _lib.load(), _lib.stream_handle()
    sc = model.scene(training=True)
    dens, app = table_params(model, "density"), table_params(model, "app")
    out = {}
    M = N * S
    for mode in ("atomic", "sorted", "sorted_again", "sorted_absmax", "sorted_separate"):
        gd = [torch.zeros_like(p) if mode == "atomic" else torch.full_like(p, float("nan")) for p in dens]   # the sorted form must write every texel
        ga = [torch.zeros_like(p) if mode == "atomic" else torch.full_like(p, float("nan")) for p in app]
        sd, sa = _grad_struct(gd), _grad_struct(ga)
        # v15: "sorted" = one pass (lines in fixed point, dv_absmax found by the call); "sorted_absmax": the caller hands max |dv| over
        # the valid samples, as ego_shade_backward does; "sorted_separate": the two-pass form of v14 (EGO_SORTED_LINES is read per call)
        absmax = None
        if mode == "sorted_absmax":
            blk = dv.view(-1, 9, 32, 16)
            valid = (torch.arange(blk.shape[0] * 32, device=dv.device).view(-1, 1, 32, 1) < M) if M % 32 else None
            absmax = (blk.abs() if valid is None else (blk.abs() * valid)).max().reshape(1).contiguous() if M else torch.zeros(1, device=dv.device)
        os.environ.pop("EGO_SORTED_LINES", None)
        if mode == "sorted_separate":
            os.environ["EGO_SORTED_LINES"] = "separate"
        if mode == "atomic":
            _lib.check(lib.ego_scatter_density(sc, C.byref(sd), coords.data_ptr(), dfeat.data_ptr(), N, S, st), "scatter_density")
            _lib.check(lib.ego_scatter_app(sc, C.byref(sa), coords.data_ptr(), dv.data_ptr(), N, S, st), "scatter_app")
        else:
            nbytes = lib.ego_scatter_sorted_workspace_bytes(sc, N, S)
            assert nbytes > 0
            ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
            _lib.check(lib.ego_scatter_sort(sc, coords.data_ptr(), N, S, ws.data_ptr(), nbytes, st), "scatter_sort")
            _lib.check(lib.ego_scatter_density_sorted(sc, C.byref(sd), coords.data_ptr(), dfeat.data_ptr(), N, S, ws.data_ptr(), nbytes, st), "density_sorted")
            _lib.check(lib.ego_scatter_app_sorted(sc, C.byref(sa), coords.data_ptr(), dv.data_ptr(), _lib.ptr(absmax), None, None, 0, N, S, ws.data_ptr(), nbytes, st), "app_sorted")
        torch.cuda.synchronize()
        os.environ.pop("EGO_SORTED_LINES", None)
        out[mode] = (gd, ga)
    return out


@pytest.mark.parametrize("n_voxel,N,S,spread", [(20 ** 3, 48, 32, 1.0), (40 ** 3, 333, 45, 1.15), (27e6, 512, 256, 1.0),
                                                (216e6, 96, 64, 1.05),    # grid [300, 346, 1036]: 20-bit cell keys, three radix passes (odd ping-pong)
                                                (20 ** 3, 1, 2, 1.0)])    # the smallest call there is
def test_sorted_scatter_equals_the_atomic_one_and_itself(n_voxel, N, S, spread):
    """Random normalised coordinates (spread > 1: some taps and whole samples beyond the table border: zero padding), random dfeat with
    exact zeros, random dv in k_shade_bwd's blocked layout."""
    cfg = synth.SceneConfig(n_voxel=n_voxel)
    model = make_model(cfg, synth.make_weights(cfg, seed=21), DEV)
    M = N * S
    g = torch.Generator().manual_seed(3)
    coords = (torch.rand(N, S, 4, generator=g) * 2 - 1) * spread
    coords[..., 3] = (torch.rand(N, S, generator=g) > 0.5).float()
    # rays are coherent: consecutive samples in neighbouring cells (as the march writes them) for half of the rays
    walk = torch.cumsum(torch.rand(N, S, 3, generator=g) * 0.02, dim=1) - 0.9
    coords[: N // 2, :, :3] = walk[: N // 2].clamp(-spread, spread)
    if S >= 4:
        coords[0, :4, 0] = torch.tensor([-1.0, 1.0, -1.3, 1.3])   # exactly on / beyond the border
    dfeat = torch.randn(N, S, generator=g)
    dfeat[torch.rand(N, S, generator=g) < 0.3] = 0.0
    Mp = (M + 31) // 32 * 32
    dv = torch.randn(Mp * 144, generator=g)
    coords, dfeat, dv = coords.to(DEV).contiguous(), dfeat.to(DEV).contiguous(), dv.to(DEV)
    out = _scatter_both(model, coords, dfeat, dv, N, S)
    for fi, field in enumerate(("density", "app")):
        for k, (a, s, s2, s3, sep) in enumerate(zip(out["atomic"][fi], out["sorted"][fi], out["sorted_again"][fi], out["sorted_absmax"][fi],
                                                    out["sorted_separate"][fi])):
            assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(sep).all()), (field, k)   # every texel written (the buffers started as NaN)
            assert torch.equal(s, s2), (field, k)                                # same bits twice
            assert torch.equal(s, s3), (field, k)                                # ... and with the caller's max |dv| (the same value -> the same unit)
            scale = max(float(a.abs().max()), 1e-20)
            assert float((a - s).abs().max()) <= 3e-5 * scale, (field, k, float((a - s).abs().max()) / scale)   # summation order only (thousands of terms per texel at the large size)
            assert float((sep - s).abs().max()) <= 3e-5 * scale, (field, k)
            # (planes: the one-pass form adds a cell's samples per LINE BLOCK and then the blocks - another order than the two-pass form's
            # where a line needs more than one block; covered by the 3e-5 bound above)
            assert M < 64 or float(s.abs().max()) > 0


def test_an_empty_batch_zero_fills_the_tables():
    """the sorted scatters promise 'every texel is written' and train.py allocates the gradient tables with torch.empty.
    The tiny scene, and one with three unequal axis resolutions, one of them odd: there no two planes and no two lines of a field have
    one size, so a table size taken from the wrong axes (vm_plane_elems / vm_line_elems, csrc/ego_device.h) leaves texels unwritten or
    writes into the guard floats on either side of a table."""
    for cfg in (synth.SceneConfig(n_voxel=20 ** 3), synth.SceneConfig(n_voxel=20 ** 3, grid=[6, 5, 8])):
        model = make_model(cfg, synth.make_weights(cfg, seed=21), DEV)
        lib, st = _lib.load(), _lib.stream_handle()
        sc = model.scene(training=True)
        GUARD = 64
        bufs = {kind: [torch.full((p.numel() + 2 * GUARD,), float("nan"), device=DEV) for p in table_params(model, kind)] for kind in ("density", "app")}
        gd, ga = ([b[GUARD:-GUARD] for b in bufs[kind]] for kind in ("density", "app"))
        sd, sa = _grad_struct(gd), _grad_struct(ga)
        nbytes = lib.ego_scatter_sorted_workspace_bytes(sc, 0, 8)
        assert nbytes > 0
        ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
        _lib.check(lib.ego_scatter_sort(sc, None, 0, 8, ws.data_ptr(), nbytes, st), "scatter_sort")
        _lib.check(lib.ego_scatter_density_sorted(sc, C.byref(sd), None, None, 0, 8, ws.data_ptr(), nbytes, st), "density_sorted")
        _lib.check(lib.ego_scatter_app_sorted(sc, C.byref(sa), None, None, None, None, None, 0, 0, 8, ws.data_ptr(), nbytes, st), "app_sorted")
        torch.cuda.synchronize()
        for g in gd + ga:
            assert float(g.abs().max()) == 0.0
        for b in bufs["density"] + bufs["app"]:   # and not a float beyond a table
            assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[-GUARD:]).all()), cfg.grid


def _float64_grid_sample_gradients(cfg, weights, coords, dfeat, dv_ref, dtype=torch.float64):
    """Independent truth for the stand-alone scatters: float64 autograd THROUGH the oracle's F.grid_sample calls
    (align_corners=True, zero padding: grid_sampler_2d_backward is an index_add of the 18 taps x C channels per sample) on the CPU.
    coords [N,S,4] normalised (r, theta, phi, is_yang); dfeat [N,S] = dL/d(density feature); dv_ref [M,144] = dL/d(plane*line products)
    in the reference's channel order.  -> (density grads, app grads) in table_params() order, reference-shaped float64 tensors."""
    from tests.helpers import make_oracle
    sc = make_oracle(cfg, weights, dtype=dtype)
    c4 = coords.reshape(-1, 4).to(dtype).cpu()
    c7 = torch.cat([c4[:, :3], c4[:, :3], c4[:, 3:4]], -1)     # the same normalised triple in the yin and the yang slot; the flag picks the tables
    keys = lambda kind: [f"{kind}_{what}_{g}.{i}" for g in ("yin", "yang") for what in ("plane", "line") for i in range(3)]
    for k in keys("density") + keys("app"):
        sc.w[k] = sc.w[k].clone().requires_grad_(True)
    loss_d = (sc.density_feature(c7) * dfeat.reshape(-1).to(dtype).cpu()).sum()      # sum_i relu(sum_c P L): EgoNeRF.py:291-347
    gd = torch.autograd.grad(loss_d, [sc.w[k] for k in keys("density")], allow_unused=True)
    gd = [torch.zeros_like(sc.w[k]) if g is None else g for g, k in zip(gd, keys("density"))]
    dvr = dv_ref.to(dtype).cpu()
    loss_a = 0.0
    is_yin = c7[:, -1] == 0
    for g, sel in (("yin", is_yin), ("yang", ~is_yin)):
        if bool(sel.any()):
            taps = sc._vm_taps([sc.table("app", "plane", g, i) for i in range(3)], [sc.table("app", "line", g, i) for i in range(3)], c7[sel][:, :3])
            prod = torch.cat([P * L for P, L in taps])                                  # [144, m]: EgoNeRF.py:349-413 before basis_mat
            loss_a = loss_a + (prod.T * dvr[sel]).sum()
    ga = torch.autograd.grad(loss_a, [sc.w[k] for k in keys("app")], allow_unused=True)
    ga = [torch.zeros_like(sc.w[k]) if g is None else g for g, k in zip(ga, keys("app"))]
    return list(gd), ga


def _blocked_dv(dv_ref, M):
    """[M,144] (reference channel order plane * 48 + c) -> k_shade_bwd's blocked layout [tile of 32][plane * 3 + c / 16][sample][c % 16]."""
    Mp = (M + 31) // 32 * 32
    full = torch.zeros(Mp, 144)
    full[:M] = dv_ref
    return full.view(Mp // 32, 32, 9, 16).permute(0, 2, 1, 3).contiguous().view(-1)


@pytest.mark.parametrize("n_voxel,N,S,spread,tol64", [(27e6, 512, 256, 1.0, 3e-5),       # the headline grid [150, 172, 516], 131 072 samples
                                                      (216e6, 96, 64, 1.05, 1.5e-4),     # 20-bit cell keys, samples beyond the border
                                                      (40 ** 3, 333, 45, 1.15, 3e-5)])
def test_scatters_against_float64_grid_sample_backward(n_voxel, N, S, spread, tol64):
    """Both forms of both scatters (sorted and float-atomic) against float64 autograd through F.grid_sample - the thing
    models/EgoNeRF.py:316-345, :377-407 differentiate - at 3e-5 of each table's largest gradient.  (A density sample whose per-plane channel
    sum lies within float32 rounding of 0 could take the other ReLU branch than float64 does; on these seeded inputs none does - the
    kernels are deterministic, so this is a fixed property of the case, not a flake.)

    On the [300, 346, 1036] grid the float64 figure is dominated by the COORDINATES, not by the sums: a float32 pixel coordinate near
    1 000 carries half an ulp = 3e-5 of a texel, so an interpolation weight - and with 6 144 samples over 10^5 texels, a whole texel's
    gradient - is off by that much against float64 whatever the kernel does (the reference's float32 grid_sample has the same error).
    There the float64 bound is 1.5e-4 and the kernels are ALSO held to 3e-5 of the reference's own arithmetic: float32 autograd through
    the same F.grid_sample calls (a few terms per texel: its summation error is negligible)."""
    cfg = synth.SceneConfig(n_voxel=n_voxel)
    weights = synth.make_weights(cfg, seed=21)
    model = make_model(cfg, weights, DEV)
    M = N * S
    g = torch.Generator().manual_seed(5)
    coords = (torch.rand(N, S, 4, generator=g) * 2 - 1) * spread
    coords[..., 3] = (torch.rand(N, S, generator=g) > 0.5).float()
    walk = torch.cumsum(torch.rand(N, S, 3, generator=g) * 0.02, dim=1) - 0.9
    coords[: N // 2, :, :3] = walk[: N // 2].clamp(-spread, spread)
    coords[0, :4, 0] = torch.tensor([-1.0, 1.0, -1.3, 1.3])
    dfeat = torch.randn(N, S, generator=g)
    dfeat[torch.rand(N, S, generator=g) < 0.3] = 0.0
    dv_ref = torch.randn(M, 144, generator=g)
    ref_d, ref_a = _float64_grid_sample_gradients(cfg, weights, coords, dfeat, dv_ref)
    ref32 = _float64_grid_sample_gradients(cfg, weights, coords, dfeat, dv_ref, dtype=torch.float32) if tol64 > 3e-5 else None
    out = _scatter_both(model, coords.to(DEV).contiguous(), dfeat.to(DEV).contiguous(), _blocked_dv(dv_ref, M).to(DEV), N, S)
    worst = 0.0
    for mode in ("sorted", "atomic"):
        for fi, (field, refs) in enumerate((("density", ref_d), ("app", ref_a))):
            for k, (got, ref) in enumerate(zip(out[mode][fi], refs)):
                assert got.shape == ref.shape, (field, k, got.shape, ref.shape)
                scale = max(float(ref.abs().max()), 1e-20)
                err = float((got.double().cpu() - ref).abs().max()) / scale
                worst = max(worst, err)
                assert err <= tol64, (mode, field, k, err)
                assert float(ref.abs().max()) > 0
                if ref32 is not None:
                    e32 = float((got.double().cpu() - ref32[fi][k].double()).abs().max()) / scale
                    assert e32 <= 3e-5, (mode, field, k, e32, "vs float32 autograd")
    print(f"scatter vs float64 grid_sample backward: worst {worst:.2e} of a table's largest gradient")


def test_training_gradients_are_bit_reproducible_and_match_the_atomic_path(golden):
    """The whole differentiable step on the tiny golden scene: default (sorted scatters, ordered weight-gradient sums) twice -> identical
    bits in all 32 gradients; against model.deterministic_scatter = False (float atomics) -> equal to summation-order rounding; both
    meet the reference's autograd goldens (tests/test_hip_train.py asserts that for the default)."""
    fx = golden("tiny")
    cfg = synth.SceneConfig(n_voxel=int(fx["n_voxel"]))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)

    def grads(det):
        model = make_model(cfg, synth.make_weights(cfg, seed=int(fx["seed_weights"])), DEV)
        model.train()
        model.deterministic_scatter = det
        rgb, *_ = model(T(fx["rays"]), is_train=True, n_coarse=16, n_fine=16, exp_sampling=True, resampling=True, use_coarse_sample=True,
                        jitter=T(fx["tr_jitter"]), u=T(fx["tr_u"]))
        torch.mean((rgb - T(fx["bw_gt"])) ** 2).backward()
        return {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    a, b, c = grads(True), grads(True), grads(False)
    assert len(a) == 32
    for k in a:
        assert torch.equal(a[k], b[k]), k
        ref = fx["bw_grad/" + k]
        scale = max(float(np.abs(ref).max()), 1e-12)
        assert float((a[k] - c[k]).abs().max()) <= 2e-5 * scale, k
        assert float(np.abs(a[k].cpu().numpy() - ref).max()) <= 2e-4 * scale, k


def test_fixed_point_line_sums_are_at_least_as_close_to_float64_as_float_sums():
    """The one-pass form adds a line's contributions as 64-bit fixed-point integers (unit >= 40 bits below the largest possible
    contribution), the two-pass form as float32 partial sums.  On the headline grid (131 072 samples, ~800 per line texel) the
    fixed-point sums must not be farther from float64 autograd than the float sums are - and a non-finite gradient input must give
    NaN line gradients, as a float sum's would be (the fixed-point conversion of a NaN is not a number either way: the call says so)."""
    cfg = synth.SceneConfig(n_voxel=27e6)
    weights = synth.make_weights(cfg, seed=21)
    model = make_model(cfg, weights, DEV)
    N, S = 512, 256
    M = N * S
    g = torch.Generator().manual_seed(11)
    coords = torch.rand(N, S, 4, generator=g) * 2 - 1
    coords[..., 3] = (torch.rand(N, S, generator=g) > 0.5).float()
    dfeat = torch.randn(N, S, generator=g)
    dv_ref = torch.randn(M, 144, generator=g)
    ref_d, ref_a = _float64_grid_sample_gradients(cfg, weights, coords, dfeat, dv_ref)
    out = _scatter_both(model, coords.to(DEV).contiguous(), dfeat.to(DEV).contiguous(), _blocked_dv(dv_ref, M).to(DEV), N, S)
    for fi, refs in enumerate((ref_d, ref_a)):
        for k in (3, 4, 5, 9, 10, 11):   # the six line tables of a field (table_params order: planes 0-2, lines 3-5 per grid)
            ref = refs[k]
            scale = float(ref.abs().max())
            e_fx = float((out["sorted"][fi][k].double().cpu() - ref).abs().max()) / scale
            e_fl = float((out["sorted_separate"][fi][k].double().cpu() - ref).abs().max()) / scale
            assert e_fx <= 1.05 * e_fl + 1e-7, (fi, k, e_fx, e_fl)   # (both ~1e-5 of max: the float32 factors of a contribution, not its sum, set it)
    bad = dfeat.clone()
    bad[3, 5] = float("nan")
    out = _scatter_both(model, coords.to(DEV).contiguous(), bad.to(DEV).contiguous(), _blocked_dv(dv_ref, M).to(DEV), N, S)
    for k in (3, 4, 5, 9, 10, 11):
        assert bool(torch.isnan(out["sorted"][0][k]).all()), k


def test_fixed_point_line_sums_do_not_overflow_when_every_sample_hits_one_texel():
    """The unit of the fixed-point line sums leaves ceil(log2(N S)) bits of headroom for a texel that receives EVERY sample's largest
    possible contribution.  65 536 identical samples (one cell, weights (1, 0) on every axis after rounding the coordinates onto a texel)
    with dfeat = dv = the largest magnitude in the batch: the line texel's gradient is M x d x plane value, far above any single
    contribution - and must come out exact to float32 rounding of a single contribution, in both fields (the planes' ordered float32
    chains of 65 536 equal terms, by contrast, carry their own 5e-4: the fixed-point sums are the MORE accurate ones here)."""
    cfg = synth.SceneConfig(n_voxel=20 ** 3)
    weights = synth.make_weights(cfg, seed=21)
    model = make_model(cfg, weights, DEV)
    N, S = 256, 256
    M = N * S
    res = [int(v) for v in model.gridSize.tolist()]          # (N_r, N_theta, N_phi)
    tex = [3, 4, 5]                                           # an interior texel per axis: x^ = 2 i / (n - 1) - 1 lands on it exactly enough
    xyz = [2.0 * t / (n - 1) - 1.0 for t, n in zip(tex, res)]
    coords = torch.tensor(xyz + [0.0]).repeat(N, S, 1).contiguous()
    dfeat = torch.full((N, S), 3.0)
    dv_ref = torch.full((M, 144), -2.0)
    ref_d, ref_a = _float64_grid_sample_gradients(cfg, weights, coords, dfeat, dv_ref)
    out = _scatter_both(model, coords.to(DEV), dfeat.to(DEV), _blocked_dv(dv_ref, M).to(DEV), N, S)
    for fi, refs in enumerate((ref_d, ref_a)):
        for k, (got, ref) in enumerate(zip(out["sorted"][fi], refs)):
            scale = float(ref.abs().max())
            if k >= 6:   # every sample lies in the yin grid: the yang tables' gradients are exactly 0 (and written)
                assert scale == 0.0 and float(got.abs().max()) == 0.0, (fi, k)
                continue
            assert scale > 1e3 or fi == 0, (fi, k, scale)      # sums of 65 536 terms
            err = float((got.double().cpu() - ref).abs().max()) / max(scale, 1e-30)
            # planes: 65 536 equal terms added one after the other in float32 (a real cell holds <= ~350 samples) - 5e-4 is that
            # chain's own rounding; lines: integer sums, exact up to the float32 factors of a contribution
            assert err <= (2e-3 if k % 6 < 3 else 2e-6), (fi, k, err)
            assert torch.equal(got, out["sorted_again"][fi][k])


def test_fixed_point_unit_follows_the_batch_not_a_constant():
    """Gradients 2^-60 small and 2^40 large go through the same kernels: the unit is derived from max |d| x max |plane texel| of the call,
    so scaling d by a power of two scales every gradient by exactly that power of two (bit for bit: float32 products and sums by a power
    of two are exact without overflow / underflow, and the fixed-point unit moves with it)."""
    cfg = synth.SceneConfig(n_voxel=24 ** 3)
    weights = synth.make_weights(cfg, seed=21)
    model = make_model(cfg, weights, DEV)
    N, S = 64, 48
    M = N * S
    g = torch.Generator().manual_seed(2)
    coords = torch.rand(N, S, 4, generator=g) * 2 - 1
    coords[..., 3] = (torch.rand(N, S, generator=g) > 0.5).float()
    dfeat = torch.randn(N, S, generator=g)
    dv_ref = torch.randn(M, 144, generator=g)
    base = _scatter_both(model, coords.to(DEV), dfeat.to(DEV), _blocked_dv(dv_ref, M).to(DEV), N, S)["sorted"]
    for e in (-60, 40):
        f = 2.0 ** e
        got = _scatter_both(model, coords.to(DEV), (dfeat * f).to(DEV), _blocked_dv(dv_ref * f, M).to(DEV), N, S)["sorted"]
        for fi in range(2):
            for k, (a, b) in enumerate(zip(got[fi], base[fi])):
                assert torch.equal(a, b * f), (e, fi, k, float((a - b * f).abs().max()))


def test_basis_gradient_rides_along_in_the_appearance_scatter():
    """ABI v15, late round 6: ego_scatter_app_sorted(dfe, gbasis) returns d(basis)[32 g + slot][plane x 48 + channel] = sum over the grid's
    samples of dfe[s][slot] x (plane value x line value)[s][channel] - the product ego_weight_grad(dfe, v dump) used to take - from the
    walk's own interpolated values.  Against float64 (the oracle's F.grid_sample taps) at 2e-5 of the largest element (bf16 hi + rounded
    residual operands: ~17 bits each), bit-identical twice, and the table gradients unchanged by the extra output."""
    from tests.helpers import make_oracle
    cfg = synth.SceneConfig(n_voxel=27e6)
    weights = synth.make_weights(cfg, seed=21)
    model = make_model(cfg, weights, DEV)
    N, S = 512, 96
    M = N * S
    g = torch.Generator().manual_seed(17)
    coords = (torch.rand(N, S, 4, generator=g) * 2 - 1) * 1.05
    coords[..., 3] = (torch.rand(N, S, generator=g) > 0.4).float()
    dv_ref = torch.randn(M, 144, generator=g)
    dfe = torch.randn(M, 32, generator=g) * torch.rand(M, 1, generator=g) * 1e-3
    lib, st = _lib.load(), _lib.stream_handle()
    sc = model.scene(training=True)
    cd, dvd, dfed = coords.to(DEV).contiguous(), _blocked_dv(dv_ref, M).to(DEV), dfe.to(DEV).contiguous()
    nbytes = lib.ego_scatter_sorted_workspace_bytes(sc, N, S)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    _lib.check(lib.ego_scatter_sort(sc, cd.data_ptr(), N, S, ws.data_ptr(), nbytes, st), "scatter_sort")
    outs = []
    for with_basis in (True, True, False):
        ga = [torch.full_like(p, float("nan")) for p in table_params(model, "app")]
        sa = _grad_struct(ga)
        gb = torch.full((64, 160), float("nan"), device=DEV)
        _lib.check(lib.ego_scatter_app_sorted(sc, C.byref(sa), cd.data_ptr(), dvd.data_ptr(), None, dfed.data_ptr() if with_basis else None,
                                              gb.data_ptr() if with_basis else None, 160 if with_basis else 0, N, S, ws.data_ptr(), nbytes, st), "app_sorted")
        torch.cuda.synchronize()
        outs.append((ga, gb))
    for k, (a, b) in enumerate(zip(outs[0][0], outs[1][0])):
        assert torch.equal(a, b), ("run to run", k, float((a - b).abs().max()))
    for k, (a, b) in enumerate(zip(outs[0][0], outs[2][0])):
        # the tables do not notice the extra product - up to the last bit of a contribution: the two template instantiations are compiled with
        # fp-contract(fast), and the compiler fuses different multiply-adds in them (each form is bit-reproducible by itself: above)
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()), ("with / without the basis product", k, float((a - b).abs().max()))
    assert torch.equal(outs[0][1][:, :144], outs[1][1][:, :144])          # same bits twice (columns 144.. of the [64][160] block are not the call's)
    assert bool(torch.isfinite(outs[0][1][:, :144]).all())
    got = outs[0][1][:, :144].double().cpu()
    # float64 truth from the oracle's taps
    o = make_oracle(cfg, weights, dtype=torch.float64)
    c4 = coords.reshape(-1, 4).double()
    ref = torch.zeros(64, 144, dtype=torch.float64)
    for gi, (name, sel) in enumerate((("yin", c4[:, 3] == 0), ("yang", c4[:, 3] != 0))):
        taps = o._vm_taps([o.table("app", "plane", name, i) for i in range(3)], [o.table("app", "line", name, i) for i in range(3)], c4[sel][:, :3])
        v = torch.cat([P * L for P, L in taps])          # [144, m]
        ref[32 * gi: 32 * gi + 32] = dfe[sel].double().T @ v.T
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max()) / scale
    assert err <= 2e-5, err


def test_walk_rederives_dv_from_the_feature_slot_gradients():
    """ABI v16: ego_scatter_app_sorted(dv = NULL) - the walk takes dv = basis_g^T dfe itself (scaled fp16 hi / lo three-term MFMA on the 27 slot
    gradients of the sample's own grid: ego_shade_backward's arithmetic for that product) instead of reading ego_shade_backward's 576-byte dv row.  Held against the same call fed a float64
    dv = dfe @ basis_g (rounded to fp32): tables within 2e-6 of the largest texel gradient (two ~22-bit operands), the d(basis) by-product
    unchanged at that order, the same bits twice, NaN-poisoning through max |dfe|, and the argument checks."""
    cfg = synth.SceneConfig(n_voxel=27e6)
    weights = synth.make_weights(cfg, seed=22)
    model = make_model(cfg, weights, DEV)
    N, S = 512, 96
    M = N * S
    g = torch.Generator().manual_seed(18)
    coords = (torch.rand(N, S, 4, generator=g) * 2 - 1) * 1.05
    coords[..., 3] = (torch.rand(N, S, generator=g) > 0.4).float()
    fmap = train._layout(2, 32, "cpu")                       # dfe column -> feature (-1: padding, zero in ego_shade_backward's output)
    dfe = torch.randn(M, 32, generator=g) * torch.rand(M, 1, generator=g) * 1e-3
    dfe[:, fmap < 0] = 0.0
    basis = [model.basis_mat_yin.weight.detach().double().cpu(), model.basis_mat_yang.weight.detach().double().cpu()]   # [27][144] each
    sel = fmap >= 0
    dv_ref = torch.zeros(M, 144, dtype=torch.float64)
    yang = coords.reshape(M, 4)[:, 3] != 0
    for gi, rows in enumerate((~yang, yang)):
        dv_ref[rows] = dfe[rows][:, sel].double() @ basis[gi][fmap[sel]]
    dv_ref = dv_ref.float()
    lib, st = _lib.load(), _lib.stream_handle()
    sc = model.scene(training=True)
    cd, dvd, dfed = coords.to(DEV).contiguous(), _blocked_dv(dv_ref, M).to(DEV), dfe.to(DEV).contiguous()
    nbytes = lib.ego_scatter_sorted_workspace_bytes(sc, N, S)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    _lib.check(lib.ego_scatter_sort(sc, cd.data_ptr(), N, S, ws.data_ptr(), nbytes, st), "scatter_sort")
    dfe_max = dfe.abs().max().reshape(1).to(DEV)
    dv_max = dv_ref.abs().max().reshape(1).to(DEV)

    def run(dv, amax, dfe_t=dfed):
        ga = [torch.full_like(p, float("nan")) for p in table_params(model, "app")]
        gb = torch.full((64, 160), float("nan"), device=DEV)
        sa = _grad_struct(ga)
        _lib.check(lib.ego_scatter_app_sorted(sc, C.byref(sa), cd.data_ptr(), _lib.ptr(dv), _lib.ptr(amax), dfe_t.data_ptr(), gb.data_ptr(), 160, N, S,
                                              ws.data_ptr(), nbytes, st), "app_sorted")
        torch.cuda.synchronize()
        return ga, gb

    want, want_gb = run(dvd, dv_max)
    got, got_gb = run(None, dfe_max)
    again, again_gb = run(None, dfe_max)
    for k, (a, b) in enumerate(zip(got, again)):
        assert torch.equal(a, b), ("run to run", k)
    assert torch.equal(got_gb[:, :144], again_gb[:, :144])
    for k, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(a).all()), k
        err = float((a - b).abs().max()) / float(b.abs().max())
        assert err <= 2e-6, ("re-derived dv vs dv handed over", k, err)
    assert float((got_gb[:, :144] - want_gb[:, :144]).abs().max()) <= 1e-6 * float(want_gb[:, :144].abs().max())
    # a non-finite feature gradient arrives as max |dfe| = NaN bits: every line texel is NaN (no silent integer overflow), as with dv handed over
    bad = dfed.clone(); bad[123, 3] = float("nan")
    nan_max = torch.full((1,), float("nan"), device=DEV)
    poisoned, _ = run(None, nan_max, bad)
    for k in (3, 4, 5, 9, 10, 11):
        assert bool(torch.isnan(poisoned[k]).all()), k
    # dv == NULL needs all of dfe, gbasis and max |dfe|
    ga = [torch.zeros_like(p) for p in table_params(model, "app")]
    sa = _grad_struct(ga)
    assert lib.ego_scatter_app_sorted(sc, C.byref(sa), cd.data_ptr(), None, None, dfed.data_ptr(), got_gb.data_ptr(), 160, N, S, ws.data_ptr(), nbytes, st) != 0
    assert lib.ego_scatter_app_sorted(sc, C.byref(sa), cd.data_ptr(), None, dfe_max.data_ptr(), None, None, 0, N, S, ws.data_ptr(), nbytes, st) != 0
