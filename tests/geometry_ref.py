"""The restatement of the ray geometry (csrc/ego_geometry.hip): the float64 oracle's autograd of the density feature with
respect to the sample positions, then the definitions of include/egonerf_hip.h (ego_ray_geometry) literally.  The mechanism is
ray_grad_ref.sample_grad_reference's with dfeat = 1, dfe = 0.

`python -m tests.geometry_ref` measures the two bounds below on the CPU (the float32 restatement against the float64 one)."""
import numpy as np
import torch

from tests import ray_grad_ref as rg
from tests.helpers import make_oracle

# The cases of tests/test_hip_geometry.py: scenes, rays and sampling of ray_grad_ref.CASES, jitter and u ignored (eval mode)
CASES = ("tiny", "tiny_resampled", "tiny_other_seeds", "grid30", "grid24", "n1_s5", "n7_s33", "n7_s5_resampled", "fine_only", "other_n_comp",
         "odd_grid")

# Kernel against restatement, per ray in the max norm (normal, acc: absolute; gradients: relative to max |g64| of the case): 4 x the worst
# distance of the FLOAT32 restatement from the float64 one on the same inputs (the float64 oracle's z, weights and charts, rounded to
# float32 as the kernel receives them) over CASES, the rule of tests/test_hip_msi.py.  Measured on the CPU (python -m tests.geometry_ref):
#   normal, un-normalised 3.87e-6 (grid24), normalised 5.56e-6 (grid24), acc 1.38e-7 (tiny_other_seeds), gradients 8.98e-7 (fine_only,
#   relative); 11 to 24 % of the samples have g = 0 exactly (n1_s5: none); the float32 z_quantile equals the float64 one on every ray.
B_KERNEL = 4 * 5.56e-6
# End to end (render_geometry against the float64 oracle's own forward(keep=True) weights and distances): 4 x the float32 oracle's own
# whole-path distance - its own forward's weights, distances and charts, then the float32 restatement - measured the same way:
#   normal, un-normalised 3.20e-5 (fine_only; 2.7e-5 other_n_comp, <= 9.2e-6 elsewhere), normalised 1.06e-4 (fine_only), acc 2.82e-5
B_END_TO_END = 4 * 1.06e-4
MOST_EXCUSED_PER_64 = 1   # the float32 restatement alone needed none on these inputs
QUANTILE_MARGIN = 1e-5    # rays whose float64 running sum comes this close to the quantile at any sample are left out of the exact check
MOST_LEFT_OUT = 0.02      # ... at most this share of a case's rays (on these inputs none: the smallest margin measured is 1.04e-4)


def geometry_reference(oracle, rays, z, weight, yang, normalize, quantile):
    """(normal [N,3], acc [N], z_quantile [N], g [N,S,3], cum [N,S]) in the oracle's dtype from rays [N,6], z, weight [N,S] and the chart
    flags yang [N,S] (bool): positions o + d z, from_cartesian with the chart forced, normalize_coord on the full grid, the density
    feature's autograd, then n_s = -g_s / |g_s| (0 where |g_s| is 0 or not finite), normal = sum_s w_s n_s (divided by its length with
    `normalize`, 0 stays 0), acc = sum_s w_s, z_quantile = z of the first sample whose running sum reaches `quantile` (0 if none does)."""
    dt = oracle.dtype
    rays, z, w = rays.to(dt), z.to(dt), weight.to(dt)
    N, S = z.shape
    x = (rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3).clone().requires_grad_(True)
    c7n = oracle.normalize_coord(oracle.from_cartesian(x, yang.reshape(-1).long()), downsample=None)
    oracle.density_feature(c7n).sum().backward()
    g = x.grad.detach().view(N, S, 3)
    length = g.norm(dim=-1, keepdim=True)
    ok = torch.isfinite(length) & (length > 0) & torch.isfinite(g).all(-1, keepdim=True)
    n = torch.where(ok, -g / torch.where(ok, length, torch.ones_like(length)), torch.zeros_like(g))
    normal = (w[..., None] * n).sum(1)
    if normalize:
        L = normal.norm(dim=-1, keepdim=True)
        normal = torch.where(L > 0, normal / torch.where(L > 0, L, torch.ones_like(L)), torch.zeros_like(normal))
    acc = w.sum(-1)
    cum = w.cumsum(-1)
    zq = quantile_depth(z, cum, quantile)
    return normal, acc, zq, torch.where(torch.isfinite(g).all(-1, keepdim=True), g, torch.zeros_like(g)), cum


def quantile_depth(z, cum, quantile):
    """z [N,S] at the first sample whose running sum cum [N,S] reaches `quantile`; 0 where none does."""
    reached = cum >= quantile
    first = torch.argmax(reached.to(torch.int8), dim=-1)
    return torch.where(reached.any(-1), z.gather(-1, first[:, None])[:, 0], torch.zeros_like(z[:, 0]))


def oracle_samples(oracle, rays, fwd):
    """The oracle's own eval forward on `rays` -> (z [N,S], weight [N,S], yang [N,S] bool) of the rendered samples, in its dtype."""
    with torch.no_grad():
        _, inter = oracle.forward(rays, keep=True, **fwd)
        z, w = inter["z"], inter["weight"]
        r = rays.to(oracle.dtype)
        xyz = r[:, None, :3] + r[:, None, 3:6] * z[..., None]
        yang = oracle.from_cartesian(xyz)[..., 6] != 0
    return z, w, yang


def _per_ray(a, b):
    return (a.double() - b.double()).abs().reshape(a.shape[0], -1).amax(1)


def measure_bounds():
    worst_k, worst_e = {}, {}
    for name in CASES:
        cfg, w, rays, fwd, *_ = rg.case_inputs(name)
        o64, o32 = make_oracle(cfg, w, dtype=torch.float64), make_oracle(cfg, w, dtype=torch.float32)
        z, wt, yang = oracle_samples(o64, rays, fwd)
        z32, wt32, yang32 = oracle_samples(o32, rays, fwd)
        margin = float((wt.cumsum(-1) - 0.5).abs().min())
        for normalize in (False, True):
            n64, a64, q64, g64, _ = geometry_reference(o64, rays, z, wt, yang, normalize, 0.5)
            # the kernel's bound: the float32 restatement on the float64 path's inputs (rounded to float32, as the kernel receives them)
            n32, a32, q32, g32, _ = geometry_reference(o32, rays, z.float(), wt.float(), yang, normalize, 0.5)
            # the end-to-end bound: the float32 oracle's own path
            e32, ea32, _, _, _ = geometry_reference(o32, rays, z32, wt32, yang32, normalize, 0.5)
            key = "normalised" if normalize else "normal"
            worst_k.setdefault(key, []).append((float(_per_ray(n32, n64).max()), name))
            worst_e.setdefault(key, []).append((float(_per_ray(e32, n64).max()), name))
        gs = max(float(g64.abs().max()), 1e-30)
        worst_k.setdefault("acc", []).append((float(_per_ray(a32, a64).max()), name))
        worst_k.setdefault("grad", []).append((float(_per_ray(g32.reshape(-1, 3), g64.reshape(-1, 3)).max()) / gs, name))
        worst_e.setdefault("acc", []).append((float(_per_ray(ea32, a64).max()), name))
        zero = float((g64 == 0).all(-1).double().mean())
        print(f"{name:18s} N {rays.shape[0]:4d} S {z.shape[1]:3d}  g == 0: {zero:.2f}  smallest |cum - 0.5| {margin:.2e}  z_q equal: "
              f"{bool((q32.double() == q64.float().double()).all())}")
    for title, d in (("kernel (float32 restatement on float64 inputs)", worst_k), ("end to end (float32 oracle's own path)", worst_e)):
        print(title)
        for what, vals in d.items():
            print(f"  {what:11s} worst {max(vals)[0]:.2e} ({max(vals)[1]})   " + " ".join(f"{v:.1e}" for v, _ in vals))


if __name__ == "__main__":
    measure_bounds()
