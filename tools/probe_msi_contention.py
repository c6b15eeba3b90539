"""How far the order of arrival of the float atomic adds moves ego_msi_render_backward's sums from run to run.

    python tools/probe_msi_contention.py            # -> profiles/r13/msi_contention.json

The inputs are those of tests/test_hip_msi_refine.py (4099 rays on 2 x 4 texels and on one texel; the 600-ray gradient case with a
background), the measure is the test's: per tensor, max |kernel - float64 autograd| over the test's tolerance max(4 max |float32
autograd - float64|, 1e-6 max |float64|).  `--runs` repetitions of the same call on the same input; recorded: the median and the
maximum of that ratio, and how many distinct results there were."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r13", "msi_contention.json"))
    a = ap.parse_args()
    import torch
    import tests.test_hip_msi_refine as t
    from tests import msi_grad_ref

    def ratios(got, refs):
        out = []
        for mine, want, f32 in zip(got, refs[torch.float64], refs[torch.float32]):
            tol = max(4 * float(np.abs(f32 - want).max()), 1e-6 * float(np.abs(want).max()))
            out.append(float(np.abs(mine - want).max()) / tol)
        return out

    def probe(radii, rays, layers, background, g_rgb, refs):
        rs = np.asarray([ratios(t.kernel_gradients(t.image(radii, layers, background), rays, g_rgb, "call"), refs) for _ in range(a.runs)])
        out = {name: dict(median=float(np.median(rs[:, i])), max=float(rs[:, i].max())) for i, name in enumerate(("layers", "background"))}
        out["distinct_results"] = len(set(map(tuple, rs)))
        return out

    cases = {}
    for shape in ((2, 4), (1, 1)):   # test_no_add_is_lost_under_contention's inputs
        g = np.random.default_rng(31)
        radii, n = t.RADII[:2], 4099
        rays = t.ball_rays(g, n, 0.6 * radii[0])
        layers = g.uniform(0, 1, (2, *shape, 4)).astype(np.float32)
        background = g.uniform(0, 1, (*shape, 4)).astype(np.float32)
        g_rgb = g.standard_normal((n, 3)).astype(np.float32)
        refs = {dt: msi_grad_ref.texel_gradients(rays, t.CENTER, radii, layers, background, g_rgb, dt) for dt in (torch.float64, torch.float32)}
        cases[f"contention {shape[0]} x {shape[1]}"] = probe(radii, rays, layers, background, g_rgb, refs)
    for saturate in (False, True):
        rays, layers, background, g_rgb, refs = t.gradient_case(saturate)
        cases[f"gradient case, saturate={saturate}"] = probe(t.RADII, rays, layers, background, g_rgb, refs[True])
    doc = dict(tool="tools/probe_msi_contention.py", runs=a.runs, error_over_tolerance=cases)
    print(json.dumps(doc, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
