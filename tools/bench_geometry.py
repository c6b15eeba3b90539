"""What the ray geometry costs on the device: ego_ray_geometry alone, the whole render_geometry, and model.forward on
the same rays in the same run.

    python tools/bench_geometry.py            # -> profiles/r18/geometry.json

Two shapes on the headline scene (synth.SceneConfig(), bench.py's): 4096 rays x 512 samples without resampling, and 8192 rays x
(128 + 128) with it.  Per shape four legs, alternated inside every repetition, `steps` calls between two device synchronisations, the
median, minimum and maximum over the repetitions:
    kernel            ego_ray_geometry (normal, acc, z_quantile; grad_out null) on the samples of the shape's own march
    kernel_gradients  the same with grad_out: every sample gathered, the w == 0 ones too
    render_geometry   the marches, the resampling and the kernel
    forward           model.forward(need_alpha=False) on the same rays: the whole colour render
and the same four on a second model with early_termination_eps = 1e-3, where the march writes exact zeros behind the surface and the
kernel skips them.  `zero_weight_share` is the share of the shape's samples with w == 0 exactly - those the kernel did not gather.
Nothing here has a pass bar.  Without a device the tool fails; it has no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
SHAPES = {"4096x512": (4096, dict(n_coarse=512)), "8192x(128+128)": (8192, dict(n_coarse=128, n_fine=128, resampling=True))}


def summary(v) -> dict:
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), n=len(v))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20, help="calls per leg and repetition")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r18", "geometry.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("tools/bench_geometry.py needs a HIP device: a time from anything else says nothing", file=sys.stderr)
        return 1
    from egonerf_amd import geometry, synth
    dev = torch.device("cuda", 0)
    cfg = synth.SceneConfig()
    weights = synth.make_weights(cfg, seed=1234)
    models = {"plain": synth.build_model(cfg, weights, dev), "early_termination_1e-3": synth.build_model(cfg, weights, dev)}
    models["early_termination_1e-3"].early_termination_eps = 1e-3
    doc = dict(tool="tools/bench_geometry.py", device=torch.cuda.get_device_name(0), scene="synth.SceneConfig(), seed 1234", grid=list(cfg.grid),
               steps_per_leg=a.steps, reps=a.reps, shapes={})
    for shape, (N, kw) in SHAPES.items():
        rays = torch.from_numpy(synth.make_rays(N, seed=1)).to(dev)
        rec = doc["shapes"][shape] = {}
        for tag, model in models.items():
            with torch.no_grad():
                z, w, crd = geometry.march_samples(model, rays, **kw)
                legs = {
                    "kernel": lambda: geometry.ray_geometry(model, rays, z, crd, w, True, 0.5),
                    "kernel_gradients": lambda: geometry.ray_geometry(model, rays, z, crd, w, True, 0.5, gradients=True),
                    "render_geometry": lambda: geometry.render_geometry(model, rays, **kw),
                    "forward": lambda: model(rays, exp_sampling=True, need_alpha=False, **kw),
                }
                for leg in legs.values():   # every shape the timed window uses, twice
                    leg(); leg()
                torch.cuda.synchronize()
                times = {k: [] for k in legs}
                for _ in range(a.reps):
                    for name, leg in legs.items():
                        t0 = time.perf_counter()
                        for _ in range(a.steps):
                            leg()
                        torch.cuda.synchronize()
                        times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
                g = geometry.ray_geometry(model, rays, z, crd, w, True, 0.5)
                ms = {k: summary(v) for k, v in times.items()}
                rec[tag] = dict(ms_per_call=ms, zero_weight_share=float((w == 0).float().mean()),
                                kernel_over_forward=ms["kernel"]["median"] / ms["forward"]["median"],
                                render_geometry_over_forward=ms["render_geometry"]["median"] / ms["forward"]["median"],
                                mean_acc=float(g.acc.mean()), rays_with_a_median=float((g.acc >= 0.5).float().mean()))
    print(json.dumps(doc, indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
